"""Four instruments for the products (stan_amd/csrc/spmv_kernels.inc) and the CG loop (cg_vector_kernels.inc,
cg_reduce_device.inc), and the yardsticks the device is held to.  Everything is observed through Matrix.spmv / to_csr /
diagonal / scaled_residual and cg_solve / cg_solve_multi with max_its = k; nothing here asks the library for more.

1. PROBING VECTORS.  colours() colours the columns of the full pattern so that no row holds two columns of one colour.  The
   probe of colour c is x = sum_j w_j e_j over its columns with w_j = +-2^e, e in [-8, 8], sign and e seeded per column: in
   the product of a row every a_ij w_j is exact and every other term an exact zero, so y_i / w_j IS the stored a_ij, bit for
   bit, whatever the order of the sums and whether or not multiply-adds are fused; a row without a column of that colour
   gives y_i == 0.  One sweep over the colours (Probes.sweep) rebuilds the whole matrix from products.  The weights differ
   from column to column on purpose: with a vector of ones a lane that gathered x from a WRONG column of the same colour
   would go unseen.

2. A LONG-DOUBLE CG.  cg_reference restates stan_oracle_cg_opt (oracle/stan_oracle.c; alglib's lincg as the reference runs
   it: s_i = 1/sqrt(A_ii), x_0 = 0, the recurrences, the literal refresh r = b^ - A^ x on every rupdate-th iteration) in
   np.longdouble on an exported CSR and returns every iterate U_k = S x_k with sqrt(r_k . r_k) / ||b^||.  "The same
   iterates" then reads in units of 2^-53 instead of 1e-9.

3. THE SHARDED RESTATEMENT.  rank_of_rows / halo_entries / slice_census read the host's partition plan onto the exported CSR,
   rank_dot is the sum of a solve on several ranks (per-rank partials added in rank order), and cg_iterates /
   cg_single_reduce_f64 take it for every sum of the loop (dot=): the float64 loop as a sharded solve orders it, which
   tests/test_product_ref.py holds inside the one-rank bounds -- and the mutants of a halo exchange outside them.

4. FROM THE DEVICE'S OWN ITERATE.  What happens late in a loop -- the restart every n_red iterations, the refinement pass behind
   a converged first one -- is out of a replay's reach (a converged recurrence, or float64 and long double orders apart by
   then).  one_step and refinement_pass take the iterate the device returned at max_its = k as exact data and predict in long
   double what it must add next; the float64 restatement of the same construction is the yardstick, one rounding of the
   iterate the floor (step_units, step_floor).  refine_driver_f64 restates the passes of stan_cg_device in float64: how many
   there are and how far every stop decision is from its threshold.

Row sums (row_units) are counted in units of 2^-53 sum_j |a_ij| |x_j|, the rounding scale of the row itself: a wrong entry
in a row far below max|y| cannot hide there.  A row of m stored entries summed in ANY order, with or without fused
multiply-adds, errs by at most m units (m - 1 additions and m products, each product sharing its rounding with an addition
when fused; first order): derived_row_units() = m + 2 leaves room for the second-order terms and the reference's own 2^-64.

The reduced-precision value streams (STAN_PREC_FIXED48, STAN_PREC_MIXED) get the same long-double CG on the matrix quantised
as the stream quantises it (QUANTISE), and a float64 loop on the matrix quantised from float64 entries as their yardstick.

The *_MEASURED constants are the oracle's errors against these references, measured on the development host (x86-64, gcc
-O2 without FMA contraction); tests/test_product_ref.py measures each again on every run and holds it within a factor of two
both ways.  The device is held to four times the oracle's figure (another summation order, fused multiply-adds: a small
factor, not an order of magnitude), or to the derived figure where that is smaller; nothing is fitted to the device."""
import numpy as np

from stan_amd import problem

assert np.finfo(np.longdouble).eps < 2e-19, "tests/product_ref.py needs an 80-bit (or wider) np.longdouble: run on x86-64 Linux"

LD = np.longdouble
U53 = 2.0 ** -53
KMAX = 22                       # iterates compared: refreshes at 10 and 20
CG_MODELS = ("cube6", "perforated12")
SPMV_MODELS = ("cube1", "cube2", "cube6", "cube20", "perforated12", "star12")
VECTORS = ("normal", "spread", "rigid_x")

# Worst row error of oracle.smv_upper over SPMV_MODELS x VECTORS in units of the row's scale.  It falls on cube20 under the
# spread vector (the oracle scatters the transposed terms into y one by one); per vector the worst model reads 2.53 (normal) /
# 8.89 (spread) / 2.08 (rigid_x), a plain float64 numpy row sum 3.39 / 5.71 / 2.10.
ORACLE_SPMV_UNITS_MEASURED = 8.89
DEVICE_SPMV_UNITS = 4 * ORACLE_SPMV_UNITS_MEASURED
# Worst error of oracle.cg(A, F, 1e-30, maxits=k, merit_stop=False) over k = 1 .. KMAX against cg_reference, in units of 2^-53:
# max|U - U_k| / max|U_k|, and |rel_residual / ref - 1|; per model, for each of the three load vectors of load_cases() (the
# first is the job's own, which every single-load form solves).
ORACLE_CG_U_UNITS_MEASURED = {"cube6": (21.1, 13.6, 37.7), "perforated12": (108.0, 32.4, 88.4)}
ORACLE_CG_RES_UNITS_MEASURED = {"cube6": (35.5, 54.2, 75.2), "perforated12": (86.5, 73.8, 61.3)}
# The same of cg_single_reduce_f64 (the Chronopoulos-Gear recurrences of cg_vector_kernels.inc in plain float64 numpy) on the
# job's own load vector: the yardstick of STAN_OPT_CG_SINGLE_REDUCE, whose alpha comes from a three-term formula and rounds
# differently.  (cg_iterates in float64, the classic loop in the same numpy arithmetic: U 34.3 / 85.8, residual 65.9 / 128.1.)
SR_CG_U_UNITS_MEASURED = {"cube6": 54.7, "perforated12": 220.0}
SR_CG_RES_UNITS_MEASURED = {"cube6": 95.1, "perforated12": 324.8}
DEVICE_CG_FACTOR = 4
# Reduced-precision value streams (STAN_PREC_FIXED48, STAN_PREC_MIXED with STAN_OPT_CG_REFINE 0; k = 1 .. KMAX_REDUCED).  The
# reference is cg_reference on the matrix quantised from the LONG-DOUBLE scaled entries; the yardstick is the float64 loop
# (cg_iterates) on the matrix quantised from the FLOAT64 scaled entries, formed as matrix_streams.hip forms them -- which
# includes the entries that fall on the other side of a quantisation boundary (FIXED-48: 20 of 51 984 and 14 of 328 716 entries
# move by one quantum of 2^-46; float32: none on these models).  (U units, recurrence-residual units) per (stream, model).
KMAX_REDUCED = 12
REDUCED_CG_UNITS_MEASURED = {("fixed48", "cube6"): (127.8, 65.4), ("fixed48", "perforated12"): (71.0, 39.0),
                             ("mixed", "cube6"): (8.2, 6.3), ("mixed", "perforated12"): (6.1, 1.8)}
# The same pair for STAN_OPT_CG_SINGLE_REDUCE on a reduced stream: cg_single_reduce_f64(quantise=) against the same reference.
REDUCED_SR_CG_UNITS_MEASURED = {("fixed48", "cube6"): (106.9, 66.4), ("fixed48", "perforated12"): (70.5, 10.2),
                                ("mixed", "cube6"): (18.5, 32.7), ("mixed", "perforated12"): (32.5, 4.2)}
# STAN_OPT_CG_REFINE 2 on the float32 stream, k = 48 .. 52: the float64 loop that refreshes on the fp64 values at iteration 50
# (and never before) against the same loop in long double.  (U units, recurrence-residual units) per model.
REFINE2_KS = (48, 49, 50, 51, 52)
REFINE2_UNITS_MEASURED = {"cube6": (4590.0, 9.66e4), "perforated12": (7.9e4, 50.4)}
# The second refinement pass of a float32 solve to REFINE_EPS, iterates 1 .. 12 behind the first pass's U_1 (refinement_pass in
# float64 through added_f64, against long double), worst over k in units of 2^-53 max|S d_k|; and the iterations of the first
# pass of the float64 stand-in.
REFINE_EPS = 1e-10
REFINE_KMAX = 12
SECOND_PASS_UNITS_MEASURED = {"cube6": 2.16e8, "perforated12": 9.85e7}
FIRST_PASS_ITS_MEASURED = {"cube6": 112, "perforated12": 322}
# FIXED-48: the eps_f at which the float64 restatement of the driver (refine_driver_f64) takes exactly two passes on both
# models with every stop decision a factor 1.01 from its threshold; (iterations of pass 1, of pass 2) on the oracle's matrix.
REFINE_EPS_FIXED48 = 1e-12
FIXED48_PASSES_MEASURED = {"cube6": (124, 2), "perforated12": (356, 60)}
# The step behind the restart (one_step), float64 against long double through added_f64: (model, k) -> (yardstick, floor) in
# units of 2^-53 max|d_ref|, STAN_OPT_CG_RUPDATE 6, the job's own load vector, the fp64 values.
RESTART_RUPDATE = 6
RESTART_CASES = (("cube1s", 1), ("cube2s", 1), ("cube2s", 2))        # (model, k / n_red)
RESTART_STEP_UNITS_MEASURED = {("cube1s", 1): (1.89e5, 5.93e5), ("cube2s", 1): (1.94e5, 8.38e4), ("cube2s", 2): (1.58e7, 1.25e7)}

# Roundings between a stored a_ij and the entry rebuilt from a product of the SCALED matrix, K x = S^-1 (A^ (S^-1 x))
# (stan_spmv_reduced, cg_entries.inc), counted from the code: s_i s_j (1) and a_ij times it (2) in k_scale_matrix /
# k_spmv_first; x_j / s_j in k_expand (3); a^_ij x^_j in the product (4; the row's other terms are exact zeros); y_i / s_i in
# k_compress_div (5).  s itself (a square root and a division) enters twice as a factor and twice as a divisor, the same
# stored number each time: its own error cancels.
SCALED_PATH_ROUNDINGS = 5


# ---- models -----------------------------------------------------------------------------------------------------------------

def star_job(k, layers=3, rings=2):
    """star_mesh clamped at z = 0, loaded on its top layer (as the parity tests' _star_job)."""
    from stan_amd.cube import star_mesh
    xyz, conn = star_mesh(k, layers, rings)
    z0 = np.nonzero(xyz[:, 2] == 0)[0]
    top = np.nonzero(xyz[:, 2] == xyz[:, 2].max())[0]
    return problem.make_job(xyz, conn, z0, np.ones((len(z0), 3)), top, np.tile([0.0, 10.0, 5.0], (len(top), 1)))


def stretched_cube_job(n):
    """problem.cube_job(n, jitter=0.1) with the coordinates stretched by (30, 1, 1/30): elements of aspect 900, a matrix on
    which the loop is nowhere near converged after n_red iterations (12 for n = 1, 54 for n = 2) -- the models of the restart."""
    j = problem.cube_job(n, jitter=0.1)
    j.xyz = np.ascontiguousarray(j.xyz * np.array([30.0, 1.0, 1.0 / 30.0]))
    return j


# name -> (builder, cube size n or None).  The smallest models that reach each branch of the products: one slice of fewer than
# 64 rows / a pair-kernel workgroup without a second slice (cube1, cube2); 17 slices with a ragged last one (cube6); packed
# column modes 1 and 2 (cube20); mixed row lengths and odd slot counts (perforated12); rows of 75 blocks (star12); 1 077
# slices, one full 256-workgroup window of the XCD-chunked mapping plus its ragged tail (cube40); 12 and 54 equations on
# which the restart of the loop every n_red iterations acts on an unconverged recurrence (cube1s, cube2s).
_BUILDERS = {
    "cube1": (lambda: problem.cube_job(1), 1),
    "cube2": (lambda: problem.cube_job(2), 2),
    "cube6": (lambda: problem.cube_job(6, jitter=0.1), 6),
    "cube20": (lambda: problem.cube_job(20, jitter=0.05), 20),
    "perforated12": (lambda: problem.perforated_job(12, 0.4), None),
    "star12": (lambda: star_job(12, rings=1), None),
    "cube40": (lambda: problem.cube_job(40), 40),
    "cube1s": (lambda: stretched_cube_job(1), 1),
    "cube2s": (lambda: stretched_cube_job(2), 2),
}
_jobs = {}


def job(name):
    if name not in _jobs:
        _jobs[name] = _BUILDERS[name][0]()
    return _jobs[name]


def row_dofs(j):
    """(node, component) of every row of the reduced system of job j."""
    free = np.nonzero(np.asarray(j.red) != -1)[0]
    assert free.shape[0] == j.n_red
    inv = np.empty(j.n_dof, dtype=np.int64)
    inv[np.asarray(j.node_dof).reshape(-1)] = np.arange(j.n_dof)
    return inv[free] // 3, inv[free] % 3


def cube_grid(name):
    """[N, 4]: grid index (i, j, k) of the node and the component of every reduced row of a cube model; None for the others."""
    n = _BUILDERS[name][1]
    if n is None:
        return None
    node, comp = row_dofs(job(name))
    m = n + 1
    return np.stack([node % m, (node // m) % m, node // (m * m), comp], axis=1)


def full_csr(A):
    """(rowptr, col, val) of the full symmetric matrix from the oracle's upper CRS, columns ascending: no arithmetic, and
    stored zeros stay in the pattern (scipy's sum of the two triangles would drop them)."""
    r, c = rows_of(A.ridx), A.idx.astype(np.int64)
    off = c != r
    rows, cols, vals = np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([A.vals, A.vals[off]])
    order = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.n))]).astype(np.int64)
    return rowptr, cols[order].astype(np.int32), vals[order]


def rows_of(rowptr):
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr))


def csr_diagonal(rowptr, col, val):
    rows = rows_of(rowptr)
    d = np.zeros(rowptr.shape[0] - 1, dtype=val.dtype)
    on = col == rows
    d[rows[on]] = val[on]
    return d


# ---- probing ------------------------------------------------------------------------------------------------------------------

def colours(rowptr, col, grid=None):
    """colour [N] of the columns of the pattern, no row holding two columns of one colour.  grid (cube_grid) given: the closed
    form, node grid index mod 3 per axis times the component: 81 colours (a row couples nodes at most one apart per axis).
    Otherwise greedy in column order: a column takes the smallest colour no column sharing a row with it has.  The result is
    checked here, in one pass: rows * n_colours + colour[col] has no repeats."""
    n = rowptr.shape[0] - 1
    rows = rows_of(rowptr)
    if grid is not None:
        g = np.asarray(grid, dtype=np.int64)
        colour = ((g[:, 0] % 3) + 3 * (g[:, 1] % 3) + 9 * (g[:, 2] % 3)) * 3 + g[:, 3]
    else:
        import scipy.sparse as sp
        P = sp.csr_matrix((np.ones(col.shape[0], dtype=np.int32), col, rowptr), shape=(n, n))
        G = (P.T @ P).tocsr()                             # columns that share a row
        colour = np.full(n, -1, dtype=np.int64)
        for j in range(n):
            c = colour[G.indices[G.indptr[j]:G.indptr[j + 1]]]
            taken = np.zeros(int(c.max(initial=-1)) + 3, dtype=bool)   # (one entry past the largest colour seen stays free)
            taken[c[c >= 0]] = True
            colour[j] = np.argmin(taken)
    nc = int(colour.max()) + 1 if n else 0
    key = rows * nc + colour[col]
    assert colour.min(initial=0) >= 0 and np.unique(key).shape[0] == key.shape[0], "two columns of one colour in a row"
    return colour


def weights(n, seed=2024, ones=False):
    """w_j = +-2^e, e in [-8, 8], per column from a fixed seed (ones: the vector that cannot see a swapped gather)."""
    if ones:
        return np.ones(n)
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-8, 9, n)


class Probes:
    """The probes of a pattern and the sweep that rebuilds a matrix from products."""

    def __init__(self, rowptr, col, colour, w):
        self.n = rowptr.shape[0] - 1
        self.colour, self.w = colour, w
        self.n_colours = int(colour.max()) + 1 if self.n else 0
        rows, ec = rows_of(rowptr), colour[col]
        self.order = np.argsort(ec, kind="stable")        # the entries colour by colour
        self.seg = np.concatenate([[0], np.cumsum(np.bincount(ec, minlength=self.n_colours))])
        self.rows, self.cols = rows[self.order], col[self.order]

    def probe(self, c):
        return np.where(self.colour == c, self.w, 0.0)

    def sweep(self, product):
        """(val in the order of the CSR, stray): val[q] = y_i / w_j of the probe of column j's colour; stray = the number of
        non-zero y_i in rows without a column of the probe's colour (anything outside the pattern)."""
        val = np.empty(self.order.shape[0])
        stray = 0
        for c in range(self.n_colours):
            y = np.asarray(product(self.probe(c)), dtype=np.float64)
            a, b = self.seg[c], self.seg[c + 1]
            hit = self.rows[a:b]                              # unique: that is the colouring's property
            val[self.order[a:b]] = y[hit] / self.w[self.cols[a:b]]
            stray += int(np.count_nonzero(y)) - int(np.count_nonzero(y[hit]))
        return val, stray


def same_bits(got, want):
    """Entry by entry: the same int64 views, or == where the stored value is a zero (-0.0 == 0.0)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return (got.view(np.int64) == want.view(np.int64)) | ((want == 0) & (got == 0))


# ---- row sums -------------------------------------------------------------------------------------------------------------------

def vectors(name):
    """name -> x [N] for model `name`, seeded: standard normal; normal times 2^e, e uniform in [-30, 30] per entry (row scales
    spread over many orders); the rigid translation, one in the x DOF of every node with a free x DOF (interior rows cancel)."""
    j = job(name)
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    x0 = rng.standard_normal(j.n_red)
    x1 = rng.standard_normal(j.n_red) * 2.0 ** rng.integers(-30, 31, j.n_red)
    x2 = (row_dofs(j)[1] == 0).astype(np.float64)
    assert x2.any()
    return dict(zip(VECTORS, (x0, x1, x2)))


def row_reference(rowptr, col, val, x):
    """(y_ref, scale) in longdouble: sum_j a_ij x_j and sum_j |a_ij| |x_j|, every row with at least one entry."""
    assert (np.diff(rowptr) > 0).all()
    t = val.astype(LD) * np.asarray(x, dtype=np.float64).astype(LD)[col]
    return np.add.reduceat(t, rowptr[:-1]), np.add.reduceat(abs(t), rowptr[:-1])


def row_units(y, y_ref, scale):
    """|y_i - ref_i| in units of 2^-53 scale_i per row (a row of scale 0 must be met exactly: 0 units, else inf)."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == y_ref.shape and np.isfinite(y).all()
    d = abs(y.astype(LD) - y_ref)
    u = np.where(scale > 0, d / np.where(scale > 0, U53 * scale, 1), np.where(d > 0, np.inf, 0.0))
    return u.astype(np.float64)


def derived_row_units(rowptr, extra=0):
    """m_i + 2 per row (+ the roundings of the scaled path): holds for any summation order, with or without FMAs."""
    return np.diff(rowptr).astype(np.float64) + 2 + extra


def row_bound(rowptr, extra=0):
    """The bound of every row: the smaller of 4 x the oracle's measured figure and the derived one."""
    return np.minimum(DEVICE_SPMV_UNITS, derived_row_units(rowptr, extra))


def scaled_residual_reference(rowptr, col, val, F, U, row_bound_units):
    """(ref, bar): ||S (F - K U)|| / ||S F|| in longdouble and the relative bar Matrix.scaled_residual is held to, formed as
      e_i = 2^-53 s_i (B_i sum_j |a_ij| |U_j| + 4 |F_i - y_i|)    B_i the row's bound in units; 4 = the subtraction, the two
                                                                    roundings of s_i (sqrt, division), the product with s_i
      bar = ||e|| / ||r|| + (N + 6) 2^-53                          (N + 3): two norms of N squares summed in any order
                                                                    (N/2 + 1 each after the root) and their division; 3: the
                                                                    entries s_i F_i of the denominator."""
    d = csr_diagonal(rowptr, col, val).astype(LD)
    s = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), 1)
    y, scale = row_reference(rowptr, col, val, U)
    Fl = np.asarray(F, dtype=np.float64).astype(LD)
    r = s * (Fl - y)
    e = U53 * s * (row_bound_units * scale + 4 * abs(Fl - y))
    nr, nb = np.sqrt((r * r).sum()), np.sqrt(((s * Fl) ** 2).sum())
    return float(nr / nb), float(np.sqrt((e * e).sum()) / nr + (r.shape[0] + 6) * U53)


# ---- CG -------------------------------------------------------------------------------------------------------------------------

class Scaled:
    """A^ = S A S, b^ = S b of an exported CSR in the number type T (np.longdouble: the reference; np.float64: the restatements
    and mutants).  quantise: applied to the scaled entries (the reduced-precision streams)."""

    def __init__(self, rowptr, col, val, T=LD, quantise=None):
        self.T, self.rowptr, self.col = T, rowptr, col
        d = csr_diagonal(rowptr, col, val).astype(T)
        self.s = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), np.ones(1, dtype=T)).astype(T)
        self.a = val.astype(T) * (self.s[rows_of(rowptr)] * self.s[col])          # a_ij (s_i s_j), as k_scale_matrix
        if quantise is not None:
            self.a = quantise(self.a).astype(T)
        assert (np.diff(rowptr) > 0).all()

    def mv(self, x):
        return np.add.reduceat(self.a * x[self.col], self.rowptr[:-1])

    def rhs(self, F):
        return np.asarray(F, dtype=np.float64).astype(self.T) * self.s


def quantise_fixed48(a):
    """rint(a^ 2^46) 2^-46 of the scaled entries (spmv_kernels.inc: the FIXED-48 stream; k_to_fx48 rounds to nearest even)."""
    return np.rint(a * 2.0 ** 46) * 2.0 ** -46


def quantise_mixed(a):
    """float32 of the scaled entries (k_to_fp32), one rounding from whatever type they come in."""
    return a.astype(np.float32)


QUANTISE = {"fixed48": quantise_fixed48, "mixed": quantise_mixed}


def _dot(a, b):
    return (a * b).sum()


def cg_iterates(A, F, kmax, rupdate=10, pap=None, late_beta=False, mv=None, dot=_dot, refresh_with=None, restart=0, b=None, stop=None):
    """The classic loop of stan_oracle_cg_opt (merit stop off) on the Scaled matrix A in A's number type:
    [(U_k, sqrt(r_k . r_k) / ||b^||) for k = 1 .. kmax].  dot(a, b): every sum of the loop (rho, r . r, ||b^||^2, p . A p) --
    rank_dot() for the order of a sharded solve; pap(p, v): the sum p . A p alone (default: dot); late_beta: beta from the rho
    of one iteration earlier; mv: another product -- the hooks of the mutants.  refresh_with(x): the product of the refresh
    iterations alone (STAN_OPT_CG_REFINE 2: the fp64 values behind a loop on a reduced stream); restart: beta = 0 behind
    every restart-th iteration (lincg's ItsBeforeRestart = n_red; 0: never, which is the loop of every model whose compared
    iterates end before n_red); b: the scaled right-hand side itself instead of S F (a refinement pass iterates on r_t); stop:
    the loop ends behind the first iterate with sqrt(r . r) <= stop ||b^|| (the driver's stand-in)."""
    mv = A.mv if mv is None else mv
    pap = dot if pap is None else pap
    refresh_with = mv if refresh_with is None else refresh_with
    b = A.rhs(F) if b is None else b
    x, r = np.zeros_like(b), b.copy()
    p = r.copy()
    rho = dot(r, r)
    rho_before = rho
    bnorm = np.sqrt(dot(b, b))
    out = []
    for k in range(1, kmax + 1):
        v = mv(p)
        alpha = rho / pap(p, v)
        x = x + alpha * p
        r = b - refresh_with(x) if rupdate and k % rupdate == 0 else r - alpha * v
        r2 = dot(r, r)
        out.append((A.s * x, np.sqrt(r2) / bnorm))
        if stop is not None and out[-1][1] <= stop:
            break
        beta = r2 / (rho_before if late_beta else rho)
        if restart and k % restart == 0:
            beta = beta * 0
        rho_before, rho = rho, r2
        p = r + beta * p
    return out


def cg_reference(csr, F, kmax, rupdate=10, quantise=None):
    """([U_k], [rel_k]) for k = 1 .. kmax in np.longdouble on the exported CSR (rowptr, col, val)."""
    its = cg_iterates(Scaled(*csr, T=LD, quantise=quantise), F, kmax, rupdate)
    return [u for u, _r in its], [r for _u, r in its]


def cg_single_reduce_f64(csr, F, kmax, rupdate=10, dot=_dot, quantise=None, restart=0):
    """The Chronopoulos-Gear recurrences as the comment block of cg_vector_kernels.inc states them, in plain float64 numpy:
      w_k = A r_k, gamma_k = r_k . r_k, delta_k = r_k . w_k
      beta_k = gamma_k / gamma_{k-1}, p_k . A p_k = delta_k - beta_k gamma_k / alpha_{k-1}, alpha_k = gamma_k / p_k . A p_k
      p = r + beta p, s = w + beta s, x' = x + alpha p, r' = r - alpha s      (refresh iterations: r' = b^ - A x')
    Returns [(U_k, sqrt(gamma_k) / ||b^||)] with gamma_k the sum the product behind iteration k forms.  dot(a, b): every sum
    (||b^||^2, gamma, delta), as in cg_iterates; quantise: the reduced-precision stream the products read (Scaled); restart:
    beta = 0 -- p = r, s = w, alpha = gamma / delta -- in the iteration behind every restart-th one, as k_vec_sr has it."""
    A = Scaled(*csr, T=np.float64, quantise=quantise)
    b = A.rhs(F)
    x, r, p, s = np.zeros_like(b), b.copy(), np.zeros_like(b), np.zeros_like(b)
    bnorm = np.sqrt(dot(b, b))
    gamma_prev = alpha_prev = None
    out = []
    for k in range(1, kmax + 2):
        w = A.mv(r)
        gamma, delta = dot(r, r), dot(r, w)
        if k > 1:
            out.append((A.s * x, np.sqrt(gamma) / bnorm))
        if k == 1 or (restart and (k - 1) % restart == 0):
            beta, pap = 0.0, delta
        else:
            beta = gamma / gamma_prev
            pap = delta - beta * gamma / alpha_prev
        alpha = gamma / pap
        p = r + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = b - A.mv(x) if rupdate and k % rupdate == 0 else r - alpha * s
        gamma_prev, alpha_prev = gamma, alpha
    return out


# ---- instruments that start from an iterate the DEVICE returned ------------------------------------------------------------------
# A replay of the whole loop cannot test what happens late in it: by then the recurrence has converged, or float64 and long
# double have drifted apart by orders.  These take the iterate U the device returned at max_its = k as exact data and predict,
# in long double, what the device must add to it next; the float64 restatement of the same construction is the yardstick.
# A difference d of two returned iterates is counted in units of 2^-53 max|d_ref| (step_units) and cannot be resolved below
# the rounding of the iterates themselves: step_floor = max|U| / max|d_ref| units.

def one_step(csr, F, U, quantise=None, T=LD):
    """S (alpha r) with x = U / s, r = b^ - A^ x, alpha = r.r / r.A^ r: the whole step of the iteration behind a restart
    (beta = 0: p = r) that is also a refresh iteration (r = b^ - A^ x).  (step, ||r|| / ||b^||)."""
    A = Scaled(*csr, T=T, quantise=quantise)
    b = A.rhs(F)
    r = b - A.mv(np.asarray(U, dtype=np.float64).astype(T) / A.s)
    rr = _dot(r, r)
    return A.s * (rr / _dot(r, A.mv(r)) * r), np.sqrt(rr / _dot(b, b))


def added_f64(U, step):
    """fl(U + step) - U in float64: what two returned iterates can show of a step (the yardsticks go through it)."""
    U = np.asarray(U, dtype=np.float64)
    return (U + np.asarray(step, dtype=np.float64)) - U


def step_units(d, d_ref):
    """max|d - d_ref| in units of 2^-53 max|d_ref|."""
    d = np.asarray(d, dtype=np.float64)
    assert np.isfinite(d).all() and d.shape == d_ref.shape
    return float(abs(d.astype(LD) - d_ref).max() / abs(d_ref).max() / U53)


def step_floor(U, d_ref):
    """max|U| / max|d_ref|: one rounding of the iterate in the units of step_units."""
    return float(abs(np.asarray(U, dtype=np.float64)).max() / abs(d_ref).max())


def refinement_pass(csr, F, U1, kmax, quantise, T=LD, rhs_quantise=None, loop_quantise="same", rupdate=10):
    """The pass of iterative refinement behind the iterate U1 (stan_cg_device): r_t = b^ - A^64 (U1 / s) with the fp64 values,
    then the loop from x = 0 on the right-hand side r_t with the reduced stream's values: [S d_k for k = 1 .. kmax], and
    ||r_t|| / ||b^||.  The hooks of the mutants: rhs_quantise -- r_t formed with those values instead of the fp64 ones;
    loop_quantise -- the loop's values (None: the fp64 matrix), "same": quantise."""
    A64 = Scaled(*csr, T=T, quantise=rhs_quantise)
    Aq = Scaled(*csr, T=T, quantise=quantise if loop_quantise == "same" else loop_quantise)
    b0 = A64.rhs(F)
    rt = b0 - A64.mv(np.asarray(U1, dtype=np.float64).astype(T) / A64.s)
    its = cg_iterates(Aq, None, kmax, rupdate, b=rt)
    return [u for u, _r in its], np.sqrt(_dot(rt, rt) / _dot(b0, b0))


def first_pass_f64(csr, F, eps, quantise, cap=2000, rupdate=10):
    """The float64 stand-in of the first pass of a reduced-precision solve: the loop on the quantised matrix until
    sqrt(r.r) <= eps ||b^||.  (n1, [rel_k for k = 1 .. n1], U_n1)."""
    A = Scaled(*csr, T=np.float64, quantise=quantise)
    its = cg_iterates(A, F, cap, rupdate, stop=eps)
    assert its[-1][1] <= eps
    return len(its), [float(r) for _u, r in its], its[-1][0]


def refine_driver_f64(csr, F, eps_f, quantise, max_passes=8, cap=5000, rupdate=10):
    """stan_cg_device's passes (STAN_OPT_CG_REFINE 1, no iteration limit) restated in float64: the loop on the quantised matrix
    until sqrt(r.r) <= eps_pass ||b_pass||, the fp64 check rel64 = ||b^ - A^64 x|| / ||b^||, x the sum of the passes' iterates,
    the next pass on r_t with eps_pass = eps_f / rel64; it ends when rel64 <= eps_f, when rel64 has not halved, or after
    max_passes.  One dict per pass: its, the loop's residual at its stop and one iteration earlier over eps_pass (stop, before:
    how far both decisions of the loop are from their threshold), rel64 / eps_f behind it (check), U = S x."""
    A64, Aq = Scaled(*csr, T=np.float64), Scaled(*csr, T=np.float64, quantise=quantise)
    b0 = A64.rhs(F)
    bn0 = np.sqrt(_dot(b0, b0))
    x, b, eps_pass, prev, out = np.zeros_like(b0), b0, eps_f, None, []
    while True:
        its = cg_iterates(Aq, None, cap, rupdate, b=b, stop=eps_pass)
        assert its[-1][1] <= eps_pass
        x = x + its[-1][0] / Aq.s
        rt = b0 - A64.mv(x)
        rel64 = float(np.sqrt(_dot(rt, rt)) / bn0)
        out.append(dict(its=len(its), stop=float(its[-1][1] / eps_pass), before=float(its[-2][1] / eps_pass) if len(its) > 1 else np.inf,
                        check=rel64 / eps_f, U=A64.s * x))
        if rel64 <= eps_f or len(out) >= max_passes or (prev is not None and not rel64 < 0.5 * prev):
            return out
        prev, b, eps_pass = rel64, rt, eps_f / rel64


def two_passes_clear_of_thresholds(passes, factor=1.01):
    """Exactly two passes of refine_driver_f64, every decision `factor` away from its threshold: each loop stops below
    eps_pass / factor having stood above factor eps_pass one iteration earlier; rel64 misses eps_f by the factor behind the
    first pass and meets it by the factor behind the second."""
    return (len(passes) == 2 and all(p["stop"] <= 1 / factor and p["before"] >= factor for p in passes) and
            passes[0]["check"] >= factor and passes[1]["check"] <= 1 / factor)


def rel64_of(csr, F, U, T=LD):
    """||b^ - A^64 (U / s)|| / ||b^||, the residual the fp64 check of a reduced-precision solve reports."""
    A = Scaled(*csr, T=T)
    b = A.rhs(F)
    r = b - A.mv(np.asarray(U, dtype=np.float64).astype(T) / A.s)
    return float(np.sqrt(_dot(r, r) / _dot(b, b)))


# ---- the sharded loop -----------------------------------------------------------------------------------------------------------
# What a solve on several ranks changes in the ARITHMETIC of the loop, restated on the exported CSR: every sum is formed rank
# by rank and the partials are added in rank order (the all-reduce of the stand-in transport and the mailboxes of p2p.hip
# alike); the product itself keeps its rows, whoever owns them.  Which row belongs to whom, which stored entries cross a cut
# (the terms whose x_j arrives through the halo exchange) and which 64-row slices the split product puts on its boundary
# list follow from the host's partition plan alone.

def rank_of_rows(j, nranks):
    """rank [N] of every reduced row of job j on nranks ranks: the host plan's cut of the block rows (host/partition.cpp: whole
    64-row slices, ranks may stay empty), a reduced row belonging to the block row of its node."""
    from stan_amd import host
    rs = host.partition_plan(j.node_index, j.conn, nranks, 0)["row_starts"]
    return np.searchsorted(rs, block_rows(j), side="right") - 1


def block_rows(j):
    """block row [N] (the node's place in the reference's DOF order) of every reduced row."""
    return np.asarray(j.node_index, dtype=np.int64)[row_dofs(j)[0]]


def halo_entries(csr, rank):
    """Boolean mask over the stored entries: row and column lie on different ranks (rank: rank_of_rows)."""
    rowptr, col, _val = csr
    return rank[rows_of(rowptr)] != rank[col]


def slice_census(j, csr, nranks):
    """[(interior, boundary)] per rank: its 64-block-row slices without / with a halo entry in any of their rows -- the two lists
    of the split product (assembly.hip: k_slice_class).  Counted on the reduced pattern: the device classes the block pattern,
    in which a clamped node keeps its columns, so a slice whose only coupling across the cut runs through clamped DOFs would
    be boundary there and interior here."""
    from stan_amd import host
    rs = host.partition_plan(j.node_index, j.conn, nranks, 0)["row_starts"]
    rank, blk = rank_of_rows(j, nranks), block_rows(j)
    touched = np.unique(blk[rows_of(csr[0])[halo_entries(csr, rank)]] // 64)          # (cuts sit on slice boundaries)
    out = []
    for r in range(nranks):
        s0, s1 = int(rs[r]) // 64, -(-int(rs[r + 1]) // 64)
        bnd = int(((touched >= s0) & (touched < s1)).sum()) if rs[r + 1] > rs[r] else 0
        out.append(((s1 - s0 if rs[r + 1] > rs[r] else 0) - bnd, bnd))
    return out


def rank_dot(rank, nranks, ranks=None):
    """dot(a, b) of a sharded solve: each rank sums its rows, the partials are added in rank order 0 .. nranks - 1, a rank
    without rows adds nothing.  ranks: the ranks that take part (a mutant leaves one out)."""
    parts = [np.nonzero(rank == r)[0] for r in (range(nranks) if ranks is None else ranks)]
    parts = [q for q in parts if q.size]

    def dot(a, b):
        total = (a[parts[0]] * b[parts[0]]).sum()
        for q in parts[1:]:
            total = total + (a[q] * b[q]).sum()
        return total
    return dot


def sharded_cg_bounds(name, lc, single_reduction=False):
    """(U, residual) bound in units of 2^-53 of a sharded loop form: the one-rank loop's own, DEVICE_CG_FACTOR x the oracle's
    figure for that load vector, or x the single-reduction yardstick (the job's own load vector only)."""
    if single_reduction:
        assert lc == 0
        return DEVICE_CG_FACTOR * SR_CG_U_UNITS_MEASURED[name], DEVICE_CG_FACTOR * SR_CG_RES_UNITS_MEASURED[name]
    return DEVICE_CG_FACTOR * ORACLE_CG_U_UNITS_MEASURED[name][lc], DEVICE_CG_FACTOR * ORACLE_CG_RES_UNITS_MEASURED[name][lc]


def u_units(U, U_ref):
    """max|U - U_k| / max|U_k| in units of 2^-53."""
    U = np.asarray(U, dtype=np.float64)
    assert np.isfinite(U).all() and U.shape == U_ref.shape
    return float(abs(U.astype(LD) - U_ref).max() / abs(U_ref).max() / U53)


def res_units(rel, rel_ref):
    """|rel_residual / ref - 1| in units of 2^-53."""
    assert np.isfinite(rel)
    return float(abs(LD(rel) / rel_ref - 1) / U53)


def load_cases(name):
    """[3, N]: the job's own load vector and two seeded ones of its size, all different (cg_solve_multi)."""
    j = job(name)
    rng = np.random.default_rng(77)
    return np.stack([j.F, rng.standard_normal(j.n_red) * np.abs(j.F).max(), np.where(np.arange(j.n_red) % 3 == 1, 25.0, -5.0)])


_refs = {}


def cached(key, make):
    """References are computed once per process and shared, unchanged, among the tests that need them."""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]
