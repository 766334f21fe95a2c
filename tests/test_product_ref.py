"""The instruments of tests/product_ref.py, the parts that need no GPU: the colouring and the probes on the oracle's matrices
(oracle.smv_upper rebuilt bit for bit), the yardsticks the device bounds derive from (measured on the oracle on every run and
held within a factor of two of the recorded constants, both ways), the condition the CG comparison stands on (no compared
iterate sits on a converged recurrence), and mutants: numpy stand-ins of a subtly wrong product or loop that every assertion
of tests/test_gpu_product_precision.py must catch; and the same for the sharded loop (tests/test_gpu_sharded_precision.py): the
float64 loop with the sums of a solve on several ranks as its yardstick, the cuts its cases are chosen for, the mutants of a halo
exchange.  The real library is never asked to misbehave."""
import numpy as np
import pytest

from tests import product_ref as P

_cache = {}


def _model(oracle, name):
    """(job, A, (rowptr, col, val)): the oracle's matrix of a model, upper CRS and full CSR."""
    if name not in _cache:
        j = P.job(name)
        rc, A = oracle.assemble(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        assert rc == 0
        _cache[name] = (j, A, P.full_csr(A))
    return _cache[name]


def _probes(oracle, name, ones=False):
    _j, _A, (rowptr, col, _val) = _model(oracle, name)
    colour = P.cached(("colours", name), lambda: P.colours(rowptr, col, P.cube_grid(name)))
    return P.Probes(rowptr, col, colour, P.weights(rowptr.shape[0] - 1, ones=ones))


def _row_sum(csr):
    """y = A x, every row summed front to back in float64: the plain stand-in of a product."""
    rowptr, col, val = csr
    return lambda x: np.add.reduceat(val * np.asarray(x)[col], rowptr[:-1])


# ---- colouring and probes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.SPMV_MODELS)
def test_probes_rebuild_the_oracles_matrix_bit_for_bit(oracle, name):
    j, A, (rowptr, col, val) = _model(oracle, name)
    pr = _probes(oracle, name)                      # (colours() checks its own property)
    widest = int(np.diff(rowptr).max())
    print("%s: %d rows, %d colours, widest row %d" % (name, pr.n, pr.n_colours, widest))
    if P.cube_grid(name) is not None:
        assert pr.n_colours <= 81 and (pr.n_colours == 81) == (name in ("cube2", "cube6", "cube20"))
    else:
        assert widest <= pr.n_colours <= 2 * widest
    mant, expo = np.frexp(np.abs(pr.w))                   # +-2^e, e in [-8, 8], and not all alike
    assert (mant == 0.5).all() and (expo >= -7).all() and (expo <= 9).all()
    assert (np.abs(pr.w) != 1).any() and (pr.w < 0).any() and (pr.w > 0).any()
    got, stray = pr.sweep(lambda x: oracle.smv_upper(A, x))
    assert stray == 0 and P.same_bits(got, val).all()
    assert np.array_equal(P.csr_diagonal(rowptr, col, val), val[col == P.rows_of(rowptr)]) and (P.csr_diagonal(rowptr, col, val) > 0).all()
    # the full CSR is the upper CRS mirrored, stored zeros included
    assert rowptr[-1] == 2 * A.nnz - A.n and np.array_equal(val[col >= P.rows_of(rowptr)], A.vals)


def test_closed_form_and_greedy_colouring_agree_on_the_property(oracle):
    """The greedy colouring on a cube's pattern (cube6) is a valid one too, and needs no more than twice the closed form's 81;
    the check every colouring goes through sees two columns of one colour in a row."""
    j, _A, (rowptr, col, _val) = _model(oracle, "cube6")
    greedy = P.colours(rowptr, col)
    assert 81 <= greedy.max() + 1 <= 162 and j.n_red == greedy.shape[0]
    bad = P.colours(rowptr, col, P.cube_grid("cube6")).copy()
    bad[col[rowptr[5] + 1]] = bad[col[rowptr[5]]]          # two columns of row 5 in one colour: the check must see it
    nc = int(bad.max()) + 1
    key = P.rows_of(rowptr) * nc + bad[col]
    assert np.unique(key).shape[0] < key.shape[0]


# ---- yardsticks -----------------------------------------------------------------------------------------------------------------

def _within_a_factor_of_two(measured, recorded):
    return 0.5 * recorded < measured < 2 * recorded


def test_spmv_yardstick_is_measured_on_the_oracle(oracle):
    """oracle.smv_upper over SPMV_MODELS x VECTORS in units of each row's scale; the plain float64 row sum meets the device
    bound on every row (another summation order stays inside the margin)."""
    worst, plain = {}, 0.0
    for name in P.SPMV_MODELS:
        _j, A, csr = _model(oracle, name)
        for vn, x in P.vectors(name).items():
            ref, scale = P.row_reference(*csr, x)
            worst[name, vn] = float(P.row_units(oracle.smv_upper(A, x), ref, scale).max())
            u = P.row_units(_row_sum(csr)(x), ref, scale)
            assert (u <= P.row_bound(csr[0])).all(), (name, vn)
            plain = max(plain, float(u.max()))
    print("oracle.smv_upper, worst row units: %s" % ", ".join("%s/%s %.2f" % (k + (v,)) for k, v in worst.items()))
    print("recorded %.2f, device bound %.2f or m_i + 2; float64 row sum %.2f" % (P.ORACLE_SPMV_UNITS_MEASURED, P.DEVICE_SPMV_UNITS, plain))
    assert len(worst) == len(P.SPMV_MODELS) * len(P.VECTORS)
    assert _within_a_factor_of_two(max(worst.values()), P.ORACLE_SPMV_UNITS_MEASURED)
    assert P.DEVICE_SPMV_UNITS == 4 * P.ORACLE_SPMV_UNITS_MEASURED
    # the spread vector does what it is for: the terms of a row lie up to 60 binary orders apart, the rows' own scales (each
    # dominated by its largest term) more than three decimal ones
    _ref, scale = P.row_reference(*_model(oracle, "cube6")[2], P.vectors("cube6")["spread"])
    assert float(scale.max() / scale.min()) > 1e3


def _cg_reference(oracle, name, lc):
    _j, _A, csr = _model(oracle, name)
    return P.cached(("cg", "oracle", name, lc), lambda: P.cg_reference(csr, P.load_cases(name)[lc], P.KMAX))


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_cg_yardsticks_are_measured_on_the_oracle(oracle, name):
    """oracle.cg stopped at max_its = k against the long-double iterates, k = 1 .. KMAX, for the three load vectors; and the
    CONDITION of the whole comparison: the reference residual at the last compared k is above 1e-6 (no comparison runs on a
    converged recurrence, where residual ratios degenerate)."""
    _j, A, _csr = _model(oracle, name)
    for lc, F in enumerate(P.load_cases(name)):
        Us, rels = _cg_reference(oracle, name, lc)
        assert len(Us) == P.KMAX and float(rels[-1]) > 1e-6 and float(min(rels)) > 1e-6
        wu = wr = 0.0
        for k in range(1, P.KMAX + 1):
            U, rep = oracle.cg(A, F, 1e-30, maxits=k, merit_stop=False)
            assert rep["terminationtype"] == 5 and rep["iterations"] == k
            wu, wr = max(wu, P.u_units(U, Us[k - 1])), max(wr, P.res_units(rep["rel_residual"], rels[k - 1]))
        print("%s load case %d: oracle U %.1f / residual %.1f units of 2^-53 (recorded %.1f / %.1f), residual at k = %d: %.2e" %
              (name, lc, wu, wr, P.ORACLE_CG_U_UNITS_MEASURED[name][lc], P.ORACLE_CG_RES_UNITS_MEASURED[name][lc], P.KMAX, float(rels[-1])))
        assert _within_a_factor_of_two(wu, P.ORACLE_CG_U_UNITS_MEASURED[name][lc])
        assert _within_a_factor_of_two(wr, P.ORACLE_CG_RES_UNITS_MEASURED[name][lc])
    F = P.load_cases(name)
    assert not any(np.array_equal(F[a], F[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def _worst(its, Us, rels):
    return (max(P.u_units(u, Us[k]) for k, (u, _r) in enumerate(its)), max(P.res_units(r, rels[k]) for k, (_u, r) in enumerate(its)))


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_single_reduction_yardstick_and_the_float64_classic_loop(oracle, name):
    """cg_single_reduce_f64 against the same long-double iterates: the recorded yardstick of STAN_OPT_CG_SINGLE_REDUCE.  The
    classic loop in the same float64 numpy arithmetic (other sums than the oracle's) stays inside 4 x the oracle's figures."""
    j, _A, csr = _model(oracle, name)
    Us, rels = _cg_reference(oracle, name, 0)
    its = P.cg_single_reduce_f64(csr, j.F, P.KMAX)
    assert len(its) == P.KMAX
    wu, wr = _worst(its, Us, rels)
    print("%s: single-reduction float64 U %.1f / residual %.1f units (recorded %.1f / %.1f)" %
          (name, wu, wr, P.SR_CG_U_UNITS_MEASURED[name], P.SR_CG_RES_UNITS_MEASURED[name]))
    assert _within_a_factor_of_two(wu, P.SR_CG_U_UNITS_MEASURED[name]) and _within_a_factor_of_two(wr, P.SR_CG_RES_UNITS_MEASURED[name])
    cu, cr = _worst(P.cg_iterates(P.Scaled(*csr, T=np.float64), j.F, P.KMAX), Us, rels)
    print("%s: classic float64 numpy U %.1f / residual %.1f units" % (name, cu, cr))
    assert cu <= P.DEVICE_CG_FACTOR * P.ORACLE_CG_U_UNITS_MEASURED[name][0] and cr <= P.DEVICE_CG_FACTOR * P.ORACLE_CG_RES_UNITS_MEASURED[name][0]


def test_scaled_residual_bar_holds_for_the_float64_statement(oracle):
    """Matrix.scaled_residual as stan_amd/hip.py states it, on the float64 row sum, against the long-double value."""
    for name in ("cube6", "perforated12"):
        j, _A, csr = _model(oracle, name)
        U = np.random.default_rng(5).standard_normal(j.n_red)
        ref, bar = P.scaled_residual_reference(*csr, j.F, U, P.row_bound(csr[0]))
        d = P.csr_diagonal(*csr)
        s = 1.0 / np.sqrt(d)
        got = float(np.linalg.norm(s * (j.F - _row_sum(csr)(U))) / np.linalg.norm(s * j.F))
        print("%s: scaled residual %.17g, reference %.17g, off by %.2e (bar %.2e)" % (name, got, ref, abs(got / ref - 1), bar))
        assert abs(got / ref - 1) <= bar < 1e-11


# ---- mutants ----------------------------------------------------------------------------------------------------------------------

def _longest_row(rowptr):
    return int(np.argmax(np.diff(rowptr)))


def _dropped_last_slot(csr):
    """The last slot of the longest row -- its last 3 x 3 block: the row's last three entries -- never reaches the sum."""
    rowptr, col, val = csr
    v = val.copy()
    end = rowptr[_longest_row(rowptr) + 1]
    assert col[end - 1] - col[end - 3] == 2 and v[end - 3:end].all()
    v[end - 3:end] = 0.0
    return _row_sum((rowptr, col, v))


def _swapped_gather(csr, colour):
    """(product, same_colour): one row gathers x for one of its entries from a column that is not the entry's -- a lane reading
    a neighbour's column word.  The wrong column has the entry's own colour wherever the colouring leaves one outside the row
    (same_colour; on star12 every column has a colour of its own, and the swap reads an exact zero instead)."""
    rowptr, col, val = csr
    n = rowptr.shape[0] - 1
    pick = None
    for i in np.argsort(-np.diff(rowptr), kind="stable"):
        mine = col[rowptr[i]:rowptr[i + 1]]
        for q in range(rowptr[i], rowptr[i + 1]):
            other = np.setdiff1d(np.nonzero(colour == colour[col[q]])[0], mine)
            if other.size and val[q] != 0:
                pick = (int(i), int(q), int(other[0]), True)
                break
        if pick:
            break
    if pick is None:
        i = int(np.argmin(np.diff(rowptr)))
        pick = (i, int(rowptr[i]), int(np.setdiff1d(np.arange(n), col[rowptr[i]:rowptr[i + 1]])[0]), False)
    i, q, j2, same = pick
    j1 = col[q]
    base = _row_sum(csr)

    def product(x):
        y = base(x)
        y[i] = y[i] - val[q] * x[j1] + val[q] * x[j2]
        return y
    return product, same


def _float32_row(csr):
    rowptr, col, val = csr
    i = _longest_row(rowptr)
    base = _row_sum(csr)

    def product(x):
        y = base(x)
        sl = slice(rowptr[i], rowptr[i + 1])
        y[i] = (val[sl].astype(np.float32) * np.asarray(x)[col[sl]].astype(np.float32)).sum(dtype=np.float32)
        return y
    return product


@pytest.mark.parametrize("name", ["cube6", "perforated12", "star12"])
def test_product_mutants_exceed_the_bounds(oracle, name):
    """Part A: a dropped slot, a swapped gather and a row accumulated in float32 each change rebuilt bits; the swap between two
    columns of one colour passes under all-ones weights, which is why the weights differ.  Part B: the dropped slot and the
    float32 row exceed the row bound under each of the three vectors."""
    _j, _A, csr = _model(oracle, name)
    rowptr, col, val = csr
    pr, pr1 = _probes(oracle, name), _probes(oracle, name, ones=True)
    got, stray = pr.sweep(_row_sum(csr))
    assert stray == 0 and P.same_bits(got, val).all()                     # the stand-in itself is exact under probing
    swapped, same_colour = _swapped_gather(csr, pr.colour)
    assert same_colour == (name != "star12")
    for label, mutant in (("dropped slot", _dropped_last_slot(csr)), ("swapped gather", swapped), ("float32 row", _float32_row(csr))):
        got, stray = pr.sweep(mutant)
        wrong = int((~P.same_bits(got, val)).sum())
        print("%s, %s: %d rebuilt entries differ, %d stray" % (name, label, wrong, stray))
        assert wrong >= 1 or stray >= 1, label
    if same_colour:
        got, stray = pr1.sweep(swapped)
        assert stray == 0 and P.same_bits(got, val).all()                 # all-ones weights cannot see the swap
    bound = P.row_bound(rowptr)
    for label, mutant in (("dropped slot", _dropped_last_slot(csr)), ("float32 row", _float32_row(csr))):
        for vn, x in P.vectors(name).items():
            ref, scale = P.row_reference(*csr, x)
            u = P.row_units(mutant(x), ref, scale)
            print("%s, %s, %s: worst row %.3g x its bound" % (name, label, vn, float((u / bound).max())))
            assert (u > bound).any(), (label, vn)


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_loop_mutants_exceed_the_bounds(oracle, name):
    """Part C: p . A p without the last block's partial (the rows of the last slice), and beta formed from the rho of one
    iteration earlier, both in the float64 classic loop: each exceeds 4 x the oracle's figures in U and in the residual, the
    first at once, the second from the iteration after it takes effect -- where a bar of 1e-9 of max|U| passes the late
    beta's early iterates."""
    j, _A, csr = _model(oracle, name)
    Us, rels = _cg_reference(oracle, name, 0)
    A = P.Scaled(*csr, T=np.float64)
    bu, br = P.DEVICE_CG_FACTOR * P.ORACLE_CG_U_UNITS_MEASURED[name][0], P.DEVICE_CG_FACTOR * P.ORACLE_CG_RES_UNITS_MEASURED[name][0]
    tail = j.n_red - 3 * 64
    for label, kw in (("p.Ap without the last block", dict(pap=lambda p, v: (p[:tail] * v[:tail]).sum())), ("late beta", dict(late_beta=True))):
        its = P.cg_iterates(A, j.F, P.KMAX, **kw)
        u = [P.u_units(x, Us[k]) for k, (x, _r) in enumerate(its)]
        r = [P.res_units(rr, rels[k]) for k, (_x, rr) in enumerate(its)]
        first = next(k + 1 for k in range(P.KMAX) if u[k] > bu or r[k] > br)
        print("%s, %s: first iterate over the bound k = %d; worst U %.3g / residual %.3g units (bounds %.0f / %.0f)" %
              (name, label, first, max(u), max(r), bu, br))
        assert first <= 3 and max(u) > bu and max(r) > br
        assert all(u[k] > bu or r[k] > br for k in range(first - 1, P.KMAX))       # and every later k stays caught


@pytest.mark.parametrize("name", P.CG_MODELS)
@pytest.mark.parametrize("stream", list(P.QUANTISE))
def test_reduced_precision_yardstick_and_the_decode_mutant(oracle, name, stream):
    """The pair (reference on the matrix quantised from long-double entries, float64 loop on the matrix quantised from float64
    entries) must tell a decode error from rounding: the yardstick stays within a factor of two of its recorded value, and the
    float64 loop with ONE of the nine entries of every block off by 2^-30 -- what iterative refinement would heal at the price
    of a few passes -- exceeds 4 x the yardstick by k = 3."""
    j, _A, csr = _model(oracle, name)
    q = P.QUANTISE[stream]
    Us, rels = P.cg_reference(csr, j.F, P.KMAX_REDUCED, quantise=q)
    assert float(min(rels)) > 1e-6
    A = P.Scaled(*csr, T=np.float64, quantise=q)
    wu, wr = _worst(P.cg_iterates(A, j.F, P.KMAX_REDUCED), Us, rels)
    ru, rr = P.REDUCED_CG_UNITS_MEASURED[stream, name]
    moved = int((A.a.astype(P.LD) != P.Scaled(*csr, T=P.LD, quantise=q).a).sum())
    print("%s %s: float64 loop U %.1f / residual %.1f units (recorded %.1f / %.1f); %d of %d entries quantised to the other side" %
          (name, stream, wu, wr, ru, rr, moved, csr[2].shape[0]))
    assert _within_a_factor_of_two(wu, ru) and _within_a_factor_of_two(wr, rr)
    one_of_nine = (P.rows_of(csr[0]) % 3 == 0) & (csr[1] % 3 == 1)
    assert one_of_nine.sum() * 9 == csr[2].shape[0]
    A.a = A.a + np.where(one_of_nine, 2.0 ** -30, 0.0)
    its = P.cg_iterates(A, j.F, 3)
    u, r = P.u_units(its[2][0], Us[2]), P.res_units(its[2][1], rels[2])
    print("%s %s: one entry of nine off by 2^-30: U %.3g / residual %.3g units at k = 3 (bounds %.0f / %.0f)" %
          (name, stream, u, r, P.DEVICE_CG_FACTOR * ru, P.DEVICE_CG_FACTOR * rr))
    assert u > P.DEVICE_CG_FACTOR * ru and r > P.DEVICE_CG_FACTOR * rr


# ---- the sharded loop: yardstick and mutants ----------------------------------------------------------------------------------------

SHARD_RANKS = (2, 3, 4, 8)


def _ranks_of(name, nranks):
    return P.cached(("rank_of_rows", name, nranks), lambda: P.rank_of_rows(P.job(name), nranks))


def _series(its, Us, rels):
    """(U units, residual units) per k; an iterate that is not finite (a mutant's division by a zero sum) counts as infinitely far."""
    finite = [bool(np.isfinite(u).all() and np.isfinite(r)) for u, r in its]
    return ([P.u_units(u, Us[k]) if finite[k] else np.inf for k, (u, _r) in enumerate(its)],
            [P.res_units(r, rels[k]) if finite[k] else np.inf for k, (_u, r) in enumerate(its)])


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_rank_ordered_sums_stay_inside_the_one_rank_bounds(oracle, built_libs, name):
    """The yardstick of tests/test_gpu_sharded_precision.py: the float64 loop with every sum formed rank by rank and added in
    rank order (P.rank_dot), on 2, 3, 4 and 8 ranks, keeps the bounds of the one-rank loop -- 4 x the oracle's figures for the
    classic loop under the job's own load vector and under the seeded normal one, 4 x the single-reduction yardstick for the
    Chronopoulos-Gear recurrences -- so a sharded solve that exceeds them does so for another reason than the order of its
    sums.  Load case 2 is left out here and on the device: its margin on perforated12 is a few per cent (a restatement that
    took the node number for the block row read 233 units against 245).
    Measured, worst over k = 1 .. 22, U / residual units on 2, 3, 4, 8 ranks (rows dealt to the ranks as the device deals them:
    the block row of a node is its place in the reference's DOF order, node_index, not its number):
      classic, load case 0     cube6 39.1/102.6 37.8/63.6 36.3/45.5 35.6/62.9 (bounds 84/142)
                               perforated12 76.5/104.0 70.3/110.3 73.4/114.5 77.1/119.7 (432/346)
      classic, load case 1     cube6 7.9/45.2 8.4/22.2 8.9/19.6 11.4/27.4 (54/217)
                               perforated12 11.9/31.6 12.8/35.8 14.2/30.2 14.2/38.6 (130/295)
      single reduction, 0      cube6 44.1/56.7 42.3/93.0 62.1/183.1 70.2/148.1 (219/380)
                               perforated12 201.4/313.3 132.6/219.1 164.1/236.9 159.1/273.5 (880/1299)"""
    j, _A, csr = _model(oracle, name)
    F = P.load_cases(name)
    A = P.Scaled(*csr, T=np.float64)
    for nranks in SHARD_RANKS:
        dot = P.rank_dot(_ranks_of(name, nranks), nranks)
        for lc in (0, 1):
            bu, br = P.sharded_cg_bounds(name, lc)
            u, r = _series(P.cg_iterates(A, F[lc], P.KMAX, dot=dot), *_cg_reference(oracle, name, lc))
            print("%s on %d ranks, classic, load case %d: U %.1f / residual %.1f units (bounds %.0f / %.0f)" % (name, nranks, lc, max(u), max(r), bu, br))
            assert max(u) <= bu and max(r) <= br, (nranks, lc)
        bu, br = P.sharded_cg_bounds(name, 0, single_reduction=True)
        u, r = _series(P.cg_single_reduce_f64(csr, F[0], P.KMAX, dot=dot), *_cg_reference(oracle, name, 0))
        print("%s on %d ranks, single reduction, load case 0: U %.1f / residual %.1f units (bounds %.0f / %.0f)" % (name, nranks, max(u), max(r), bu, br))
        assert max(u) <= bu and max(r) <= br, nranks
    assert np.array_equal(F[0], j.F) and (F[1] != 0).all()      # load case 1 is nonzero in every row: every halo entry works from k = 1


def test_the_sharded_cases_cut_where_they_are_meant_to(oracle, built_libs):
    """What the cases of tests/test_gpu_sharded_precision.py are there for, on the oracle's pattern: every rank that owns rows has
    entries across a cut, whatever the model and the rank count; cube6 on 2 ranks runs both lists of the split product on both
    ranks ((1, 2) and (1, 2) interior / boundary slices), on 4 ranks no rank has an interior slice at all (the boundary launch
    alone: (0, 1) (0, 2) (0, 1) (0, 2)), on 8 ranks ranks 0 and 4 own no row (block rows cut at 0 0 64 128 192 192 256 320 343).
    perforated12 on 3 ranks: (7, 4) (0, 11) (5, 7); on 4: (5, 3) (0, 9) (0, 8) (2, 7)."""
    from stan_amd import host
    for name in P.CG_MODELS:
        j, _A, csr = _model(oracle, name)
        for nranks in SHARD_RANKS:
            rank = _ranks_of(name, nranks)
            halo = P.halo_entries(csr, rank)
            owners = np.unique(rank)
            census = P.slice_census(j, csr, nranks)
            print("%s on %d ranks: %d halo entries of %d, slices (interior, boundary) %s" % (name, nranks, halo.sum(), halo.shape[0], census))
            assert np.array_equal(np.unique(rank[P.rows_of(csr[0])[halo]]), owners)
            assert all((i + b > 0) == (r in owners) for r, (i, b) in enumerate(census))
            assert sum(i + b for i, b in census) == -(-j.xyz.shape[0] // 64)
    j, _A, csr = _model(oracle, "cube6")
    assert P.slice_census(j, csr, 2) == [(1, 2), (1, 2)]
    assert any(i == 0 and b > 0 for i, b in P.slice_census(j, csr, 4))
    assert any(i + b == 0 for i, b in P.slice_census(j, csr, 8))
    assert list(host.partition_plan(j.node_index, j.conn, 8, 0)["row_starts"]) == [0, 0, 64, 128, 192, 192, 256, 320, 343]
    assert np.array_equal(np.bincount(_ranks_of("cube6", 8), minlength=8) == 0, [True, False, False, False, True, False, False, False])


class _HaloProduct:
    """y = A^ x with the terms across a cut reading another vector than x: seen(x, previous) -- what the halo region holds when
    the product runs; previous is the vector of the product before this one (the first product: x itself)."""

    def __init__(self, A, halo, seen):
        self.A, self.halo, self.seen, self.previous = A, halo, seen, None

    def __call__(self, x):
        xh = self.seen(x, x if self.previous is None else self.previous)
        self.previous = x
        return np.add.reduceat(self.A.a * np.where(self.halo, xh[self.A.col], x[self.A.col]), self.A.rowptr[:-1])


def _first_over(u, r, bu, br):
    return next((k + 1 for k in range(len(u)) if u[k] > bu or r[k] > br), None)


@pytest.mark.parametrize("nranks", [2, 3, 4])
@pytest.mark.parametrize("name", P.CG_MODELS)
def test_sharded_mutants_exceed_the_bounds(oracle, built_libs, name, nranks):
    """Stand-ins of what a sharded loop can get wrong and both transports would share, each in the float64 classic loop with
    rank-ordered sums, each over the bound of the yardstick test at the stated k AND at every later k:
      (a) the halo columns read the vector of the product before (a missing wait for the exchange): load case 0, from k = 2;
      (b) the halo columns read float32(p): load case 0, from k = 1 -- the first product whose vector is not float32 in a halo
          column: k = 2 for perforated12 on 2 ranks, whose cut lies where the job's load vector is still zero;
      (c) p . A p without the last rank's partial: load case 0, from k = 1;
      (d) ONE term a_ij x_j across a cut dropped -- the first, the middle and the last of the non-zero halo entries: load case 1,
          from k = 1.  Under the job's own load vector the same mutant is first caught as late as k = 6 (cube6) or k = 9
          (perforated12 on 4 ranks): the load reaches that row late.  That is why the device test runs load case 1 as well.
    A bar of 1e-4 of max|U| passes (b) by three orders (1e9 units are 1e-7) and (d) where the dropped term is small (cube6 on 4
    ranks, the middle entry: 4.2e11 units, 4.6e-5)."""
    j, _A, csr = _model(oracle, name)
    A = P.Scaled(*csr, T=np.float64)
    F = P.load_cases(name)
    rank = _ranks_of(name, nranks)
    halo = P.halo_entries(csr, rank)
    dot = P.rank_dot(rank, nranks)
    owners = [int(r) for r in np.unique(rank)]

    def run(lc, **kw):
        bu, br = P.sharded_cg_bounds(name, lc)
        u, r = _series(P.cg_iterates(A, F[lc], P.KMAX, dot=dot, **kw), *_cg_reference(oracle, name, lc))
        first = _first_over(u, r, bu, br)
        return first, first is not None and all(u[k] > bu or r[k] > br for k in range(first - 1, P.KMAX)), max(u), max(r)

    f32 = lambda x, _previous: x.astype(np.float32).astype(np.float64)      # noqa: E731
    # (b) can act from the first product whose vector is no float32 number in a column some non-zero halo entry reads
    seen = []
    P.cg_iterates(A, F[0], 3, dot=dot, mv=lambda x: (seen.append(x), A.mv(x))[1])
    live = np.nonzero(halo & (A.a != 0))[0]
    k_f32 = next(k + 1 for k, x in enumerate(seen) if (f32(x, None) != x)[A.col[live]].any())
    assert k_f32 == (2 if (name, nranks) == ("perforated12", 2) else 1)
    mutants = [("(a) stale halo", 0, 2, dict(mv=_HaloProduct(A, halo, lambda _x, previous: previous))),
               ("(b) float32 halo", 0, k_f32, dict(mv=_HaloProduct(A, halo, f32))),
               ("(c) p.Ap without the last rank", 0, 1, dict(pap=P.rank_dot(rank, nranks, ranks=owners[:-1])))]
    late = []
    for label, q in (("first", live[0]), ("middle", live[live.shape[0] // 2]), ("last", live[-1])):
        B = P.Scaled(*csr, T=np.float64)
        B.a[q] = 0.0
        mutants.append(("(d) %s halo term dropped" % label, 1, 1, dict(mv=B.mv)))
        late.append(run(0, mv=B.mv)[0])
    for label, lc, k_stated, kw in mutants:
        first, stays, wu, wr = run(lc, **kw)
        print("%s on %d ranks, %s, load case %d: first iterate over the bound k = %s; worst U %.3g / residual %.3g units" %
              (name, nranks, label, lc, first, wu, wr))
        assert first == k_stated and stays, label
    print("%s on %d ranks, (d) under load case 0: first caught at k = %s" % (name, nranks, late))
    assert all(k is not None for k in late) and max(late) > 1


# ---- the reduced streams in the single-reduction loop, REFINE 2, the refinement passes, the restart ----------------------------------
# (tests/test_gpu_reduced_forms.py, tests/test_gpu_refinement_passes.py, tests/test_gpu_cg_restart.py)

def _one_of_nine(csr):
    mask = (P.rows_of(csr[0]) % 3 == 0) & (csr[1] % 3 == 1)
    assert mask.sum() * 9 == csr[2].shape[0]
    return mask


@pytest.mark.parametrize("name", P.CG_MODELS)
@pytest.mark.parametrize("stream", list(P.QUANTISE))
def test_reduced_single_reduction_yardstick_and_the_decode_mutant(oracle, name, stream):
    """The Chronopoulos-Gear restatement on the quantised matrix (cg_single_reduce_f64(quantise=)) against the long-double CG on
    the matrix quantised from long-double entries: within a factor of two of the recorded constant both ways, and with one
    entry of nine off by 2^-30 over 4 x it in U and in the residual by k = 3."""
    j, _A, csr = _model(oracle, name)
    q = P.QUANTISE[stream]
    Us, rels = P.cg_reference(csr, j.F, P.KMAX_REDUCED, quantise=q)
    wu, wr = _worst(P.cg_single_reduce_f64(csr, j.F, P.KMAX_REDUCED, quantise=q), Us, rels)
    ru, rr = P.REDUCED_SR_CG_UNITS_MEASURED[stream, name]
    print("%s %s: single-reduction float64 loop U %.1f / residual %.1f units (recorded %.1f / %.1f)" % (name, stream, wu, wr, ru, rr))
    assert _within_a_factor_of_two(wu, ru) and _within_a_factor_of_two(wr, rr)
    bump = np.where(_one_of_nine(csr), 2.0 ** -30, 0.0)
    its = P.cg_single_reduce_f64(csr, j.F, 3, quantise=lambda a: q(a) + bump)
    u, r = P.u_units(its[2][0], Us[2]), P.res_units(its[2][1], rels[2])
    print("%s %s: one entry of nine off by 2^-30: U %.3g / residual %.3g units at k = 3" % (name, stream, u, r))
    assert u > P.DEVICE_CG_FACTOR * ru and r > P.DEVICE_CG_FACTOR * rr


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_refine2_yardstick_and_the_refresh_on_the_reduced_values(oracle, name):
    """STAN_OPT_CG_REFINE 2 on the float32 stream: the loop that refreshes at iteration 50 and not before, with b^ - A^64 x there.
    The float64 restatement against long double at k = 48 .. 52 stays within a factor of two of its recorded figures; no
    compared iterate sits on a converged recurrence; and the mutant -- the refresh at 50 formed with the REDUCED values, what
    REFINE 1 does -- is the same bits up to 49 and exceeds 4 x the yardstick at k = 51 and 52 in U, and from k = 50 in the
    recurrence residual, which is why the device test asserts both.  FIXED-48: the two references themselves are closer than
    the yardstick in U (printed), so no iterate comparison can tell the two refreshes apart; the device test counts products."""
    j, _A, csr = _model(oracle, name)
    for stream in ("mixed", "fixed48"):
        q = P.QUANTISE[stream]
        AqL, A64L = P.Scaled(*csr, T=P.LD, quantise=q), P.Scaled(*csr, T=P.LD)
        Aq, A64 = P.Scaled(*csr, T=np.float64, quantise=q), P.Scaled(*csr, T=np.float64)
        ref = P.cg_iterates(AqL, j.F, 52, rupdate=50, refresh_with=A64L.mv)
        other = P.cg_iterates(AqL, j.F, 52, rupdate=50)
        yard = P.cg_iterates(Aq, j.F, 52, rupdate=50, refresh_with=A64.mv)
        mutant = P.cg_iterates(Aq, j.F, 52, rupdate=50)
        ks = [k - 1 for k in P.REFINE2_KS]
        yu, yr = max(P.u_units(yard[k][0], ref[k][0]) for k in ks), max(P.res_units(yard[k][1], ref[k][1]) for k in ks)
        mu = {k + 1: P.u_units(mutant[k][0], ref[k][0]) for k in ks}
        mr = {k + 1: P.res_units(mutant[k][1], ref[k][1]) for k in ks}
        apart = {k + 1: P.u_units(np.asarray(other[k][0], dtype=np.float64), ref[k][0]) for k in (50, 51)}
        print("%s %s: REFINE 2 yardstick U %.3g / residual %.3g units; refresh on the reduced values: U %s, residual %s; the two "
              "references apart by %s; residual at k = 52: %.2e" % (name, stream, yu, yr, {k: "%.3g" % v for k, v in mu.items()},
                                                                    {k: "%.3g" % v for k, v in mr.items()}, {k: "%.3g" % v for k, v in apart.items()}, float(ref[51][1])))
        assert float(min(r for _u, r in ref)) > 1e-6
        if stream == "fixed48":
            assert max(apart.values()) < yu                      # nothing to tell apart
            continue
        ru, rr = P.REFINE2_UNITS_MEASURED[name]
        assert _within_a_factor_of_two(yu, ru) and _within_a_factor_of_two(yr, rr)
        assert all(np.array_equal(mutant[k][0], yard[k][0]) for k in range(49))
        assert mu[51] > P.DEVICE_CG_FACTOR * yu and mu[52] > P.DEVICE_CG_FACTOR * yu
        assert all(mr[k] > P.DEVICE_CG_FACTOR * yr for k in (50, 51, 52))


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_second_pass_yardstick_its_condition_and_mutants(oracle, name):
    """The refinement passes of a float32 solve to 1e-10.  CONDITION: at the first pass's stop n1 and one iteration earlier the
    float64 stand-in's residual is at least 1 % from eps (measured: 3 % on perforated12, 15 % on cube6).  That makes n1 the
    device's on cube6, where no order of the sums moves the third digit; on perforated12, 322 iterations in, the order of the
    sums alone moves the residual at the stop between 0.93 and 0.98 eps and long double stops at 320: the device may read 322
    or 323, and its test takes n1 from the device.  The second
    pass from the stand-in's U_1: the float64 restatement (r_t and the loop in float64, fl(U_1 + S d_k) - U_1) against long
    double stays within a factor of two of its recorded figure, and at 4 x it
      r_t formed with the reduced values (the pass would iterate on its own recurrence's residual) is over at every k,
      a pass that iterates on the fp64 matrix is over at k = 10 and 12 (it starts out inside: one step barely tells),
      a dropped k_accumulate (U = S d_k alone) is over at every k."""
    j, _A, csr = _model(oracle, name)
    q = P.QUANTISE["mixed"]
    n1, rels, U1 = P.first_pass_f64(csr, j.F, P.REFINE_EPS, q)
    margins = [abs(r / P.REFINE_EPS - 1) for r in rels[-2:]]
    rel64 = P.rel64_of(csr, j.F, U1)
    print("%s: first pass %d iterations, |rel / eps - 1| before / at the stop %.3f / %.3f, rel64 %.3e" % (name, n1, margins[0], margins[1], rel64))
    assert n1 == P.FIRST_PASS_ITS_MEASURED[name] and min(margins) >= 0.01 and rel64 > 1.01 * P.REFINE_EPS
    # what that margin is worth: the same loop with its sums formed in 64 and in 256 chunks, and in long double
    Aq = P.Scaled(*csr, T=np.float64, quantise=q)
    chunked = {c: P.cg_iterates(Aq, j.F, 2 * n1, stop=P.REFINE_EPS, dot=P.rank_dot(np.arange(j.n_red) * c // j.n_red, c)) for c in (64, 256)}
    n1_ld = len(P.cg_iterates(P.Scaled(*csr, T=P.LD, quantise=q), j.F, 2 * n1, stop=P.REFINE_EPS))
    print("%s: residual over eps at the stop with the sums in 64 / 256 chunks: %s; long double stops at %d" %
          (name, ", ".join("%.3f at %d" % (its[-1][1] / P.REFINE_EPS, len(its)) for its in chunked.values()), n1_ld))
    assert all(abs(len(its) - n1) <= 1 for its in chunked.values()) and abs(n1_ld - n1) <= 2
    ref, _rt = P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q)
    units = lambda ds: [P.step_units(P.added_f64(U1, d), ref[k]) for k, d in enumerate(ds)]      # noqa: E731
    yard = units(P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q, T=np.float64)[0])
    reduced_rt = units(P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q, T=np.float64, rhs_quantise=q)[0])
    fp64_loop = units(P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q, T=np.float64, loop_quantise=None)[0])
    dropped = [P.step_units(d - U1, ref[k]) for k, d in enumerate(P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q, T=np.float64)[0])]
    bound = P.DEVICE_CG_FACTOR * max(yard)
    print("%s: second pass yardstick %.3g units (recorded %.3g); r_t from the reduced values %.3g .. %.3g, fp64 loop %.3g .. %.3g, "
          "dropped accumulate %.3g .. %.3g; max|S d_k| / max|U_1| %.2e .. %.2e" %
          (name, max(yard), P.SECOND_PASS_UNITS_MEASURED[name], min(reduced_rt), max(reduced_rt), min(fp64_loop), max(fp64_loop),
           min(dropped), max(dropped), float(abs(ref[0]).max() / abs(U1).max()), float(abs(ref[-1]).max() / abs(U1).max())))
    assert _within_a_factor_of_two(max(yard), P.SECOND_PASS_UNITS_MEASURED[name])
    assert min(reduced_rt) > bound and min(dropped) > bound
    assert fp64_loop[9] > bound and fp64_loop[11] > bound


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_fixed48_driver_takes_two_passes_away_from_every_threshold(oracle, name):
    """FIXED-48 at eps_f = REFINE_EPS_FIXED48: the float64 restatement of the driver takes exactly two passes, and every stop
    decision -- the loop's residual at each pass's stop and one iteration earlier against eps_pass, the fp64 check behind each
    pass against eps_f -- is a factor 1.01 from its threshold.  (The iterates of the second pass are not compared on the
    device: rel64 behind pass 1 is 2e-12 and max|S d| / max|U_1| 4e-14, a few hundred units of 2^-53 of U_1 -- rounding noise.)"""
    j, _A, csr = _model(oracle, name)
    passes = P.refine_driver_f64(csr, j.F, P.REFINE_EPS_FIXED48, P.QUANTISE["fixed48"])
    print("%s: %s" % (name, [(p["its"], round(p["stop"], 3), round(p["before"], 3), round(p["check"], 3)) for p in passes]))
    assert tuple(p["its"] for p in passes) == P.FIXED48_PASSES_MEASURED[name]
    assert P.two_passes_clear_of_thresholds(passes)


@pytest.mark.parametrize("name,mult", P.RESTART_CASES)
def test_one_step_instrument_sees_a_loop_without_the_restart(oracle, name, mult):
    """The restart every n_red iterations (k_update: beta stays 0 when k % its_before_restart == 0), on the stretched cubes
    under STAN_OPT_CG_RUPDATE 6, where k = n_red is a refresh iteration too: the step behind it is S (alpha r) with r = b^ - A^
    x_k, whatever came before (P.one_step, from the loop's own U_k).  CONDITION: the true residual at U_k is above 1e-4 (on
    cube1 / cube2 the recurrence has converged by n_red and the step is below rounding).  The float64 loop WITH the restart
    stays inside 4 x max(yardstick, floor) -- on the fp64 values, both reduced streams, the three load vectors and in the
    single-reduction recurrences (k_vec_sr restarts in the iteration behind, (k - 1) % n_red == 0) -- and the loop WITHOUT it
    (k = n_red only: by 2 n_red that loop has converged) exceeds the bound by a factor of 1e6 and more (measured: 1e10)."""
    j, _A, csr = _model(oracle, name)
    n, ru = j.n_red, P.RESTART_RUPDATE
    k = mult * n
    assert n % ru == 0 and n == {"cube1s": 12, "cube2s": 54}[name]

    def figures(U_k, U_next, F, q):
        d_ref, true_res = P.one_step(csr, F, U_k, quantise=q)
        yard = P.step_units(P.added_f64(U_k, P.one_step(csr, F, U_k, quantise=q, T=np.float64)[0]), d_ref)
        return P.step_units(U_next - U_k, d_ref), yard, P.step_floor(U_k, d_ref), float(true_res)

    for stream, q in [("fp64", None)] + list(P.QUANTISE.items()):
        A = P.Scaled(*csr, T=np.float64, quantise=q)
        for lc, F in enumerate(P.load_cases(name) if q is None else [j.F]):
            its = P.cg_iterates(A, F, k + 1, rupdate=ru, restart=n)
            got, yard, floor, true_res = figures(its[k - 1][0], its[k][0], F, q)
            print("%s %s load case %d, k = %d: the float64 loop reads %.3g units (yardstick %.3g, floor %.3g), true residual %.2e" %
                  (name, stream, lc, k, got, yard, floor, true_res))
            assert true_res > 1e-4 and got <= P.DEVICE_CG_FACTOR * max(yard, floor)
            if q is None and lc == 0:
                ry, rf = P.RESTART_STEP_UNITS_MEASURED[name, mult]
                assert _within_a_factor_of_two(yard, ry) and _within_a_factor_of_two(floor, rf)
            if mult == 1:
                its = P.cg_iterates(A, F, k + 1, rupdate=ru)
                got, yard, floor, _res = figures(its[k - 1][0], its[k][0], F, q)
                print("    without the restart: %.3g units, %.1e x the bound" % (got, got / (P.DEVICE_CG_FACTOR * max(yard, floor))))
                assert got > 1e6 * P.DEVICE_CG_FACTOR * max(yard, floor)
    for restart in (n, 0):
        its = P.cg_single_reduce_f64(csr, j.F, k + 1, rupdate=ru, restart=restart)
        got, yard, floor, _res = figures(its[k - 1][0], its[k][0], j.F, None)
        print("%s single reduction, restart %d, k = %d: %.3g units (yardstick %.3g, floor %.3g)" % (name, restart, k, got, yard, floor))
        if restart:
            assert got <= P.DEVICE_CG_FACTOR * max(yard, floor)
        elif mult == 1:
            assert got > 1e6 * P.DEVICE_CG_FACTOR * max(yard, floor)
