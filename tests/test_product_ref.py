"""The instruments of tests/product_ref.py, the parts that need no GPU: the colouring and the probes on the oracle's matrices
(oracle.smv_upper rebuilt bit for bit), the yardsticks the device bounds derive from (measured on the oracle on every run and
held within a factor of two of the recorded constants, both ways), the condition the CG comparison stands on (no compared
iterate sits on a converged recurrence), and mutants: numpy stand-ins of a subtly wrong product or loop that every assertion
of tests/test_gpu_product_precision.py must catch.  The real library is never asked to misbehave."""
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
