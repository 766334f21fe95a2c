"""The product kernels (spmv_kernels.inc) and the CG loop (cg_vector_kernels.inc, cg_reduce_device.inc, cg_multi.inc) against
the instruments of tests/product_ref.py, through Matrix.spmv / to_csr / diagonal / scaled_residual and cg_solve /
cg_solve_multi stopped at max_its = k -- no entry of the library's is added for it.

A  Probing vectors rebuild the matrix from products, entry by entry: bit for bit on a fresh matrix, for every form
   launch_product routes Matrix.spmv to; within the derived (R + 2) x 2^-53 |a_ij| once a solve has scaled the matrix (which
   is also where the packed column stream and the folded copy exist: a fresh matrix has neither, see below).
B  Row sums against a long-double reference in units of 2^-53 sum_j |a_ij| |x_j|: at most the smaller of 4 x the oracle's
   worst figure and the derived m_i + 2.
C  Every CG iterate k = 1 .. 22 against a long-double CG on the exported matrix, U and the reported residual in units of 2^-53:
   at most 4 x the oracle's figure for the same model and load vector.

No bound here is fitted to the device; each test prints the worst figure it saw, and the docstrings record them.

A fact the forms below rest on: the packed column stream is built by a solve (cg_run::setup, stan_matrix_make_cols16), not by
the assembly.  Matrix.spmv on a FRESH matrix therefore walks the int32 columns whatever STAN_OPT_PACKED_COLUMNS says; both
settings are still run there, and the packed loops (walk_slots' two-slots-per-trip form with its tail, k_spmv_small's packed
branch, modes 1 and 2) are reached by the sweeps on the scaled matrix, where the profile of the solve in front of them says
how many slots are packed."""
import numpy as np
import pytest

from stan_amd import hip
from tests import product_ref as P
from tests.gpu_models import LARGE, PADDED, assemble as _assemble, model as _model, options as _options, reduced_reference, reference as _reference

pytestmark = pytest.mark.gpu

# form -> options: what launch_product (cg.hip) routes a plain fp64 product to
FORMS = {
    "small": {},                                                    # k_spmv_small<double, 0>
    "v0": {**PADDED, hip.OPT_SPMV_VARIANT: 0},                 # k_spmv<double, 0, 0>
    "v9": {**PADDED, hip.OPT_SPMV_VARIANT: 9},                 # k_spmv<double, 0, 9>
    "v12": {**PADDED, hip.OPT_SPMV_VARIANT: 12},               # k_spmv<double, 0, 12>
    "pair": {**PADDED, hip.OPT_SPMV_VARIANT: 20},              # k_spmv_pair<double, 0, true>
    "fold": {**LARGE, hip.OPT_ROW_FOLDING: 1},                # k_spmv_fold<double, 0, 1>: the scaled matrix only
}
FRESH_FORMS = ("small", "v0", "v9", "v12", "pair")
FRESH_CASES = ([(m, f, 1) for m in P.SPMV_MODELS for f in FRESH_FORMS] + [("cube40", "v9", 1), ("cube40", "pair", 1)] +
               [("perforated12", "small", 32), ("perforated12", "v9", 32)])        # sigma 32: the SELL-C-sigma permutation (rowof)
SCALED_CASES = [(m, f) for m in P.SPMV_MODELS for f in FRESH_FORMS] + [("perforated12", "fold"), ("star12", "fold")]
R = P.SCALED_PATH_ROUNDINGS


def _same_export(K, csr):
    """A fresh assembly of the same job exports the same bits as the cached one (the assembly is deterministic)."""
    got = K.to_csr(upper_only=False)
    return all(np.array_equal(a, b) for a, b in zip(got[:2], csr[:2])) and P.same_bits(got[2], csr[2]).all()


def _row_figures(K, csr, name, extra=0):
    """Worst row units of K.spmv over the three vectors, and whether every row keeps its bound."""
    worst, ok = {}, True
    bound = P.row_bound(csr[0], extra)
    for vn, x in P.vectors(name).items():
        ref, scale = P.cached(("rowref", name, vn), lambda: P.row_reference(*csr, x))
        u = P.row_units(K.spmv(x), ref, scale)
        worst[vn], ok = float(u.max()), ok and bool((u <= bound).all())
    return worst, ok


# ---- A and B on a fresh matrix ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,form,sigma", FRESH_CASES)
def test_fresh_matrix_is_rebuilt_bit_for_bit_from_products(gpu_ctx, name, form, sigma):
    """A, no tolerance anywhere: one sweep over the colours rebuilds every stored value from y_i / w_j bit for bit (== where a
    zero is stored), nothing lies outside the pattern, the diagonal is the CSR's -- under STAN_OPT_PACKED_COLUMNS 1 and 0.
    B on the same matrix (cube40 excepted): every row of the three vectors within min(4 x oracle, m_i + 2) units.
    Measured on the device, worst row units over the models: k_spmv_small 4.30, k_spmv (variants 0, 9 and 12 alike: the same
    sums) 7.32, k_spmv_pair 5.39, each under the spread vector (cube20 for k_spmv; the oracle: 8.89 there); standard normal at
    most 4.19, the rigid translation 2.06.  sigma 32 changes no figure: the rows keep their sums wherever they sit."""
    csr, probes = _model(gpu_ctx, name)
    K = _assemble(gpu_ctx, name, sigma)
    try:
        assert _same_export(K, csr)
        with _options(gpu_ctx, FORMS[form]):
            for packed in (1, 0):
                gpu_ctx.set_option(hip.OPT_PACKED_COLUMNS, packed)
                got, stray = probes.sweep(K.spmv)
                same = P.same_bits(got, csr[2])
                assert same.all(), "%d entries differ, the first at CSR position %d" % ((~same).sum(), int(np.argmin(same)))
                assert stray == 0
            gpu_ctx.set_option(hip.OPT_PACKED_COLUMNS, 1)
            assert P.same_bits(K.diagonal(), P.csr_diagonal(*csr)).all()
            if name != "cube40":
                worst, ok = _row_figures(K, csr, name)
                print("fresh %s %s sigma %d: worst row units %s (bound min(%.1f, m_i + 2))" %
                      (name, form, sigma, ", ".join("%s %.2f" % kv for kv in worst.items()), P.DEVICE_SPMV_UNITS))
                assert ok
        assert K.info()["scaled"] == 0
    finally:
        gpu_ctx.set_option(hip.OPT_PACKED_COLUMNS, 1)
        K.free()


# ---- A and B on the scaled matrix: packed columns, the folded copy -----------------------------------------------------------------

@pytest.mark.parametrize("name,form", SCALED_CASES)
def test_scaled_matrix_is_rebuilt_within_the_derived_bound(gpu_ctx, name, form):
    """After one cg_solve the values carry S K S and Matrix.spmv computes S^-1 (A^ (S^-1 x)).  Compared with the values exported
    BEFORE the solve, a rebuilt entry may differ by the R = 5 roundings of that path (product_ref.SCALED_PATH_ROUNDINGS:
    s_i s_j, a_ij times it, x_j / s_j, the product, y_i / s_i; the error of s itself cancels): |got - a_ij| <= (R + 2) x 2^-53
    |a_ij|, derived, not measured; zeros stay exact zeros and nothing lies outside the pattern.  B: every row within
    min(4 x oracle, m_i + 2 + R) units.  The solve in front of each sweep runs under the sweep's own options, so it builds the
    packed column stream (STAN_OPT_PACKED_COLUMNS 1: col_slots_packed of its profile is asserted positive) or leaves it unused
    (0), and the folded copy for the fold form (repacked_streams == 1: no silent fallback).
    Measured on the device: rebuilt entries off by at most 3.89 units of 2^-53 |a_ij| (bound 7) for every form; worst row units
    k_spmv_small 5.18, k_spmv 7.61, k_spmv_pair 7.15, k_spmv_fold 7.15 (bound 35.6); packed and int32 columns give the same
    figures, as the same products in the same order must; 8 (cube1) to 3 735 (cube20) slots are packed."""
    csr, probes = _model(gpu_ctx, name)
    j = P.job(name)
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**FORMS[form], hip.OPT_CG_MERIT_STOP: 0}):
            for packed in (1, 0):
                gpu_ctx.set_option(hip.OPT_PACKED_COLUMNS, packed)
                _U, rep = K.cg_solve(j.F, 1e-30, max_its=1)
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and K.info()["scaled"] == 1
                assert pr["repacked_streams"] == (1 if form == "fold" else 0)
                if form != "fold":             # (the folded copy has a packed stream of its own; the profile counts the padded one)
                    assert packed == 1 or pr["col_slots_packed"] == 0
                    assert packed == 0 or pr["col_slots_packed"] > 0
                got, stray = probes.sweep(K.spmv)
                off = np.abs(got - csr[2])
                assert stray == 0 and (off <= (R + 2) * P.U53 * np.abs(csr[2])).all()
                nz = csr[2] != 0
                worst, ok = _row_figures(K, csr, name, extra=R)
                print("scaled %s %s packed %d (%d slots packed): rebuilt entries off by at most %.2f units of 2^-53 |a_ij| (bound %d); "
                      "worst row units %s" % (name, form, packed, pr["col_slots_packed"], float((off[nz] / (P.U53 * np.abs(csr[2][nz]))).max()),
                                              R + 2, ", ".join("%s %.2f" % kv for kv in worst.items())))
                assert ok
            d, want = K.diagonal(), P.csr_diagonal(*csr)
            assert (np.abs(d - want) <= 4 * P.U53 * want).all()       # a_ii (s_i s_i) / (s_i s_i): two roundings
    finally:
        gpu_ctx.set_option(hip.OPT_PACKED_COLUMNS, 1)
        K.free()


@pytest.mark.parametrize("name", ["cube6", "perforated12"])
def test_scaled_residual_against_the_long_double_value(gpu_ctx, name):
    """Matrix.scaled_residual(F, U) for a random U against ||S (F - K U)|| / ||S F|| in long double.  The relative bar is formed
    from the row bound B_i of part B applied to the norm (product_ref.scaled_residual_reference):
      e_i = 2^-53 s_i (B_i sum_j |a_ij| |U_j| + 4 |F_i - y_i|),     bar = ||e|| / ||r|| + (N + 6) 2^-53
    (the subtraction, the two roundings of s_i, the product with it; two norms of N squares in any order and their quotient;
    the entries s_i F_i): 1.1e-13 on cube6, 6.7e-13 on perforated12.  Measured on the device: the float64 nearest to the
    long-double value on both models (off by 0)."""
    csr, _probes = _model(gpu_ctx, name)
    j = P.job(name)
    U = np.random.default_rng(5).standard_normal(j.n_red)
    ref, bar = P.scaled_residual_reference(*csr, j.F, U, P.row_bound(csr[0]))
    K = _assemble(gpu_ctx, name)
    try:
        got = K.scaled_residual(j.F, U)
    finally:
        K.free()
    print("%s: scaled_residual off by %.2e of the long-double value (bar %.2e)" % (name, abs(got / ref - 1), bar))
    assert abs(got / ref - 1) <= bar < 1e-11


# ---- C: the iterates ------------------------------------------------------------------------------------------------------------------

S60 = {**PADDED, hip.OPT_VALUE_STREAM_60: 1}
# loop form -> (options, a fresh matrix for every solve, models)
LOOPS = {
    "default": ({}, False, P.CG_MODELS),                                       # k_spmv_small, fused refresh, deferred x, folded sums
    "large_fresh": (PADDED, True, P.CG_MODELS),                                 # k_spmv<.., 9>; k_spmv_first scales the matrix on the way
    "large_scaled": (PADDED, False, P.CG_MODELS),                               # the same on the scaled matrix
    "fold": (FORMS["fold"], False, ("perforated12",)),                         # k_spmv_fold<double, 1, 1 / 2>
    "stream60": (S60, False, P.CG_MODELS),                                     # k_spmv<s60_t, 1, 9>
    "separate_reductions": ({hip.OPT_CG_FOLD_REDUCE: 0}, False, P.CG_MODELS),  # k_reduce
    "literal_refresh": ({hip.OPT_CG_FUSED_REFRESH: 0}, False, P.CG_MODELS),    # k_refresh behind a second product
    "x_in_k_step": ({hip.OPT_CG_DEFER_X: 0}, False, P.CG_MODELS),
    "single_reduction": ({hip.OPT_CG_SINGLE_REDUCE: 1}, False, P.CG_MODELS),   # k_vec_sr, DOT = 2 products
}
LOOP_CASES = [(m, f) for f, (_o, _fresh, models) in LOOPS.items() for m in models]


@pytest.mark.parametrize("name,form", LOOP_CASES)
def test_every_iterate_against_the_long_double_cg(gpu_ctx, name, form):
    """cg_solve(F, 1e-30, max_its = k), merit stop off, for every k in 1 .. 22 (refreshes at 10 and 20): termination type 5 after
    exactly k iterations, max|U - U_k| / max|U_k| and |rel_residual / ref - 1| within 4 x the oracle's figure in units of 2^-53
    (single_reduction: 4 x the float64 restatement of the Chronopoulos-Gear recurrences, which round differently).  The loop
    forms are one step away from the default each.  The large-system forms switch STAN_OPT_SPMV_SMALL and STAN_OPT_ROW_FOLDING off
    (left to itself the library folds the perforated box) and leave STAN_OPT_SPMV_VARIANT at its default, which picks variant 9
    and is what lets the loop's first product scale a fresh matrix (k_spmv_first; an explicit variant takes the scaling pass):
    large_fresh assembles a fresh matrix for every k, large_scaled and stream60 scale theirs with one solve in front; fold asserts repacked_streams == 1 and stream60 value_stream == VALUE_STREAM_60.
    Oracle (recorded): U 21.1 / 108.0, residual 35.5 / 86.5 units on cube6 / perforated12; single-reduction yardstick 54.7 /
    220.0 and 95.1 / 324.8.  Measured on the device, worst over k, U / residual units on cube6 and on perforated12:
      default, separate_reductions, x_in_k_step    9.7 / 37.5    60.9 / 98.1     (the three are the same bits)
      literal_refresh                              7.7 / 37.1    55.6 / 98.1
      large_fresh, large_scaled, stream60         11.5 / 61.6    47.4 / 78.3     (the same bits: who scales the matrix and which
      fold                                                       54.8 / 89.8      stream carries the values changes nothing)
      single_reduction                            31.6 / 77.2    65.3 / 63.6
    -- at or under the oracle's own figures, five orders under the 1e-9 bar of the loop tests."""
    opts, fresh, _models = LOOPS[form]
    j = P.job(name)
    Us, rels = _reference(gpu_ctx, name)
    sr = form == "single_reduction"
    bu = P.DEVICE_CG_FACTOR * (P.SR_CG_U_UNITS_MEASURED[name] if sr else P.ORACLE_CG_U_UNITS_MEASURED[name][0])
    br = P.DEVICE_CG_FACTOR * (P.SR_CG_RES_UNITS_MEASURED[name] if sr else P.ORACLE_CG_RES_UNITS_MEASURED[name][0])
    wu = wr = 0.0
    K = None
    try:
        with _options(gpu_ctx, {**opts, hip.OPT_CG_MERIT_STOP: 0}):
            for k in range(1, P.KMAX + 1):
                if K is None or fresh:
                    if K is not None:
                        K.free()
                    K = _assemble(gpu_ctx, name)
                    if form in ("large_scaled", "stream60"):   # scaled before the first compared solve (the 60-bit stream is encoded
                        K.cg_solve(j.F, 1e-30, max_its=1)      # from the scaled values: the scaling solve itself streams fp64)
                U, rep = K.cg_solve(j.F, 1e-30, max_its=k)
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and rep["iterations"] == k, rep
                assert K.info()["scaled"] == 1
                assert pr["repacked_streams"] == (1 if form == "fold" else 0)
                assert pr["value_stream"] == (hip.VALUE_STREAM_60 if form == "stream60" else hip.PREC_FP64)
                u, r = P.u_units(U, Us[k - 1]), P.res_units(rep["rel_residual"], rels[k - 1])
                assert u <= bu and r <= br, (k, u, r, bu, br)
                wu, wr = max(wu, u), max(wr, r)
    finally:
        if K is not None:
            K.free()
    print("cg %s %s: worst over k = 1 .. %d: U %.1f units (bound %.0f), residual %.1f units (bound %.0f)" % (name, form, P.KMAX, wu, bu, wr, br))


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_every_iterate_of_three_load_cases_in_one_loop(gpu_ctx, name):
    """cg_solve_multi with the three different load vectors of product_ref.load_cases (k_spmm and the M-column vector kernels;
    the group of two and the single column): each column against the long-double CG of ITS load vector, bounds 4 x the oracle's
    figures for that vector.  Measured on the device, U / residual units per load case: 10.3 / 16.9, 14.6 / 42.7, 40.0 / 68.0 on
    cube6; 63.0 / 94.0, 18.5 / 28.7, 184.9 / 205.8 on perforated12 (oracle: product_ref.ORACLE_CG_*_UNITS_MEASURED)."""
    j = P.job(name)
    F = P.load_cases(name)
    refs = [_reference(gpu_ctx, name, lc) for lc in range(3)]
    worst = [[0.0, 0.0] for _ in range(3)]
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {hip.OPT_CG_MERIT_STOP: 0}):
            for k in range(1, P.KMAX + 1):
                U, reps = K.cg_solve_multi(F, 1e-30, max_its=k)
                for lc in range(3):
                    assert reps[lc]["terminationtype"] == 5 and reps[lc]["iterations"] == k, reps[lc]
                    u, r = P.u_units(U[lc], refs[lc][0][k - 1]), P.res_units(reps[lc]["rel_residual"], refs[lc][1][k - 1])
                    bu = P.DEVICE_CG_FACTOR * P.ORACLE_CG_U_UNITS_MEASURED[name][lc]
                    br = P.DEVICE_CG_FACTOR * P.ORACLE_CG_RES_UNITS_MEASURED[name][lc]
                    assert u <= bu and r <= br, (k, lc, u, r, bu, br)
                    worst[lc] = [max(worst[lc][0], u), max(worst[lc][1], r)]
    finally:
        K.free()
    print("cg_solve_multi %s: worst U / residual units per load case: %s (oracle %s / %s)" %
          (name, ", ".join("%.1f / %.1f" % tuple(w) for w in worst), P.ORACLE_CG_U_UNITS_MEASURED[name], P.ORACLE_CG_RES_UNITS_MEASURED[name]))
    assert j.n_red == F.shape[1]


# ---- C on the reduced-precision value streams -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.CG_MODELS)
@pytest.mark.parametrize("stream", list(P.QUANTISE))
def test_every_iterate_of_a_reduced_precision_solve(gpu_ctx, name, stream):
    """STAN_PREC_FIXED48 / STAN_PREC_MIXED with STAN_OPT_CG_REFINE 0, k = 1 .. 12.  Every product of such a pass reads the reduced
    stream (cg.hip: cg_run::iterate multiplies with `vs`, the fused refresh at k = 10 included -- refine < 2 keeps kind_refresh =
    vs); only the fp64 check behind the pass (cg_run::fp64_check) reads the fp64 values, and what it changes is the REPORTED
    residual, so the recurrence's own is taken from the profile (rel_residual_recurrence).  Reference: the long-double CG on the
    matrix quantised here from the long-double scaled entries (rint(a^ 2^46) 2^-46; float32).  Bound: 4 x the float64 loop on
    the matrix quantised from float64 entries, which a decode error of 2^-30 in one entry of nine exceeds by orders at k = 3
    (tests/test_product_ref.py) where refinement would have healed it unseen.

    The yardstick is measured HERE, on the matrix this test exports, not taken from the recorded constants
    (product_ref.REDUCED_CG_UNITS_MEASURED, the oracle's matrix), and this is why.  With the recorded figure the first run on the
    device read, FIXED-48 on cube6 at k = 12: U 233 units (bound 511), residual 267 (bound 262).  The FIXED-48 figure is not
    rounding noise of the loop: the float64 loop on the matrix quantised from the long-double entries -- the same loop without
    the entries that fall on the other side of a quantisation boundary -- stays at 5 .. 15 units, and the 12 .. 48 entries (of
    52 k / 329 k) that do move by one quantum of 2^-46 make the rest.  WHICH entries move depends on the last bits of the
    assembled values: the oracle's matrix with every entry moved by up to 3 ulps, as another summation order in the assembly
    moves them, reads U 128 / 261 / 262 / 296 and residual 65 / 40 / 105 / 242 on cube6 (four realisations), 71 .. 144 and 6 ..
    83 on perforated12.  The device assembles its own realisation (1e-13 from the oracle's), so a constant recorded on the
    oracle's matrix is no yardstick for it; the float64 loop on the exported matrix itself, whose quantised entries are the
    device's own (k_scale_matrix and k_to_fx48 restated), is.  The recorded constants stay what tests/test_product_ref.py holds
    the oracle's matrix to.  Measured on the device, U / recurrence residual units (yardstick on the same matrix): FIXED-48
    233.0 / 267.1 (233.0 / 265.2) on cube6, 171.6 / 55.2 (169.7 / 47.5) on perforated12 -- the device follows the restated
    quantisation to two units; float32 8.7 / 3.3 (9.7 / 14.1) and 7.7 / 7.2 (7.4 / 6.9)."""
    j = P.job(name)
    csr, _probes = _model(gpu_ctx, name)
    Us, rels = reduced_reference(gpu_ctx, name, stream)
    mode = {"fixed48": hip.PREC_FIXED48, "mixed": hip.PREC_MIXED}[stream]
    its = P.cg_iterates(P.Scaled(*csr, T=np.float64, quantise=P.QUANTISE[stream]), j.F, P.KMAX_REDUCED)
    yu = max(P.u_units(x, Us[k]) for k, (x, _r) in enumerate(its))
    yr = max(P.res_units(r, rels[k]) for k, (_x, r) in enumerate(its))
    bu, br = P.DEVICE_CG_FACTOR * yu, P.DEVICE_CG_FACTOR * yr
    worst, over = [0.0, 0.0], []
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 0}):
            for k in range(1, P.KMAX_REDUCED + 1):
                U, rep = K.cg_solve(j.F, 1e-30, max_its=k, precision_mode=mode)
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and rep["iterations"] == k and pr["refine_passes"] == 1, (rep, pr["refine_passes"])
                assert pr["value_stream"] == mode and pr["fp64_products"] == 1
                u, r = P.u_units(U, Us[k - 1]), P.res_units(pr["rel_residual_recurrence"], rels[k - 1])
                worst = [max(worst[0], u), max(worst[1], r)]
                if u > bu or r > br:
                    over.append((k, u, r))
    finally:
        K.free()
    print("cg %s %s: worst over k = 1 .. %d: U %.1f units (yardstick on this matrix %.1f, on the oracle's %.1f), recurrence residual "
          "%.1f units (yardstick %.1f, on the oracle's %.1f)" % ((name, stream, P.KMAX_REDUCED, worst[0], yu, P.REDUCED_CG_UNITS_MEASURED[stream, name][0],
                                                                 worst[1], yr, P.REDUCED_CG_UNITS_MEASURED[stream, name][1])))
    assert not over, over
