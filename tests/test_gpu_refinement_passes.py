"""The refinement passes of a reduced-precision solve (stan_cg_device, stan_amd/csrc/cg.hip): the fp64 check behind a pass,
r_t = b^ - A^64 x; k_accumulate, x = x_1 + d_2 + ...; the next pass on r_t with eps_pass = eps_f / rel64; the max_its budget carried
across the passes.  The other tests look at end results only.

Here the first pass is taken as the device delivers it: n1, its length, is the largest max_its whose solve still reports one pass
(a solve stopped at max_its = n1 ends with type 5 -- out of iterations -- where the recurrence has just converged, and returns
U_1), and the recurrence's own residual must be at or below eps_f there and above it one iteration earlier.  n1 is printed next
to the float64 stand-in's and NOT asserted equal to it: the stand-in's stop is 3 % from eps_f on perforated12 (15 % on cube6),
but after 322 iterations the order of the loop's sums alone moves its residual there by 5 % and long double stops two iterations
earlier (tests/test_product_ref.py measures both) -- the device read 322 with k_spmv_small and 323 with k_spmv on perforated12,
112 on cube6 in both forms.  What follows does not depend on the history.  Then U(max_its = n1 + k) - U_1, k = 1 .. 12, is held to S d_k: the long-double CG iterate on the
float32-quantised matrix with the right-hand side r_t = b^ - A^64 (U_1 / s) formed in long double FROM THE DEVICE'S U_1
(product_ref.refinement_pass), in units of 2^-53 max|S d_k|, within 4 x the float64 restatement of the same construction on the
exported matrix.  A pass that forms r_t with the reduced values, one that iterates on the fp64 matrix and a dropped
k_accumulate each exceed that (tests/test_product_ref.py).  Nothing is fitted to the device; each test prints what it saw."""
import numpy as np
import pytest

from stan_amd import hip
from tests import product_ref as P
from tests.gpu_models import PADDED, assemble as _assemble, model as _model, options as _options

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "padded": PADDED}            # k_spmv_small / k_spmv on the padded streams
CASES = [(m, f) for m in P.CG_MODELS for f in FORMS]
R = P.SCALED_PATH_ROUNDINGS


def _reported_residual_is_the_true_one(csr, F, U, rep, label):
    """rel_residual of a reduced-precision solve is the fp64 check's ||b^ - A^64 x|| / ||b^||: against ||S (F - K U)|| / ||S F|| of
    the RETURNED U in long double, within the bar of product_ref.scaled_residual_reference (rows of the scaled matrix: the
    row bound with the R = 5 roundings of the scaled path).  Returns the long-double value."""
    ref, bar = P.scaled_residual_reference(*csr, F, U, P.row_bound(csr[0], extra=R))
    off = abs(rep["rel_residual"] / ref - 1)
    print("%s: reported residual %.6e, long double %.6e, off by %.2e (bar %.2e)" % (label, rep["rel_residual"], ref, off, bar))
    assert off <= bar, (label, off, bar)
    return ref


def _first_pass_length(ctx, K, F, eps, mode, guess, total):
    """The largest max_its whose solve still reports refine_passes == 1 (the profile does not tell the passes' iterations
    apart): the stand-in's n1 is probed first, then bisection."""
    def passes(m):
        K.cg_solve(F, eps, max_its=m, precision_mode=mode)
        return ctx.profile()["refine_passes"]
    if 1 <= guess < total and passes(guess) == 1 and passes(guess + 1) == 2:
        return guess
    lo, hi = 1, total                       # passes(lo) == 1 (one iteration cannot converge), passes(total) >= 2
    assert passes(lo) == 1 and passes(hi) >= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if passes(mid) == 1 else (lo, mid)
    return lo


@pytest.mark.parametrize("name,form", CASES)
def test_second_pass_of_a_float32_solve_from_the_observed_iterate(gpu_ctx, name, form):
    """STAN_PREC_MIXED, STAN_OPT_CG_REFINE 1, eps_f = 1e-10, merit stop off.
    1  The unbounded solve: type 1, at least two passes, the reported residual the long-double one of the returned U and <=
       eps_f.  n1 from it (see above); the solves at max_its = n1 - 1 and n1: type 5, one pass, the recurrence's residual above
       eps_f and at or below it; the second returns U_1.
    2  max_its = n1 + k, k = 1 .. 12: type 5 after n1 + k iterations in two passes (the budget is carried across: the second
       pass gets max_its - n1), the reported residual the long-double one of the returned U, and U - U_1 within 4 x the
       float64 restatement of S d_k (worst over k, measured here).
    Oracle's matrix: n1 = 112 / 322 on cube6 / perforated12, rel64 behind the first pass 1.0e-6 / 5.1e-6, max|S d_k| / max|U_1|
    3e-8 .. 6e-7, yardstick 2.2e8 / 9.9e7 units (the cancellation in r_t: rel64 of 1e-6 leaves 2^-53 / 1e-6 of it).
    Measured on the device: n1 = 112 / 112 (cube6, default / padded; 173 iterations in all) and 322 / 323 (perforated12; 541 /
    542), the recurrence's residual over eps_f at n1 - 1 and n1 1.153, 0.756 on cube6 and 1.113, 0.953 / 1.002, 0.848 on
    perforated12; U - U_1 over k = 1 .. 12: 6.8e7 .. 1.09e8 (yardstick 1.53e8) and 7.3e7 .. 1.35e8 (1.26e8) on cube6, 6.2e7 ..
    8.8e7 (1.20e8) and 6.2e7 .. 9.5e7 (9.1e7) on perforated12; the reported residual within 5e-9 of the long-double one
    (bars 8e-7 .. 9e-6) behind U_1 and every k, within 1.5e-5 (bar 1e-2 .. 4e-2) at the end."""
    j = P.job(name)
    csr, _probes = _model(gpu_ctx, name)
    q, eps, mode = P.QUANTISE["mixed"], P.REFINE_EPS, hip.PREC_MIXED
    n1_cpu = P.cached(("gpu", "first pass", name), lambda: P.first_pass_f64(csr, j.F, eps, q)[0])
    label = "refinement %s %s" % (name, form)
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**FORMS[form], hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 1}):
            U, rep = K.cg_solve(j.F, eps, precision_mode=mode)
            pr = gpu_ctx.profile()
            assert rep["terminationtype"] == 1 and pr["refine_passes"] >= 2 and pr["value_stream"] == mode, (rep, pr["refine_passes"])
            assert _reported_residual_is_the_true_one(csr, j.F, U, rep, label + " unbounded") <= eps
            total, total_passes = rep["iterations"], pr["refine_passes"]
            n1 = _first_pass_length(gpu_ctx, K, j.F, eps, mode, n1_cpu, total)
            print("%s: the unbounded solve takes %d iterations in %d passes; first pass %d (float64 stand-in: %d)" % (label, total, total_passes, n1, n1_cpu))
            _U, rep = K.cg_solve(j.F, eps, max_its=n1 - 1, precision_mode=mode)
            before = gpu_ctx.profile()["rel_residual_recurrence"]
            assert rep["terminationtype"] == 5 and rep["iterations"] == n1 - 1 and gpu_ctx.profile()["refine_passes"] == 1, rep
            U1, rep = K.cg_solve(j.F, eps, max_its=n1, precision_mode=mode)
            at = gpu_ctx.profile()["rel_residual_recurrence"]
            assert rep["terminationtype"] == 5 and rep["iterations"] == n1 and gpu_ctx.profile()["refine_passes"] == 1, rep
            print("%s: the recurrence's residual over eps_f at n1 - 1 / n1: %.3f / %.3f" % (label, before / eps, at / eps))
            assert at <= eps < before                # the first pass ends where ITS OWN recurrence says, no tolerance
            rel64 = _reported_residual_is_the_true_one(csr, j.F, U1, rep, label + " U_1")
            assert rel64 > eps
            ref, _rt = P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q)
            f64, _rt = P.refinement_pass(csr, j.F, U1, P.REFINE_KMAX, q, T=np.float64)
            yard = max(P.step_units(P.added_f64(U1, d), ref[k]) for k, d in enumerate(f64))
            seen, over = [], []
            for k in range(1, P.REFINE_KMAX + 1):
                U, rep = K.cg_solve(j.F, eps, max_its=n1 + k, precision_mode=mode)
                assert rep["terminationtype"] == 5 and rep["iterations"] == n1 + k and gpu_ctx.profile()["refine_passes"] == 2, (k, rep)
                _reported_residual_is_the_true_one(csr, j.F, U, rep, label + " k = %d" % k)
                u = P.step_units(U - U1, ref[k - 1])
                seen.append(u)
                if u > P.DEVICE_CG_FACTOR * yard:
                    over.append((k, u))
    finally:
        K.free()
    print("%s: U - U_1 against S d_k, k = 1 .. %d: %s units of 2^-53 max|S d_k| (yardstick %.3g); max|S d_k| / max|U_1| %.2e .. %.2e" %
          (label, P.REFINE_KMAX, " ".join("%.3g" % u for u in seen), yard, float(abs(ref[0]).max() / abs(U1).max()),
           float(abs(ref[-1]).max() / abs(U1).max())))
    assert not over, (over, P.DEVICE_CG_FACTOR * yard)


@pytest.mark.parametrize("name,form", CASES)
def test_fixed48_solve_refines_in_two_passes(gpu_ctx, name, form):
    """STAN_PREC_FIXED48 at eps_f = 1e-12, where the float64 restatement of the driver (product_ref.refine_driver_f64, on the
    exported matrix) takes exactly two passes with every stop decision a factor 1.01 from its threshold -- asserted here on the
    exported matrix, as tests/test_product_ref.py asserts it on the oracle's: the device takes two passes, ends with type 1, and
    reports the long-double residual of the U it returns, which is <= eps_f.  No iterate of the second pass is compared: rel64
    behind the first pass is 2e-12 and max|S d| / max|U_1| 4e-14, a few hundred units of 2^-53 of U_1 -- the step is rounding
    noise of the iterate it is added to.  Measured on the device: 125 / 126 iterations on cube6 (default / padded; stand-in 123 +
    2), 416 / 416 on perforated12 (356 + 60), two passes each, reported residual 8.1e-13 .. 9.6e-13, within 8e-4 of the long-double
    one -- whose bar at such a residual is 1 .. 4: the row sums' rounding is as large as what is left of F - K U."""
    j = P.job(name)
    csr, _probes = _model(gpu_ctx, name)
    eps = P.REFINE_EPS_FIXED48
    passes = P.cached(("gpu", "fixed48 driver", name), lambda: P.refine_driver_f64(csr, j.F, eps, P.QUANTISE["fixed48"]))
    assert P.two_passes_clear_of_thresholds(passes), [(p["its"], p["stop"], p["before"], p["check"]) for p in passes]
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**FORMS[form], hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 1}):
            U, rep = K.cg_solve(j.F, eps, precision_mode=hip.PREC_FIXED48)
            pr = gpu_ctx.profile()
    finally:
        K.free()
    print("refinement %s %s fixed48: %d iterations in %d passes (float64 stand-in: %s)" %
          (name, form, rep["iterations"], pr["refine_passes"], " + ".join(str(p["its"]) for p in passes)))
    assert rep["terminationtype"] == 1 and pr["refine_passes"] == 2 and pr["value_stream"] == hip.PREC_FIXED48, (rep, pr["refine_passes"])
    assert pr["fp64_products"] == 2
    assert _reported_residual_is_the_true_one(csr, j.F, U, rep, "refinement %s %s fixed48" % (name, form)) <= eps
