"""The restart of the CG loop every n_red iterations (lincg's ItsBeforeRestart = N): beta stays 0 when k % its_before_restart == 0
in k_update, k_update<.., RING> and k_update_m, and in the iteration behind it, (k - 1) % its_before_restart == 0, in k_vec_sr
(stan_amd/csrc/cg_vector_kernels.inc, cg_multi.inc; the oracle: stan_oracle_cg_opt).  No other test runs a loop through k = n_red
and looks at what came out.

A replay of the whole loop cannot test it: where the loop is well conditioned the recurrence has converged by n_red, where it
is not float64 and long double are ten orders apart by then.  So the instrument takes the iterate the DEVICE returned at max_its
= k, U_k, and predicts the next one from it in long double (product_ref.one_step): with STAN_OPT_CG_RUPDATE 6 the iteration k =
n_red (12 = 2 x 6 on cube1s, 54 = 9 x 6 on cube2s) is a refresh iteration too, r_k = b^ - A^ x_k, and the restart makes
p_{k+1} = r_k, so U_{k+1} - U_k = S (alpha r) with alpha = r.r / r.A^ r -- whatever happened before.  The models are the stretched
cubes of product_ref (aspect 900), on which the true residual at k = n_red is 1e-2 and the step 1e-6 .. 1e-5 of max|U|.

d = U(max_its = k + 1) - U(max_its = k) is held to max|d - d_ref| <= 4 x max(yardstick, floor) in units of 2^-53 max|d_ref|:
the yardstick is the float64 one_step through fl(U_k + .) - U_k, the floor max|U_k| / max|d_ref| -- one rounding of the iterates
the difference is taken from.  A loop WITHOUT the restart misses that by ten orders (tests/test_product_ref.py: 1e16 .. 1e17 units
against 1e5 .. 1e6).  Nothing is fitted to the device; each test prints what it saw."""
import numpy as np
import pytest

from stan_amd import hip
from tests import product_ref as P
from tests.gpu_models import PADDED, assemble as _assemble, model as _model, options as _options

pytestmark = pytest.mark.gpu

BASE = {hip.OPT_CG_RUPDATE: P.RESTART_RUPDATE, hip.OPT_CG_MERIT_STOP: 0}
# form -> (options on top of BASE, value stream)
FORMS = {
    "default": ({}, None),                                           # k_update<.., false> with the deferred x
    "padded": (PADDED, None),                                        # the same behind the large-system products
    "x_ring": ({**PADDED, hip.OPT_CG_X_RING: 1}, None),              # k_update<.., true>: the restart inside a ring window (W = 6)
    "x_in_k_step": ({hip.OPT_CG_DEFER_X: 0}, None),
    "literal_refresh": ({hip.OPT_CG_FUSED_REFRESH: 0}, None),        # r_k from k_refresh
    "mixed": ({hip.OPT_CG_REFINE: 0}, "mixed"),                      # the instrument on the quantised matrix
    "fixed48": ({hip.OPT_CG_REFINE: 0}, "fixed48"),
    "single_reduction": ({hip.OPT_CG_SINGLE_REDUCE: 1}, None),       # k_vec_sr
}
MODE = {None: hip.PREC_FP64, "mixed": hip.PREC_MIXED, "fixed48": hip.PREC_FIXED48}


def _held(csr, F, U_k, U_next, quantise, label):
    """Prints the figures of one step and says whether it keeps its bound; asserts the condition the instrument stands on."""
    d_ref, true_res = P.one_step(csr, F, U_k, quantise=quantise)
    yard = P.step_units(P.added_f64(U_k, P.one_step(csr, F, U_k, quantise=quantise, T=np.float64)[0]), d_ref)
    floor = P.step_floor(U_k, d_ref)
    got = P.step_units(U_next - U_k, d_ref)
    print("%s: %.3g units of 2^-53 max|d_ref| (yardstick %.3g, floor %.3g); true residual at U_k %.2e, max|d| / max|U| %.2e" %
          (label, got, yard, floor, float(true_res), float(abs(d_ref).max() / abs(U_k).max())))
    assert float(true_res) > 1e-4, "the step is noise"
    return got <= P.DEVICE_CG_FACTOR * max(yard, floor)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,mult", P.RESTART_CASES)
def test_the_step_behind_the_restart(gpu_ctx, name, mult, form):
    """cg_solve(F, 1e-30) at max_its = k and k + 1 with k = n_red (cube2s: 2 n_red as well) under STAN_OPT_CG_RUPDATE 6, merit stop
    off: termination type 5 at both counts, the true residual at U_k above 1e-4 in long double, and the step between the two
    within 4 x max(yardstick, floor) of the long-double step from U_k.  The reduced streams run under STAN_OPT_CG_REFINE 0, their
    refresh at k reads the reduced values, and the instrument runs on the matrix quantised as the stream quantises it.
    single_reduction: k_vec_sr of iteration k (a refresh iteration) forms x_k and leaves r to k_refresh, r = b^ - A^ x_k; the
    kernel of iteration k + 1 finds (k + 1 - 1) % n_red == 0 and takes beta = 0, p = r, p.Ap = delta = r.A^ r, alpha = gamma /
    delta: the same step, held to the same instrument.  x_ring asserts the window 6 of the ring: k = n_red falls on a flush.
    Oracle's matrix (yardstick, floor): cube1s 1.89e5, 5.93e5; cube2s 1.94e5, 8.38e4 at k = 54 and 1.58e7, 1.25e7 at k = 108.
    Measured on the device, units (yardstick, floor of the same U_k) at k = 12 on cube1s, k = 54 and k = 108 on cube2s:
      default, x_in_k_step (the same bits)   8.09e5 (3.36e5, 6.71e5)   2.99e5 (2.16e5, 8.36e4)   7.56e6 (7.46e6, 4.81e6)
      padded, x_ring (the same bits)         2.15e5 (1.59e5, 5.20e5)   1.32e5 (1.86e5, 6.92e4)   3.02e7 (1.58e7, 9.85e6)
      literal_refresh                        5.35e5 (6.06e5, 6.69e5)   1.86e5 (9.13e4, 4.80e4)   3.46e7 (1.44e7, 7.85e6)
      mixed                                  4.74e6 (4.50e6, 3.95e6)   1.04e5 (6.89e4, 1.22e5)   3.02e7 (3.68e7, 1.13e7)
      fixed48                                2.87e6 (1.01e6, 1.57e6)   1.80e5 (1.26e5, 7.82e4)   1.75e7 (1.67e7, 1.16e7)
      single_reduction                       3.34e6 (1.40e7, 1.01e7)   9.59e4 (1.07e5, 2.71e4)   2.65e7 (2.10e7, 1.14e7)
    -- 0.2 .. 2.4 of max(yardstick, floor), true residuals 2.7e-4 .. 3.7e-2; without the restart: 1e15 .. 1e17 units."""
    opts, stream = FORMS[form]
    j = P.job(name)
    csr, _probes = _model(gpu_ctx, name)
    k = mult * j.n_red
    assert j.n_red == {"cube1s": 12, "cube2s": 54}[name] and k % P.RESTART_RUPDATE == 0
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**BASE, **opts}):
            got = []
            for its in (k, k + 1):
                U, rep = K.cg_solve(j.F, 1e-30, max_its=its, precision_mode=MODE[stream])
                assert rep["terminationtype"] == 5 and rep["iterations"] == its, rep
                assert gpu_ctx.profile()["value_stream"] == MODE[stream]
                if form == "x_ring":
                    assert gpu_ctx.cg_x_ring_info()[0] == P.RESTART_RUPDATE
                got.append(U)
    finally:
        K.free()
    assert _held(csr, j.F, got[0], got[1], P.QUANTISE.get(stream), "restart %s %s k = %d" % (name, form, k))


@pytest.mark.parametrize("name,mult", P.RESTART_CASES)
def test_the_step_behind_the_restart_of_three_load_cases(gpu_ctx, name, mult):
    """cg_solve_multi with the three load vectors of product_ref.load_cases (k_update_m; its refresh is the literal second
    product): every column held to the step from ITS OWN U_k.  Measured on the device, per load case, units (yardstick, floor):
    cube1s 1.34e5 (7.68e5, 5.21e5), 2.34e5 (2.34e5, 2.37e5), 3.78e4 (2.61e4, 4.14e4); cube2s at k = 54 2.39e5 (9.97e4, 6.61e4),
    1.40e5 (1.58e5, 497), 6.07e4 (5.00e4, 1.55e4), at k = 108 1.77e7 (3.95e7, 1.04e7), 5.89e5 (1.02e6, 2.49e5), 2.59e7 (2.59e7,
    5.97e6)."""
    j = P.job(name)
    csr, _probes = _model(gpu_ctx, name)
    F = P.load_cases(name)
    k = mult * j.n_red
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, BASE):
            got = []
            for its in (k, k + 1):
                U, reps = K.cg_solve_multi(F, 1e-30, max_its=its)
                assert all(r["terminationtype"] == 5 and r["iterations"] == its for r in reps), reps
                got.append(U)
    finally:
        K.free()
    held = [_held(csr, F[lc], got[0][lc], got[1][lc], None, "restart %s multi load case %d k = %d" % (name, lc, k)) for lc in range(3)]
    assert all(held), held
