"""The reduced-precision value streams (STAN_PREC_FIXED48, STAN_PREC_MIXED) in EVERY product and loop form, iterate by iterate.

tests/test_gpu_product_precision.py holds the fp64 stream to a long-double CG in nine forms and the reduced streams in one, the
default: k_spmv_small<float | uint32_t, 1> and k_spmv2.  launch_product (stan_amd/csrc/cg.hip) instantiates for the two reduced
value types also k_spmv<VT, 0 | 1 | 2, 0 | 9 | 12>, k_spmv_pair<VT, DOT, true>, k_spmv_fold<VT, DOT, 1> and k_spmv_fold<VT, 1, 2>:
what runs above 150 000 block rows, the only sizes the reduced streams exist for.  Their other checks are refined solves to
1e-6 .. 1e-9, which a decode error of 2^-30 passes at the price of a few refinement passes (tests/test_product_ref.py).

Here: the table FORMS below, both streams, with the reference, the yardstick and the bound of
test_every_iterate_of_a_reduced_precision_solve unchanged -- the long-double CG on the matrix quantised from the long-double
scaled entries; the float64 loop on the EXPORTED matrix quantised from float64 entries, measured in the test; 4 x that -- under
STAN_OPT_CG_REFINE 0 and STAN_OPT_CG_MERIT_STOP 0 for k = 1 .. 12, U from the solve and the residual from the profile
(rel_residual_recurrence).  And STAN_OPT_CG_REFINE 2, whose refresh on the fp64 values comes at iteration 50, at k = 48 .. 52.

No bound is fitted to the device; each test prints the worst figure it saw."""
import numpy as np
import pytest

from stan_amd import hip
from tests import product_ref as P
from tests.gpu_models import LARGE, PADDED, assemble as _assemble, model as _model, options as _options, reduced_reference

pytestmark = pytest.mark.gpu

MODE = {"fixed48": hip.PREC_FIXED48, "mixed": hip.PREC_MIXED}
ALL = P.CG_MODELS
# form -> (options, models, SELL sigma of the assembly, single reduction).  Each is one step away from PADDED (STAN_OPT_SPMV_SMALL 0
# and STAN_OPT_ROW_FOLDING 0: k_spmv on the padded streams) unless it says otherwise.  What launch_product makes of it, VT = uint32_t
# (FIXED-48) / float (float32), V = the stream's own variant (product_plan::var: 12 for FIXED-48, 9 for float32); every loop's
# refresh at k = 10 is the fused two-product pass k_spmv2<VT> (k_spmv_fold<VT, 1, 2> on the folded copy) unless stated:
FORMS = {
    "small": ({}, ALL, 1, False),                                                       # k_spmv_small<VT, 1> (the neighbour's case)
    "wave_auto": (PADDED, ALL, 1, False),                                               # k_spmv<VT, 1, 12> / k_spmv<VT, 1, 9>
    "v0": ({**PADDED, hip.OPT_SPMV_VARIANT: 0}, ALL, 1, False),                         # k_spmv<VT, 1, 0>
    "v9": ({**PADDED, hip.OPT_SPMV_VARIANT: 9}, ALL, 1, False),                         # k_spmv<VT, 1, 9>
    "v12": ({**PADDED, hip.OPT_SPMV_VARIANT: 12}, ALL, 1, False),                       # k_spmv<VT, 1, 12>
    "pair": ({**PADDED, hip.OPT_SPMV_VARIANT: 20}, ALL, 1, False),                      # k_spmv_pair<VT, 1, true>
    "fold": ({**LARGE, hip.OPT_ROW_FOLDING: 1}, ("perforated12", "star12"), 1, False),  # k_spmv_fold<VT, 1, 1>, <VT, 1, 2> at k = 10
    "int32_columns": ({**PADDED, hip.OPT_PACKED_COLUMNS: 0}, ALL, 1, False),            # the unpacked walk of k_spmv<VT, 1, V>
    "sigma32": (PADDED, ("perforated12",), 32, False),                                  # the rowof permutation
    "literal_refresh": ({**PADDED, hip.OPT_CG_FUSED_REFRESH: 0}, ALL, 1, False),        # k_spmv<VT, 0, V> behind k_refresh at k = 10
    "separate_reductions": ({**PADDED, hip.OPT_CG_FOLD_REDUCE: 0}, ALL, 1, False),      # k_reduce forms every sum
    "x_in_k_step": ({**PADDED, hip.OPT_CG_DEFER_X: 0}, ALL, 1, False),
    "single_reduction_small": ({hip.OPT_CG_SINGLE_REDUCE: 1}, ALL, 1, True),            # k_spmv_small<VT, 2>, <VT, 0> at k = 10
    "single_reduction": ({**PADDED, hip.OPT_CG_SINGLE_REDUCE: 1}, ALL, 1, True),        # k_spmv<VT, 2, V>, <VT, 0, V> at k = 10
}
CASES = [(s, m, f) for f, (_o, models, _sigma, _sr) in FORMS.items() for m in models for s in P.QUANTISE]
# the same products in the same order: another variant of k_spmv only changes how the stream is fetched and which workgroup takes
# which slices, the int32 columns name the same blocks
SAME_BITS = ("wave_auto", "v0", "v9", "v12", "int32_columns")


def _yardstick(ctx, name, stream, sr):
    """(U units, recurrence-residual units) of the float64 loop -- the Chronopoulos-Gear restatement for the single-reduction
    forms -- on the exported matrix quantised from float64 entries, worst over k = 1 .. 12: once per pytest run."""
    def make():
        csr, _probes = _model(ctx, name)
        Us, rels = reduced_reference(ctx, name, stream)
        q = P.QUANTISE[stream]
        its = (P.cg_single_reduce_f64(csr, P.job(name).F, P.KMAX_REDUCED, quantise=q) if sr else
               P.cg_iterates(P.Scaled(*csr, T=np.float64, quantise=q), P.job(name).F, P.KMAX_REDUCED))
        return (max(P.u_units(x, Us[k]) for k, (x, _r) in enumerate(its)), max(P.res_units(r, rels[k]) for k, (_x, r) in enumerate(its)))
    return P.cached(("gpu", "reduced yardstick", name, stream, sr), make)


def _check_profile(pr, form, mode):
    assert pr["refine_passes"] == 1 and pr["fp64_products"] == 1 and pr["value_stream"] == mode, pr
    assert pr["repacked_streams"] == (1 if form == "fold" else 0)
    if form == "int32_columns":
        assert pr["col_slots_packed"] == 0
    elif form != "fold":                 # (the folded copy has a packed stream of its own; the profile counts the padded one)
        assert pr["col_slots_packed"] > 0


@pytest.mark.parametrize("stream,name,form", CASES)
def test_every_iterate_of_a_reduced_precision_solve_in_every_form(gpu_ctx, stream, name, form):
    """cg_solve(F, 1e-30, max_its = k, precision_mode) for k = 1 .. 12 under the options of FORMS[form]: termination type 5 after
    exactly k iterations, one pass, one fp64 product (the check behind the pass), value_stream the stream asked for; U and the
    recurrence's residual within 4 x the float64 loop on the exported matrix.  The packed forms assert col_slots_packed > 0,
    int32_columns == 0, fold repacked_streams == 1 (no silent fallback to the padded streams).

    The rows were read against plan_products / launch_product, and two needed a remark rather than a correction:
    every explicit STAN_OPT_SPMV_VARIANT keeps the pair and wave forms away from k_spmv_small whatever STAN_OPT_SPMV_SMALL says
    (plan_products: SMALL needs v < 0), and the single-reduction loop's refresh at k = 10 is a literal product k_spmv<VT, 0, V> /
    k_spmv_small<VT, 0> behind k_refresh, so those two rows reach DOT = 0 as well as DOT = 2.
    Measured on the device, worst over k, U / recurrence-residual units (yardstick on the same matrix), cube6 and perforated12:
      FIXED-48  yardstick 233.0 / 265.2 and 169.7 / 47.5 (single reduction: 264.0 / 325.6 and 179.2 / 111.8)
        small, fold (perforated12)                       233.0 / 267.1    171.6 / 55.2
        wave_auto, v0, v9, v12, int32_columns,
        separate_reductions, x_in_k_step                 233.0 / 270.9    172.1 / 50.6     (the same bits)
        pair 223.5 / 267.1 and 172.1 / 55.2; literal_refresh 235.4 / 270.9 and 172.1 / 53.7; sigma32 170.6 / 55.2
        single_reduction_small 281.8 / 355.8 and 171.1 / 24.6; single_reduction 272.3 / 376.5 and 169.7 / 50.6
      float32   yardstick 9.7 / 14.1 and 7.4 / 6.9 (single reduction: 34.3 / 49.6 and 31.8 / 8.8)
        small 8.7 / 3.3 and 7.7 / 7.2; the wave forms 5.2 / 3.7 and 5.5 / 2.9; pair 11.0 / 6.7 and 5.0 / 4.3; fold 6.6 / 4.6;
        literal_refresh 5.8 / 3.7 and 5.6 / 3.2; sigma32 5.3 / 5.7
        single_reduction_small 32.4 / 37.2 and 24.9 / 25.1; single_reduction 26.1 / 34.9 and 14.0 / 10.2
      star12, fold: FIXED-48 178.2 / 52.8 (yardstick 89.7 / 57.8), float32 84.7 / 5.4 (149.6 / 21.2)
    -- every stream follows its restated quantisation to the rounding of the loop in every form."""
    opts, _models, sigma, sr = FORMS[form]
    j = P.job(name)
    Us, rels = reduced_reference(gpu_ctx, name, stream)
    yu, yr = _yardstick(gpu_ctx, name, stream, sr)
    bu, br = P.DEVICE_CG_FACTOR * yu, P.DEVICE_CG_FACTOR * yr
    worst, over = [0.0, 0.0], []
    K = _assemble(gpu_ctx, name, sigma)
    try:
        with _options(gpu_ctx, {**opts, hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 0}):
            for k in range(1, P.KMAX_REDUCED + 1):
                U, rep = K.cg_solve(j.F, 1e-30, max_its=k, precision_mode=MODE[stream])
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and rep["iterations"] == k, rep
                _check_profile(pr, form, MODE[stream])
                u, r = P.u_units(U, Us[k - 1]), P.res_units(pr["rel_residual_recurrence"], rels[k - 1])
                worst = [max(worst[0], u), max(worst[1], r)]
                if u > bu or r > br:
                    over.append((k, u, r))
    finally:
        K.free()
    print("cg %s %s %s: worst over k = 1 .. %d: U %.1f units (yardstick %.1f), recurrence residual %.1f units (yardstick %.1f)" %
          (name, stream, form, P.KMAX_REDUCED, worst[0], yu, worst[1], yr))
    assert not over, (over, bu, br)


@pytest.mark.parametrize("name", P.CG_MODELS)
@pytest.mark.parametrize("stream", list(P.QUANTISE))
def test_variants_and_column_streams_give_the_same_bits(gpu_ctx, stream, name):
    """k_spmv<VT, 1, 0 | 9 | 12> and the packed and int32 column walks form the same sums in the same order: the same U and the
    same recurrence residual, bit for bit, at k = 3, at the refresh (10) and behind it (12).  No tolerance.  (Variants 9 and 12
    deal the workgroups of every full window of 256 to the XCDs in chunks, which would reorder the partial sums; these models
    launch 5 and 30 workgroups, the ragged tail that keeps the identity mapping.)"""
    j = P.job(name)
    seen = {}
    for form in SAME_BITS:
        K = _assemble(gpu_ctx, name)
        try:
            with _options(gpu_ctx, {**FORMS[form][0], hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 0}):
                for k in (3, 10, 12):
                    U, rep = K.cg_solve(j.F, 1e-30, max_its=k, precision_mode=MODE[stream])
                    pr = gpu_ctx.profile()
                    assert rep["terminationtype"] == 5 and rep["iterations"] == k and pr["value_stream"] == MODE[stream]
                    seen[form, k] = (U.tobytes(), float(pr["rel_residual_recurrence"]).hex())
        finally:
            K.free()
    differ = [(form, k) for (form, k), v in seen.items() if v != seen[SAME_BITS[0], k]]
    assert not differ, differ


# ---- STAN_OPT_CG_REFINE 2 ---------------------------------------------------------------------------------------------------------------

def _refine2_loops(ctx, name, stream):
    """(reference, yardstick) iterates 1 .. 52: the loop on the quantised matrix with no refresh before iteration 50 and
    r = b^ - A^64 x there, in long double and in float64 on the exported matrix."""
    def make():
        csr, _probes = _model(ctx, name)
        q, F = P.QUANTISE[stream], P.job(name).F
        ref = P.cg_iterates(P.Scaled(*csr, T=P.LD, quantise=q), F, 52, rupdate=50, refresh_with=P.Scaled(*csr, T=P.LD).mv)
        yard = P.cg_iterates(P.Scaled(*csr, T=np.float64, quantise=q), F, 52, rupdate=50, refresh_with=P.Scaled(*csr, T=np.float64).mv)
        return ref, yard
    return P.cached(("gpu", "refine2", name, stream), make)


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_refine2_refreshes_on_the_fp64_values_at_iteration_50(gpu_ctx, name):
    """STAN_OPT_CG_REFINE 2, STAN_PREC_MIXED, the padded streams: cg_run::iterate replaces the fused refresh by a literal product
    on the FP64 values every REFRESH64 = 50 iterations and refreshes nowhere else.  Five solves, max_its = 48 .. 52, against the
    long-double loop that does exactly that; bound 4 x the float64 restatement on the exported matrix, in U and in the
    recurrence's residual (tests/test_product_ref.py: a refresh on the reduced values is over the bound by four orders in U at
    k = 51 and 52, and by more in the residual from k = 50).  fp64_products counts the check behind the pass, plus the refresh
    from k = 50 on -- which it did not before this test: the count took in the refresh launches the host had enqueued past the
    stop (cg_run::fp64_check drained every span; now those of iterations that ran), and read 2 at k = 48.
    Oracle's matrix: yardstick U 4 590 / 79 000 units, residual 96 600 / 50.4 on cube6 / perforated12.  Measured on the device,
    k = 48 .. 52: U 587 .. 2 750 (bound 9 390) and 14 800 .. 120 000 (278 000), residual 229 .. 53 000 (262 000) and 9.9 .. 57.9
    (222): the refresh at 50 is the fp64 one."""
    j = P.job(name)
    ref, yard = _refine2_loops(gpu_ctx, name, "mixed")
    ks = P.REFINE2_KS
    bu = P.DEVICE_CG_FACTOR * max(P.u_units(yard[k - 1][0], ref[k - 1][0]) for k in ks)
    br = P.DEVICE_CG_FACTOR * max(P.res_units(yard[k - 1][1], ref[k - 1][1]) for k in ks)
    seen, over = [], []
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**PADDED, hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 2}):
            for k in ks:
                U, rep = K.cg_solve(j.F, 1e-30, max_its=k, precision_mode=hip.PREC_MIXED)
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and rep["iterations"] == k and pr["refine_passes"] == 1, (rep, pr["refine_passes"])
                assert pr["value_stream"] == hip.PREC_MIXED and pr["fp64_products"] == (1 if k < 50 else 2), (k, pr["fp64_products"])
                u, r = P.u_units(U, ref[k - 1][0]), P.res_units(pr["rel_residual_recurrence"], ref[k - 1][1])
                seen.append("k = %d: U %.3g, residual %.3g" % (k, u, r))
                if u > bu or r > br:
                    over.append((k, u, r))
    finally:
        K.free()
    print("cg %s mixed REFINE 2: %s units (bounds %.3g / %.3g)" % (name, "; ".join(seen), bu, br))
    assert not over, (over, bu, br)


@pytest.mark.parametrize("name", P.CG_MODELS)
def test_refine2_on_fixed48_counts_its_fp64_products(gpu_ctx, name):
    """The same on STAN_PREC_FIXED48, the counts only: one fp64 product up to k = 49, two from 50 on, one pass, the FIXED-48
    stream.  No iterate comparison: on this stream the loop that refreshes on the fp64 values and the loop that refreshes on
    the reduced ones are 411 / 885 units of 2^-53 apart at k = 51 / 52 where the float64 restatement of either is 4.3e3 / 7.2e3
    from its own long-double reference (tests/test_product_ref.py asserts that the two lie closer than the yardstick): no
    bound derived from rounding can tell them apart."""
    j = P.job(name)
    K = _assemble(gpu_ctx, name)
    try:
        with _options(gpu_ctx, {**PADDED, hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_REFINE: 2}):
            for k in P.REFINE2_KS:
                _U, rep = K.cg_solve(j.F, 1e-30, max_its=k, precision_mode=hip.PREC_FIXED48)
                pr = gpu_ctx.profile()
                assert rep["terminationtype"] == 5 and rep["iterations"] == k and pr["refine_passes"] == 1
                assert pr["value_stream"] == hip.PREC_FIXED48 and pr["fp64_products"] == (1 if k < 50 else 2), (k, pr["fp64_products"])
    finally:
        K.free()
