"""STAN_OPT_CG_REFRESH_60: in a solve whose plain products read the lossless 60-bit stream the fused refresh passes read
it too (k_spmv2<s60_t>): the same doubles, and the row sums spelled out as the fp64 pass forms them (spmv_kernels.inc:
s60_row).  Every test compares option 1 against option 0 on the same matrix with STAN_OPT_VALUE_STREAM_60 1 and asks for the
same bits -- U, the termination type, the iteration count, the residual -- and that the refresh passes REPORT the stream
they read: a solve that never took the stream cannot pass as success.

The models are problem.cube_job(n, jitter=0.05) at n = 6 and n = 14 with STAN_OPT_SPMV_SMALL 0, the large-system kernels: six
slices, and 53 slices with a ragged last workgroup (packed and int32 columns, odd slot counts)."""
import pytest

from stan_amd import problem

pytestmark = pytest.mark.gpu

SIZES = [6, 14]


def _defaults(hip):
    return {hip.OPT_CG_MERIT_STOP: 1, hip.OPT_CG_RUPDATE: 10, hip.OPT_SPMV_SMALL: 1, hip.OPT_ROW_FOLDING: -1,
            hip.OPT_SPMV_VARIANT: -1, hip.OPT_VALUE_STREAM_60: -1, hip.OPT_CG_X_RING: -1, hip.OPT_CG_REFRESH_60: -1}


@pytest.fixture(scope="module")
def jobs():
    return {n: problem.cube_job(n, jitter=0.05) for n in SIZES}


@pytest.fixture(scope="module")
def scaled(gpu_ctx, jobs):
    """One matrix per size, scaled and with its 60-bit stream built by one short solve: what the solves of a test share."""
    from stan_amd import hip
    Ks = {}
    try:
        for k, v in {hip.OPT_SPMV_SMALL: 0, hip.OPT_ROW_FOLDING: 0, hip.OPT_VALUE_STREAM_60: 1}.items():
            gpu_ctx.set_option(k, v)
        for n in SIZES:
            j = jobs[n]
            Ks[n] = gpu_ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
            Ks[n].cg_solve(j.F, 0.0, max_its=3)
    finally:
        for k, v in _defaults(hip).items():
            gpu_ctx.set_option(k, v)
    yield Ks
    for K in Ks.values():
        K.free()


def _solve(ctx, K, F, refresh60, eps=1e-10, opts=None):
    """(U, report, profile, (ring window, flushes, refresh stream)) of one solve on the 60-bit stream"""
    from stan_amd import hip
    setting = {hip.OPT_SPMV_SMALL: 0, hip.OPT_ROW_FOLDING: 0, hip.OPT_VALUE_STREAM_60: 1, hip.OPT_CG_X_RING: 0,
               hip.OPT_CG_REFRESH_60: refresh60}
    setting.update(opts or {})
    ctx.set_profiling(True)
    try:
        for k, v in setting.items():
            ctx.set_option(k, v)
        U, rep = K.cg_solve(F, eps)
        return U, rep, ctx.profile(), ctx.cg_loop_info()
    finally:
        for k, v in _defaults(hip).items():
            ctx.set_option(k, v)
        ctx.set_profiling(False)


def _same(hip, off, on):
    (U0, rep0, pr0, info0), (U1, rep1, pr1, info1) = off, on
    assert U1.tobytes() == U0.tobytes()
    assert rep1["terminationtype"] == rep0["terminationtype"] and rep1["iterations"] == rep0["iterations"]
    assert float(rep1["rel_residual"]).hex() == float(rep0["rel_residual"]).hex()
    assert pr0["spmv2_launches"] > 0 and pr1["spmv2_launches"] == pr0["spmv2_launches"]
    assert pr1["loop_kernel_launches"] - info1[1] == pr0["loop_kernel_launches"] - info0[1]
    assert info0[2] == hip.PREC_FP64 and info1[2] == hip.VALUE_STREAM_60


@pytest.mark.parametrize("variant", [9, 12])
@pytest.mark.parametrize("rupdate", [1, 10])
@pytest.mark.parametrize("n", SIZES)
def test_refresh_passes_on_the_stream_keep_every_bit(gpu_ctx, jobs, scaled, n, rupdate, variant):
    """eps 1e-10 with a refresh every 10 iterations and with one every iteration (every product of the loop a two-product
    pass), next to the plain products of STAN_OPT_SPMV_VARIANT 9 and 12."""
    from stan_amd import hip
    opts = {hip.OPT_CG_RUPDATE: rupdate, hip.OPT_SPMV_VARIANT: variant}
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, opts=opts)
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, opts=opts)
    _same(hip, off, on)
    assert off[1]["iterations"] > 30
    if rupdate == 10:   # (with a refresh every iteration there is no plain product to report)
        assert off[2]["value_stream"] == hip.VALUE_STREAM_60 and on[2]["value_stream"] == hip.VALUE_STREAM_60


@pytest.mark.parametrize("n", SIZES)
def test_both_parts_together(gpu_ctx, jobs, scaled, n):
    """The ring of directions and the refresh passes on the stream in one solve (merit stop off), against neither."""
    from stan_amd import hip
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, opts={hip.OPT_CG_MERIT_STOP: 0})
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, opts={hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_X_RING: 1})
    _same(hip, off, on)
    assert off[3][0] == 0 and on[3][0] == 10 and on[3][1] > 1


@pytest.mark.parametrize("n", SIZES)
def test_without_the_stream_the_option_selects_nothing(gpu_ctx, jobs, scaled, n):
    """STAN_OPT_VALUE_STREAM_60 0: the refresh passes read the fp64 values whatever this option says."""
    from stan_amd import hip
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, opts={hip.OPT_VALUE_STREAM_60: 0})
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, opts={hip.OPT_VALUE_STREAM_60: 0})
    assert on[0].tobytes() == off[0].tobytes() and on[1] == off[1]
    assert on[3][2] == hip.PREC_FP64 and on[2]["value_stream"] == hip.PREC_FP64


def test_option_values(gpu_ctx):
    from stan_amd import hip
    for bad in (-2, 2):
        with pytest.raises(hip.StanHipError):
            gpu_ctx.set_option(hip.OPT_CG_REFRESH_60, bad)
    gpu_ctx.set_option(hip.OPT_CG_REFRESH_60, -1)
