"""STAN_OPT_CG_X_RING: with the merit stop off nothing reads the iterate between two residual refreshes, so the loop keeps
the search directions of a window in a ring, k_update writes p' into the next slot and leaves x alone, and k_xring_flush
forms x once per window (and once behind the loop) with one fused multiply-add per pending term, in iteration order
(stan_amd/csrc/x_ring.h).  The same operations in the same order: every test here compares option 1 against option 0 on
the same matrix and asks for the same bits -- U, the termination type, the iteration count, the residual.

The models are problem.cube_job(n, jitter=0.05) at n = 6 and n = 14 with STAN_OPT_SPMV_SMALL 0, the large-system kernels: six
slices, and 53 slices with a ragged last workgroup."""
import numpy as np
import pytest

from stan_amd import problem

pytestmark = pytest.mark.gpu

SIZES = [6, 14]


def _defaults(hip):
    return {hip.OPT_CG_MERIT_STOP: 1, hip.OPT_CG_RUPDATE: 10, hip.OPT_SPMV_SMALL: 1, hip.OPT_CG_FUSED_REFRESH: 1,
            hip.OPT_CG_SINGLE_REDUCE: 0, hip.OPT_CG_X_RING: -1}


def _assemble(ctx, job):
    return ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)


@pytest.fixture(scope="module")
def jobs():
    return {n: problem.cube_job(n, jitter=0.05) for n in SIZES}


@pytest.fixture(scope="module")
def scaled(gpu_ctx, jobs):
    """One matrix per size, brought into its scaled form by one iteration: what the solves of a test share."""
    from stan_amd import hip
    gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 0)
    Ks = {}
    try:
        for n in SIZES:
            Ks[n] = _assemble(gpu_ctx, jobs[n])
            Ks[n].cg_solve(jobs[n].F, 0.0, max_its=1)
    finally:
        gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 1)
    yield Ks
    for K in Ks.values():
        K.free()


def _solve(ctx, K, F, ring, eps=1e-10, max_its=0, prec=0, opts=None):
    """One solve with the large-system kernels and the merit stop off unless `opts` (STAN_OPT_* by number) say otherwise;
    returns (U, report, profile, (window, flushes))."""
    from stan_amd import hip
    setting = {hip.OPT_SPMV_SMALL: 0, hip.OPT_CG_MERIT_STOP: 0, hip.OPT_CG_X_RING: ring}
    setting.update(opts or {})
    ctx.set_profiling(True)
    try:
        for k, v in setting.items():
            ctx.set_option(k, v)
        U, rep = K.cg_solve(F, eps, max_its=max_its, precision_mode=prec)
        return U, rep, ctx.profile(), ctx.cg_x_ring_info()
    finally:
        for k, v in _defaults(hip).items():
            ctx.set_option(k, v)
        ctx.set_profiling(False)


def _same(a, b):
    (U0, rep0), (U1, rep1) = a[:2], b[:2]
    assert U1.tobytes() == U0.tobytes()
    assert rep1["terminationtype"] == rep0["terminationtype"] and rep1["iterations"] == rep0["iterations"]
    assert float(rep1["rel_residual"]).hex() == float(rep0["rel_residual"]).hex()


def _flushes(enqueued, rupdate):
    """flush launches of a loop that enqueued this many iterations: one in front of every refresh iteration -- or, without a
    refresh, in front of iterations 11, 21, ... (W = 10) -- and the closing one"""
    return (enqueued // rupdate if rupdate else (enqueued - 1) // 10) + 1


@pytest.mark.parametrize("n", SIZES)
def test_many_windows_ending_inside_one(gpu_ctx, jobs, scaled, n):
    """eps 1e-10: dozens of windows of 10, the stop somewhere inside the last; and the launch count differs from the plain
    loop's by exactly the flush launches."""
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0)
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1)
    _same(off, on)
    assert off[1]["terminationtype"] == 1 and off[1]["iterations"] > 30
    assert off[3] == (0, 0)
    window, flushes = on[3]
    assert window == 10 and flushes == _flushes(on[2]["loop_iterations_enqueued"], 10)
    assert on[2]["loop_iterations_enqueued"] == off[2]["loop_iterations_enqueued"]
    assert on[2]["loop_kernel_launches"] - off[2]["loop_kernel_launches"] == flushes
    assert on[2]["cg_iteration_vector_bytes"] < off[2]["cg_iteration_vector_bytes"]


@pytest.mark.parametrize("max_its", [1, 7, 9, 10, 11, 19, 20, 21])
@pytest.mark.parametrize("n", SIZES)
def test_stop_by_iteration_count(gpu_ctx, jobs, scaled, n, max_its):
    """Type 5 before the first refresh, on the iteration before a refresh, on it and behind it: the closing flush sums
    what is pending, none, one term or a window's worth."""
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, eps=0.0, max_its=max_its)
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, eps=0.0, max_its=max_its)
    _same(off, on)
    assert on[1]["terminationtype"] == 5 and on[1]["iterations"] == max_its and on[3][0] == 10


@pytest.mark.parametrize("rupdate", [0, 2, 3, 10])
@pytest.mark.parametrize("n", SIZES)
def test_refresh_periods(gpu_ctx, jobs, scaled, n, rupdate):
    """The window follows the refresh period; without a refresh it is 10 and the ring's capacity decides the flushes."""
    from stan_amd import hip
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, opts={hip.OPT_CG_RUPDATE: rupdate})
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, opts={hip.OPT_CG_RUPDATE: rupdate})
    _same(off, on)
    window, flushes = on[3]
    assert window == (rupdate or 10) and flushes == _flushes(on[2]["loop_iterations_enqueued"], rupdate)
    assert on[2]["loop_kernel_launches"] - off[2]["loop_kernel_launches"] == flushes
    assert on[2]["spmv2_launches"] == off[2]["spmv2_launches"]


@pytest.mark.parametrize("n", SIZES)
def test_zero_right_hand_side(gpu_ctx, jobs, scaled, n):
    """The first residual test ends the solve: no iteration, no flush, U = 0."""
    F = np.zeros_like(jobs[n].F)
    off = _solve(gpu_ctx, scaled[n], F, 0)
    on = _solve(gpu_ctx, scaled[n], F, 1)
    _same(off, on)
    assert on[1]["iterations"] == 0 and not on[0].any() and on[3][1] == 0


@pytest.mark.parametrize("n", SIZES)
def test_fresh_matrix(gpu_ctx, jobs, n):
    """A matrix each, so that the first product of either solve scales K on its way (k_spmv_first) and reads p_1 from its slot."""
    out = []
    for ring in (0, 1):
        K = _assemble(gpu_ctx, jobs[n])
        try:
            out.append(_solve(gpu_ctx, K, jobs[n].F, ring))
        finally:
            K.free()
    _same(*out)
    assert out[0][3][0] == 0 and out[1][3][0] == 10


def _counts(profile):
    """every profile field that is not a time"""
    return {k: v for k, v in profile.items() if "_ms" not in k}


@pytest.mark.parametrize("form", ["merit_stop_1", "fused_refresh_0", "rupdate_1", "single_reduce_1", "fixed48", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_ring_left_out(gpu_ctx, jobs, scaled, n, form):
    """Where the loop does not defer x today -- the merit stop on, a literal second product, a refresh every iteration, the
    single-reduction loop, a reduced-precision stream -- option 1 changes neither a bit nor a profile field."""
    from stan_amd import hip
    opts, prec = {"merit_stop_1": ({hip.OPT_CG_MERIT_STOP: 1}, hip.PREC_FP64),
                  "fused_refresh_0": ({hip.OPT_CG_FUSED_REFRESH: 0}, hip.PREC_FP64),
                  "rupdate_1": ({hip.OPT_CG_RUPDATE: 1}, hip.PREC_FP64),
                  "single_reduce_1": ({hip.OPT_CG_SINGLE_REDUCE: 1}, hip.PREC_FP64),
                  "fixed48": ({}, hip.PREC_FIXED48), "mixed": ({}, hip.PREC_MIXED)}[form]
    off = _solve(gpu_ctx, scaled[n], jobs[n].F, 0, eps=1e-8, prec=prec, opts=opts)
    on = _solve(gpu_ctx, scaled[n], jobs[n].F, 1, eps=1e-8, prec=prec, opts=opts)
    _same(off, on)
    assert off[1]["iterations"] > 10
    assert _counts(on[2]) == _counts(off[2])
    assert on[3] == (0, 0) and off[3] == (0, 0)


def test_option_values(gpu_ctx):
    from stan_amd import hip
    for bad in (-2, 2):
        with pytest.raises(hip.StanHipError):
            gpu_ctx.set_option(hip.OPT_CG_X_RING, bad)
    gpu_ctx.set_option(hip.OPT_CG_X_RING, -1)
