"""STAN_OPT_VALUE_STREAM_60: the plain products of an fp64 solve read the scaled values as lossless 60-bit words
(stan_amd/csrc/s60.h: sign, 7-bit exponent code, the 52 mantissa bits; 68 B per 3x3 block instead of 72).  The decoded
double is the stored double, so everything a solve returns keeps its bits; what the format cannot carry is refused and
the solve streams the fp64 values."""
import numpy as np
import pytest

from stan_amd import problem

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -126   # the smallest magnitude the format carries


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _spread(rng, n):
    """full 52-bit mantissas, both signs, exponents spread over -126 ... 0"""
    m = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52          # [1, 2), every mantissa bit random
    return np.ldexp(m, rng.integers(-126, 1, n).astype(np.int32)) * rng.choice([-1.0, 1.0], n)


def _unit(rng, n):
    """doubles in (-1, 1) with full 52-bit mantissas"""
    m = 1.0 + rng.integers(0, 1 << 52, n).astype(np.float64) * 2.0 ** -52
    return np.ldexp(m, rng.integers(-60, 0, n).astype(np.int32)) * rng.choice([-1.0, 1.0], n)


EDGES = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(2.0, 0.0), TINY, -TINY])


@pytest.mark.parametrize("n", [1, 9 * 64, 4096 + 37])
def test_encodable_values_come_back_bit_for_bit(gpu_ctx, n):
    """Encoder of the solve, decoder of the products, on the device (stan_hip_stream60_roundtrip): array lengths 1, one
    slot, and one that is no multiple of 64; int64 views, so that -0.0 and every mantissa bit count."""
    rng = np.random.default_rng(60 + n)
    cases = [np.resize(EDGES, n), np.resize(EDGES[::-1], n), _spread(rng, n), _unit(rng, n)]
    if n > 4096:   # 4 096 random doubles of (-1, 1), the edge values and the spread exponents in one array
        cases.append(np.concatenate([_unit(rng, 4096), EDGES, _spread(rng, n - 4096 - EDGES.size)]))
    for values in cases:
        back, refused = gpu_ctx.stream60_roundtrip(values)
        assert refused == 0
        assert np.array_equal(_bits(back), _bits(values))


@pytest.mark.parametrize("bad", [2.0, np.nextafter(TINY, 0.0), 5e-324, np.inf, np.nan], ids=["two", "below_tiny", "subnormal", "inf", "nan"])
@pytest.mark.parametrize("n", [1, 9 * 64, 1000])
def test_values_outside_the_range_are_refused(gpu_ctx, bad, n):
    """Each in a call of its own, at the array's last place and -- negated -- somewhere inside it: the count says how many."""
    values = np.resize(EDGES, n).copy()
    values[-1] = bad
    back, refused = gpu_ctx.stream60_roundtrip(values)
    assert refused == 1
    assert np.array_equal(_bits(back[:-1]), _bits(values[:-1]))
    if n > 1:
        values[n // 3] = -bad
        assert gpu_ctx.stream60_roundtrip(values)[1] == 2


def _solve(ctx, K, F, eps, on, prec=0):
    from stan_amd import hip
    ctx.set_option(hip.OPT_VALUE_STREAM_60, on)
    U, rep = K.cg_solve(F, eps, precision_mode=prec)
    return U, rep, ctx.profile()


@pytest.mark.parametrize("variant", [9, 12])
@pytest.mark.parametrize("model", ["cube6", "cube20", "perforated12"])
def test_solve_with_the_stream_forced_on_keeps_every_bit(gpu_ctx, model, variant):
    """Forced on (1) against forced off (0) on models below the automatic choice's size: cube_job(6) (1 029 block rows, 17
    slices, interior 27-neighbour rows, a ragged last slice with int32 columns), cube_job(20) (packed-column modes 1 and 2),
    perforated_job(12, 0.4) (mixed row lengths, odd slot counts: the loop's tail).  The stream belongs to k_spmv on the
    padded streams, so both runs take the large-system kernels (STAN_OPT_SPMV_SMALL 0) without the folded copy
    (STAN_OPT_ROW_FOLDING 0): the small-system and the folded kernels add a row's products in another order and never read
    this stream.  Both kernels the stream is instantiated for: STAN_OPT_SPMV_VARIANT 9 (the library's choice) and 12 (the
    int32-column loop unrolled by 4), each against the fp64 kernel of the same variant.  U, the iteration count, the
    residual's bits and the termination type must be equal, and the forced-on run must REPORT the stream: a refusal cannot
    pass as success."""
    from stan_amd import hip
    job = {"cube6": lambda: problem.cube_job(6), "cube20": lambda: problem.cube_job(20),
           "perforated12": lambda: problem.perforated_job(12, 0.4)}[model]()
    args = (job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    gpu_ctx.set_profiling(True)
    gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 0)
    gpu_ctx.set_option(hip.OPT_ROW_FOLDING, 0)
    gpu_ctx.set_option(hip.OPT_SPMV_VARIANT, variant)
    try:
        res = {}
        for on in (0, 1):          # a matrix each: the first product of either run scales K on its way
            K = gpu_ctx.assemble_hex8(*args)
            try:
                res[on] = _solve(gpu_ctx, K, job.F, 1e-10, on)
                if on:             # ... and a second solve on the same, scaled matrix: the stream made by the first
                    res[2] = _solve(gpu_ctx, K, job.F, 1e-10, 1)
            finally:
                K.free()
    finally:
        gpu_ctx.set_option(hip.OPT_VALUE_STREAM_60, -1)
        gpu_ctx.set_option(hip.OPT_SPMV_VARIANT, -1)
        gpu_ctx.set_option(hip.OPT_ROW_FOLDING, -1)
        gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 1)
        gpu_ctx.set_profiling(False)
    (U0, rep0, pr0), (U1, rep1, pr1), (U2, rep2, pr2) = res[0], res[1], res[2]
    assert pr0["value_stream"] == hip.PREC_FP64
    assert pr1["value_stream"] == hip.VALUE_STREAM_60 and pr2["value_stream"] == hip.VALUE_STREAM_60
    assert rep0["iterations"] > 20 and rep0["terminationtype"] in (1, 7)
    for U, rep in ((U1, rep1), (U2, rep2)):
        assert np.array_equal(_bits(U), _bits(U0))
        assert rep["iterations"] == rep0["iterations"] and rep["terminationtype"] == rep0["terminationtype"]
        assert _bits([rep["rel_residual"]])[0] == _bits([rep0["rel_residual"]])[0]
    info_blocks = pr0["spmv_bytes"] - pr1["spmv_bytes"]
    assert info_blocks > 0 and info_blocks % 4 == 0     # 4 B less per structural block, nothing else changes
    assert pr1["spmv_launches"] > 0 and pr1["col_slots_packed"] == pr0["col_slots_packed"]


@pytest.mark.parametrize("prec", ["fixed48", "mixed"])
def test_the_option_does_not_apply_to_the_reduced_precision_streams(gpu_ctx, prec):
    """STAN_PREC_FIXED48 and STAN_PREC_MIXED with the option at 1 behave exactly as with 0: their streams, their bits."""
    from stan_amd import hip
    pm = {"fixed48": hip.PREC_FIXED48, "mixed": hip.PREC_MIXED}[prec]
    job = problem.cube_job(6)
    K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    gpu_ctx.set_profiling(True)
    gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 0)
    try:
        U0, rep0, pr0 = _solve(gpu_ctx, K, job.F, 1e-8, 0, pm)
        U1, rep1, pr1 = _solve(gpu_ctx, K, job.F, 1e-8, 1, pm)
    finally:
        K.free()
        gpu_ctx.set_option(hip.OPT_VALUE_STREAM_60, -1)
        gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 1)
        gpu_ctx.set_profiling(False)
    assert pr0["value_stream"] == pm and pr1["value_stream"] == pm
    assert np.array_equal(_bits(U1), _bits(U0)) and rep1 == rep0
    for k in ("spmv_bytes", "refine_passes", "fp64_products", "iterations", "termination_type"):
        assert pr1[k] == pr0[k], k


def test_a_matrix_the_format_cannot_carry_streams_fp64(gpu_ctx):
    """E < 0: S K S has entries far above 2 in magnitude; the stream is refused for the whole matrix, the solve streams
    the fp64 values, says so in its profile and ends as it does without the option (alglib's -5)."""
    from stan_amd import hip
    job = problem.cube_job(4)
    job.mat_E_nu = np.array([[-210000.0, 0.3]])
    gpu_ctx.set_profiling(True)
    gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 0)
    try:
        out = []
        for on in (0, 1):
            K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
            try:
                out.append(_solve(gpu_ctx, K, job.F, 1e-8, on))
            finally:
                K.free()
    finally:
        gpu_ctx.set_option(hip.OPT_VALUE_STREAM_60, -1)
        gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 1)
        gpu_ctx.set_profiling(False)
    (U0, rep0, pr0), (U1, rep1, pr1) = out
    assert pr1["value_stream"] == hip.PREC_FP64 and pr1["spmv_bytes"] == pr0["spmv_bytes"]
    assert rep1["terminationtype"] == rep0["terminationtype"] == -5 and rep1["iterations"] == rep0["iterations"]
    assert np.array_equal(_bits(U1), _bits(U0))


def test_no_room_within_the_pool_budget_streams_fp64(gpu_ctx):
    """The block is a second copy of the values for the life of the matrix, so the solve decides whether there is room
    before it allocates.  A context of its own whose pool may park 8 MB (STAN_OPT_POOL_MAX_BYTES): the values of
    cube_job(20) and their 60-bit copy, tens of MB each, would not both stay parked when the matrix is freed -- the solve
    with the option at 1 streams fp64, says so in its profile and returns the same bits.  With the budget raised the next
    solve of the same matrix takes the stream: it was the budget, and the decision is made per solve."""
    from stan_amd import hip
    job = problem.cube_job(20)
    ctx = hip.Context(0)
    try:
        ctx.set_profiling(True)
        ctx.set_option(hip.OPT_SPMV_SMALL, 0)
        ctx.set_option(hip.OPT_ROW_FOLDING, 0)
        ctx.set_option(hip.OPT_POOL_MAX_BYTES, 8 << 20)
        K = ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
        U0, rep0, pr0 = _solve(ctx, K, job.F, 1e-10, 0)
        U1, rep1, pr1 = _solve(ctx, K, job.F, 1e-10, 1)
        ctx.set_option(hip.OPT_POOL_MAX_BYTES, 1 << 30)
        U2, rep2, pr2 = _solve(ctx, K, job.F, 1e-10, 1)
        K.free()
    finally:
        ctx.close()
    assert pr0["value_stream"] == hip.PREC_FP64
    assert pr0["spmv_bytes"] * 68 // 76 > 8 << 20     # the 60-bit copy alone (68 of a block's 76 B, at least) is over the budget
    assert pr1["value_stream"] == hip.PREC_FP64 and pr1["spmv_bytes"] == pr0["spmv_bytes"]
    assert pr2["value_stream"] == hip.VALUE_STREAM_60 and pr2["spmv_bytes"] < pr0["spmv_bytes"]
    for U, rep in ((U1, rep1), (U2, rep2)):
        assert np.array_equal(_bits(U), _bits(U0)) and rep == rep0


def test_option_values(gpu_ctx):
    from stan_amd import hip
    for bad in (-2, 2):
        with pytest.raises(hip.StanHipError):
            gpu_ctx.set_option(hip.OPT_VALUE_STREAM_60, bad)
    gpu_ctx.set_option(hip.OPT_VALUE_STREAM_60, -1)
