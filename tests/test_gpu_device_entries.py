"""The entries that take the caller's own device memory -- stan_hip_assemble_hex8_dev, stan_hip_cg_solve_dev,
stan_hip_cg_solve_multi_dev, stan_hip_recover_hex8_dev -- and stan_hip_set_stream: the path bench.py times and INTEGRATION.md
offers to a host whose data is already in HBM.

The host entries are held to extended-precision references by the rest of the suite, so every comparison here is BIT EQUALITY
with the host entry (tobytes() / array_equal, on values and on the report fields): that carries each of those bounds over,
and there is no tolerance in this file.  What the device-pointer entries add is what the host entries hide, and
tests/device_buffers.py makes it visible: every array is one allocation [guard | payload | guard], outputs prefilled with a
NaN pattern ("never written"), guards with another, inputs compared whole with a clone taken before the call, and every case
runs once with the payloads on a 256-byte boundary and once one element past it (natural alignment only).

Findings these tests pin (include/stan_hip.h says the same):
  * no kernel stores outside [0, N) / [0, 48 n_elem) of a caller's output, and every entry of it is written for every
    termination code (1, 5, 7, -5; iteration 0 with F = 0), so d_U need not be initialised;
  * N = 0 (every DOF fixed): nothing is stored -- a one-element d_U comes back untouched;
  * every access through a caller's pointer is one element wide: natural alignment is enough;
  * a call orders itself behind the work already enqueued on the stream the context was given (stan_hip_set_stream) and
    returns with its outputs complete; on the context's own stream nothing orders it behind another stream's work (the
    control below reads the stale input, as it must for the first statement to mean anything)."""
import os

import numpy as np
import pytest

from stan_amd import hip, problem
from stan_amd.cube import cube_bcs, cube_mesh, revolved_mesh
from tests import device_buffers as B
from tests import forces_ref
from tests import product_ref as P
from tests.conftest import fake_rccl_env
from tests.gpu_models import DEFAULTS
from tests.test_gpu_element_precision import _max_row_blocks_of_the_fast_kernel, _mixed
from tests.test_gpu_product_precision import FORMS, LARGE, PADDED
from tests.test_gpu_sharded import ASYNC_BANNER, _torchrun

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OFFSETS = (0, 1)
RESTORE = {**DEFAULTS, hip.OPT_ASSEMBLY_MODE: 0}
PROFILE_FIELDS = ("value_stream", "refine_passes", "iterations", "termination_type")


@pytest.fixture(scope="module")
def ctx(built_libs):
    """A context of this module's own: the stream tests never touch the session-wide one."""
    import torch  # noqa: F401  (first, so one HIP runtime is shared)
    c = hip.Context(0)
    yield c
    c.close()


def _sync():
    import torch
    torch.cuda.synchronize()


class _options:
    """Options (and profiling) set for a block, every one restored to its default behind it."""

    def __init__(self, ctx, opts, profiling=False):
        self.ctx, self.opts, self.profiling = ctx, opts, profiling

    def __enter__(self):
        self.ctx.set_profiling(self.profiling)
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        try:
            for k in self.opts:
                self.ctx.set_option(k, RESTORE[k])
        finally:
            self.ctx.set_profiling(False)


def _job(name):
    """cube1; the jittered 3^3 cube and revolved_mesh(36, 2, 3) with mixed element types and materials, as
    tests/test_gpu_element_precision.py builds them; the models of tests/product_ref.py by their names."""
    def make():
        if name == "cube3mixed":
            xyz, conn = cube_mesh(3, jitter=0.1)
            spc, ld, f = cube_bcs(3)
        elif name == "revolved":
            xyz, conn = revolved_mesh(36, 2, 3)
            spc, ld, f = np.nonzero(xyz[:, 2] == 0.0)[0], np.nonzero(xyz[:, 2] == 3.0)[0], np.array([0.0, 10.0, 5.0])
        else:
            return P.job(name)
        return _mixed(problem.make_job(xyz, conn, spc, np.ones((len(spc), 3)), ld, np.tile(f, (len(ld), 1))), 31)
    return P.cached(("device_entries", name), make)


def _host_args(job, **replace):
    g = lambda k: replace.get(k, getattr(job, k))
    return (g("xyz"), g("node_dof"), g("conn"), g("elem_mat"), g("elem_type"), job.mat_E_nu, g("red"))


def _describe(K, export=True):
    """export=False: info() only (the degenerate models, whose export the host tests do not make either)."""
    if not export:
        return dict(info=K.info())
    return dict(csr=K.to_csr(upper_only=False), diagonal=K.diagonal(), info=K.info())


def _assert_same_matrix(got, want):
    assert got.keys() == want.keys()
    for a, b, what in zip(got.get("csr", ()), want.get("csr", ()), ("rowptr", "col", "val")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    if "diagonal" in want:
        assert got["diagonal"].tobytes() == want["diagonal"].tobytes()
    assert got["info"] == want["info"]


def _vec(name, values, n_dof, offset):
    return B.input_(name, values, B.guard_len(n_dof), DEV, offset)


def _out(name, n, n_dof, offset):
    return B.output(name, n, B.guard_len(n_dof), DEV, offset)


# ---- assembly ----------------------------------------------------------------------------------------------------------------------

ASSEMBLY_CASES = [("cube1", 0), ("cube3mixed", 0), ("cube3mixed", 1), ("revolved", 0), ("revolved", 1), ("star12", 0)]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name,mode", ASSEMBLY_CASES)
def test_assembly_from_device_arrays_has_the_host_entry_bits(ctx, name, mode, offset):
    """The CSR export (all three arrays, both triangles), the diagonal and info() as a whole; the inputs unchanged.  The
    revolved mesh has rows wider than the LDS accumulators take (k_numeric_wide); mode 1 is the colour scatter."""
    job = _job(name)

    def host():
        K = ctx.assemble_hex8(*_host_args(job))
        try:
            return _describe(K)
        finally:
            K.free()
    with _options(ctx, {hip.OPT_ASSEMBLY_MODE: mode}):
        want = P.cached(("device_entries", "K", name, mode), host)
        mesh = B.Mesh(job, DEV, offset)
        _sync()
        K = ctx.assemble_hex8_dev(*mesh.assemble_args())
        try:
            got = _describe(K)
        finally:
            K.free()
    _sync()
    B.check(mesh.inputs)
    _assert_same_matrix(got, want)
    if name == "revolved":
        assert want["info"]["max_row_blocks"] > _max_row_blocks_of_the_fast_kernel()


@pytest.mark.parametrize("offset", OFFSETS)
def test_assembly_errors_from_device_arrays(ctx, offset):
    """A flattened element is STAN_E_DETJ and last_bad_element() its index IN THE ARRAYS PASSED (here the model without its
    first two elements); a shifted node_dof entry is STAN_E_DOF_LAYOUT.  Both checks run on the device behind the host entry
    too.  (No out-of-range connectivity or material index goes to a device-pointer entry: nothing promises a device check.)"""
    job = problem.cube_job(3)
    xyz = job.xyz.copy()
    xyz[job.conn[5]] = xyz[job.conn[5]] * [1, 1, 0]
    with pytest.raises(hip.StanHipError) as ei:
        ctx.assemble_hex8(*_host_args(job, xyz=xyz))
    host_bad = ctx.last_bad_element()
    assert ei.value.code == hip.E_DETJ and host_bad >= 1
    for skip in (0, min(2, host_bad)):
        mesh = B.Mesh(job, DEV, offset, xyz=xyz, conn=job.conn[skip:], elem_mat=job.elem_mat[skip:], elem_type=job.elem_type[skip:])
        _sync()
        with pytest.raises(hip.StanHipError) as ei:
            ctx.assemble_hex8_dev(*mesh.assemble_args())
        assert ei.value.code == hip.E_DETJ and ctx.last_bad_element() == host_bad - skip
        _sync()
        B.check(mesh.inputs)
    bad_dof = job.node_dof.copy()
    bad_dof[4, 1] += 7
    mesh = B.Mesh(job, DEV, offset, node_dof=bad_dof)
    _sync()
    with pytest.raises(hip.StanHipError) as ei:
        ctx.assemble_hex8_dev(*mesh.assemble_args())
    assert ei.value.code == hip.E_DOF_LAYOUT
    _sync()
    B.check(mesh.inputs)


# ---- solve -------------------------------------------------------------------------------------------------------------------------

STREAM60 = {hip.OPT_VALUE_STREAM_60: 1}
# form -> (model, options on top of STAN_OPT_CG_MERIT_STOP 0, precision mode, the value stream the profile must report or None)
SOLVE_FORMS = {
    "cube6-small": ("cube6", FORMS["small"], hip.PREC_FP64, None),                        # k_spmv_small
    "cube6-padded-v9": ("cube6", FORMS["v9"], hip.PREC_FP64, None),                       # k_spmv<double, 0, 9>
    "cube6-large-stream60": ("cube6", {**LARGE, **STREAM60}, hip.PREC_FP64, None),        # as the library routes it
    "cube6-padded-stream60": ("cube6", {**PADDED, **STREAM60}, hip.PREC_FP64, hip.VALUE_STREAM_60),   # ... and where the stream is certainly read
    "cube6-single-reduce": ("cube6", {hip.OPT_CG_SINGLE_REDUCE: 1}, hip.PREC_FP64, None),
    "cube6-fixed48": ("cube6", {}, hip.PREC_FIXED48, hip.PREC_FIXED48),
    "cube6-mixed": ("cube6", {hip.OPT_CG_REFINE: 1}, hip.PREC_MIXED, hip.PREC_MIXED),
    "perforated12-small": ("perforated12", FORMS["small"], hip.PREC_FP64, None),
    "perforated12-fold": ("perforated12", FORMS["fold"], hip.PREC_FP64, None),            # k_spmv_fold
}
RUNS = ((1e-8, 0), (1e-8, 7))   # to convergence; stopped at max_its = 7 (type 5)


@pytest.mark.parametrize("form", sorted(SOLVE_FORMS))
def test_solve_from_device_vectors_has_the_host_entry_bits(ctx, form):
    """Assembly and both solves through the device-pointer entries against the same sequence through the host entries, each
    on a matrix of its own: U, the three report fields and the profile fields that describe what ran (the timings and byte
    counts of stan_profile are not results).  d_U starts as NaN: every entry is written, nothing beside it."""
    name, opts, prec, want_stream = SOLVE_FORMS[form]
    job = P.job(name)
    with _options(ctx, {**opts, hip.OPT_CG_MERIT_STOP: 0}, profiling=True):
        want = []
        K = ctx.assemble_hex8(*_host_args(job))
        try:
            for eps, max_its in RUNS:
                U, rep = K.cg_solve(job.F, eps, max_its, prec)
                pr = ctx.profile()
                want.append((U, rep, {k: pr[k] for k in PROFILE_FIELDS}))
        finally:
            K.free()
        assert want[0][1]["terminationtype"] in (1, 7) and want[0][1]["iterations"] > 7 and want[1][1]["terminationtype"] == 5
        if want_stream is not None:
            assert want[0][2]["value_stream"] == want_stream
        for offset in OFFSETS:
            mesh = B.Mesh(job, DEV, offset)
            dF, dU = _vec("F", job.F, job.n_dof, offset), _out("U", job.n_red, job.n_dof, offset)
            _sync()
            K = ctx.assemble_hex8_dev(*mesh.assemble_args())
            try:
                for (eps, max_its), (U, rep, pr) in zip(RUNS, want):
                    dU.refill()
                    _sync()
                    got = K.cg_solve_dev(dF.ptr, dU.ptr, eps, max_its, prec)
                    got_pr = ctx.profile()
                    _sync()
                    B.check(mesh.inputs + [dF, dU])
                    assert dU.numpy().tobytes() == U.tobytes(), (form, offset, max_its)
                    assert got == rep and np.float64(got["rel_residual"]).tobytes() == np.float64(rep["rel_residual"]).tobytes()
                    assert {k: got_pr[k] for k in PROFILE_FIELDS} == pr
            finally:
                K.free()


def _edge_models():
    """name -> (host assembly arguments as a dict of replacements on cube_job(2), F): the degenerate inputs of
    tests/test_gpu_parity.py::test_edge_cases_empty_and_fully_fixed, F = 0, and the two smallest cubes."""
    from stan_amd import host
    job = problem.cube_job(2)
    out = {}
    xyz = np.vstack([job.xyz, [[9.0, 9.0, 9.0]]])
    nd = np.vstack([job.node_dof, [[81, 82, 83]]]).astype(np.int32)
    red, nfix = host.dof_reduction(84, nd, np.nonzero(job.xyz[:, 0] == 0)[0], np.ones((9, 3)))
    F = np.zeros(84 - nfix)
    F[:54] = job.F
    out["orphan_node"] = (job, dict(xyz=xyz, node_dof=nd, red=red), F, None)
    out["no_elements"] = (job, dict(conn=np.zeros((0, 8), np.int32), elem_mat=np.zeros(0, np.int32), elem_type=np.zeros(0, np.uint8)),
                          job.F, -5)
    out["zero_load"] = (job, {}, np.zeros_like(job.F), 1)
    out["cube2"] = (job, {}, job.F, None)
    out["cube1"] = (problem.cube_job(1), {}, problem.cube_job(1).F, None)
    return out


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ["orphan_node", "no_elements", "zero_load", "cube2", "cube1"])
def test_edge_cases_write_every_entry_of_U(ctx, name, offset):
    """'U returned for every code' on a d_U that was NaN before: an orphan node (three empty rows: zeros), a model without
    elements (type -5: zeros), F = 0 (iteration 0, type 1: zeros), one and eight elements -- each entry equal to the host
    entry's, which starts from a zeroed buffer of its own."""
    job, rep_, F, want_type = _edge_models()[name]

    class J:
        pass
    j = J()
    for k in ("xyz", "node_dof", "conn", "elem_mat", "elem_type", "mat_E_nu", "red"):
        setattr(j, k, rep_.get(k, getattr(job, k)))
    export = name != "no_elements"
    K = ctx.assemble_hex8(*_host_args(j))
    try:
        want_K = _describe(K, export)
        U, rep = K.cg_solve(F, 1e-8)
    finally:
        K.free()
    if want_type is not None:
        assert rep["terminationtype"] == want_type and not U.any()
        assert name != "zero_load" or rep["iterations"] == 0
    if name == "orphan_node":
        assert not U[54:].any() and U[:54].any()
    mesh = B.Mesh(j, DEV, offset)
    dF, dU = _vec("F", F, mesh.n_dof, offset), _out("U", F.shape[0], mesh.n_dof, offset)
    _sync()
    K = ctx.assemble_hex8_dev(*mesh.assemble_args())
    try:
        _assert_same_matrix(_describe(K, export), want_K)
        got = K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8)
    finally:
        K.free()
    _sync()
    B.check(mesh.inputs + [dF, dU])
    print("%s offset %d: host %s, device pointers %s" % (name, offset, rep, got))
    assert got == rep and dU.numpy().tobytes() == U.tobytes()


@pytest.mark.parametrize("offset", OFFSETS)
def test_fully_fixed_model_stores_nothing(ctx, offset):
    """N = 0: the reduced system is empty, the host entry returns an empty U with type 1 at iteration 0.  The device-pointer
    entry needs non-null pointers, so it gets one-element payloads -- and leaves d_U UNTOUCHED (k_result stores on free DOFs
    only): not the pattern's bits changed, not a zero, no guard entry."""
    job = problem.cube_job(2)
    allfix = np.full(job.n_dof, -1, np.int32)
    K = ctx.assemble_hex8(*_host_args(job, red=allfix))
    try:
        want_K = _describe(K, export=False)
        U, rep = K.cg_solve(np.zeros(0), 1e-8)
    finally:
        K.free()
    assert U.shape == (0,) and rep["terminationtype"] == 1 and rep["iterations"] == 0 and want_K["info"]["n_reduced"] == 0
    mesh = B.Mesh(job, DEV, offset, red=allfix)
    dF, dU = _vec("F", np.array([3.0]), job.n_dof, offset), _out("U", 1, job.n_dof, offset)
    _sync()
    K = ctx.assemble_hex8_dev(*mesh.assemble_args())
    try:
        _assert_same_matrix(_describe(K, export=False), want_K)
        got = K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8)
    finally:
        K.free()
    _sync()
    assert got == rep
    B.check(mesh.inputs + [dF, dU], written=False)
    found = dU.problems()
    assert len(found) == 1 and "1 payload entries never written" in found[0]     # untouched


def test_the_bench_cycle_repeats_its_bits(ctx):
    """bench.py's step, three times on the same tensors: assemble_hex8_dev, cg_solve_dev, free.  The pool hands the blocks
    of one cycle to the next in stream order; d_U is NaN again before each solve."""
    job = P.job("cube6")
    mesh = B.Mesh(job, DEV)
    dF, dU = _vec("F", job.F, job.n_dof, 0), _out("U", job.n_red, job.n_dof, 0)
    _sync()
    seen = []
    with _options(ctx, {hip.OPT_CG_MERIT_STOP: 0}, profiling=True):
        for _cycle in range(3):
            dU.refill()
            _sync()
            K = ctx.assemble_hex8_dev(*mesh.assemble_args())
            try:
                rep = K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8)
                info = K.info()
            finally:
                K.free()
            _sync()
            B.check(mesh.inputs + [dF, dU])
            seen.append((dU.numpy().tobytes(), rep, np.float64(rep["rel_residual"]).tobytes(), info))
        K = ctx.assemble_hex8(*_host_args(job))
        try:
            U, rep = K.cg_solve(job.F, 1e-8)
        finally:
            K.free()
    assert seen[0] == seen[1] == seen[2]
    assert seen[0][0] == U.tobytes() and seen[0][1] == rep and rep["terminationtype"] == 1


# ---- batched solve -----------------------------------------------------------------------------------------------------------------

def _fifteen_columns():
    """[15, N]: the three vectors of product_ref.load_cases repeated, scaled by +-2^e, a zero column in the middle: one group
    each of 8, 4, 2 and 1 columns (stan_cg_multi_device)."""
    lc = P.load_cases("cube6")
    F = np.stack([lc[c % 3] * ((-1.0) ** c * 2.0 ** (c - 7)) for c in range(15)])
    F[7] = 0.0
    return np.ascontiguousarray(F)


@pytest.mark.parametrize("offset", OFFSETS)
def test_batched_solve_from_device_vectors_has_the_host_entry_bits(ctx, offset):
    job = P.job("cube6")
    F = _fifteen_columns()
    N = job.n_red
    with _options(ctx, {hip.OPT_CG_MERIT_STOP: 0}):
        def host():
            K = ctx.assemble_hex8(*_host_args(job))
            try:
                return K.cg_solve_multi(F, 1e-8)
            finally:
                K.free()
        U, reps = P.cached(("device_entries", "multi"), host)
        assert [r["terminationtype"] for r in reps] == [1] * 15 and reps[7]["iterations"] == 0 and not U[7].any()
        assert min(r["iterations"] for r in reps[:7] + reps[8:]) > 7
        mesh = B.Mesh(job, DEV, offset)
        dF, dU = _vec("F", F, job.n_dof, offset), _out("U", 15 * N, job.n_dof, offset)
        _sync()
        K = ctx.assemble_hex8_dev(*mesh.assemble_args())
        try:
            got = K.cg_solve_multi_dev(dF.ptr, dU.ptr, 15, 1e-8)
        finally:
            K.free()
    _sync()
    B.check(mesh.inputs + [dF, dU])
    assert dU.numpy().tobytes() == U.tobytes()
    assert got == reps
    assert [np.float64(r["rel_residual"]).tobytes() for r in got] == [np.float64(r["rel_residual"]).tobytes() for r in reps]


# ---- recovery ----------------------------------------------------------------------------------------------------------------------

TWO_MATERIALS = [[210000.0, 0.3], [70000.0, 0.33]]


def _recovery_model(name):
    """Strips of k elements around the 8 of a wave and the 32 of a block, and the jittered 3^3 cube: two materials, a random
    displacement field."""
    def make():
        xyz, conn = cube_mesh(3, jitter=0.1) if name == "cube3" else forces_ref.strip_mesh(int(name))
        m = forces_ref.model(xyz, conn, elem_mat=np.arange(conn.shape[0]) % 2, mat_E_nu=TWO_MATERIALS)
        return m, forces_ref.random_disp(m, 900 + conn.shape[0])
    return P.cached(("device_entries", "recovery", name), make)


def _recover_dev(ctx, mesh, strain, stress):
    return ctx.recover_hex8_dev(*mesh.recover_args(), strain.ptr, stress.ptr)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ["1", "7", "8", "9", "31", "32", "33", "cube3"])
def test_recovery_into_device_arrays_has_the_host_entry_bits(ctx, name, offset):
    """A guard sits directly behind element k - 1 of both outputs: where a tail that does not stop at n_elem would write."""
    m, disp = _recovery_model(name)
    ne = m.conn.shape[0]
    strain, stress = ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    assert np.isfinite(strain).all() and strain.any() and stress.any()
    mesh = B.Mesh(m, DEV, offset, disp=disp)
    d_strain, d_stress = _out("strain", 48 * ne, m.n_dof, offset), _out("stress", 48 * ne, m.n_dof, offset)
    _sync()
    _recover_dev(ctx, mesh, d_strain, d_stress)
    _sync()
    B.check(mesh.inputs + [d_strain, d_stress])
    assert d_strain.numpy().tobytes() == strain.tobytes() and d_stress.numpy().tobytes() == stress.tobytes()


@pytest.mark.parametrize("offset", OFFSETS)
def test_recovery_refuses_a_hex8_g1_element_like_the_host_entry(ctx, offset):
    """STAN_E_UNSUPPORTED with the host entry's element number; after an error code only the guards are promised."""
    m, disp = _recovery_model("9")
    types = m.elem_type.copy()
    types[[4, 6]] = hip.HEX8_G1
    with pytest.raises(hip.StanHipError) as ei:
        ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, types, m.mat_E_nu)
    host_bad = ctx.last_bad_element()
    assert ei.value.code == hip.E_UNSUPPORTED and host_bad == 4
    mesh = B.Mesh(m, DEV, offset, disp=disp, elem_type=types)
    d_strain, d_stress = _out("strain", 48 * 9, m.n_dof, offset), _out("stress", 48 * 9, m.n_dof, offset)
    _sync()
    with pytest.raises(hip.StanHipError) as ei:
        _recover_dev(ctx, mesh, d_strain, d_stress)
    assert ei.value.code == hip.E_UNSUPPORTED and ctx.last_bad_element() == host_bad
    _sync()
    B.check(mesh.inputs + [d_strain, d_stress], written=False)


# ---- a caller's stream -------------------------------------------------------------------------------------------------------------

class _Producer:
    """A stream of the caller's with a delay on it: 50-200 ms, two orders of magnitude above the library's time to its first
    kernel, sized by measuring it once with two events on the stream."""

    def __init__(self):
        import torch
        self.torch, self.stream = torch, torch.cuda.Stream()
        if not self._sleeps():
            self.scratch = torch.ones(1 << 24, dtype=torch.float32, device=DEV)
            self.scratch2 = torch.empty_like(self.scratch)
        torch.cuda.synchronize()
        self.units = 10
        self._measure()                                   # warm-up: the first launch of the delay kernel
        ms = self._measure()
        for _attempt in range(5):
            if 50.0 <= ms <= 200.0:
                break
            self.units = max(1, int(self.units * min(200.0, 100.0 / max(ms, 1e-3))))   # (a step of 200 x at most)
            ms = self._measure()
        self.ms = ms
        print("producer delay: %.1f ms (%d units of %s)" % (ms, self.units, "torch.cuda._sleep(10^5 cycles)" if self._sleeps() else "a 2^24 cumsum"))
        assert 50.0 <= ms <= 200.0, "the delay could not be sized: %.1f ms" % ms

    def _sleeps(self):
        return hasattr(self.torch.cuda, "_sleep")

    def enqueue_delay(self):
        """On the current torch stream."""
        if self._sleeps():
            self.torch.cuda._sleep(self.units * 100000)
        else:
            for _ in range(self.units):
                self.torch.cumsum(self.scratch, 0, out=self.scratch2)

    def _measure(self):
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(self.stream):
            a.record()
            self.enqueue_delay()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def late_write(self, guarded, fresh):
        """The delay, then payload <- fresh (a device tensor), both on the producer's stream; returns at once."""
        with self.torch.cuda.stream(self.stream):
            self.enqueue_delay()
            guarded.payload.copy_(fresh, non_blocking=True)


@pytest.fixture(scope="module")
def producer(ctx):
    p = _Producer()
    yield p
    _sync()


def _race(ctx, producer, on_callers_stream, guarded, fresh, call):
    """guarded holds the STALE input; the fresh one is written late on the producer's stream and `call` made at once, no host
    synchronisation in between.  The context is on the producer's stream, or (the control) on its own."""
    import torch
    d_fresh = torch.from_numpy(np.ascontiguousarray(fresh).reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    if on_callers_stream:
        ctx.set_stream(producer.stream.cuda_stream)
    try:
        producer.late_write(guarded, d_fresh)
        return call()
    finally:
        torch.cuda.synchronize()
        if on_callers_stream:
            ctx.set_stream(None)


@pytest.mark.parametrize("on_callers_stream", [True, False], ids=["callers_stream", "own_stream_control"])
def test_solve_orders_itself_on_the_callers_stream(ctx, producer, on_callers_stream):
    """d_F holds load case 1; load case 0 arrives behind a delay on the caller's stream.  On that stream the solve has the
    bits of U(F_0).  The control -- the context on its own stream, nothing synchronised -- has the bits of U(F_1): a stale read,
    a valid solve of a valid load vector, which shows that the delay is long enough for the first statement to mean
    something.  max_its bounds both."""
    job = P.job("cube6")
    F0, F1 = P.load_cases("cube6")[0], P.load_cases("cube6")[1]
    K = ctx.assemble_hex8(*_host_args(job))
    try:
        K.cg_solve(F0, 1e-8, 3)                                       # (the first solve scales the matrix: every solve compared runs on the scaled one)
        (U0, rep0), (U1, rep1) = K.cg_solve(F0, 1e-8, 200), K.cg_solve(F1, 1e-8, 200)
        assert U0.tobytes() != U1.tobytes()
        dF, dU = _vec("F", F1, job.n_dof, 0), _out("U", job.n_red, job.n_dof, 0)
        got = _race(ctx, producer, on_callers_stream, dF, F0, lambda: K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8, 200))
    finally:
        K.free()
    B.check([dU])
    assert dF.numpy().tobytes() == F0.tobytes()                       # the late write did arrive
    bits = dU.numpy().tobytes()
    which = "U(F_0)" if bits == U0.tobytes() else "U(F_1), the stale vector" if bits == U1.tobytes() else "neither U(F_0) nor U(F_1)"
    if on_callers_stream:
        assert bits == U0.tobytes() and got == rep0, "the solve returned " + which
    else:
        assert bits == U1.tobytes() and got == rep1, \
            "the control returned %s: if it did not read stale data, lengthen the delay (%.1f ms)" % (which, producer.ms)


@pytest.mark.parametrize("on_callers_stream", [True, False], ids=["callers_stream", "own_stream_control"])
def test_assembly_orders_itself_on_the_callers_stream(ctx, producer, on_callers_stream):
    """d_xyz holds the unjittered cube; the jittered coordinates arrive late."""
    job = _job("cube3mixed")
    plain = cube_mesh(3)[0]
    assert plain.shape == job.xyz.shape and plain.tobytes() != job.xyz.tobytes()
    want = {}
    for key, xyz in (("fresh", job.xyz), ("stale", plain)):
        K = ctx.assemble_hex8(*_host_args(job, xyz=xyz))
        try:
            want[key] = _describe(K)
        finally:
            K.free()
    assert want["fresh"]["csr"][2].tobytes() != want["stale"]["csr"][2].tobytes()
    mesh = B.Mesh(job, DEV, xyz=plain)

    def call():
        K = ctx.assemble_hex8_dev(*mesh.assemble_args())
        try:
            return _describe(K)
        finally:
            K.free()
    got = _race(ctx, producer, on_callers_stream, mesh.xyz, job.xyz, call)
    assert mesh.xyz.numpy().tobytes() == job.xyz.tobytes()
    B.check([a for a in mesh.inputs if a is not mesh.xyz])
    _assert_same_matrix(got, want["fresh" if on_callers_stream else "stale"])


@pytest.mark.parametrize("on_callers_stream", [True, False], ids=["callers_stream", "own_stream_control"])
def test_recovery_orders_itself_on_the_callers_stream(ctx, producer, on_callers_stream):
    """d_disp holds another displacement field; the one asked for arrives late."""
    m, disp = _recovery_model("33")
    other = forces_ref.random_disp(m, 77)
    want = {"fresh": ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu),
            "stale": ctx.recover_hex8(m.xyz, other, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)}
    assert want["fresh"][0].tobytes() != want["stale"][0].tobytes()
    mesh = B.Mesh(m, DEV, disp=other)
    d_strain, d_stress = _out("strain", 48 * 33, m.n_dof, 0), _out("stress", 48 * 33, m.n_dof, 0)
    _race(ctx, producer, on_callers_stream, mesh.disp, disp, lambda: _recover_dev(ctx, mesh, d_strain, d_stress))
    B.check([d_strain, d_stress] + [a for a in mesh.inputs if a is not mesh.disp])
    strain, stress = want["fresh" if on_callers_stream else "stale"]
    assert d_strain.numpy().tobytes() == strain.tobytes() and d_stress.numpy().tobytes() == stress.tobytes()


def test_switching_streams_keeps_the_bits_and_the_pool(ctx):
    """Own stream, the caller's, own, the caller's again: a solve after each switch on a matrix that lives across them, an
    assembly cycle on each stream.  Every solve has the same bits; set_stream itself parks and releases nothing."""
    import torch
    job = P.job("cube6")
    s = torch.cuda.Stream()
    mesh = B.Mesh(job, DEV)
    dF, dU = _vec("F", job.F, job.n_dof, 0), _out("U", job.n_red, job.n_dof, 0)
    _sync()
    K = ctx.assemble_hex8(*_host_args(job))
    seen = []
    try:
        K.cg_solve(job.F, 1e-8, 3)                                    # (scales the matrix)
        U, rep = K.cg_solve(job.F, 1e-8)
        for stream in (None, s, None, s):
            before = ctx.pool_info()
            ctx.set_stream(None if stream is None else stream.cuda_stream)
            assert ctx.pool_info() == before
            dU.refill()
            _sync()
            got = K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8)
            K2 = ctx.assemble_hex8_dev(*mesh.assemble_args())
            try:
                info2 = K2.info()
            finally:
                K2.free()
            _sync()
            B.check(mesh.inputs + [dF, dU])
            seen.append((dU.numpy().tobytes(), got, info2))
            parked_bytes, parked_blocks = ctx.pool_info()
            assert parked_bytes >= 0 and parked_blocks >= 0 and (parked_bytes == 0) == (parked_blocks == 0)
    finally:
        ctx.set_stream(None)
        K.free()
    assert all(x == seen[0] for x in seen) and seen[0][0] == U.tobytes() and seen[0][1] == rep


def test_a_multi_device_handle_refuses_device_pointers_and_streams(built_libs):
    """stan_hip_init_multi with ONE device needs no communicator; the handle takes the host entries and returns
    STAN_E_UNSUPPORTED from set_stream and from the four device-pointer entries, before it touches an argument."""
    import torch
    job = problem.cube_job(2)
    group = hip.Context(devices=[0])
    try:
        mesh = B.Mesh(job, DEV, disp=np.zeros_like(job.xyz))
        dF, dU = _vec("F", np.tile(job.F, 2), job.n_dof, 0), _out("U", 2 * job.n_red, job.n_dof, 0)
        d_strain, d_stress = _out("strain", 48 * 8, job.n_dof, 0), _out("stress", 48 * 8, job.n_dof, 0)
        _sync()
        K = group.assemble_hex8(*_host_args(job))
        try:
            U, rep = K.cg_solve(job.F, 1e-8)
            assert rep["terminationtype"] in (1, 7) and U.any()
            calls = {"set_stream": lambda: group.set_stream(torch.cuda.Stream().cuda_stream),
                     "assemble_hex8_dev": lambda: group.assemble_hex8_dev(*mesh.assemble_args()),
                     "cg_solve_dev": lambda: K.cg_solve_dev(dF.ptr, dU.ptr, 1e-8),
                     "cg_solve_multi_dev": lambda: K.cg_solve_multi_dev(dF.ptr, dU.ptr, 2, 1e-8),
                     "recover_hex8_dev": lambda: group.recover_hex8_dev(*mesh.recover_args(), d_strain.ptr, d_stress.ptr)}
            for what, call in calls.items():
                with pytest.raises(hip.StanHipError) as ei:
                    call()
                assert ei.value.code == hip.E_UNSUPPORTED, what
        finally:
            K.free()
        _sync()
        outs = [dU, d_strain, d_stress]
        B.check(mesh.inputs + [dF] + outs, written=False)
        assert all("never written" in a.problems()[0] and str(a.n) in a.problems()[0] for a in outs)   # nothing ran
    finally:
        group.close()


def test_the_guard_check_sees_what_the_device_writes(ctx):
    """The harness on the GPU: d_U given as the payload's address minus 8 bytes.  The write stays inside the allocation, the
    checker reports the front guard (and the last payload entry as never written)."""
    job = problem.cube_job(1)
    K = ctx.assemble_hex8(*_host_args(job))
    try:
        K.cg_solve(job.F, 1e-8, 1)                                    # (scales the matrix)
        U, _rep = K.cg_solve(job.F, 1e-8)
        dF, dU = _vec("F", job.F, job.n_dof, 0), _out("U", job.n_red, job.n_dof, 0)
        _sync()
        K.cg_solve_dev(dF.ptr, dU.ptr - 8, 1e-8)
    finally:
        K.free()
    _sync()
    found = dU.problems()
    assert len(found) == 2 and "front guard, 1 entries, payload indices -1 .. -1" in found[0], found
    assert "1 payload entries never written, the first at %d" % (job.n_red - 1) in found[1], found
    assert dU.alloc[dU.start - 1:dU.start + job.n_red - 1].cpu().numpy().tobytes() == U.tobytes()


# ---- a rank that passes only its own elements ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,spec", [(2, "12"), (3, "12"), (4, "fuzz:101")])
def test_a_rank_that_passes_only_its_elements_gets_the_host_entry_bits(built_libs, tmp_path, world, spec, fake_mode):
    """bench.py --gpus N's path (tests/sharded_dev_worker.py): every rank checks its device-pointer assembly and solve against
    its host entries, bit for bit, with guarded arrays; here: every rank ended well and all hold the same U.  In fuzz:101
    rank 0 owns no rows."""
    out = _torchrun(world, [os.path.join(ROOT, "tests", "sharded_dev_worker.py"), spec, str(tmp_path)], fake_rccl_env(fake_mode),
                    timeout=150, attempts=1)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    print("".join(l + "\n" for l in out.stdout.splitlines() if l.startswith("rank ")), end="")
    assert (ASYNC_BANNER in out.stderr) == (fake_mode == "async")
    r0 = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    assert r0["U"].any() and int(r0["term"]) in (1, 7)
    picked = 0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert d["U"].tobytes() == r0["U"].tobytes() and int(d["its"]) == int(r0["its"]) and int(d["term"]) == int(r0["term"])
        picked += int(d["n_picked"])
    assert picked >= int(r0["n_elem"])                                # boundary elements are held by both owners
