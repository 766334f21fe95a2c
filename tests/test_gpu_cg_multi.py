"""Several load cases in one CG loop over a single pass of K (stan_hip_cg_solve_multi, cg_multi.inc).

Every column is alglib's loop on its own data: with the single solve told to run the one form the batched loop has
(one wavefront per slice, literal refresh product, no folded rows) column j of a batched solve has the BITS of
cg_solve(F_j) -- which pins the batched loop to the loop the oracle fixtures already pin, with no tolerance to choose.
A difference in bits is a bug (summation order, a scalar's parity slot, a stopped column written again)."""
import numpy as np
import pytest

from stan_amd import problem

pytestmark = pytest.mark.gpu
U_TOL = 1e-6

# (eps_f, max_its, merit stop)
SETTINGS = {
    "1e-8_merit_off": (1e-8, 0, 0),
    "1e-3_merit_on": (1e-3, 0, 1),     # the columns stop 30-50 iterations apart: frozen columns
    "1e-10_merit_on": (1e-10, 0, 1),   # type 7: the previous point is returned
    "maxits_7": (1e-30, 7, 1),
    "maxits_31": (1e-30, 31, 1),       # refresh iterations (10, 20, 30) inside
}
_jobs, _singles = {}, {}


def _job(mesh):
    if mesh not in _jobs:
        if mesh == "perforated":
            job = problem.perforated_job(16, 0.4)
        elif mesh == "indefinite":
            job = problem.cube_job(3, E=-210000.0)
        else:
            job = problem.cube_job(int(mesh), jitter=0.05)
        _jobs[mesh] = job
    return _jobs[mesh]


def _columns(job):
    """The six load cases of the issue, seeded; column j of a wider solve is _columns[j % 6]."""
    rng = np.random.default_rng(11)
    N = job.F.shape[0]
    unit = np.zeros(N)
    unit[N // 3] = 1.0
    return [job.F.copy(), np.zeros(N), rng.standard_normal(N), 1e6 * job.F, unit, np.sin(0.01 * np.arange(N))]


def _assemble(ctx, job):
    return ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)


def _single_form_options(ctx, hip, on):
    """The single solve in the form the batched loop has (on) or back to its defaults (off)."""
    ctx.set_option(hip.OPT_SPMV_SMALL, 0 if on else 1)
    ctx.set_option(hip.OPT_CG_FUSED_REFRESH, 0 if on else 1)
    ctx.set_option(hip.OPT_ROW_FOLDING, 0 if on else -1)


def _defaults(ctx, hip):
    ctx.set_option(hip.OPT_CG_MERIT_STOP, 1)
    ctx.set_option(hip.OPT_CG_SINGLE_REDUCE, 0)


def _single_reference(ctx, hip, K, mesh, setting, cols):
    """cg_solve of each of the six columns, computed once per (mesh, setting) and left unchanged."""
    key = (mesh, setting)
    if key not in _singles:
        eps, maxits, _ = SETTINGS[setting]
        _singles[key] = [K.cg_solve(c, eps, max_its=maxits) for c in cols]
    return _singles[key]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mesh", ["10", "perforated"])
def test_columns_have_the_bits_of_the_single_solve(gpu_ctx, mesh, setting):
    from stan_amd import hip
    job = _job(mesh)
    cols = _columns(job)
    eps, maxits, merit = SETTINGS[setting]
    K = _assemble(gpu_ctx, job)
    try:
        gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, merit)
        _single_form_options(gpu_ctx, hip, True)
        ref = _single_reference(gpu_ctx, hip, K, mesh, setting, cols)
        print(mesh, setting, [(r["terminationtype"], r["iterations"]) for _, r in ref])
        assert ref[1][1]["iterations"] == 0 and ref[1][1]["terminationtype"] == 1     # the zero column
        if setting == "1e-3_merit_on":
            its = [r["iterations"] for _, r in ref if r["iterations"] > 0]
            assert max(its) - min(its) >= 10, its        # columns really stop at different iterations
        for n_rhs in (1, 2, 3, 5, 8, 11):
            F = np.stack([cols[j % 6] for j in range(n_rhs)])
            U, reps = K.cg_solve_multi(F, eps, max_its=maxits)
            for j in range(n_rhs):
                Us, rs = ref[j % 6]
                assert reps[j] == rs, (n_rhs, j, reps[j], rs)
                assert np.array_equal(U[j], Us), (n_rhs, j, float(np.abs(U[j] - Us).max()))
    finally:
        _single_form_options(gpu_ctx, hip, False)
        _defaults(gpu_ctx, hip)
        K.free()


def test_columns_have_the_bits_of_the_single_solve_40_cubed(gpu_ctx):
    """1077 slices = 270 workgroups: one full XCD-chunk window plus a ragged tail of the product's mapping."""
    from stan_amd import hip
    job = _job("40")
    cols = _columns(job)
    K = _assemble(gpu_ctx, job)
    try:
        gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
        _single_form_options(gpu_ctx, hip, True)
        pick = [0, 2, 1, 5]
        ref = [K.cg_solve(cols[j], 1e-8) for j in pick]
        U, reps = K.cg_solve_multi(np.stack([cols[j] for j in pick]), 1e-8)
        print([(r["terminationtype"], r["iterations"]) for r in reps])
        for j in range(4):
            assert reps[j] == ref[j][1], (j, reps[j], ref[j][1])
            assert np.array_equal(U[j], ref[j][0]), (j, float(np.abs(U[j] - ref[j][0]).max()))
        assert reps[0]["terminationtype"] == 1 and reps[0]["iterations"] > 300
    finally:
        _single_form_options(gpu_ctx, hip, False)
        _defaults(gpu_ctx, hip)
        K.free()


def test_a_column_does_not_depend_on_the_others(gpu_ctx):
    """Default options, 20^3: column j of an 11-column solve, of a 4-column solve with the columns permuted and of the
    1-column solve are bit-identical, and so are two runs of the same call."""
    job = _job("20")
    cols = _columns(job)
    K = _assemble(gpu_ctx, job)
    try:
        eps = 1e-8
        F11 = np.stack([cols[j % 6] for j in range(11)])
        U11, r11 = K.cg_solve_multi(F11, eps)
        U11b, r11b = K.cg_solve_multi(F11, eps)
        assert r11 == r11b and np.array_equal(U11, U11b)
        print([(r["terminationtype"], r["iterations"]) for r in r11])
        for j in range(6, 11):   # the repeated columns (groups of 8, 2, 1: other widths, other positions)
            assert r11[j] == r11[j - 6] and np.array_equal(U11[j], U11[j - 6]), j
        perm = [5, 0, 3, 2]
        U4, r4 = K.cg_solve_multi(np.stack([cols[j] for j in perm]), eps)
        for q, j in enumerate(perm):
            assert r4[q] == r11[j] and np.array_equal(U4[q], U11[j]), (q, j)
        for j in range(6):
            U1, r1 = K.cg_solve_multi(cols[j][None, :], eps)
            assert r1[0] == r11[j] and np.array_equal(U1[0], U11[j]), j
        assert len({r["iterations"] for r in r11[:6]}) > 2
    finally:
        K.free()


def test_against_the_oracle(gpu_ctx, oracle):
    """10^3 at eps 1e-12: every column within the project's north-star bar of the oracle's answer, iterations within
    the rule of test_gpu_cg_loops.py."""
    job = _job("10")
    cols = _columns(job)
    K = _assemble(gpu_ctx, job)
    rc, A = oracle.assemble(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red, n_threads=8)
    assert rc == 0
    try:
        U, reps = K.cg_solve_multi(np.stack(cols), 1e-12)
        for j, c in enumerate(cols):
            Uo, repo = oracle.cg(A, c, 1e-12)
            print(j, reps[j], repo)
            slack = max(3, repo["iterations"] // 50) if repo["terminationtype"] == 1 else max(5, repo["iterations"] // 4)
            assert abs(reps[j]["iterations"] - repo["iterations"]) <= slack, (j, reps[j], repo)
            assert np.abs(U[j] - Uo).max() <= U_TOL * np.abs(Uo).max(), j
    finally:
        K.free()


def test_codes(gpu_ctx):
    """An indefinite K: p.Ap <= 0 at the first iteration of the loaded columns (-5, previous point = 0), the zero
    column converged at iteration 0 -- each column's own code.  eps_f = max_its = 0 means 1e-6."""
    from stan_amd import hip
    job = _job("indefinite")
    N = job.F.shape[0]
    K = _assemble(gpu_ctx, job)
    try:
        U, reps = K.cg_solve_multi(np.stack([job.F, np.ones(N), np.zeros(N)]), 1e-8)
        assert [r["terminationtype"] for r in reps] == [-5, -5, 1], reps
        assert [r["iterations"] for r in reps] == [1, 1, 0], reps
        assert not U.any()
    finally:
        K.free()
    job = _job("10")
    cols = _columns(job)
    K = _assemble(gpu_ctx, job)
    try:
        gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
        F = np.stack(cols)
        U0, r0 = K.cg_solve_multi(F, 0.0, max_its=0)
        U6, r6 = K.cg_solve_multi(F, 1e-6, max_its=0)
        assert r0 == r6 and np.array_equal(U0, U6)
        for r in r0:
            assert r["terminationtype"] == 1 and r["rel_residual"] <= 1e-6, r
        assert sum(r["iterations"] > 50 for r in r0) == 5
    finally:
        _defaults(gpu_ctx, hip)
        K.free()


def test_refusals_and_the_single_solve_next_to_a_batched_one(gpu_ctx):
    from stan_amd import hip
    job = _job("10")
    cols = _columns(job)
    F = np.stack(cols[:3])
    K = _assemble(gpu_ctx, job)
    K2 = _assemble(gpu_ctx, job)
    try:
        U_alone, r_alone = K.cg_solve(job.F, 1e-8)          # a single solve that never saw a batched one
        assert K2.info()["scaled"] == 0
        Um, rm = K2.cg_solve_multi(F, 1e-8)                 # a batched solve on a fresh matrix
        assert K2.info()["scaled"] == 1
        for pm in (hip.PREC_MIXED, hip.PREC_FIXED48):
            with pytest.raises(hip.StanHipError) as ei:
                K2.cg_solve_multi(F, 1e-8, precision_mode=pm)
            assert ei.value.code == hip.E_UNSUPPORTED and "fp64" in str(ei.value)
        gpu_ctx.set_option(hip.OPT_CG_SINGLE_REDUCE, 1)
        try:
            with pytest.raises(hip.StanHipError) as ei:
                K2.cg_solve_multi(F, 1e-8)
            assert ei.value.code == hip.E_UNSUPPORTED and "single-reduction" in str(ei.value)
        finally:
            gpu_ctx.set_option(hip.OPT_CG_SINGLE_REDUCE, 0)
        with pytest.raises(hip.StanHipError) as ei:
            K2.cg_solve_multi(np.zeros((0, job.F.shape[0])), 1e-8)
        assert ei.value.code == hip.E_ARG
        # K solves normally afterwards: the single solve after a batched one has the bits it has alone, and the
        # batched solve after it its own
        U_after, r_after = K2.cg_solve(job.F, 1e-8)
        assert r_after == r_alone and np.array_equal(U_after, U_alone)
        Um2, rm2 = K2.cg_solve_multi(F, 1e-8)
        assert rm2 == rm and np.array_equal(Um2, Um)
        Um3, rm3 = K.cg_solve_multi(F, 1e-8)                # ... and on the matrix the single solve scaled
        assert rm3 == rm and np.array_equal(Um3, Um)
    finally:
        _defaults(gpu_ctx, hip)
        K.free()
        K2.free()
