"""Internal forces, support reactions and the equilibrium sums on the GPU (stan_hip_internal_forces_hex8) against
tests/forces_ref.py: f_ref = sum_e K_e u_e accumulated in longdouble from the oracle's element matrices, the rounding scale
a = sum_e |K_e| |u_e|, and rho = max_i |f_i - f_ref_i| / (2^-52 a_i).  The kernel is held to rho_gpu <= 4 rho_np, rho_np the
worst rho of the plain-fp64 numpy restatement of the same Gauss-point form over the same inputs (forces_ref.rho_np).

Measured on an MI355X when the tests were written: rho_np 5.41 (the 31-element strip; cap 21.63); rho_gpu per case -- strips of
1, 7, 8, 9, 31, 33 elements 0.71, 1.06, 3.57, 1.88, 9.29, 11.41; cubes 3^3 1.11, 5^3 3.76; mixed G1/G2 4^3 1.46; revolved 1.36;
star 3.11; rigid motion on the 5^3 cube: |f_int| at most 0.21 units of 2^-52 a."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import problem
from tests import forces_ref as R
from tests import scalars_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
U52 = R.U52


def forces(ctx, m, disp, F=None, **kw):
    return ctx.internal_forces_hex8(m.xyz, disp, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, F, **kw)


@pytest.fixture(scope="module")
def rho_np():
    return R.rho_np(verbose=True)


PARITY = ["strip%d" % n for n in R.STRIPS] + ["cube3", "cube5", "mixed4", "revolved", "star"]


@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_reference(gpu_ctx, rho_np, name):
    m, disp = R.cases()[name]
    f_ref, a = R.reference(m, disp)
    f_int, reaction, eq = forces(gpu_ctx, m, disp)
    rho = R.rho(f_int, f_ref, a)
    print("%s: rho_gpu %.2f (numpy restatement on this case %.2f; rho_np %.2f, cap %.2f)" % (name, rho, R._rho_np[name], rho_np, 4 * rho_np))
    assert np.isfinite(f_int).all() and rho <= 4 * rho_np
    fixed = m.red == -1
    assert np.abs(disp.reshape(-1)[m.red[np.asarray(m.node_dof).reshape(-1)] == -1]).min() > 0      # non-zero at fixed DOFs too
    assert np.array_equal(reaction, np.where(fixed, f_int, 0.0)) and eq.n_fixed == int(fixed.sum()) == m.n_fixed
    if name == "revolved":      # the axis node is named twice by each of its 72 wedges: 144 incidences, both corners count
        nd, cnt = np.unique(m.conn, return_counts=True)
        assert cnt.max() == 144 and m.conn[0, 0] == m.conn[0, 3]
    if name == "star":
        assert np.unique(m.conn, return_counts=True)[1].max() == 14
    if name == "mixed4":
        assert set(m.elem_type.tolist()) == {1, 2} and set(m.elem_mat.tolist()) == {0, 1}


def test_rigid_motion_gives_no_force(gpu_ctx, rho_np):
    """u = t + w x X on the jittered 5^3 cube: every entry cancels to rounding."""
    m, disp = R.cases()["rigid5"]
    f_ref, a = R.reference(m, disp)
    f_int, _, _ = forces(gpu_ctx, m, disp, reaction=False, eq=False)
    worst = float((np.abs(f_int) / (U52 * a)).max())
    print("rigid motion: max |f_int| = %.2f units of 2^-52 a (cap %.2f); max a %.3e" % (worst, 4 * rho_np, a.max()))
    assert (np.abs(f_int) <= 4 * rho_np * U52 * a).all() and a.min() > 0


@pytest.mark.parametrize("name", ["cube5", "mixed4", "revolved"])
def test_global_balance_for_any_displacement(gpu_ctx, rho_np, name):
    """fint_sum[c] is zero up to rounding for random u, no solve; with F = NULL the load sums are 0 and the residual is f_int."""
    m, disp = R.cases()[name]
    _, a = R.reference(m, disp)
    f_int, _, eq = forces(gpu_ctx, m, disp)
    print("%s: fint_sum %s, bound %.3e" % (name, list(eq.fint_sum), 4 * rho_np * U52 * a.sum()))
    for c in range(3):
        assert abs(eq.fint_sum[c]) <= 4 * rho_np * U52 * a.sum()
    assert list(eq.load_sum) == [0.0, 0.0, 0.0] and eq.load_norm2 == 0.0
    free = m.red != -1
    assert eq.residual_max == np.abs(f_int[free]).max()
    assert eq.residual_max_dof == int(np.nonzero(free)[0][np.argmax(np.abs(f_int[free]))])
    assert np.isclose(eq.residual_norm2, np.linalg.norm(f_int[free]), rtol=1e-13, atol=0)
    d = np.asarray(m.node_dof).reshape(-1, 3)
    for c in range(3):
        want = f_int[d[:, c]][m.red[d[:, c]] == -1].sum()
        assert np.isclose(eq.reaction_sum[c], want, rtol=0, atol=m.n_dof * 2.0 ** -53 * np.abs(f_int).sum())


@pytest.fixture(scope="module")
def solved(gpu_ctx):
    """4^3 and jittered 6^3 (clamp x = 0, (0, 0, 50) on x = n) solved with eps_f 1e-12, merit stop off."""
    from stan_amd import hip, host
    out = {}
    gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
    try:
        for n, jit in ((4, 0.0), (6, 0.1), (5, 0.1)):
            job = problem.cube_job(n, jitter=jit)
            K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
            U, rep = K.cg_solve(job.F, 1e-12)
            diag = K.diagonal()
            K.free()
            disp = host.nodal_displacements(job.node_dof, job.red, U).reshape(-1, 3)
            out[n] = (job, U, rep, diag, disp)
    finally:
        gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 1)
    return out


@pytest.mark.parametrize("n", [4, 6])
def test_equilibrium_after_a_solve(gpu_ctx, rho_np, solved, n):
    """r = S^-1 r_s gives |r| / |F| <= sqrt(max d / min d) rel_residual for the loop's residual; on top of it the rounding of
    f_int (4 rho_np units of 2^-52 a) and of the loop's own residual against b - A x: one product of the last refresh
    (a row of K has at most 81 entries: 81 x 2^-53 |K||U| <= 41 units of a), doubled for the at most 10 recurrence steps
    since.  reaction + load = sum of the free residuals (Cauchy-Schwarz: sqrt(N) |r|) + fint_sum (4 rho_np units of sum a)
    + the rounding of three sums of at most n_dof terms in any order (n_dof 2^-53 (sum |f_int| + sum |F|))."""
    job, U, rep, diag, disp = solved[n]
    _, a = R.reference(job, disp)
    f_int, reaction, eq = forces(gpu_ctx, job, disp, job.F)
    free = job.red != -1
    N = int(free.sum())
    units = (4 * rho_np + 2 * 41) * U52
    lhs = eq.residual_norm2 / eq.load_norm2
    rhs = np.sqrt(diag.max() / diag.min()) * rep["rel_residual"] + units * np.linalg.norm(a[free]) / eq.load_norm2
    print("n=%d: its %d type %d rel_residual %.3e; |F - f_int| / |F| = %.3e <= %.3e (rounding part %.3e)" %
          (n, rep["iterations"], rep["terminationtype"], rep["rel_residual"], lhs, rhs, units * np.linalg.norm(a[free]) / eq.load_norm2))
    assert lhs <= rhs and rhs < 1e-6
    rounding = 4 * rho_np * U52 * a.sum() + job.n_dof * 2.0 ** -53 * (np.abs(f_int).sum() + np.abs(job.F).sum())
    for c in range(3):
        print("   direction %d: reaction %.9e + load %.9e = %.3e <= %.3e" % (c, eq.reaction_sum[c], eq.load_sum[c],
              eq.reaction_sum[c] + eq.load_sum[c], np.sqrt(N) * eq.residual_norm2 + rounding))
        assert abs(eq.reaction_sum[c] + eq.load_sum[c]) <= np.sqrt(N) * eq.residual_norm2 + rounding
    assert eq.load_sum[2] == 50.0 * (n + 1) ** 2 and eq.load_sum[0] == 0.0 and eq.load_sum[1] == 0.0
    assert eq.n_fixed == job.n_fixed == 3 * (n + 1) ** 2
    assert np.isclose(eq.load_norm2, np.linalg.norm(job.F), rtol=1e-14, atol=0)
    assert 0 <= eq.residual_max_dof < job.n_dof and free[eq.residual_max_dof]
    Ffull = np.zeros(job.n_dof); Ffull[free] = job.F
    assert eq.residual_max == np.abs(Ffull - f_int)[free].max()
    assert np.array_equal(reaction, np.where(free, 0.0, f_int))


def test_bits(gpu_ctx, solved):
    """Same bytes from two calls, with an assembly and a solve on the context in between, whichever outputs are asked for,
    and from the device-pointer entry."""
    import torch
    m, disp = R.cases()["revolved"]
    f1, r1, e1 = forces(gpu_ctx, m, disp, m.F)
    f2, r2, e2 = forces(gpu_ctx, m, disp, m.F)
    assert f1.tobytes() == f2.tobytes() and r1.tobytes() == r2.tobytes() and bytes(e1) == bytes(e2)
    job = problem.cube_job(4, jitter=0.1)
    K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    K.cg_solve(job.F, 1e-8)
    K.free()
    f3, r3, e3 = forces(gpu_ctx, m, disp, m.F)
    assert f1.tobytes() == f3.tobytes() and r1.tobytes() == r3.tobytes() and bytes(e1) == bytes(e3)
    f4, none_r, none_e = forces(gpu_ctx, m, disp, m.F, reaction=False, eq=False)
    assert none_r is None and none_e is None and f4.tobytes() == f1.tobytes()
    none_f, r5, none_e = forces(gpu_ctx, m, disp, m.F, f_int=False, eq=False)
    assert none_f is None and r5.tobytes() == r1.tobytes()
    none_f, none_r, e6 = forces(gpu_ctx, m, disp, m.F, f_int=False, reaction=False)
    assert none_f is None and none_r is None and bytes(e6) == bytes(e1)
    # device pointers
    dev = torch.device("cuda:0")
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    dx, du, dd = t(m.xyz, np.float64), t(disp, np.float64), t(m.node_dof, np.int32)
    dc, dm, dty, dr, dF = t(m.conn, np.int32), t(m.elem_mat, np.int32), t(m.elem_type, np.uint8), t(m.red, np.int32), t(m.F, np.float64)
    dfi = torch.full((m.n_dof,), float("nan"), dtype=torch.float64, device=dev)
    dre = torch.full((m.n_dof,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    e7 = gpu_ctx.internal_forces_hex8_dev(m.xyz.shape[0], dx.data_ptr(), du.data_ptr(), dd.data_ptr(), m.conn.shape[0], dc.data_ptr(),
                                          dm.data_ptr(), dty.data_ptr(), m.mat_E_nu, m.n_dof, dr.data_ptr(), dF.data_ptr(),
                                          dfi.data_ptr(), dre.data_ptr())
    assert dfi.cpu().numpy().tobytes() == f1.tobytes() and dre.cpu().numpy().tobytes() == r1.tobytes() and bytes(e7) == bytes(e1)


def test_not_the_quirk_of_nodal_forces(gpu_ctx, rho_np, solved):
    """stan_hip_nodal_forces_hex8 keeps the reference's quirk (the node-extrapolated stress used as Gauss-point stress): on a
    solved jittered cube its R is not K u, f_int is.  For a constant-strain field u = A x the quirk vanishes (the
    extrapolation of a constant is the constant): the two agree with each other and with f_ref.  R's bound there: f_int's
    (the same Gauss-point form: 4 rho_np units of 2^-52 a), plus the extrapolation's rounding carried into the forces.  The
    extrapolation is three stages of two rounded operations on values magnified by (|ca| + |cb|)^3 = 3 sqrt 3, i.e. a
    relative error of 6 x 3 sqrt 3 x 2^-53 < 16 x 2^-52 of the (constant) stress at each Gauss point; a relative error of the
    Gauss-point stresses enters the forces multiplied by s = sum_g |B_g^T| |sig_g| |det J_g w| (forces_ref.fint_gauss,
    scale=True), so |R - f_ref| <= 2^-52 (4 rho_np a + 16 s), and |f_int - R| <= 2^-52 (8 rho_np a + 16 s)."""
    job, U, rep, diag, disp = solved[5]
    f_ref, a = R.reference(job, disp)
    f_int, _, _ = forces(gpu_ctx, job, disp, reaction=False, eq=False)
    _, Rq = gpu_ctx.nodal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    apart = float((np.abs(f_int - Rq) / (U52 * a)).max())
    print("solved 5^3: rho(f_int) %.2f; |f_int - R| up to %.3e units of 2^-52 a" % (R.rho(f_int, f_ref, a), apart))
    assert R.rho(f_int, f_ref, a) <= 4 * rho_np and apart > 1e6
    A = np.array([[1.0e-3, 2.0e-4, -3.0e-4], [1.5e-4, -7.0e-4, 2.5e-4], [-1.0e-4, 3.0e-4, 5.0e-4]])
    lin = job.xyz @ A.T
    f_ref, a = R.reference(job, lin)
    f_int, _, _ = forces(gpu_ctx, job, lin, reaction=False, eq=False)
    _, Rq = gpu_ctx.nodal_forces_hex8(job.xyz, lin, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    _, s = R.fint_gauss(job, lin, scale=True)
    capR = U52 * (4 * rho_np * a + 16 * s)
    errR, gap = np.abs(Rq.astype(np.longdouble) - f_ref).astype(np.float64), np.abs(f_int - Rq)
    print("u = A x: rho(f_int) %.2f (cap %.2f), rho(R) %.2f; max |R - f_ref| / cap %.3f, max |f_int - R| / cap %.3f; s / a up to %.2f" %
          (R.rho(f_int, f_ref, a), 4 * rho_np, R.rho(Rq, f_ref, a), (errR / capR).max(), (gap / (capR + U52 * 4 * rho_np * a)).max(),
           (s / a).max()))
    assert R.rho(f_int, f_ref, a) <= 4 * rho_np and a.min() > 0
    assert (errR <= capR).all()
    assert (gap <= capR + U52 * 4 * rho_np * a).all()


def _with(job, **kw):
    import copy
    j = copy.copy(job)
    for k, v in kw.items():
        setattr(j, k, np.ascontiguousarray(v).reshape(np.asarray(getattr(job, k)).shape))
    return j


def test_errors(gpu_ctx):
    from stan_amd import hip
    job = problem.cube_job(3)
    disp = R.random_disp(job, 9)

    def code(**kw):
        j = kw.pop("job", job)
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.internal_forces_hex8(kw.pop("xyz", j.xyz), disp, j.node_dof, kw.pop("conn", j.conn), kw.pop("elem_mat", j.elem_mat),
                                         kw.pop("elem_type", j.elem_type), j.mat_E_nu, j.red, **kw)
        return ei.value.code
    xyz = job.xyz.copy()
    xyz[job.conn[5]] = xyz[job.conn[5]] * [1, 1, 0]       # flatten one element: det J == 0
    assert code(xyz=xyz) == hip.E_DETJ and gpu_ctx.last_bad_element() == 5
    bad = job.conn.copy(); bad[7, 3] = job.xyz.shape[0]
    assert code(conn=bad) == hip.E_ARG
    bad[7, 3] = -1
    assert code(conn=bad) == hip.E_ARG
    mat = job.elem_mat.copy(); mat[11] = 1
    assert code(elem_mat=mat) == hip.E_ARG
    typ = job.elem_type.copy(); typ[2] = 3
    assert code(elem_type=typ) == hip.E_ARG
    assert code(f_int=False, reaction=False, eq=False) == hip.E_ARG           # all outputs NULL
    # Node.DOF: a node whose three DOFs are not consecutive, two nodes that name the same three
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[4, [1, 2]] = dof[4, [2, 1]]
    assert code(job=_with(job, node_dof=dof)) == hip.E_DOF_LAYOUT
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[9] = dof[20]
    assert code(job=_with(job, node_dof=dof)) == hip.E_DOF_LAYOUT
    # ndof_reduction: neither -1 nor within [0, i]
    free = int(np.nonzero(job.red != -1)[0][3])
    for v in (-2, free + 1):
        red = job.red.copy(); red[free] = v
        assert code(job=_with(job, red=red)) == hip.E_ARG
    # the same bad integers in DEVICE memory are caught by the library's device-side check, before anything is indexed
    import torch
    dev = torch.device("cuda:0")
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    dx, du, dd = t(job.xyz, np.float64), t(disp, np.float64), t(job.node_dof, np.int32)
    dm, dty, dr = t(job.elem_mat, np.int32), t(job.elem_type, np.uint8), t(job.red, np.int32)
    bad[7, 3] = 1 << 30
    dc = t(bad, np.int32)
    torch.cuda.synchronize()
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.internal_forces_hex8_dev(job.xyz.shape[0], dx.data_ptr(), du.data_ptr(), dd.data_ptr(), job.conn.shape[0], dc.data_ptr(),
                                         dm.data_ptr(), dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr())
    assert ei.value.code == hip.E_ARG
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[9] = dof[20]
    dd2, dc = t(dof, np.int32), t(job.conn, np.int32)
    torch.cuda.synchronize()
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.internal_forces_hex8_dev(job.xyz.shape[0], dx.data_ptr(), du.data_ptr(), dd2.data_ptr(), job.conn.shape[0], dc.data_ptr(),
                                         dm.data_ptr(), dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr())
    assert ei.value.code == hip.E_DOF_LAYOUT
    # F == NULL is accepted; the context is still usable
    f_int, reaction, eq = forces(gpu_ctx, job, disp)
    assert list(eq.load_sum) == [0.0, 0.0, 0.0] and eq.load_norm2 == 0.0 and np.isfinite(f_int).all()


def test_multi_device_handle_is_refused(built_libs):
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from stan_amd import hip, problem
job = problem.cube_job(3)
disp = np.random.default_rng(1).standard_normal(job.xyz.shape) * 1e-3
ctx = hip.Context(devices=[0, 0])
try:
    ctx.internal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red, job.F)
    print("HOST NOERROR")
except hip.StanHipError as e:
    print("HOST", e.code, "multi-device" in str(e))
t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to("cuda:0")
dx, du, dd, dc = t(job.xyz, np.float64), t(disp, np.float64), t(job.node_dof, np.int32), t(job.conn, np.int32)
dm, dty, dr = t(job.elem_mat, np.int32), t(job.elem_type, np.uint8), t(job.red, np.int32)
torch.cuda.synchronize()
try:
    ctx.internal_forces_hex8_dev(job.xyz.shape[0], dx.data_ptr(), du.data_ptr(), dd.data_ptr(), job.conn.shape[0], dc.data_ptr(),
                                 dm.data_ptr(), dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr())
    print("DEV NOERROR")
except hip.StanHipError as e:
    print("DEV", e.code, "multi-device" in str(e))
ctx.close()
print("CLOSED")
''' % ROOT
    env = dict(os.environ, STAN_RCCL_LIB=FAKE)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert "HOST -8 True" in lines and "DEV -8 True" in lines and "CLOSED" in lines, p.stdout


def _write_model(path, n):
    from stan_amd import host
    from stan_amd.cube import cube_bcs, cube_mesh
    xyz, conn = cube_mesh(n, jitter=0.1)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", 210000.0, 0.3)
    d.assign_part(1, 1, "HEX8_G2")
    spc, ld, f = cube_bcs(n)
    d.add_bc(1, "fix", "SPC", spc + 1, np.ones((len(spc), 3)))
    d.add_bc(2, "load", "PointLoad", ld + 1, np.tile(f, (len(ld), 1)))
    d.set_analysis(tol=1e-10)
    d.write_stdb(path)


def test_console_driver_reactions(gpu_ctx, tmp_path):
    """stan_solver --reactions --json --vtu on a 4^3 model: the "equilibrium" object is the binding's result for the U the
    run stored; the .STdb is the one a run without the flag writes; the .vtu carries three more point arrays."""
    from stan_amd import host
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    plain, path = str(tmp_path / "plain.STdb"), str(tmp_path / "model.STdb")
    _write_model(plain, 4)
    _write_model(path, 4)
    out0 = subprocess.run([exe, "--json", plain], capture_output=True, text=True, timeout=300)
    assert out0.returncode == 0, out0.stdout + out0.stderr
    assert "equilibrium" not in out0.stdout and "reactions" not in out0.stdout.lower()
    out = subprocess.run([exe, "--reactions", "--json", "--vtu", str(tmp_path / "out"), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == open(plain, "rb").read()          # the .STdb does not know about --reactions
    for word in ("Support reactions:", "Applied load:", "Out of balance:", "Largest:"):
        assert word in out.stdout, out.stdout
    js = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    js0 = json.loads([l for l in out0.stdout.splitlines() if l.startswith("{")][0])
    assert set(js) - set(js0) == {"equilibrium"}
    q = js["equilibrium"]
    job = problem.cube_job(4, jitter=0.1)
    disp = host.Db.read_stdb(path).results(1)[0]
    f_int, reaction, eq = forces(gpu_ctx, job, disp, job.F)
    for k in ("reaction_sum", "load_sum", "fint_sum"):
        assert q[k] == list(getattr(eq, k)), k
    for k in ("residual_norm2", "load_norm2", "residual_max", "residual_max_dof", "n_fixed"):
        assert q[k] == getattr(eq, k), k
    assert q["load_sum"][2] == 50.0 * 25 and q["residual_norm2"] < 1e-6 * q["load_norm2"]
    _, _, arr = S.parse_vtu(str(tmp_path / "out_001.vtu"))
    names = [n for n, _, _ in arr["PointData"]]
    assert names == S.NAMES + ["Reaction Force X", "Reaction Force Y", "Reaction Force Z"]
    d = np.asarray(job.node_dof).reshape(-1, 3)
    for c in range(3):
        got = arr["PointData"][24 + c][1]
        assert got.dtype == np.dtype("<f4") and np.array_equal(got, reaction[d[:, c]].astype(np.float32))
    assert np.abs(arr["PointData"][26][1]).max() > 0
    # --vtu without the flag: the 24 arrays, as before
    _write_model(path, 4)
    out = subprocess.run([exe, "--vtu", str(tmp_path / "p"), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and [n for n, _, _ in S.parse_vtu(str(tmp_path / "p_001.vtu"))[2]["PointData"]] == S.NAMES
