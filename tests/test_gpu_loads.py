"""The load vector of distributed loads and prescribed displacements on the GPU (stan_hip_load_vector_hex8) against
tests/loads_ref.py: l_ref evaluated and scattered in longdouble, the rounding scale s = sum |N_a| |b| |det J| +
sum |p| N_a |n dA|_1, and rho = max_i |l_i - l_ref_i| / (2^-52 s_i).  The kernel is held to rho_gpu <= 4 rho_np, rho_np the
worst rho of the plain-fp64 numpy restatement of the same operation form over the same inputs (loads_ref.rho_np): FMA
contraction and the butterfly order of the point sums move the constant by a small factor, not by an order of magnitude.

volume and area are held to (n_elem + 8) x 2^-52 relative to the longdouble sums themselves: the issue's n_elem x 2^-52, plus
the eight rounded point terms that one element's sum is made of (a face has four) -- without them the bound is one unit for a
single element, which eight determinants with a rounding each and seven additions exceed even in the numpy restatement (1.44
units on the one-element strip).  The constant matters for the few-element cases only.

Measured on an MI355X when the tests were written: rho_np 15.84 (the 31-element strip with a body force; cap 63.35), worst
rho_gpu 8.55 (a single face on the last element of the 33-element strip); per case in profiles/r08/loads_n148.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import problem
from tests import forces_ref as R
from tests import loads_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
U52 = L.U52


def loads(ctx, m, case=None, **kw):
    a = dict(case.kw()) if case is not None else {}
    a.update(kw)
    return ctx.load_vector_hex8(m.xyz, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, **a)


def free_part(m, full):
    """[n_dof] -> [N] through the reduction map"""
    d = np.nonzero(m.red != -1)[0]
    out = np.zeros(m.n_dof - m.n_fixed)
    out[d - m.red[d]] = full[d]
    return out


@pytest.fixture(scope="module")
def rho_np():
    return L.rho_np(verbose=True)


@pytest.fixture(scope="module")
def rho_np_forces():
    return R.rho_np()


@pytest.mark.parametrize("name", sorted(L.cases()))
def test_parity_with_the_reference(gpu_ctx, rho_np, name):
    m, case = L.cases()[name]
    l_ref, vol_ref, area_ref = L.reference(m, case)
    s = L.scale(m, case)
    _, _, l, sums = loads(gpu_ctx, m, case)
    rho = L.rho(l, l_ref, s)
    ne = m.conn.shape[0]
    vtol, atol = (ne + 8) * U52 * abs(float(vol_ref)), (ne + 8) * U52 * abs(float(area_ref))
    print("%s: rho_gpu %.2f (numpy restatement on this case %.2f; rho_np %.2f, cap %.2f); volume error %.4f, area error %.4f "
          "of the bound (n_elem + 8) 2^-52 x the sum" % (name, rho, L._rho_np[name], rho_np, 4 * rho_np,
                                                        abs(sums.volume - vol_ref) / vtol if vtol else 0.0,
                                                        abs(sums.area - area_ref) / atol if atol else 0.0))
    assert np.isfinite(l).all() and rho <= 4 * rho_np
    assert (l[s == 0] == 0).all()                                   # nothing where no load reaches
    assert abs(sums.volume - vol_ref) <= vtol and abs(sums.area - area_ref) <= atol
    assert sums.n_faces == case.n_faces and sums.n_fixed == m.n_fixed
    if case.mat_body is None:
        assert sums.volume == 0.0
    if case.n_faces == 0:
        assert sums.area == 0.0


@pytest.mark.parametrize("name", ["cube5-surf", "revolved-surf", "mixed4-body", "strip33-sel"])
def test_F_semantics(gpu_ctx, name):
    """F_out = F_in + l as ONE fp64 add per entry; load_full is l; F_solve without disp0 is F_out (or l when F is NULL); the
    sums split into free and fixed parts."""
    m, case = L.cases()[name]
    F_in = np.random.default_rng(3).standard_normal(m.n_dof - m.n_fixed) * 7.0
    F_out, F_solve, l, sums = loads(gpu_ctx, m, case, F=F_in, F_solve=True)
    lf = free_part(m, l)
    assert F_out.tobytes() == (F_in + lf).tobytes() and F_solve.tobytes() == F_out.tobytes()
    none_F, F_solve2, l2, _ = loads(gpu_ctx, m, case, F_solve=True)
    assert none_F is None and F_solve2.tobytes() == lf.tobytes() and l2.tobytes() == l.tobytes()
    d = np.asarray(m.node_dof).reshape(-1, 3)
    tol = m.n_dof * 2.0 ** -53 * np.abs(l).sum()
    for c in range(3):
        fixed = m.red[d[:, c]] == -1
        assert abs(sums.load_sum[c] - l[d[:, c]].sum()) <= tol
        assert abs(sums.free_sum[c] - l[d[:, c]][~fixed].sum()) <= tol
        assert abs(sums.free_sum[c] + l[d[:, c]][fixed].sum() - sums.load_sum[c]) <= tol
    assert np.abs(l[m.red == -1]).max() > 0                        # some load does fall on supports


def test_bits(gpu_ctx):
    """Same bytes from two calls, from the device-pointer entry, for every subset of the outputs; a node's result does not
    change when faces elsewhere are added to the list."""
    import itertools
    import torch
    m, case = L.cases()["revolved-surf"]
    F_in = np.random.default_rng(4).standard_normal(m.n_dof - m.n_fixed)
    u0 = np.random.default_rng(5).standard_normal(m.xyz.shape) * 1e-3
    ref = loads(gpu_ctx, m, case, F=F_in, disp0=u0)
    again = loads(gpu_ctx, m, case, F=F_in, disp0=u0)
    for a, b in zip(ref, again):
        assert bytes(a) == bytes(b)
    assert ref[1].tobytes() != ref[0].tobytes()                    # disp0 does reach F_solve
    solve_only = loads(gpu_ctx, m, case, disp0=u0)[1]              # l - f_int(u0): F_solve when no F is given
    assert solve_only.tobytes() != ref[1].tobytes()
    for wF, wS, wL, wQ in itertools.product([False, True], repeat=4):
        if not (wF or wS or wL or wQ):
            continue
        disp0 = u0 if wS else None                                 # (disp0 needs F_solve)
        want = ref                                                 # F, load_full and sums do not depend on disp0
        got = loads(gpu_ctx, m, case, F=F_in if wF else None, disp0=disp0, F_solve=wS, load_full=wL, sums=wQ)
        for k, on in enumerate((wF, wS and wF, wL, wQ)):           # F_solve depends on F: two references
            if on:
                assert bytes(got[k]) == bytes(want[k]), (wF, wS, wL, wQ, k)
        if wS and not wF:
            assert got[1].tobytes() == solve_only.tobytes(), (wF, wS, wL, wQ)
        for k, on in enumerate((wF, wS, wL, wQ)):
            assert (got[k] is None) == (not on)
    # device pointers
    dev = torch.device("cuda:0")
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    dx, dd, dc = t(m.xyz, np.float64), t(m.node_dof, np.int32), t(m.conn, np.int32)
    dm, dty, dr = t(m.elem_mat, np.int32), t(m.elem_type, np.uint8), t(m.red, np.int32)
    dfe, dfi, dfp = t(case.face_elem, np.int32), t(case.face_id, np.uint8), t(case.face_p, np.float64)
    du, dF = t(u0, np.float64), t(F_in, np.float64)
    dFs = torch.full((F_in.shape[0],), float("nan"), dtype=torch.float64, device=dev)
    dl = torch.full((m.n_dof,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    q = gpu_ctx.load_vector_hex8_dev(m.xyz.shape[0], dx.data_ptr(), dd.data_ptr(), m.conn.shape[0], dc.data_ptr(), dm.data_ptr(),
                                     dty.data_ptr(), m.mat_E_nu, m.n_dof, dr.data_ptr(), case.mat_body, case.n_faces, dfe.data_ptr(),
                                     dfi.data_ptr(), dfp.data_ptr(), du.data_ptr(), dF.data_ptr(), dFs.data_ptr(), dl.data_ptr())
    assert dF.cpu().numpy().tobytes() == ref[0].tobytes() and dFs.cpu().numpy().tobytes() == ref[1].tobytes()
    assert dl.cpu().numpy().tobytes() == ref[2].tobytes() and bytes(q) == bytes(ref[3])
    # faces elsewhere: the 33-element strip with faces on element 8, then also on elements 31 and 32
    m, case = L.cases()["strip33-surf"]
    near = L.Case(case.mat_body, [8, 8], [2, 5], [1.5, -0.5])
    far = L.Case(case.mat_body, [8, 8, 31, 32, 32], [2, 5, 4, 1, 3], [1.5, -0.5, 2.0, 0.75, 1.0])
    l_near, l_far = loads(gpu_ctx, m, near)[2], loads(gpu_ctx, m, far)[2]
    untouched = np.setdiff1d(np.arange(m.xyz.shape[0]), m.conn[[31, 32]].reshape(-1))
    d = np.asarray(m.node_dof).reshape(-1, 3)[untouched].reshape(-1)
    assert l_near[d].tobytes() == l_far[d].tobytes() and l_near.tobytes() != l_far.tobytes()


def _solve(ctx, m, F):
    """(U, report, diag, lambda_min of the reduced K, its upper CRS) with eps_f 1e-12, merit stop off"""
    from stan_amd import hip
    ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
    try:
        K = ctx.assemble_hex8(m.xyz, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red)
        rowptr, col, val = K.to_csr(upper_only=True)
        U, rep = K.cg_solve(F, 1e-12)
        diag = K.diagonal()
        K.free()
    finally:
        ctx.set_option(hip.OPT_CG_MERIT_STOP, 1)
    N = F.shape[0]
    A = np.zeros((N, N))
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    A[rows, col] = val
    A = A + A.T - np.diag(np.diag(A))
    return U, rep, diag, float(np.linalg.eigvalsh(A)[0]), A


def _residual_bound(rep, diag, a_free, F_norm, rho_f):
    """|F - f_int(U)|_2 after a solve, the bound tests/test_gpu_internal_forces.py::test_equilibrium_after_a_solve derives:
    sqrt(max d / min d) rel_residual |F| + (4 rho_np + 2 x 41) 2^-52 |a|."""
    return np.sqrt(diag.max() / diag.min()) * rep["rel_residual"] * F_norm + (4 * rho_f + 2 * 41) * U52 * np.linalg.norm(a_free)


def _full(m, U, u0=None):
    from stan_amd import host
    disp = host.nodal_displacements(m.node_dof, m.red, U).reshape(-1, 3)
    if u0 is not None:
        fixed = m.red[np.asarray(m.node_dof).reshape(-1, 3)] == -1
        disp[fixed] = u0[fixed]
    return disp


def test_pressure_patch_end_to_end(gpu_ctx, rho_np, rho_np_forces):
    """4^3 HEX8_G2, interior jittered: symmetry supports on x = 0, y = 0, z = 0, pressure p on z = L.  The exact field
    u = (nu p x / E, nu p y / E, -p z / E) is in the element space, so (a) F - f_int(u_exact) vanishes on the free DOFs up to
    the rounding of both sides, 4 (rho_np_forces a_i + rho_np_loads s_i) 2^-52; (b) after a solve U - u_exact = K^-1 ((F - K
    u_exact) - (F - K U)), so |U - u_exact|_2 <= (|F - f_int(u_exact)| + |F - f_int(U)|) / lambda_min(K) with the second
    term bounded as test_equilibrium_after_a_solve bounds it; (c) the recovered sigma_zz is linear in u: a strain component is
    a sum of at most 16 products grad N u, a stress component (3 lam + 2 G) times the largest of them, and the extrapolation
    to the nodes magnifies by at most 3 sqrt 3 -- that times |U - u_exact|_inf, plus the same chain's rounding on u_exact
    itself (fewer than 64 rounded operations)."""
    n, p = 4, 1000.0
    m = L.patch_model(n)
    E, nu = m.mat_E_nu[0]
    el, fid = L.cube_face(n, 5)
    case = L.Case(None, el, fid, np.full(el.size, p))
    F, _, l, sums = loads(gpu_ctx, m, case, F=np.zeros(m.n_dof - m.n_fixed))
    assert abs(sums.area - n * n) <= 1e-12 and abs(sums.load_sum[2] + p * n * n) <= 1e-9 * p
    u_ex = m.xyz * np.array([nu * p / E, nu * p / E, -p / E])
    _, a = R.reference(m, u_ex)
    s = L.scale(m, case)
    f_int, _, eq = gpu_ctx.internal_forces_hex8(m.xyz, u_ex, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, F)
    free = m.red != -1
    Ffull = np.zeros(m.n_dof); Ffull[free] = F
    cap = 4 * (rho_np_forces * a + rho_np * s) * U52
    worst = (np.abs(Ffull - f_int)[free] / cap[free]).max()
    print("patch: max |F - f_int(u_exact)| / cap = %.3f (loads up to %.1f, residual up to %.3e)" % (worst, np.abs(F).max(), eq.residual_max))
    assert (np.abs(Ffull - f_int)[free] <= cap[free]).all() and np.abs(F).max() > 1.0
    # (b)
    U, rep, diag, lam_min, _ = _solve(gpu_ctx, m, F)
    disp = _full(m, U)
    _, aU = R.reference(m, disp)
    _, _, eqU = gpu_ctx.internal_forces_hex8(m.xyz, disp, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, F)
    res_bound = _residual_bound(rep, diag, aU[free], eqU.load_norm2, rho_np_forces)
    err = np.linalg.norm(free_part(m, (disp - u_ex).reshape(-1)[np.argsort(np.asarray(m.node_dof).reshape(-1))]))
    u_bound = (res_bound + np.linalg.norm(cap[free])) / lam_min
    print("   its %d rel_residual %.3e: |F - f_int(U)| %.3e <= %.3e; |U - u_exact|_2 %.3e <= %.3e (|u| %.3e)" %
          (rep["iterations"], rep["rel_residual"], eqU.residual_norm2, res_bound, err, u_bound, np.linalg.norm(u_ex)))
    assert eqU.residual_norm2 <= res_bound and err <= u_bound and u_bound < 1e-6 * np.linalg.norm(u_ex)
    # (c)
    lam, G = (E * nu) / ((1 - 2 * nu) * (1 + nu)), 0.5 * E / (1 + nu)
    chain = (3 * lam + 2 * G) * 16 * L.grad_max(m) * 3 * np.sqrt(3.0)
    _, stress = gpu_ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    s_err = np.abs(stress[:, :, 2] + p).max()
    s_bound = chain * (u_bound + 64 * U52 * np.abs(u_ex).max())
    print("   max |sigma_zz + p| %.3e <= %.3e" % (s_err, s_bound))
    assert s_err <= s_bound and s_bound < 1e-4 * p


@pytest.mark.parametrize("n,jit", [(4, 0.0), (6, 0.1)])
def test_gravity_reactions(gpu_ctx, rho_np, rho_np_forces, n, jit):
    """Self-weight on the cube clamped at x = 0: after the solve the supports carry what reached the free DOFs.
    reaction_sum + load_sum is bounded as in test_equilibrium_after_a_solve (sqrt(N) |r| + rounding); eq.load_sum is the sum
    of the F this call wrote, sums.free_sum the sum of the same numbers in another order: n_dof 2^-53 sum |F| apart."""
    job = problem.cube_job(n, jitter=jit)
    body = np.array([[0.0, 0.0, -7.85e-2]])
    F, _, l, sums = loads(gpu_ctx, job, mat_body=body, F=np.zeros(job.n_red))
    U, rep, diag, _, _ = _solve(gpu_ctx, job, F)
    disp = _full(job, U)
    _, a = R.reference(job, disp)
    f_int, _, eq = gpu_ctx.internal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu,
                                                job.red, F)
    free = job.red != -1
    N = int(free.sum())
    assert eq.residual_norm2 <= _residual_bound(rep, diag, a[free], eq.load_norm2, rho_np_forces)
    rounding = 4 * rho_np_forces * U52 * a.sum() + job.n_dof * 2.0 ** -53 * (np.abs(f_int).sum() + np.abs(F).sum())
    for c in range(3):
        print("n=%d direction %d: reaction %.9e + load %.9e = %.3e <= %.3e" % (n, c, eq.reaction_sum[c], eq.load_sum[c],
              eq.reaction_sum[c] + eq.load_sum[c], np.sqrt(N) * eq.residual_norm2 + rounding))
        assert abs(eq.reaction_sum[c] + eq.load_sum[c]) <= np.sqrt(N) * eq.residual_norm2 + rounding
        assert abs(eq.load_sum[c] - sums.free_sum[c]) <= job.n_dof * 2.0 ** -53 * np.abs(F).sum()
    # partition of unity: the loads sum to b V; every entry of l within 4 rho_np units of 2^-52 s, their sum in any order
    case = L.Case(mat_body=body)
    _, vol_ref, _ = L.reference(job, case)
    tol = 4 * rho_np * U52 * L.scale(job, case).sum() + job.n_dof * 2.0 ** -53 * np.abs(l).sum()
    assert abs(sums.load_sum[2] - body[0, 2] * float(vol_ref)) <= tol and sums.load_sum[0] == 0.0 and sums.load_sum[1] == 0.0
    if jit == 0.0:
        assert abs(sums.volume - n ** 3) <= (n ** 3 + 8) * U52 * n ** 3
    assert sums.load_sum[2] < sums.free_sum[2] < 0                 # the clamped face takes its share


def test_prescribed_displacement(gpu_ctx, rho_np_forces):
    """Boundary of a jittered 4^3 cube moved by u = A x: f_int of the linear field vanishes at the interior nodes, so
    F_solve = -f_int(u0)|free = K_ff u_f,exact.  Against numpy's product with the exported reduced CRS: the rounding of
    f_int (4 rho_np_forces units of 2^-52 a(u0)), of the product (a row has at most 81 entries: 41 units of |K| |u_f|) and of
    the assembled values themselves: an entry adds at most 8 element entries (7 roundings: 4 units of a(u_f) =
    sum_e |K_e| |u_e|), each formed in fp64 from the Gauss-point quantities the internal forces use (the same 4 rho_np_forces
    units of a(u_f)).  Independently of K, F_solve is held against -f_ref(u0) of the oracle's element matrices in longdouble,
    in f_int's own units.  The solved interior follows as in the pressure patch test; the reactions of a self-equilibrated
    field sum to zero."""
    m = L.patch_model(4, supports="all")
    A = np.array([[1.0e-3, 2.0e-4, -3.0e-4], [1.5e-4, -7.0e-4, 2.5e-4], [-1.0e-4, 3.0e-4, 5.0e-4]])
    lin = m.xyz @ A.T
    fixed_nodes = (m.red[np.asarray(m.node_dof).reshape(-1, 3)] == -1)
    u0 = np.where(fixed_nodes, lin, 123.0)                         # entries at free DOFs are ignored
    _, F_solve, l, sums = loads(gpu_ctx, m, disp0=u0, load_full=True)
    assert (l == 0).all() and list(sums.load_sum) == [0.0, 0.0, 0.0] and sums.n_fixed == m.n_fixed
    U, rep, diag, lam_min, Kff = _solve(gpu_ctx, m, F_solve)
    order = np.argsort(np.asarray(m.node_dof).reshape(-1))         # DOF -> 3 * node + component
    u_f = free_part(m, lin.reshape(-1)[order])
    f0, a0 = R.reference(m, np.where(fixed_nodes, lin, 0.0))
    _, af = R.reference(m, np.where(fixed_nodes, 0.0, lin))
    direct = np.abs(F_solve + free_part(m, f0.astype(np.float64)))          # (f0 is exact to a rounding: 1 more unit of a0)
    cap0 = U52 * (4 * rho_np_forces + 1) * free_part(m, a0)
    cap = U52 * (4 * rho_np_forces * free_part(m, a0 + af) + 4 * free_part(m, af) + 41 * (np.abs(Kff) @ np.abs(u_f)))
    gap = np.abs(F_solve - Kff @ u_f)
    print("prescribed: max |F_solve + f_ref(u0)| / cap = %.3f; max |F_solve - K_ff u_f| / cap = %.3f (|F_solve| up to %.3e)" %
          ((direct / cap0).max(), (gap / cap).max(), np.abs(F_solve).max()))
    assert (direct <= cap0).all() and (gap <= cap).all() and np.abs(F_solve).max() > 1.0
    disp = _full(m, U, u0)
    assert np.array_equal(disp[fixed_nodes], lin[fixed_nodes])
    _, aU = R.reference(m, disp)
    free = m.red != -1
    f_int, reaction, eq = gpu_ctx.internal_forces_hex8(m.xyz, disp, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red)
    res_bound = _residual_bound(rep, diag, aU[free], np.linalg.norm(F_solve), rho_np_forces) + np.linalg.norm(cap)
    err, u_bound = np.linalg.norm(U - u_f), (res_bound + np.linalg.norm(cap)) / lam_min
    print("   its %d rel_residual %.3e: |f_int(U + u0)|free %.3e <= %.3e; |U - A x|_2 %.3e <= %.3e" %
          (rep["iterations"], rep["rel_residual"], eq.residual_norm2, res_bound, err, u_bound))
    assert eq.residual_norm2 <= res_bound and err <= u_bound and u_bound < 1e-6 * np.linalg.norm(u_f)
    rounding = 4 * rho_np_forces * U52 * aU.sum() + m.n_dof * 2.0 ** -53 * np.abs(f_int).sum()
    for c in range(3):
        assert abs(eq.reaction_sum[c]) <= np.sqrt(int(free.sum())) * eq.residual_norm2 + rounding
    assert np.abs(reaction).max() > 1.0


def _with(job, **kw):
    import copy
    j = copy.copy(job)
    for k, v in kw.items():
        setattr(j, k, np.ascontiguousarray(v).reshape(np.asarray(getattr(job, k)).shape))
    return j


def test_errors(gpu_ctx):
    from stan_amd import hip
    job = problem.cube_job(3)
    body = np.array([[0.0, 0.0, -1.0]])
    el, fid = L.cube_face(3, 1)
    faces = dict(face_elem=el, face_id=fid, face_pressure=np.ones(el.size))

    def code(j=job, **kw):
        with pytest.raises(hip.StanHipError) as ei:
            loads(gpu_ctx, j, **kw)
        return ei.value.code
    # the face list: unsorted, duplicate, element / face id out of range
    assert code(face_elem=el[::-1], face_id=fid, face_pressure=np.ones(el.size)) == hip.E_ARG
    assert code(face_elem=[2, 2], face_id=[1, 1], face_pressure=[1.0, 1.0]) == hip.E_ARG
    assert code(face_elem=[2, 2], face_id=[3, 1], face_pressure=[1.0, 1.0]) == hip.E_ARG
    assert code(face_elem=[27], face_id=[0], face_pressure=[1.0]) == hip.E_ARG
    assert code(face_elem=[-1], face_id=[0], face_pressure=[1.0]) == hip.E_ARG
    assert code(face_elem=[26], face_id=[6], face_pressure=[1.0]) == hip.E_ARG
    # material, node index, element type
    mat = job.elem_mat.copy(); mat[11] = 1
    assert code(_with(job, elem_mat=mat), mat_body=body) == hip.E_ARG
    bad = job.conn.copy(); bad[7, 3] = job.xyz.shape[0]
    assert code(_with(job, conn=bad), mat_body=body) == hip.E_ARG
    bad[7, 3] = -1
    assert code(_with(job, conn=bad), **faces) == hip.E_ARG
    typ = job.elem_type.copy(); typ[2] = 3
    assert code(_with(job, elem_type=typ), mat_body=body) == hip.E_ARG
    # n_dof != 3 n_nodes; a bad reduction map
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.load_vector_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red[:-3], mat_body=body)
    assert ei.value.code == hip.E_ARG
    free = int(np.nonzero(job.red != -1)[0][3])
    for v in (-2, free + 1):
        red = job.red.copy(); red[free] = v
        assert code(_with(job, red=red), mat_body=body) == hip.E_ARG
    # nothing to do, nothing asked for, disp0 without F_solve
    assert code() == hip.E_ARG
    assert code(mat_body=body, load_full=False, sums=False) == hip.E_ARG
    assert code(mat_body=body, disp0=np.zeros(job.xyz.shape), F_solve=False) == hip.E_ARG
    # Node.DOF
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[4, [1, 2]] = dof[4, [2, 1]]
    assert code(_with(job, node_dof=dof), mat_body=body) == hip.E_DOF_LAYOUT
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[9] = dof[20]
    assert code(_with(job, node_dof=dof), **faces) == hip.E_DOF_LAYOUT
    # det J == 0: no error for body forces and pressures, STAN_E_DETJ from the disp0 part only
    xyz = job.xyz.copy()
    xyz[job.conn[5]] = xyz[job.conn[5]] * [1, 1, 0]
    flat = _with(job, xyz=xyz)
    _, _, l, sums = loads(gpu_ctx, flat, mat_body=body, **faces)
    assert np.isfinite(l).all()
    assert code(flat, mat_body=body, disp0=np.full(job.xyz.shape, 1e-3)) == hip.E_DETJ and gpu_ctx.last_bad_element() == 5
    # the same bad integers in DEVICE memory are caught by the device-side check, before anything is indexed
    import torch
    dev = torch.device("cuda:0")
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    dx, dd, dc = t(job.xyz, np.float64), t(job.node_dof, np.int32), t(job.conn, np.int32)
    dm, dty, dr = t(job.elem_mat, np.int32), t(job.elem_type, np.uint8), t(job.red, np.int32)
    dl = torch.zeros(job.n_dof, dtype=torch.float64, device=dev)
    for fe_, fi_ in (([1 << 30], [0]), ([3, 3], [2, 2]), ([3], [200])):
        dfe, dfi, dfp = t(fe_, np.int32), t(fi_, np.uint8), t(np.ones(len(fe_)), np.float64)
        torch.cuda.synchronize()
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.load_vector_hex8_dev(job.xyz.shape[0], dx.data_ptr(), dd.data_ptr(), job.conn.shape[0], dc.data_ptr(), dm.data_ptr(),
                                         dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr(), None, len(fe_), dfe.data_ptr(),
                                         dfi.data_ptr(), dfp.data_ptr(), d_load_full=dl.data_ptr())
        assert ei.value.code == hip.E_ARG
    # n_elem >= 2^28 is refused before any kernel runs and before any array is touched
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.load_vector_hex8_dev(job.xyz.shape[0], dx.data_ptr(), dd.data_ptr(), 1 << 28, dc.data_ptr(), dm.data_ptr(),
                                     dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr(), body, d_load_full=dl.data_ptr())
    assert ei.value.code == hip.E_ARG and "2^28" in str(ei.value)
    bad[7, 3] = 1 << 30
    dcb = t(bad, np.int32)
    torch.cuda.synchronize()
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.load_vector_hex8_dev(job.xyz.shape[0], dx.data_ptr(), dd.data_ptr(), job.conn.shape[0], dcb.data_ptr(), dm.data_ptr(),
                                     dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr(), body, d_load_full=dl.data_ptr())
    assert ei.value.code == hip.E_ARG
    # the context is still usable
    _, _, l, sums = loads(gpu_ctx, job, mat_body=body, **faces)
    assert abs(sums.volume - 27.0) <= 1e-12 and abs(sums.area - 9.0) <= 1e-12


def test_multi_device_handle_is_refused(built_libs):
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from stan_amd import hip, problem
job = problem.cube_job(3)
body = np.array([[0.0, 0.0, -1.0]])
ctx = hip.Context(devices=[0, 0])
try:
    ctx.load_vector_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red, mat_body=body)
    print("HOST NOERROR")
except hip.StanHipError as e:
    print("HOST", e.code, "multi-device" in str(e))
t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to("cuda:0")
dx, dd, dc = t(job.xyz, np.float64), t(job.node_dof, np.int32), t(job.conn, np.int32)
dm, dty, dr = t(job.elem_mat, np.int32), t(job.elem_type, np.uint8), t(job.red, np.int32)
dl = torch.zeros(job.n_dof, dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
try:
    ctx.load_vector_hex8_dev(job.xyz.shape[0], dx.data_ptr(), dd.data_ptr(), job.conn.shape[0], dc.data_ptr(), dm.data_ptr(),
                             dty.data_ptr(), job.mat_E_nu, job.n_dof, dr.data_ptr(), body, d_load_full=dl.data_ptr())
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


def _write_model(path, n, distributed):
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
    if distributed:
        d.add_bc(3, "weight", "BodyForce", [1], [distributed["body"]])
        d.add_bc(4, "push", "Pressure", ld + 1, np.column_stack([np.full(len(ld), distributed["p"]), np.zeros((len(ld), 2))]))
        d.add_bc(5, "settle", "Displacement", spc + 1, np.tile(distributed["move"], (len(spc), 1)))
    d.set_analysis(tol=1e-10)
    d.write_stdb(path)
    return spc


def test_console_driver_distributed_loads(gpu_ctx, tmp_path):
    """stan_solver --reactions --json on a 4^3 .STdb with "BodyForce" + "Pressure" + "Displacement" next to its point loads:
    the block and the "loads" object are the binding's sums for the same model, the stored displacements carry u0 at the
    fixed DOFs, the equilibrium check sees the EXTERNAL load; a file without such BCs has neither the block nor the key."""
    import json
    from stan_amd import host
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    plain, path = str(tmp_path / "plain.STdb"), str(tmp_path / "model.STdb")
    what = dict(body=[0.0, 0.0, -7.85e-2], p=3.5, move=[1.0e-3, 0.0, -2.0e-3])
    _write_model(plain, 4, None)
    spc = _write_model(path, 4, what)
    out0 = subprocess.run([exe, "--reactions", "--json", plain], capture_output=True, text=True, timeout=300)
    assert out0.returncode == 0, out0.stdout + out0.stderr
    assert "Distributed loads" not in out0.stdout and "\"loads\"" not in out0.stdout
    out = subprocess.run([exe, "--reactions", "--json", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("Distributed loads:", "Total:", "On free DOFs:", "Loaded volume:", "loaded area:", "(16 faces)", "prescribed DOFs: %d" % (2 * len(spc))):
        assert word in out.stdout, out.stdout
    js = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    js0 = json.loads([l for l in out0.stdout.splitlines() if l.startswith("{")][0])
    assert set(js) - set(js0) == {"loads"}
    job = problem.cube_job(4, jitter=0.1)
    el, fid = L.cube_face(4, 1)
    u0 = np.zeros(job.xyz.shape); u0[spc] = what["move"]
    F, F_solve, _, sums = loads(gpu_ctx, job, mat_body=[what["body"]], face_elem=el, face_id=fid,
                                face_pressure=np.full(el.size, what["p"]), disp0=u0, F=job.F)
    q = js["loads"]
    assert q["load_sum"] == list(sums.load_sum) and q["free_sum"] == list(sums.free_sum)
    assert q["volume"] == sums.volume and q["area"] == sums.area and q["n_faces"] == 16 and q["n_fixed"] == sums.n_fixed
    assert q["n_prescribed"] == 2 * len(spc)
    disp = host.Db.read_stdb(path).results(1)[0]
    assert np.array_equal(disp[spc], np.tile(what["move"], (len(spc), 1)))
    f_int, reaction, eq = gpu_ctx.internal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type,
                                                       job.mat_E_nu, job.red, F)
    e = js["equilibrium"]
    for k in ("reaction_sum", "load_sum", "fint_sum"):
        assert e[k] == list(getattr(eq, k)), k
    assert e["residual_norm2"] == eq.residual_norm2 and e["residual_norm2"] < 1e-6 * e["load_norm2"]
    assert abs(e["load_sum"][0] - sums.free_sum[0]) <= 1e-9 and abs(e["load_sum"][2] - (50.0 * 25 + sums.free_sum[2])) <= 1e-9


def test_phase_times(gpu_ctx):
    """stan_hip_load_vector_times: zero without profiling, the three phases of the last call with it."""
    m, case = L.cases()["cube5-surf"]
    loads(gpu_ctx, m, case)
    assert list(gpu_ctx.load_vector_times().values()) == [0.0, 0.0, 0.0]
    gpu_ctx.set_profiling(True)
    try:
        loads(gpu_ctx, m, case)
        t = gpu_ctx.load_vector_times()
    finally:
        gpu_ctx.set_profiling(False)
    assert all(0.0 < v < 100.0 for v in t.values()), t
