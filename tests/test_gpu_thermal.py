"""Thermal loads on the GPU (stan_hip_thermal_load_hex8, stan_hip_thermal_stress_hex8) against
tests/thermal_ref.py: l_ref evaluated and scattered in longdouble, the rounding scale s = sum |grad N_a| |beta dT(q)| |det J w|
and rho = max_i |l_i - l_ref_i| / (2^-52 s_i).  The kernel is held to rho_gpu <= 4 rho_np, rho_np the worst rho of the plain-fp64
numpy restatement of the same operation form over the same inputs (thermal_ref.rho_np): FMA contraction and the butterfly order
of the point sums move the constant by a small factor, not by an order of magnitude (tests/forces_ref.py).

The sums.  load_sum and free_sum add entries that are each within 4 rho_np 2^-52 s_i of the reference's, in another order than
the reference adds them: 4 rho_np 2^-52 sum s_i plus n_nodes roundings of at most 2^-53 sum |l_i| each.  volume is held to
(n_elem + 8) 2^-52 of the longdouble sum (the bound and the reason of tests/test_gpu_loads.py: the eight rounded point terms of
an element, then one rounding per element on the way to the total); dT_integral to (n_elem + 8 + 16) 2^-52 of
sum_q (sum_a |N_a dT_a|) |det J w|: the interpolation adds eight rounded products (15 roundings) and the product with det J w one.

Measured on an MI355X when the tests were written: rho_np 30.88 (the 31-element strip with a random dT; cap 123.53), worst
rho_gpu 20.83 (the 33-element strip with a random dT); volume and dT_integral within 0.06 and 0.11 of their bounds; the stress
pass within 0.495 of its unit; per case in profiles/r09/thermal_n148.md."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import hip
from stan_amd.cube import cube_mesh
from tests import device_buffers as B
from tests import forces_ref as R
from tests import loads_ref as L
from tests import thermal_ref as T
from tests.test_gpu_loads import _full, _residual_bound, _solve, _with, free_part

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
U52 = T.U52
DEV = "cuda:0"


def thermal(ctx, m, case, **kw):
    return ctx.thermal_load_hex8(m.xyz, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, case.mat_alpha, case.dT, **kw)


def corrected(ctx, m, case, stress):
    return ctx.thermal_stress_hex8(case.dT, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, case.mat_alpha, stress)


@pytest.fixture(scope="module")
def rho_np():
    return T.rho_np(verbose=True)


@pytest.fixture(scope="module")
def rho_np_forces():
    return R.rho_np()


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.cases()))
def test_parity_with_the_reference(gpu_ctx, rho_np, name):
    m, case = T.cases()[name]
    l_ref, vol_ref, int_ref = T.reference(m, case)
    s = T.scale(m, case)
    _, l, sums = thermal(gpu_ctx, m, case)
    rho = T.rho(l, l_ref, s)
    ne, nn = m.conn.shape[0], m.xyz.shape[0]
    vtol = (ne + 8) * U52 * abs(float(vol_ref))
    itol = (ne + 8 + 16) * U52 * T.integral_scale(m, case)
    print("%s: rho_gpu %.2f (numpy restatement on this case %.2f; rho_np %.2f, cap %.2f); volume error %.4f, dT_integral error "
          "%.4f of their bounds" % (name, rho, T._rho_np[name], rho_np, 4 * rho_np, abs(sums.volume - vol_ref) / vtol,
                                    abs(sums.dT_integral - int_ref) / itol))
    assert np.isfinite(l).all() and rho <= 4 * rho_np
    assert (l[s == 0] == 0).all()                                   # nothing where no temperature reaches
    assert abs(sums.volume - vol_ref) <= vtol and abs(sums.dT_integral - int_ref) <= itol
    assert sums.n_fixed == m.n_fixed
    d = np.asarray(m.node_dof).reshape(-1, 3)
    for c in range(3):
        fixed = m.red[d[:, c]] == -1
        order = nn * 2.0 ** -53 * np.abs(l[d[:, c]]).sum()
        for got, keep in ((sums.load_sum[c], np.ones(nn, dtype=bool)), (sums.free_sum[c], ~fixed)):
            want = l_ref[d[:, c]][keep].sum()
            assert abs(got - want) <= 4 * rho_np * U52 * s[d[:, c]][keep].sum() + order, (c, got, float(want))


# ---- 2. F semantics and bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube5-rand", "revolved-rand", "mixed4-cold", "strip33-sel"])
def test_F_semantics(gpu_ctx, name):
    """F_out = F_in + the free part of l as ONE fp64 add per entry; load_full is l; where the temperature reaches the supports
    some of l falls on them."""
    m, case = T.cases()[name]
    F_in = np.random.default_rng(3).standard_normal(m.n_dof - m.n_fixed) * 7.0
    F_out, l, _ = thermal(gpu_ctx, m, case, F=F_in)
    assert F_out.tobytes() == (F_in + free_part(m, l)).tobytes()
    none_F, l2, _ = thermal(gpu_ctx, m, case)
    assert none_F is None and l2.tobytes() == l.tobytes()
    assert np.abs(free_part(m, l)).max() > 0
    if not name.endswith("-sel"):                                   # (there the heated elements are away from the supports)
        assert np.abs(l[m.red == -1]).max() > 0


def _dev_call(ctx, mesh, case, d_dT, d_F=None, d_l=None, sums=True):
    return ctx.thermal_load_hex8_dev(mesh.n_nodes, mesh.xyz.ptr, mesh.node_dof.ptr, mesh.n_elem, mesh._e(mesh.conn),
                                     mesh._e(mesh.elem_mat), mesh._e(mesh.elem_type), mesh.mat_E_nu, mesh.n_dof, mesh.red.ptr,
                                     case.mat_alpha, d_dT.ptr, None if d_F is None else d_F.ptr, None if d_l is None else d_l.ptr,
                                     sums=sums)


def test_bits(gpu_ctx):
    """Same bytes from two calls and for every subset of the outputs."""
    m, case = T.cases()["revolved-rand"]
    F_in = np.random.default_rng(4).standard_normal(m.n_dof - m.n_fixed)
    ref = thermal(gpu_ctx, m, case, F=F_in)
    again = thermal(gpu_ctx, m, case, F=F_in)
    for a, b in zip(ref, again):
        assert bytes(a) == bytes(b)
    for wF, wL, wQ in itertools.product([False, True], repeat=3):
        if not (wF or wL or wQ):
            continue
        got = thermal(gpu_ctx, m, case, F=F_in if wF else None, load_full=wL, sums=wQ)
        for k, on in enumerate((wF, wL, wQ)):
            assert (got[k] is None) == (not on)
            if on:
                assert bytes(got[k]) == bytes(ref[k]), (wF, wL, wQ, k)


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("name", ["strip9-rand", "strip33-sel", "mixed4-cold", "revolved-rand"])
def test_device_entry_in_guards(gpu_ctx, name, offset):
    """The _dev entry between guards, aligned and one element past a 256-byte boundary: the host entry's bytes, nothing stored
    outside an output, every entry written, inputs unchanged; F alone and load_full alone too."""
    import torch
    m, case = T.cases()[name]
    N = m.n_dof - m.n_fixed
    F_in = np.random.default_rng(6).standard_normal(N)
    F_ref, l_ref, q_ref = thermal(gpu_ctx, m, case, F=F_in)
    g = B.guard_len(m.n_dof)
    mesh = B.Mesh(m, DEV, offset)
    d_dT = B.input_("dT", case.dT, g, DEV, offset)
    d_F, d_l = B.output("F", N, g, DEV, offset), B.output("load_full", m.n_dof, g, DEV, offset)
    for wF, wL in ((True, True), (True, False), (False, True)):
        d_F.refill(); d_l.refill()
        d_F.payload.copy_(torch.from_numpy(F_in))
        _sync()
        q = _dev_call(gpu_ctx, mesh, case, d_dT, d_F if wF else None, d_l if wL else None)
        _sync()
        B.check(mesh.inputs + [d_dT] + ([d_F] if wF else []) + ([d_l] if wL else []))
        assert bytes(q) == bytes(q_ref)
        assert d_F.numpy().tobytes() == (F_ref if wF else F_in).tobytes()
        if wL:
            assert d_l.numpy().tobytes() == l_ref.tobytes()
        else:
            B.check([d_l], written=False)
            assert (B._bits(d_l.payload) == B.UNWRITTEN_BITS).all()


# ---- 3. thermal stress ---------------------------------------------------------------------------------------------------
def _two_material_cube():
    xyz, conn = cube_mesh(3, jitter=0.1)
    m = R.model(xyz, conn, elem_mat=np.arange(conn.shape[0]) % 2, mat_E_nu=[[210000.0, 0.3], [70000.0, 0.33]])
    return m, T.Case([1.2e-5, 2.3e-5], np.random.default_rng(31).uniform(-50.0, 150.0, xyz.shape[0]))


STRESS_MODELS = {"cube5": lambda: T.cases()["cube5-rand"], "strip33": lambda: T.cases()["strip33-sel"], "cube3x2": _two_material_cube}


@pytest.mark.parametrize("name", sorted(STRESS_MODELS))
def test_thermal_stress(gpu_ctx, name):
    """Every corrected entry within 2^-52 (|sigma| + |beta dT|) of sigma - beta dT (one product rounding plus one difference
    rounding; the kernel's fused multiply-add makes one); shear entries bit-unchanged; on kept results the same bytes, the
    strain untouched."""
    m, case = STRESS_MODELS[name]()
    disp = R.random_disp(m, 77)
    strain, stress = gpu_ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    got = corrected(gpu_ctx, m, case, stress)
    want, mag = T.stress_expected(m, case, stress)
    err = np.abs(got.astype(np.longdouble) - want)[:, :, :3]
    print("%s: worst |got - (sigma - beta dT)| / (2^-52 (|sigma| + |beta dT|)) = %.3f" % (name, float((err / (U52 * mag)).max())))
    assert (err <= U52 * mag).all()
    assert got[:, :, 3:].tobytes() == stress[:, :, 3:].tobytes()
    assert np.abs(got[:, :, :3] - stress[:, :, :3]).max() > 1.0     # the correction is there
    assert corrected(gpu_ctx, m, case, stress).tobytes() == got.tobytes()
    res = gpu_ctx.recover_hex8_keep(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    try:
        ne = m.conn.shape[0]
        e0, s0 = res.map(0, ne)
        assert e0.tobytes() == strain.tobytes() and s0.tobytes() == stress.tobytes()
        res.thermal_stress(case.dT, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, case.mat_alpha)
        e1, s1 = res.map(0, ne)
        assert e1.tobytes() == strain.tobytes() and s1.tobytes() == got.tobytes()
    finally:
        res.free()


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("name", ["strip33", "cube3x2"])
def test_thermal_stress_device_entry_in_guards(gpu_ctx, name, offset):
    import torch
    m, case = STRESS_MODELS[name]()
    ne = m.conn.shape[0]
    stress = np.random.default_rng(8).standard_normal((ne, 8, 6)) * 50.0
    want = corrected(gpu_ctx, m, case, stress)
    g = B.guard_len(m.n_dof)
    mesh = B.Mesh(m, DEV, offset)
    d_dT = B.input_("dT", case.dT, g, DEV, offset)
    d_s = B.output("stress", 48 * ne, g, DEV, offset)
    d_s.payload.copy_(torch.from_numpy(stress.reshape(-1)))
    _sync()
    gpu_ctx.thermal_stress_hex8_dev(mesh.n_nodes, d_dT.ptr, ne, mesh.conn.ptr, mesh.elem_mat.ptr, mesh.elem_type.ptr, mesh.mat_E_nu,
                                    case.mat_alpha, d_s.ptr)
    _sync()
    B.check(mesh.inputs + [d_dT, d_s])
    assert d_s.numpy().tobytes() == want.tobytes()


# ---- 4. free expansion, end to end ---------------------------------------------------------------------------------------
def test_free_expansion_end_to_end(gpu_ctx, rho_np, rho_np_forces):
    """4^3 HEX8_G2, interior jittered, symmetry supports, one material, uniform dT.  u = alpha dT x is in the element space and
    the load uses the stiffness rule, so (a) F - f_int(u_exact) vanishes on the free DOFs up to the rounding of both sides,
    4 (rho_np_forces a_i + rho_np s_i) 2^-52; (b) |U - u_exact|_2 <= (|F - f_int(u_exact)| + |F - f_int(U)|) / lambda_min(K),
    the second term bounded by _residual_bound of tests/test_gpu_loads.py from the solve's own rel_residual; (c) the recovered
    stress is linear in u and equals beta dT on u_exact: a strain component is a sum of at most 16 products grad N u, a stress
    component (3 lam + 2 G) times the largest, the extrapolation to the nodes magnifies by at most 3 sqrt 3 -- that times
    |U - u_exact|, plus the same chain's rounding on u_exact (fewer than 64 operations), plus the correction's own two
    roundings of beta dT."""
    alpha, dT = 1.2e-5, 100.0
    m = L.patch_model(4, 0.2, "sym")
    E, nu = m.mat_E_nu[0]
    case = T.Case([alpha], np.full(m.xyz.shape[0], dT))
    bdT = float(T.beta(m, case.mat_alpha)[0]) * dT
    F, l, sums = thermal(gpu_ctx, m, case, F=np.zeros(m.n_dof - m.n_fixed))
    assert abs(sums.volume - 64.0) <= 72 * U52 * 64.0 and abs(sums.dT_integral - 6400.0) <= 88 * U52 * 6400.0
    u_ex = alpha * dT * m.xyz
    _, a = R.reference(m, u_ex)
    s = T.scale(m, case)
    f_int, _, eq = gpu_ctx.internal_forces_hex8(m.xyz, u_ex, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, F)
    free = m.red != -1
    Ffull = np.zeros(m.n_dof); Ffull[free] = F
    cap = 4 * (rho_np_forces * a + rho_np * s) * U52
    print("free expansion: max |F - f_int(u_exact)| / cap = %.3f (loads up to %.1f)" %
          ((np.abs(Ffull - f_int)[free] / cap[free]).max(), np.abs(F).max()))
    assert (np.abs(Ffull - f_int)[free] <= cap[free]).all() and np.abs(F).max() > 1.0
    U, rep, diag, lam_min, _ = _solve(gpu_ctx, m, F)
    disp = _full(m, U)
    _, aU = R.reference(m, disp)
    _, _, eqU = gpu_ctx.internal_forces_hex8(m.xyz, disp, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red, F)
    res_bound = _residual_bound(rep, diag, aU[free], eqU.load_norm2, rho_np_forces)
    err = np.linalg.norm(free_part(m, (disp - u_ex).reshape(-1)[np.argsort(np.asarray(m.node_dof).reshape(-1))]))
    u_bound = (res_bound + np.linalg.norm(cap[free])) / lam_min
    print("   its %d rel_residual %.3e: |F - f_int(U)| %.3e <= %.3e; |U - alpha dT x|_2 %.3e <= %.3e (|u| %.3e)" %
          (rep["iterations"], rep["rel_residual"], eqU.residual_norm2, res_bound, err, u_bound, np.linalg.norm(u_ex)))
    assert eqU.residual_norm2 <= res_bound and err <= u_bound and u_bound < 1e-6 * np.linalg.norm(u_ex)
    lam, G = (E * nu) / ((1 - 2 * nu) * (1 + nu)), 0.5 * E / (1 + nu)
    chain = (3 * lam + 2 * G) * 16 * L.grad_max(m) * 3 * np.sqrt(3.0)
    _, stress = gpu_ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    got = corrected(gpu_ctx, m, case, stress)
    s_err = np.abs(got).max()
    s_bound = chain * (u_bound + 64 * U52 * np.abs(u_ex).max()) + 2 * U52 * bdT
    print("   max |corrected stress| %.3e <= %.3e (beta dT %.3e)" % (s_err, s_bound, bdT))
    assert s_err <= s_bound and s_bound < 1e-2 * bdT and np.abs(stress[:, :, :3]).min() > 0.99 * bdT


# ---- 5. full restraint ---------------------------------------------------------------------------------------------------
def test_full_restraint(gpu_ctx, rho_np, rho_np_forces):
    """Every boundary node of the jittered 4^3 cube fixed, uniform dT: the exact load vanishes at the interior nodes, so the
    free part is what the parity bound leaves of it, |F_i| <= (4 rho_np + 1) 2^-52 s_i (the reference's own entry there is a
    longdouble rounding); U = K^-1 F is bounded by (|F| + the solve's residual bound) / lambda_min; the recovered stress of that
    U by the chain of the free-expansion test, so the corrected stress is -beta dT in xx, yy, zz and 0 in shear within it (plus
    the correction's two roundings); the supports exert f_int(U) - l: -l up to |f_int| <= a(U), and their sum by direction is
    sum_fixed f_int - (sum_all l - sum_free l): at most sum a(U), the parity bound on every entry of l over all DOFs and again
    over the free ones (the exact sums are zero), and the n_nodes roundings of adding them."""
    alpha, dT = 1.2e-5, 100.0
    m = L.patch_model(4, 0.2, "all")
    E, nu = m.mat_E_nu[0]
    case = T.Case([alpha], np.full(m.xyz.shape[0], dT))
    bdT = float(T.beta(m, case.mat_alpha)[0]) * dT
    F, l, sums = thermal(gpu_ctx, m, case, F=np.zeros(m.n_dof - m.n_fixed))
    s = T.scale(m, case)
    free = m.red != -1
    assert (np.abs(l[free]) <= (4 * rho_np + 1) * U52 * s[free]).all() and np.abs(l[~free]).max() > 1.0
    assert F.tobytes() == (np.zeros_like(F) + free_part(m, l)).tobytes()
    if F.any():
        U, rep, diag, lam_min, _ = _solve(gpu_ctx, m, F)
        disp = _full(m, U)
        _, aU = R.reference(m, disp)
        u_bound = (np.linalg.norm(F) + _residual_bound(rep, diag, aU[free], np.linalg.norm(F), rho_np_forces)) / lam_min
    else:
        U, u_bound = np.zeros_like(F), 0.0
        disp = _full(m, U)
        _, aU = R.reference(m, disp)
    print("full restraint: |F|_inf %.3e, |U|_2 %.3e <= %.3e" % (np.abs(F).max(), np.linalg.norm(U), u_bound))
    assert np.linalg.norm(U) <= u_bound and u_bound < 1e-9 * alpha * dT
    lam, G = (E * nu) / ((1 - 2 * nu) * (1 + nu)), 0.5 * E / (1 + nu)
    chain = (3 * lam + 2 * G) * 16 * L.grad_max(m) * 3 * np.sqrt(3.0)
    _, stress = gpu_ctx.recover_hex8(m.xyz, disp, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu)
    got = corrected(gpu_ctx, m, case, stress)
    s_bound = chain * u_bound + 2 * U52 * bdT
    print("   max |sigma_nn + beta dT| %.3e, max |shear| %.3e <= %.3e" % (np.abs(got[:, :, :3] + bdT).max(), np.abs(got[:, :, 3:]).max(), s_bound))
    assert (np.abs(got[:, :, :3] + bdT) <= s_bound).all() and (np.abs(got[:, :, 3:]) <= s_bound).all() and s_bound < 1e-6 * bdT
    f_int, _, _ = gpu_ctx.internal_forces_hex8(m.xyz, disp, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, m.red)
    reaction = np.where(free, 0.0, f_int - l)
    # (reaction + l is formed in fp64 here: the difference and the sum round once each, relative to |l|)
    assert (np.abs(reaction + l)[~free] <= (1 + 4 * rho_np_forces * U52) * aU[~free] + 2 * U52 * np.abs(l[~free])).all()
    d = np.asarray(m.node_dof).reshape(-1, 3)
    nn = m.xyz.shape[0]
    for c in range(3):
        tol = 2 * (4 * rho_np + 1) * U52 * s[d[:, c]].sum() + nn * 2.0 ** -52 * np.abs(l[d[:, c]]).sum() + 2 * aU[d[:, c]].sum()
        print("   direction %d: reactions sum to %.3e <= %.3e (of %.3e in magnitude)" % (c, reaction[d[:, c]].sum(), tol, np.abs(reaction[d[:, c]]).sum()))
        assert abs(reaction[d[:, c]].sum()) <= tol and abs(sums.load_sum[c]) <= tol and abs(sums.free_sum[c]) <= tol
        assert tol < 1e-9 * np.abs(reaction[d[:, c]]).sum()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    from stan_amd import problem
    job = problem.cube_job(3)
    nn, ne = job.xyz.shape[0], job.conn.shape[0]
    case = T.Case([1.2e-5], np.linspace(10.0, 90.0, nn))

    def code(j=job, c=case, **kw):
        with pytest.raises(hip.StanHipError) as ei:
            thermal(gpu_ctx, j, c, **kw)
        return ei.value.code
    # NULL mat_alpha / dT; every output NULL
    for a, t in ((None, case.dT), (case.mat_alpha, None)):
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.thermal_load_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red, a, t)
        assert ei.value.code == hip.E_ARG
    assert code(load_full=False, sums=False) == hip.E_ARG
    # material, node index, element type
    mat = job.elem_mat.copy(); mat[11] = 1
    assert code(_with(job, elem_mat=mat)) == hip.E_ARG
    bad = job.conn.copy(); bad[7, 3] = nn
    assert code(_with(job, conn=bad)) == hip.E_ARG
    bad[7, 3] = -1
    assert code(_with(job, conn=bad)) == hip.E_ARG
    typ = job.elem_type.copy(); typ[2] = 3
    assert code(_with(job, elem_type=typ)) == hip.E_ARG
    # n_dof != 3 n_nodes; a bad reduction map
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.thermal_load_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red[:-3],
                                  case.mat_alpha, case.dT)
    assert ei.value.code == hip.E_ARG
    first_free = int(np.nonzero(job.red != -1)[0][3])
    for v in (-2, first_free + 1):
        red = job.red.copy(); red[first_free] = v
        assert code(_with(job, red=red)) == hip.E_ARG
    # Node.DOF
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[4, [1, 2]] = dof[4, [2, 1]]
    assert code(_with(job, node_dof=dof)) == hip.E_DOF_LAYOUT
    dof = np.asarray(job.node_dof).copy().reshape(-1, 3)
    dof[9] = dof[20]
    assert code(_with(job, node_dof=dof)) == hip.E_DOF_LAYOUT
    # a singular element: accepted where its material does not expand, refused with its index where it does
    xyz = job.xyz.copy()
    xyz[job.conn[5]] = xyz[job.conn[5]] * [1, 1, 0]
    two = _with(job, xyz=xyz, elem_mat=(np.arange(ne) == 5).astype(np.int32))
    two.mat_E_nu = np.array([[210000.0, 0.3], [70000.0, 0.33]])
    _, l, sums = thermal(gpu_ctx, two, T.Case([1.2e-5, 0.0], case.dT))
    assert np.isfinite(l).all() and np.isfinite(sums.volume) and l.any()
    assert code(two, T.Case([1.2e-5, 2.0e-5], case.dT)) == hip.E_DETJ and gpu_ctx.last_bad_element() == 5
    assert code(two, T.Case([0.0, 2.0e-5], case.dT)) == hip.E_DETJ and gpu_ctx.last_bad_element() == 5
    # thermal stress: HEX8_G1 is refused with its element, as in the recovery; indices out of range
    stress = np.random.default_rng(1).standard_normal((ne, 8, 6))

    def scode(**kw):
        a = dict(conn=job.conn, elem_mat=job.elem_mat, elem_type=job.elem_type)
        a.update(kw)
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.thermal_stress_hex8(case.dT, a["conn"], a["elem_mat"], a["elem_type"], job.mat_E_nu, case.mat_alpha, stress)
        return ei.value.code
    g1 = job.elem_type.copy(); g1[[6, 19]] = hip.HEX8_G1
    assert scode(elem_type=g1) == hip.E_UNSUPPORTED and gpu_ctx.last_bad_element() == 6
    assert scode(elem_type=typ) == hip.E_ARG and scode(elem_mat=mat) == hip.E_ARG
    bad[7, 3] = nn
    assert scode(conn=bad) == hip.E_ARG
    # the context is still usable
    _, l, sums = thermal(gpu_ctx, job, case)
    assert abs(sums.volume - 27.0) <= 1e-12 and np.isfinite(l).all()


@pytest.mark.parametrize("what", ["detj", "conn", "g1"])
def test_outputs_are_untouched_on_an_error(gpu_ctx, what):
    """The same bad values in DEVICE memory: refused by the device-side checks, and neither F, load_full nor the stress has been
    stored into (det J == 0 is known after the element pass, before the gather)."""
    import torch
    from stan_amd import problem
    job = problem.cube_job(3)
    nn, ne = job.xyz.shape[0], job.conn.shape[0]
    case = T.Case([1.2e-5], np.linspace(10.0, 90.0, nn))
    xyz, conn, typ = job.xyz.copy(), job.conn.copy(), job.elem_type.copy()
    if what == "detj":
        xyz[job.conn[5]] = xyz[job.conn[5]] * [1, 1, 0]
    elif what == "conn":
        conn[7, 3] = 1 << 30
    else:
        typ[6] = hip.HEX8_G1
    g = B.guard_len(job.n_dof)
    mesh = B.Mesh(job, DEV, 1, xyz=xyz, conn=conn, elem_type=typ)
    d_dT = B.input_("dT", case.dT, g, DEV, 1)
    N = job.n_dof - job.n_fixed
    d_F, d_l, d_s = B.output("F", N, g, DEV, 1), B.output("load_full", job.n_dof, g, DEV, 1), B.output("stress", 48 * ne, g, DEV, 1)
    _sync()
    if what != "g1":
        with pytest.raises(hip.StanHipError) as ei:
            _dev_call(gpu_ctx, mesh, case, d_dT, d_F, d_l)
        assert ei.value.code == (hip.E_DETJ if what == "detj" else hip.E_ARG)
    if what != "detj":
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.thermal_stress_hex8_dev(nn, d_dT.ptr, ne, mesh.conn.ptr, mesh.elem_mat.ptr, mesh.elem_type.ptr, mesh.mat_E_nu,
                                            case.mat_alpha, d_s.ptr)
        assert ei.value.code == (hip.E_UNSUPPORTED if what == "g1" else hip.E_ARG)
    _sync()
    B.check(mesh.inputs + [d_dT, d_F, d_l, d_s], written=False)
    for out in (d_F, d_l, d_s):
        assert bool((B._bits(out.payload) == B.UNWRITTEN_BITS).all()), out.name
    # n_elem >= 2^28 is refused before any kernel runs
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.thermal_load_hex8_dev(nn, mesh.xyz.ptr, mesh.node_dof.ptr, 1 << 28, mesh.conn.ptr, mesh.elem_mat.ptr, mesh.elem_type.ptr,
                                      mesh.mat_E_nu, mesh.n_dof, mesh.red.ptr, case.mat_alpha, d_dT.ptr, d_load_full=d_l.ptr)
    assert ei.value.code == hip.E_ARG and "2^28" in str(ei.value)


@pytest.mark.parametrize("kind", ["multi", "comm"])
def test_multi_device_handle_and_communicator_are_refused(built_libs, kind):
    """STAN_E_UNSUPPORTED from every entry on a multi-device handle, and on a single-device context that carries a communicator
    (one rank over the test transport, as tests/rccl_single_worker.py makes it), in a child process.  The phase times are a
    record of the context, not work on its device: refused on a multi-device handle like every entry that names one context,
    zeros on a context with a communicator (no thermal-load call can have run there)."""
    make, word = {"multi": ("ctx = hip.Context(devices=[0, 0])", "multi-device"),
                  "comm": ("ctx = hip.Context(0); ctx.comm_init(0, 1, ctx.unique_id())", "communicator")}[kind]
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from stan_amd import hip, problem
job = problem.cube_job(3)
nn, ne = job.xyz.shape[0], job.conn.shape[0]
alpha, dT = np.array([1.2e-5]), np.full(nn, 50.0)
%s
def attempt(tag, f):
    try:
        print(tag, "NOERROR", f())
    except hip.StanHipError as e:
        print(tag, e.code, %r in str(e))
attempt("HOST", lambda: ctx.thermal_load_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red, alpha, dT)[2])
attempt("STRESS", lambda: ctx.thermal_stress_hex8(dT, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, alpha, np.zeros((ne, 8, 6))).shape)
attempt("TIMES", lambda: list(ctx.thermal_load_times().values()))
t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to("cuda:0")
dx, dd, dc = t(job.xyz, np.float64), t(job.node_dof, np.int32), t(job.conn, np.int32)
dm, dty, dr, dt_ = t(job.elem_mat, np.int32), t(job.elem_type, np.uint8), t(job.red, np.int32), t(dT, np.float64)
dl = torch.zeros(job.n_dof, dtype=torch.float64, device="cuda:0")
ds = torch.zeros(ne * 48, dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
attempt("DEV", lambda: ctx.thermal_load_hex8_dev(nn, dx.data_ptr(), dd.data_ptr(), ne, dc.data_ptr(), dm.data_ptr(), dty.data_ptr(),
                                                 job.mat_E_nu, job.n_dof, dr.data_ptr(), alpha, dt_.data_ptr(), d_load_full=dl.data_ptr()))
attempt("STRESSDEV", lambda: ctx.thermal_stress_hex8_dev(nn, dt_.data_ptr(), ne, dc.data_ptr(), dm.data_ptr(), dty.data_ptr(), job.mat_E_nu,
                                                         alpha, ds.data_ptr()))
torch.cuda.synchronize()
print("UNTOUCHED", bool((dl == 0).all()) and bool((ds == 0).all()))
res = ctx.recover_hex8_keep(job.xyz, np.zeros(job.xyz.shape), job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
attempt("RESULTS", lambda: res.thermal_stress(dT, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, alpha))
res.free()
ctx.close()
print("CLOSED")
''' % (ROOT, make, word)
    env = dict(os.environ, STAN_RCCL_LIB=FAKE)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    for tag in ("HOST", "STRESS", "DEV", "STRESSDEV", "RESULTS"):
        assert tag + " -8 True" in lines, p.stdout
    assert ("TIMES -8 True" if kind == "multi" else "TIMES NOERROR [0.0, 0.0, 0.0]") in lines, p.stdout
    assert "UNTOUCHED True" in lines and "CLOSED" in lines, p.stdout


# ---- 7. console driver ---------------------------------------------------------------------------------------------------
def _write_model(path, n, thermal, alpha=1.2e-5, dT=100.0, point_load=True):
    """The jittered n^3 cube of loads_ref.patch_model with symmetry supports as a .STdb: a point load on the far corner, the two
    thermal BCs -- either may be left out."""
    from stan_amd import host
    m = L.patch_model(n, 0.2, "sym")
    d = host.Db()
    nn, ne = m.xyz.shape[0], m.conn.shape[0]
    d.set_mesh(np.arange(1, nn + 1), m.xyz, np.arange(1, ne + 1), np.ones(ne), m.conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", float(m.mat_E_nu[0, 0]), float(m.mat_E_nu[0, 1]))
    d.assign_part(1, 1, "HEX8_G2")
    flags = (np.rint(m.xyz) == 0).astype(np.float64)
    spc = np.nonzero(flags.any(axis=1))[0]
    d.add_bc(1, "sym", "SPC", spc + 1, flags[spc])
    corner = np.array([nn - 1])
    if point_load:
        d.add_bc(2, "pull", "PointLoad", corner + 1, [[0.0, 0.0, 25.0]])
    if thermal:
        d.add_bc(3, "warm", "Temperature", np.arange(1, nn + 1), np.column_stack([np.full(nn, dT), np.zeros((nn, 2))]))
        d.add_bc(4, "steel", "ThermalExpansion", [1], [[alpha, 0.0, 0.0]])
    d.set_analysis(tol=1e-12)
    d.write_stdb(path)
    return m, corner


def test_console_driver_thermal_loads(gpu_ctx, tmp_path, rho_np):
    """stan_solver --reactions --json on a 4^3 .STdb with "Temperature" + "ThermalExpansion" next to a point load: the block
    and the "thermal" object are the binding's sums for the same model; the stored stresses are the binding's recovery of the
    stored displacements, corrected, bit for bit; the reactions are f_int - l.  With the point load taken out the stored
    displacements are the free expansion alpha dT x and the stored stress vanishes (the bounds of
    test_free_expansion_end_to_end, with the driver's own CG report).  The file without the two BCs has neither the block nor
    the key, the same reduced system, and writes the bytes that the binding's own assembly, solve, recovery and export of that
    file give: nothing changes when no such BC is present."""
    import json
    from stan_amd import host
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    alpha, dT = 1.2e-5, 100.0
    plain, plain0, path = str(tmp_path / "plain.STdb"), str(tmp_path / "plain_as_written.STdb"), str(tmp_path / "model.STdb")
    _write_model(plain, 4, False)
    _write_model(plain0, 4, False)                                  # (the driver overwrites its input)
    m, corner = _write_model(path, 4, True)
    case = T.Case([alpha], np.full(m.xyz.shape[0], dT))
    out0 = subprocess.run([exe, "--reactions", "--json", plain], capture_output=True, text=True, timeout=300)
    assert out0.returncode == 0, out0.stdout + out0.stderr
    assert "Thermal loads" not in out0.stdout and "\"thermal\"" not in out0.stdout
    out = subprocess.run([exe, "--reactions", "--json", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for word in ("Thermal loads:", "Total:", "On free DOFs:", "Heated volume: 6.400000e+01", "mean dT: 1.000000e+02"):
        assert word in out.stdout, out.stdout
    js = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    js0 = json.loads([l for l in out0.stdout.splitlines() if l.startswith("{")][0])
    assert set(js) - set(js0) == {"thermal"} and js["n_reduced"] == js0["n_reduced"] and js["blocks_3x3"] == js0["blocks_3x3"]
    db = host.Db.read_stdb(path)
    db.assign_dof()
    flat, (red, n_fixed, F0) = db.flat(), db.reduction()
    job = _with(m, xyz=flat["xyz"], conn=flat["conn"], node_dof=flat["node_dof"], red=red)
    F, l, sums = thermal(gpu_ctx, job, case, F=F0)
    q = js["thermal"]
    assert q["load_sum"] == list(sums.load_sum) and q["free_sum"] == list(sums.free_sum) and q["n_fixed"] == sums.n_fixed == n_fixed
    assert q["volume"] == sums.volume and q["dT_integral"] == sums.dT_integral and q["mean_dT"] == sums.dT_integral / sums.volume
    # stored results: the recovery of the stored displacements, corrected
    disp, strain, stress = db.results(1)
    s_raw_e, s_raw = gpu_ctx.recover_hex8(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    assert strain.tobytes() == s_raw_e.tobytes() and stress.tobytes() == corrected(gpu_ctx, job, case, s_raw).tobytes()
    assert np.abs(stress - s_raw).max() > 1.0
    # reactions: f_int - l at the fixed DOFs; the equilibrium check saw the whole external F
    f_int, reaction, eq = gpu_ctx.internal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type,
                                                       job.mat_E_nu, job.red, F)
    e = js["equilibrium"]
    fixed = job.red == -1
    d = np.asarray(job.node_dof).reshape(-1, 3)
    for c in range(3):
        lc = l[d[:, c]][fixed[d[:, c]]]
        assert abs(e["reaction_sum"][c] - (eq.reaction_sum[c] - lc.sum())) <= len(lc) * 2.0 ** -52 * (np.abs(lc).sum() + abs(eq.reaction_sum[c]))
        assert e["load_sum"][c] == eq.load_sum[c] and e["fint_sum"][c] == eq.fint_sum[c]
    assert e["residual_norm2"] == eq.residual_norm2 and e["residual_norm2"] < 1e-6 * e["load_norm2"]
    # the supports balance the point load alone, the thermal load is self-equilibrated: sum_fixed (f_int - l) + P =
    # sum_all f_int + sum_free (F - f_int) - sum_all l, so within |fint_sum| + sqrt(N) |F - f_int|_2 + |load_sum of l| and the
    # roundings of those sums
    N = int((~fixed).sum())
    for c, P in enumerate((0.0, 0.0, 25.0)):
        tol = (abs(e["fint_sum"][c]) + np.sqrt(N) * e["residual_norm2"] + abs(sums.load_sum[c]) +
               job.n_dof * 2.0 ** -52 * (np.abs(f_int).sum() + np.abs(l).sum() + np.abs(F).sum()))
        print("driver, direction %d: reactions %.9e + point load %.1f = %.3e <= %.3e" % (c, e["reaction_sum"][c], P, e["reaction_sum"][c] + P, tol))
        assert abs(e["reaction_sum"][c] + P) <= tol and tol < 1e-3
    # the file without the BCs goes the way it went before there were thermal loads: its output is, byte for byte, the
    # binding's own assembly, solve (the file's tolerance and iteration limit, the context's defaults), recovery and export
    db0 = host.Db.read_stdb(plain0)
    db0.assign_dof()
    red0, _, Fp = db0.reduction()
    assert np.array_equal(red0, job.red)
    K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    try:
        U0, rep0 = K.cg_solve(Fp, 1e-12)
    finally:
        K.free()
    d0 = host.nodal_displacements(job.node_dof, job.red, U0).reshape(-1, 3)
    e0, s0 = gpu_ctx.recover_hex8(job.xyz, d0, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    disp0, strain0, stress0 = host.Db.read_stdb(plain).results(1)
    assert rep0["iterations"] == js0["cg_iterations"] and disp0.tobytes() == d0.tobytes()
    assert strain0.tobytes() == e0.tobytes() and stress0.tobytes() == s0.tobytes()
    mine = str(tmp_path / "plain_binding.STdb")
    db0.write_stdb_with_results(mine, d0, e0, s0)
    assert open(mine, "rb").read() == open(plain, "rb").read()
    assert js0["equilibrium"]["load_sum"] == [0.0, 0.0, 25.0]


def test_console_driver_free_expansion(gpu_ctx, tmp_path, rho_np, rho_np_forces):
    """The same file without its point load, on the kept-on-device path and with --object-results: the stored displacements
    are alpha dT x and the stored stresses vanish, within the bounds of test_free_expansion_end_to_end formed with the driver's
    own rel_residual; both paths store the same bytes."""
    import json
    from stan_amd import host
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    alpha, dT = 1.2e-5, 100.0
    stored = []
    for flag in ([], ["--object-results"]):
        path = str(tmp_path / ("free%d.STdb" % len(flag)))
        m, _ = _write_model(path, 4, True, alpha, dT, point_load=False)
        out = subprocess.run([exe, "--json"] + flag + [path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        js = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        stored.append((host.Db.read_stdb(path).results(1), js, open(path, "rb").read()))
    assert stored[0][2] == stored[1][2]
    (disp, strain, stress), js, _ = stored[0]
    E, nu = m.mat_E_nu[0]
    case = T.Case([alpha], np.full(m.xyz.shape[0], dT))
    bdT = float(T.beta(m, case.mat_alpha)[0]) * dT
    u_ex = alpha * dT * m.xyz                                       # (zero at the fixed DOFs, as the driver stores them)
    F, _, _ = thermal(gpu_ctx, m, case, F=np.zeros(m.n_dof - m.n_fixed))
    _, rep, diag, lam_min, _ = _solve(gpu_ctx, m, F)               # the diagonal and lambda_min of K; the report is the driver's
    rep = dict(rep, rel_residual=js["rel_residual"])
    _, a = R.reference(m, u_ex)
    _, aU = R.reference(m, disp)
    free = m.red != -1
    cap = 4 * (rho_np_forces * a + rho_np * T.scale(m, case)) * U52
    u_bound = (_residual_bound(rep, diag, aU[free], np.linalg.norm(F), rho_np_forces) + np.linalg.norm(cap[free])) / lam_min
    err = np.linalg.norm(disp - u_ex)
    lam, G = (E * nu) / ((1 - 2 * nu) * (1 + nu)), 0.5 * E / (1 + nu)
    chain = (3 * lam + 2 * G) * 16 * L.grad_max(m) * 3 * np.sqrt(3.0)
    s_bound = chain * (u_bound + 64 * U52 * np.abs(u_ex).max()) + 2 * U52 * bdT
    print("driver: rel_residual %.3e, |U - alpha dT x|_2 %.3e <= %.3e; max |stored stress| %.3e <= %.3e (beta dT %.3e)" %
          (js["rel_residual"], err, u_bound, np.abs(stress).max(), s_bound, bdT))
    assert err <= u_bound and u_bound < 1e-6 * np.linalg.norm(u_ex)
    assert np.abs(stress).max() <= s_bound and s_bound < 1e-2 * bdT


# ---- 8. phase times ------------------------------------------------------------------------------------------------------
def test_phase_times(gpu_ctx):
    """stan_hip_thermal_load_times: zero without profiling, the three phases of the last call with it."""
    m, case = T.cases()["cube5-rand"]
    thermal(gpu_ctx, m, case)
    assert list(gpu_ctx.thermal_load_times().values()) == [0.0, 0.0, 0.0]
    gpu_ctx.set_profiling(True)
    try:
        thermal(gpu_ctx, m, case)
        t = gpu_ctx.thermal_load_times()
    finally:
        gpu_ctx.set_profiling(False)
    assert all(0.0 < v < 100.0 for v in t.values()), t
