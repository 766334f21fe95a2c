"""Internal forces, reactions and the equilibrium check (stan_hip_internal_forces_hex8), the parts that need no GPU: the
C-ABI surface, the reference of the GPU tests (tests/forces_ref.py) against the oracle's assembled matrix, and the console
driver's flag."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import forces_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_header_exports_and_binding(built_libs):
    from stan_amd import hip
    h = open(os.path.join(ROOT, "include", "stan_hip.h")).read()
    lib = hip.load()
    for f in ("stan_hip_internal_forces_hex8", "stan_hip_internal_forces_hex8_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % f, h), f
        assert f in hip.EXPORTS and hasattr(lib, f), f
    body = re.search(r"typedef\s+struct\s+stan_equilibrium\s*\{(.*?)\}\s*stan_equilibrium\s*;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [re.sub(r"\s+", " ", x.strip()) for x in body.split(";") if x.strip()]
    assert fields == ["double reaction_sum[3]", "double load_sum[3]", "double fint_sum[3]", "double residual_norm2",
                      "double load_norm2", "double residual_max", "int64_t residual_max_dof", "int64_t n_fixed"]
    assert [n for n, _ in hip.Equilibrium._fields_] == [x.split()[1].split("[")[0] for x in fields]
    assert ctypes.sizeof(hip.Equilibrium) == 9 * 8 + 3 * 8 + 2 * 8
    assert callable(hip.Context.internal_forces_hex8) and callable(hip.Context.internal_forces_hex8_dev)
    names = [n for n, _ in hip.Profile._fields_]
    assert names[-3:] == ["forces_elem_ms", "forces_list_ms", "forces_gather_ms"]       # appended: the struct is ABI
    assert names[-4] == "scalars_point_ms"
    cs = open(os.path.join(ROOT, "integration", "StanHip.cs")).read()
    assert "struct StanEquilibrium" in cs and "stan_hip_internal_forces_hex8_dev" in cs
    hh = open(os.path.join(ROOT, "stan_amd", "host", "solver_functions.h")).read()
    assert re.search(r"\bvoid\s+Equilibrium\s*\(", hh)


def test_reference_against_the_oracles_assembled_matrix(built_libs, oracle):
    """f_ref = sum_e K_e u_e (longdouble) against K u with K assembled by the oracle with no fixed DOF on a jittered 3^3
    cube: the assembled product rounds differently (entries summed over elements first, then a row of up to 81 terms) and
    must agree within 4 rho_np units of 2^-52 a.  The numpy Gauss-point restatement is held to its own yardstick."""
    rho_np = R.rho_np(verbose=True)
    m = R.jittered_cube(3)
    disp = R.random_disp(m, 7)
    rc, A = oracle.assemble(m.xyz, m.node_dof, m.conn, m.elem_mat, m.elem_type, m.mat_E_nu, np.zeros(m.n_dof, np.int32))
    assert rc == 0 and A.n == m.n_dof
    u = np.zeros(m.n_dof)
    u[np.asarray(m.node_dof).reshape(-1)] = disp.reshape(-1)
    f_ref, a = R.reference(m, disp)
    rho_ku = R.rho(oracle.smv_upper(A, u), f_ref, a)
    rho_gp = R.rho(R.fint_gauss(m, disp), f_ref, a)
    print("rho_np %.2f; K u of the assembled matrix: rho %.2f; Gauss-point restatement here: rho %.2f" % (rho_np, rho_ku, rho_gp))
    assert (a > 0).all() and np.abs(f_ref).max() > 0
    assert rho_ku <= 4 * rho_np
    assert rho_gp <= 4 * rho_np and 0 < rho_np < 64
    # the reference restates the scatter: every corner counts, a collapsed hex gives both, an unreferenced node gets 0
    one = R.model(*R.strip_mesh(1))
    one.conn = np.array([[0, 1, 2, 0, 4, 5, 6, 4]], dtype=np.int32)      # nodes 3 and 7 unreferenced
    fe = np.arange(1.0, 25.0).reshape(1, 8, 3)
    f = R.scatter(one, fe, np.float64).reshape(-1)
    nd = np.asarray(one.node_dof).reshape(-1, 3)
    assert f[nd[0, 0]] == fe[0, 0, 0] + fe[0, 3, 0] and f[nd[4, 2]] == fe[0, 4, 2] + fe[0, 7, 2]
    assert (f[nd[3]] == 0).all() and (f[nd[7]] == 0).all()


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


def test_console_flag_without_a_gpu_fails_loudly(built_libs, tmp_path):
    """stan_solver --reactions --json: known to the driver (refused with several devices before anything is read); without
    a GPU the run fails at the device context, as every run does, and leaves the input file alone."""
    import torch
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    path = str(tmp_path / "model.STdb")
    _write_model(path, 2)
    before = open(path, "rb").read()
    out = subprocess.run([exe, "--reactions", "--devices", "0,0", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--reactions works on one device" in out.stderr, out.stdout + out.stderr
    assert open(path, "rb").read() == before
    assert "--reactions" in subprocess.run([exe], capture_output=True, text=True, timeout=60).stderr      # the usage line
    out = subprocess.run([exe, "--reactions", "--json", path], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert out.returncode == 0 and '"equilibrium"' in out.stdout and "Support reactions" in out.stdout, out.stdout + out.stderr
    else:
        assert out.returncode != 0 and "ERROR" in out.stderr, out.stdout + out.stderr
        assert '"equilibrium"' not in out.stdout and "Support reactions" not in out.stdout
        assert open(path, "rb").read() == before
