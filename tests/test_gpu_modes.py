"""Modal analysis on the device: the lumped mass against the load-vector entry bit for bit, the block
kernels alone against np.longdouble, stan_hip_modes against scipy's dense eigen-solve of the exported K (tests/modes_ref.py),
its reproducibility, what it leaves of K, and its error cases.

Bounds.  gram: an entry of A is a sum of N fused multiply-adds in some order: at most N roundings on the way, N 2^-53 sum |z w|
(first order, any order).  A term of B is (z_i z_j) m: one rounding more before it is added, (N + 1) 2^-53 sum |z_i m z_j|.
rotate: q fused multiply-adds, q 2^-53 sum_l |z_l Q_lj|.  modes: the bounds of the issue, see each test."""
import numpy as np
import pytest

from tests import device_buffers as DB
from tests import modes_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
TOL = 1e-6


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, K, M, ref): K assembled once per model, the reference from K.to_csr()."""
    made = {}

    def get(name):
        if name not in made:
            j = R.job(name)
            K = gpu_ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
            M, mass_node, _ = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red,
                                                       R.mat_rho(name))
            ref = R.reference(name, R.dense(*K.to_csr(upper_only=False)))
            made[name] = dict(job=j, K=K, M=M, mass_node=mass_node, ref=ref)
        return made[name]

    yield get
    for m in made.values():
        m["K"].free()


# ---- 1. mass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.MODELS)
def test_mass_has_the_bits_of_the_load_vector_entry(gpu_ctx, name):
    import torch
    j, rho = R.job(name), R.mat_rho(name)
    body = np.zeros((len(rho), 3))
    body[:, 0] = rho
    _, _, lf, ls = gpu_ctx.load_vector_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, mat_body=body)
    M, mass_node, sums = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, rho)
    d0 = np.asarray(j.node_dof).reshape(-1, 3)[:, 0]
    assert np.array_equal(mass_node.view(np.int64), lf[d0].view(np.int64))
    full = np.zeros(j.n_dof)
    for c in range(3):
        full[d0 + c] = mass_node
    free = np.asarray(j.red) != -1
    assert np.array_equal(M.view(np.int64), full[free].view(np.int64))
    # the numpy restatement, to the rounding of positive sums; the sums by direction
    Mn, mn, _, vol = R.lumped_mass(j, rho)
    assert np.abs(mass_node - mn).max() <= 32 * U53 * mn.max()
    assert sums.volume == ls.volume and sums.n_fixed == j.n_fixed
    assert abs(sums.total_mass - mn.sum()) <= 64 * U53 * mn.sum()
    for c in range(3):
        assert abs(sums.free_sum[c] + sums.fixed_sum[c] - sums.total_mass) <= 64 * U53 * sums.total_mass
    assert abs(sum(sums.free_sum) - M.sum()) <= 64 * U53 * M.sum()
    # the device-pointer entry: same bits, nothing beside the outputs, inputs untouched, every entry stored
    dev = torch.device("cuda:0")
    mesh = DB.Mesh(j, dev, offset=1)
    g = DB.guard_len(j.n_dof)
    dM, dn = DB.output("M", j.n_red, g, dev, 1), DB.output("mass_node", j.xyz.shape[0], g, dev, 3)
    torch.cuda.synchronize()
    s2 = gpu_ctx.lumped_mass_hex8_dev(*mesh.assemble_args(), rho, d_M=dM.ptr, d_mass_node=dn.ptr)
    DB.check(mesh.inputs + [dM, dn])
    assert np.array_equal(dM.numpy().view(np.int64), M.view(np.int64))
    assert np.array_equal(dn.numpy().view(np.int64), mass_node.view(np.int64))
    assert s2.as_dict() == sums.as_dict()
    # an output alone has the same bits
    M1, n1, q1 = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, rho,
                                          mass_node=False, sums=False)
    assert n1 is None and q1 is None and np.array_equal(M1.view(np.int64), M.view(np.int64))


def test_mass_error_cases(gpu_ctx):
    import torch
    from stan_amd import hip
    j = R.job("two_mat")
    args = (j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    for rho in ([-1.0, 1.0], [1.0, float("nan")], [float("inf"), 1.0], None):
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.lumped_mass_hex8(*args, rho)
        assert ei.value.code == hip.E_ARG, rho
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.lumped_mass_hex8(*args, [1.0, 1.0], M=False, mass_node=False, sums=False)
    assert ei.value.code == hip.E_ARG
    # material 1 without mass: a node all of whose elements are of material 1 has free DOFs and no mass
    mats = np.asarray(j.elem_mat)
    only1 = np.ones(j.xyz.shape[0], bool)
    only1[np.unique(j.conn[mats == 0])] = False
    d0 = np.asarray(j.node_dof).reshape(-1, 3)[:, 0]
    free_node = (np.asarray(j.red)[d0[:, None] + np.arange(3)] != -1).any(axis=1)
    want = np.nonzero(only1 & free_node)[0]
    j2 = j
    if want.size == 0:      # every node touches material 0: take all mass away instead
        rho0, first = [0.0, 0.0], int(np.nonzero(free_node)[0][0])
    else:
        rho0, first = [1.0, 0.0], int(want[0])
    dev = torch.device("cuda:0")
    mesh = DB.Mesh(j2, dev)
    g = DB.guard_len(j.n_dof)
    dM, dn = DB.output("M", j.n_red, g, dev), DB.output("mass_node", j.xyz.shape[0], g, dev)
    torch.cuda.synchronize()
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.lumped_mass_hex8_dev(*mesh.assemble_args(), rho0, d_M=dM.ptr, d_mass_node=dn.ptr)
    assert ei.value.code == hip.E_ARG and ("node %d " % first) in str(ei.value)
    DB.check(mesh.inputs + [dM, dn], written=False)
    for out in (dM, dn):       # on an error nothing is written
        assert bool((out.payload.view(torch.int64) == DB.UNWRITTEN_BITS).all())


# ---- 2. the block kernels alone -----------------------------------------------------------------------------------------------
def _block(N, q, seed):
    rng = np.random.default_rng(seed)
    mk = lambda: rng.standard_normal((q, N)) * 10.0 ** rng.uniform(-3, 3, (q, N))
    return mk(), mk(), 10.0 ** rng.uniform(-3, 3, N)


GRAM_N = (1, 63, 64, 65, 4097, 200003)
GRAM_Q = (1, 2, 5, 8, 12, 16, 17, 32)


@pytest.mark.parametrize("N", GRAM_N)
def test_gram_against_longdouble(gpu_ctx, N):
    for q in GRAM_Q:
        Z, W, M = _block(N, q, 1000 * q + N % 997)
        A, B = gpu_ctx.block_gram(Z, W, M)
        Zl, Wl, Ml = Z.astype(LD), W.astype(LD), M.astype(LD)
        Ar, Br = Zl @ Wl.T, (Zl * Ml[None, :]) @ Zl.T
        As, Bs = np.abs(Zl) @ np.abs(Wl).T, (np.abs(Zl) * Ml[None, :]) @ np.abs(Zl).T
        ea = (np.abs(A.astype(LD) - Ar) / (N * U53 * As)).max()
        eb = (np.abs(B.astype(LD) - Br) / ((N + 1) * U53 * Bs)).max()
        print("gram N=%d q=%d: A %.3f of its bound, B %.3f" % (N, q, ea, eb))
        assert ea <= 1.0 and eb <= 1.0, (N, q, float(ea), float(eb))
        assert np.array_equal(B, B.T), (N, q)          # B is symmetric to the bit
        A2, _ = gpu_ctx.block_gram(Z, Z, M)              # Z^T Z: fused multiply-adds of commuting products
        assert np.array_equal(A2, A2.T), (N, q)
        A3, B3 = gpu_ctx.block_gram(Z, W, M)
        assert np.array_equal(A3.view(np.int64), A.view(np.int64)) and np.array_equal(B3.view(np.int64), B.view(np.int64))


@pytest.mark.parametrize("N", (1, 255, 257, 4097))
def test_rotate_against_longdouble(gpu_ctx, N):
    for q in (1, 5, 8, 9, 16, 17, 24, 25, 32):
        Z, W, M = _block(N, q, 77 * q + N)
        rng = np.random.default_rng(q)
        Q = rng.standard_normal((q, q))
        lam = 10.0 ** rng.uniform(0, 2, q)
        rhs0 = rng.standard_normal((q, N))
        Zl, Wl, Ql = Z.astype(LD), W.astype(LD), Q.astype(LD)
        Xr, KXr = Ql.T @ Zl, Ql.T @ Wl
        Xs, KXs = np.abs(Ql).T @ np.abs(Zl), np.abs(Ql).T @ np.abs(Wl)
        got = {}
        for in_place in (False, True):
            for mask in (np.zeros(q, np.uint8), np.ones(q, np.uint8), (np.arange(q) % 2).astype(np.uint8)):
                X, KX, rhs, rho2 = gpu_ctx.block_rotate(Z, W, M, Q, lam, mask=mask, in_place=in_place, rhs=rhs0)
                assert (np.abs(X.astype(LD) - Xr) <= q * U53 * Xs).all(), (N, q, in_place)
                assert (np.abs(KX.astype(LD) - KXr) <= q * U53 * KXs).all(), (N, q, in_place)
                # the residual, its norm and the next right-hand side from the device's own X and KX (fp64 operations,
                # one rounding each: 4 on R where nothing cancels, so compared on the scale of its terms)
                Rr = KX.astype(LD) - (M.astype(LD)[None, :] * X.astype(LD)) * lam.astype(LD)[:, None]
                Rs = np.abs(KX) + np.abs(M[None, :] * X) * lam[:, None]
                keep = mask.astype(bool)
                assert np.array_equal(rhs[keep], rhs0[keep]), (N, q, "masked columns stay")
                assert (np.abs(rhs[~keep].astype(LD) + Rr[~keep] / lam[~keep, None]) <= 4 * U53 * Rs[~keep] / lam[~keep, None]).all()
                r2 = (Rr * Rr / M.astype(LD)[None, :]).sum(axis=1)
                r2s = ((Rs * Rs) / M[None, :]).sum(axis=1)
                assert (np.abs(rho2.astype(LD) - r2) <= (N + 12) * U53 * r2s).all(), (N, q)
                key = bytes(mask)
                if key in got:        # aliased and unaliased: the same bits
                    for a, b in zip(got[key], (X, KX, rhs, rho2)):
                        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (N, q)
                got[key] = (X, KX, rhs, rho2)
        X2 = gpu_ctx.block_rotate(Z, W, M, Q, lam)[0]
        assert np.array_equal(X2.view(np.int64), got[bytes(np.zeros(q, np.uint8))][0].view(np.int64))


# ---- 3. modes -------------------------------------------------------------------------------------------------------------
_ORTH = {}


@pytest.mark.parametrize("name", R.MODELS)
def test_modes_against_the_dense_eigen_solve(gpu_ctx, models, name):
    m = models(name)
    K, M, ref = m["K"], m["M"], m["ref"]
    k, lam_ref, Kd = ref["k"], ref["lam"], ref["Kd"]
    assert np.array_equal(M.view(np.int64), ref["M"].view(np.int64)) or np.abs(M - ref["M"]).max() <= 32 * U53 * M.max()
    lam, phi, rho, rep = K.modes(M, k, tol=TOL)
    print(name, "k", k, rep, "rho", rho)
    assert rep["converged"] == 1 and rep["block"] == R.block_size(M.shape[0], k) and rep["cg_worst_type"] in (1, 7)
    assert (rho <= TOL).all() and rep["max_rho"] == rho.max()
    assert (R.rho_host(Kd, M, lam, phi) <= 2 * TOL).all()
    assert (np.diff(lam) >= 0).all()
    assert (np.abs(lam - lam_ref[:k]) <= 2 * TOL * lam_ref[:k]).all(), np.abs(lam / lam_ref[:k] - 1)
    for a, b, gap in R.clusters(lam_ref, k):
        s = R.sin_max_angle(phi[a:b].T, ref["Phi"][:, a:b], M)
        bound = 2 * (rho[a:b] * lam[a:b]).max() / gap
        print("  cluster", a, b, "sin %.3e bound %.3e" % (s, bound))
        assert s <= bound, (a, b, s, bound)
    for x in phi:
        i = int(np.argmax(np.abs(x)))
        assert x[i] > 0
    # M-orthonormality: 4 x what the numpy restatement of the loop leaves on the same model
    r = R.restatement(Kd, M, k, tol=TOL)
    orth_np = np.abs((r["phi"] * M[None, :]) @ r["phi"].T - np.eye(k)).max()
    orth = np.abs((phi * M[None, :]) @ phi.T - np.eye(k)).max()
    _ORTH[name] = (orth, orth_np)
    print("  orthonormality: device %.3e, numpy restatement %.3e" % (orth, orth_np))
    assert orth <= 4 * orth_np, (orth, orth_np)


# ---- 4. max_outer = 1 -----------------------------------------------------------------------------------------------------
def test_one_outer_step_reports_honest_residuals(models):
    m = models("cube6j")
    k = m["ref"]["k"]
    lam, phi, rho, rep = m["K"].modes(m["M"], k, tol=TOL, max_outer=1)
    assert rep["converged"] == 0 and rep["outer"] == 1
    host = R.rho_host(m["ref"]["Kd"], m["M"], lam, phi)
    assert (rho > TOL).any()
    assert (rho <= 2 * host).all() and (host <= 2 * rho).all(), (rho, host)


# ---- 5. reproducibility, the _dev entry, K afterwards -----------------------------------------------------------------------
def test_same_bits_twice_from_device_pointers_and_k_afterwards(gpu_ctx, models):
    import torch
    m = models("cube6")
    j, K, M, k = m["job"], m["K"], m["M"], m["ref"]["k"]
    first = K.modes(M, k, tol=TOL)
    again = K.modes(M, k, tol=TOL)
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert {x: v for x, v in first[3].items() if not x.endswith("_ms")} == {x: v for x, v in again[3].items() if not x.endswith("_ms")}
    dev = torch.device("cuda:0")
    N = M.shape[0]
    g = DB.guard_len(N)
    dM = DB.input_("M", M, g, dev, 1)
    outs = [DB.output("lambda", k, g, dev, 1), DB.output("phi", k * N, g, dev, 3), DB.output("rho", k, g, dev, 5)]
    torch.cuda.synchronize()
    rep = K.modes_dev(dM.ptr, k, outs[0].ptr, outs[1].ptr, outs[2].ptr, tol=TOL)
    DB.check([dM] + outs)
    assert rep["converged"] == 1
    for a, o in zip(first[:3], outs):
        assert np.array_equal(a.reshape(-1).view(np.int64), o.numpy().view(np.int64)), o.name
    # K afterwards: a solve has the bits it has on a fresh assembly
    U, r = K.cg_solve(j.F, 1e-10)
    K2 = gpu_ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    U2, r2 = K2.cg_solve(j.F, 1e-10)
    K2.free()
    assert r == r2 and np.array_equal(U.view(np.int64), U2.view(np.int64))


# ---- 6. error cases -------------------------------------------------------------------------------------------------------
def test_modes_error_cases(gpu_ctx, models):
    from stan_amd import hip
    m = models("cube6")
    K, M = m["K"], m["M"]
    N = M.shape[0]

    def code(call):
        with pytest.raises(hip.StanHipError) as ei:
            call()
        return ei.value.code

    assert code(lambda: K.modes(M, 0)) == hip.E_ARG
    assert code(lambda: K.modes(M, N + 1)) == hip.E_ARG
    assert code(lambda: K.modes(M, 25)) == hip.E_ARG               # a block of 33 columns
    assert code(lambda: K.modes(M, 4, tol=-1.0)) == hip.E_ARG
    assert code(lambda: K.modes(M, 4, solve_eps=-1e-6)) == hip.E_ARG
    assert code(lambda: K.modes(M, 4, max_outer=-1)) == hip.E_ARG
    assert code(lambda: K.modes(M, 4, solve_max_its=-1)) == hip.E_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        M2 = M.copy()
        M2[N // 2] = bad
        assert code(lambda: K.modes(M2, 4)) == hip.E_ARG, bad
    assert code(lambda: K.modes_dev(None, 4, None, None, None)) == hip.E_ARG          # NULL pointers
    other = hip.Context(0)
    try:
        k_here = K.ctx
        K.ctx = other              # the handle of another context with this context's K
        assert code(lambda: K.modes(M, 4)) == hip.E_ARG
        K.ctx = k_here
    finally:
        K.ctx = k_here
        other.close()
    # a multi-device handle (one device, no communicator): refused
    j = m["job"]
    multi = hip.Context(devices=[0])
    try:
        Km = multi.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        assert code(lambda: Km.modes(M, 4)) == hip.E_UNSUPPORTED
        assert code(lambda: multi.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red,
                                                   R.mat_rho("cube6"))) == hip.E_UNSUPPORTED
        assert code(lambda: multi.block_gram(np.ones((2, 8)), np.ones((2, 8)), np.ones(8))) == hip.E_UNSUPPORTED
        Km.free()
    finally:
        multi.close()
    # a context with a communicator (a detached rank of two): refused, with a reason of its own
    ranked = hip.Context(0)
    try:
        ranked.comm_init(0, 2, None)
        Kr = ranked.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        with pytest.raises(hip.StanHipError) as ei:
            Kr.modes(np.ones(Kr.info()["n_reduced"]), 2)
        assert ei.value.code == hip.E_UNSUPPORTED and "communicator" in str(ei.value) and "chunk boundary" not in str(ei.value)
        assert code(lambda: ranked.block_gram(np.ones((2, 8)), np.ones((2, 8)), np.ones(8))) == hip.E_UNSUPPORTED
        Kr.free()
    finally:
        ranked.close()
    # the model still solves after all of it
    lam = K.modes(M, 2, tol=TOL)[0]
    assert (np.abs(lam - m["ref"]["lam"][:2]) <= 2 * TOL * m["ref"]["lam"][:2]).all()


# ---- 7. console -----------------------------------------------------------------------------------------------------------
def _console_db(path, density):
    from stan_amd import host
    from stan_amd.cube import cube_mesh
    xyz, conn = cube_mesh(4)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", 210000.0, 0.3)
    d.assign_part(1, 1, "HEX8_G2")
    fixed = np.nonzero(xyz[:, 0] == 0.0)[0]
    d.add_bc(1, "fix", "SPC", fixed + 1, np.ones((fixed.size, 3)))
    if density:
        d.add_bc(2, "rho", "Density", [1], np.array([[R.RHO, 0.0, 0.0]]))
    d.set_analysis(tol=1e-10)
    d.assign_dof()
    d.write_stdb(path)
    return xyz.shape[0]


def test_console_modes(tmp_path, built_libs):
    import json
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "m.STdb"), str(tmp_path / "out")
    n_nodes = _console_db(path, True)
    original = before = open(path, "rb").read()
    out = subprocess.run([exe, "--modes", "4", "--json", "--vtu", prefix, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    assert "Natural frequencies:" in out.stdout
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    m = json.loads(line)["modes"]
    assert set(m) >= {"n_modes", "block", "outer", "converged", "cg_iterations", "lambda", "frequency_hz", "rho", "total_mass"}
    assert m["n_modes"] == 4 and m["block"] == 8 and m["converged"] == 1 and len(m["lambda"]) == 4
    lam = np.array(m["lambda"])
    assert np.array_equal(np.array(m["frequency_hz"]), np.sqrt(lam) / (2 * np.pi)) or \
        np.abs(np.array(m["frequency_hz"]) / (np.sqrt(lam) / (2 * np.pi)) - 1).max() <= 4 * U53
    assert (np.diff(lam) >= 0).all() and (np.array(m["rho"]) <= 1e-6).all()
    assert abs(m["total_mass"] - R.RHO * 64.0) <= 64 * U53 * R.RHO * 64.0
    # the console block carries the same numbers
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Natural frequencies:")[1], flags=re.M)[:4]
    assert [int(r[0]) for r in rows] == [1, 2, 3, 4]
    assert np.allclose([float(r[1]) for r in rows], lam, rtol=1e-8) and np.allclose([float(r[2]) for r in rows], m["frequency_hz"], rtol=1e-8)
    for k in range(1, 5):
        text = open("%s_mode_%03d.vtu" % (prefix, k), "rb").read()      # (the arrays are appended raw: bytes)
        for name in ("Mode Shape X", "Mode Shape Y", "Mode Shape Z", "Magnitude"):
            assert ('Name="%s"' % name).encode() in text, (k, name)
        assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    assert not os.path.exists("%s_mode_005.vtu" % prefix) and not os.path.exists(prefix + "_001.vtu")
    # without "Density" the run is refused and the file is untouched; so is a run on several devices
    plain = str(tmp_path / "plain.STdb")
    _console_db(plain, False)
    before = open(plain, "rb").read()
    out = subprocess.run([exe, "--modes", "4", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "Density" in out.stderr and open(plain, "rb").read() == before
    out = subprocess.run([exe, "--modes", "4", "--devices", "0,0", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "one device" in out.stderr and open(path, "rb").read() == original
