"""Linear buckling on the device: the element scalars of the geometric stiffness against np.longdouble,
the assembled G bit for bit against the ordered sum of the device's own element scalars, the two new block kernels against
np.longdouble, stan_hip_buckling against scipy's eigh(H, K) of the exported matrices (tests/buckling_ref.py), reproducibility,
what the calls leave of K and of G, the error cases and the console.

Bounds.  Element scalars: 4 x what the plain-fp64 restatement reads over the same family in units of each entry's rounding
scale (B.DEVICE_KG_UNITS = 4 x 0.364 = 1.456; the yardstick is the restatement, never the device).  Measured on the first GPU run: the
device reads 0.572 units at worst (the random field on "aspect_rot", HEX8_G2), the restatement 0.364.  Products on G: a row adds at most nnz_row terms, nnz_row 2^-53 sum |terms|.  Block kernels: q
fused multiply-adds for X; for R a term is fma(mu, w, -y) times Q, added by a fused multiply-add: two roundings per term and
none that is not, (2q + 1) 2^-53 sum (|mu w| + |y|) |Q|.  Factors: the bounds of the issue, see the test."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import buckling_ref as B
from tests import device_buffers as DB
from tests import element_ref as E
from tests import modes_ref as MR

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
MODELS = MR.MODELS + ("column20",)
# (k, tol) per model, found on the CPU with the restatement on the oracle's K by pick_k's rule (the smallest k >= 4 with a
# relative gap > 1e-3 behind it and k positive mu), k lowered until the restatement converges within 150 outer steps:
#   column20      k = 4 at once (11 steps)
#   perforated12  k = 4 does not within 150, k = 3 does in 92
#   two_mat       k = 4 takes 191, k = 2 takes 120
#   cube6, cube6j under their transverse tip load have a spectrum symmetric in sign (half the block serves the reversed load)
#                 and factors 9 to 11 % apart: at tol 1e-6 k = 4 takes 287 steps, k = 2 179 and k = 1 153 -- no k meets the
#                 condition (the shifted pencil of DESIGN.md section 8 is what such a model wants).  They run with k = 1 at
#                 tol 1e-5, which the restatement reaches in 129 steps; every bound below is relative to the device's own
#                 residuals, so it asks the same of these two.
# The fixture checks the conditions again on the exported matrices (B.input_conditions).
CASES = {"cube6": (1, 1e-5), "cube6j": (1, 1e-5), "perforated12": (3, 1e-6), "two_mat": (2, 1e-6), "column20": (4, 1e-6)}


def _job(name):
    return B.column_job(20) if name == "column20" else MR.job(name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _mesh_args(j):
    return (j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


def _device_scalars(ctx, j, disp):
    """s [n_elem, 8, 8] from stan_hip_kg_hex8_batch, material by material"""
    X, u = j.xyz[j.conn], np.asarray(disp).reshape(-1, 3)[j.conn]
    s36 = np.zeros((j.conn.shape[0], 36))
    for m, (Em, nu) in enumerate(np.asarray(j.mat_E_nu).reshape(-1, 2)):
        sel = np.nonzero(np.asarray(j.elem_mat) == m)[0]
        if sel.size:
            s36[sel] = ctx.kg_hex8_batch(X[sel], u[sel], Em, nu, np.asarray(j.elem_type)[sel])
    return B.untri(s36)


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, K, U, disp, G, Kd, Hd, ref): K assembled and solved once per model under its own load, G from that U,
    the reference from the exported matrices; computed once and left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            j = _job(name)
            K = gpu_ctx.assemble_hex8(*_mesh_args(j))
            csr0 = K.to_csr(upper_only=False)
            U, rep = K.cg_solve(j.F, 1e-12)
            assert rep["terminationtype"] in (1, 7)
            disp = B.disp_full(j, U)
            G = K.geometric_stiffness(j.xyz, disp, *_mesh_args(j)[1:])
            Kd, Hd = MR.dense(*csr0), -MR.dense(*G.to_csr(upper_only=False))
            mu_ref, Phi, low = B.eigh_ref(Hd, Kd, B.N_REF)
            k, tol = CASES[name]
            rest = B.input_conditions(Kd, Hd, mu_ref, k, tol, limit=150)
            made[name] = dict(job=j, K=K, U=U, disp=disp, G=G, Kd=Kd, Hd=Hd, csr0=csr0, mu_ref=mu_ref, Phi=Phi, low=low, k=k, tol=tol,
                              rest=rest)
        return made[name]

    yield get
    for m in made.values():
        m["G"].free()
        m["K"].free()


# ---- 1. the element scalars ---------------------------------------------------------------------------------------------------
def test_element_scalars_against_longdouble(gpu_ctx):
    worst = (0.0, None)
    for name, X in E.geometries().items():
        for fname, u in E.fields(X).items():
            for t in (E.G1, E.G2):
                ref, S = B.kg(E.LD, X, u, *E.REC_MATERIAL, t)
                got = B.untri(gpu_ctx.kg_hex8_batch(X, u, *E.REC_MATERIAL, np.full(X.shape[0], t, np.uint8)))
                un = E.units(got, ref, S)
                print("kg %-24s %-7s type %d: %.3f units" % (name, fname, t, un))
                if un > worst[0]:
                    worst = (un, (name, fname, t))
    print("element scalars: device %.3f units at %s; fp64 restatement %.2f; bound %.2f" %
          (worst[0], worst[1], B.KG_F64_UNITS_MEASURED, B.DEVICE_KG_UNITS))
    assert worst[0] <= B.DEVICE_KG_UNITS, worst


def test_element_scalars_zero_field_scaling_and_errors(gpu_ctx):
    from stan_amd import hip
    X = E.geometries()["plain"]
    u = E.fields(X)["random"]
    t = np.full(X.shape[0], E.G2, np.uint8)
    s = gpu_ctx.kg_hex8_batch(X, u, 210000.0, 0.3, t)
    assert not gpu_ctx.kg_hex8_batch(X, np.zeros_like(u), 210000.0, 0.3, t).any()
    assert np.array_equal(_bits(gpu_ctx.kg_hex8_batch(X, 2.0 * u, 210000.0, 0.3, t)), _bits(2.0 * s))
    assert np.array_equal(_bits(gpu_ctx.kg_hex8_batch(X, u, 210000.0, 0.3, t)), _bits(s))
    # more than one workgroup and a ragged last wave: element e of a batch does not depend on its neighbours
    reps = 5
    big = gpu_ctx.kg_hex8_batch(np.tile(X, (reps, 1, 1))[:-3], np.tile(u, (reps, 1, 1))[:-3], 210000.0, 0.3, np.tile(t, reps)[:-3])
    assert np.array_equal(_bits(big), _bits(np.tile(s, (reps, 1))[:-3]))
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.kg_hex8_batch(X, u, 210000.0, 0.3, np.full(X.shape[0], 7, np.uint8))
    assert ei.value.code == hip.E_UNSUPPORTED
    flat = X.copy()
    flat[3, :, 2] = 0.0                      # element 3 squashed into a plane: det J == 0
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.kg_hex8_batch(flat, u, 210000.0, 0.3, t)
    assert ei.value.code == hip.E_DETJ and gpu_ctx.last_bad_element() == 3


# ---- 2. the assembled matrix --------------------------------------------------------------------------------------------------
def _expected_csr(ctx, j, disp, rowptr, col):
    return B.csr_values(j, B.gather_nodes(j, _device_scalars(ctx, j, disp)), rowptr, col)


@pytest.mark.parametrize("name", MODELS)
def test_g_is_the_ordered_sum_of_the_devices_element_scalars(gpu_ctx, models, name):
    m = models(name)
    j, K, G = m["job"], m["K"], m["G"]
    rowptr, col, val = G.to_csr(upper_only=False)
    r0, c0, v0 = m["csr0"]
    assert np.array_equal(rowptr, r0) and np.array_equal(col, c0)            # K's pattern, fixed DOFs dropped alike
    want = _expected_csr(gpu_ctx, j, m["disp"], rowptr, col)
    assert np.array_equal(_bits(val), _bits(want)), int((_bits(val) != _bits(want)).sum())
    Gd = MR.dense(rowptr, col, val)
    assert np.array_equal(_bits(Gd), _bits(Gd.T.copy()))                     # symmetric to the bit
    gi, ki = G.info(), K.info()
    assert gi["scaled"] == 0 and ki["scaled"] == 1
    assert {x: v for x, v in gi.items() if x not in ("scaled", "folded_slots_permille")} == \
        {x: v for x, v in ki.items() if x not in ("scaled", "folded_slots_permille")}
    # the same bits twice (here from a K that a solve has scaled; the fixture's G too), and K untouched by it
    G2 = K.geometric_stiffness(j.xyz, m["disp"], *_mesh_args(j)[1:])
    assert np.array_equal(_bits(G2.to_csr(upper_only=False)[2]), _bits(val))
    G2.free()
    # products on G against the dense product in longdouble
    x = np.random.default_rng(11).standard_normal(j.n_red)
    y = G.spmv(x)
    rows = np.repeat(np.arange(j.n_red), np.diff(rowptr))
    terms = val.astype(LD) * x.astype(LD)[col]
    yr, ys = np.zeros(j.n_red, dtype=LD), np.zeros(j.n_red, dtype=LD)
    np.add.at(yr, rows, terms)
    np.add.at(ys, rows, np.abs(terms))
    nnz_row = int(np.diff(rowptr).max())
    assert (np.abs(y.astype(LD) - yr) <= nnz_row * U53 * ys).all()


def test_g_on_a_fresh_k_under_sell_sigma_and_from_device_pointers(gpu_ctx, models):
    import torch
    from stan_amd import hip
    m = models("cube6j")
    j, disp = m["job"], m["disp"]
    val = m["G"].to_csr(upper_only=False)[2]
    # a fresh K (no solve has scaled it): the same G, and K's export, info and later solve bits are those of an untouched K
    K1 = gpu_ctx.assemble_hex8(*_mesh_args(j))
    info0, csr0 = K1.info(), K1.to_csr(upper_only=False)
    G1 = K1.geometric_stiffness(j.xyz, disp, *_mesh_args(j)[1:])
    assert np.array_equal(_bits(G1.to_csr(upper_only=False)[2]), _bits(val))
    assert K1.info() == info0 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(K1.to_csr(upper_only=False), csr0))
    U1, r1 = K1.cg_solve(j.F, 1e-12)
    assert np.array_equal(_bits(U1), _bits(m["U"]))                          # as the fixture's K solved, before any G
    # the device-pointer entry inside guards: same bits, inputs untouched
    dev = torch.device("cuda:0")
    mesh = DB.Mesh(j, dev, offset=1, disp=disp)
    torch.cuda.synchronize()
    G3 = K1.geometric_stiffness_dev(mesh.n_nodes, mesh.xyz.ptr, mesh.disp.ptr, mesh.node_dof.ptr, mesh.n_elem, mesh.conn.ptr,
                                    mesh.elem_mat.ptr, mesh.elem_type.ptr, mesh.mat_E_nu, mesh.n_dof, mesh.red.ptr)
    DB.check(mesh.inputs)
    assert np.array_equal(_bits(G3.to_csr(upper_only=False)[2]), _bits(val))
    # K afterwards (scaled by the solve above, G built twice more): the solve's bits again
    U2, r2 = K1.cg_solve(j.F, 1e-12)
    assert r2 == r1 and np.array_equal(_bits(U2), _bits(U1))
    for x in (G1, G3, K1):
        x.free()
    # another layout: rows sorted over windows of 32 slices
    ctx = hip.Context(0)
    try:
        ctx.set_option(hip.OPT_SELL_SIGMA, 32)
        Ks = ctx.assemble_hex8(*_mesh_args(j))
        assert Ks.info()["sell_sigma"] == 32
        Gs = Ks.geometric_stiffness(j.xyz, disp, *_mesh_args(j)[1:])
        rp, cl, vs = Gs.to_csr(upper_only=False)
        assert np.array_equal(rp, m["csr0"][0]) and np.array_equal(cl, m["csr0"][1]) and np.array_equal(_bits(vs), _bits(val))
        Gs.free()
        Ks.free()
    finally:
        ctx.close()


# ---- 3. the new block kernels -------------------------------------------------------------------------------------------------
BLOCK_N = (1, 63, 64, 65, 4097, 200003)
BLOCK_Q = (1, 2, 5, 8, 16, 17, 32)


@pytest.mark.parametrize("N", BLOCK_N)
def test_block_kernels_against_longdouble(gpu_ctx, N):
    for q in BLOCK_Q:
        rng = np.random.default_rng(1000 * q + N % 997)
        mk = lambda: rng.standard_normal((q, N)) * 10.0 ** rng.uniform(-3, 3, (q, N))       # noqa: E731
        Z, W, Y, D = mk(), mk(), mk(), 10.0 ** rng.uniform(-3, 3, N)
        Q = rng.standard_normal((q, q))
        mu = rng.standard_normal(q) * 10.0 ** rng.uniform(-2, 2, q)
        X, KX, R, r2, kx2 = gpu_ctx.buckling_rotate(Z, W, Y, D, Q, mu)
        Zl, Wl, Yl, Ql, mul, Dl = (a.astype(LD) for a in (Z, W, Y, Q, mu, D))
        aQ = np.abs(Ql)
        assert (np.abs(X.astype(LD) - Ql.T @ Zl) <= q * U53 * (aQ.T @ np.abs(Zl))).all(), (N, q)
        assert (np.abs(KX.astype(LD) - Ql.T @ Wl) <= q * U53 * (aQ.T @ np.abs(Wl))).all(), (N, q)
        Rr = mul[:, None] * (Ql.T @ Wl) - Ql.T @ Yl
        Rs = np.abs(mul)[:, None] * (aQ.T @ np.abs(Wl)) + aQ.T @ np.abs(Yl)
        assert (np.abs(R.astype(LD) - Rr) <= (2 * q + 1) * U53 * Rs).all(), (N, q)
        # the sums from the device's own R and KX: a term costs three roundings, the sum at most N more
        for got, V in ((r2, R), (kx2, KX)):
            want = (V.astype(LD) ** 2 / Dl[None, :]).sum(axis=1)
            assert (np.abs(got.astype(LD) - want) <= (N + 4) * U53 * want).all(), (N, q)
        again = gpu_ctx.buckling_rotate(Z, W, Y, D, Q, mu)
        for a, b in zip((X, KX, R, r2, kx2), again):
            assert np.array_equal(_bits(a), _bits(b)), (N, q)


# ---- 4. the factors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_factors_against_the_dense_eigen_solve(gpu_ctx, models, name):
    m = models(name)
    K, G, Kd, Hd, mu_ref, k, rest, TOL = m["K"], m["G"], m["Kd"], m["Hd"], m["mu_ref"], m["k"], m["rest"], m["tol"]
    N = Kd.shape[0]
    assert k >= 1 and (mu_ref[:k] > 0).all() and (mu_ref[k - 1] - mu_ref[k]) / mu_ref[k - 1] > 1e-3
    assert rest["converged"] and rest["outer"] <= 150
    gbits = _bits(G.to_csr(upper_only=False)[2])
    fac, phi, rho, rep = gpu_ctx.buckling(K, G, k, tol=TOL, max_outer=300)
    print(name, "N", N, "k", k, "restatement outer", rest["outer"], rep, "factors", fac, "rho", rho)
    assert rep["converged"] == 1 and rep["block"] == MR.block_size(N, k) and rep["cg_worst_type"] > 0
    assert rep["outer"] <= rest["outer"] + 3 and rep["n_positive"] >= k
    assert (rho <= TOL).all() and rep["max_rho"] == rho.max()
    assert (np.diff(fac) >= 0).all() and (fac > 0).all()
    mu = 1.0 / fac
    assert (B.rho_host(Kd, Hd, mu, phi) <= 2 * TOL).all()
    bound, rn = B.residual_bound(Kd, Hd, mu, phi)
    assert (np.abs(mu - mu_ref[:k]) <= bound + 8 * U53 * np.abs(mu_ref[:k])).all(), (mu, mu_ref[:k], bound)
    for a, b, gap in B.clusters(mu_ref, k):
        s = B.sin_max_angle_K(phi[a:b].T, m["Phi"][:, a:b], Kd)
        print("  cluster", a, b, "sin %.3e bound %.3e" % (s, 2 * rn[a:b].max() / gap))
        assert s <= 2 * rn[a:b].max() / gap, (a, b, s)
    for x in phi:                                       # the entry of largest magnitude is exactly 1, at the lowest index
        i = int(np.argmax(np.abs(x)))
        assert x[i] == 1.0 and np.abs(x).max() == 1.0
    if rep["lowest_negative_factor"] != 0.0:            # the extreme of the other end of the spectrum, not converged on purpose
        assert rep["lowest_negative_factor"] < 0.0 and 1.0 / rep["lowest_negative_factor"] >= m["low"] * (1 + 1e-9)
    assert np.array_equal(_bits(G.to_csr(upper_only=False)[2]), gbits)       # G is unchanged to the bit


def test_same_bits_twice_from_device_pointers_and_k_afterwards(gpu_ctx, models):
    import torch
    m = models("column20")
    j, K, G, k, TOL = m["job"], m["K"], m["G"], m["k"], m["tol"]
    N = j.n_red
    first = gpu_ctx.buckling(K, G, k, tol=TOL, max_outer=300)
    again = gpu_ctx.buckling(K, G, k, tol=TOL, max_outer=300)
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    strip = lambda r: {x: v for x, v in r.items() if not x.endswith("_ms")}       # noqa: E731
    assert strip(first[3]) == strip(again[3])
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    outs = [DB.output("factor", k, g, dev, 1), DB.output("phi", k * N, g, dev, 3), DB.output("rho", k, g, dev, 5)]
    torch.cuda.synchronize()
    rep = gpu_ctx.buckling_dev(K, G, k, outs[0].ptr, outs[1].ptr, outs[2].ptr, tol=TOL, max_outer=300)
    DB.check(outs)
    assert strip(rep) == strip(first[3])
    for a, o in zip(first[:3], outs):
        assert np.array_equal(_bits(a.reshape(-1)), _bits(o.numpy())), o.name
    # the caller's merit-stop setting comes back; K afterwards solves with the bits of a fresh assembly
    U, r = K.cg_solve(j.F, 1e-10)
    K2 = gpu_ctx.assemble_hex8(*_mesh_args(j))
    U2, r2 = K2.cg_solve(j.F, 1e-10)
    K2.free()
    assert r == r2 and np.array_equal(_bits(U), _bits(U2))
    # one outer step: honest residuals, converged = 0
    f1, p1, rho1, rep1 = gpu_ctx.buckling(K, G, k, tol=TOL, max_outer=1)
    assert rep1["outer"] == 1 and rep1["converged"] == 0 and (rho1 > TOL).any()
    host = B.rho_host(m["Kd"], m["Hd"], 1.0 / f1, p1)
    assert (rho1 <= 2 * host).all() and (host <= 2 * rho1).all(), (rho1, host)


# ---- 5. error cases -----------------------------------------------------------------------------------------------------------
def test_error_cases(gpu_ctx, models):
    from stan_amd import hip
    m, other = models("cube6"), models("column20")
    j, K, G = m["job"], m["K"], m["G"]
    N = j.n_red

    def code(call):
        with pytest.raises(hip.StanHipError) as ei:
            call()
        return ei.value.code

    assert code(lambda: gpu_ctx.buckling(K, other["G"], 2)) == hip.E_ARG              # a G of another layout
    assert code(lambda: gpu_ctx.buckling(K, G, N + 1)) == hip.E_ARG
    assert code(lambda: gpu_ctx.buckling(K, G, 0)) == hip.E_ARG
    assert code(lambda: gpu_ctx.buckling(K, G, 25)) == hip.E_ARG                      # a block of 33 columns
    assert code(lambda: gpu_ctx.buckling(K, G, 2, tol=-1.0)) == hip.E_ARG
    assert code(lambda: gpu_ctx.buckling_dev(K, G, 2, None, None, None)) == hip.E_ARG
    # a mesh that is not K's
    oj = other["job"]
    assert code(lambda: K.geometric_stiffness(oj.xyz, other["disp"], *_mesh_args(oj)[1:])) == hip.E_ARG
    bad = j.conn.copy()
    bad[5, 2] = j.xyz.shape[0]
    assert code(lambda: K.geometric_stiffness(j.xyz, m["disp"], j.node_dof, bad, *_mesh_args(j)[3:])) == hip.E_ARG
    far = j.conn.copy()
    far[0, 6] = j.conn[-1, 6]                # in range (det J != 0: a stretched corner), but a coupling K's pattern does not have
    assert code(lambda: K.geometric_stiffness(j.xyz, m["disp"], j.node_dof, far, *_mesh_args(j)[3:])) == hip.E_ARG
    # a free-free model: K is not positive definite
    from tests import transient_ref as T
    fj = T.job(T.FREE)
    Kf = gpu_ctx.assemble_hex8(*_mesh_args(fj))
    Gf = Kf.geometric_stiffness(fj.xyz, np.random.default_rng(2).standard_normal(fj.xyz.shape) * 1e-3, *_mesh_args(fj)[1:])
    assert code(lambda: gpu_ctx.buckling(Kf, Gf, 2, max_outer=5)) == hip.E_UNSUPPORTED
    Gf.free()
    Kf.free()
    # a multi-device handle
    multi = hip.Context(devices=[0])
    try:
        Km = multi.assemble_hex8(*_mesh_args(j))
        assert code(lambda: Km.geometric_stiffness(j.xyz, m["disp"], *_mesh_args(j)[1:])) == hip.E_UNSUPPORTED
        assert code(lambda: multi.buckling(Km, Km, 2)) == hip.E_UNSUPPORTED
        Km.free()
    finally:
        multi.close()
    # the model still answers after all of it
    fac = gpu_ctx.buckling(K, G, 1, tol=m["tol"], max_outer=300)[0]
    assert abs(1.0 / fac[0] - m["mu_ref"][0]) <= 2 * m["tol"] * m["mu_ref"][0]


# ---- 6. console ---------------------------------------------------------------------------------------------------------------
def _console_db(path, supports=True, temperature=False, nz=10):
    """The clamped 2 x 2 x nz column under an end load (B.column_job's mesh), as an STdb"""
    from stan_amd import host
    xyz, conn = B.box_mesh(2, 2, nz)
    xyz = xyz * [0.5, 0.5, B.COLUMN_L / nz]
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", B.COLUMN_E, 0.0)
    d.assign_part(1, 1, "HEX8_G2")
    fixed = np.nonzero(xyz[:, 2] == 0.0)[0]
    top = np.nonzero(xyz[:, 2] == xyz[:, 2].max())[0]
    if supports:
        d.add_bc(1, "fix", "SPC", fixed + 1, np.ones((fixed.size, 3)))
    loads = np.zeros((top.size, 3))
    loads[:, 2] = -np.where(xyz[top, 0] == 0.5, 0.5, 0.25) * np.where(xyz[top, 1] == 0.5, 0.5, 0.25)
    d.add_bc(2, "load", "PointLoad", top + 1, loads)
    if temperature:
        d.add_bc(3, "heat", "Temperature", top + 1, np.tile([10.0, 0.0, 0.0], (top.size, 1)))
    d.set_analysis(tol=1e-12)
    d.assign_dof()
    d.write_stdb(path)
    return xyz.shape[0]


def test_console_buckling(tmp_path, built_libs):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "c.STdb"), str(tmp_path / "out")
    n_nodes = _console_db(path)
    before = open(path, "rb").read()
    out = subprocess.run([exe, "--buckling", "4", "--json", "--vtu", prefix, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    assert "Buckling load factors:" in out.stdout
    b = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["buckling"]
    assert set(b) >= {"n_modes", "block", "outer", "converged", "n_positive", "cg_iterations", "lowest_negative_factor", "factor", "rho"}
    assert b["n_modes"] == 4 and b["block"] == 8 and b["converged"] == 1 and len(b["factor"]) == 4 and b["n_positive"] >= 4
    fac = np.array(b["factor"])
    assert (np.diff(fac) >= 0).all() and (np.array(b["rho"]) <= 1e-6).all()
    # the column of tests/test_buckling.py: its lowest factor is 1.4939 x Euler's load (a unit end load), twice (two bending planes)
    assert abs(fac[0] / B.euler_load() - 1.4939) <= 1e-3 and abs(fac[1] / fac[0] - 1) <= 1e-5
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Buckling load factors:")[1], flags=re.M)[:4]
    assert [int(r[0]) for r in rows] == [1, 2, 3, 4] and np.allclose([float(r[1]) for r in rows], fac, rtol=1e-8)
    for k in range(1, 5):
        text = open("%s_buckle_%03d.vtu" % (prefix, k), "rb").read()
        for name in ("Buckling Shape X", "Buckling Shape Y", "Buckling Shape Z", "Magnitude"):
            assert ('Name="%s"' % name).encode() in text, (k, name)
        assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    assert not os.path.exists("%s_buckle_005.vtu" % prefix) and not os.path.exists(prefix + "_001.vtu")
    # --solve-eps and --buckling-tol are taken: a looser run needs no more outer steps
    out = subprocess.run([exe, "--buckling", "2", "--buckling-tol", "1e-4", "--solve-eps", "1e-8", "--json", path],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    b2 = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["buckling"]
    assert b2["converged"] == 1 and b2["outer"] <= b["outer"] and abs(b2["factor"][0] / fac[0] - 1) <= 1e-4
    # the refusals, each before anything is computed; the file is untouched
    out = subprocess.run([exe, "--buckling", "4", "--devices", "0,0", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "one device" in out.stderr
    out = subprocess.run([exe, "--buckling", "0", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2
    hot = str(tmp_path / "hot.STdb")
    _console_db(hot, temperature=True)
    kept = open(hot, "rb").read()
    out = subprocess.run([exe, "--buckling", "4", hot], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "Temperature" in out.stderr and open(hot, "rb").read() == kept
    free = str(tmp_path / "free.STdb")
    _console_db(free, supports=False)
    kept = open(free, "rb").read()
    out = subprocess.run([exe, "--buckling", "4", free], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "support" in out.stderr and open(free, "rb").read() == kept
    assert open(path, "rb").read() == before
