"""The consistent mass on the device: the element scalars against np.longdouble, the assembled M_c bit
for bit against the ordered sum of the device's own element scalars, A + sigma B bit for bit against the fused multiply-add of the
two exports, stan_hip_modes_pencil against scipy's eigh of the exported matrices, reproducibility, what the calls leave of their
inputs, and the error cases (tests/mass_ref.py).

Bounds.  Element scalars: 4 x what the plain-fp64 restatement reads over the conditioning family in units of each entry's
rounding scale (M.DEVICE_MASS_UNITS = 4 x 2.78 = 11.12; the yardstick is the restatement, never the device).  Measured on the first
GPU run: the device reads 2.926 units at worst (on "aspect_rot"; at most 0.51 outside the two stretched and rotated groups),
the restatement 2.771 (on "aspect_rot_shift_union").  Row sums and the rigid
translation: see K_ROWSUM and K_TOTAL below.  Eigenvalues: the residual bound of tests/test_gpu_buckling.py."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import buckling_ref as B
from tests import device_buffers as DB
from tests import element_ref as E
from tests import mass_ref as M
from tests import modes_ref as MR
from tests import transient_ref as T

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
MATRIX_MODELS = MR.MODELS + ("column20", "cube2")        # cube2: 27 block rows, one partial slice
TOL = 1e-6
FREE_K = 8                                               # tests/test_mass.py: the shifted free cube, 23 outer steps at k = 8
FREE_OUTER = 23
# Row sum of to_csr(M_c) (added here in long double: no rounding of its own) against the lumped M of the same DOF, both from the
# same t_g = fl(N_a det J_g) (one inlined routine on one record in both kernels).  All terms are positive, so every rounding moves
# the sum by at most 2^-53 of it:
#   consistent: N_b 5 (three factors 1 + s p, two products; sum_b N_b = 1 holds for any p, so the rounded sqrt(1/3) is no error
#               here), the term t_g N_b 1, the butterfly over 8 points 3, the factor rho 1, the gather's 7 additions   = 17
#   lumped:     the butterfly 3, the factor rho 1, the node gather's 7 additions                                        = 11
K_ROWSUM = 28
# x^T M_c x of a unit translation = the sum of those row sums (exact here) against total_mass of stan_mass_sums, which adds the
# n_nodes node masses in some fixed order: at most n_nodes - 1 more roundings
K_TOTAL = lambda n_nodes: K_ROWSUM + n_nodes - 1      # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _job(name):
    from stan_amd import problem
    if name == "column20":
        return B.column_job(20)
    if name == "cube2":
        return problem.cube_job(2, jitter=0.1)
    if name == T.FREE:
        return T.job(T.FREE)
    return MR.job(name)


def _rho(name):
    return MR.mat_rho(name) if name in MR.MODELS else np.array([MR.RHO])


def _mesh_args(j):
    return (j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


def _mass(K, j, rho):
    return K.consistent_mass(*_mesh_args(j), rho)


def _device_scalars(ctx, j, rho):
    """m [n_elem, 8, 8] from stan_hip_mass_hex8_batch, material by material"""
    X = j.xyz[j.conn]
    m36 = np.zeros((j.conn.shape[0], 36))
    for mat, r in enumerate(np.asarray(rho)):
        sel = np.nonzero(np.asarray(j.elem_mat) == mat)[0]
        if sel.size:
            m36[sel] = ctx.mass_hex8_batch(X[sel], r)
    return B.untri(m36)


def _expected_csr(ctx, j, rho, rowptr, col):
    return B.csr_values(j, B.gather_nodes(j, _device_scalars(ctx, j, rho)), rowptr, col)


def _code(call):
    from stan_amd import hip
    with pytest.raises(hip.StanHipError) as ei:
        call()
    return ei.value.code


def _load(j, N):
    F = np.asarray(j.F, dtype=np.float64)
    return F if np.abs(F).max() > 0 else np.random.default_rng(3).standard_normal(N)


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, rho, K (scaled by a solve), csr0 (the export of the fresh K), U, Mc, mval): once, left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            j, rho = _job(name), _rho(name)
            K = gpu_ctx.assemble_hex8(*_mesh_args(j))
            csr0 = K.to_csr(upper_only=False)
            F = _load(j, j.n_red)
            if name == T.FREE:
                K.cg_solve(F, 1e-8, max_its=50)          # singular: the solve only has to leave S K S in place
                U = None
            else:
                U, rep = K.cg_solve(F, 1e-12)
                assert rep["terminationtype"] in (1, 7)
            assert K.info()["scaled"] == 1
            Mc = _mass(K, j, rho)
            made[name] = dict(job=j, rho=rho, K=K, csr0=csr0, F=F, U=U, Mc=Mc, mval=Mc.to_csr(upper_only=False)[2])
        return made[name]

    yield get
    for m in made.values():
        m["Mc"].free()
        m["K"].free()


# ---- 1. the element scalars ---------------------------------------------------------------------------------------------------
def test_element_scalars_against_longdouble(gpu_ctx):
    worst = (0.0, None)
    for name, X in E.geometries().items():
        ref, S = M.mass(E.LD, X, MR.RHO)
        got = B.untri(gpu_ctx.mass_hex8_batch(X, MR.RHO))
        un = E.units(got, ref, S)
        print("mass %-24s %.3f units" % (name, un))
        if un > worst[0]:
            worst = (un, name)
    print("element scalars: device %.3f units at %s; fp64 restatement %.2f; bound %.2f" %
          (worst[0], worst[1], M.MASS_F64_UNITS_MEASURED, M.DEVICE_MASS_UNITS))
    assert worst[0] <= M.DEVICE_MASS_UNITS, worst


@pytest.mark.parametrize("n", (1, 7, 8, 9, 33))
def test_element_scalars_batch_tails(gpu_ctx, n):
    """8 elements per wave, 32 per workgroup: an element of a batch does not depend on its neighbours or on its place."""
    fam = E.geometries()
    X = np.concatenate([fam["plain"], fam["aspect_rot"], fam["thin_1e-4"]])[:n]
    assert X.shape[0] == n
    got = gpu_ctx.mass_hex8_batch(X, MR.RHO)
    assert got.shape == (n, 36) and np.array_equal(_bits(got), _bits(gpu_ctx.mass_hex8_batch(X, MR.RHO)))      # the same bits twice
    for e in (0, n // 2, n - 1):
        assert np.array_equal(_bits(got[e]), _bits(gpu_ctx.mass_hex8_batch(X[e:e + 1], MR.RHO)[0])), e
    assert np.array_equal(_bits(gpu_ctx.mass_hex8_batch(X[::-1].copy(), MR.RHO)[::-1]), _bits(got))
    ref, S = M.mass(E.LD, X, MR.RHO)
    assert E.units(B.untri(got), ref, S) <= M.DEVICE_MASS_UNITS


def test_element_scalars_properties_and_errors(gpu_ctx):
    from stan_amd import hip
    X = E.geometries()["plain"]
    m = gpu_ctx.mass_hex8_batch(X, 1.0)
    assert (m > 0).all()
    assert np.array_equal(_bits(gpu_ctx.mass_hex8_batch(X, 4.0)), _bits(4.0 * m))            # rho multiplies the finished sum
    unit = B.untri(gpu_ctx.mass_hex8_batch(E.geometries()["unit_cube"], 1.0))[0]
    assert np.abs(unit - M.unit_cube()).max() <= 8 * U53 * M.unit_cube().max()
    for rho in (0.0, -1.0, float("nan"), float("inf")):
        assert _code(lambda: gpu_ctx.mass_hex8_batch(X, rho)) == hip.E_ARG, rho
    flat = X.copy()
    flat[3, :, 2] = 0.0                      # element 3 squashed into a plane: det J == 0
    assert _code(lambda: gpu_ctx.mass_hex8_batch(flat, 1.0)) == hip.E_DETJ and gpu_ctx.last_bad_element() == 3


# ---- 2. the assembled matrix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRIX_MODELS)
def test_mc_is_the_ordered_sum_of_the_devices_element_scalars(gpu_ctx, models, name):
    m = models(name)
    j, K, Mc, rho = m["job"], m["K"], m["Mc"], m["rho"]
    rowptr, col, val = Mc.to_csr(upper_only=False)
    r0, c0, _v0 = m["csr0"]
    assert np.array_equal(rowptr, r0) and np.array_equal(col, c0)            # K's pattern, fixed DOFs dropped alike
    want = _expected_csr(gpu_ctx, j, rho, rowptr, col)
    assert np.array_equal(_bits(val), _bits(want)), int((_bits(val) != _bits(want)).sum())
    Md = MR.dense(rowptr, col, val)
    assert np.array_equal(_bits(Md), _bits(Md.T.copy()))                     # symmetric to the bit
    mi, ki = Mc.info(), K.info()
    assert mi["scaled"] == 0 and ki["scaled"] == 1                           # built from a K a solve has scaled
    assert {x: v for x, v in mi.items() if x not in ("scaled", "folded_slots_permille")} == \
        {x: v for x, v in ki.items() if x not in ("scaled", "folded_slots_permille")}
    M2 = _mass(K, j, rho)                                                    # the same bits twice
    assert np.array_equal(_bits(M2.to_csr(upper_only=False)[2]), _bits(val))
    M2.free()
    # the element's type does not enter: the 2 x 2 x 2 rule for both
    other = np.where(np.arange(j.conn.shape[0]) % 2 == 0, E.G1, E.G2).astype(np.uint8)
    M3 = K.consistent_mass(j.xyz, j.node_dof, j.conn, j.elem_mat, other, j.mat_E_nu, j.red, rho)
    assert np.array_equal(_bits(M3.to_csr(upper_only=False)[2]), _bits(val))
    M3.free()
    assert np.linalg.eigvalsh(Md)[0] > 0 if Md.shape[0] <= 1000 else True    # positive definite


def test_mc_on_a_fresh_k_under_sell_sigma_and_from_device_pointers(gpu_ctx, models):
    import torch
    from stan_amd import hip
    m = models("cube6j")
    j, rho, val = m["job"], m["rho"], m["mval"]
    # a fresh K (no solve has scaled it): the same M_c, and K's export, info and later solve bits are those of an untouched K
    K1 = gpu_ctx.assemble_hex8(*_mesh_args(j))
    info0, csr0 = K1.info(), K1.to_csr(upper_only=False)
    M1 = _mass(K1, j, rho)
    assert np.array_equal(_bits(M1.to_csr(upper_only=False)[2]), _bits(val))
    assert K1.info() == info0 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(K1.to_csr(upper_only=False), csr0))
    U1, r1 = K1.cg_solve(j.F, 1e-12)
    assert np.array_equal(_bits(U1), _bits(m["U"]))                          # as the fixture's K solved, before any M_c
    # the device-pointer entry inside guards: same bits, inputs untouched
    dev = torch.device("cuda:0")
    mesh = DB.Mesh(j, dev, offset=1)
    torch.cuda.synchronize()
    M3 = K1.consistent_mass_dev(mesh.n_nodes, mesh.xyz.ptr, rho, mesh.node_dof.ptr, mesh.n_elem, mesh.conn.ptr, mesh.elem_mat.ptr,
                                mesh.elem_type.ptr, mesh.mat_E_nu, mesh.n_dof, mesh.red.ptr)
    DB.check(mesh.inputs)
    assert np.array_equal(_bits(M3.to_csr(upper_only=False)[2]), _bits(val))
    U2, r2 = K1.cg_solve(j.F, 1e-12)                                         # K afterwards: the solve's bits again
    assert r2 == r1 and np.array_equal(_bits(U2), _bits(U1))
    for x in (M1, M3, K1):
        x.free()
    ctx = hip.Context(0)                                                     # another layout: rows sorted over windows of 32 slices
    try:
        ctx.set_option(hip.OPT_SELL_SIGMA, 32)
        Ks = ctx.assemble_hex8(*_mesh_args(j))
        assert Ks.info()["sell_sigma"] == 32
        Ms = _mass(Ks, j, rho)
        rp, cl, vs = Ms.to_csr(upper_only=False)
        assert np.array_equal(rp, m["csr0"][0]) and np.array_equal(cl, m["csr0"][1]) and np.array_equal(_bits(vs), _bits(val))
        Ms.free()
        Ks.free()
    finally:
        ctx.close()


def test_row_sums_are_the_lumped_mass_and_a_translation_weighs_the_model(gpu_ctx, models):
    m = models(T.FREE)
    j, rho = m["job"], m["rho"]
    assert j.n_red == j.n_dof                                                # no fixed DOFs
    rowptr, col, val = m["Mc"].to_csr(upper_only=False)
    lumped, _mn, sums = gpu_ctx.lumped_mass_hex8(*_mesh_args(j), rho)
    rows = np.repeat(np.arange(j.n_red), np.diff(rowptr))
    assert (val >= 0).all()
    rs = np.zeros(j.n_red, dtype=LD)
    np.add.at(rs, rows, val.astype(LD))
    err = np.abs(rs - lumped.astype(LD)) / (U53 * rs)
    print("row sums against the lumped mass: worst %.2f x 2^-53 of the row sum (bound %d)" % (float(err.max()), K_ROWSUM))
    assert (err <= K_ROWSUM).all()
    # a rigid translation along each axis: the component's rows (the other components of a block are zeros)
    node, comp = B._reduced_maps(j)
    for c in range(3):
        x = (comp == c).astype(np.float64)
        xMx = (val.astype(LD) * x.astype(LD)[rows] * x.astype(LD)[col]).sum()
        e = abs(xMx - LD(sums.total_mass)) / (U53 * xMx)
        print("translation %d: x^T M_c x = %.17g, total mass %.17g, %.2f x 2^-53 (bound %d)" %
              (c, float(xMx), sums.total_mass, float(e), K_TOTAL(j.xyz.shape[0])))
        assert e <= K_TOTAL(j.xyz.shape[0])
        y = m["Mc"].spmv(x)                                                  # and the product agrees with the export
        assert abs(float((y.astype(LD) * x.astype(LD)).sum()) - float(xMx)) <= 64 * U53 * float(xMx)


def test_matrix_error_cases(gpu_ctx, models):
    from stan_amd import hip
    m, other = models("cube6"), models("column20")
    j, K, rho = m["job"], m["K"], m["rho"]
    oj = other["job"]
    assert _code(lambda: _mass(K, oj, other["rho"])) == hip.E_ARG                                      # a mesh that is not K's
    far = j.conn.copy()
    far[0, 6] = j.conn[-1, 6]                # the same node count, a coupling K's pattern does not have
    assert _code(lambda: K.consistent_mass(j.xyz, j.node_dof, far, *_mesh_args(j)[3:], rho)) == hip.E_ARG
    bad = j.conn.copy()
    bad[5, 2] = j.xyz.shape[0]
    assert _code(lambda: K.consistent_mass(j.xyz, j.node_dof, bad, *_mesh_args(j)[3:], rho)) == hip.E_ARG
    for r in ([0.0], [-1.0], [float("nan")]):
        assert _code(lambda: _mass(K, j, np.array(r))) == hip.E_ARG, r
    # a material no element uses is not looked at; one an element uses is
    two = np.array([[210000.0, 0.3], [1.0, 0.0]])
    M2 = K.consistent_mass(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, two, j.red, np.array([MR.RHO, 0.0]))
    assert np.array_equal(_bits(M2.to_csr(upper_only=False)[2]), _bits(m["mval"]))
    M2.free()
    used = j.elem_mat.copy()
    used[7] = 1
    assert _code(lambda: K.consistent_mass(j.xyz, j.node_dof, j.conn, used, j.elem_type, two, j.red, np.array([MR.RHO, 0.0]))) == hip.E_ARG
    assert "element 7" in gpu_ctx.lib.stan_hip_last_error(gpu_ctx.h).decode()
    # a K of another context; NULL pointers; on an error *out is not written
    ctx2 = hip.Context(0)
    try:
        K2 = ctx2.assemble_hex8(*_mesh_args(j))
        k = C.c_void_p(0x5EED)
        args = hip._mesh(xyz=j.xyz, node_dof=j.node_dof, conn=j.conn, elem_mat=j.elem_mat, elem_type=j.elem_type, mat_E_nu=j.mat_E_nu,
                         red=j.red)
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = args
        rh = np.ascontiguousarray(rho, dtype=np.float64)

        def raw(ctx, Kh, rho_ptr, out):
            return ctx.lib.stan_hip_consistent_mass_hex8(
                ctx.h, Kh, C.c_int64(xyz.shape[0]), hip._ptr(xyz, C.c_double), rho_ptr, hip._ptr(node_dof, C.c_int32),
                C.c_int64(conn.shape[0]), hip._ptr(conn, C.c_int32), hip._ptr(elem_mat, C.c_int32), hip._ptr(elem_type, C.c_uint8),
                C.c_int32(mat_E_nu.shape[0]), hip._ptr(mat_E_nu, C.c_double), C.c_int64(red.shape[0]), hip._ptr(red, C.c_int32), out)
        assert raw(gpu_ctx, K2.k, hip._ptr(rh, C.c_double), C.byref(k)) == hip.E_ARG and k.value == 0x5EED     # another context's K
        assert raw(gpu_ctx, K.k, None, C.byref(k)) == hip.E_ARG and k.value == 0x5EED                          # NULL mat_rho
        assert raw(gpu_ctx, None, hip._ptr(rh, C.c_double), C.byref(k)) == hip.E_ARG and k.value == 0x5EED     # NULL K
        assert raw(gpu_ctx, K.k, hip._ptr(rh, C.c_double), None) == hip.E_ARG                                  # NULL out
        zero = np.zeros_like(rh)
        assert raw(gpu_ctx, K.k, hip._ptr(zero, C.c_double), C.byref(k)) == hip.E_ARG and k.value == 0x5EED
        K2.free()
    finally:
        ctx2.close()
    multi = hip.Context(devices=[0])
    try:
        Km = multi.assemble_hex8(*_mesh_args(j))
        assert _code(lambda: _mass(Km, j, rho)) == hip.E_UNSUPPORTED
        assert _code(lambda: Km.axpy(1.0, Km)) == hip.E_UNSUPPORTED
        assert _code(lambda: multi.modes_pencil(Km, Km, 2)) == hip.E_UNSUPPORTED
        Km.free()
    finally:
        multi.close()


# ---- 3. A + sigma B -----------------------------------------------------------------------------------------------------------
def _split(v):
    """float64 array -> (integer mantissas [python ints], exponents): v = m 2^e exactly"""
    mant, ex = np.frexp(np.asarray(v, dtype=np.float64))
    return [int(x) for x in (mant * 2.0 ** 53).astype(np.int64)], [int(x) - 53 for x in ex]


def _fma(sigma, b, a):
    """fl(sigma b + a) entry by entry with one rounding: exact integers, rounded once by float() (round to nearest even)."""
    (ms,), (es,) = _split([sigma])
    mb, eb = _split(b)
    ma, ea = _split(a)
    out = np.empty(len(ma))
    for i in range(len(ma)):
        ep = es + eb[i]
        lo = min(ep, ea[i])
        out[i] = math.ldexp(float(((ms * mb[i]) << (ep - lo)) + (ma[i] << (ea[i] - lo))), lo)
    return out


def _same(got, want):
    """bit for bit; a zero result compares by value (the sign of an exact zero sum is fma's)"""
    return bool(np.array_equal(got == 0.0, want == 0.0) and np.array_equal(_bits(got[want != 0.0]), _bits(want[want != 0.0])))


def test_fma_helper():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(2000) * 10.0 ** rng.uniform(-8, 8, 2000), rng.standard_normal(2000) * 10.0 ** rng.uniform(-8, 8, 2000)
    got = _fma(3.0, b, a)
    want = (3 * b.astype(LD) + a.astype(LD)).astype(np.float64)      # 3 b is exact in 64 bits; double rounding is rare but real
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all() and (got == want).mean() > 0.99
    assert _fma(0.0, b, a).tolist() == a.tolist() and _fma(2.0 ** -30, a, -2.0 ** -30 * a).tolist() == [0.0] * 2000


def _g_for(m, K):
    j = m["job"]
    return K.geometric_stiffness(j.xyz, B.disp_full(j, m["U"]), *_mesh_args(j)[1:])


def _check_axpy(ctx, m, pair, a_scaled, b_scaled, options=()):
    from stan_amd import hip
    assert pair == "mass" or not b_scaled
    j, rho, F = m["job"], m["rho"], m["F"]
    for opt, val in options:
        ctx.set_option(opt, val)
    made = []
    try:
        A = ctx.assemble_hex8(*_mesh_args(j))
        made.append(A)
        Bm = _mass(A, j, rho) if pair == "mass" else _g_for(m, A)
        made.append(Bm)
        ea, eb = A.to_csr(upper_only=False), Bm.to_csr(upper_only=False)
        if b_scaled:                                   # a solve on M_c first
            Bm.cg_solve(F, 1e-8, max_its=200)
            assert Bm.info()["scaled"] == 1
        if a_scaled:
            A.cg_solve(F, 1e-8)
            assert A.info()["scaled"] == 1
        # the exports after scaling are what the kernel's a and b are
        xa, xb = A.to_csr(upper_only=False), Bm.to_csr(upper_only=False)
        assert np.array_equal(xa[1], xb[1]) and np.array_equal(xa[0], ea[0])
        ia, ib = A.info(), Bm.info()
        lam1 = float(np.abs(ea[2]).max() / np.abs(eb[2]).max())
        for sigma in (0.0, T.coef(1e-4)["a0"] if pair == "mass" else 0.37 * lam1, -0.25 * lam1):
            S = A.axpy(sigma, Bm)
            made.append(S)
            got = S.to_csr(upper_only=False)
            assert np.array_equal(got[0], xa[0]) and np.array_equal(got[1], xa[1])
            want = _fma(sigma, xb[2], xa[2])
            assert _same(got[2], want), (pair, a_scaled, b_scaled, sigma, int((got[2] != want).sum()))
            if sigma == 0.0:
                assert np.array_equal(got[2], xa[2])
            si = S.info()
            assert si["scaled"] == 0 and {k: v for k, v in si.items() if k not in ("scaled", "folded_slots_permille")} == \
                {k: v for k, v in ia.items() if k not in ("scaled", "folded_slots_permille")}
            S2 = A.axpy(sigma, Bm)                         # the same bits twice
            assert np.array_equal(_bits(S2.to_csr(upper_only=False)[2]), _bits(got[2]))
            S2.free()
            # A and B are unchanged to the bit
            assert A.info() == ia and Bm.info() == ib
            assert np.array_equal(_bits(A.to_csr(upper_only=False)[2]), _bits(xa[2]))
            assert np.array_equal(_bits(Bm.to_csr(upper_only=False)[2]), _bits(xb[2]))
            made.pop().free()
    finally:
        for x in made[::-1]:
            x.free()
        for opt, _val in options:
            ctx.set_option(opt, {hip.OPT_SELL_SIGMA: 1, hip.OPT_ROW_FOLDING: -1}[opt])


# (G is indefinite: no solve scales it; M_c is positive definite and one case solves on it first)
@pytest.mark.parametrize("pair,a_scaled,b_scaled", (("mass", False, False), ("mass", True, False), ("mass", False, True), ("mass", True, True),
                                                    ("geometric", False, False), ("geometric", True, False)))
def test_axpy_is_the_fma_of_the_two_exports(gpu_ctx, models, pair, a_scaled, b_scaled):
    _check_axpy(gpu_ctx, models("cube6j"), pair, a_scaled, b_scaled)


def test_axpy_under_sell_sigma_and_row_folding(gpu_ctx, models):
    from stan_amd import hip
    ctx = hip.Context(0)
    try:
        _check_axpy(ctx, models("cube6j"), "mass", True, True, options=((hip.OPT_SELL_SIGMA, 32), (hip.OPT_ROW_FOLDING, 1)))
        _check_axpy(ctx, models("two_mat"), "geometric", True, False, options=((hip.OPT_ROW_FOLDING, 1),))
    finally:
        ctx.close()


def _scaled_residual(csr, b, x):
    """||S (b - A x)|| / ||S b|| in long double, S = diag(A)^-1/2, A the exported matrix (tests/test_gpu_transient.py's form)"""
    rowptr, col, val = csr
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    s = 1.0 / np.sqrt(val[rows == col].astype(LD))
    r = s * (np.asarray(b, dtype=LD) - T.csr_ld(rowptr, col, val)(x))
    return float(np.sqrt((r * r).sum()) / np.sqrt(((s * np.asarray(b, dtype=LD)) ** 2).sum()))


@pytest.mark.parametrize("name", ("cube6j", "two_mat"))
def test_a_solve_on_k_plus_sigma_mc(gpu_ctx, models, name):
    from stan_amd import hip
    m = models(name)
    K, Mc, F = m["K"], m["Mc"], m["F"]
    lam1 = float(np.abs(m["csr0"][2]).max() / np.abs(m["mval"]).max())
    for sigma in (T.coef(1e-4)["a0"], 0.1 * lam1):
        S = K.axpy(sigma, Mc)
        try:
            csr = S.to_csr(upper_only=False)
            for eps in (1e-6, 1e-10):
                if eps < 1e-7:
                    gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
                try:
                    x, rep = S.cg_solve(F, eps)
                finally:
                    gpu_ctx.set_option(hip.OPT_CG_MERIT_STOP, 1)
                res = _scaled_residual(csr, F, x)
                print("%s sigma=%.3e eps=%g: type %d, %d its, scaled residual %.3e" % (name, sigma, eps, rep["terminationtype"], rep["iterations"], res))
                assert rep["terminationtype"] == 1 and res <= 2 * eps, (name, sigma, eps, res)
        finally:
            S.free()


def test_axpy_error_cases(gpu_ctx, models):
    from stan_amd import hip
    from stan_amd.cube import cube_mesh
    m = models("cube6j")
    K, Mc = m["K"], m["Mc"]
    for sigma in (float("nan"), float("inf")):
        assert _code(lambda: K.axpy(sigma, Mc)) == hip.E_ARG
    assert _code(lambda: K.axpy(1.0, None)) == hip.E_ARG
    assert _code(lambda: K.axpy(1.0, models("column20")["Mc"])) == hip.E_ARG            # other sizes: found on the host
    # the same cube with other supports: the same sizes and pattern, fixmask and the reduction map differ (found on the device)
    xyz, conn = cube_mesh(4, jitter=0.1)
    lo, hi = np.nonzero(np.arange(125) % 5 == 0)[0], np.nonzero(np.arange(125) % 5 == 4)[0]
    ja = B.box_job(xyz, conn, lo, hi, np.tile([1.0, 0.0, 0.0], (hi.shape[0], 1)))
    jb = B.box_job(xyz, conn, hi, lo, np.tile([1.0, 0.0, 0.0], (lo.shape[0], 1)))
    Ka, Kb = gpu_ctx.assemble_hex8(*_mesh_args(ja)), gpu_ctx.assemble_hex8(*_mesh_args(jb))
    ia, ib = Ka.info(), Kb.info()
    assert {k: v for k, v in ia.items() if k != "bytes_matrix"} == {k: v for k, v in ib.items() if k != "bytes_matrix"}
    assert _code(lambda: Ka.axpy(1.0, Kb)) == hip.E_ARG
    # layouts that differ in pattern: one corner of one element moved to another node of the mesh
    far = conn.copy()
    far[0, 6] = conn[-1, 6]
    jc = B.box_job(xyz, far, lo, hi, np.tile([1.0, 0.0, 0.0], (hi.shape[0], 1)))
    Kc = gpu_ctx.assemble_hex8(*_mesh_args(jc))
    assert _code(lambda: Ka.axpy(1.0, Kc)) == hip.E_ARG
    S = Ka.axpy(1.0, Ka)                                                                # and a matrix with itself is fine: 2 A
    assert np.array_equal(S.to_csr(upper_only=False)[2], 2.0 * Ka.to_csr(upper_only=False)[2])
    # on an error *out is not written
    k = C.c_void_p(0x5EED)
    assert gpu_ctx.lib.stan_hip_matrix_axpy(gpu_ctx.h, Ka.k, C.c_double(1.0), Kb.k, C.byref(k)) == hip.E_ARG and k.value == 0x5EED
    ctx2 = hip.Context(0)
    try:
        K2 = ctx2.assemble_hex8(*_mesh_args(ja))
        assert _code(lambda: Ka.axpy(1.0, K2)) == hip.E_ARG                             # another context's matrix
        K2.free()
    finally:
        ctx2.close()
    for x in (S, Kc, Kb, Ka):
        x.free()


# ---- 4. modes on the pencil ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pencils(gpu_ctx, models):
    """name -> dict(Kd, Md, mu_ref descending, Phi, rest): the reference from the exported matrices, once."""
    made = {}

    def get(name):
        if name not in made:
            m = models(name)
            Kd, Md = MR.dense(*m["csr0"]), MR.dense(*m["Mc"].to_csr(upper_only=False))
            mu_ref, Phi, _low = B.eigh_ref(Md, Kd, B.N_REF)
            k = M.K_MODES[name]
            rest = M.restatement(Kd, Md, k, tol=TOL, max_outer=100)
            made[name] = dict(Kd=Kd, Md=Md, mu_ref=mu_ref, Phi=Phi, rest=rest, k=k)
        return made[name]
    return get


def _check_pairs(name, Kd, Md, mu_ref, Phi, k, lam, phi, skip=0):
    """the rigorous bounds of tests/test_gpu_buckling.py on the pairs from index `skip` on"""
    mu = 1.0 / lam
    bound, rn = B.residual_bound(Kd, Md, mu, phi)
    ok = np.abs(mu - mu_ref[:k]) <= bound + 8 * U53 * np.abs(mu_ref[:k])
    assert ok[skip:].all(), (name, mu, mu_ref[:k], bound)
    for a, b, gap in B.clusters(mu_ref, k):
        if a < skip:
            continue
        s = B.sin_max_angle_K(phi[a:b].T, Phi[:, a:b], Kd)
        print("  cluster", a, b, "sin %.3e bound %.3e" % (s, 2 * rn[a:b].max() / gap))
        assert s <= 2 * rn[a:b].max() / gap, (name, a, b, s)


@pytest.mark.parametrize("name", M.MODELS)
def test_modes_on_the_pencil_against_the_dense_eigen_solve(gpu_ctx, models, pencils, name):
    m, p = models(name), pencils(name)
    K, Mc, Kd, Md, mu_ref, k, rest = m["K"], m["Mc"], p["Kd"], p["Md"], p["mu_ref"], p["k"], p["rest"]
    N = Kd.shape[0]
    assert (mu_ref[k - 1] - mu_ref[k]) / mu_ref[k - 1] > 1e-3 * mu_ref[k] / mu_ref[k - 1]      # MR.pick_k's gap, in lambda
    assert rest["converged"] and rest["outer"] <= M.RESTATEMENT_OUTER[name]
    mbits = _bits(m["mval"])
    # the solves are the CG's at solve_eps 1e-6, not exact: three steps on top of the restatement's count, as the buckling test
    lam, phi, rho, rep = gpu_ctx.modes_pencil(K, Mc, k, tol=TOL, max_outer=M.RESTATEMENT_OUTER[name] + 3)
    orth, orth_ref = M.orthonormality(phi, Md), M.orthonormality(rest["phi"], Md)
    print(name, "N", N, "k", k, "restatement outer", rest["outer"], rep, "lambda", lam, "rho", rho)
    print("  max |Phi^T M_c Phi - I|: device %.3e, restatement %.3e" % (orth, orth_ref))
    assert rep["converged"] == 1 and rep["block"] == MR.block_size(N, k) and rep["cg_worst_type"] > 0
    assert rep["outer"] <= rest["outer"] + 3 and rep["n_positive"] == rep["block"] and rep["lowest_negative_factor"] == 0.0
    assert (rho <= TOL).all() and rep["max_rho"] == rho.max()
    assert (np.diff(lam) >= 0).all() and (lam > 0).all()
    assert (B.rho_host(Kd, Md, 1.0 / lam, phi) <= 2 * TOL).all()
    _check_pairs(name, Kd, Md, mu_ref, p["Phi"], k, lam, phi)
    assert orth <= 4 * orth_ref, (orth, orth_ref)
    for x in phi:                                       # the entry of largest magnitude is positive, at the lowest index
        assert x[int(np.argmax(np.abs(x)))] > 0
    assert np.array_equal(_bits(Mc.to_csr(upper_only=False)[2]), mbits)       # M_c is unchanged to the bit


def test_pencil_same_bits_twice_from_device_pointers_and_k_afterwards(gpu_ctx, models, pencils):
    import torch
    name = "cube6"
    m, p = models(name), pencils(name)
    j, K, Mc, k = m["job"], m["K"], m["Mc"], p["k"]
    N, outer = j.n_red, M.RESTATEMENT_OUTER[name] + 3
    first = gpu_ctx.modes_pencil(K, Mc, k, tol=TOL, max_outer=outer)
    again = gpu_ctx.modes_pencil(K, Mc, k, tol=TOL, max_outer=outer)
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    strip = lambda r: {x: v for x, v in r.items() if not x.endswith("_ms")}       # noqa: E731
    assert strip(first[3]) == strip(again[3])
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    outs = [DB.output("lambda", k, g, dev, 1), DB.output("phi", k * N, g, dev, 3), DB.output("rho", k, g, dev, 5)]
    torch.cuda.synchronize()
    rep = gpu_ctx.modes_pencil_dev(K, Mc, k, outs[0].ptr, outs[1].ptr, outs[2].ptr, tol=TOL, max_outer=outer)
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
    l1, p1, rho1, rep1 = gpu_ctx.modes_pencil(K, Mc, k, tol=TOL, max_outer=1)
    assert rep1["outer"] == 1 and rep1["converged"] == 0 and (rho1 > TOL).any()
    host = B.rho_host(p["Kd"], p["Md"], 1.0 / l1, p1)
    assert (rho1 <= 2 * host).all() and (host <= 2 * rho1).all(), (rho1, host)


def test_pencil_on_the_free_cube_through_the_shift(gpu_ctx, models):
    """K is singular: the modes of K + sigma M_c at sigma = lambda_7 are lambda + sigma, six of them sigma itself."""
    m = models(T.FREE)
    K, Mc = m["K"], m["Mc"]
    Kd, Md = MR.dense(*m["csr0"]), MR.dense(*Mc.to_csr(upper_only=False))
    import scipy.linalg
    sigma = float(scipy.linalg.eigh(Kd, Md, eigvals_only=True, subset_by_index=[6, 6])[0])
    S = K.axpy(sigma, Mc)
    try:
        Sd = MR.dense(*S.to_csr(upper_only=False))
        mu_ref, Phi, _low = B.eigh_ref(Md, Sd, B.N_REF)
        rest = M.restatement(Sd, Md, FREE_K, tol=TOL, max_outer=100)
        assert rest["converged"] and rest["outer"] <= FREE_OUTER
        lam, phi, rho, rep = gpu_ctx.modes_pencil(S, Mc, FREE_K, tol=TOL, max_outer=FREE_OUTER + 3)
        print("free cube: sigma %.6e" % sigma, rep, "lambda - sigma", lam - sigma, "rho", rho)
        assert rep["converged"] == 1 and (rho <= TOL).all() and rep["outer"] <= rest["outer"] + 3
        assert (np.abs(lam[:6] - sigma) <= 2 * TOL * sigma).all()                 # the rigid-body modes
        _check_pairs(T.FREE, Sd, Md, mu_ref, Phi, FREE_K, lam, phi, skip=6)       # the elastic ones
        assert abs((lam[6] - sigma) / sigma - 1.0) <= 1e-6
    finally:
        S.free()


def test_pencil_error_cases(gpu_ctx, models, pencils):
    from stan_amd import hip
    m, other = models("cube6"), models("column20")
    K, Mc = m["K"], m["Mc"]
    N = m["job"].n_red
    assert _code(lambda: gpu_ctx.modes_pencil(K, other["Mc"], 2)) == hip.E_ARG        # a mass of another layout
    assert _code(lambda: gpu_ctx.modes_pencil(K, Mc, N + 1)) == hip.E_ARG
    assert _code(lambda: gpu_ctx.modes_pencil(K, Mc, 0)) == hip.E_ARG
    assert _code(lambda: gpu_ctx.modes_pencil(K, Mc, 25)) == hip.E_ARG                # a block of 33 columns
    assert _code(lambda: gpu_ctx.modes_pencil(K, Mc, 2, tol=-1.0)) == hip.E_ARG
    assert _code(lambda: gpu_ctx.modes_pencil_dev(K, Mc, 2, None, None, None)) == hip.E_ARG
    f = models(T.FREE)                                                                # a free-free K is not positive definite
    assert _code(lambda: gpu_ctx.modes_pencil(f["K"], f["Mc"], 2, max_outer=5)) == hip.E_UNSUPPORTED
    # a mass that is not positive definite: -M_c (fma(-2, m, m) is exact) has no positive mu at all; the call says converged = 0,
    # fills nothing, and names the most negative mu, which is -1 / lambda_1
    neg = Mc.axpy(-2.0, Mc)
    try:
        assert np.array_equal(neg.to_csr(upper_only=False)[2], -m["mval"])
        lam, phi, rho, rep = gpu_ctx.modes_pencil(K, neg, 2, tol=TOL, max_outer=20)
        print("negative mass:", rep, lam)
        assert rep["converged"] == 0 and rep["outer"] == 20 and rep["n_positive"] == 0
        assert not lam.any() and not phi.any() and not rho.any()
        lam1 = 1.0 / pencils("cube6")["mu_ref"][0]
        assert abs(rep["lowest_negative_factor"] + lam1) <= 1e-3 * lam1
    finally:
        neg.free()
    lam = gpu_ctx.modes_pencil(K, Mc, 1, tol=TOL, max_outer=40)[0]                    # the model still answers after all of it
    assert lam[0] > 0


# ---- 5. console ---------------------------------------------------------------------------------------------------------------
def test_console_modes_on_the_consistent_mass(gpu_ctx, tmp_path, built_libs):
    import json
    import os
    import re
    import subprocess
    from stan_amd.cube import cube_mesh
    from tests.test_gpu_modes import _console_db
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "m.STdb"), str(tmp_path / "out")
    n_nodes = _console_db(path, True)
    before = open(path, "rb").read()
    out = subprocess.run([exe, "--modes", "3", "--mass", "consistent", "--json", "--vtu", prefix, path], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    assert "Natural frequencies: (consistent mass, block 6," in out.stdout
    mo = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["modes"]
    assert mo["mass"] == "consistent" and mo["n_modes"] == 3 and mo["block"] == 6 and mo["converged"] == 1
    lam = np.array(mo["lambda"])
    assert (np.diff(lam) >= 0).all() and (np.array(mo["rho"]) <= 1e-6).all()
    assert abs(mo["total_mass"] - MR.RHO * 64.0) <= 64 * U53 * MR.RHO * 64.0
    # its lambda are the entry's on the same model (the console numbers the DOFs itself: equal up to the second order of rho)
    xyz, conn = cube_mesh(4)
    fixed = np.nonzero(xyz[:, 0] == 0.0)[0]
    j = B.box_job(xyz, conn, fixed, fixed[:1], np.zeros((1, 3)))
    K = gpu_ctx.assemble_hex8(*_mesh_args(j))
    Mc = _mass(K, j, np.array([MR.RHO]))
    try:
        want = gpu_ctx.modes_pencil(K, Mc, 3)[0]
    finally:
        Mc.free()
        K.free()
    assert (np.abs(lam - want) <= 1e-9 * want).all(), (lam, want)
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Natural frequencies:")[1], flags=re.M)[:3]
    assert [int(r[0]) for r in rows] == [1, 2, 3] and np.allclose([float(r[1]) for r in rows], lam, rtol=1e-8)
    for k in range(1, 4):
        text = open("%s_mode_%03d.vtu" % (prefix, k), "rb").read()
        for name in ("Mode Shape X", "Mode Shape Y", "Mode Shape Z", "Magnitude"):
            assert ('Name="%s"' % name).encode() in text, (k, name)
        assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    assert not os.path.exists("%s_mode_004.vtu" % prefix)
    # --modes alone: today's output, untouched by the option
    out0 = subprocess.run([exe, "--modes", "3", "--json", path], capture_output=True, text=True, timeout=300)
    assert out0.returncode == 0 and "consistent" not in out0.stdout and "Natural frequencies: (block 6," in out0.stdout
    m0 = json.loads([l for l in out0.stdout.splitlines() if l.startswith("{")][-1])["modes"]
    assert "mass" not in m0 and len(m0["lambda"]) == 3
    out1 = subprocess.run([exe, "--modes", "3", "--mass", "lumped", "--json", path], capture_output=True, text=True, timeout=300)
    assert out1.returncode == 0 and json.loads([l for l in out1.stdout.splitlines() if l.startswith("{")][-1])["modes"]["lambda"] == m0["lambda"]
    # the refusals: no "Density", another word, --mass consistent without --modes; the files are untouched
    plain = str(tmp_path / "plain.STdb")
    _console_db(plain, False)
    kept = open(plain, "rb").read()
    out = subprocess.run([exe, "--modes", "3", "--mass", "consistent", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "Density" in out.stderr and open(plain, "rb").read() == kept
    out = subprocess.run([exe, "--modes", "3", "--mass", "hrz", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--mass" in out.stderr
    out = subprocess.run([exe, "--mass", "consistent", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--modes" in out.stderr
    out = subprocess.run([exe, "--modes", "3", "--mass", "consistent", "--devices", "0,0", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "one device" in out.stderr
    assert open(path, "rb").read() == before
