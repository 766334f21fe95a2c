"""Transient dynamics on the device: the shifted matrix K + sigma M bit for bit against the export of K,
what it leaves of K and what the solver makes of it; the Newmark step kernels alone against np.longdouble; every step of
stan_hip_transient as a Newmark step of the device's own state; the trajectory against the numpy restatement with exact solves
(tests/transient_ref.py); reproducibility, the device-pointer entry, the error cases; free-free modes through the shift.

Kernel bounds (k 2^-53 sum |terms| against long double, k = the floating-point operations of the entry's expression, first
order; a contraction to a fused multiply-add only removes a rounding):
  w  = a1 u + a4 v + a5 a                                      k = 5   (3 products, 2 sums)
  b  = (g F + M (p + alpha_R w) [+ beta_R Kw]) / c_K           k = 18 / 20: p 5, w 5, alpha_R w 1, the sum 1, M x 1, g F 1, the sum 1,
                                                               [beta_R Kw 1, the sum 1,] the division 1, and c_K = 1 + a1 beta_R 2
  a' = a0 (u' - u) - a2 v - a3 a                               k = 6   (the difference, 3 products, 2 differences)
  v' = v + dt ((1 - gamma) a + gamma a')                       k = 12: 1 - gamma 1, 2 products, the sum 1, dt x 1, the sum 1, and a' 6
  a0 = (g F - alpha_R (M v0) - beta_R Kv0 - Ku0) / M           k = 8, plus the two products' own errors (see the test)
  energies: a term is 2 products, a sum of N terms adds N - 1 roundings, the factor one more: (N + 2) 2^-53 sum |terms|."""
import fractions

import numpy as np
import pytest

from tests import device_buffers as DB
from tests import modes_ref as R
from tests import transient_ref as T

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
STEPS = 40
DTS = (1.0 / 2000, 1.0 / 20, 5.0)      # dt / T1
ALL = T.MODELS + (T.FREE,)


class _tight:
    """A solve below the floor of ALGLIB's merit stop (near 1e-7 for these systems: the loop ends with type 7 there, as
    tests/test_gpu_parity.py notes) needs STAN_OPT_CG_MERIT_STOP 0 -- what stan_hip_transient sets for its own solves; the default
    comes back."""

    def __init__(self, ctx, eps):
        self.ctx, self.off = ctx, eps < 1e-7

    def __enter__(self):
        from stan_amd import hip
        if self.off:
            self.ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)

    def __exit__(self, *exc):
        from stan_amd import hip
        if self.off:
            self.ctx.set_option(hip.OPT_CG_MERIT_STOP, 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assemble(ctx, j):
    return ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


def _load(j, N, seed=3):
    F = np.asarray(j.F, dtype=np.float64)
    return F if np.abs(F).max() > 0 else np.random.default_rng(seed).standard_normal(N)     # (the free cube carries no load)


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, M, F, csr (full export of a fresh K), Kd, lam, Phi, T1, U_fresh): computed once, left unchanged.
    T1 of the free cube is the period of its first elastic mode (lambda_7)."""
    made = {}

    def get(name):
        if name not in made:
            j = T.job(name)
            K = _assemble(gpu_ctx, j)
            M = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, T.mat_rho(name))[0]
            csr = K.to_csr(upper_only=False)
            Kd = R.dense(*csr)
            F = _load(j, M.shape[0])
            if name == T.FREE:
                lam, Phi = R.eigh_ref(Kd, M)
                first = 6
            else:
                r = T.reference(name, Kd)
                lam, Phi, first = r["lam"], r["Phi"], 0
            U_fresh = K.cg_solve(F, 1e-8) if name != T.FREE else None
            K.free()
            made[name] = dict(job=j, M=M, F=F, csr=csr, Kd=Kd, lam=lam, Phi=Phi, T1=2.0 * np.pi / np.sqrt(lam[first]), U_fresh=U_fresh)
        return made[name]
    return get


def _fma_diag(rowptr, col, val, M, sigma):
    """val with fl(v + sigma M_d) on the diagonal, one rounding (exact rational arithmetic, rounded once by float())."""
    out = val.copy()
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    fs = fractions.Fraction(float(sigma))
    for q in np.nonzero(rows == col)[0]:
        out[q] = float(fractions.Fraction(float(val[q])) + fs * fractions.Fraction(float(M[col[q]])))
    return out


def _scaled_residual(csr, b, x):
    """||S (b - A x)|| / ||S b|| in long double, S = diag(A)^-1/2, A the exported matrix"""
    rowptr, col, val = csr
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    s = 1.0 / np.sqrt(val[rows == col].astype(LD))
    r = s * (np.asarray(b, dtype=LD) - T.csr_ld(rowptr, col, val)(x))
    return float(np.sqrt((r * r).sum()) / np.sqrt(((s * np.asarray(b, dtype=LD)) ** 2).sum()))


def _sigmas(m):
    return (0.0,) + tuple(T.coef(r * m["T1"])["a0"] for r in DTS)


# ---- 1. the shifted matrix ----------------------------------------------------------------------------------------------------
def _check_shifted(ctx, name, m, after_solve, options=()):
    from stan_amd import hip
    j, M, F = m["job"], m["M"], m["F"]
    for opt, val in options:
        ctx.set_option(opt, val)
    K = _assemble(ctx, j)
    try:
        if after_solve:
            K.cg_solve(F, 1e-8, max_its=50)       # (the free cube's K is singular: the solve only has to leave S K S in place)
            assert K.info()["scaled"] == 1
        info0, csr0 = K.info(), K.to_csr(upper_only=False)
        if not after_solve and not options:
            assert all(np.array_equal(a, b) for a, b in zip(csr0, m["csr"]))
        pool0 = None
        for sigma in _sigmas(m):
            S = K.shifted(sigma, M)
            try:
                got = S.to_csr(upper_only=False)
                assert np.array_equal(got[0], csr0[0]) and np.array_equal(got[1], csr0[1]), "pattern differs"
                want = _fma_diag(csr0[0], csr0[1], csr0[2], M, sigma)
                diff = np.nonzero(_bits(got[2]) != _bits(want))[0]
                assert diff.size == 0, (name, sigma, diff.size, int(diff[0]) if diff.size else -1)
                si = S.info()
                assert si["scaled"] == 0 and si["n_reduced"] == info0["n_reduced"] and si["n_slots"] == info0["n_slots"]
                assert si["sell_sigma"] == info0["sell_sigma"]
                # K itself: export and info unchanged to the bit
                again = K.to_csr(upper_only=False)
                assert all(np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
                           for a, b in zip(again, csr0))
                assert K.info() == info0
                if sigma > 0:
                    # a solve on the shifted matrix: the scaled residual, recomputed in long double from its export
                    for eps in (1e-6, 1e-10):
                        with _tight(ctx, eps):
                            x, rep = S.cg_solve(F, eps)
                        res = _scaled_residual(got, F, x)
                        print("%s sigma=%.3e eps=%g: type %d, %d its, scaled residual %.3e" %
                              (name, sigma, eps, rep["terminationtype"], rep["iterations"], res))
                        assert rep["terminationtype"] == 1 and res <= 2 * eps, (name, sigma, eps, res)
                    assert S.info()["scaled"] == 1 and K.info() == info0
            finally:
                S.free()
            # the calls leave the pool as the first one left it
            if pool0 is None:
                pool0 = ctx.pool_info()
            assert ctx.pool_info() == pool0
        if m["U_fresh"] is not None and not options:
            U, rep = K.cg_solve(F, 1e-8)
            assert np.array_equal(_bits(U), _bits(m["U_fresh"][0])) and rep == m["U_fresh"][1]
    finally:
        K.free()
        for opt, _ in options:
            ctx.set_option(opt, {hip.OPT_SELL_SIGMA: 1, hip.OPT_ROW_FOLDING: -1}[opt])


@pytest.mark.parametrize("after_solve", (False, True), ids=("fresh", "scaled"))
@pytest.mark.parametrize("name", ALL)
def test_shifted_matrix_has_the_bits_of_the_export_plus_the_fused_shift(gpu_ctx, models, name, after_solve):
    _check_shifted(gpu_ctx, name, models(name), after_solve)


@pytest.mark.parametrize("option", ("sell_sigma_32", "row_folding_1"))
def test_shifted_matrix_under_the_layout_options(gpu_ctx, models, option):
    from stan_amd import hip
    opts = {"sell_sigma_32": ((hip.OPT_SELL_SIGMA, 32),), "row_folding_1": ((hip.OPT_ROW_FOLDING, 1),)}[option]
    for after_solve in (False, True):
        _check_shifted(gpu_ctx, "perforated12", models("perforated12"), after_solve, opts)


def test_shifted_matrix_outlives_K_and_takes_the_batched_solve(gpu_ctx, models):
    """The shifted matrix survives freeing K; stan_hip_cg_solve_multi on it gives column j the bits of the single solve under
    the three options the header names."""
    from stan_amd import hip
    m = models("cube6j")
    M, F = m["M"], m["F"]
    sigma = T.coef(m["T1"] / 20)["a0"]
    K = _assemble(gpu_ctx, m["job"])
    S = K.shifted(sigma, M)
    before = S.to_csr(upper_only=False)
    K.free()
    try:
        after = S.to_csr(upper_only=False)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        rng = np.random.default_rng(11)
        cols = np.stack([F, rng.standard_normal(F.shape[0]), M * m["Phi"][:, 0]])
        for o in (hip.OPT_SPMV_SMALL, hip.OPT_CG_FUSED_REFRESH, hip.OPT_ROW_FOLDING):
            gpu_ctx.set_option(o, 0)
        try:
            with _tight(gpu_ctx, 1e-8):
                singles = [S.cg_solve(c, 1e-8) for c in cols]
                U, reps = S.cg_solve_multi(cols, 1e-8)
        finally:
            gpu_ctx.set_option(hip.OPT_SPMV_SMALL, 150000)
            gpu_ctx.set_option(hip.OPT_CG_FUSED_REFRESH, 1)
            gpu_ctx.set_option(hip.OPT_ROW_FOLDING, -1)
        for jc in range(3):
            assert reps[jc] == singles[jc][1] and np.array_equal(_bits(U[jc]), _bits(singles[jc][0])), jc
            assert _scaled_residual(after, cols[jc], U[jc]) <= 2e-8
    finally:
        S.free()


def test_shifted_matrix_error_cases(gpu_ctx, models):
    import torch
    from stan_amd import hip
    m = models("cube6")
    M = m["M"]
    K = _assemble(gpu_ctx, m["job"])
    other = hip.Context(0)
    try:
        K.shifted(1.0, M).free()
        pool0 = gpu_ctx.pool_info()
        bad_M = [M.copy() for _ in range(4)]
        bad_M[0][7] = 0.0; bad_M[1][0] = -1.0; bad_M[2][-1] = float("nan"); bad_M[3][5] = float("inf")
        cases = [(-1.0, M), (float("nan"), M), (float("inf"), M)] + [(1.0, b) for b in bad_M]
        for sigma, Mx in cases:
            with pytest.raises(hip.StanHipError) as ei:
                K.shifted(sigma, Mx)
            assert ei.value.code == hip.E_ARG, (sigma,)
            assert gpu_ctx.pool_info() == pool0
        assert "M[7]" in _raises(hip, lambda: K.shifted(1.0, bad_M[0]), hip.E_ARG)
        # NULL pointers, a K of another context: *out is not written
        lib, out = gpu_ctx.lib, hip.C.c_void_p(12345)
        Mp = M.ctypes.data_as(hip.C.POINTER(hip.C.c_double))
        assert lib.stan_hip_matrix_shifted(gpu_ctx.h, K.k, hip.C.c_double(1.0), None, hip.C.byref(out)) == hip.E_ARG
        assert lib.stan_hip_matrix_shifted(gpu_ctx.h, None, hip.C.c_double(1.0), Mp, hip.C.byref(out)) == hip.E_ARG
        assert lib.stan_hip_matrix_shifted(gpu_ctx.h, K.k, hip.C.c_double(1.0), Mp, None) == hip.E_ARG
        assert lib.stan_hip_matrix_shifted(other.h, K.k, hip.C.c_double(1.0), Mp, hip.C.byref(out)) == hip.E_ARG
        assert lib.stan_hip_matrix_shifted_dev(gpu_ctx.h, K.k, hip.C.c_double(1.0), None, hip.C.byref(out)) == hip.E_ARG
        assert out.value == 12345 and gpu_ctx.pool_info() == pool0
        # the device entry: M through a caller's pointer one element past a 256-byte boundary, read only
        dev = torch.device("cuda:0")
        dM = DB.input_("M", M, DB.guard_len(M.shape[0]), dev, offset=1)
        torch.cuda.synchronize()
        S = K.shifted_dev(2.5, dM.ptr)
        S2 = K.shifted(2.5, M)
        DB.check([dM])
        assert all(np.array_equal(a, b) for a, b in zip(S.to_csr(False), S2.to_csr(False)))
        S.free(); S2.free()
    finally:
        other.close()
        K.free()


def test_shifted_matrix_is_refused_on_a_communicator(gpu_ctx, models):
    from stan_amd import hip
    m = models("cube6")
    c = hip.Context(0)
    try:
        c.comm_init(0, 2, None)              # a detached rank of two
        K = _assemble(c, m["job"])
        try:
            assert "communicator" in _raises(hip, lambda: K.shifted(1.0, m["M"]), hip.E_UNSUPPORTED)
            assert "communicator" in _raises(hip, lambda: K.transient(m["M"], m["F"], 1.0, 1), hip.E_UNSUPPORTED)
        finally:
            K.free()
    finally:
        c.close()
    multi = hip.Context(devices=[0])         # a multi-device handle (one device, no communicator)
    try:
        j = m["job"]
        Km = multi.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        assert "multi-device" in _raises(hip, lambda: Km.shifted(1.0, m["M"]), hip.E_UNSUPPORTED)
        assert "multi-device" in _raises(hip, lambda: Km.transient(m["M"], m["F"], 1.0, 1), hip.E_UNSUPPORTED)
        N = m["M"].shape[0]
        one = np.ones(N)
        _raises(hip, lambda: multi.newmark_predict(one, one, one, one, one, T.coef(1.0)["vec"], 1.0), hip.E_UNSUPPORTED)
        _raises(hip, lambda: multi.newmark_correct(one, one, one, one, T.coef(1.0)["vec"], 1.0, 0.5), hip.E_UNSUPPORTED)
        Km.free()
    finally:
        multi.close()


def _raises(hip, fn, code):
    with pytest.raises(hip.StanHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


# ---- 2. the step kernels alone ----------------------------------------------------------------------------------------------
KERNEL_N = (1, 63, 64, 65, 255, 257, 4097, 200003)


def _vec(rng, N):
    return rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 6, N)


def _predict_ref(c, u, v, a, F, M, Kw, gF):
    """(w, its term sum, b, its term sum) in long double; c: transient_ref.coef"""
    u, v, a, F, M = (x.astype(LD) for x in (u, v, a, F, M))
    a0, a1, a2, a3, a4, a5, al, be, cK = (LD(c[k]) for k in ("a0", "a1", "a2", "a3", "a4", "a5", "alpha_R", "beta_R", "c_K"))
    w, ws = a1 * u + a4 * v + a5 * a, np.abs(a1 * u) + np.abs(a4 * v) + np.abs(a5 * a)
    p, ps = a0 * u + a2 * v + a3 * a, np.abs(a0 * u) + np.abs(a2 * v) + np.abs(a3 * a)
    b, bs = LD(gF) * F + M * (p + al * w), np.abs(LD(gF) * F) + M * (ps + al * ws)
    if Kw is not None:
        b, bs = b + be * Kw.astype(LD), bs + np.abs(be * Kw.astype(LD))
    return w, ws, b / cK, bs / cK


def _correct_ref(c, un, u, v, a):
    un, u, v, a = (x.astype(LD) for x in (un, u, v, a))
    a0, a2, a3, dt, g = (LD(c[k]) for k in ("a0", "a2", "a3", "dt", "gamma"))
    an, ans = a0 * (un - u) - a2 * v - a3 * a, np.abs(a0 * un) + np.abs(a0 * u) + np.abs(a2 * v) + np.abs(a3 * a)
    vn, vns = v + dt * ((1 - g) * a + g * an), np.abs(v) + dt * (np.abs((1 - g) * a) + g * ans)
    return an, ans, vn, vns


def _energy_ref(u, v, M, F, Ku, gF):
    u, v, M, F, Ku = (x.astype(LD) for x in (u, v, M, F, Ku))
    terms = np.stack([LD(0.5) * M * v * v, LD(0.5) * u * Ku, LD(gF) * F * u])
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


@pytest.mark.parametrize("N", KERNEL_N)
def test_step_kernels_against_longdouble(gpu_ctx, N):
    rng = np.random.default_rng(100 + N % 991)
    u, v, a, F, Kw, un, Ku = (_vec(rng, N) for _ in range(7))
    M = 10.0 ** rng.uniform(-6, 6, N)
    for damped in (False, True):
        c = T.coef(3.7e-4, 0.3025, 0.6, 0.8, 2.5e-5) if damped else T.coef(3.7e-4)
        gF = 0.625
        w, b = gpu_ctx.newmark_predict(u, v, a, F, M, c["vec"], gF, Kw=Kw if damped else None)
        wr, ws, br, bs = _predict_ref(c, u, v, a, F, M, Kw if damped else None, gF)
        ew = (np.abs(w.astype(LD) - wr) / (5 * U53 * ws)).max()
        eb = (np.abs(b.astype(LD) - br) / ((20 if damped else 18) * U53 * bs)).max()
        un2, vn, an, e = gpu_ctx.newmark_correct(un, u, v, a, c["vec"], c["dt"], c["gamma"], M=M, F=F, Ku=Ku, gF=gF, energy=True)
        ar, ars, vr, vrs = _correct_ref(c, un, u, v, a)
        ea = (np.abs(an.astype(LD) - ar) / (6 * U53 * ars)).max()
        ev = (np.abs(vn.astype(LD) - vr) / (12 * U53 * vrs)).max()
        assert np.array_equal(_bits(un2), _bits(un))
        er, ers = _energy_ref(un2, vn, M, F, Ku, gF)      # of the device's own u', v'
        ee = (np.abs(e.astype(LD) - er) / ((N + 2) * U53 * ers)).max()
        print("N=%d damped=%d: w %.3f b %.3f a' %.3f v' %.3f energies %.3f of their bounds" % (N, damped, ew, eb, ea, ev, ee))
        assert max(ew, eb, ea, ev, ee) <= 1.0, (N, damped, float(ew), float(eb), float(ea), float(ev), float(ee))
        # without the energies: the same bits; twice: the same bits
        _, vn2, an2, e2 = gpu_ctx.newmark_correct(un, u, v, a, c["vec"], c["dt"], c["gamma"])
        assert e2 is None and np.array_equal(_bits(vn2), _bits(vn)) and np.array_equal(_bits(an2), _bits(an))
        _, _, _, e3 = gpu_ctx.newmark_correct(un, u, v, a, c["vec"], c["dt"], c["gamma"], M=M, F=F, Ku=Ku, gF=gF, energy=True)
        assert np.array_equal(_bits(e3), _bits(e))
        w2, b2 = gpu_ctx.newmark_predict(u, v, a, F, M, c["vec"], gF, Kw=Kw if damped else None, want_w=False)
        assert w2 is None and np.array_equal(_bits(b2), _bits(b))


# ---- 3. the driver ----------------------------------------------------------------------------------------------------------------
def _damping(m, damped):
    return T.rayleigh(np.sqrt(m["lam"][0]), np.sqrt(m["lam"][2]), 0.02) if damped else (0.0, 0.0)


def _run(K, m, dt, damped, eps, **kw):
    al, be = _damping(m, damped)
    return K.transient(m["M"], m["F"], dt, STEPS, alpha_R=al, beta_R=be, solve_eps=eps, **kw)


@pytest.fixture(scope="module")
def matrices(gpu_ctx, models):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _assemble(gpu_ctx, models(name)["job"])
        return made[name]
    yield get
    for K in made.values():
        K.free()


@pytest.mark.parametrize("eps", (1e-6, 1e-10))
@pytest.mark.parametrize("damped", (False, True), ids=("undamped", "rayleigh"))
@pytest.mark.parametrize("dt_over_T1", DTS)
@pytest.mark.parametrize("name", T.MODELS)
def test_every_step_is_a_newmark_step(gpu_ctx, models, matrices, name, dt_over_T1, damped, eps):
    """snap_every = 1: from the device's own state at step n, b in long double; u_{n+1} meets the scaled residual bound 2 eps,
    a_{n+1} and v_{n+1} follow from it within the kernel bounds, and so does a_0.  The start state is u0 = 0.3 phi_2,
    v0 = omega_1 phi_1 (so that every term of a_0 is there)."""
    m, K = models(name), matrices(name)
    M, F = m["M"], m["F"]
    dt = dt_over_T1 * m["T1"]
    al, be = _damping(m, damped)
    c = T.coef(dt, alpha_R=al, beta_R=be)
    u0 = 0.3 * m["Phi"][:, 1] * np.abs(m["U_fresh"][0]).max() / np.abs(m["Phi"][:, 1]).max()
    v0 = np.sqrt(m["lam"][0]) * np.abs(u0).max() / np.abs(m["Phi"][:, 0]).max() * m["Phi"][:, 0]
    out = _run(K, m, dt, damped, eps, u0=u0, v0=v0, snap_every=1)
    rep, sn = out["report"], out["snaps"]
    assert rep["steps"] == STEPS and rep["cg_worst_type"] == 1 and rep["failed_step"] == 0
    assert rep["sigma"] == c["sigma"] and rep["cg_min_iterations"] <= rep["cg_max_iterations"]
    assert rep["cg_min_iterations"] * STEPS <= rep["cg_iterations"] <= rep["cg_max_iterations"] * STEPS
    assert sn.shape == (STEPS + 1, 3, M.shape[0])
    assert np.array_equal(_bits(sn[0, 0]), _bits(u0)) and np.array_equal(_bits(sn[0, 1]), _bits(v0))
    for q, key in enumerate(("u", "v", "a")):
        assert np.array_equal(_bits(sn[STEPS, q]), _bits(out[key]))
    rowptr, col, val = m["csr"]
    Kmul = T.csr_ld(rowptr, col, val)
    Kabs = T.csr_ld(rowptr, col, np.abs(val))
    nnz_row = int(np.diff(rowptr).max())
    Ml, Fl = M.astype(LD), F.astype(LD)
    # a_0: the kernel's 8 operations on its terms, and the two products K v0, K u0 as the device forms them: a row of the
    # product is a sum of at most nnz_row terms a_ij x_j, each through the two scalings of S K S and back (4 more roundings)
    kp = (nnz_row + 4) * U53
    r0 = Fl - LD(al) * (Ml * v0) - LD(be) * Kmul(v0) - Kmul(u0)
    r0s = np.abs(Fl) + LD(al) * np.abs(Ml * v0) + LD(be) * np.abs(Kmul(v0)) + np.abs(Kmul(u0))
    bound0 = (8 * U53 * r0s + kp * (LD(be) * Kabs(np.abs(v0)) + Kabs(np.abs(u0)))) / Ml
    e0 = (np.abs(sn[0, 2].astype(LD) - r0 / Ml) / bound0).max()
    assert e0 <= 1.0, float(e0)
    # the shifted operator in long double: (K + sigma M) x
    diag = (np.repeat(np.arange(M.shape[0]), np.diff(rowptr)) == col)
    sig = LD(c["sigma"])
    d_shift = val[diag].astype(LD) + sig * Ml
    s = 1.0 / np.sqrt(d_shift)
    worst_res = worst_a = worst_v = 0.0
    for n in range(STEPS):
        u, v, a = (sn[n, q] for q in range(3))
        un, vn, an = (sn[n + 1, q] for q in range(3))
        Kw = None
        if damped:
            Kw = np.asarray(Kmul(c["a1"] * u.astype(LD) + c["a4"] * v.astype(LD) + c["a5"] * a.astype(LD)))
        _, _, b, _ = _predict_ref(c, u, v, a, F, M, Kw, 1.0)
        r = s * (b - (Kmul(un) + sig * Ml * un.astype(LD)))
        worst_res = max(worst_res, float(np.sqrt((r * r).sum()) / np.sqrt(((s * b) ** 2).sum())))
        ar, ars, vr, vrs = _correct_ref(c, un, u, v, a)
        worst_a = max(worst_a, float((np.abs(an.astype(LD) - ar) / (6 * U53 * ars)).max()))
        worst_v = max(worst_v, float((np.abs(vn.astype(LD) - vr) / (12 * U53 * vrs)).max()))
    print("%s dt/T1=%g damped=%d eps=%g: its %d..%d, worst scaled residual %.3e (bound %.1e), a0 %.3f a' %.3f v' %.3f of their bounds"
          % (name, dt_over_T1, damped, eps, rep["cg_min_iterations"], rep["cg_max_iterations"], worst_res, 2 * eps, e0, worst_a, worst_v))
    assert worst_res <= 2 * eps, (worst_res, eps)
    assert worst_a <= 1.0 and worst_v <= 1.0, (worst_a, worst_v)


_yard = {}


def _yardstick(m, name, case, dt, F, kw):
    """The largest deviation of 8 perturbed-solve runs of the restatement (eps = 1e-6) from its exact-solve run: of u in the
    M-norm relative to max_n ||u_n||_M, and of the energies relative to the largest energy term.  (exact run, yardstick of u,
    yardstick of the energies, scale), computed once and left unchanged."""
    key = (name, case, dt)
    if key not in _yard:
        M = m["M"]
        exact = T.newmark(m["Kd"], M, F, dt, STEPS, **kw)
        scale = max(T.m_norm(x, M) for x in exact["U"])
        big = np.abs(exact["energy"]).max()
        rng = np.random.default_rng(77)
        dev = dev_e = 0.0
        for _ in range(8):
            p = T.newmark(m["Kd"], M, F, dt, STEPS, eps=1e-6, rng=rng, **kw)
            dev = max(dev, max(T.m_norm(p["U"][n] - exact["U"][n], M) for n in range(STEPS + 1)) / scale)
            dev_e = max(dev_e, float(np.abs(p["energy"] - exact["energy"]).max() / big))
        _yard[key] = (exact, dev, dev_e, scale)
    return _yard[key]


@pytest.mark.parametrize("case", ("step_load", "rayleigh", "free_vibration"))
@pytest.mark.parametrize("dt_over_T1", DTS)
@pytest.mark.parametrize("name", ("cube6", "two_mat"))
def test_trajectory_against_the_restatement(gpu_ctx, models, matrices, name, dt_over_T1, case):
    """u_end, the probe history and the energies against tests/transient_ref.newmark with exact solves.  The yardstick is
    measured on the REFERENCE: the largest deviation of 8 perturbed-solve runs from the exact-solve run; the device may lie
    4 x that away (the factor test_gpu_modes.py gives the device over its restatement)."""
    m, K = models(name), matrices(name)
    M = m["M"]
    dt = dt_over_T1 * m["T1"]
    F, kw = m["F"], {}
    if case == "rayleigh":
        kw["alpha_R"], kw["beta_R"] = _damping(m, True)
    if case == "free_vibration":
        F, kw = np.zeros_like(M), dict(u0=m["Phi"][:, 0].copy())
    exact, yard, yard_e, scale = _yardstick(m, name, case, dt, F, kw)
    probe = np.array([0, M.shape[0] // 2, M.shape[0] - 1], dtype=np.int32)
    out = K.transient(M, F, dt, STEPS, solve_eps=1e-6, probe_dof=probe, snap_every=1, energy=True, **kw)
    dev = max(T.m_norm(out["snaps"][n, 0] - exact["U"][n], M) for n in range(STEPS + 1)) / scale
    end = T.m_norm(out["u"] - exact["U"][STEPS], M) / scale
    e, er = out["energy"], exact["energy"]
    big = np.abs(er).max()
    dev_e = float(np.abs(e - er).max() / big)
    print("%s %s dt/T1=%g: yardstick u %.3e, device %.3e (end state %.3e); yardstick energies %.3e, device %.3e; its %d..%d" %
          (name, case, dt_over_T1, yard, dev, end, yard_e, dev_e, out["report"]["cg_min_iterations"], out["report"]["cg_max_iterations"]))
    assert yard > 0 and dev <= 4 * yard and end <= 4 * yard, (yard, dev, end)
    # the probes are entries of the snapshots, and so lie as close
    assert np.array_equal(_bits(out["probe_u"]), _bits(out["snaps"][:, 0, probe]))
    # the energies against the restatement's, by the yardstick measured on them in the same way
    assert dev_e <= 4 * yard_e, (yard_e, dev_e)
    if case == "free_vibration":      # the closed form of tests/test_transient.py (its bar 1e-9 for the restatement's own distance)
        theta = 2.0 * np.arctan(np.sqrt(m["lam"][0]) * dt / 2.0)
        want = np.cos(np.arange(STEPS + 1) * theta)[:, None] * m["Phi"][:, 0][None, :]
        assert max(T.m_norm(out["snaps"][n, 0] - want[n], M) for n in range(STEPS + 1)) <= (4 * yard + 1e-9) * scale
    if case == "step_load":           # the energy balance: three terms, each within 4 x the yardstick, and the CPU bar
        bal = e[:, 0] + e[:, 1] - e[:, 2]
        assert np.abs(bal - bal[0]).max() <= (2 * 3 * 4 * yard_e + 1e-9) * big


def test_same_bits_twice_and_from_the_device_entry(gpu_ctx, models, matrices):
    """Two calls give the same bits; the host and the _dev entry give the same bits, with the caller's buffers one element past
    a 256-byte boundary: nothing stored outside an output, every entry written, inputs unchanged."""
    import torch
    m, K = models("two_mat"), matrices("two_mat")
    M, F, N = m["M"], m["F"], m["M"].shape[0]
    dt = m["T1"] / 20
    al, be = _damping(m, True)
    u0, v0 = 1e-3 * m["Phi"][:, 1], 0.1 * m["Phi"][:, 0]
    probe = np.array([1, N - 2, 17], dtype=np.int32)
    curve = [(0.0, 0.0), (4 * dt, 1.0), (9 * dt, 1.0), (9 * dt, 0.25)]
    kw = dict(u0=u0, v0=v0, alpha_R=al, beta_R=be, curve=curve, solve_eps=1e-8, probe_dof=probe, snap_every=3, energy=True)
    n_steps = 10
    a = K.transient(M, F, dt, n_steps, **kw)
    b = K.transient(M, F, dt, n_steps, **kw)
    keys = ("u", "v", "a", "probe_u", "snaps", "energy")
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["snaps"].shape == (4, 3, N)
    assert {k: v for k, v in a["report"].items() if not k.endswith("_ms")} == {k: v for k, v in b["report"].items() if not k.endswith("_ms")}
    assert np.array_equal(_bits(a["probe_u"][::3]), _bits(a["snaps"][:, 0, probe]))
    assert a["energy"][0, 2] == 0.0 and a["energy"][-1, 2] != 0.0          # g(0) = 0
    dev = torch.device("cuda:0")
    for offset in (0, 1):
        g = DB.guard_len(N)
        ins = [DB.input_(n, x, g, dev, offset) for n, x in (("M", M), ("F", F), ("u0", u0), ("v0", v0))]
        dp = DB.input_("probe", probe, g, dev, offset)
        outs = [DB.output("u_end", N, g, dev, offset), DB.output("v_end", N, g, dev, offset), DB.output("a_end", N, g, dev, offset),
                DB.output("probe_u", (n_steps + 1) * 3, g, dev, offset), DB.output("snaps", 4 * 3 * N, g, dev, offset),
                DB.output("energy", (n_steps + 1) * 3, g, dev, offset)]
        torch.cuda.synchronize()
        rep = K.transient_dev(ins[0].ptr, ins[1].ptr, dt, n_steps, outs[0].ptr, outs[1].ptr, outs[2].ptr, d_u0=ins[2].ptr,
                              d_v0=ins[3].ptr, alpha_R=al, beta_R=be, curve=curve, solve_eps=1e-8, n_probe=3, d_probe_dof=dp.ptr,
                              d_probe_u=outs[3].ptr, snap_every=3, d_snaps=outs[4].ptr, d_energy=outs[5].ptr)
        DB.check(ins + [dp] + outs)
        for o, k in zip(outs, keys):
            assert np.array_equal(_bits(o.numpy()), _bits(a[k]).reshape(-1)), (offset, k)
        assert rep["steps"] == n_steps and rep["cg_iterations"] == a["report"]["cg_iterations"]
    # K is left as a solve leaves it: a later solve has the bits it has on a fresh assembly
    U, r = K.cg_solve(F, 1e-8)
    assert np.array_equal(_bits(U), _bits(m["U_fresh"][0])) and r == m["U_fresh"][1]


def test_no_steps_returns_the_start_state_and_a0(gpu_ctx, models, matrices):
    m, K = models("cube6"), matrices("cube6")
    M, F = m["M"], m["F"]
    u0 = 1e-3 * m["Phi"][:, 0]
    out = K.transient(M, F, m["T1"] / 20, 0, u0=u0, probe_dof=[3], snap_every=2, energy=True)
    assert out["report"]["steps"] == 0 and out["report"]["cg_iterations"] == 0
    assert np.array_equal(_bits(out["u"]), _bits(u0)) and not out["v"].any()
    want = (F - m["Kd"] @ u0) / M
    assert np.abs(out["a"] - want).max() <= 1e-12 * np.abs(want).max()
    assert out["probe_u"].shape == (1, 1) and out["probe_u"][0, 0] == u0[3]
    assert out["snaps"].shape == (1, 3, M.shape[0]) and np.array_equal(_bits(out["snaps"][0, 2]), _bits(out["a"]))
    assert out["energy"].shape == (1, 3) and out["energy"][0, 0] == 0.0
    # without u0 no product is made: a_0 = F / M to the bit
    out = K.transient(M, F, m["T1"] / 20, 0)
    assert np.array_equal(_bits(out["a"]), _bits(F / M))


def test_a_failed_solve_stops_the_run(gpu_ctx, models, matrices):
    from stan_amd import hip
    m, K = models("cube6"), matrices("cube6")
    with pytest.raises(hip.StanHipError) as ei:
        K.transient(m["M"], m["F"], 5 * m["T1"], 5, solve_eps=1e-10, solve_max_its=1)
    assert ei.value.code == hip.E_UNSUPPORTED and "step 1" in str(ei.value) and "type 5" in str(ei.value)
    rep = ei.value.report
    assert rep["failed_step"] == 1 and rep["steps"] == 0 and rep["cg_worst_type"] == 5 and rep["cg_iterations"] == 1


def test_transient_error_cases(gpu_ctx, models, matrices):
    import torch
    from stan_amd import hip
    m, K = models("cube6"), matrices("cube6")
    M, F, N = m["M"], m["F"], m["M"].shape[0]
    dt = m["T1"] / 20
    bad_M = M.copy(); bad_M[3] = 0.0
    cases = dict(
        dt_zero=dict(dt=0.0), dt_negative=dict(dt=-1.0), dt_nan=dict(dt=float("nan")), steps=dict(n_steps=-1),
        gamma_low=dict(beta_N=0.25, gamma=0.4), beta_low=dict(beta_N=0.2, gamma=0.5), beta_for_gamma=dict(beta_N=0.25, gamma=0.6),
        alpha=dict(alpha_R=-1.0), beta=dict(beta_R=-1e-3), eps=dict(solve_eps=-1.0), its=dict(solve_max_its=-1),
        curve_descends=dict(curve=[(0.0, 1.0), (2.0, 1.0), (1.0, 0.0)]), curve_nan=dict(curve=[(0.0, float("nan"))]),
        curve_inf=dict(curve=[(float("inf"), 1.0)]), probe_high=dict(probe_dof=[0, N]), probe_low=dict(probe_dof=[-1]),
        snap=dict(snap_every=-1), mass=dict(M=bad_M))
    for name, kw in cases.items():
        args = dict(M=M, F=F, dt=dt, n_steps=2)
        args.update(kw)
        with pytest.raises(hip.StanHipError) as ei:
            K.transient(args.pop("M"), args.pop("F"), args.pop("dt"), args.pop("n_steps"), **args)
        assert ei.value.code == hip.E_ARG, (name, str(ei.value))
    # NULL where an array is required; nothing is written through the outputs on an error (device entry, guarded)
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    dM, dF, dbad = DB.input_("M", M, g, dev), DB.input_("F", F, g, dev), DB.input_("M", bad_M, g, dev)
    dp = DB.input_("probe", np.array([0, N], dtype=np.int32), g, dev)
    outs = [DB.output(n, N, g, dev) for n in ("u_end", "v_end", "a_end")] + [DB.output("probe_u", 6, g, dev)]
    torch.cuda.synchronize()
    o = [x.ptr for x in outs]
    for call in (lambda: K.transient_dev(None, dF.ptr, dt, 2, o[0], o[1], o[2]),
                 lambda: K.transient_dev(dM.ptr, None, dt, 2, o[0], o[1], o[2]),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, dt, 2, None, o[1], o[2]),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], None),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=2, d_probe_dof=dp.ptr),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=-1, d_probe_dof=dp.ptr, d_probe_u=o[3]),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=2, d_probe_dof=dp.ptr, d_probe_u=o[3]),
                 lambda: K.transient_dev(dbad.ptr, dF.ptr, dt, 2, o[0], o[1], o[2]),
                 lambda: K.transient_dev(dM.ptr, dF.ptr, 5 * m["T1"], 3, o[0], o[1], o[2], solve_eps=1e-10, solve_max_its=1)):
        with pytest.raises(hip.StanHipError) as ei:
            call()
        assert ei.value.code in (hip.E_ARG, hip.E_UNSUPPORTED)
    DB.check([dM, dF, dbad, dp] + outs, written=False)
    for x in outs:
        assert bool((x.payload.view(torch.int64) == DB.UNWRITTEN_BITS).all()), x.name
    # the defaults: beta_N = gamma = 0 is 1/4, 1/2; snaps without snap_every is ignored
    a = K.transient(M, F, dt, 3)
    b = K.transient(M, F, dt, 3, beta_N=0.25, gamma=0.5)
    assert np.array_equal(_bits(a["u"]), _bits(b["u"])) and a["snaps"] is None


# ---- 4. free-free modes through the shift -----------------------------------------------------------------------------------
def test_free_free_modes_through_the_shift(gpu_ctx, models):
    """The free cube 4^3 at sigma = lambda_7 of the dense reference, tol 1e-6: six rigid-body values |lambda_j| <= 2 tol sigma,
    the elastic ones |lambda_j - lambda_ref| <= 2 tol (lambda_ref + sigma); the subspace checks of test_gpu_modes.py on the
    shifted pencil (eigenvalues mu = lambda + sigma); without the shift the model is refused with type -5."""
    from stan_amd import hip
    m = models(T.FREE)
    M, lam_ref, Phi = m["M"], m["lam"], m["Phi"]
    tol, sigma = 1e-6, float(m["lam"][6])
    assert np.abs(lam_ref[:6]).max() <= 1e-6 * sigma          # the reference sees six rigid-body modes
    mu_ref = lam_ref + sigma
    k = R.pick_k(mu_ref, 8)                                    # six rigid-body modes, two elastic ones, and up to a gap
    K = _assemble(gpu_ctx, m["job"])
    try:
        with pytest.raises(hip.StanHipError) as ei:
            K.modes(M, k, tol=tol)
        assert ei.value.code == hip.E_UNSUPPORTED and "-5" in str(ei.value) and "shift" in str(ei.value)
        lam, phi, rho, rep = K.modes_shifted(M, k, sigma, tol=tol)
        print("free-free: lambda", lam, "rho", rho, "outer", rep["outer"])
        assert rep["converged"] == 1 and rep["shift"] == sigma and rep["max_rho"] <= tol
        assert np.abs(lam[:6]).max() <= 2 * tol * sigma, lam[:6]
        assert (np.abs(lam[6:] - lam_ref[6:k]) <= 2 * tol * (lam_ref[6:k] + sigma)).all(), (lam[6:], lam_ref[6:k])
        assert (rho <= tol).all()
        G = (phi * M[None, :]) @ phi.T
        assert np.abs(G - np.eye(k)).max() <= 1e-10
        # the checks of test_gpu_modes.py on the shifted pencil (K + sigma M, M), eigenvalues mu = lambda + sigma: rho recomputed
        # on the host with its margin 2, and every cluster of the reference (the six rigid-body modes are one) as a subspace
        mu = lam + sigma
        Ks = T.shifted_dense(m["Kd"], M, sigma)
        assert (R.rho_host(Ks, M, mu, phi) <= 2 * tol).all()
        cl = R.clusters(mu_ref, k)
        assert cl[0][:2] == (0, 6), cl
        for a, b, gap in cl:
            sin = R.sin_max_angle(phi[a:b].T, Phi[:, a:b], M)
            bound = 2 * (rho[a:b] * mu[a:b]).max() / gap
            print("  cluster", a, b, "sin %.3e bound %.3e" % (sin, bound))
            assert sin <= bound, (a, b, sin, bound)
    finally:
        K.free()


# ---- 5. console -----------------------------------------------------------------------------------------------------------
def _console_db(path, density=True, move=None, supports=True):
    """A 4^3 cube as tests/test_gpu_modes.py builds its own: clamped on x = 0, PointLoad (0, 0, 50) on the nodes of x = 4."""
    from stan_amd import host
    from stan_amd.cube import cube_mesh
    xyz, conn = cube_mesh(4)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", 210000.0, 0.3)
    d.assign_part(1, 1, "HEX8_G2")
    fixed = np.nonzero(xyz[:, 0] == 0.0)[0]
    tip = np.nonzero(xyz[:, 0] == 4.0)[0]
    if supports:
        d.add_bc(1, "fix", "SPC", fixed + 1, np.ones((fixed.size, 3)))
    d.add_bc(2, "load", "PointLoad", tip + 1, np.tile([0.0, 0.0, 50.0], (tip.size, 1)))
    if density:
        d.add_bc(3, "rho", "Density", [1], np.array([[R.RHO, 0.0, 0.0]]))
    if move is not None:
        d.add_bc(4, "move", "Displacement", fixed + 1, np.tile(move, (fixed.size, 1)))
    d.set_analysis(tol=1e-10)
    d.assign_dof()
    d.write_stdb(path)
    return xyz.shape[0], int(tip[-1]) + 1


def test_console_transient(tmp_path, built_libs):
    import json
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "t.STdb"), str(tmp_path / "out")
    n_nodes, tip = _console_db(path)
    before = open(path, "rb").read()
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True, timeout=300)
    # T1 of the model from the console's own modal analysis
    out = run("--modes", "1", "--json", path)
    assert out.returncode == 0, out.stdout + out.stderr
    lam1 = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["modes"]["lambda"][0]
    dt = 2 * np.pi / np.sqrt(lam1) / 20
    args = ["--transient", "--dt", repr(float(dt)), "--steps", "12", "--rayleigh", "10,1e-7", "--load-curve", "0,0,%r,1" % float(3 * dt),
            "--probe-node", str(tip), "--solve-eps", "1e-8", "--json", "--vtu", prefix, "--vtu-every", "4"]
    out = run(*(args + [path]))
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    assert "Transient:" in out.stdout and "CG iterations per step: min" in out.stdout and "Final energies:" in out.stdout
    t = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["transient"]
    c = T.coef(dt, alpha_R=10.0, beta_R=1e-7)
    assert t["steps"] == 12 and t["dt"] == dt and t["sigma"] == c["sigma"] and (t["beta_N"], t["gamma"]) == (0.25, 0.5)
    assert t["cg_worst_type"] == 1 and 0 < t["cg_min_iterations"] <= t["cg_max_iterations"]
    assert t["cg_min_iterations"] * 12 <= t["cg_iterations"] <= t["cg_max_iterations"] * 12
    assert abs(t["total_mass"] - R.RHO * 64.0) <= 64 * U53 * R.RHO * 64.0
    pu = np.array(t["probe_u"])
    assert t["probe_node"] == tip and t["probe_direction"] == [0, 1, 2] and pu.shape == (13, 3)
    assert not pu[0].any() and pu[-1, 2] > 0 and np.abs(pu[-1, 2]) > np.abs(pu[-1, 1])       # from rest, pulled in z
    ek, es, ee = t["energy_final"]
    assert ek > 0 and es > 0 and ee > 0 and ek + es < ee                                      # damping has taken its share
    # the block carries the same numbers
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Probe node")[1], flags=re.M)[:13]
    assert [int(r[0]) for r in rows] == list(range(13))
    assert np.allclose([[float(x) for x in r[2:]] for r in rows], pu, rtol=1e-8, atol=0)
    assert ("sigma of K + sigma M: %.8e" % c["sigma"]) in out.stdout
    for s in (0, 4, 8, 12):
        text = open("%s_step_%04d.vtu" % (prefix, s), "rb").read()
        for q in ("Displacement", "Velocity", "Acceleration"):
            for ax in "XYZ":
                assert ('Name="%s %s"' % (q, ax)).encode() in text, (s, q, ax)
        assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    assert sorted(os.listdir(str(tmp_path))) == ["out_step_0000.vtu", "out_step_0004.vtu", "out_step_0008.vtu", "out_step_0012.vtu", "t.STdb"]
    # the refusals: no "Density", a non-zero "Displacement", several devices, an unknown probe node; the files stay as they were
    base = ["--transient", "--dt", repr(float(dt)), "--steps", "2"]
    plain = str(tmp_path / "plain.STdb")
    _console_db(plain, density=False)
    b2 = open(plain, "rb").read()
    out = run(*(base + [plain]))
    assert out.returncode == 2 and "Density" in out.stderr and open(plain, "rb").read() == b2
    moved = str(tmp_path / "moved.STdb")
    _console_db(moved, move=[0.0, 0.01, 0.0])
    b3 = open(moved, "rb").read()
    out = run(*(base + [moved]))
    assert out.returncode == 2 and "Displacement" in out.stderr and open(moved, "rb").read() == b3
    zero = str(tmp_path / "zero.STdb")
    _console_db(zero, move=[0.0, 0.0, 0.0])         # a homogeneous "Displacement" is a support
    out = run(*(base + [zero]))
    assert out.returncode == 0, out.stdout + out.stderr
    out = run(*(base + ["--devices", "0,0", path]))
    assert out.returncode == 2 and "one device" in out.stderr
    out = run(*(base + ["--probe-node", "9999", path]))
    assert out.returncode == 2 and "no such node" in out.stderr
    assert open(path, "rb").read() == before


def test_console_modes_shift(tmp_path, built_libs):
    """A model without supports: refused without the flag, the refusal names it; with it six rigid-body values and the elastic
    ones of the library's own shifted run."""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path = str(tmp_path / "free.STdb")
    _console_db(path, supports=False)
    before = open(path, "rb").read()
    out = subprocess.run([exe, "--modes", "8", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "--modes-shift" in out.stderr and open(path, "rb").read() == before
    sigma = 1e10
    out = subprocess.run([exe, "--modes", "8", "--modes-shift", repr(sigma), "--json", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before and "convergence measure of the shifted" in out.stdout
    m = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["modes"]
    lam = np.array(m["lambda"])
    assert m["shift"] == sigma and m["converged"] == 1 and (np.array(m["rho"]) <= 1e-6).all()
    assert np.abs(lam[:6]).max() <= 2e-6 * sigma and (lam[6:] > 100 * 2e-6 * sigma).all(), lam
    assert m["frequency_hz"][:6] == [np.sqrt(l) / (2 * np.pi) if l > 0 else 0.0 for l in lam[:6]]
