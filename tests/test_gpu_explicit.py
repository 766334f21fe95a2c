"""Explicit dynamics on the device: the central-difference update kernel alone, in every template form,
against np.longdouble; every step of stan_hip_explicit as a central-difference step of the device's own state, on a fresh K and
on one a static solve has scaled; trajectories and energies against the restatement (tests/explicit_ref.py); the stable step
(stan_hip_stable_step) against the export's row sums, scipy's lambda_max and the restated power iteration; reproducibility, the
device-pointer entries, the error cases.

Kernel bounds (k 2^-53 sum |terms| against long double, k = the floating-point operations of the entry's expression, first
order; a contraction to a fused multiply-add only removes a rounding).  The coefficients dt2, two_dt, om, op reach the kernel as
doubles and enter the reference with those bits.
  u' = ((2 u - om u_p) + dt2 ((g F - Ku) / M)) / op    k = 8: g F 1, the difference 1, / M 1, dt2 x 1, om u_p 1, 2 u - 1 (2 u is
                                                       exact), the sum 1, / op 1; scaled form: Ku = y / s one more, k = 9
  u' / s                                               k + 1
  v  = (u' - u_p) / two_dt                             k = 2, of the device's own u'
  a  = ((u' - 2 u) + u_p) / dt2                        k = 3, of the device's own u'
  a0 = ((g F - Ku0) - alpha_R (M v0)) / M              k = 6, plus the product's own error
  u-1 = (u0 - dt v0) + (dt2 / 2) a0                    k = 4 (dt2 / 2 is exact), of the device's own a0
  energies: a term is 2 products, a sum of N terms adds N - 1 roundings, the factor one more: (N + 2) 2^-53 sum |terms|.
A row of the product is a sum of at most nnz_row terms a_ij x_j, each through the two scalings of S K S and back (the export's
two roundings, x / s, the final / s): (nnz_row + 4) 2^-53 sum_j |K_ij| |u_j|, the unit of tests/test_gpu_transient.py."""
import numpy as np
import pytest

from tests import device_buffers as DB
from tests import explicit_ref as X
from tests import modes_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
STEPS = 40
RATIOS = (0.5, 0.9, 0.99)      # dt / dt_crit, dt_crit = 2 / sqrt(lambda_max) from scipy.linalg.eigh


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assemble(ctx, j):
    return ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


def _raises(hip, fn, code):
    with pytest.raises(hip.StanHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, M, F, csr (full export of a fresh K), Kd, lam, Phi, lam_max, dt_crit, U_fresh): computed once, left
    unchanged."""
    made = {}

    def get(name):
        if name not in made:
            j = X.job(name)
            K = _assemble(gpu_ctx, j)
            M = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, X.mat_rho(name))[0]
            csr = K.to_csr(upper_only=False)
            info = K.info()
            Kd = R.dense(*csr)
            r = R.reference(name, Kd)
            lam_max, _ = X.top_pair(name, Kd, M)
            F = np.asarray(j.F, dtype=np.float64)
            U_fresh = K.cg_solve(F, 1e-8)
            K.free()
            made[name] = dict(job=j, M=M, F=F, csr=csr, info=info, Kd=Kd, lam=r["lam"], Phi=r["Phi"], lam_max=lam_max,
                              dt_crit=2.0 / np.sqrt(lam_max), U_fresh=U_fresh)
        return made[name]
    return get


@pytest.fixture(scope="module")
def matrices(gpu_ctx, models):
    """(name, scaled) -> K; scaled: a static solve has left S K S in place"""
    made = {}

    def get(name, scaled=False):
        if (name, scaled) not in made:
            K = _assemble(gpu_ctx, models(name)["job"])
            if scaled:
                K.cg_solve(models(name)["F"], 1e-8)
            assert K.info()["scaled"] == int(scaled)
            made[(name, scaled)] = K
        return made[(name, scaled)]
    yield get
    for K in made.values():
        K.free()


# ---- 1. the update kernel alone ----------------------------------------------------------------------------------------------
KERNEL_N = (1, 63, 64, 65, 255, 257, 4097, 200003)


def _vec(rng, N):
    return rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 6, N)


def _update_ref(c, g, y, s, u, up, M, F):
    """(Ku, u', its term sum) in long double from the kernel's own coefficients"""
    y, u, up, M, F = (x.astype(LD) for x in (y, u, up, M, F))
    dt2, om, op, g = LD(c["dt2"]), LD(c["om"]), LD(c["op"]), LD(g)
    ku = y if s is None else y / s.astype(LD)
    w = ((2 * u - om * up) + dt2 * ((g * F - ku) / M)) / op
    ws = ((2 * np.abs(u) + np.abs(om * up)) + dt2 * ((np.abs(g * F) + np.abs(ku)) / M)) / np.abs(op)
    return ku, w, ws


def _state_ref(c, w, u, up):
    w, u, up = (x.astype(LD) for x in (w, u, up))
    two_dt, dt2 = LD(c["two_dt"]), LD(c["dt2"])
    return (w - up) / two_dt, (np.abs(w) + np.abs(up)) / two_dt, ((w - 2 * u) + up) / dt2, (np.abs(w) + 2 * np.abs(u) + np.abs(up)) / dt2


def _energy_ref(g, ku, M, F, u, v):
    u, v, M, F = (x.astype(LD) for x in (u, v, M, F))
    terms = np.stack([LD(0.5) * M * v * v, LD(0.5) * u * ku, LD(g) * F * u])
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


@pytest.mark.parametrize("N", KERNEL_N)
def test_update_kernel_against_longdouble(gpu_ctx, N):
    """Every template form through stan_hip_central_update: plain / scaled x with and without the state x with and without the
    energies; alpha_R zero and not; the flag."""
    rng = np.random.default_rng(200 + N % 991)
    y, u, up, F = (_vec(rng, N) for _ in range(4))
    M = 10.0 ** rng.uniform(-6, 6, N)
    sc = 10.0 ** rng.uniform(-3, 3, N)
    dt, g = 3.7e-4, 0.625
    for alpha in (0.0, 0.8):
        c = X.coef(dt, alpha)
        for s in (None, sc):
            k = 8 if s is None else 9
            full = gpu_ctx.central_update(y, u, up, M, F, dt, alpha, g, step=7, s=s, state=True, energy=True)
            ku, wr, ws = _update_ref(c, g, y, s, u, up, M, F)
            w = full["u_next"]
            ew = (np.abs(w.astype(LD) - wr) / (k * U53 * ws)).max()
            eh = 0.0
            if s is not None:
                eh = (np.abs(full["u_next_scaled"].astype(LD) - wr / s.astype(LD)) / ((k + 1) * U53 * ws / s)).max()
            vr, vs, ar, as_ = _state_ref(c, w, u, up)
            ev = (np.abs(full["v"].astype(LD) - vr) / (2 * U53 * vs)).max()
            ea = (np.abs(full["a"].astype(LD) - ar) / (3 * U53 * as_)).max()
            er, ers = _energy_ref(g, ku, M, F, u, full["v"])
            ee = (np.abs(full["energy"].astype(LD) - er) / ((N + 2) * U53 * ers)).max()
            print("N=%d alpha=%g scaled=%d: u' %.3f u'/s %.3f v %.3f a %.3f energies %.3f of their bounds" %
                  (N, alpha, s is not None, ew, eh, ev, ea, ee))
            assert max(ew, eh, ev, ea, ee) <= 1.0, (N, alpha, float(ew), float(eh), float(ev), float(ea), float(ee))
            assert full["first_nonfinite"] == 0
            # the other forms: the same bits of what they share; twice: the same bits
            for state in (False, True):
                for energy in (False, True):
                    o = gpu_ctx.central_update(y, u, up, M, F, dt, alpha, g, step=7, s=s, state=state, energy=energy)
                    assert np.array_equal(_bits(o["u_next"]), _bits(w))
                    if s is not None:
                        assert np.array_equal(_bits(o["u_next_scaled"]), _bits(full["u_next_scaled"]))
                    if state:
                        assert np.array_equal(_bits(o["v"]), _bits(full["v"])) and np.array_equal(_bits(o["a"]), _bits(full["a"]))
                    if energy:
                        assert np.array_equal(_bits(o["energy"]), _bits(full["energy"]))
    # the flag: an overflow in 2 u - om u_p at one entry reports the step it is given, nothing else does
    ub, pb = u.copy(), up.copy()
    ub[N // 2], pb[N // 2] = 1.5e308, -1.5e308
    o = gpu_ctx.central_update(y, ub, pb, M, F, dt, 0.0, g, step=12345678901)
    assert o["first_nonfinite"] == 12345678901 and not np.isfinite(o["u_next"][N // 2])
    assert np.isfinite(np.delete(o["u_next"], N // 2)).all()


# ---- 2. every step of a run -----------------------------------------------------------------------------------------------------
def _alpha(m, damped):
    return 2.0 * 0.02 * np.sqrt(m["lam"][0]) if damped else 0.0


@pytest.mark.parametrize("scaled", (False, True), ids=("fresh", "scaled"))
@pytest.mark.parametrize("damped", (False, True), ids=("undamped", "mass_damped"))
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", X.MODELS)
def test_every_step_is_a_central_difference_step(gpu_ctx, models, matrices, name, ratio, damped, scaled):
    """snap_every = 1: u_{n+1} recomputed in long double from the device's own u_n, u_{n-1} (the product by csr_ld on the export)
    within the update's bound plus the product row's; v_n, a_n from the device's own u's within theirs; a_0 and, through u_{-1},
    u_1 likewise.  The start state is u0 = 0.3 phi_2, v0 = omega_1 phi_1 (so that every term of a_0 is there).  On a K that a
    static solve has scaled the loop runs the scaled form of the kernel: a wrong s would show here."""
    m, K = models(name), matrices(name, scaled)
    M, F = m["M"], m["F"]
    dt, al = ratio * m["dt_crit"], _alpha(m, damped)
    c = X.coef(dt, al)
    u0 = 0.3 * m["Phi"][:, 1] * np.abs(m["U_fresh"][0]).max() / np.abs(m["Phi"][:, 1]).max()
    v0 = np.sqrt(m["lam"][0]) * np.abs(u0).max() / np.abs(m["Phi"][:, 0]).max() * m["Phi"][:, 0]
    out = K.explicit(M, F, dt, STEPS, u0=u0, v0=v0, alpha_R=al, snap_every=1)
    rep, sn = out["report"], out["snaps"]
    assert rep["steps"] == STEPS and rep["first_nonfinite_step"] == 0 and K.info()["scaled"] == int(scaled)
    assert sn.shape == (STEPS + 1, 3, M.shape[0])
    assert np.array_equal(_bits(sn[0, 0]), _bits(u0)) and np.array_equal(_bits(sn[0, 1]), _bits(v0))
    for q, key in enumerate(("u", "v", "a")):
        assert np.array_equal(_bits(sn[STEPS, q]), _bits(out[key]))
    rowptr, col, val = m["csr"]
    Kmul, Kabs = X.csr_ld(rowptr, col, val), X.csr_ld(rowptr, col, np.abs(val))
    kp = (int(np.diff(rowptr).max()) + 4) * U53
    Ml, Fl = M.astype(LD), F.astype(LD)
    dt2, om, op = LD(c["dt2"]), LD(c["om"]), LD(c["op"])
    # a_0
    Ku0 = Kmul(u0)
    r0 = (Fl - Ku0) - LD(al) * (Ml * v0)
    r0s = np.abs(Fl) + np.abs(Ku0) + LD(al) * np.abs(Ml * v0)
    e0 = (np.abs(sn[0, 2].astype(LD) - r0 / Ml) / ((6 * U53 * r0s + kp * Kabs(np.abs(u0))) / Ml)).max()
    # u_{-1} from the device's own a_0, in long double, and its bound
    a0 = sn[0, 2].astype(LD)
    um = (u0.astype(LD) - LD(c["dt"]) * v0) + (dt2 / 2) * a0
    ums = 4 * U53 * (np.abs(u0) + LD(c["dt"]) * np.abs(v0) + (dt2 / 2) * np.abs(a0))
    worst_u = worst_v = worst_a = 0.0
    for n in range(STEPS):
        u, un = sn[n, 0], sn[n + 1, 0]
        up = um if n == 0 else sn[n - 1, 0].astype(LD)
        Ku = Kmul(u)
        w = ((2 * u.astype(LD) - om * up) + dt2 * ((Fl - Ku) / Ml)) / op
        ws = ((2 * np.abs(u) + np.abs(om * up)) + dt2 * ((np.abs(Fl) + np.abs(Ku)) / Ml)) / op
        bound = (8 + int(scaled)) * U53 * ws + dt2 * kp * Kabs(np.abs(u)) / Ml / op
        if n == 0:
            bound = bound + np.abs(om) * ums / op
        worst_u = max(worst_u, float((np.abs(un.astype(LD) - w) / bound).max()))
        if n >= 1:
            vr, vs, ar, as_ = _state_ref(c, un, u, sn[n - 1, 0])
            worst_v = max(worst_v, float((np.abs(sn[n, 1].astype(LD) - vr) / (2 * U53 * vs)).max()))
            worst_a = max(worst_a, float((np.abs(sn[n, 2].astype(LD) - ar) / (3 * U53 * as_)).max()))
    print("%s dt/dt_crit=%g damped=%d scaled=%d: a0 %.3f u' %.3f v %.3f a %.3f of their bounds" %
          (name, ratio, damped, scaled, e0, worst_u, worst_v, worst_a))
    assert e0 <= 1.0 and worst_u <= 1.0 and worst_v <= 1.0 and worst_a <= 1.0, (float(e0), worst_u, worst_v, worst_a)


# ---- 3. trajectories --------------------------------------------------------------------------------------------------------------
_yard = {}


def _yardstick(m, key, dt, F, kw):
    """(long-double run, yardstick of u, yardstick of the energies, scale of u, largest energy term): the fp64 restatement's
    largest deviation from the long-double restatement over the run -- of u in the M-norm relative to max_n ||u_n||_M, of the
    energies relative to the largest energy term.  Computed once and left unchanged."""
    if key not in _yard:
        M = m["M"]
        exact = X.central(X.csr_ld(*m["csr"]), M, F, dt, STEPS, ft=LD, **kw)
        plain = X.central(m["Kd"].__matmul__, M, F, dt, STEPS, **kw)
        scale = max(X.m_norm(x, M) for x in exact["U"])
        big = float(np.abs(exact["energy"]).max())
        dev = max(X.m_norm(plain["U"][n] - exact["U"][n], M) for n in range(STEPS + 1)) / scale
        dev_e = float(np.abs(plain["energy"] - exact["energy"]).max()) / big
        _yard[key] = (exact, float(dev), dev_e, float(scale), big)
    return _yard[key]


@pytest.mark.parametrize("case", ("step_load", "mass_damped", "free_vibration"))
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", ("cube6", "two_mat"))
def test_trajectory_against_the_restatement(gpu_ctx, models, matrices, name, ratio, case):
    """The snapshots, the end state and the energies against tests/explicit_ref.central in long double.  The yardstick is the fp64
    restatement's own largest deviation from that run; the device may lie 4 x that away (the project's margin for a device
    result against a restated yardstick)."""
    m, K = models(name), matrices(name)
    M = m["M"]
    dt = ratio * m["dt_crit"]
    F, kw = m["F"], {}
    if case == "mass_damped":
        kw["alpha_R"] = _alpha(m, True)
    if case == "free_vibration":
        F, kw = np.zeros_like(M), dict(u0=m["Phi"][:, 0].copy())
    exact, yard, yard_e, scale, big = _yardstick(m, (name, case, ratio), dt, F, kw)
    probe = np.array([0, M.shape[0] // 2, M.shape[0] - 1], dtype=np.int32)
    out = K.explicit(M, F, dt, STEPS, probe_dof=probe, snap_every=1, energy_every=1, **kw)
    dev = max(X.m_norm(out["snaps"][n, 0] - exact["U"][n], M) for n in range(STEPS + 1)) / scale
    end = X.m_norm(out["u"] - exact["U"][STEPS], M) / scale
    dev_e = float(np.abs(out["energy"] - exact["energy"]).max()) / big
    print("%s %s dt/dt_crit=%g: yardstick u %.3e, device %.3e (end state %.3e); yardstick energies %.3e, device %.3e" %
          (name, case, ratio, yard, dev, end, yard_e, dev_e))
    assert yard > 0 and dev <= 4 * yard and end <= 4 * yard, (yard, dev, end)
    assert np.array_equal(_bits(out["probe_u"]), _bits(out["snaps"][:, 0, probe]))
    assert yard_e > 0 and dev_e <= 4 * yard_e, (yard_e, dev_e)


# ---- 4. the stable step ---------------------------------------------------------------------------------------------------------
def _check_stable(ctx, name, m, K, n_power=30):
    """lambda_upper against the long-double row sums of the export and scipy's lambda_max; lambda_power below lambda_max"""
    M = m["M"]
    rowptr, col, val = m["csr"]
    up, pw, dts = K.stable_step(M, n_power)
    ref = X.lambda_upper(rowptr, col, val, M, LD)
    tol = (int(np.diff(rowptr).max()) + 2) * U53
    print("%s n_power=%d: lambda_upper / lambda_max %.4f, lambda_power / lambda_max %.6f" % (name, n_power, up / m["lam_max"], pw / m["lam_max"]))
    assert abs(LD(up) - ref) <= tol * ref, (name, up, float(ref))
    assert up >= m["lam_max"] and dts == 2.0 / np.sqrt(up)
    assert 0 < pw <= m["lam_max"] * (1 + 8 * np.finfo(float).eps)
    return up, pw


@pytest.mark.parametrize("name", X.MODELS)
def test_stable_step_brackets_lambda_max(gpu_ctx, models, matrices, name):
    import torch
    m = models(name)
    M = m["M"]
    K, Ks = matrices(name), matrices(name, True)
    up, pw = _check_stable(gpu_ctx, name, m, K)
    # twice, without the power iteration, from a device pointer one element past a 256-byte boundary: the same bits
    assert K.stable_step(M, 30) == (up, pw, 2.0 / np.sqrt(up))
    assert K.stable_step(M, 0) == (up, 0.0, 2.0 / np.sqrt(up))
    dM = DB.input_("M", M, DB.guard_len(M.shape[0]), torch.device("cuda:0"), offset=1)
    torch.cuda.synchronize()
    assert K.stable_step_dev(dM.ptr, 30) == (up, pw, 2.0 / np.sqrt(up))
    DB.check([dM])
    # the scaled K: the export's own expression, so within the row bound of the fresh one (and of the reference)
    ups, pws = _check_stable(gpu_ctx, name + " (scaled)", m, Ks)
    assert abs(ups - up) <= 2 * (int(np.diff(m["csr"][0]).max()) + 2) * U53 * up
    assert K.info() == m["info"] and Ks.info()["scaled"] == 1


@pytest.mark.parametrize("scaled", (False, True), ids=("fresh", "scaled"))
@pytest.mark.parametrize("name", X.MODELS)
def test_power_iteration_against_the_restatement(gpu_ctx, models, matrices, name, scaled):
    """lambda_power at n_power = 30 against tests/explicit_ref.lambda_power in long double; the yardstick is the fp64
    restatement's own deviation from that run, the device is allowed 4 x that.  The quantity is ONE double, and on cube6 the
    fp64 restatement lands on the double nearest to the long-double value (1.4e-17 away, an eighth of a unit in the last
    place), so 4 x the yardstick admits no other double there: the quotient's two sums are carried as pairs hi + lo
    (k_power_sums), which leaves the double nearest to what the vectors give, whatever order adds them.  Measured, relative
    deviations from the long-double run, yardstick / device (the same on the fresh and on the scaled K):
      cube6         1.38e-17 / 1.38e-17
      cube6j        1.58e-16 / 8.53e-18
      perforated12  1.44e-16 / 1.40e-17
      two_mat       1.15e-16 / 8.00e-17"""
    m, K = models(name), matrices(name, scaled)
    M = m["M"]
    rowptr, col, val = m["csr"]
    pw = K.stable_step(M, 30)[1]
    exact = X.lambda_power(X.csr_ld(rowptr, col, val), M, 30, LD)
    plain = X.lambda_power(m["Kd"].__matmul__, M, 30)
    yard, dev = abs(float((LD(plain) - exact) / exact)), abs(float((LD(pw) - exact) / exact))
    print("%s scaled=%d n_power=30: power iteration: yardstick %.3e, device %.3e (fp64 restatement %.17g, device %.17g)" %
          (name, scaled, yard, dev, plain, pw))
    assert yard > 0 and dev <= 4 * yard, (name, yard, dev)


@pytest.mark.parametrize("option", ("sell_sigma_32", "row_folding_1"))
def test_stable_step_under_the_layout_options(gpu_ctx, models, option):
    from stan_amd import hip
    opt, val, default = {"sell_sigma_32": (hip.OPT_SELL_SIGMA, 32, 1), "row_folding_1": (hip.OPT_ROW_FOLDING, 1, -1)}[option]
    m = models("perforated12")
    gpu_ctx.set_option(opt, val)
    try:
        K = _assemble(gpu_ctx, m["job"])
        try:
            _check_stable(gpu_ctx, "perforated12 " + option, m, K)
            K.cg_solve(m["F"], 1e-8)
            _check_stable(gpu_ctx, "perforated12 " + option + " (scaled)", m, K)
        finally:
            K.free()
    finally:
        gpu_ctx.set_option(opt, default)


# ---- 5. the contract --------------------------------------------------------------------------------------------------------------
def _no_ms(rep):
    return {k: v for k, v in rep.items() if not k.endswith("_ms")}


def test_same_bits_twice_and_from_the_device_entry(gpu_ctx, models, matrices):
    """Two calls give the same bits; the host and the _dev entry give the same bits, with the caller's buffers on and one element
    past a 256-byte boundary: nothing stored outside an output, every entry written, inputs unchanged; K's export, info and a
    later solve's bits are what they were."""
    import torch
    m = models("two_mat")
    K = _assemble(gpu_ctx, m["job"])
    try:
        M, F, N = m["M"], m["F"], m["M"].shape[0]
        dt, al = 0.9 * m["dt_crit"], _alpha(m, True)
        u0, v0 = 1e-3 * m["Phi"][:, 1], 0.1 * m["Phi"][:, 0]
        probe = np.array([1, N - 2, 17], dtype=np.int32)
        curve = [(0.0, 0.0), (4 * dt, 1.0), (9 * dt, 1.0), (9 * dt, 0.25)]
        kw = dict(u0=u0, v0=v0, alpha_R=al, curve=curve, probe_dof=probe, snap_every=3, energy_every=2, n_power=5)
        n_steps = 10
        a = K.explicit(M, F, dt, n_steps, **kw)
        b = K.explicit(M, F, dt, n_steps, **kw)
        keys = ("u", "v", "a", "probe_u", "snaps", "energy")
        for k in keys:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert a["snaps"].shape == (4, 3, N) and a["energy"].shape == (6, 3) and a["probe_u"].shape == (11, 3)
        assert _no_ms(a["report"]) == _no_ms(b["report"]) and a["report"]["steps"] == n_steps
        assert a["report"]["lambda_power"] > 0 and a["report"]["dt_stable"] == 2.0 / np.sqrt(a["report"]["lambda_upper"])
        assert (a["report"]["lambda_upper"], a["report"]["lambda_power"]) == K.stable_step(M, 5)[:2]
        assert np.array_equal(_bits(a["probe_u"][::3]), _bits(a["snaps"][:, 0, probe]))
        assert a["energy"][0, 2] == 0.0 and a["energy"][-1, 2] != 0.0          # g(0) = 0
        # the energies every step are the same numbers where both record
        every = K.explicit(M, F, dt, n_steps, **dict(kw, energy_every=1))
        assert np.array_equal(_bits(every["energy"][::2]), _bits(a["energy"])) and np.array_equal(_bits(every["u"]), _bits(a["u"]))
        dev = torch.device("cuda:0")
        for offset in (0, 1):
            g = DB.guard_len(N)
            ins = [DB.input_(n, x, g, dev, offset) for n, x in (("M", M), ("F", F), ("u0", u0), ("v0", v0))]
            dp = DB.input_("probe", probe, g, dev, offset)
            outs = [DB.output("u_end", N, g, dev, offset), DB.output("v_end", N, g, dev, offset), DB.output("a_end", N, g, dev, offset),
                    DB.output("probe_u", (n_steps + 1) * 3, g, dev, offset), DB.output("snaps", 4 * 3 * N, g, dev, offset),
                    DB.output("energy", 6 * 3, g, dev, offset)]
            torch.cuda.synchronize()
            rep = K.explicit_dev(ins[0].ptr, ins[1].ptr, dt, n_steps, outs[0].ptr, outs[1].ptr, outs[2].ptr, d_u0=ins[2].ptr,
                                 d_v0=ins[3].ptr, alpha_R=al, curve=curve, n_probe=3, d_probe_dof=dp.ptr, d_probe_u=outs[3].ptr,
                                 snap_every=3, d_snaps=outs[4].ptr, energy_every=2, d_energy=outs[5].ptr, n_power=5)
            DB.check(ins + [dp] + outs)
            for o, k in zip(outs, keys):
                assert np.array_equal(_bits(o.numpy()), _bits(a[k]).reshape(-1)), (offset, k)
            assert _no_ms(rep) == _no_ms(a["report"])
        # K is read only: export, info and a later solve's bits are those of a fresh assembly
        again = K.to_csr(upper_only=False)
        assert all(np.array_equal(x, y) for x, y in zip(again, m["csr"])) and K.info() == m["info"]
        U, r = K.cg_solve(F, 1e-8)
        assert np.array_equal(_bits(U), _bits(m["U_fresh"][0])) and r == m["U_fresh"][1]
    finally:
        K.free()


def test_no_steps_returns_the_start_state_and_a0(gpu_ctx, models, matrices):
    m, K = models("cube6"), matrices("cube6")
    M, F = m["M"], m["F"]
    dt = 0.9 * m["dt_crit"]
    u0, v0 = 1e-3 * m["Phi"][:, 0], 0.2 * m["Phi"][:, 1]
    out = K.explicit(M, F, dt, 0, u0=u0, v0=v0, probe_dof=[3], snap_every=2, energy_every=5)
    assert out["report"]["steps"] == 0
    assert np.array_equal(_bits(out["u"]), _bits(u0)) and np.array_equal(_bits(out["v"]), _bits(v0))
    want = (F - m["Kd"] @ u0) / M
    assert np.abs(out["a"] - want).max() <= 1e-12 * np.abs(want).max()
    assert out["probe_u"].shape == (1, 1) and out["probe_u"][0, 0] == u0[3]
    assert out["snaps"].shape == (1, 3, M.shape[0]) and np.array_equal(_bits(out["snaps"][0, 2]), _bits(out["a"]))
    assert out["energy"].shape == (1, 3) and abs(out["energy"][0, 0] - 0.5 * (M * v0 * v0).sum()) <= 1e-9 * 0.5 * (M * v0 * v0).sum()
    # without u0 no product is made: a_0 = F / M to the bit
    out = K.explicit(M, F, dt, 0)
    assert np.array_equal(_bits(out["a"]), _bits(F / M)) and not out["u"].any() and not out["v"].any()


def _sentinel_outputs(N, n_steps, n_probe):
    return dict(u=np.full(N, -7.25), v=np.full(N, -7.25), a=np.full(N, -7.25), probe_u=np.full((n_steps + 1, n_probe), -7.25),
                snaps=np.full((n_steps + 1, 3, N), -7.25), energy=np.full((n_steps + 1, 3), -7.25))


def _untouched(o):
    return all((x == -7.25).all() for x in o.values())


@pytest.mark.parametrize("name", ("cube6", "two_mat"))
def test_a_step_above_the_proven_limit_is_refused(gpu_ctx, models, matrices, name):
    """dt = 1.05 dt_crit with n_power = 30: lambda_power already exceeds lambda_max / 1.05^2 (tests/test_explicit.py), so the call
    is STAN_E_ARG, names both numbers and leaves the outputs alone; the same dt without the power iteration runs."""
    from stan_amd import hip
    m, K = models(name), matrices(name)
    M, F, N = m["M"], m["F"], m["M"].shape[0]
    dt = 1.05 * m["dt_crit"]
    o = _sentinel_outputs(N, 5, 1)
    with pytest.raises(hip.StanHipError) as ei:
        K.explicit(M, F, dt, 5, probe_dof=[0], snap_every=1, energy_every=1, n_power=30, out=o)
    msg, rep = str(ei.value), ei.value.report
    assert ei.value.code == hip.E_ARG and "unstable" in msg and "%.17g" % dt in msg and "%.17g" % (2.0 / np.sqrt(rep["lambda_power"])) in msg
    assert _untouched(o) and rep["steps"] == 0 and rep["lambda_power"] > m["lam_max"] / 1.05 ** 2
    assert K.explicit(M, F, dt, 5)["report"]["steps"] == 5
    assert K.explicit(M, F, 0.9 * rep["dt_stable"], 5, n_power=30)["report"]["steps"] == 5


def test_an_overflow_ends_the_run_with_the_step(gpu_ctx, models, matrices):
    """A load of 1e300: an arithmetic overflow the flag reports, nothing more."""
    from stan_amd import hip
    m, K = models("cube6"), matrices("cube6")
    M, N = m["M"], m["M"].shape[0]
    o = _sentinel_outputs(N, 20, 1)
    with pytest.raises(hip.StanHipError) as ei:
        K.explicit(M, 1e300 * m["F"], 0.9 * m["dt_crit"], 20, probe_dof=[0], snap_every=1, energy_every=1, out=o)
    rep = ei.value.report
    assert ei.value.code == hip.E_UNSUPPORTED and rep["first_nonfinite_step"] >= 1
    assert "step %d" % rep["first_nonfinite_step"] in str(ei.value) and "not finite" in str(ei.value)
    assert _untouched(o)
    # without snapshots the flag is read at the end: the same step
    with pytest.raises(hip.StanHipError) as ei2:
        K.explicit(M, 1e300 * m["F"], 0.9 * m["dt_crit"], 20)
    assert ei2.value.code == hip.E_UNSUPPORTED and ei2.value.report["first_nonfinite_step"] == rep["first_nonfinite_step"]
    assert ei2.value.report["steps"] == 20 and rep["steps"] < 20


def test_explicit_error_cases(gpu_ctx, models, matrices):
    import torch
    from stan_amd import hip
    m, K = models("cube6"), matrices("cube6")
    M, F, N = m["M"], m["F"], m["M"].shape[0]
    dt = 0.9 * m["dt_crit"]
    bad_M = M.copy(); bad_M[3] = 0.0
    cases = dict(
        dt_zero=dict(dt=0.0), dt_negative=dict(dt=-1.0), dt_nan=dict(dt=float("nan")), steps=dict(n_steps=-1),
        alpha=dict(alpha_R=-1.0), alpha_nan=dict(alpha_R=float("nan")), power=dict(n_power=-1),
        curve_descends=dict(curve=[(0.0, 1.0), (2.0, 1.0), (1.0, 0.0)]), curve_nan=dict(curve=[(0.0, float("nan"))]),
        curve_inf=dict(curve=[(float("inf"), 1.0)]), probe_high=dict(probe_dof=[0, N]), probe_low=dict(probe_dof=[-1]), mass=dict(M=bad_M))
    for name, kw in cases.items():
        args = dict(M=M, F=F, dt=dt, n_steps=2)
        args.update(kw)
        with pytest.raises(hip.StanHipError) as ei:
            K.explicit(args.pop("M"), args.pop("F"), args.pop("dt"), args.pop("n_steps"), **args)
        assert ei.value.code == hip.E_ARG, (name, str(ei.value))
    assert "M[3]" in _raises(hip, lambda: K.stable_step(bad_M), hip.E_ARG)
    _raises(hip, lambda: K.stable_step(M, -1), hip.E_ARG)
    # NULL where an array is required, negative counts; nothing is written through the outputs on an error (device entry, guarded)
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    dM, dF, dbad = DB.input_("M", M, g, dev), DB.input_("F", F, g, dev), DB.input_("M", bad_M, g, dev)
    dp = DB.input_("probe", np.array([0, N], dtype=np.int32), g, dev)
    outs = [DB.output(n, N, g, dev) for n in ("u_end", "v_end", "a_end")] + [DB.output("probe_u", 6, g, dev), DB.output("energy", 9, g, dev)]
    torch.cuda.synchronize()
    o = [x.ptr for x in outs]
    for call in (lambda: K.explicit_dev(None, dF.ptr, dt, 2, o[0], o[1], o[2]),
                 lambda: K.explicit_dev(dM.ptr, None, dt, 2, o[0], o[1], o[2]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, None, o[1], o[2]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], None),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=2, d_probe_dof=dp.ptr),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=-1, d_probe_dof=dp.ptr, d_probe_u=o[3]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], n_probe=2, d_probe_dof=dp.ptr, d_probe_u=o[3]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], snap_every=-1),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], energy_every=-1, d_energy=o[4]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, dt, 2, o[0], o[1], o[2], energy_every=1),
                 lambda: K.explicit_dev(dbad.ptr, dF.ptr, dt, 2, o[0], o[1], o[2]),
                 lambda: K.explicit_dev(dM.ptr, dF.ptr, 1.05 * m["dt_crit"], 2, o[0], o[1], o[2], n_power=30)):
        with pytest.raises(hip.StanHipError) as ei:
            call()
        assert ei.value.code == hip.E_ARG, str(ei.value)
    DB.check([dM, dF, dbad, dp] + outs, written=False)
    for x in outs:
        assert bool((x.payload.view(torch.int64) == DB.UNWRITTEN_BITS).all()), x.name
    # a K of another context; the update helper's own checks
    other = hip.Context(0)
    try:
        rep = hip.ExplicitReport()
        Mp, Fp = (x.ctypes.data_as(hip.C.POINTER(hip.C.c_double)) for x in (M, F))
        e = np.zeros(N)
        ep = e.ctypes.data_as(hip.C.POINTER(hip.C.c_double))
        rc = gpu_ctx.lib.stan_hip_explicit(other.h, K.k, Mp, Fp, None, None, hip.C.c_double(dt), hip.C.c_int32(1), hip.C.c_double(0.0),
                                           hip.C.c_int32(0), None, None, hip.C.c_int32(0), None, None, hip.C.c_int32(0), None,
                                           hip.C.c_int32(0), None, ep, ep, ep, hip.C.c_int32(0), hip.C.byref(rep))
        assert rc == hip.E_ARG and not e.any()
    finally:
        other.close()
    one = np.ones(5)
    lib, dp_ = gpu_ctx.lib, lambda x: x.ctypes.data_as(hip.C.POINTER(hip.C.c_double))
    out5 = np.zeros(5)
    assert lib.stan_hip_central_update(gpu_ctx.h, hip.C.c_int64(5), dp_(one), None, dp_(one), dp_(one), dp_(one), dp_(one),
                                       hip.C.c_double(1.0), hip.C.c_double(0.0), hip.C.c_double(1.0), hip.C.c_int64(1), dp_(out5), None,
                                       dp_(out5), None, None, None) == hip.E_ARG       # v without a
    assert lib.stan_hip_central_update(gpu_ctx.h, hip.C.c_int64(5), dp_(one), dp_(one), dp_(one), dp_(one), dp_(one), dp_(one),
                                       hip.C.c_double(1.0), hip.C.c_double(0.0), hip.C.c_double(1.0), hip.C.c_int64(1), dp_(out5), None,
                                       None, None, None, None) == hip.E_ARG            # s without u_next_scaled
    assert not out5.any()


def test_explicit_is_refused_on_a_communicator(gpu_ctx, models):
    from stan_amd import hip
    m = models("cube6")
    c = hip.Context(0)
    try:
        c.comm_init(0, 2, None)              # a detached rank of two
        K = _assemble(c, m["job"])
        try:
            assert "communicator" in _raises(hip, lambda: K.explicit(m["M"], m["F"], 1e-8, 1), hip.E_UNSUPPORTED)
            assert "communicator" in _raises(hip, lambda: K.stable_step(m["M"]), hip.E_UNSUPPORTED)
        finally:
            K.free()
    finally:
        c.close()
    multi = hip.Context(devices=[0])         # a multi-device handle (one device, no communicator)
    try:
        j = m["job"]
        Km = multi.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        assert "multi-device" in _raises(hip, lambda: Km.explicit(m["M"], m["F"], 1e-8, 1), hip.E_UNSUPPORTED)
        assert "multi-device" in _raises(hip, lambda: Km.stable_step(m["M"]), hip.E_UNSUPPORTED)
        one = np.ones(8)
        _raises(hip, lambda: multi.central_update(one, one, one, one, one, 1.0), hip.E_UNSUPPORTED)
        Km.free()
    finally:
        multi.close()


# ---- 6. console -----------------------------------------------------------------------------------------------------------------
def test_console_explicit(tmp_path, built_libs, gpu_ctx):
    """stan_solver --explicit --dt auto on the 4^3 cube of tests/test_gpu_transient.py: the "explicit" JSON object (dt = 0.9
    dt_stable, the probe history with the bits of the library call on the same model), the block, the .vtu arrays, the input
    file byte-identical afterwards, and every refusal."""
    import json
    import os
    import re
    import subprocess
    from stan_amd import problem
    from tests.test_gpu_transient import _console_db
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "t.STdb"), str(tmp_path / "out")
    n_nodes, tip = _console_db(path)
    before = open(path, "rb").read()
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True, timeout=300)
    # the library's own numbers on the same model
    j = problem.cube_job(4)
    K = _assemble(gpu_ctx, j)
    try:
        M = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, np.array([R.RHO]))[0]
        up, _, dts = K.stable_step(M, 0)
        dt = 0.9 * dts
        dofs = np.asarray(j.node_dof).reshape(-1, 3)[tip - 1]
        red = np.asarray(j.red)
        assert (red[dofs] != -1).all()
        curve = [(0.0, 0.0), (3 * dt, 1.0)]
        lib = K.explicit(M, np.asarray(j.F, dtype=np.float64), dt, 12, alpha_R=10.0, curve=curve, probe_dof=dofs - red[dofs],
                         energy_every=12, n_power=30)
    finally:
        K.free()
    args = ["--explicit", "--dt", "auto", "--steps", "12", "--rayleigh", "10,0", "--load-curve", "0,0,%r,1" % float(3 * dt),
            "--probe-node", str(tip), "--json", "--vtu", prefix, "--vtu-every", "4"]
    out = run(*(args + [path]))
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    assert "Explicit:" in out.stdout and "dt_stable" in out.stdout and "lambda_upper" in out.stdout and "Final energies:" in out.stdout
    t = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["explicit"]
    assert t["steps"] == 12 and t["dt_auto"] == 1 and t["dt_scale"] == 0.9 and t["alpha_R"] == 10.0 and t["first_nonfinite_step"] == 0
    assert t["dt"] == 0.9 * t["dt_stable"] and t["dt_stable"] == 2.0 / np.sqrt(t["lambda_upper"])
    assert (t["lambda_upper"], t["dt_stable"], t["dt"]) == (up, dts, dt) and t["lambda_power"] == lib["report"]["lambda_power"]
    assert 0 < t["lambda_power"] <= t["lambda_upper"] and t["n_power"] == 30
    assert abs(t["total_mass"] - R.RHO * 64.0) <= 64 * U53 * R.RHO * 64.0
    pu = np.array(t["probe_u"])
    assert t["probe_node"] == tip and t["probe_direction"] == [0, 1, 2] and pu.shape == (13, 3)
    assert np.array_equal(_bits(pu), _bits(lib["probe_u"])), "the console's probe history has the library call's bits"
    assert np.array_equal(_bits(np.array(t["energy_final"])), _bits(lib["energy"][-1]))
    assert not pu[0].any() and pu[-1, 2] > 0
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Probe node")[1], flags=re.M)[:13]
    assert [int(r[0]) for r in rows] == list(range(13))
    assert np.allclose([[float(x) for x in r[2:]] for r in rows], pu, rtol=1e-8, atol=0)
    for s in (0, 4, 8, 12):
        text = open("%s_step_%04d.vtu" % (prefix, s), "rb").read()
        for q in ("Displacement", "Velocity", "Acceleration"):
            for ax in "XYZ":
                assert ('Name="%s %s"' % (q, ax)).encode() in text, (s, q, ax)
        assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    assert sorted(os.listdir(str(tmp_path))) == ["out_step_0000.vtu", "out_step_0004.vtu", "out_step_0008.vtu", "out_step_0012.vtu", "t.STdb"]
    # --dt-scale, and a given dt; a dt the power iteration proves unstable is the library's refusal (exit code 1)
    out = run("--explicit", "--dt", "auto", "--dt-scale", "0.5", "--steps", "2", "--json", path)
    assert out.returncode == 0, out.stdout + out.stderr
    t2 = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["explicit"]
    assert t2["dt"] == 0.5 * dts and t2["dt_scale"] == 0.5
    out = run("--explicit", "--dt", repr(float(dt)), "--steps", "2", "--json", path)
    assert out.returncode == 0 and json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])["explicit"]["dt_auto"] == 0
    out = run("--explicit", "--dt", repr(float(3 * dts)), "--steps", "2", path)
    assert out.returncode == 1 and "unstable" in out.stderr
    # the refusals before anything runs (exit code 2, argv alone) ...
    base = ["--explicit", "--dt", "auto", "--steps", "2"]
    for extra, word in ((["--rayleigh", "1,1e-7"], "beta_R"), (["--transient"], "one per run"), (["--modes", "2"], "one per run"),
                        (["--buckling", "2"], "one per run"), (["--devices", "0,0"], "one device"), (["--dt-scale", "0"], "--dt-scale"),
                        (["--newmark", "0.25,0.5"], "--transient"), (["--solve-eps", "1e-8"], "--transient"), (["--dt", "1e-7"], "one per run")):
        out = run(*(base + extra + [path]))
        assert out.returncode == 2 and word in out.stderr and "STAN" not in out.stdout, (extra, out.stderr)
    out = run("--explicit", "--steps", "2", path)
    assert out.returncode == 2 and "--dt auto" in out.stderr
    for alone in (["--dt", "auto"], ["--dt-scale", "0.5"]):
        out = run(*(alone + [path]))
        assert out.returncode == 2 and "belong to --explicit" in out.stderr
    out = run("--help")
    assert out.returncode == 0 and "--dt-scale S  default 0.9: the usual convention of explicit codes, not a measured value" in out.stdout
    # ... and those of the file: no "Density", a non-zero "Displacement", an unknown probe node; the files stay as they were
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
    out = run(*(base + ["--probe-node", "9999", path]))
    assert out.returncode == 2 and "no such node" in out.stderr
    assert open(path, "rb").read() == before
