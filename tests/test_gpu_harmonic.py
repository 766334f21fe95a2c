"""The frequency response on the GPU (stan_hip_harmonic).

  1. the kernels on synthetic arrays against the long-double restatement (tests/harmonic_ref.py), by operation count:
       p_j        within N u sum |phi F|
       r_d        within (k + 2) u (|u_s| + sum |phi p / lambda|), p the device's own; r is read off the device as the response
                  at w = 1e76, undamped: there |a_jf| = |p_j| / w^2 is 152 orders below r, every fma(phi, a, r) returns r
       re, im     within (k + 10) u (|r_d| + sum_j |phi_jd| |p_j| |H_j|), p and r the device's own; the 10 covers the table's
                  roundings (c: 3, d: 1, e: 1, D: 2, the quotient: 1, the product with p: 1, rounded up)
       peak_idx   an index whose long-double amplitude from the device's own snapshots is within 4 ulp of the largest
       peak       within 2 ulp of that amplitude (amp2 two roundings, the root one)
     u = 2^-53, one ulp = 2 u relative;
  2. end to end on cube6j and two_mat with the device's own modes and static solution: the device against the dense complex
     solve stays within 4 x the deviation of the float64 restatement fed the same modes and u_static;
  3. the contract: the same bits twice, from the _dev entry inside guards, on the caller's stream; the error cases with the
     outputs untouched; the refusals;
  4. the console."""
import numpy as np
import pytest

from tests import device_buffers as DB
from tests import harmonic_ref as H
from tests import modes_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
U53 = 2.0 ** -53
ULP = 2.0 ** -52
FAR = 1e76   # the frequency at which the response is r to the bit


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _raises(hip, fn, code):
    with pytest.raises(hip.StanHipError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def _assemble(ctx, j):
    return ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


# ---- 1. the kernels on synthetic arrays ---------------------------------------------------------------------------------------
# a covering subset of N x n_modes x n_freq: every value of the three lists, every table width (4 .. 32: the mode count rounded up
# to a multiple of 4), the full trips of 4 (1 beyond 24 modes) frequencies with every remainder, one row, one more and one less than
# a wave and than a workgroup, more than one workgroup of the projection (1024 rows)
SHAPES = ((1, 1, 1), (63, 2, 3), (64, 7, 4), (65, 8, 5), (255, 9, 64), (256, 24, 65), (257, 32, 1), (1000, 1, 65), (4097, 24, 5),
          (4097, 32, 65), (1000, 9, 3), (255, 2, 4), (64, 32, 3), (65, 7, 64), (256, 8, 1), (257, 13, 5), (63, 17, 4), (1000, 25, 65),
          (1000, 28, 3), (4097, 20, 64))


def _synthetic(N, k, nf, damping, seed=0):
    rng = np.random.default_rng(1000 * N + 10 * k + nf + seed)
    phi, F, us = rng.standard_normal((k, N)), rng.standard_normal(N), rng.standard_normal(N)
    lam = np.sort(rng.uniform(1.0, 400.0, k))
    omega = np.linspace(0.0, 1.3 * np.sqrt(lam[-1]), nf) if nf > 1 else np.array([0.7 * np.sqrt(lam[0])])
    kw = dict(alpha_R=0.3, beta_R=1e-3) if damping == "rayleigh" else dict(zeta=rng.uniform(0.01, 0.05, k))
    probe = np.unique(np.concatenate([[0, N - 1], rng.integers(0, N, 5)])).astype(np.int32)
    return phi, F, us, lam, omega, kw, probe


def _device_r(ctx, lam, phi, F, us):
    out = ctx.harmonic(lam, phi, F, [FAR], u_static=us, snap_freq=[0], peak=False)
    return out["snaps"][0, 0], out["p"]


@pytest.mark.parametrize("damping", ("rayleigh", "modal"))
@pytest.mark.parametrize("N,k,nf", SHAPES)
def test_kernels_against_longdouble(gpu_ctx, N, k, nf, damping):
    phi, F, us, lam, omega, kw, probe = _synthetic(N, k, nf, damping)
    out = gpu_ctx.harmonic(lam, phi, F, omega, u_static=us, probe_dof=probe, snap_freq=np.arange(nf), **kw)
    p, snaps, pr, peak, at = out["p"], out["snaps"], out["probe"], out["peak"], out["peak_idx"]
    # p
    p_ld, _ = H.project(phi, F, lam, None, LD)
    p_bound = N * U53 * np.abs(phi * F[None, :]).sum(axis=1)
    assert (np.abs(p.astype(LD) - p_ld) <= p_bound).all(), np.abs(p.astype(LD) - p_ld) / p_bound
    # r, with the device's own p
    r_dev, p_far = _device_r(gpu_ctx, lam, phi, F, us)
    assert np.array_equal(_bits(p_far), _bits(p))
    c_ld = p.astype(LD) / lam.astype(LD)
    r_ld = us.astype(LD) - (phi.astype(LD) * c_ld[:, None]).sum(axis=0)
    r_bound = (k + 2) * U53 * (np.abs(us) + (np.abs(phi) * np.abs(c_ld.astype(np.float64))[:, None]).sum(axis=0))
    assert (np.abs(r_dev.astype(LD) - r_ld) <= r_bound).all(), (np.abs(r_dev.astype(LD) - r_ld) / r_bound).max()
    # every snapshot and probe component, with the device's own p and r
    a, b = H.table(p, lam, omega, ft=LD, **kw)
    re, im = H.response(phi, r_dev, a, b)
    g, h = H.transfer(lam, omega, ft=LD, **kw)
    absH = np.sqrt(g * g + h * h).astype(np.float64)                                     # [nf, k]
    x_bound = (k + 10) * U53 * (np.abs(r_dev)[None, :] + (absH * np.abs(p)[None, :]) @ np.abs(phi))
    for got, want, name in ((snaps[:, 0], re, "re"), (snaps[:, 1], im, "im")):
        err = np.abs(got.astype(LD) - want)
        assert (err <= x_bound).all(), (name, float((err / x_bound).max()))
    # the snapshots of all frequencies carry the bits of the probes at the same DOFs
    assert pr.shape == (nf, probe.shape[0], 2)
    assert np.array_equal(_bits(snaps[:, 0][:, probe]), _bits(pr[:, :, 0])) and np.array_equal(_bits(snaps[:, 1][:, probe]), _bits(pr[:, :, 1]))
    # peak_idx and peak, from the device's own snapshots
    amp = np.sqrt(snaps[:, 0].astype(LD) ** 2 + snaps[:, 1].astype(LD) ** 2)
    rows = np.arange(N)
    assert ((at >= 0) & (at < nf)).all()
    assert (amp[at, rows] >= amp.max(axis=0) * (1 - 4 * ULP)).all()
    assert (np.abs(peak.astype(LD) - amp[at, rows]) <= 2 * ULP * amp[at, rows]).all()
    rep = out["report"]
    assert rep["n_modes"] == k and rep["n_freq"] == nf and rep["static_correction"] == 1
    assert rep["peak"] == peak.max() and rep["peak_dof"] == int(np.argmax(peak)) and rep["peak_freq"] == at[rep["peak_dof"]]


def test_the_lowest_index_wins_an_exact_tie(gpu_ctx):
    """Frequencies 1 and 3 (and 0 and 4) are equal: their responses are the same bits, so indices 3 and 4 never win."""
    N, k = 1000, 9
    phi, F, us, lam, _, kw, _ = _synthetic(N, k, 5, "modal")
    w = np.sqrt(lam[0]) * 1.01
    omega = np.array([0.3 * w, w, 2.0 * w, w, 0.3 * w, 5.0 * w])
    out = gpu_ctx.harmonic(lam, phi, F, omega, u_static=us, snap_freq=np.arange(6), **kw)
    assert np.array_equal(_bits(out["snaps"][1]), _bits(out["snaps"][3])) and np.array_equal(_bits(out["snaps"][0]), _bits(out["snaps"][4]))
    at = out["peak_idx"]
    assert (at != 3).all() and (at != 4).all() and (at == 1).sum() > N // 2


def test_a_load_that_is_not_a_number_leaves_no_peak_row(gpu_ctx):
    """phi and F are not checked for finite entries: a NaN in F makes every p_j, so every response, NaN; no entry of peak compares
    larger than another, and the report says so (-1, -1, NaN) instead of naming a row."""
    phi, F, us, lam, omega, kw, _ = _synthetic(300, 3, 4, "modal")
    F[7] = float("nan")
    out = gpu_ctx.harmonic(lam, phi, F, omega, u_static=us, **kw)
    rep = out["report"]
    assert np.isnan(out["peak"]).all() and rep["peak_dof"] == -1 and rep["peak_freq"] == -1 and np.isnan(rep["peak"])


@pytest.mark.parametrize("N,k,nf", ((257, 9, 5), (1000, 24, 4)))
def test_no_static_solution_equals_the_modal_static_solution(gpu_ctx, N, k, nf):
    """u_static = NULL is r = 0; u_static = Phi (p / lambda) leaves an r within its bound of 0, and the responses differ by no more
    than that r and the roundings of two sums of k terms that start from different values."""
    phi, F, _, lam, omega, kw, _ = _synthetic(N, k, nf, "rayleigh")
    none = gpu_ctx.harmonic(lam, phi, F, omega, snap_freq=np.arange(nf), **kw)
    assert none["report"]["static_correction"] == 0
    c = none["p"] / lam
    us = (phi * c[:, None]).sum(axis=0)
    full = gpu_ctx.harmonic(lam, phi, F, omega, u_static=us, snap_freq=np.arange(nf), **kw)
    assert np.array_equal(_bits(full["p"]), _bits(none["p"]))
    r_bound = (k + 2) * U53 * (np.abs(us) + (np.abs(phi) * np.abs(c)[:, None]).sum(axis=0))
    g, h = H.transfer(lam, omega, ft=LD, **kw)
    S = (np.sqrt(g * g + h * h).astype(np.float64) * np.abs(none["p"])[None, :]) @ np.abs(phi)
    tol = r_bound[None, :] + 2 * (k + 10) * U53 * (r_bound[None, :] + S)
    for c_ in (0, 1):
        assert (np.abs(full["snaps"][:, c_] - none["snaps"][:, c_]) <= tol).all()
    assert np.array_equal(_bits(full["snaps"][:, 1]), _bits(none["snaps"][:, 1]))   # the imaginary part does not see r


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------
K_MODES = 6


@pytest.fixture(scope="module")
def models(gpu_ctx):
    """name -> dict(job, M, F, Kd, lam, phi (stan_hip_modes, K_MODES), U (stan_hip_cg_solve)): computed once, left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            j = H.job(name)
            K = _assemble(gpu_ctx, j)
            try:
                M = gpu_ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, H.mat_rho(name))[0]
                Kd = R.dense(*K.to_csr(upper_only=False))
                F = np.asarray(j.F, dtype=np.float64)
                lam, phi, _, rep = K.modes(M, K_MODES, tol=1e-9)
                assert rep["converged"] == 1
                U = K.cg_solve(F, 1e-13)[0]
            finally:
                K.free()
            made[name] = dict(job=j, M=M, F=F, Kd=Kd, lam=lam, phi=phi, U=U)
        return made[name]
    return get


def _sweep_frequencies(lam):
    w1, w2 = np.sqrt(lam[0]), np.sqrt(lam[1])
    return np.array([0.0, 0.5 * w1, 0.5 * (w1 + w2), 1.02 * w1])


def _against_direct(ctx, Kd, Mref, F, lam, phi, U, label):
    omega = _sweep_frequencies(lam)
    w1 = np.sqrt(lam[0])
    al, be = 0.02 * w1, 0.02 / w1
    out = ctx.harmonic(lam, phi, F, omega, u_static=U, alpha_R=al, beta_R=be, snap_freq=np.arange(4), peak=False)
    re64, im64 = H.modal_sum(phi, lam, F, omega, al, be, None, U, ft=np.float64)
    for f, w in enumerate(omega):
        x = H.direct(Kd, Mref, F, w, al, be)
        scale = np.abs(x).max()
        yard = np.abs((re64[f] + 1j * im64[f]) - x).max() / scale
        dev = np.abs((out["snaps"][f, 0] + 1j * out["snaps"][f, 1]) - x).max() / scale
        print("%s w = %.6e: restatement %.3e, device %.3e" % (label, w, yard, dev))
        assert dev <= 4 * yard, (label, f, dev, yard)


@pytest.mark.parametrize("name", ("cube6j", "two_mat"))
def test_response_against_the_direct_solve(gpu_ctx, models, name):
    m = models(name)
    _against_direct(gpu_ctx, m["Kd"], m["M"], m["F"], m["lam"], m["phi"], m["U"], name)


def test_response_with_the_pencils_modes(gpu_ctx, models):
    """The modes of stan_hip_modes_pencil on the consistent mass: Phi^T M_c Phi = I, the same entry."""
    m = models("cube6j")
    j = m["job"]
    K = _assemble(gpu_ctx, j)
    try:
        Mc = K.consistent_mass(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, H.mat_rho("cube6j"))
        try:
            Md = R.dense(*Mc.to_csr(upper_only=False))
            lam, phi, _, rep = gpu_ctx.modes_pencil(K, Mc, K_MODES, tol=1e-9)
            assert rep["converged"] == 1
        finally:
            Mc.free()
    finally:
        K.free()
    _against_direct(gpu_ctx, m["Kd"], Md, m["F"], lam, phi, m["U"], "cube6j consistent")


# ---- 3. the contract ----------------------------------------------------------------------------------------------------------
def _no_ms(rep):
    return {k: v for k, v in rep.items() if not k.endswith("_ms")}


KEYS = ("p", "probe", "snaps", "peak", "peak_idx")


def _same(a, b):
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.tobytes() == y.tobytes(), key


def test_same_bits_twice_and_from_the_device_entry(gpu_ctx, models):
    import torch
    m = models("two_mat")
    lam, phi, F, U = m["lam"], m["phi"], m["F"], m["U"]
    k, N = phi.shape
    omega = np.linspace(0.0, 1.5 * np.sqrt(lam[-1]), 11)
    zeta = np.linspace(0.01, 0.03, k)
    probe, snap = np.array([1, N - 2, 17], dtype=np.int32), np.array([0, 5, 10, 5], dtype=np.int32)
    kw = dict(u_static=U, alpha_R=0.5, beta_R=1e-9, zeta=zeta, probe_dof=probe, snap_freq=snap)
    a = gpu_ctx.harmonic(lam, phi, F, omega, **kw)
    b = gpu_ctx.harmonic(lam, phi, F, omega, **kw)
    _same(a, b)
    assert _no_ms(a["report"]) == _no_ms(b["report"])
    assert a["snaps"].shape == (4, 2, N) and a["probe"].shape == (11, 3, 2) and a["peak_idx"].dtype == np.int32
    assert np.array_equal(_bits(a["snaps"][1]), _bits(a["snaps"][3]))
    dev = torch.device("cuda:0")
    for offset in (0, 1):
        g = DB.guard_len(N)
        ins = [DB.input_(n, x, g, dev, offset) for n, x in (("lambda", lam), ("phi", phi), ("F", F), ("u_static", U))]
        dp = DB.input_("probe_dof", probe, g, dev, offset)
        outs = [DB.output("p", k, g, dev, offset), DB.output("probe", 11 * 3 * 2, g, dev, offset), DB.output("snaps", 4 * 2 * N, g, dev, offset),
                DB.output("peak", N, g, dev, offset)]
        pi = DB.Guarded("peak_idx", N, torch.int32, g, dev, offset, True)
        pi.alloc.fill_(-77)
        torch.cuda.synchronize()
        rep = gpu_ctx.harmonic_dev(N, k, ins[0].ptr, ins[1].ptr, ins[2].ptr, omega, outs[0].ptr, d_u_static=ins[3].ptr, alpha_R=0.5,
                                   beta_R=1e-9, zeta=zeta, n_probe=3, d_probe_dof=dp.ptr, d_probe=outs[1].ptr, snap_freq=snap,
                                   d_snaps=outs[2].ptr, d_peak=outs[3].ptr, d_peak_idx=pi.ptr)
        DB.check(ins + [dp] + outs)
        for o, key in zip(outs, KEYS):
            assert o.numpy().tobytes() == np.ascontiguousarray(a[key]).tobytes(), (offset, key)
        assert bool((pi.front == -77).all()) and bool((pi.back == -77).all())
        assert pi.numpy().tobytes() == a["peak_idx"].tobytes()
        assert _no_ms(rep) == _no_ms(a["report"])


def test_the_call_orders_itself_on_the_callers_stream(gpu_ctx, models):
    """d_F holds another load; the model's own arrives behind a delay on the caller's stream: the call has the bits of the host
    entry with the model's load."""
    import torch
    from tests.test_gpu_device_entries import _Producer, _race
    m = models("cube6j")
    lam, phi, F = m["lam"], m["phi"], m["F"]
    k, N = phi.shape
    omega = np.array([0.5 * np.sqrt(lam[0])])
    want = gpu_ctx.harmonic(lam, phi, F, omega, zeta=np.full(k, 0.02))
    stale = gpu_ctx.harmonic(lam, phi, F[::-1].copy(), omega, zeta=np.full(k, 0.02))
    assert want["peak"].tobytes() != stale["peak"].tobytes()
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    dl, dphi, dF = DB.input_("lambda", lam, g, dev), DB.input_("phi", phi, g, dev), DB.input_("F", F[::-1].copy(), g, dev)
    outs = [DB.output("p", k, g, dev), DB.output("peak", N, g, dev)]
    pi = torch.full((N,), -1, dtype=torch.int32, device=dev)
    producer = _Producer()
    _race(gpu_ctx, producer, True, dF, F, lambda: gpu_ctx.harmonic_dev(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, outs[0].ptr, zeta=np.full(k, 0.02),
                                                                      d_peak=outs[1].ptr, d_peak_idx=pi.data_ptr()))
    DB.check(outs)
    assert outs[0].numpy().tobytes() == want["p"].tobytes() and outs[1].numpy().tobytes() == want["peak"].tobytes()
    assert pi.cpu().numpy().tobytes() == want["peak_idx"].tobytes()


def _sentinels(k, N, nf, n_probe, n_snap):
    return dict(p=np.full(k, -7.25), probe=np.full((nf, n_probe, 2), -7.25), snaps=np.full((n_snap, 2, N), -7.25), peak=np.full(N, -7.25),
                peak_idx=np.full(N, -7, dtype=np.int32))


def _untouched(o):
    return all((x == (-7 if x.dtype == np.int32 else -7.25)).all() for x in o.values())


def test_harmonic_error_cases(gpu_ctx):
    import torch
    from stan_amd import hip
    N, k, nf = 300, 3, 4
    phi, F, us, lam, omega, _, _ = _synthetic(N, k, nf, "modal")
    base = dict(lam=lam, phi=phi, F=F, omega=omega, u_static=us, alpha_R=0.1, beta_R=1e-4, zeta=np.full(k, 0.01), probe_dof=[0, N - 1],
                snap_freq=[0, nf - 1])
    nan, inf = float("nan"), float("inf")
    cases = dict(
        lambda_zero=dict(lam=np.array([1.0, 0.0, 3.0])), lambda_negative=dict(lam=np.array([1.0, 2.0, -3.0])),
        lambda_nan=dict(lam=np.array([nan, 2.0, 3.0])), lambda_inf=dict(lam=np.array([1.0, 2.0, inf])),
        alpha_negative=dict(alpha_R=-1.0), alpha_nan=dict(alpha_R=nan), beta_negative=dict(beta_R=-1.0), beta_inf=dict(beta_R=inf),
        zeta_negative=dict(zeta=np.array([0.01, -0.01, 0.01])), zeta_nan=dict(zeta=np.array([0.01, 0.01, nan])),
        omega_negative=dict(omega=np.array([1.0, -1.0])), omega_nan=dict(omega=np.array([nan])), omega_inf=dict(omega=np.array([1.0, inf])),
        omega_overflows=dict(omega=np.array([1e200])),
        probe_high=dict(probe_dof=[0, N]), probe_low=dict(probe_dof=[-1]), snap_high=dict(snap_freq=[nf]), snap_low=dict(snap_freq=[-1]),
        too_many_frequencies=dict(omega=np.linspace(0.0, 1.0, 65537)))
    for name, kw in cases.items():
        args = dict(base)
        args.update(kw)
        nfq = np.asarray(args["omega"]).shape[0]
        o = _sentinels(k, N, nfq, len(args["probe_dof"]), len(args["snap_freq"]))
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.harmonic(args.pop("lam"), args.pop("phi"), args.pop("F"), args.pop("omega"), out=o, **args)
        assert ei.value.code == hip.E_ARG, (name, str(ei.value))
        assert _untouched(o), name
    # an undamped load exactly on a resonance names the frequency and the mode
    o = _sentinels(2, N, 2, 1, 1)
    with pytest.raises(hip.StanHipError) as ei:
        gpu_ctx.harmonic([4.0, 9.0], phi[:2], F, [1.0, 3.0], probe_dof=[0], snap_freq=[0], out=o)
    assert ei.value.code == hip.E_ARG and "frequency 1 and mode 1" in str(ei.value) and _untouched(o)
    assert ei.value.report["n_modes"] == 0          # an argument error: the report is not written
    gpu_ctx.harmonic([4.0, 9.0], phi[:2], F, [1.0, 3.0], zeta=[0.0, 1e-3])   # damped, it runs
    # counts, NULL where an array is required, peak without peak_idx: the device entry, nothing written through the outputs
    dev = torch.device("cuda:0")
    g = DB.guard_len(N)
    dl, dphi, dF = DB.input_("lambda", lam, g, dev), DB.input_("phi", phi, g, dev), DB.input_("F", F, g, dev)
    dpd = DB.input_("probe_dof", np.array([0, N], dtype=np.int32), g, dev)
    outs = [DB.output("p", k, g, dev), DB.output("peak", N, g, dev), DB.output("probe", nf * 2 * 2, g, dev), DB.output("snaps", 2 * N, g, dev)]
    pi = torch.full((N,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c, hd = gpu_ctx, gpu_ctx.harmonic_dev
    p_, pk_, pr_, sn_ = (x.ptr for x in outs)
    for call in (lambda: hd(0, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_), lambda: hd(-1, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_),
                 lambda: hd(N, 0, dl.ptr, dphi.ptr, dF.ptr, omega, p_), lambda: hd(N, 33, dl.ptr, dphi.ptr, dF.ptr, omega, p_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, np.zeros(0), p_),
                 lambda: hd(N, k, None, dphi.ptr, dF.ptr, omega, p_), lambda: hd(N, k, dl.ptr, None, dF.ptr, omega, p_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, None, omega, p_), lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, None),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, d_peak=pk_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, d_peak_idx=pi.data_ptr()),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, n_probe=2, d_probe=pr_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, n_probe=-1, d_probe_dof=dpd.ptr, d_probe=pr_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, n_probe=2, d_probe_dof=dpd.ptr, d_probe=pr_),
                 lambda: hd(N, k, dl.ptr, dphi.ptr, dF.ptr, omega, p_, snap_freq=[nf], d_snaps=sn_)):
        with pytest.raises(hip.StanHipError) as ei:
            call()
        assert ei.value.code == hip.E_ARG, str(ei.value)
    DB.check([dl, dphi, dF, dpd] + outs, written=False)
    for x in outs:
        assert bool((x.payload.view(torch.int64) == DB.UNWRITTEN_BITS).all()), x.name
    assert bool((pi == -1).all())
    assert c.lib.stan_hip_harmonic(None, hip.C.c_int64(1), hip.C.c_int32(1), None, None, None, None, hip.C.c_double(0), hip.C.c_double(0), None,
                                   hip.C.c_int32(1), None, hip.C.c_int32(0), None, None, hip.C.c_int32(0), None, None, None, None, None,
                                   None) == hip.E_ARG


def test_harmonic_is_refused_on_a_communicator():
    from stan_amd import hip
    one, lam = np.ones((1, 8)), np.ones(1)
    c = hip.Context(0)
    try:
        c.comm_init(0, 2, None)              # a detached rank of two
        assert "communicator" in _raises(hip, lambda: c.harmonic(lam, one, one[0], [0.5]), hip.E_UNSUPPORTED)
    finally:
        c.close()
    multi = hip.Context(devices=[0])         # a multi-device handle (one device, no communicator)
    try:
        assert "multi-device" in _raises(hip, lambda: multi.harmonic(lam, one, one[0], [0.5]), hip.E_UNSUPPORTED)
    finally:
        multi.close()


# ---- 4. console -----------------------------------------------------------------------------------------------------------------
def test_console_harmonic(tmp_path, built_libs, gpu_ctx):
    """stan_solver --harmonic on the 4^3 cube of tests/test_gpu_transient.py: the block, the "harmonic" JSON object (the modes those
    of --modes, the probe at f = 0 the static displacement, the peak that of the probe where the probe holds it), the .vtu arrays,
    the input file byte-identical afterwards, and the refusals of the file."""
    import json
    import os
    import re
    import subprocess
    from tests.test_gpu_transient import _console_db
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path, prefix = str(tmp_path / "t.STdb"), str(tmp_path / "out")
    n_nodes, tip = _console_db(path)
    before = open(path, "rb").read()
    run = lambda *a: subprocess.run([exe] + list(a), capture_output=True, text=True, timeout=300)
    last_json = lambda out: json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    out = run("--modes", "6", "--json", path)
    assert out.returncode == 0, out.stdout + out.stderr
    modes = last_json(out)["modes"]
    f1 = modes["frequency_hz"][0]
    args = ["--harmonic", "0,%r,9" % (1.6 * f1), "--modes", "6", "--rayleigh", "0,1e-7", "--modal-damping", "0.02", "--probe-node", str(tip),
            "--json", "--vtu", prefix, "--vtu-every", "4"]
    out = run(*(args + [path]))
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == before, "the input file must stay as it was"
    for word in ("Frequency response: (9 frequencies", "6 modes, static correction", "damping: Rayleigh alpha 0 beta 1e-07, modal ratio 0.02",
                 "Largest amplitude:", "Probe node %d:" % tip):
        assert word in out.stdout, word
    t = last_json(out)["harmonic"]
    assert t["n_modes"] == 6 and t["n_freq"] == 9 and t["f0_hz"] == 0.0 and t["f1_hz"] == 1.6 * f1 and t["modal_damping"] == 0.02
    assert t["alpha_R"] == 0.0 and t["beta_R"] == 1e-7 and t["modes_converged"] == 1 and t["static_cg_iterations"] > 0
    assert np.array_equal(_bits(np.array(t["lambda"])), _bits(np.array(modes["lambda"]))), "the modes are those of --modes, bit for bit"
    assert np.array_equal(_bits(np.array(t["mode_frequency_hz"])), _bits(np.array(modes["frequency_hz"])))
    hz = np.array(t["frequency_hz"])
    assert hz.shape == (9,) and hz[0] == 0.0 and hz[-1] == 1.6 * f1 and (np.diff(hz) > 0).all()
    lam = np.array(t["lambda"])
    ratio = 1e-7 * lam / (2 * np.sqrt(lam)) + 0.02
    assert np.allclose(t["damping_ratio"], ratio, rtol=1e-14, atol=0)
    pr = np.array(t["probe_re_im"])
    assert t["probe_node"] == tip and t["probe_direction"] == [0, 1, 2] and pr.shape == (9, 3, 2)
    amp = np.hypot(pr[:, :, 0], pr[:, :, 1])
    assert not pr[0, :, 1].any() and pr[0, 2, 0] > 0                      # f = 0: the static displacement, in phase, along the load
    assert int(np.argmax(amp[:, 2])) == 5                                 # 8 steps to 1.6 f1: index 5 is f1
    assert amp[5, 2] > 5 * amp[0, 2] and pr[5, 2, 1] < 0                  # the resonance lags the load
    assert t["peak"] >= amp.max() * (1 - 1e-15) and t["peak_frequency_index"] == 5 and t["peak_frequency_hz"] == hz[5]
    if t["peak_node"] == tip:
        assert t["peak"] == amp[5, t["peak_direction"]]
    rows = re.findall(r"^\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", out.stdout.split("Probe node")[1], flags=re.M)[:9]
    assert [int(r[0]) for r in rows] == list(range(9))
    assert np.allclose([[float(r[2]), float(r[4]), float(r[6])] for r in rows], amp, rtol=1e-8, atol=0)
    assert np.allclose([float(r[7]) for r in rows], np.degrees(np.arctan2(pr[:, 2, 1], pr[:, 2, 0])), rtol=1e-7, atol=1e-9)
    text = open(prefix + "_peak.vtu", "rb").read()
    assert b'Name="Peak Amplitude" NumberOfComponents="3"' in text and b'Name="Peak Frequency" format' in text
    assert ('NumberOfPoints="%d"' % n_nodes).encode() in text
    for f in (0, 4, 8):
        text = open("%s_freq_%04d.vtu" % (prefix, f), "rb").read()
        assert b'Name="Displacement Re" NumberOfComponents="3"' in text and b'Name="Displacement Im" NumberOfComponents="3"' in text
    assert sorted(os.listdir(str(tmp_path))) == ["out_freq_0000.vtu", "out_freq_0004.vtu", "out_freq_0008.vtu", "out_peak.vtu", "t.STdb"]
    # the consistent mass, one frequency; an undamped load on a resonance is the library's refusal (exit code 1)
    out = run("--harmonic", "%r,0,1" % (0.5 * f1), "--modes", "4", "--mass", "consistent", "--json", path)
    assert out.returncode == 2 and "F1 >= F0" in out.stderr
    out = run("--harmonic", "%r,%r,1" % (0.5 * f1, 0.5 * f1), "--modes", "4", "--mass", "consistent", "--json", path)
    assert out.returncode == 0, out.stdout + out.stderr
    t2 = last_json(out)["harmonic"]
    assert t2["mass"] == "consistent" and t2["n_freq"] == 1 and t2["frequency_hz"] == [0.5 * f1] and "consistent mass" in out.stdout
    out = run("--harmonic", "%r,%r,1" % (f1, f1), "--modes", "2", path)
    if out.returncode != 0:     # (sqrt(lambda) / 2 pi * 2 pi squared need not return lambda to the bit)
        assert out.returncode == 1 and "frequency 0 and mode 0" in out.stderr
    # the refusals of the file: no "Density", a non-zero "Displacement", an unknown probe node; the files stay as they were
    base = ["--harmonic", "0,10,3", "--modes", "2"]
    plain = str(tmp_path / "plain.STdb")
    _console_db(plain, density=False)
    b2 = open(plain, "rb").read()
    out = run(*(base + [plain]))
    assert out.returncode == 2 and "--harmonic needs a \"Density\" boundary condition" in out.stderr and open(plain, "rb").read() == b2
    moved = str(tmp_path / "moved.STdb")
    _console_db(moved, move=[0.0, 0.01, 0.0])
    b3 = open(moved, "rb").read()
    out = run(*(base + [moved]))
    assert out.returncode == 2 and "--harmonic takes homogeneous supports only" in out.stderr and open(moved, "rb").read() == b3
    out = run(*(base + ["--probe-node", "9999", path]))
    assert out.returncode == 2 and "no such node" in out.stderr
    assert open(path, "rb").read() == before
