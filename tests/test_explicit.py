"""The numpy restatement of the central-difference loop and of the stable step (tests/explicit_ref.py) against what is known in
closed form: the checks that the reference of tests/test_gpu_explicit.py deserves trust.  CPU only; K from the CPU oracle.

Bars.  A step is u' = 2 u - u_p + dt^2 (...): no solve, a handful of roundings per entry, but the scheme is a second difference:
a rounding error e in u_n comes back as a linearly growing term n e, so over STEPS = 40 steps the states carry about
STEPS^2 / 2 x 2^-53 = 9e-14 relative to the largest state, times the few operations of a step.  The bar is 1e-10 for states
relative to the largest state of the run (M-norm) and for the invariant relative to its largest term.  Measured (printed by each
test): free vibration <= 6.0e-14 (mode 1) and <= 1.9e-14 (the highest mode, theta up to 2.86); the mass-damped mode <= 7.9e-14;
the discrete invariant <= 2.5e-15.  lambda_upper / lambda_max is 1.74 (cube6), 2.18 (cube6j), 1.34 (perforated12), 2.04 (two_mat);
lambda_power / lambda_max after 30 iterations 0.9955, 0.9938, 0.9841, 0.9840, after 100 iterations 0.9978, 1.0000, 0.9932, 0.9935
-- at 30 all above 1 / 1.05^2 = 0.907, which is what lets dt = 1.05 dt_crit be refused with n_power = 30
(tests/test_gpu_explicit.py).  At 1.01 dt_crit the largest state reaches 1.5e45 static deflections in 400 steps, at 0.99 dt_crit
1.9987."""
import numpy as np
import pytest

from tests import explicit_ref as X
from tests import modes_ref as R

STEPS = 40
RATIOS = (0.5, 0.9, 0.99)      # dt / dt_crit, dt_crit = 2 / sqrt(lambda_max)
BAR = 1e-10
CPU_MODELS = ("cube6", "two_mat")


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name not in made:
            r = R.reference(name)
            lam_max, phi_max = X.top_pair(name, r["Kd"], r["M"])
            made[name] = dict(r, lam_max=lam_max, phi_max=phi_max, dt_crit=2.0 / np.sqrt(lam_max),
                              F=np.asarray(X.job(name).F, dtype=np.float64))
        return made[name]
    return get


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("mode", ("first", "highest"))
def test_free_vibration_is_a_cosine_of_the_discrete_frequency(refs, name, ratio, mode):
    """u0 = phi_j, v0 = 0, F = 0, no damping: u_n = phi_j cos(n theta), sin(theta / 2) = omega_j dt / 2; the start's u_{-1} is
    phi_j cos(theta) exactly."""
    r = refs(name)
    lam, phi = (r["lam"][0], r["Phi"][:, 0]) if mode == "first" else (r["lam_max"], r["phi_max"])
    M = r["M"]
    dt = ratio * r["dt_crit"]
    out = X.central(r["Kd"].__matmul__, M, np.zeros_like(M), dt, STEPS, u0=phi)
    theta = 2.0 * np.arcsin(np.sqrt(lam) * dt / 2.0)
    want = np.cos(np.arange(STEPS + 2) * theta)[:, None] * phi[None, :]
    err = max(X.m_norm(out["U"][n] - want[n], M) for n in range(STEPS + 1)) / X.m_norm(phi, M)
    err = max(err, X.m_norm(out["U_next"] - want[STEPS + 1], M) / X.m_norm(phi, M))
    print("free vibration %s %s dt/dt_crit=%g: theta %.4f, %.3e" % (name, mode, ratio, theta, err))
    assert err <= BAR


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("ratio", RATIOS)
def test_a_mass_damped_mode_is_the_scalar_recursion(refs, name, ratio):
    """alpha_R M keeps a mode a mode: the restatement on phi_1 with v0 = omega phi_1 / 2 is central_sdof times phi_1; 2 % and
    (so that the damping shows within 40 steps) 20 % of critical at mode 1."""
    r = refs(name)
    lam, phi, M = r["lam"][0], r["Phi"][:, 0], r["M"]
    dt = ratio * r["dt_crit"]
    for zeta in (0.02, 0.2):
        al = 2.0 * zeta * np.sqrt(lam)
        out = X.central(r["Kd"].__matmul__, M, np.zeros_like(M), dt, STEPS, u0=phi, v0=0.5 * np.sqrt(lam) * phi, alpha_R=al)
        us = X.central_sdof(lam, al, 0.0, 1.0, 0.5 * np.sqrt(lam), dt, STEPS)
        err = max(X.m_norm(out["U"][n] - us[n] * phi, M) for n in range(STEPS + 1)) / np.abs(us).max()
        err = max(err, X.m_norm(out["U_next"] - us[STEPS + 1] * phi, M) / np.abs(us).max())
        print("damped mode %s dt/dt_crit=%g zeta=%g: %.3e" % (name, ratio, zeta, err))
        assert err <= BAR


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("ratio", RATIOS)
def test_the_discrete_invariant_of_a_step_load_is_constant(refs, name, ratio):
    """Constant load, no damping: 1/2 w.M w + 1/2 u_n.K u_{n+1} - F.(u_n + u_{n+1}) / 2 with w = (u_{n+1} - u_n) / dt does not change."""
    r = refs(name)
    Kd, M, F = r["Kd"], r["M"], r["F"]
    dt = ratio * r["dt_crit"]
    out = X.central(Kd.__matmul__, M, F, dt, STEPS)
    U = np.vstack([out["U"], out["U_next"][None, :]])
    inv, scale = [], 0.0
    for n in range(STEPS + 1):
        w = (U[n + 1] - U[n]) / dt
        terms = (0.5 * (w * M * w).sum(), 0.5 * U[n] @ (Kd @ U[n + 1]), 0.5 * F @ (U[n] + U[n + 1]))
        inv.append(terms[0] + terms[1] - terms[2])
        scale = max(scale, max(abs(t) for t in terms))
    err = np.abs(np.array(inv) - inv[0]).max() / scale
    print("invariant %s dt/dt_crit=%g: %.3e" % (name, ratio, err))
    assert scale > 0 and err <= BAR


@pytest.mark.parametrize("name", X.MODELS)
def test_the_two_lambdas_bracket_lambda_max(refs, name):
    """lambda_upper >= lambda_max(eigh) >= lambda_power, lambda_power does not decrease in n_power, and at 30 iterations it
    already exceeds lambda_max / 1.05^2: a dt of 1.05 dt_crit is refused by proof."""
    r = refs(name)
    Kd, M, lam_max = r["Kd"], r["M"], r["lam_max"]
    rows, cols = np.nonzero(Kd)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M.shape[0]))])
    up = X.lambda_upper(rowptr, cols, Kd[rows, cols], M)
    powers = [X.lambda_power(Kd.__matmul__, M, n) for n in (0, 1, 2, 5, 10, 30, 100)]
    print("%s: lambda_max %.6e, upper / max %.4f, power / max %s" % (name, lam_max, up / lam_max, ["%.4f" % (p / lam_max) for p in powers]))
    assert up >= lam_max
    assert all(p <= lam_max * (1 + 8 * np.finfo(float).eps) for p in powers)
    assert all(b >= a * (1 - 8 * np.finfo(float).eps) for a, b in zip(powers, powers[1:]))
    assert powers[5] > lam_max / 1.05 ** 2


def test_the_stability_limit_is_where_the_eigenvalue_says(refs):
    """cube6 under its own load as a step load, 400 steps: at dt = 0.99 dt_crit every mode is u_st (1 - cos n theta), so
    ||u_n||_M <= 2 ||u_st||_M; at 1.01 dt_crit the highest mode grows by 1.33 per step."""
    r = refs("cube6")
    Kd, M, F = r["Kd"], r["M"], r["F"]
    static = X.m_norm(np.linalg.solve(Kd, F), M)
    stable = X.central(Kd.__matmul__, M, F, 0.99 * r["dt_crit"], 400)
    unstable = X.central(Kd.__matmul__, M, F, 1.01 * r["dt_crit"], 400)
    big_s = max(X.m_norm(u, M) for u in stable["U"]) / static
    with np.errstate(over="ignore", invalid="ignore"):
        big_u = max(X.m_norm(u, M) for u in unstable["U"]) / static
    print("max ||u_n||_M / ||u_st||_M over 400 steps: %.4f at 0.99 dt_crit, %.3e at 1.01 dt_crit" % (big_s, big_u))
    assert big_s <= 2.0 * (1 + 1e-9)
    assert not big_u <= 1e30
