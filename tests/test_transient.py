"""The numpy restatement of the Newmark loop (tests/transient_ref.py) against what is known in closed form: the checks that the
reference of tests/test_gpu_transient.py deserves trust.  CPU only; K from the CPU oracle.

Bars.  A step solves (K + sigma M) u' = b by a dense Cholesky factorisation: backward stable, so u' carries a relative error of
about cond_S 2^-53 in the energy norm, cond_S the condition of the Jacobi-scaled K + sigma M (below 1e5 for these models at
every dt used: measured 7.6e4 at dt = 5 T1 on two_mat); over 40 steps of a scheme that neither amplifies nor damps (beta_N = 1/4,
gamma = 1/2) the errors add up at worst linearly: 40 x 1e5 x 1.1e-16 = 4.4e-10.  The bar below is 1e-9, for states relative to
the largest state of the run (M-norm) and for the energy balance relative to the largest energy term.  Measured (printed by
each test): free vibration <= 5.7e-13; damped mode u <= 5.4e-13, v <= 1.8e-11, a <= 2.0e-10 (the largest at dt = T1 / 2000, where
a' = a0 (u' - u) - ... is a difference quotient of u: it loses the digits that u' - u cancels); energy balance <= 9.4e-14."""
import numpy as np
import pytest

from tests import modes_ref as R
from tests import transient_ref as T

STEPS = 40
DTS = (1.0 / 2000, 1.0 / 20, 5.0)     # dt / T1: mass-dominated, ordinary, stiffness-dominated
BAR = 1e-9
CPU_MODELS = ("cube6", "two_mat")


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name not in made:
            r = R.reference(name)
            made[name] = dict(r, T1=2.0 * np.pi / np.sqrt(r["lam"][0]), F=np.asarray(T.job(name).F, dtype=np.float64))
        return made[name]
    return get


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("dt_over_T1", DTS)
def test_free_vibration_is_a_cosine_of_the_discrete_frequency(refs, name, dt_over_T1):
    """u0 = phi_1, v0 = 0, F = 0, no damping, beta_N = 1/4, gamma = 1/2: u_n = phi_1 cos(n theta), tan(theta / 2) = omega dt / 2."""
    r = refs(name)
    lam, phi, M = r["lam"][0], r["Phi"][:, 0], r["M"]
    dt = dt_over_T1 * r["T1"]
    out = T.newmark(r["Kd"], M, np.zeros_like(M), dt, STEPS, u0=phi)
    theta = 2.0 * np.arctan(np.sqrt(lam) * dt / 2.0)
    want = np.cos(np.arange(STEPS + 1) * theta)[:, None] * phi[None, :]
    err = max(T.m_norm(out["U"][n] - want[n], M) for n in range(STEPS + 1)) / T.m_norm(phi, M)
    print("free vibration %s dt/T1=%g: %.3e" % (name, dt_over_T1, err))
    assert err <= BAR


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("dt_over_T1", DTS)
def test_a_damped_mode_is_the_scalar_recursion(refs, name, dt_over_T1):
    """Rayleigh damping keeps a mode a mode: the restatement on phi_1 is newmark_sdof with c = alpha_R + beta_R lambda times phi_1."""
    r = refs(name)
    lam, phi, M = r["lam"][0], r["Phi"][:, 0], r["M"]
    dt = dt_over_T1 * r["T1"]
    al, be = T.rayleigh(np.sqrt(r["lam"][0]), np.sqrt(r["lam"][2]), 0.02)
    assert al > 0 and be > 0
    out = T.newmark(r["Kd"], M, np.zeros_like(M), dt, STEPS, u0=phi, v0=0.5 * np.sqrt(lam) * phi, alpha_R=al, beta_R=be)
    us, vs, as_ = T.newmark_sdof(lam, al + be * lam, 0.0, 1.0, 0.5 * np.sqrt(lam), dt, STEPS)
    eu = max(T.m_norm(out["U"][n] - us[n] * phi, M) for n in range(STEPS + 1)) / np.abs(us).max()
    ev = max(T.m_norm(out["V"][n] - vs[n] * phi, M) for n in range(STEPS + 1)) / np.abs(vs).max()
    ea = max(T.m_norm(out["A"][n] - as_[n] * phi, M) for n in range(STEPS + 1)) / np.abs(as_).max()
    print("damped mode %s dt/T1=%g: u %.3e v %.3e a %.3e" % (name, dt_over_T1, eu, ev, ea))
    assert max(eu, ev, ea) <= BAR


@pytest.mark.parametrize("name", CPU_MODELS)
@pytest.mark.parametrize("dt_over_T1", DTS)
def test_the_energy_balance_of_a_step_load_is_constant(refs, name, dt_over_T1):
    """Step load, no damping, beta_N = 1/4, gamma = 1/2: kinetic + strain - external does not change over the steps."""
    r = refs(name)
    dt = dt_over_T1 * r["T1"]
    out = T.newmark(r["Kd"], r["M"], r["F"], dt, STEPS)
    e = out["energy"]
    bal = e[:, 0] + e[:, 1] - e[:, 2]
    scale = np.abs(e).max()
    assert scale > 0 and bal[0] == 0.0
    err = np.abs(bal - bal[0]).max() / scale
    print("energy %s dt/T1=%g: %.3e" % (name, dt_over_T1, err))
    assert err <= BAR


def test_the_perturbed_solves_leave_the_residual_they_claim(refs):
    """The yardstick of the device test: a perturbed solve's u' has the scaled residual eps against the unperturbed b."""
    r = refs("cube6")
    dt = r["T1"] / 20
    rng = np.random.default_rng(5)
    exact = T.newmark(r["Kd"], r["M"], r["F"], dt, 1)
    pert = T.newmark(r["Kd"], r["M"], r["F"], dt, 1, eps=1e-6, rng=rng)
    c = T.coef(dt)
    Ks = T.shifted_dense(r["Kd"], r["M"], c["sigma"])
    s = 1.0 / np.sqrt(np.diag(Ks))
    b = Ks @ exact["U"][1]
    res = np.linalg.norm(s * (b - Ks @ pert["U"][1])) / np.linalg.norm(s * b)
    assert abs(res - 1e-6) <= 1e-9


def test_curve_and_constants():
    cv = [(0.0, 0.0), (1.0, 2.0), (1.0, 5.0), (3.0, 1.0)]
    assert [T.curve_at(cv, x) for x in (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 9.0)] == [0.0, 0.0, 1.0, 5.0, 3.0, 1.0, 1.0]
    assert T.curve_at(None, 3.0) == 1.0
    c = T.coef(0.5)
    assert (c["a0"], c["a1"], c["a2"], c["a3"], c["a4"], c["a5"], c["c_K"], c["sigma"]) == (16.0, 4.0, 8.0, 1.0, 1.0, 0.0, 1.0, 16.0)
    al, be = T.rayleigh(3.0, 7.0, 0.02)
    for w in (3.0, 7.0):
        assert abs(al / (2 * w) + be * w / 2 - 0.02) <= 1e-15


def test_console_refuses_bad_transient_arguments_before_it_reads_anything(built_libs, tmp_path):
    """stan_solver --transient: the argument checks come before the file is opened and before a device is touched (exit code
    2, the reason on stderr, no file created)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stan_amd", "bin", "stan_solver")
    path = str(tmp_path / "none.STdb")
    ok = ["--transient", "--dt", "1e-3", "--steps", "4"]
    cases = [
        (["--transient", "--steps", "4"], "--dt"),
        (["--transient", "--dt", "0", "--steps", "4"], "--dt"),
        (["--transient", "--dt", "-1", "--steps", "4"], "--dt"),
        (["--transient", "--dt", "1e-3", "--steps", "-1"], "--steps"),
        (["--dt", "1e-3"], "belong to --transient"),
        (["--load-curve", "0,1"], "belong to --transient"),
        (ok + ["--newmark", "0.25"], "two numbers"),
        (ok + ["--newmark", "0.2,0.5"], "unconditional stability"),
        (ok + ["--newmark", "0.25,0.4"], "unconditional stability"),
        (ok + ["--rayleigh", "1,x"], "two numbers"),
        (ok + ["--rayleigh", "-1,0"], "--rayleigh"),
        (ok + ["--load-curve", "0,1,2"], "even count"),
        (ok + ["--load-curve", "0,1,2,1,1,0"], "descend"),
        (ok + ["--load-curve", "0,nan"], "finite"),
        (ok + ["--solve-eps", "-1"], "--solve-eps"),
        (ok + ["--vtu", str(tmp_path / "o"), "--vtu-every", "0"], "--vtu-every"),
        (ok + ["--modes", "3"], "two analyses"),
        (ok + ["--devices", "0,0"], "one device"),
        (["--modes-shift", "1.0"], "--modes"),
        (["--modes", "3", "--modes-shift", "-1"], "SIGMA > 0"),
    ]
    for args, needle in cases:
        out = subprocess.run([exe] + args + [path], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and needle in out.stderr, (args, out.returncode, out.stderr)
        assert "Reading input file" not in out.stdout, args
    assert not os.listdir(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--transient --dt DT --steps N" in out.stderr and "--modes-shift SIGMA" in out.stderr


def test_the_bindings_carry_the_header_constants():
    """stan_amd.hip.newmark_coef is the expression of the header (and of transient_ref.coef), bit for bit."""
    from stan_amd import hip
    for dt, bN, g, al, be in ((0.37, 0.25, 0.5, 0.0, 0.0), (1e-5, 0.3025, 0.6, 0.11, 2e-4)):
        assert np.array_equal(hip.newmark_coef(dt, bN, g, al, be), T.coef(dt, bN, g, al, be)["vec"])
