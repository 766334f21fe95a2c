"""Reference for the transient dynamics (stan_hip_matrix_shifted, stan_hip_transient).

  MODELS                    the four supported models of tests/modes_ref.py; FREE = "free4": a free-free cube 4^3 (jitter 0.1, no
                            supports), for the shifted matrix and the shifted modal analysis only
  job(name), mat_rho(name)  the models and their densities (modes_ref's; the free cube has modes_ref.RHO)
  coef(dt, ...)             the Newmark constants of include/stan_hip.h as a dict: a0 .. a5, c_K, sigma, and `vec` [8] as the
                            step helpers take them
  curve_at(curve, x)        the piecewise-linear load curve, the expression of api_transient.hip
  shifted_dense(Kd, M, s)   Kd + s diag(M)
  rayleigh(w_a, w_b, zeta)  (alpha_R, beta_R) with the damping ratio zeta at the angular frequencies w_a and w_b
  newmark(Kd, M, F, ...)    the loop of the driver line by line in fp64 numpy with EXACT dense solves (Cholesky of K + sigma M):
                            dict(U, V, A [n_steps + 1, N], energy [n_steps + 1, 3], sigma).  eps > 0: every solve's right-hand
                            side is perturbed by a random vector d with ||S d|| = eps ||S b||, S = diag(K + sigma M)^-1/2 -- the
                            residual a CG that stops on ||S r|| <= eps ||S b|| may leave, so the worst a conforming CG returns
  newmark_sdof(lam, c, ...) the same recursion for m = 1, stiffness lam, damping c, load f g(t): (u, v, a) [n_steps + 1]
  m_norm(x, M)              sqrt(x . M x)
  csr_ld(rowptr, col, val)  a product y = A x in np.longdouble from a full CSR (the dense matrices in long double would not fit)"""
import numpy as np
import scipy.linalg

from stan_amd import problem
from stan_amd.cube import cube_mesh
from tests import modes_ref as R

LD = np.longdouble
MODELS = R.MODELS
FREE = "free4"
_free = {}


def job(name):
    if name != FREE:
        return R.job(name)
    if FREE not in _free:
        xyz, conn = cube_mesh(4, jitter=0.1)
        none = np.zeros(0, dtype=np.int32)
        _free[FREE] = problem.make_job(xyz, conn, none, np.zeros((0, 3)), none, np.zeros((0, 3)))
    return _free[FREE]


def mat_rho(name):
    return np.array([R.RHO]) if name == FREE else R.mat_rho(name)


def coef(dt, beta_N=0.25, gamma=0.5, alpha_R=0.0, beta_R=0.0):
    a0 = 1.0 / (beta_N * dt * dt)
    a1 = gamma / (beta_N * dt)
    a2 = 1.0 / (beta_N * dt)
    a3 = 1.0 / (2.0 * beta_N) - 1.0
    a4 = gamma / beta_N - 1.0
    a5 = dt * (gamma / (2.0 * beta_N) - 1.0)
    c_K = 1.0 + a1 * beta_R
    return dict(a0=a0, a1=a1, a2=a2, a3=a3, a4=a4, a5=a5, c_K=c_K, sigma=(a0 + a1 * alpha_R) / c_K, dt=dt, gamma=gamma,
                beta_N=beta_N, alpha_R=alpha_R, beta_R=beta_R, vec=np.array([a0, a1, a2, a3, a4, a5, alpha_R, beta_R]))


def curve_at(curve, x):
    if curve is None or len(curve) == 0:
        return 1.0
    c = np.asarray(curve, dtype=np.float64).reshape(-1, 2)
    t, g = c[:, 0], c[:, 1]
    if x <= t[0]:
        return float(g[0])
    if x >= t[-1]:
        return float(g[-1])
    i = int(np.searchsorted(t, x, side="right")) - 1
    return float(g[i] + (g[i + 1] - g[i]) * ((x - t[i]) / (t[i + 1] - t[i])))


def shifted_dense(Kd, M, sigma):
    return Kd + np.diag(sigma * M)


def rayleigh(w_a, w_b, zeta):
    """zeta = alpha / (2 w) + beta w / 2 at both frequencies"""
    return 2.0 * zeta * w_a * w_b / (w_a + w_b), 2.0 * zeta / (w_a + w_b)


def m_norm(x, M):
    return float(np.sqrt((np.asarray(x) * M * np.asarray(x)).sum()))


def energies(Kd, M, F, u, v, g):
    return np.array([0.5 * (v * M * v).sum(), 0.5 * u @ (Kd @ u), g * (F @ u)])


def newmark(Kd, M, F, dt, n_steps, u0=None, v0=None, beta_N=0.25, gamma=0.5, alpha_R=0.0, beta_R=0.0, curve=None, eps=0.0,
            rng=None):
    c = coef(dt, beta_N, gamma, alpha_R, beta_R)
    N = M.shape[0]
    Ks = shifted_dense(Kd, M, c["sigma"])
    cho = scipy.linalg.cho_factor(Ks)
    s = 1.0 / np.sqrt(np.diag(Ks))
    u = np.zeros(N) if u0 is None else np.array(u0, dtype=np.float64)
    v = np.zeros(N) if v0 is None else np.array(v0, dtype=np.float64)
    r = curve_at(curve, 0.0) * F
    if v0 is not None and alpha_R != 0.0:
        r = r - alpha_R * (M * v)
    if v0 is not None and beta_R != 0.0:
        r = r - beta_R * (Kd @ v)
    if u0 is not None:
        r = r - Kd @ u
    a = r / M
    U, V, A, E = [u.copy()], [v.copy()], [a.copy()], [energies(Kd, M, F, u, v, curve_at(curve, 0.0))]
    for n in range(1, n_steps + 1):
        g = curve_at(curve, n * dt)
        p = c["a0"] * u + c["a2"] * v + c["a3"] * a
        w = c["a1"] * u + c["a4"] * v + c["a5"] * a
        b = g * F + M * (p + alpha_R * w)
        if beta_R != 0.0:
            b = b + beta_R * (Kd @ w)
        b = b / c["c_K"]
        if eps > 0.0:
            d = rng.standard_normal(N)
            d *= eps * np.linalg.norm(s * b) / np.linalg.norm(s * d)
            b = b + d
        un = scipy.linalg.cho_solve(cho, b)
        an = c["a0"] * (un - u) - c["a2"] * v - c["a3"] * a
        vn = v + dt * ((1.0 - gamma) * a + gamma * an)
        u, v, a = un, vn, an
        U.append(u.copy()); V.append(v.copy()); A.append(a.copy()); E.append(energies(Kd, M, F, u, v, g))
    return dict(U=np.array(U), V=np.array(V), A=np.array(A), energy=np.array(E), sigma=c["sigma"])


def newmark_sdof(lam, cd, f, u0, v0, dt, n_steps, beta_N=0.25, gamma=0.5, curve=None):
    a0, a1, a2 = 1.0 / (beta_N * dt * dt), gamma / (beta_N * dt), 1.0 / (beta_N * dt)
    a3, a4, a5 = 1.0 / (2.0 * beta_N) - 1.0, gamma / beta_N - 1.0, dt * (gamma / (2.0 * beta_N) - 1.0)
    u, v = float(u0), float(v0)
    a = curve_at(curve, 0.0) * f - cd * v - lam * u
    us, vs, as_ = [u], [v], [a]
    for n in range(1, n_steps + 1):
        b = curve_at(curve, n * dt) * f + (a0 * u + a2 * v + a3 * a) + cd * (a1 * u + a4 * v + a5 * a)
        un = b / (lam + a0 + a1 * cd)
        an = a0 * (un - u) - a2 * v - a3 * a
        vn = v + dt * ((1.0 - gamma) * a + gamma * an)
        u, v, a = un, vn, an
        us.append(u); vs.append(v); as_.append(a)
    return np.array(us), np.array(vs), np.array(as_)


def csr_ld(rowptr, col, val):
    """x -> A x in long double; every row of the full CSR has an entry (its diagonal)."""
    vl, starts = val.astype(LD), np.asarray(rowptr[:-1], dtype=np.int64)

    def mul(x):
        return np.add.reduceat(vl * np.asarray(x, dtype=LD)[col], starts)
    return mul


_ref = {}


def reference(name, Kd):
    """dict(M, lam, Phi, Kd, T1) of a supported model from the Kd given first (modes_ref.reference), left unchanged."""
    if name not in _ref:
        r = R.reference(name, Kd)
        _ref[name] = dict(r, T1=2.0 * np.pi / np.sqrt(r["lam"][0]))
    return _ref[name]
