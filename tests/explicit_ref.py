"""Reference for the explicit dynamics (stan_hip_explicit, stan_hip_stable_step): the binding restatement
of explicit.hip's header, line by line, in a floating-point type of the caller's choice (np.float64, or np.longdouble as the
near-exact run).

  coef(dt, alpha_R, ft)     dt, dt2 = dt dt, two_dt = 2 dt, om = 1 - h, op = 1 + h with h = alpha_R dt / 2, formed in `ft`
                            (ft = float64: the bits stan_cd_make_coef hands the kernel)
  start(c, g0, Ku0, ...)    a_0 = ((g0 F - Ku0) - alpha_R (M v0)) / M,  u_{-1} = (u0 - dt v0) + (dt2 / 2) a_0
  update(c, g, Ku, ...)     u_{n+1} = ((2 u_n - om u_{n-1}) + dt2 ((g F - Ku) / M)) / op
  state(c, w, u, up)        v_n = (w - up) / two_dt,  a_n = ((w - 2 u) + up) / dt2
  energies(g, Ku, M, F, u, v)   1/2 v.M v, 1/2 u.Ku, g F.u
  central(Kmul, M, F, dt, n_steps, ...)
                            the driver's loop: dict(U, V, A [n_steps + 1, N], energy [n_steps + 1, 3], U_next [N] = u_{n_steps+1});
                            step 0 reports u0, v0 and the start's a_0, the energies use the central difference v_n at every step;
                            Kmul: x -> K x in `ft` (Kd.__matmul__, or transient_ref.csr_ld for long double)
  central_sdof(lam, alpha_R, f, u0, v0, dt, n_steps)
                            the same recursion for m = 1: u [n_steps + 2] (u_0 .. u_{n_steps+1})
  lambda_upper(rowptr, col, val, M, ft)
                            max_d (sum_j |K_dj|) / M_d over a full CSR of the free DOFs
  start_vector(N)           the power iteration's x_0: the integer hash of (row, 0) of buckling_ref.start_block
  lambda_power(Kmul, M, n_power, ft)
                            x <- (K x / M) / sqrt(Kx.Kx / M), n_power times, then x.Kx / x.Mx
  top_pair(name, Kd, M)     (lambda_max, phi_max) of K x = lambda M x by scipy.linalg.eigh on D^-1/2 K D^-1/2, phi_max M-normalised;
                            computed once per model and left unchanged
  models, mat_rho, curve_at, csr_ld, m_norm   transient_ref's and modes_ref's"""
import numpy as np
import scipy.linalg

from tests import buckling_ref as B
from tests import modes_ref as R
from tests import transient_ref as T

LD = np.longdouble
MODELS = R.MODELS
job, mat_rho = R.job, R.mat_rho
curve_at, csr_ld, m_norm = T.curve_at, T.csr_ld, T.m_norm


def coef(dt, alpha_R=0.0, ft=np.float64):
    dt, al = ft(dt), ft(alpha_R)
    h = al * dt / ft(2)
    return dict(dt=dt, dt2=dt * dt, two_dt=ft(2) * dt, om=ft(1) - h, op=ft(1) + h, alpha_R=al)


def start(c, g0, Ku0, M, F, u0, v0):
    a0 = ((g0 * F - Ku0) - c["alpha_R"] * (M * v0)) / M
    um = (u0 - c["dt"] * v0) + (c["dt2"] / 2) * a0
    return a0, um


def update(c, g, Ku, M, F, u, up):
    r = g * F - Ku
    q = c["dt2"] * (r / M)
    w = (2 * u - c["om"] * up) + q
    return w / c["op"]


def state(c, w, u, up):
    return (w - up) / c["two_dt"], ((w - 2 * u) + up) / c["dt2"]


def energies(g, Ku, M, F, u, v):
    return np.array([0.5 * ((M * v) * v).sum(), 0.5 * (u * Ku).sum(), g * (F * u).sum()])


def central(Kmul, M, F, dt, n_steps, u0=None, v0=None, alpha_R=0.0, curve=None, ft=np.float64):
    c = coef(dt, alpha_R, ft)
    M, F = np.asarray(M, dtype=ft), np.asarray(F, dtype=ft)
    N = M.shape[0]
    u = np.zeros(N, dtype=ft) if u0 is None else np.asarray(u0, dtype=ft)
    v = np.zeros(N, dtype=ft) if v0 is None else np.asarray(v0, dtype=ft)
    Ku = np.zeros(N, dtype=ft) if u0 is None else np.asarray(Kmul(u), dtype=ft)
    a, up = start(c, ft(curve_at(curve, 0.0)), Ku, M, F, u, v)
    U, V, A, E = [], [], [], []
    for n in range(n_steps + 1):
        g = ft(curve_at(curve, n * float(dt)))
        if n > 0:
            Ku = np.asarray(Kmul(u), dtype=ft)
        w = update(c, g, Ku, M, F, u, up)
        vn, an = state(c, w, u, up)
        E.append(energies(g, Ku, M, F, u, vn))
        if n > 0:
            v, a = vn, an
        U.append(u); V.append(v); A.append(a)
        up, u = u, w
    return dict(U=np.array(U), V=np.array(V), A=np.array(A), energy=np.array(E), U_next=u)


def central_sdof(lam, alpha_R, f, u0, v0, dt, n_steps):
    c = coef(dt, alpha_R)
    u = float(u0)
    a0 = ((f - lam * u) - alpha_R * v0) / 1.0
    up = (u - dt * v0) + (c["dt2"] / 2) * a0
    us = [u]
    for n in range(n_steps + 1):
        w = ((2 * u - c["om"] * up) + c["dt2"] * (f - lam * u)) / c["op"]
        up, u = u, w
        us.append(u)
    return np.array(us)


def lambda_upper(rowptr, col, val, M, ft=np.float64):
    sums = np.add.reduceat(np.abs(val.astype(ft)), np.asarray(rowptr[:-1], dtype=np.int64))
    return (sums / np.asarray(M, dtype=ft)).max()


def start_vector(N):
    return B.start_block(N, 1)[0]


def lambda_power(Kmul, M, n_power, ft=np.float64):
    M = np.asarray(M, dtype=ft)
    x = start_vector(M.shape[0]).astype(ft)
    for _ in range(n_power):
        Kx = np.asarray(Kmul(x), dtype=ft)
        x = (Kx / M) / np.sqrt(((Kx * Kx) / M).sum())
    Kx = np.asarray(Kmul(x), dtype=ft)
    return (x * Kx).sum() / (x * (M * x)).sum()


_top = {}


def top_pair(name, Kd, M):
    if name not in _top:
        d = 1.0 / np.sqrt(M)
        N = M.shape[0]
        lam, y = scipy.linalg.eigh(d[:, None] * Kd * d[None, :], subset_by_index=[N - 1, N - 1])
        phi = d * y[:, 0]
        _top[name] = (float(lam[0]), phi / np.sqrt((M * phi * phi).sum()))
    return _top[name]
