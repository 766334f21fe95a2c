"""Reference for the frequency response (stan_hip_harmonic): the restatement of the header's expressions,
line by line, in a floating-point type of the caller's choice (np.float64, or np.longdouble as the near-exact run), and the
direct solve the modal sum is measured against.

  project(phi, F, lam, u_static, ft)       (p [k], r [N]): p_j = phi_j . F, r = u_static - sum_j phi_j (p_j / lam_j), j ascending;
                                           u_static None: r = 0
  damping(lam, alpha_R, beta_R, zeta, ft)  c_j = alpha_R + beta_R lam_j + 2 zeta_j sqrt(lam_j)
  transfer(lam, omega, alpha_R, beta_R, zeta, ft)
                                           (g, h) [n_freq, k]: d = lam_j - w^2, e = w c_j, D = d d + e e, g = d / D, h = e / D; the
                                           complex transfer function of mode j is H_j = g - i h
  table(p, lam, omega, alpha_R, beta_R, zeta, ft)
                                           (a, b) [n_freq, k]: a = p_j g, b = -(p_j h)
  response(phi, r, a, b, dofs)             (re, im) [n_freq, n]: re = r_d + sum_j phi_jd a_jf, im = sum_j phi_jd b_jf, j ascending, at
                                           the DOFs `dofs` (None: all)
  peak(re, im)                             (sqrt(max_f amp2), the lowest f that attains it) per DOF, amp2 = re re + im im
  direct(Kd, M, F, w, alpha_R, beta_R, C)  x = (K - w^2 M + i w (alpha_R M + beta_R K + C))^-1 F by a dense complex solve; M [N] (the
                                           lumped mass) or [N, N]; C (default none) e.g. modal_damping_matrix(M, lam, Phi, zeta)
  modal_sum(phi, lam, F, omega, ...)       (re, im) [n_freq, N] of the modes given through project, table and response
  job, mat_rho, reference                  modes_ref's models"""
import numpy as np

from tests import modes_ref as R

LD = np.longdouble
U53 = 2.0 ** -53
job, mat_rho, reference = R.job, R.mat_rho, R.reference


def project(phi, F, lam, u_static=None, ft=np.float64):
    phi, F, lam = np.asarray(phi, dtype=ft), np.asarray(F, dtype=ft), np.asarray(lam, dtype=ft)
    p = np.array([(phi[j] * F).sum() for j in range(phi.shape[0])], dtype=ft)
    r = np.zeros(phi.shape[1], dtype=ft)
    if u_static is not None:
        r = np.asarray(u_static, dtype=ft).copy()
        for j in range(phi.shape[0]):
            r = r - phi[j] * (p[j] / lam[j])
    return p, r


def damping(lam, alpha_R=0.0, beta_R=0.0, zeta=None, ft=np.float64):
    lam = np.asarray(lam, dtype=ft)
    z = np.zeros(lam.shape[0], dtype=ft) if zeta is None else np.asarray(zeta, dtype=ft)
    return (ft(alpha_R) + ft(beta_R) * lam) + ft(2) * z * np.sqrt(lam)


def transfer(lam, omega, alpha_R=0.0, beta_R=0.0, zeta=None, ft=np.float64):
    lam, w = np.asarray(lam, dtype=ft)[None, :], np.asarray(omega, dtype=ft)[:, None]
    c = damping(lam[0], alpha_R, beta_R, zeta, ft)[None, :]
    d = lam - w * w
    e = w * c
    D = d * d + e * e
    return d / D, e / D


def table(p, lam, omega, alpha_R=0.0, beta_R=0.0, zeta=None, ft=np.float64):
    g, h = transfer(lam, omega, alpha_R, beta_R, zeta, ft)
    p = np.asarray(p, dtype=ft)[None, :]
    return p * g, -(p * h)


def response(phi, r, a, b, dofs=None):
    ft = a.dtype.type
    phi = np.asarray(phi, dtype=ft)
    r = np.asarray(r, dtype=ft)
    if dofs is not None:
        phi, r = phi[:, dofs], r[dofs]
    re = np.repeat(r[None, :], a.shape[0], axis=0)
    im = np.zeros_like(re)
    for j in range(phi.shape[0]):
        re = re + a[:, j, None] * phi[j][None, :]
        im = im + b[:, j, None] * phi[j][None, :]
    return re, im


def peak(re, im):
    a2 = re * re + im * im
    at = np.argmax(a2, axis=0)   # the first index of the maximum
    return np.sqrt(a2[at, np.arange(a2.shape[1])]), at.astype(np.int32)


def direct(Kd, M, F, w, alpha_R=0.0, beta_R=0.0, C=None):
    Md = np.diag(M) if np.ndim(M) == 1 else np.asarray(M)
    Cd = alpha_R * Md + beta_R * Kd
    if C is not None:
        Cd = Cd + C
    A = (Kd - (w * w) * Md) + 1j * w * Cd
    return np.linalg.solve(A, np.asarray(F, dtype=np.complex128))


def modal_damping_matrix(M, lam, Phi, zeta):
    """C = M Phi diag(2 zeta_j sqrt(lam_j)) Phi^T M for ALL the modes (Phi [N, N], M-orthonormal columns, M [N] diagonal): the
    matrix whose modal damping is zeta_j."""
    MP = M[:, None] * Phi
    return (MP * (2.0 * np.asarray(zeta) * np.sqrt(lam))[None, :]) @ MP.T


def modal_sum(phi, lam, F, omega, alpha_R=0.0, beta_R=0.0, zeta=None, u_static=None, ft=LD):
    """x [n_freq, N] complex (as a pair re, im in `ft`) of the k modes given, through the restatement."""
    p, r = project(phi, F, lam, u_static, ft)
    a, b = table(p, lam, omega, alpha_R, beta_R, zeta, ft)
    return response(phi, r, a, b)
