"""Reference for the modal analysis (stan_hip_lumped_mass_hex8, stan_hip_modes).

  job(name)                 the models: "cube6" (stan_amd.cube's 6^3 cube clamped on x, no jitter: the y and z bending pairs are
                            exactly degenerate), "cube6j" (jitter 0.2: every eigenvalue distinct), "perforated12"
                            (tests/product_ref.py's), "two_mat" (the jittered cube, two materials, rho 1 : 10)
  mat_rho(name)             the densities per material
  lumped_mass(j, rho)       (M [N], mass_node [n_nodes], l [n_dof], volume) in plain fp64 numpy: tests/loads_ref.py's element
                            routines with mat_body = (rho, 0, 0), the node's mass = l at its first DOF
  dense(rowptr, col, val)   a full CSR as a dense matrix
  eigh_ref(Kd, M)           scipy.linalg.eigh(Kd, diag(M)), the lowest N_REF pairs: (lambda ascending, Phi [N, N_REF], M-orthonormal
                            columns)
  start_block(M, q)         the driver's start block X0 [q, N] (column 0 = M, column j the integer hash of (row, j))
  small_gen_eig(A, B)       A Q = B Q Lambda through the Cholesky factor of B
  restatement(Kd, M, k, tol, max_outer)
                            the driver loop of api_modal.hip line by line in numpy with EXACT inner solves:
                            dict(lam, phi [k, N], rho, outer, converged, block)
  normalise(X, M)           M-norm 1, the entry of largest magnitude positive (lowest index on a tie)
  rho_host(Kd, M, lam, phi) ||K x - lambda M x||_{M^-1} / lambda per mode in fp64
  pick_k(lam_ref)           the smallest k >= 6 with a relative gap > 1e-3 behind it
  clusters(lam_ref, k)      [(first, last + 1, gap)]: runs of relative gap < 1e-6 among the first k reference eigenvalues, gap =
                            the reference distance from the cluster to the rest of the spectrum
  sin_max_angle(P, Pref, M) the sine of the largest M-principal angle between span P and span Pref (columns)"""
import numpy as np
import scipy.linalg

from stan_amd import problem
from tests import loads_ref as L
from tests import product_ref as P

RHO = 7.85e-9
U53 = 2.0 ** -53
_jobs = {}


def _two_mat():
    j = problem.cube_job(6, jitter=0.1)
    j.elem_mat = (np.arange(j.conn.shape[0]) % 3 == 0).astype(np.int32)
    j.mat_E_nu = np.array([[210000.0, 0.3], [70000.0, 0.33]])
    return j


_BUILDERS = {"cube6": lambda: problem.cube_job(6), "cube6j": lambda: problem.cube_job(6, jitter=0.2),
             "perforated12": lambda: P.job("perforated12"), "two_mat": _two_mat}
MODELS = tuple(_BUILDERS)


def job(name):
    if name not in _jobs:
        _jobs[name] = _BUILDERS[name]()
    return _jobs[name]


def mat_rho(name):
    return np.array([RHO, 10 * RHO]) if name == "two_mat" else np.array([RHO])


def lumped_mass(j, rho):
    body = np.zeros((len(rho), 3))
    body[:, 0] = rho
    l, vol, _ = L.loads_np(j, L.Case(mat_body=body))
    d0 = np.asarray(j.node_dof).reshape(-1, 3)[:, 0]
    mass_node = l[d0]
    full = np.zeros(j.n_dof)
    for c in range(3):
        full[d0 + c] = mass_node
    free = np.nonzero(np.asarray(j.red) != -1)[0]
    return full[free], mass_node, l, vol


def dense(rowptr, col, val):
    n = rowptr.shape[0] - 1
    K = np.zeros((n, n))
    K[P.rows_of(rowptr), col] = val
    return K


def dense_upper(rowptr, col, val):
    K = dense(rowptr, col, val)
    return K + np.triu(K, 1).T


N_REF = 48   # eigenpairs kept: the modes asked for, their clusters and the gap behind them lie well inside


def eigh_ref(Kd, M):
    return scipy.linalg.eigh(Kd, np.diag(M), subset_by_index=[0, min(N_REF, M.shape[0]) - 1])


def start_block(M, q):
    N = M.shape[0]
    X = np.empty((q, N))
    X[0] = M
    i = np.arange(N, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        for j in range(1, q):
            h = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(j) * np.uint64(0xD1B54A32D192ED03)
            h ^= h >> np.uint64(30); h *= np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(27); h *= np.uint64(0x94D049BB133111EB)
            h ^= h >> np.uint64(31)
            X[j] = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5
    return X


def small_gen_eig(A, B):
    Lc = np.linalg.cholesky(0.5 * (B + B.T))
    T = scipy.linalg.solve_triangular(Lc, 0.5 * (A + A.T), lower=True)
    C = scipy.linalg.solve_triangular(Lc, T.T, lower=True).T
    lam, V = np.linalg.eigh(0.5 * (C + C.T))
    return lam, scipy.linalg.solve_triangular(Lc.T, V, lower=False)


def normalise(X, M):
    out = np.empty_like(X)
    for j, x in enumerate(X):
        x = x / np.sqrt((M * x * x).sum())
        i = int(np.argmax(np.abs(x)))          # the first index of the maximum
        out[j] = -x if x[i] < 0 else x
    return out


def block_size(N, k):
    return min(N, min(2 * k, k + 8))


def restatement(Kd, M, k, tol=1e-6, max_outer=100):
    N = M.shape[0]
    q = block_size(N, k)
    cho = scipy.linalg.cho_factor(Kd)
    solve = lambda F: scipy.linalg.cho_solve(cho, F.T).T      # exact inner solves, [n, N] -> [n, N]
    Z = solve(M[None, :] * start_block(M, q))
    outer = 0
    while True:
        outer += 1
        W = (Kd @ Z.T).T
        A, B = Z @ W.T, (Z * M[None, :]) @ Z.T
        lam, Q = small_gen_eig(A, B)
        X, KX = Q.T @ Z, Q.T @ W
        R = KX - (M[None, :] * X) * lam[:, None]
        rho = np.sqrt((R * R / M[None, :]).sum(axis=1)) / lam
        done = bool((rho[:k] <= tol).all())
        if done or outer >= max_outer:
            break
        todo = rho > tol
        D = np.zeros_like(X)
        D[todo] = solve(-R[todo] / lam[todo, None])
        Z = X / lam[:, None] + D
    return dict(lam=lam[:k], phi=normalise(X[:k], M), rho=rho[:k], outer=outer, converged=done, block=q)


def rho_host(Kd, M, lam, phi):
    R = (Kd @ phi.T).T - (M[None, :] * phi) * lam[:, None]
    return np.sqrt((R * R / M[None, :]).sum(axis=1)) / lam


def pick_k(lam_ref, kmin=6):
    k = kmin
    while (lam_ref[k] - lam_ref[k - 1]) / lam_ref[k - 1] <= 1e-3:
        k += 1
    return k


def clusters(lam_ref, k):
    out, a = [], 0
    while a < k:
        b = a + 1
        while b < k and (lam_ref[b] - lam_ref[b - 1]) / lam_ref[b - 1] < 1e-6:
            b += 1
        below = lam_ref[a] - lam_ref[a - 1] if a > 0 else np.inf
        above = lam_ref[b] - lam_ref[b - 1] if b < lam_ref.shape[0] else np.inf
        out.append((a, b, min(below, above)))
        a = b
    return out


def sin_max_angle(Pm, Pref, M):
    """Columns of Pm and Pref span the two subspaces (same dimension)."""
    s = np.sqrt(M)[:, None]
    Qa, _ = np.linalg.qr(s * Pm)
    Qb, _ = np.linalg.qr(s * Pref)
    c = np.linalg.svd(Qa.T @ Qb, compute_uv=False)
    # sin of the largest angle from the residual of the projection (cos near 1 loses it to rounding)
    return float(np.linalg.norm(Qa - Qb @ (Qb.T @ Qa), 2)) if c.size else 0.0


_ref = {}


def reference(name, Kd=None):
    """dict(M, lam, Phi, k) of a model, computed once from the CPU oracle's K (or the Kd given first) and left unchanged."""
    if name not in _ref:
        j = job(name)
        M = lumped_mass(j, mat_rho(name))[0]
        if Kd is None:
            from oracle import pyoracle as O
            rc, A = O.assemble(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
            assert rc == 0
            Kd = dense(*P.full_csr(A))
        lam, Phi = eigh_ref(Kd, M)
        _ref[name] = dict(M=M, lam=lam, Phi=Phi, k=pick_k(lam), Kd=Kd)
    return _ref[name]
