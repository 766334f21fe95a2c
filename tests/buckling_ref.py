"""Reference for linear buckling (stan_hip_kg_hex8_batch, stan_hip_geometric_stiffness_hex8, stan_hip_buckling, DESIGN.md
section 3.12).

  kg(T, X, u, E, nu, etype)   (s, S) [e, 8, 8]: the element scalars of the geometric stiffness over a number type of
                              tests/element_ref.py (LD: the reference, F64: the plain-fp64 restatement) with their rounding scale
  tri(s)                      [e, 8, 8] -> [e, 36], the upper triangle row-major (the layout of stan_hip_kg_hex8_batch)
  gather_nodes(j, s)          the ordered gather: Gn [n_nodes, n_nodes], entry (r, c) the sum of s[e][a][b] over ascending
                              element, then a, then b, in fp64 in exactly that order
  csr_values(j, Gn, rowptr, col)  the values stan_hip_matrix_to_csr exports for G on K's (full) pattern
  dense_reduced(j, Gn)        G on the free DOFs, dense
  disp_full(j, U)             the reduced solution as disp [n_nodes, 3] in NodeLib order
  box_job(nx, ny, nz, ...)    a clamped box of nx x ny x nz unit-spaced elements with nodal loads
  column_job(nz), cube4j_job(), cantilever_job()   the three models of tests/test_buckling.py
  start_block(N, q)           the driver's start block X0 [q, N]: column j >= 0 the integer hash of (row, j)
  restatement(Kd, Hd, k, ...) the driver loop of api_buckling.hip line by line in numpy with EXACT inner solves (perturb: a
                              relative perturbation of every solve)
  eigh_ref(Hd, Kd, n_ref)     scipy.linalg.eigh(H, K): (mu descending, Phi K-orthonormal columns, the lowest mu)
  pick_k, input_conditions, clusters, sin_max_angle_K, residual_bound   what the factor tests are built from"""
import numpy as np
import scipy.linalg
import scipy.sparse

from stan_amd import problem
from stan_amd.cube import cube_mesh
from tests import element_ref as E
from tests import modes_ref as MR

U53 = 2.0 ** -53
# Worst error of the plain-fp64 restatement kg(F64, ...) against kg(LD, ...) over E.family() x E.fields(), both element types,
# in units of 2^-52 S (E.units): measured on the development host; tests/test_buckling.py measures it again on every run and
# asserts it stays under twice this value.  What the device is held to: 4 x the measured value (FMA contraction and the
# butterfly order of the Gauss-point sum move the constant by a small factor).
KG_F64_UNITS_MEASURED = 0.364
DEVICE_KG_UNITS = 4 * KG_F64_UNITS_MEASURED


def _sig_tensor(sig):
    """[e, 6] (xx, yy, zz, xy, yz, xz) -> [e, 3, 3]"""
    return np.stack([np.stack([sig[:, 0], sig[:, 3], sig[:, 5]], axis=1), np.stack([sig[:, 3], sig[:, 1], sig[:, 4]], axis=1),
                     np.stack([sig[:, 5], sig[:, 4], sig[:, 2]], axis=1)], axis=1)


def kg(T, X, u, Em, nu, etype):
    """s[a][b] = sum_g w_g det J_g (grad N_a)^T Sigma_g grad N_b with sigma_g = D (B_g u), and its rounding scale: the product
    rule with absolute values over the gradients (dgr), the stress (the BL0 rows of dgr against |u|, through |D|) and det J
    (ddet), plus one rounding of the term itself."""
    X, u = T.arr(X), T.arr(u)
    ne = X.shape[0]
    lam, G = (np.broadcast_to(v, (ne,))[:, None] for v in E.lame(T, Em, nu))
    s, S = 0, 0
    for q in E.gauss_points(T, X, etype):
        gr, dgr = q["gr"], q["dgr"]
        eps, Se = E._bl0(gr, u), E._bl0(dgr, abs(u))
        tr, Str = lam * (eps[:, 0] + eps[:, 1] + eps[:, 2])[:, None], abs(lam) * (Se[:, 0] + Se[:, 1] + Se[:, 2])[:, None]
        sig = np.concatenate([tr + 2 * G * eps[:, :3], G * eps[:, 3:]], axis=1)
        Ssig = np.concatenate([Str + 2 * abs(G) * Se[:, :3], abs(G) * Se[:, 3:]], axis=1)
        Sg, aSg, dSg = _sig_tensor(sig), _sig_tensor(abs(sig)), _sig_tensor(Ssig)
        c = (q["det"] * q["w"])[:, None, None]
        form = lambda ga, Sm, gb: ((ga[:, :, :, None] * Sm[:, :, None, :]).sum(axis=1)[:, :, :, None] * gb[:, None, :, :]).sum(axis=2)   # noqa: E731
        s = s + c * form(gr, Sg, gr)                                  # [e, a, b] = sum_mn gr[m, a] Sig[m, n] gr[n, b]
        agr = abs(gr)
        S = (S + abs(c) * (form(dgr, aSg, agr) + form(agr, aSg, dgr) + form(agr, dSg, agr) + form(agr, aSg, agr)) +
             (q["ddet"] * q["w"])[:, None, None] * form(agr, aSg, agr))
    return s, S


_IU = np.triu_indices(8)


def tri(s):
    return np.asarray(s)[:, _IU[0], _IU[1]]


def untri(s36):
    s36 = np.asarray(s36)
    s = np.zeros((s36.shape[0], 8, 8), dtype=s36.dtype)
    s[:, _IU[0], _IU[1]] = s36
    s[:, _IU[1], _IU[0]] = s36
    return s


def element_scalars(T, j, disp):
    """kg over a job of mixed element types and materials: (s, S) [n_elem, 8, 8]."""
    ne = j.conn.shape[0]
    X, u = j.xyz[j.conn], np.asarray(disp).reshape(-1, 3)[j.conn]
    mat = np.asarray(j.mat_E_nu).reshape(-1, 2)[np.asarray(j.elem_mat)]
    dt = np.longdouble if T is E.LD else np.float64
    s, S = np.zeros((ne, 8, 8), dtype=dt), np.zeros((ne, 8, 8), dtype=dt)
    for t in (E.G1, E.G2):
        sel = np.nonzero(np.asarray(j.elem_type) == t)[0]
        if sel.size:
            s[sel], S[sel] = kg(T, X[sel], u[sel], mat[sel, 0], mat[sel, 1], t)
    return s, S


def gather_nodes(j, s):
    """Element after element, a = 0..7, b = 0..7: every entry of Gn receives its terms in ascending (element, a, b)."""
    n = j.xyz.shape[0]
    Gn = np.zeros((n, n))
    s = np.asarray(s, dtype=np.float64)
    conn = np.asarray(j.conn)
    for e in range(conn.shape[0]):
        c = conn[e]
        if np.unique(c).shape[0] == 8:          # distinct nodes: 64 distinct entries, one term each
            Gn[np.ix_(c, c)] += s[e]
        else:
            for a in range(8):
                for b in range(8):
                    Gn[c[a], c[b]] += s[e, a, b]
    return Gn


def _reduced_maps(j):
    """per reduced index: (node, component)"""
    nd = np.asarray(j.node_dof).reshape(-1, 3)
    red = np.asarray(j.red)
    node_of = np.empty(j.n_dof, dtype=np.int64)
    comp_of = np.empty(j.n_dof, dtype=np.int64)
    for c in range(3):
        node_of[nd[:, c]] = np.arange(nd.shape[0])
        comp_of[nd[:, c]] = c
    free = np.nonzero(red != -1)[0]
    return node_of[free], comp_of[free]


def csr_values(j, Gn, rowptr, col):
    node, comp = _reduced_maps(j)
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    return np.where(comp[rows] == comp[col], Gn[node[rows], node[col]], 0.0)


def dense_reduced(j, Gn):
    node, comp = _reduced_maps(j)
    return np.where(comp[:, None] == comp[None, :], Gn[np.ix_(node, node)], 0.0)


def disp_full(j, U):
    full = np.zeros(j.n_dof)
    full[np.asarray(j.red) != -1] = U
    return full[np.asarray(j.node_dof).reshape(-1)].reshape(-1, 3)


# ---- models -----------------------------------------------------------------------------------------------------------------
def box_mesh(nx, ny, nz, jitter=0.0, seed=5):
    """cube_mesh's numbering (x fastest, CHEXA order) on nx x ny x nz unit elements"""
    mx, my, mz = nx + 1, ny + 1, nz + 1
    k, jj, i = np.meshgrid(np.arange(mz), np.arange(my), np.arange(mx), indexing="ij")
    xyz = np.stack([i, jj, k], axis=-1).reshape(-1, 3).astype(np.float64)
    if jitter:
        xyz = xyz + np.random.default_rng(seed).uniform(-jitter, jitter, xyz.shape)
    ek, ej, ei = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    base = (ei + mx * (ej + my * ek)).reshape(-1)
    off = np.array([0, 1, 1 + mx, mx, mx * my, 1 + mx * my, 1 + mx + mx * my, mx + mx * my])
    return xyz, (base[:, None] + off[None, :]).astype(np.int32)


def box_job(xyz, conn, fixed, load_nodes, load_vals, Em=210000.0, nu=0.3):
    fixed = np.asarray(fixed, dtype=np.int32)
    return problem.make_job(xyz, conn, fixed, np.ones((fixed.shape[0], 3)), np.asarray(load_nodes, dtype=np.int32),
                            np.asarray(load_vals, dtype=np.float64), E=Em, nu=nu)


COLUMN_L, COLUMN_E = 10.0, 210000.0


def column_job(nz):
    """A 1 x 1 x 10 column of 2 x 2 x nz elements clamped at z = 0, nu = 0, under a uniform end pressure of total force 1 in -z
    (the consistent nodal loads of the 2 x 2 top face: corners 1/16, edge mids 1/8, the centre 1/4)."""
    xyz, conn = box_mesh(2, 2, nz)
    xyz = xyz * [0.5, 0.5, COLUMN_L / nz]
    top = np.nonzero(xyz[:, 2] == xyz[:, 2].max())[0]
    wx = np.where(xyz[top, 0] == 0.5, 0.5, 0.25)
    wy = np.where(xyz[top, 1] == 0.5, 0.5, 0.25)
    loads = np.zeros((top.shape[0], 3))
    loads[:, 2] = -wx * wy
    return box_job(xyz, conn, np.nonzero(xyz[:, 2] == 0.0)[0], top, loads, Em=COLUMN_E, nu=0.0)


def euler_load():
    """pi^2 E I / (4 L^2) of the clamped-free column, I = 1/12"""
    return np.pi ** 2 * COLUMN_E * (1.0 / 12.0) / (4.0 * COLUMN_L ** 2)


def cube4j_job():
    """A jittered 4^3 cube clamped at z = 0 under a compressive load on its top face"""
    xyz, conn = cube_mesh(4, jitter=0.15)
    top = np.nonzero(np.arange(125) // 25 == 4)[0]
    return box_job(xyz, conn, np.nonzero(np.arange(125) // 25 == 0)[0], top, np.tile([0.0, 0.0, -50.0], (top.shape[0], 1)))


def cantilever_job():
    """An 8 x 2 x 1 cantilever clamped at x = 0 under a transverse tip load: the spectrum is symmetric in sign"""
    xyz, conn = box_mesh(8, 2, 1)
    xyz = xyz * [1.0, 0.5, 0.25]
    tip = np.nonzero(xyz[:, 0] == 8.0)[0]
    return box_job(xyz, conn, np.nonzero(xyz[:, 0] == 0.0)[0], tip, np.tile([0.0, 10.0, 0.0], (tip.shape[0], 1)))


def cpu_matrices(j, T=E.F64):
    """(Kd, Hd, U) dense on the free DOFs from the CPU oracle's K, a dense static solve and the restatement of G; H = -G."""
    from oracle import pyoracle as O
    from tests import product_ref as P
    rc, A = O.assemble(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    assert rc == 0
    Kd = MR.dense(*P.full_csr(A))
    U = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Kd), j.F)
    s, _ = element_scalars(T, j, disp_full(j, U))
    return Kd, -dense_reduced(j, gather_nodes(j, np.asarray(s, dtype=np.float64))), U


# ---- the driver -------------------------------------------------------------------------------------------------------------
def start_block(N, q):
    X = np.empty((q, N))
    i = np.arange(N, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        for j in range(q):
            h = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(j) * np.uint64(0xD1B54A32D192ED03)
            h ^= h >> np.uint64(30); h *= np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(27); h *= np.uint64(0x94D049BB133111EB)
            h ^= h >> np.uint64(31)
            X[j] = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5
    return X


def normalise(X):
    """the entry of largest magnitude exactly +1 (the lowest index on a tie)"""
    out = np.empty_like(X)
    for j, x in enumerate(X):
        out[j] = x / x[int(np.argmax(np.abs(x)))]
    return out


def restatement(Kd, Hd, k, tol=1e-6, max_outer=100, perturb=0.0):
    N = Kd.shape[0]
    q = MR.block_size(N, k)
    cho = scipy.linalg.cho_factor(Kd)
    rng = np.random.default_rng(1)

    def solve(F):                                          # exact inner solves, [n, N] -> [n, N]
        out = scipy.linalg.cho_solve(cho, F.T).T
        return out * (1 + perturb * rng.standard_normal(out.shape)) if perturb else out
    Dg = np.diag(Kd).copy()
    Ks, Hs = scipy.sparse.csr_matrix(Kd), scipy.sparse.csr_matrix(Hd)      # the same products, without the zeros
    Z = solve((Hs @ start_block(N, q).T).T)
    outer = 0
    while True:
        outer += 1
        W, Y = (Ks @ Z.T).T, (Hs @ Z.T).T                  # 1
        A, B = Z @ W.T, Z @ Y.T                            # 2
        A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)            # 3
        mu, Q = MR.small_gen_eig(B, A)                     # 4: through the Cholesky factor of A
        order = np.argsort(-mu, kind="stable")
        mu, Q = mu[order], Q[:, order]
        X, KX, HX = Q.T @ Z, Q.T @ W, Q.T @ Y              # 5
        R = mu[:, None] * KX - HX
        rho = np.sqrt((R * R / Dg).sum(axis=1)) / (np.abs(mu) * np.sqrt((KX * KX / Dg).sum(axis=1)))      # 6
        done = bool((mu[:k] > 0).all() and (rho[:k] <= tol).all())                                        # 7
        if done or outer >= max_outer:
            break
        todo = rho > tol                                   # 8
        D = np.zeros_like(X)
        if todo.any():
            D[todo] = solve(-R[todo])
        Z = mu[:, None] * X + D
    npos = int((mu > 0).sum())
    kk = min(k, npos)
    return dict(mu=mu[:kk], factor=1.0 / mu[:kk], phi=normalise(X[:kk]), rho=rho[:kk], outer=outer, converged=done, block=q,
                n_positive=npos, lowest_negative_factor=(1.0 / mu[-1] if mu[-1] < 0 else 0.0), mu_block=mu)


N_REF = 48   # eigenpairs kept of a large model: the factors asked for, their clusters and the gap behind them lie well inside


def eigh_ref(Hd, Kd, n_ref=None):
    """(mu descending, Phi columns, the most negative mu); n_ref: only the n_ref largest mu (and the single lowest)"""
    Hs, N = 0.5 * (Hd + Hd.T), Kd.shape[0]
    if n_ref is None or n_ref >= N:
        mu, Phi = scipy.linalg.eigh(Hs, Kd)
        return mu[::-1].copy(), Phi[:, ::-1].copy(), float(mu[0])
    mu, Phi = scipy.linalg.eigh(Hs, Kd, subset_by_index=[N - n_ref, N - 1])
    low = scipy.linalg.eigh(Hs, Kd, subset_by_index=[0, 0], eigvals_only=True)
    return mu[::-1].copy(), Phi[:, ::-1].copy(), float(low[0])


def pick_k(mu_ref, kmin=4, kmax=24):
    """the smallest k >= kmin with a relative gap > 1e-3 in mu behind it and k positive mu in the reference"""
    npos = int((mu_ref > 0).sum())
    k = min(kmin, npos)
    while k < min(kmax, npos) and (mu_ref[k - 1] - mu_ref[k]) / mu_ref[k - 1] <= 1e-3:
        k += 1
    assert k >= 1 and mu_ref[k - 1] > 0 and (mu_ref[k - 1] - mu_ref[k]) / mu_ref[k - 1] > 1e-3
    return k


def input_conditions(Kd, Hd, mu_ref, k, tol, limit=150):
    """What a (model, k, tol) of the device tests has to meet, checked on the CPU: a relative gap > 1e-3 in mu behind k, at
    least k positive mu in the reference, and the restatement converging within `limit` outer steps.  Returns the restatement."""
    assert 1 <= k < mu_ref.shape[0] and mu_ref[k - 1] > 0 and (mu_ref[k - 1] - mu_ref[k]) / mu_ref[k - 1] > 1e-3, (k, mu_ref[:k + 1])
    r = restatement(Kd, Hd, k, tol=tol, max_outer=limit)
    assert r["converged"] and r["outer"] <= limit, (k, tol, r["outer"], r["rho"])
    return r


def clusters(mu_ref, k):
    """[(first, last + 1, gap)]: runs of relative gap < 1e-6 among the first k reference mu (descending), gap = the reference
    distance from the cluster to the rest of the spectrum"""
    out, a = [], 0
    while a < k:
        b = a + 1
        while b < k and (mu_ref[b - 1] - mu_ref[b]) / abs(mu_ref[b - 1]) < 1e-6:
            b += 1
        above = mu_ref[a - 1] - mu_ref[a] if a > 0 else np.inf
        below = mu_ref[b - 1] - mu_ref[b] if b < mu_ref.shape[0] else np.inf
        out.append((a, b, min(above, below)))
        a = b
    return out


def residual_bound(Kd, Hd, mu, X):
    """||H x - mu K x||_{K^-1} / ||x||_K per row of X: no eigenvalue of the pencil is farther from mu_j (K^-1 H is self-adjoint
    in the K-inner product)."""
    cho = scipy.linalg.cho_factor(Kd)
    R = (Hd @ X.T).T - mu[:, None] * (Kd @ X.T).T
    rn = np.sqrt(np.einsum("ij,ij->i", R, scipy.linalg.cho_solve(cho, R.T).T))
    return rn / np.sqrt(np.einsum("ij,ij->i", X, (Kd @ X.T).T)), rn


def rho_host(Kd, Hd, mu, X):
    Dg = np.diag(Kd)
    KX = (Kd @ X.T).T
    R = mu[:, None] * KX - (Hd @ X.T).T
    return np.sqrt((R * R / Dg).sum(axis=1)) / (np.abs(mu) * np.sqrt((KX * KX / Dg).sum(axis=1)))


def sin_max_angle_K(Pm, Pref, Kd):
    """the sine of the largest K-principal angle between span Pm and span Pref (columns, same dimension)"""
    Lc = np.linalg.cholesky(Kd)
    Qa, _ = np.linalg.qr(Lc.T @ Pm)
    Qb, _ = np.linalg.qr(Lc.T @ Pref)
    return float(np.linalg.norm(Qa - Qb @ (Qb.T @ Qa), 2))
