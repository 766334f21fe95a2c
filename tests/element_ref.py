"""Extended-precision reference for the HEX8 element math (stan_amd/csrc/hex8_device.h, k_recover in recovery.hip) and
the rounding scale the kernels are held to.

A literal restatement of what the device header states -- the sign tables, dN/d(xi, eta, zeta) in the factorised form,
J = dN X, Det3, adjugate over det, grad = J^-1 dN, c = det * w (HEX8_G2: eight points at +-sqrt(1/3), weight 1; HEX8_G1:
one point at the origin, weight 8),
    K_ab = sum_g c (lam ga gb^T + G gb ga^T + G (ga . gb) I),      lam, G as stan_lame forms them,
and for recovery eps_g = B_g u (BL0 rows xx, yy, zz, xy, yz, xz), sig_g = D eps_g, node value_i = sum_g N[i][g] value_g with
N[i][g] = prod over the axes of 1/2 (1 + s_i s_g sqrt 3) -- written once over a number type:

  LD    np.longdouble, all elements of a call at once (what every test compares with);
  F64   np.float64: the same formulas in the arithmetic of the kernels (numpy does not contract into FMAs) -- the "fp64
        restatement" of tests/test_element_ref.py and the body of its mutants;
  mp()  mpmath at 50 digits (inside mpmath.workdps(50)), element by element: what LD itself is checked against.

sqrt(1/3) and sqrt 3 are computed in the working type.  Inputs are float64 and taken as exact.

Every result comes with its ROUNDING SCALE S, a first-order propagation with absolute values of one relative rounding per
stored number (per Gauss point):
    Ja   = |dN| |X|                                        what an error of J is proportional to
    dgr  = |J^-1| Ja |J^-1| |dN| + |gr|                    d(J^-1) = J^-1 dJ J^-1, plus the gradient's own rounding
    ddet = |det| (sum(|J^-T| * Ja) + 1)                    d(det) = det tr(J^-1 dJ), plus its own rounding
    S(K_ab)   = sum_g |c| t(dgr_a |gb|^T + |ga| dgr_b^T) + ddet w t(|ga| |gb|^T),
                t(Q) = |lam| Q + |G| Q^T + |G| tr(Q) I      (the product rule on ga gb^T, each term weighted as in K_ab)
    S(eps_g)  = the BL0 rows of dgr against |u|
    S(sig_g)  = |lam| (S_xx + S_yy + S_zz) + 2 |G| S(eps_g) for the normal components, |G| S(eps_g) for the shears
    node values: S_i = sum_g |N[i][g]| S_g.
Errors are counted in units of 2^-52 S, entry by entry.  The scale follows the conditioning (coordinates far from the
origin, stretched and thin elements) over many orders of magnitude where a bar relative to max|K_e| cannot; it is pessimistic
on translated elements, which is the acceptable side.

Also here: the conditioning family, the displacement fields of the recovery tests, the dense scatter of K_e and S_e, and the
measured yardsticks with the bounds derived from them."""
import numpy as np

from tests.util import UNIT, random_hexes

# The reference needs an extended type: x86's 80-bit long double (eps 1.08e-19).  Where np.longdouble is the 64-bit double
# (Windows, some ARM builds) or a double-double with other rounding, run these tests on an x86-64 Linux host instead -- the
# mpmath path is exact anywhere but takes a second per element.
assert np.finfo(np.longdouble).eps < 2e-19, "tests/element_ref.py needs an 80-bit (or wider) np.longdouble: run on x86-64 Linux"

U52 = 2.0 ** -52
G1, G2 = 1, 2
# FE_Library.cs:225-235 / :121-128: natural-coordinate signs of node (and Gauss point) i, as hex8_device.h's HEX8_S* masks
SGN = np.array([[1.0 if (m >> i) & 1 else -1.0 for m in (0x66, 0xCC, 0xF0)] for i in range(8)])

# Worst error of the project's C restatement of the reference (oracle/stan_oracle.c: stan_oracle_ke_hex8, both element
# types; stan_oracle_recover_hex8, the three fields of fields()) over family(), against LD, in units of 2^-52 S: measured
# on the development host (x86-64, gcc -O2 without FMA contraction); tests/test_element_ref.py measures both again on every
# run, prints the worst per group and asserts they stay under twice these values, so the yardsticks cannot rot.  Both
# maxima fall on the stretched and rotated elements of "aspect_rot_shift_union" (K_e of HEX8_G2; the random field); the
# groups of well-shaped elements stay at or under 0.37 and 0.43.  For comparison, the F64 restatement of this file over
# the same family: 0.59 (K_e) and 0.96 (strain and stress).  (Under a coarser K_e scale -- every term weighted by
# |lam| + 2 |G|, the error carried through one of the two gradients only -- the same oracle errors read 0.38, and 0.28
# without the union group: S here is 1.3 to 25 times sharper, most where lam >> G.)
ORACLE_KE_UNITS_MEASURED = 0.60
ORACLE_REC_UNITS_MEASURED = 1.21
# What the device is held to: 4 x the measured values.  The margin covers FMA contraction and another summation order (the
# M-form, the butterfly extrapolation), each of which moves the constant by a small factor, not by an order of magnitude.
DEVICE_KE_UNITS = 4 * ORACLE_KE_UNITS_MEASURED
DEVICE_REC_UNITS = 4 * ORACLE_REC_UNITS_MEASURED
# The fields of fields() are rounded to float64 once, after an evaluation in LD: the strain of the rounded field differs from
# the exact field's (zero for the rigid one, sym(A) for the affine one) by at most sum |gr| 2^-53 |u| <= half a unit of S.
FIELD_ROUNDING_UNITS = 0.5

DEFAULT_MATERIAL = (210000.0, 0.3)
MIXED_MATERIALS = [(210000.0, 0.3), (1.0, 0.0), (1000.0, 0.4999), (2.1e11, 0.3), (7000.0, -0.2)]


# ---- number types ----------------------------------------------------------------------------------------------------------

class Num:
    """arr(a): float64 data as an array of the working type; sqrt(x): of one number of that type."""

    def __init__(self, name, arr, sqrt):
        self.name, self.arr, self.sqrt = name, arr, sqrt


LD = Num("longdouble", lambda a: np.asarray(a, dtype=np.float64).astype(np.longdouble), np.sqrt)
F64 = Num("float64", lambda a: np.asarray(a, dtype=np.float64).copy(), np.sqrt)


def mp():
    """mpmath numbers in object arrays; use inside `with mpmath.workdps(50)`."""
    import mpmath

    def arr(a):
        a = np.asarray(a, dtype=np.float64)
        return np.array([mpmath.mpf(float(v)) for v in a.ravel()] + [None], dtype=object)[:-1].reshape(a.shape)
    return Num("mpmath", arr, mpmath.sqrt)


def to_mp(a):
    """A longdouble (or float64) array as exact mpmath numbers: hi + lo, both float64."""
    import mpmath
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    lo = (a - hi).astype(np.float64)
    assert np.array_equal(hi.astype(np.longdouble) + lo.astype(np.longdouble), a)
    return np.array([mpmath.mpf(float(h)) + mpmath.mpf(float(l)) for h, l in zip(hi.ravel(), lo.ravel())] + [None],
                    dtype=object)[:-1].reshape(a.shape)


def _one(T):
    return T.arr(1.0)[()]


def _mat(a, b):
    """a [e, p, q] b [e, q, r] -> [e, p, r] (plain broadcasting: object arrays go through it too)."""
    return (a[:, :, :, None] * b[:, None, :, :]).sum(axis=2)


# ---- the element, Gauss point by Gauss point -------------------------------------------------------------------------------

def gauss_loc(T, etype, rel=0.0):
    """sqrt(1/3) in the working type (HEX8_G2) or 0 (HEX8_G1); rel: a relative error, for the mutants."""
    one = _one(T)
    if etype != G2:
        return 0 * one
    return T.sqrt(one / (3 * one)) * (1 + rel)


def dnl(T, p):
    """dN_i/d(xi, eta, zeta) at the natural point p[3], factorised as hex8_dnl: [3, 8]."""
    s = T.arr(SGN)
    f = 1 + s * p[None, :]                                  # [8, 3]: 1 + s_i p per axis
    return np.stack([0.125 * s[:, 0] * f[:, 1] * f[:, 2], 0.125 * s[:, 1] * f[:, 0] * f[:, 2], 0.125 * s[:, 2] * f[:, 0] * f[:, 1]])


def gauss_points(T, X, etype, gl_rel=0.0):
    """For each of the 8 Gauss points (HEX8_G1: the one) a dict: det [e], w, gr [e, 3, 8] and the scale parts
    dgr [e, 3, 8], ddet [e].  X: [e, 8, 3] of the working type."""
    gl = gauss_loc(T, etype, gl_rel)
    aX = abs(X)
    for g in range(8 if etype == G2 else 1):
        d = dnl(T, T.arr(SGN[g]) * gl)
        J = (d[None, :, :, None] * X[:, None, :, :]).sum(axis=2)            # [e, r, c] = sum_i d[r, i] X[i, c]
        j = [J[:, k // 3, k % 3] for k in range(9)]
        # MatrixST.cs:270-287 Det3, :294-319 Inverse, term by term as hex8_gp_setup
        det = (j[0] * j[4] * j[8] + j[3] * j[7] * j[2] + j[6] * j[1] * j[5] -
               j[2] * j[4] * j[6] - j[0] * j[5] * j[7] - j[8] * j[1] * j[3])
        x = 1 / det
        inv = np.stack([x * (j[4] * j[8] - j[5] * j[7]), x * (j[2] * j[7] - j[1] * j[8]), x * (j[1] * j[5] - j[2] * j[4]),
                        x * (j[5] * j[6] - j[3] * j[8]), x * (j[0] * j[8] - j[2] * j[6]), x * (j[2] * j[3] - j[0] * j[5]),
                        x * (j[3] * j[7] - j[4] * j[6]), x * (j[1] * j[6] - j[0] * j[7]), x * (j[0] * j[4] - j[1] * j[3])],
                       axis=1).reshape(-1, 3, 3)
        gr = (inv[:, :, :, None] * d[None, None, :, :]).sum(axis=2)          # [e, r, i]
        ad, ainv = abs(d), abs(inv)
        Ja = (ad[None, :, :, None] * aX[:, None, :, :]).sum(axis=2)
        dgr = (_mat(_mat(ainv, Ja), ainv)[:, :, :, None] * ad[None, None, :, :]).sum(axis=2) + abs(gr)
        ddet = abs(det) * ((ainv.transpose(0, 2, 1) * Ja).sum(axis=2).sum(axis=1) + 1)
        yield dict(det=det, w=1.0 if etype == G2 else 8.0, gr=gr, dgr=dgr, ddet=ddet)


def lame(T, E, nu):
    """Material.cs:39-40 as stan_lame writes them, in the working type."""
    E, nu = T.arr(E), T.arr(nu)
    return (E * nu) / ((1 - 2 * nu) * (1 + nu)), (0.5 * E) / (1 + nu)


def _outer(ga, gb):
    """[e, 3, 8] x [e, 3, 8] -> [e, a, m, b, n] = ga[m, a] gb[n, b]"""
    return ga.transpose(0, 2, 1)[:, :, :, None, None] * gb.transpose(0, 2, 1)[:, None, None, :, :]


def _iso(lam, G, P, transpose=True):
    """lam P + G P^T + G tr(P) I on every (a, b) block of P [e, a, m, b, n]."""
    out = lam * P + G * (P.swapaxes(2, 4) if transpose else P)
    tr = G[:, :, 0, :, 0] * (P[:, :, 0, :, 0] + P[:, :, 1, :, 1] + P[:, :, 2, :, 2])
    for m in range(3):
        out[:, :, m, :, m] = out[:, :, m, :, m] + tr
    return out


def ke(T, X, E, nu, etype, gl_rel=0.0, transpose=True):
    """(K_e, S_e), both [e, 24, 24] of the working type.  X [e, 8, 3] float64; E, nu scalars or [e]; one element type per
    call.  gl_rel and transpose=False make the mutants of tests/test_element_ref.py."""
    X = T.arr(X)
    ne = X.shape[0]
    lam, G = (np.broadcast_to(v, (ne,))[:, None, None, None, None] for v in lame(T, E, nu))
    alam, aG = abs(lam), abs(G)
    K, S = 0, 0
    for q in gauss_points(T, X, etype, gl_rel):
        c = (q["det"] * q["w"])[:, None, None, None, None]
        K = K + c * _iso(lam, G, _outer(q["gr"], q["gr"]), transpose)
        agr = abs(q["gr"])
        S = (S + abs(c) * _iso(alam, aG, _outer(q["dgr"], agr) + _outer(agr, q["dgr"])) +
             (q["ddet"] * q["w"])[:, None, None, None, None] * _iso(alam, aG, _outer(agr, agr)))
    return K.reshape(ne, 24, 24), S.reshape(ne, 24, 24)


def _bl0(gr, u):
    """The six BL0 rows (Element.cs:316-324) of gr [e, 3, 8] against u [e, 8, 3]: [e, 6] as xx, yy, zz, xy, yz, xz."""
    p = lambda r, c: (gr[:, r, :] * u[:, :, c]).sum(axis=1)    # noqa: E731
    return np.stack([p(0, 0), p(1, 1), p(2, 2), p(1, 0) + p(0, 1), p(2, 1) + p(1, 2), p(2, 0) + p(0, 2)], axis=1)


def extrapolation(T, s3_rel=0.0):
    """N[i][g] = prod over the axes of 1/2 (1 + s_i s_g sqrt 3): [8, 8]."""
    one = _one(T)
    s = T.arr(SGN)
    n3 = 0.5 * (1 + s[:, None, :] * s[None, :, :] * (T.sqrt(3 * one) * (1 + s3_rel)))
    return n3[:, :, 0] * n3[:, :, 1] * n3[:, :, 2]


def recover(T, X, u, E, nu, gl_rel=0.0, s3_rel=0.0):
    """(strain, stress, S_strain, S_stress) at the nodes of HEX8_G2 elements, all [e, 8, 6].  X, u [e, 8, 3] float64."""
    X, u = T.arr(X), T.arr(u)
    ne = X.shape[0]
    lam, G = (np.broadcast_to(v, (ne,))[:, None] for v in lame(T, E, nu))
    eg, sg, Seg, Ssg = [], [], [], []
    for q in gauss_points(T, X, G2, gl_rel):
        eps, Se = _bl0(q["gr"], u), _bl0(q["dgr"], abs(u))
        tr, Str = lam * (eps[:, 0] + eps[:, 1] + eps[:, 2])[:, None], abs(lam) * (Se[:, 0] + Se[:, 1] + Se[:, 2])[:, None]
        eg.append(eps)
        Seg.append(Se)
        sg.append(np.concatenate([tr + 2 * G * eps[:, :3], G * eps[:, 3:]], axis=1))
        Ssg.append(np.concatenate([Str + 2 * abs(G) * Se[:, :3], abs(G) * Se[:, 3:]], axis=1))
    N = extrapolation(T, s3_rel)
    node = lambda n, v: (n[None, :, :, None] * np.stack(v, axis=1)[:, None, :, :]).sum(axis=2)    # noqa: E731
    return node(N, eg), node(N, sg), node(abs(N), Seg), node(abs(N), Ssg)


def units(got, ref, S):
    """max |got - ref| / (2^-52 S) over every entry, as a float; the scale must be positive and finite everywhere."""
    S = np.asarray(S, dtype=np.longdouble)
    assert np.isfinite(S).all() and (S > 0).all()
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == S.shape and np.isfinite(got).all()
    return float((abs(got.astype(np.longdouble) - ref) / (U52 * S)).max())


# ---- the conditioning family -----------------------------------------------------------------------------------------------

def rotation(rng):
    Q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
    return Q if np.linalg.det(Q) > 0 else -Q


def stretch_rotate_shift(xyz):
    """Coordinates of a whole mesh stretched 1:1000 along x, rotated (a fixed proper rotation), translated by 1e4."""
    return (xyz * [1000.0, 1.0, 1.0]) @ rotation(np.random.default_rng(77)).T + 1e4


def family(seed=3, n=16):
    """name -> list of (X [k, 8, 3], E, nu): the conditioning family, from random_hexes(n, seed) ("plain": the hexes the
    parity tests use)."""
    rng = np.random.default_rng(seed + 1000)
    P = random_hexes(n, seed=seed)
    E0, nu0 = DEFAULT_MATERIAL
    Q = rotation(rng)
    stretched = P * [1000.0, 1.0, 1.0]
    thin = P.copy()
    thin[:, 4:] = thin[:, :4] + [0.0, 0.0, 1e-4]          # the top face 1e-4 above the (warped) bottom face
    anyhow = np.stack([(x * [10.0 ** rng.uniform(0, 3), 1.0, 1.0]) @ rotation(rng).T +
                       10.0 ** rng.uniform(0, 4) * rng.choice([-1.0, 1.0], 3) for x in P])
    fam = {
        "plain": [(P, E0, nu0)],
        "shift_1e3": [(P + 1e3, E0, nu0)],
        "shift_1e6": [(P + [1e6, -3e5, 7e5], E0, nu0)],
        "aspect_rot": [(stretched @ Q.T, E0, nu0)],
        "aspect_rot_shift_1e4": [(stretched @ Q.T + 1e4, E0, nu0)],
        "thin_1e-4": [(thin, E0, nu0)],
        "nu_0.4999": [(P, E0, 0.4999)],
        "nu_0": [(P, E0, 0.0)],
        "micro_E_2.1e11": [(P * 1e-6, 2.1e11, 0.3)],
        # the union of stretched, rotated and translated, each alone and all three at random per element
        "aspect_rot_shift_union": [(np.concatenate([stretched, P @ Q.T, P + 1e3, anyhow]), E0, nu0)],
        "materials": [(P[i::len(MIXED_MATERIALS)], E, nu) for i, (E, nu) in enumerate(MIXED_MATERIALS)],
        "unit_cube": [(UNIT[None].copy(), E0, nu0)],
    }
    return fam


def geometries(fam=None):
    """name -> X [k, 8, 3]: the elements of each group without their materials (the recovery tests bring nu = 0.4999)."""
    fam = family() if fam is None else fam
    return {name: np.concatenate([X for X, _E, _nu in parts]) for name, parts in fam.items()}


REC_MATERIAL = (210000.0, 0.4999)
AFFINE = np.array([[1.1e-3, -0.4e-3, 0.7e-3], [0.9e-3, -1.3e-3, 0.2e-3], [-0.6e-3, 0.5e-3, 0.8e-3]])
AFFINE_STRAIN = np.array([AFFINE[0, 0], AFFINE[1, 1], AFFINE[2, 2], AFFINE[0, 1] + AFFINE[1, 0],
                          AFFINE[1, 2] + AFFINE[2, 1], AFFINE[0, 2] + AFFINE[2, 0]])     # the shear as stored, not halved


def fields(X, seed=17):
    """name -> u [k, 8, 3] float64 for disconnected hexes X [k, 8, 3]:
      random  standard normal at 1e-3;
      rigid   w x X + t, |t| = 0.6 and |w| |X| up to 1e4 where the strains are 0;
      affine  AFFINE X: the exact strain is AFFINE_STRAIN at every corner.
    The last two are evaluated in longdouble and rounded once (FIELD_ROUNDING_UNITS)."""
    Xl = np.asarray(X, dtype=np.float64).astype(np.longdouble)
    t = np.array([0.3, -0.2, 0.5]).astype(np.longdouble)
    w = np.array([0.01, 0.02, -0.015]).astype(np.longdouble)
    rigid = np.stack([w[1] * Xl[..., 2] - w[2] * Xl[..., 1], w[2] * Xl[..., 0] - w[0] * Xl[..., 2],
                      w[0] * Xl[..., 1] - w[1] * Xl[..., 0]], axis=-1) + t
    A = AFFINE.astype(np.longdouble)
    affine = (Xl[..., None, :] * A).sum(axis=-1)
    return {"random": np.random.default_rng(seed).standard_normal(X.shape) * 1e-3,
            "rigid": rigid.astype(np.float64), "affine": affine.astype(np.float64)}


# ---- references by case, cached ---------------------------------------------------------------------------------------------

_cache = {}


def ke_reference(name, etype):
    """[(X, E, nu, K_ref, S), ...] in LD for the parts of group `name` as elements of type `etype`."""
    key = ("ke", name, etype)
    if key not in _cache:
        _cache[key] = [(X, E, nu) + ke(LD, X, E, nu, etype) for X, E, nu in family()[name]]
    return _cache[key]


def rec_reference(name, field):
    """(X, u, strain, stress, S_strain, S_stress) in LD for the geometry of group `name` under fields()[field] with
    REC_MATERIAL."""
    key = ("rec", name, field)
    if key not in _cache:
        X = geometries()[name]
        u = fields(X)[field]
        _cache[key] = (X, u) + recover(LD, X, u, *REC_MATERIAL)
    return _cache[key]


# ---- the assembled matrix ---------------------------------------------------------------------------------------------------

def scatter_dense(m, vals):
    """vals [n_elem, 24, 24] into the dense reduced matrix [n_red, n_red] through node_dof and red, in longdouble.  Every
    listing of a node counts (a collapsed hex adds to the same entry twice, as the K scatter does); fixed DOFs (red == -1)
    drop out."""
    dof = np.asarray(m.node_dof).reshape(-1, 3)[m.conn].reshape(-1, 24).astype(np.int64)       # [n_elem, 24]
    red = np.asarray(m.red)[dof]                # Solver.cs:121-132: -1 fixed, else the number of fixed DOFs before this one
    r = np.where(red >= 0, dof - red, -1)
    rows, cols = np.broadcast_arrays(r[:, :, None], r[:, None, :])
    keep = (rows >= 0) & (cols >= 0)
    D = np.zeros((m.n_red, m.n_red), dtype=np.longdouble)
    np.add.at(D, (rows[keep], cols[keep]), np.asarray(vals, dtype=np.longdouble)[keep])
    return D


def model_reference(m):
    """(K, S) dense [n_red, n_red] in LD for a job of mixed element types and materials."""
    ne = m.conn.shape[0]
    K = np.zeros((ne, 24, 24), dtype=np.longdouble)
    S = np.zeros((ne, 24, 24), dtype=np.longdouble)
    mat = np.asarray(m.mat_E_nu).reshape(-1, 2)[np.asarray(m.elem_mat)]
    for t in (G1, G2):
        sel = np.nonzero(np.asarray(m.elem_type) == t)[0]
        if sel.size:
            K[sel], S[sel] = ke(LD, m.xyz[m.conn[sel]], mat[sel, 0], mat[sel, 1], t)
    assert set(np.unique(m.elem_type)) <= {G1, G2}
    return scatter_dense(m, K), scatter_dense(m, S)
