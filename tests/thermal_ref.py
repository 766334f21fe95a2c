"""Reference for the thermal load and the thermal stress (stan_hip_thermal_load_hex8).

  beta(m, alpha)             beta_m = E alpha / (1 - 2 nu) per material, in fp64 exactly as written: an INPUT of the definitions
                             (the library forms it the same way on the host), not a rounding of the kernel
  Case                       mat_alpha [n_mat] and dT [n_nodes]
  reference(m, case)         (l_ref [n_dof], volume, dT_integral): the definitions evaluated and scattered in np.longdouble
                               f_a = sum_g grad N_a(q_g) beta dT(q_g) det J_g w,  dT(q) = sum_a N_a(q) dT_a
                             over the element's stiffness rule (HEX8_G2 2x2x2 weight 1, HEX8_G1 one point weight 8), elements
                             with alpha == 0 left out; volume = sum det J w, dT_integral = sum dT(q) det J w over the others
  scale(m, case)             s = sum |grad N_a| |beta dT(q)| |det J w|, scattered the same way (fp64 of a longdouble sum)
  rho(l, l_ref, s)           max_i |l_i - l_ref_i| / (2^-52 s_i) over the entries with s_i > 0
  loads_np(m, case)          (l, volume, dT_integral): a plain-fp64 numpy restatement in the operation form of the kernel (J
                             accumulated node by node, Det3 and the adjugate inverse as written, grad = J^-1 dN, dT(q) added
                             node by node, the force as (grad * (beta dT(q))) * (det J w)); the point terms are added in order
                             where the kernel adds them as a butterfly, and numpy does not contract into FMAs
  rho_np()                   the maximum of rho(loads_np) over cases(): the kernel is held to 4 x this number, the margin and the
                             reason of tests/forces_ref.py
  stress_expected(...)       sigma - beta dT at the corner's node in xx, yy, zz, in longdouble, with the bound's scale
The input set: the models of forces_ref.cases() without rigid5 (strips one below and one above 8 elements per wave and 32 per
workgroup, cubes, mixed4 with both element types and two materials in shuffled wire order, collapsed hexes, a star) with
(a) a random dT and per-material alpha, (b) a uniform dT, (c) alpha == 0 on one of mixed4's materials, (d) dT non-zero only at
the nodes of elements 7, 8, 31, 32 of the strips that have them."""

import numpy as np

from tests import forces_ref as R

U52 = R.U52
SX, SY, SZ, GL = R.SX, R.SY, R.SZ, R.GL
HEX8_G2 = 2


def beta(m, alpha):
    E, nu = m.mat_E_nu[:, 0], m.mat_E_nu[:, 1]
    return E * np.asarray(alpha, dtype=np.float64) / (1 - 2 * nu)


class Case:
    def __init__(self, mat_alpha, dT):
        self.mat_alpha = np.ascontiguousarray(mat_alpha, dtype=np.float64).reshape(-1)
        self.dT = np.ascontiguousarray(dT, dtype=np.float64).reshape(-1)


def _element_loads(m, case, dtype, want_scale=False):
    """fe [n_elem, 8, 3], volume, dT_integral (and the scale se) in `dtype`, in the operation form described above."""
    ne = m.conn.shape[0]
    fe = np.zeros((ne, 8, 3), dtype=dtype)
    se = np.zeros((ne, 8, 3), dtype=dtype)
    hot = np.nonzero(case.mat_alpha[m.elem_mat] != 0)[0]
    volume, integral = dtype(0), dtype(0)
    if hot.size:
        X = m.xyz[m.conn[hot]].astype(dtype)                       # [nh, 8, 3]
        T = case.dT[m.conn[hot]].astype(dtype)                     # [nh, 8]
        b = beta(m, case.mat_alpha)[m.elem_mat[hot]].astype(dtype)
        g2 = np.asarray(m.elem_type)[hot] == HEX8_G2
        one = dtype(GL) if dtype is np.float64 else dtype(1) / np.sqrt(dtype(3))
        gl = np.where(g2, one, dtype(0))
        f = np.zeros(X.shape, dtype=dtype)
        sa = np.zeros(X.shape, dtype=dtype)
        for g in range(8):
            w = np.where(g2, dtype(1), dtype(8 if g == 0 else 0))
            px, py, pz = dtype(SX[g]) * gl, dtype(SY[g]) * gl, dtype(SZ[g]) * gl
            d = np.empty((8, 3) + gl.shape, dtype=dtype)
            N = np.empty((8,) + gl.shape, dtype=dtype)
            for i in range(8):
                fx, fy, fz = 1 + dtype(SX[i]) * px, 1 + dtype(SY[i]) * py, 1 + dtype(SZ[i]) * pz
                d[i, 0] = dtype(0.125) * dtype(SX[i]) * fy * fz
                d[i, 1] = dtype(0.125) * dtype(SY[i]) * fx * fz
                d[i, 2] = dtype(0.125) * dtype(SZ[i]) * fx * fy
                N[i] = dtype(0.125) * fx * fy * fz
            J = np.zeros((9,) + gl.shape, dtype=dtype)
            for i in range(8):
                for r in range(3):
                    for c in range(3):
                        J[3 * r + c] += d[i, r] * X[:, i, c]
            det = (J[0] * J[4] * J[8] + J[3] * J[7] * J[2] + J[6] * J[1] * J[5] -
                   J[2] * J[4] * J[6] - J[0] * J[5] * J[7] - J[8] * J[1] * J[3])
            Xi = 1 / det
            inv = [Xi * (J[4] * J[8] - J[5] * J[7]), Xi * (J[2] * J[7] - J[1] * J[8]), Xi * (J[1] * J[5] - J[2] * J[4]),
                   Xi * (J[5] * J[6] - J[3] * J[8]), Xi * (J[0] * J[8] - J[2] * J[6]), Xi * (J[2] * J[3] - J[0] * J[5]),
                   Xi * (J[3] * J[7] - J[4] * J[6]), Xi * (J[1] * J[6] - J[0] * J[7]), Xi * (J[0] * J[4] - J[1] * J[3])]
            sc = det * w
            t = np.zeros(gl.shape, dtype=dtype)
            for a in range(8):
                t += N[a] * T[:, a]
            s = b * t
            volume += sc.sum()
            integral += (t * sc).sum()
            for a in range(8):
                for r in range(3):
                    gr = inv[3 * r] * d[a, 0] + inv[3 * r + 1] * d[a, 1] + inv[3 * r + 2] * d[a, 2]
                    f[:, a, r] += (gr * s) * sc
                    sa[:, a, r] += np.abs(gr) * np.abs(s) * np.abs(sc)
        fe[hot] = f
        se[hot] = sa
    return (fe, volume, integral, se) if want_scale else (fe, volume, integral)


_ref = {}


def reference(m, case):
    """(l_ref [n_dof] longdouble, volume, dT_integral) -- cached per (model, case) object pair and left unchanged."""
    key = (id(m), id(case))
    if key not in _ref:
        fe, vol, integral, se = _element_loads(m, case, np.longdouble, want_scale=True)
        _ref[key] = (m, case, R.scatter(m, fe, np.longdouble), vol, integral, R.scatter(m, se, np.longdouble).astype(np.float64))
    return _ref[key][2], _ref[key][3], _ref[key][4]


def scale(m, case):
    reference(m, case)
    return _ref[(id(m), id(case))][5]


def rho(l, l_ref, s):
    ok = s > 0
    if not ok.any():
        return 0.0
    err = np.abs(np.asarray(l, dtype=np.longdouble) - l_ref)[ok]
    return float((err / (U52 * s[ok])).max())


def loads_np(m, case):
    fe, vol, integral = _element_loads(m, case, np.float64)
    return R.scatter(m, fe, np.float64), float(vol), float(integral)


def integral_scale(m, case):
    """sum_q (sum_a |N_a dT_a|) |det J w| over the heated elements: what the roundings of dT_integral are relative to."""
    c = Case(case.mat_alpha, np.abs(case.dT))
    return float(abs(_element_loads(m, c, np.longdouble)[2]))


def stress_expected(m, case, stress):
    """(sigma - beta dT at the corner's node in xx, yy, zz [n_elem, 8, 6] longdouble, |sigma| + |beta dT| on those entries)"""
    bt = (beta(m, case.mat_alpha)[m.elem_mat].astype(np.longdouble)[:, None] * case.dT[m.conn].astype(np.longdouble))
    want = np.asarray(stress, dtype=np.float64).astype(np.longdouble).copy()
    want[:, :, :3] -= bt[:, :, None]
    mag = np.abs(np.asarray(stress, dtype=np.float64))[:, :, :3] + np.abs(bt).astype(np.float64)[:, :, None]
    return want, mag


# ---- the input set ------------------------------------------------------------------------------------------------------
def _alpha(m, seed):
    return np.random.default_rng(seed).uniform(0.8e-5, 2.4e-5, m.mat_E_nu.shape[0])


def _dT(m, seed):
    return np.random.default_rng(seed).uniform(-50.0, 150.0, m.xyz.shape[0])


_cases = {}


def cases():
    """name -> (model, Case): "<model>-rand" and "<model>-unif" for every model of forces_ref.cases() but rigid5 (cube5 again),
    "mixed4-cold" (material 1 does not expand), "<strip>-sel" (dT at the nodes of elements 7, 8, 31, 32 only)."""
    if not _cases:
        k = 0
        for name, (m, _) in R.cases().items():
            if name == "rigid5":
                continue
            k += 1
            ne, nn = m.conn.shape[0], m.xyz.shape[0]
            alpha = _alpha(m, 1700 + k)
            _cases[name + "-rand"] = (m, Case(alpha, _dT(m, 1800 + k)))
            _cases[name + "-unif"] = (m, Case(alpha, np.full(nn, 80.0)))
            if name == "mixed4":
                cold = alpha.copy(); cold[1] = 0.0
                _cases[name + "-cold"] = (m, Case(cold, _dT(m, 1900 + k)))
            el = np.array([e for e in (7, 8, 31, 32) if e < ne])
            if name.startswith("strip") and el.size:
                t = np.zeros(nn)
                nodes = np.unique(m.conn[el])
                t[nodes] = np.random.default_rng(2000 + k).uniform(20.0, 120.0, nodes.size)
                _cases[name + "-sel"] = (m, Case(alpha, t))
    return _cases


_rho_np = {}


def rho_np(verbose=False):
    """max over cases() of rho(loads_np): the yardstick the kernel is held to (x 4)."""
    if "all" not in _rho_np:
        worst = 0.0
        for name, (m, case) in cases().items():
            l_ref, _, _ = reference(m, case)
            r = rho(loads_np(m, case)[0], l_ref, scale(m, case))
            _rho_np[name] = r
            worst = max(worst, r)
        _rho_np["all"] = worst
    if verbose:
        print("rho_np per case: " + ", ".join("%s %.2f" % (k, v) for k, v in _rho_np.items()))
    return _rho_np["all"]
