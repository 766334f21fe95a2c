"""Reference for the load vector of distributed loads (stan_hip_load_vector_hex8).

  FACE_NODES             the local nodes of the six faces in CHEXA order; face (axis, s) = (f // 2, -1 / +1)
  Case                   mat_body [n_mat, 3] or None plus a canonical face list (face_elem, face_id, face_p) or None
  reference(m, case)     (l_ref [n_dof], volume, area): the definitions evaluated and scattered in np.longdouble
                           body      f_a = b_m sum_{2x2x2} N_a(q) det J(q)
                           pressure  f_a = -p sum_{2x2} N_a(q) n dA(q),  n dA = s (x_beta x x_gamma), (beta, gamma) the cyclic
                                     successors of the axis
                         volume = sum of det J(q) over the elements whose material has b != 0, area = sum over the listed faces
                         of |n dA(q)|_2
  scale(m, case)         s = sum |N_a| |b| |det J| + sum |p| N_a |n dA|_1, scattered the same way (fp64 of a longdouble sum)
  rho(l, l_ref, s)       max_i |l_i - l_ref_i| / (2^-52 s_i) over the entries with s_i > 0
  loads_np(m, case)      (l, volume, area): a plain-fp64 numpy restatement in the operation form of the kernel (J accumulated
                         node by node, Det3 as written, N_a = 0.125 fx fy fz, the point sum first and b / -p applied to it, faces
                         in ascending id after the body term); the point terms are added in order where the kernel adds them as a
                         butterfly, and numpy does not contract into FMAs
  rho_np()               the maximum of rho(loads_np) over cases(): the kernel is held to 4 x this number, the margin and the
                         reason of tests/forces_ref.py.
The input set is the smallest at which the kernels can go wrong: the models of forces_ref.cases() (strips one below and one
above 8 elements per wave and 32 per workgroup, cubes, mixed types and materials in shuffled wire order, collapsed hexes, a
star) with the face lists none / all six faces of every element / the free surface / a single face on the last element /
faces on elements 7, 8, 31, 32 of a strip only."""

import numpy as np

from tests import forces_ref as R

U52 = R.U52
SX, SY, SZ, GL = R.SX, R.SY, R.SZ, R.GL
S3 = np.stack([SX, SY, SZ])                                  # [axis, node]
FACE_NODES = [[0, 3, 4, 7], [1, 2, 5, 6], [0, 1, 4, 5], [2, 3, 6, 7], [0, 1, 2, 3], [4, 5, 6, 7]]


class Case:
    def __init__(self, mat_body=None, face_elem=None, face_id=None, face_p=None):
        self.mat_body = None if mat_body is None else np.ascontiguousarray(mat_body, dtype=np.float64).reshape(-1, 3)
        self.face_elem = None if face_elem is None else np.ascontiguousarray(face_elem, dtype=np.int32)
        self.face_id = None if face_elem is None else np.ascontiguousarray(face_id, dtype=np.uint8)
        self.face_p = None if face_elem is None else np.ascontiguousarray(face_p, dtype=np.float64)

    @property
    def n_faces(self):
        return 0 if self.face_elem is None else int(self.face_elem.shape[0])

    def kw(self):
        """keyword arguments of hip.Context.load_vector_hex8"""
        return dict(mat_body=self.mat_body, face_elem=self.face_elem, face_id=self.face_id, face_pressure=self.face_p)


def _points(dtype):
    gl = dtype(1) / np.sqrt(dtype(3))
    return gl


def _dnl(p, dtype):
    """dN_i / d(xi, eta, zeta) at natural point p (3 scalars): [8, 3], hex8_dnl's form."""
    d = np.empty((8, 3), dtype=dtype)
    for i in range(8):
        fx, fy, fz = 1 + dtype(SX[i]) * p[0], 1 + dtype(SY[i]) * p[1], 1 + dtype(SZ[i]) * p[2]
        d[i, 0] = dtype(0.125) * dtype(SX[i]) * fy * fz
        d[i, 1] = dtype(0.125) * dtype(SY[i]) * fx * fz
        d[i, 2] = dtype(0.125) * dtype(SZ[i]) * fx * fy
    return d


def _shape(p, dtype):
    return np.array([dtype(0.125) * (1 + dtype(SX[i]) * p[0]) * (1 + dtype(SY[i]) * p[1]) * (1 + dtype(SZ[i]) * p[2])
                     for i in range(8)], dtype=dtype)


def _jac(X, d):
    """J[e, r, c] = sum_i d[i, r] X[e, i, c], accumulated node by node (hex8_jacobian)."""
    J = np.zeros((X.shape[0], 3, 3), dtype=X.dtype)
    for i in range(8):
        for r in range(3):
            J[:, r, :] += d[i, r] * X[:, i, :]
    return J


def _det3(J):
    j = [J[:, r, c] for r in range(3) for c in range(3)]
    return (j[0] * j[4] * j[8] + j[3] * j[7] * j[2] + j[6] * j[1] * j[5] -
            j[2] * j[4] * j[6] - j[0] * j[5] * j[7] - j[8] * j[1] * j[3])


def _face_point(f, q, gl, dtype):
    """natural coordinates of point q (bit 0 -> beta, bit 1 -> gamma) of face f, and (axis, s, beta, gamma)"""
    axis, s = f // 2, dtype(1 if f & 1 else -1)
    beta, gamma = (axis + 1) % 3, (axis + 2) % 3
    p = [None, None, None]
    p[axis] = s
    p[beta] = gl if q & 1 else -gl
    p[gamma] = gl if q & 2 else -gl
    return p, axis, s, beta, gamma


def _cross(b, c):
    return np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2],
                     b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], axis=1)


def _element_loads(m, case, dtype, want_scale=False):
    """fe [n_elem, 8, 3], volume, area (and the scale se) in `dtype`, in the operation form described above."""
    X = m.xyz[m.conn].astype(dtype)
    ne = X.shape[0]
    gl = dtype(GL) if dtype is np.float64 else _points(dtype)
    fe = np.zeros((ne, 8, 3), dtype=dtype)
    se = np.zeros((ne, 8, 3), dtype=dtype)
    volume, area = dtype(0), dtype(0)
    if case.mat_body is not None:
        b = case.mat_body[m.elem_mat].astype(dtype)                          # [ne, 3]
        has = (case.mat_body[m.elem_mat] != 0).any(axis=1)
        w = np.zeros((ne, 8), dtype=dtype)
        wa = np.zeros((ne, 8), dtype=dtype)
        for g in range(8):
            p = [dtype(SX[g]) * gl, dtype(SY[g]) * gl, dtype(SZ[g]) * gl]
            det = np.where(has, _det3(_jac(X, _dnl(p, dtype))), dtype(0))
            N = _shape(p, dtype)
            w += N[None, :] * det[:, None]
            wa += np.abs(N)[None, :] * np.abs(det)[:, None]
            volume += det.sum()
        fe += b[:, None, :] * w[:, :, None]
        se += np.abs(b)[:, None, :] * wa[:, :, None]
    if case.n_faces:
        for f in range(6):                                                   # an element's faces in ascending id
            k = np.nonzero(case.face_id == f)[0]
            if k.size == 0:
                continue
            el = case.face_elem[k]
            Xf = X[el]
            v = np.zeros((k.size, 8, 3), dtype=dtype)
            va = np.zeros((k.size, 8), dtype=dtype)
            for q in range(4):
                p, axis, s, beta, gamma = _face_point(f, q, gl, dtype)
                J = _jac(Xf, _dnl(p, dtype))
                n = s * _cross(J[:, beta, :], J[:, gamma, :])
                N = _shape(p, dtype)
                v += N[None, :, None] * n[:, None, :]
                va += N[None, :] * np.abs(n).sum(axis=1)[:, None]
                area += np.sqrt((n * n).sum(axis=1)).sum()
            pk = case.face_p[k].astype(dtype)
            fe[el] -= pk[:, None, None] * v                                  # (el are distinct within one face id)
            se[el] += np.abs(pk)[:, None, None] * va[:, :, None]
    return (fe, volume, area, se) if want_scale else (fe, volume, area)


_ref = {}


def reference(m, case):
    """(l_ref [n_dof] longdouble, volume, area) -- cached per (model, case) object pair and left unchanged."""
    key = (id(m), id(case))
    if key not in _ref:
        fe, vol, area, se = _element_loads(m, case, np.longdouble, want_scale=True)
        _ref[key] = (m, case, R.scatter(m, fe, np.longdouble), vol, area, R.scatter(m, se, np.longdouble).astype(np.float64))
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
    fe, vol, area = _element_loads(m, case, np.float64)
    return R.scatter(m, fe, np.float64), float(vol), float(area)


# ---- face lists ---------------------------------------------------------------------------------------------------------
def canonical(face_elem, face_id, face_p):
    key = np.asarray(face_elem, dtype=np.int64) * 6 + np.asarray(face_id, dtype=np.int64)
    o = np.argsort(key, kind="stable")
    assert (np.diff(key[o]) > 0).all()
    return np.asarray(face_elem)[o], np.asarray(face_id)[o], np.asarray(face_p)[o]


def all_faces(m):
    ne = m.conn.shape[0]
    return np.repeat(np.arange(ne), 6), np.tile(np.arange(6), ne)


def free_surface(m):
    """(face_elem, face_id) of the faces whose sorted distinct node set occurs once; faces with fewer than three distinct
    nodes are left out."""
    fe, fi = all_faces(m)
    seen = {}
    for e, f in zip(fe, fi):
        nodes = tuple(sorted(set(m.conn[e, FACE_NODES[f]].tolist())))
        if len(nodes) >= 3:
            seen.setdefault(nodes, []).append((e, f))
    out = sorted(v[0] for v in seen.values() if len(v) == 1)
    return np.array([e for e, _ in out]), np.array([f for _, f in out])


def _pressures(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, n)


def _body(m, seed):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (m.mat_E_nu.shape[0], 3))


PARTS = ("body", "all6", "surf", "last")      # body only | faces only, all six | both, free surface | faces only, one face
_cases = {}


def cases():
    """name -> (model, Case): "<model>-<part>" for every model of forces_ref.cases() (rigid5 is cube5 again: left out), plus
    "<strip>-sel": body and faces on elements 7, 8, 31, 32 only."""
    if not _cases:
        k = 0
        for name, (m, _) in R.cases().items():
            if name == "rigid5":
                continue
            k += 1
            ne = m.conn.shape[0]
            body = _body(m, 700 + k)
            _cases[name + "-body"] = (m, Case(mat_body=body))
            fe, fi = all_faces(m)
            _cases[name + "-all6"] = (m, Case(None, *canonical(fe, fi, _pressures(fe.size, 800 + k))))
            fe, fi = free_surface(m)
            _cases[name + "-surf"] = (m, Case(body, *canonical(fe, fi, _pressures(fe.size, 900 + k))))
            _cases[name + "-last"] = (m, Case(None, [ne - 1], [(3 * k) % 6], [1.25]))
            if name in ("strip9", "strip33"):
                el = np.array([e for e in (7, 8, 31, 32) if e < ne])
                fe, fi = np.repeat(el, 2), np.tile([1 + k % 2, 4], el.size)
                _cases[name + "-sel"] = (m, Case(body, *canonical(fe, fi, _pressures(fe.size, 1000 + k))))
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


# ---- models of the patch tests (tests/test_loads.py on the CPU, tests/test_gpu_loads.py end to end) ----------------------
def patch_model(n=4, jitter=0.2, supports="sym"):
    """n^3 HEX8_G2 cube, interior nodes jittered, boundary planes planar.  supports "sym": x = 0 fixed in x, y = 0 in y,
    z = 0 in z; "all": every boundary node fixed in all three directions; "clamp": x = 0 clamped.  No point loads."""
    from stan_amd import problem
    from stan_amd.cube import cube_mesh
    xyz, conn = cube_mesh(n)
    ijk = np.rint(xyz).astype(np.int64)
    inner = ((ijk > 0) & (ijk < n)).all(axis=1)
    xyz = xyz.copy()
    xyz[inner] += np.random.default_rng(77 + n).uniform(-jitter, jitter, (int(inner.sum()), 3))
    if supports == "sym":
        flags = (ijk == 0).astype(np.float64)
    elif supports == "all":
        flags = np.repeat((~inner)[:, None], 3, axis=1).astype(np.float64)
    else:
        flags = np.repeat((ijk[:, 0] == 0)[:, None], 3, axis=1).astype(np.float64)
    spc = np.nonzero(flags.any(axis=1))[0].astype(np.int32)
    none = np.zeros(0, dtype=np.int32)
    return problem.make_job(xyz, conn, spc, flags[spc], none, np.zeros((0, 3)))


def grad_max(m):
    """max |d N_i / d x_c| over the elements and the 2x2x2 points and corners of every element"""
    X = m.xyz[m.conn]
    worst = 0.0
    for gl in (GL, 1.0):
        for g in range(8):
            d = _dnl([SX[g] * gl, SY[g] * gl, SZ[g] * gl], np.float64)
            gr = np.linalg.inv(_jac(X, d)) @ d.T                   # [ne, 3, 8]
            worst = max(worst, float(np.abs(gr).max()))
    return worst


def cube_face(n, f):
    """(face_elem, face_id) of the boundary face f of the n^3 cube of cube_mesh (elements x fastest)."""
    e = np.arange(n ** 3)
    idx = [e % n, (e // n) % n, e // (n * n)][f // 2]
    el = e[idx == (n - 1 if f & 1 else 0)]
    return el, np.full(el.size, f)
