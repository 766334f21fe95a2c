"""Reference for the result scalars (stan_hip_result_scalars_hex8): a literal restatement of Part.Load_Scalar
(Part.cs:301-391 cell scalars, :431-521 point scalars) in numpy.  Principals come from numpy.linalg.eigvalsh (the
reference calls MathNet's Evd), every sum is a sequential Python-order sum (LINQ Average = sum in order / count), max and
min keep the first of equals as LINQ's do, N.EList is the node's incident elements in element order with duplicates
removed (Database.cs:149-158, RemoveElemDuplicates) and the corner is NList.IndexOf(N.ID): the FIRST position.

Also here: the eigenvalue yardstick family and the bound the device is held to."""
import re
import struct

import numpy as np

N_SCALARS = 24
COPIED = [0, 1, 2] + list(range(4, 10)) + list(range(14, 20))     # displacement X Y Z, stress and strain components
DERIVED_STRESS, DERIVED_STRAIN = [10, 11, 12, 13], [20, 21, 22, 23]
NAMES = ["Displacement X", "Displacement Y", "Displacement Z", "Total Displacement",
         "Stress XX", "Stress YY", "Stress ZZ", "Stress XY", "Stress YZ", "Stress XZ",
         "Stress P1", "Stress P2", "Stress P3", "von Mises Stress",
         "Strain XX", "Strain YY", "Strain ZZ", "Strain XY", "Strain YZ", "Strain XZ",
         "Strain P1", "Strain P2", "Strain P3", "Effective Strain"]          # Part.cs:403-428

UNIT = 2.0 ** -52     # errors of eigenvalues are counted in units of 2^-52 ||S||_F
# Worst error of numpy.linalg.eigvalsh (LAPACK) over yardstick_family(), against mpmath at 50 digits, in those units:
# measured 3.16 on the development host (tests/test_result_scalars.py measures it again on every run and asserts it stays
# under 8, so that this yardstick cannot rot).  For comparison, over the same family: cyclic Jacobi with 6 sweeps (what the
# device runs, emulated in Python without FMA) 1.5; the trigonometric closed form misses by 3.5e7.
EIGVALSH_UNITS_MEASURED = 3.16
# What the device is held to, against eigvalsh: 4 x the measured value.  The margin covers FMA contraction and another
# rotation order; the closed form misses by seven orders of magnitude, so any margin below 1e6 still tells the two apart.
DEVICE_UNITS = 4 * EIGVALSH_UNITS_MEASURED


def tensor(v6):
    """3x3 from xx, yy, zz, xy, yz, xz (Part.cs:333-341; the shear strain as stored, not halved)."""
    xx, yy, zz, xy, yz, xz = v6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def fro(v6):
    """||S||_F of the tensor of v6 (leading dimensions kept)."""
    v6 = np.asarray(v6, dtype=np.float64)
    return np.sqrt((v6[..., :3] ** 2).sum(-1) + 2 * (v6[..., 3:] ** 2).sum(-1))


def yardstick_family(seed=12345):
    """[n, 6] tensors as xx, yy, zz, xy, yz, xz: 300 random symmetric at scales 1e-3 .. 1e5, 100 with two eigenvalues
    1e-6 .. 1e-14 apart, 100 within 1e-6 .. 1e-14 of hydrostatic, the zero tensor, diag(3, 3, 3), a uniaxial tensor, a
    pure shear, diag(1, 1, -2)."""
    rng = np.random.default_rng(seed)

    def six(S):
        S = 0.5 * (S + S.T)
        return [S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[1, 2], S[0, 2]]

    out = []
    for _ in range(300):
        out.append(six(rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-3, 5)))
    for _ in range(100):
        Q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        a, b = rng.standard_normal(2) * 10.0 ** rng.uniform(-1, 3)
        gap = abs(a) * 10.0 ** rng.uniform(-14, -6)
        out.append(six(Q @ np.diag([a, a + gap, b]) @ Q.T))
    for _ in range(100):
        p = rng.standard_normal() * 10.0 ** rng.uniform(-1, 3)
        out.append(six(p * np.eye(3) + abs(p) * 10.0 ** rng.uniform(-14, -6) * rng.standard_normal((3, 3))))
    out += [[0, 0, 0, 0, 0, 0], [3, 3, 3, 0, 0, 0], [250.0, 0, 0, 0, 0, 0], [0, 0, 0, 40.0, 0, 0], [1, 1, -2, 0, 0, 0]]
    return np.array(out, dtype=np.float64)


def exact_eigenvalues(v6):
    """Descending eigenvalues of one tensor with mpmath at 50 digits (as mpmath numbers)."""
    import mpmath as mp
    with mp.workdps(50):
        E = mp.eigsy(mp.matrix(tensor([mp.mpf(float(x)) for x in v6]).tolist()), eigvals_only=True)
        return sorted([+e for e in E], reverse=True)


def worst_units(v6s, eig_fn):
    """max over the tensors of |eig_fn(v6) - exact| / (2^-52 ||S||_F) (tensors of norm 0 must come out exactly 0)."""
    import mpmath as mp
    worst = 0.0
    for v6 in v6s:
        got = eig_fn(v6)
        want = exact_eigenvalues(v6)
        nrm = fro(v6)
        for g, w in zip(got, want):
            with mp.workdps(50):
                err = float(abs(mp.mpf(float(g)) - w))
            if nrm == 0:
                assert err == 0
            else:
                worst = max(worst, err / (UNIT * nrm))
    return worst


def principals(v6):
    """P1 >= P2 >= P3 as the reference takes them from Evd (ascending, read backwards: Part.cs:343-346)."""
    w = np.linalg.eigvalsh(tensor(v6))
    return w[2], w[1], w[0]


def corner(u, eps6, sig6):
    """The 24 values of one (element, node) corner, Part.cs:318-379."""
    v = [0.0] * N_SCALARS
    v[0], v[1], v[2] = float(u[0]), float(u[1]), float(u[2])
    v[3] = float(np.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2))
    for base, t6 in ((4, sig6), (14, eps6)):
        for c in range(6):
            v[base + c] = float(t6[c])
        P1, P2, P3 = principals(t6)
        v[base + 6], v[base + 7], v[base + 8] = float(P1), float(P2), float(P3)
        v[base + 9] = float(np.sqrt(((P1 - P2) ** 2 + (P2 - P3) ** 2 + (P3 - P1) ** 2) / 2))
    v[23] = (2.0 / 3.0) * v[23]
    return v


def _seq_sum(xs):
    s = 0.0
    for x in xs:
        s = s + x
    return s


def _first_max(xs):
    m = xs[0]
    for x in xs[1:]:
        if x > m:
            m = x
    return m


def _first_min(xs):
    m = xs[0]
    for x in xs[1:]:
        if x < m:
            m = x
    return m


class Reference:
    """All 24 scalars of a model: .corners [n_elem, 8, 24], .norms [n_elem, 8, 2] (||stress||_F, ||strain||_F),
    .cell [24, 3, n_elem] (max, average, min), .point [24, n_nodes], and for the error bounds .cell_norm [2, n_elem] /
    .point_norm [2, n_nodes]: the largest tensor norm entering that output (stress, strain)."""

    def __init__(self, disp, conn, strain, stress):
        disp = np.asarray(disp, dtype=np.float64).reshape(-1, 3)
        conn = np.asarray(conn).reshape(-1, 8)
        strain = np.asarray(strain, dtype=np.float64).reshape(-1, 8, 6)
        stress = np.asarray(stress, dtype=np.float64).reshape(-1, 8, 6)
        ne, nn = conn.shape[0], disp.shape[0]
        self.corners = np.zeros((ne, 8, N_SCALARS))
        for e in range(ne):
            for i in range(8):
                self.corners[e, i] = corner(disp[conn[e, i]], strain[e, i], stress[e, i])
        self.norms = np.stack([fro(stress), fro(strain)], axis=-1)
        self.cell = np.zeros((N_SCALARS, 3, ne))
        for e in range(ne):
            for s in range(N_SCALARS):
                vals = [float(x) for x in self.corners[e, :, s]]
                self.cell[s, 0, e] = _first_max(vals)
                self.cell[s, 1, e] = _seq_sum(vals) / 8          # LINQ Average
                self.cell[s, 2, e] = _first_min(vals)
        self.cell_norm = self.norms.max(axis=1).T if ne else np.zeros((2, 0))
        # N.EList: incident elements in element order, each once; the corner is NList.IndexOf(N.ID)
        elist = [[] for _ in range(nn)]
        for e in range(ne):
            for i in range(8):
                n = int(conn[e, i])
                if not elist[n] or elist[n][-1][0] != e:
                    elist[n].append((e, i))
        self.elist = elist
        self.point = np.zeros((N_SCALARS, nn))
        self.point_norm = np.zeros((2, nn))
        for n in range(nn):
            if not elist[n]:
                continue      # the reference divides by zero here; the library defines 0
            for s in range(N_SCALARS):
                self.point[s, n] = _seq_sum([float(self.corners[e, i, s]) for e, i in elist[n]]) / len(elist[n])
            self.point_norm[:, n] = np.max([self.norms[e, i] for e, i in elist[n]], axis=0)


def ulp_diff(a, b):
    """Distance in units in the last place between two float64 arrays of the same sign pattern."""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


def check_against(ref, sel, point, cell):
    """The assertions of the issue for outputs `point` [n_sel, n_nodes] / `cell` [n_sel, 3, n_elem] (either None) of the
    selection `sel` against a Reference.  Returns the worst derived-scalar error seen, in units of 2^-52 ||S||_F."""
    worst = 0.0
    for k, s in enumerate(sel):
        pairs = []
        if point is not None:
            pairs.append((point[k], ref.point[s], ref.point_norm))
        if cell is not None:
            pairs += [(cell[k, j], ref.cell[s, j], ref.cell_norm) for j in range(3)]
        for got, want, norm in pairs:
            assert np.isfinite(got).all(), NAMES[s]
            if s in COPIED:
                assert np.array_equal(got.view(np.int64), want.view(np.int64)), NAMES[s]       # bit-equal, signed zeros too
            elif s == 3:
                assert (ulp_diff(got, want) <= 4).all(), NAMES[s]
            else:
                nrm = norm[0 if s in DERIVED_STRESS else 1]
                err = np.abs(got - want)
                assert (err <= DEVICE_UNITS * UNIT * nrm).all(), (NAMES[s], float((err / np.where(nrm > 0, UNIT * nrm, 1)).max()))
                if nrm.size and (nrm > 0).any():
                    worst = max(worst, float((err[nrm > 0] / (UNIT * nrm[nrm > 0])).max()))
    for base in (10, 20):     # P1 >= P2 >= P3 everywhere
        if all(b in sel for b in (base, base + 1, base + 2)):
            i1, i2, i3 = (list(sel).index(b) for b in (base, base + 1, base + 2))
            # (ordered corner by corner; max, min and the sequential sums are monotone, so every output is ordered too)
            for out in ([point] if point is not None else []) + ([cell[:, j] for j in range(3)] if cell is not None else []):
                assert (out[i1] >= out[i2]).all() and (out[i2] >= out[i3]).all()
    return worst


def parse_vtu(path):
    """A .vtu as stan_host_write_vtu writes it: the XML head up to the `_` of the appended block, then the UInt64-prefixed
    arrays by offset.  Returns (attributes of VTKFile, attributes of Piece, {section: [(name, array), ...]})."""
    raw = open(path, "rb").read()
    m = re.search(rb"<AppendedData encoding=\"raw\">\s*_", raw)
    assert m, "no appended raw block"
    head, blob = raw[:m.end()].decode(), raw[m.end():]
    assert blob.rstrip().endswith(b"</VTKFile>") and b"</AppendedData>" in blob[-64:]
    vtk = dict(re.findall(r'(\w+)="([^"]*)"', re.search(r"<VTKFile([^>]*)>", head).group(1)))
    piece = dict(re.findall(r'(\w+)="([^"]*)"', re.search(r"<Piece([^>]*)>", head).group(1)))
    dt = {"Float64": "<f8", "Float32": "<f4", "Int64": "<i8", "UInt8": "u1"}
    out = {}
    for sec in ("Points", "Cells", "PointData", "CellData"):
        body = re.search(r"<%s>(.*?)</%s>" % (sec, sec), head, flags=re.S).group(1)
        out[sec] = []
        for a in re.findall(r"<DataArray([^>]*)/>", body):
            at = dict(re.findall(r'(\w+)="([^"]*)"', a))
            assert at["format"] == "appended"
            off = int(at["offset"])
            nbytes = struct.unpack("<Q", blob[off:off + 8])[0]
            out[sec].append((at.get("Name"), np.frombuffer(blob[off + 8:off + 8 + nbytes], dtype=dt[at["type"]]), at))
    return vtk, piece, out
