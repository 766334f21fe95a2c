"""Linear buckling on the CPU: the numpy restatement of tests/buckling_ref.py -- the element scalars of
the geometric stiffness, the ordered gather, the driver loop with exact solves -- held to closed forms and to
scipy.linalg.eigh(H, K).  The GPU tests (tests/test_gpu_buckling.py) hold the device to this restatement.

Measured on the development host (printed again by every run):
  the fp64 restatement of the element scalars against longdouble over the conditioning family x the three fields x both element
  types: 0.364 units of 2^-52 S at worst (the random field on the stretched, rotated elements of "aspect_rot_shift_union");
  lowest factor of the clamped column over Euler's pi^2 E I / 4 L^2 at nz = 10, 20, 40: 1.4939, 1.1187, 1.0251;
  outer steps of the restatement at tol 1e-6 (k = 4): column 10, jittered cube 51, cantilever 48, the same with every solve
  perturbed at 1e-3 relative; factors within 5e-12 relative of eigh's."""
import numpy as np
import pytest

from tests import buckling_ref as B
from tests import element_ref as E

U53 = 2.0 ** -53
TOL = 1e-6


# ---- the element scalars ------------------------------------------------------------------------------------------------------
def test_unit_cube_under_uniform_stress_is_the_tensor_product():
    """sigma_xx = s0 alone (nu = 0, u_x = e0 x): s = s0 Kx (x) My (x) Mz, the 1-D stiffness in x and the 1-D masses in y, z."""
    Em, e0 = 210000.0, 1e-3
    u = np.zeros((1, 8, 3))
    u[0, :, 0] = e0 * E.UNIT[:, 0]
    s, _ = B.kg(E.F64, E.UNIT[None], u, Em, 0.0, E.G2)
    K1, M1 = np.array([[1.0, -1.0], [-1.0, 1.0]]), np.array([[1.0 / 3, 1.0 / 6], [1.0 / 6, 1.0 / 3]])
    ix, iy, iz = (E.UNIT[:, c].astype(int) for c in range(3))
    exact = Em * e0 * K1[np.ix_(ix, ix)] * M1[np.ix_(iy, iy)] * M1[np.ix_(iz, iz)]
    err = np.abs(s[0] - exact).max(axis=1) / (U53 * np.abs(exact).sum(axis=1))
    print("uniform stress: %.2f units of 2^-53 of the row's absolute sum" % err.max())
    assert err.max() <= 8.0


@pytest.mark.parametrize("etype", (E.G1, E.G2))
def test_translation_symmetry_zero_and_scaling(etype):
    worst_row, worst_sym = 0.0, 0.0
    for name, X in E.geometries().items():
        u = E.fields(X)["random"]
        Em, nu = E.REC_MATERIAL
        s, S = B.kg(E.F64, X, u, Em, nu, etype)
        S = np.asarray(S, dtype=np.float64)
        # a translation: every row sums to 0, to the roundings of its terms and of the sum
        worst_row = max(worst_row, float((np.abs(s.sum(axis=2)) / (E.U52 * S.sum(axis=2))).max()))
        worst_sym = max(worst_sym, float((np.abs(s - s.transpose(0, 2, 1)) / (E.U52 * S)).max()))
        z, _ = B.kg(E.F64, X, np.zeros_like(u), Em, nu, etype)
        assert not z.any(), name                                           # U = 0: G = 0 exactly
        s2, _ = B.kg(E.F64, X, 2.0 * u, Em, nu, etype)
        assert np.array_equal((2.0 * s).view(np.int64), s2.view(np.int64)), name    # G(2U) = 2 G(U) to the bit
    print("type %d: row sums %.3f, asymmetry %.3f units of 2^-52 S" % (etype, worst_row, worst_sym))
    assert worst_row <= 2.0 and worst_sym <= 2.0


def test_fp64_restatement_against_longdouble():
    worst = 0.0
    for name, X in E.geometries().items():
        for fname, u in E.fields(X).items():
            for t in (E.G1, E.G2):
                ref, S = B.kg(E.LD, X, u, *E.REC_MATERIAL, t)
                got, _ = B.kg(E.F64, X, u, *E.REC_MATERIAL, t)
                worst = max(worst, E.units(got, ref, S))
    print("fp64 restatement of the element scalars: %.3f units (recorded %.2f)" % (worst, B.KG_F64_UNITS_MEASURED))
    assert worst <= 2 * B.KG_F64_UNITS_MEASURED


def test_ordered_gather_against_a_dense_scatter():
    j = B.cube4j_job()
    disp = np.random.default_rng(3).standard_normal(j.xyz.shape) * 1e-3
    s, _ = B.element_scalars(E.F64, j, disp)
    Gn = B.gather_nodes(j, s)
    ref = np.zeros_like(Gn, dtype=np.longdouble)
    for a in range(8):
        for b in range(8):
            np.add.at(ref, (j.conn[:, a], j.conn[:, b]), s[:, a, b].astype(np.longdouble))
    mag = np.zeros_like(Gn)
    for a in range(8):
        for b in range(8):
            np.add.at(mag, (j.conn[:, a], j.conn[:, b]), np.abs(s[:, a, b]))
    assert (np.abs(Gn - ref) <= 8 * U53 * mag).all()
    Gd = B.dense_reduced(j, Gn)
    assert Gd.shape == (j.n_red, j.n_red) and np.abs(Gd - Gd.T).max() <= 64 * U53 * np.abs(Gd).max()


# ---- Euler's column -----------------------------------------------------------------------------------------------------------
_column = {}


def _column_model(nz):
    if nz not in _column:
        j = B.column_job(nz)
        Kd, Hd, U = B.cpu_matrices(j)
        _column[nz] = (j, Kd, Hd, B.eigh_ref(Hd, Kd))
    return _column[nz]


def test_column_approaches_eulers_load_from_above():
    ratios = [1.0 / _column_model(nz)[3][0][0] / B.euler_load() for nz in (10, 20, 40)]      # (a unit end load)
    print("lowest factor over pi^2 E I / 4 L^2 at nz = 10, 20, 40: %.4f %.4f %.4f" % tuple(ratios))
    assert ratios[0] > ratios[1] > ratios[2]
    assert 0.99 <= ratios[2] <= 1.05


# ---- the driver against eigh --------------------------------------------------------------------------------------------------
def _models():
    return {"column": lambda: _column_model(10)[:3], "cube4j": lambda: (lambda j: (j,) + B.cpu_matrices(j)[:2])(B.cube4j_job()),
            "cantilever": lambda: (lambda j: (j,) + B.cpu_matrices(j)[:2])(B.cantilever_job())}


@pytest.mark.parametrize("name", ("column", "cube4j", "cantilever"))
def test_restatement_reproduces_eigh(name):
    j, Kd, Hd = _models()[name]()
    mu_ref, Phi, low = B.eigh_ref(Hd, Kd)
    k = B.pick_k(mu_ref)
    r = B.restatement(Kd, Hd, k, tol=TOL, max_outer=150)
    rp = B.restatement(Kd, Hd, k, tol=TOL, max_outer=150, perturb=1e-3)
    print(name, "N", Kd.shape[0], "k", k, "outer", r["outer"], "perturbed", rp["outer"], "factors", r["factor"],
          "rel err", np.abs(r["mu"] / mu_ref[:k] - 1).max())
    assert r["converged"] and rp["converged"] and r["n_positive"] >= k
    assert abs(rp["outer"] - r["outer"]) <= 2          # the correction form: an inexact solve costs no outer step
    assert (r["rho"] <= TOL).all() and (np.diff(r["factor"]) >= 0).all()
    bound, rn = B.residual_bound(Kd, Hd, r["mu"], r["phi"])
    assert (np.abs(r["mu"] - mu_ref[:k]) <= bound + 8 * U53 * np.abs(mu_ref[:k])).all(), (r["mu"], mu_ref[:k], bound)
    for a, b, gap in B.clusters(mu_ref, k):
        s = B.sin_max_angle_K(r["phi"][a:b].T, Phi[:, a:b], Kd)
        assert s <= 2 * rn[a:b].max() / gap, (a, b, s)
    for x in r["phi"]:
        assert x.max() == 1.0 and np.abs(x).max() == 1.0
    if name == "column":            # an exactly degenerate pair (bending about x and about y)
        assert B.clusters(mu_ref, k)[0][:2] == (0, 2)
    if name == "cantilever":        # a transverse load: the spectrum is symmetric in sign
        assert abs(low + mu_ref[0]) <= 1e-9 * mu_ref[0]
        assert abs(r["lowest_negative_factor"] + r["factor"][0]) <= 1e-8 * r["factor"][0]
    # the most negative Ritz value lies inside the spectrum and tells the reference's sign: 1 / it >= eigh's lowest mu
    if low < 0 and r["block"] > r["n_positive"]:
        assert r["lowest_negative_factor"] < 0.0 and 1.0 / r["lowest_negative_factor"] >= low * (1 + 1e-9)
    if low >= 0:
        assert r["lowest_negative_factor"] == 0.0
