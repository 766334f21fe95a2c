"""The consistent mass on the CPU: the restatement of tests/mass_ref.py against closed forms, against
the lumped mass, its plain-fp64 form against np.longdouble (the yardstick of the device test), and the restated pencil driver
with exact solves against scipy.linalg.eigh(K, M_c) on the models of tests/test_gpu_consistent_mass.py."""
import numpy as np
import pytest

from tests import element_ref as E
from tests import mass_ref as M
from tests import modes_ref as MR
from tests.util import UNIT

LD = np.longdouble


def _parallelepipeds(n=12, seed=4):
    """UNIT under random affine maps of positive determinant: (X [n, 8, 3], volume [n])"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, 3, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1, 1))
    A[np.linalg.det(A) < 0, 0] *= -1.0
    t = rng.standard_normal((n, 1, 3)) * 10.0
    X = np.einsum("kj,nij->nki", UNIT, A) + t
    return X, np.linalg.det(A.astype(LD).astype(np.float64))


def test_unit_cube_and_parallelepipeds():
    """m[a][b] = rho V 2^(3 - d) / 216: the 2 x 2 x 2 rule is exact where det J is constant."""
    want = M.unit_cube()
    assert abs(want.sum() - 1.0) <= 1e-15 and want[0, 0] == 8.0 / 216.0 and want[0, 6] == 1.0 / 216.0      # corners 0 and 6: opposite
    want = (want * 216.0).astype(LD) / 216                           # 2^(3 - d) is exact; one rounding in the working type
    m, _ = M.mass(E.LD, UNIT[None], 1.0)
    assert (np.abs(m[0] - want) <= 32 * np.finfo(LD).eps * want).all()  # 8 points x (sqrt(1/3), three factors, a product) each
    X, vol = _parallelepipeds()
    rho = 7.85e-9
    m, S = M.mass(E.LD, X, rho)
    ref = rho * vol.astype(LD)[:, None, None] * want[None]
    # the volume here is a float64 determinant of the map (1e-15 relative); the coordinates were rounded once (the scale S)
    assert (np.abs(m - ref) <= 4 * E.U52 * S + 1e-14 * np.abs(ref)).all()
    assert np.array_equal(m, m.transpose(0, 2, 1))


def test_sums_are_the_mass_and_the_lumped_rows():
    rho = 2.5
    for name, X in E.geometries().items():
        m, S = M.mass(E.LD, X, rho)
        rows = M.lumped_rows(E.LD, X, rho)
        # sum_b N_b = 1 at every point: the row sums are the lumped contributions, term by term
        assert (np.abs(m.sum(axis=2) - rows) <= E.U52 * S.sum(axis=2) * 2.0 ** -8).all(), name
        # and their sum is rho V, V = sum_g det J_g
        vol = sum(q["det"] for q in E.gauss_points(E.LD, E.LD.arr(X), E.G2))
        assert (np.abs(m.sum(axis=(1, 2)) - rho * vol) <= E.U52 * S.sum(axis=(1, 2)) * 2.0 ** -8).all(), name


def test_fp64_restatement_against_longdouble():
    """The yardstick of the device test: what the same formulas read in plain fp64, in units of the rounding scale."""
    worst = (0.0, None)
    for name, X in E.geometries().items():
        ref, S = M.mass(E.LD, X, MR.RHO)
        un = E.units(M.mass(E.F64, X, MR.RHO)[0], ref, S)
        print("mass %-24s fp64 restatement %.3f units" % (name, un))
        if un > worst[0]:
            worst = (un, name)
    print("worst %.3f at %s; recorded %.2f" % (worst[0], worst[1], M.MASS_F64_UNITS_MEASURED))
    assert worst[0] <= 2 * M.MASS_F64_UNITS_MEASURED and worst[0] >= 0.5 * M.MASS_F64_UNITS_MEASURED, worst


def test_a_one_point_rule_would_be_singular():
    """Why both element types take the 2 x 2 x 2 rule: the one-point mass of an element has rank 1."""
    N0 = np.full(8, 0.125)
    assert np.linalg.matrix_rank(np.outer(N0, N0) * 8.0) == 1
    assert np.linalg.matrix_rank(M.unit_cube()) == 8


@pytest.mark.parametrize("name", M.MODELS)
def test_restated_pencil_driver_against_eigh(name):
    """The loop of stan_hip_modes_pencil with exact solves converges on every model of the device test within the recorded
    outer count, and its eigenvalues are scipy's."""
    c = M.cpu_pencil(name)
    Kd, Md, lam_ref = c["Kd"], c["Md"], c["lam_ref"]
    assert np.array_equal(Md, Md.T) and np.linalg.eigvalsh(Md)[0] > 0
    k = M.K_MODES[name]
    assert k == MR.pick_k(lam_ref)
    r = M.restatement(Kd, Md, k, tol=1e-6, max_outer=100)
    print(name, "N", Kd.shape[0], "k", k, "outer", r["outer"], "orthonormality", M.orthonormality(r["phi"], Md))
    assert r["converged"] and r["outer"] <= M.RESTATEMENT_OUTER[name] and r["n_positive"] == r["block"]
    assert (r["rho"] <= 1e-6).all() and (np.diff(r["lam"]) >= 0).all()
    # rho is a relative residual: the eigenvalue error is of second order in it
    assert (np.abs(r["lam"] - lam_ref[:k]) <= 1e-9 * lam_ref[:k]).all()
    assert M.orthonormality(r["phi"], Md) <= 1e-9      # (the Ritz vectors are M_c-orthogonal up to the Jacobi sweep's rounding)
    for x in r["phi"]:
        assert x[int(np.argmax(np.abs(x)))] > 0


def test_restated_pencil_on_the_shifted_free_cube():
    """The free-free 4^3 cube through K + sigma M_c at sigma = lambda_7: six values are sigma itself, the restatement converges
    at k = 8 (the relative gap behind it is 0.39) in the 23 outer steps the device test allows for."""
    import scipy.linalg
    from oracle import pyoracle as O
    from tests import product_ref as P
    from tests import transient_ref as T
    j = T.job(T.FREE)
    rc, A = O.assemble(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    assert rc == 0
    Kd, Md = MR.dense(*P.full_csr(A)), M.dense_mass(j, T.mat_rho(T.FREE))[0]
    lam = scipy.linalg.eigh(Kd, Md, eigvals_only=True)
    sigma = lam[6]
    assert (np.abs(lam[:6]) <= 1e-10 * sigma).all() and (lam[8] - lam[7]) / (lam[7] + sigma) > 1e-3
    r = M.restatement(Kd + sigma * Md, Md, 8, tol=1e-6, max_outer=100)
    print("free cube: outer", r["outer"], "lambda - sigma", r["lam"] - sigma)
    assert r["converged"] and r["outer"] <= 23
    assert (np.abs(r["lam"][:6] - sigma) <= 2e-6 * sigma).all() and (np.abs(r["lam"][6:] - sigma - lam[6:8]) <= 1e-9 * sigma).all()
