"""Reference for the consistent mass (stan_hip_mass_hex8_batch, stan_hip_consistent_mass_hex8, stan_hip_matrix_axpy,
stan_hip_modes_pencil).

  mass(T, X, rho)            (m, S) [e, 8, 8]: the element scalars m[a][b] = rho sum_g N_a(q_g) N_b(q_g) det J_g over the 2 x 2 x 2
                             rule (both element types) over a number type of tests/element_ref.py (LD: the reference, F64: the
                             plain-fp64 restatement) with their rounding scale
  lumped_rows(T, X, rho)     [e, 8]: rho sum_g N_a(q_g) det J_g, the element's contribution to the row-sum lumped mass
  unit_cube()                [8, 8]: 2^(3 - d) / 216, d the number of coordinates in which corners a and b differ
  element_scalars(T, j, rho) mass() over a job with its materials' densities
  dense_mass(j, rho)         (M_c dense on the free DOFs, m [n_elem, 8, 8]) in plain fp64 through tests/buckling_ref.py's ordered
                             gather
  MODELS, K_MODES            the models of the pencil tests and the number of modes asked of each
  cpu_pencil(name)           dict(Kd, Md, lam_ref, Phi): the CPU oracle's K, dense_mass and scipy.linalg.eigh(K, M_c), once
  restatement(Kd, Md, k, ...)  the driver loop of api_buckling.hip with H = +M_c line by line in numpy with exact inner solves
                             (tests/buckling_ref.py's, which takes any H) and the final scaling to phi^T M_c phi = 1
  normalise(X, Md)           that scaling: M_c-norm 1, the entry of largest magnitude positive (lowest index on a tie)"""
import numpy as np
import scipy.linalg

from tests import buckling_ref as B
from tests import element_ref as E
from tests import modes_ref as MR

U53 = 2.0 ** -53
# Worst error of the plain-fp64 restatement mass(F64, ...) against mass(LD, ...) over E.geometries(), in units of 2^-52 S
# (E.units): measured on the development host (2.77 on the stretched and rotated elements of "aspect_rot_shift_union", 2.65 on
# "aspect_rot", where the six triple products of det J cancel; at most 0.55 on every other group); tests/test_mass.py measures
# it again on every run and asserts that it stays under twice this value.  What the device is held to: 4 x the measured value
# (FMA contraction and the butterfly order of the Gauss-point sum move the constant by a small factor) -- the margin of the
# element tests (tests/element_ref.py).  The device reads 2.926 at worst (tests/test_gpu_consistent_mass.py).
MASS_F64_UNITS_MEASURED = 2.78
DEVICE_MASS_UNITS = 4 * MASS_F64_UNITS_MEASURED


def shape_values(T, g):
    """N_a at Gauss point g of the 2 x 2 x 2 rule: [8], 1/8 prod over the axes of (1 + s_a s_g sqrt(1/3)) as hex8_shape."""
    s = T.arr(E.SGN)
    f = 1 + s * (T.arr(E.SGN[g]) * E.gauss_loc(T, E.G2))[None, :]
    return 0.125 * f[:, 0] * f[:, 1] * f[:, 2]


def mass(T, X, rho):
    """(m, S).  The scale is the product rule with absolute values over the terms of det J (ddet of E.gauss_points, which holds
    the determinant's own rounding) plus one relative rounding each for N_a, N_b and the term: S = rho sum_g N_a N_b (ddet_g +
    3 |det_g|).  rho: a scalar or [e]."""
    X = T.arr(X)
    rho = np.broadcast_to(T.arr(rho), (X.shape[0],))[:, None, None]
    m, S = 0, 0
    for g, q in enumerate(E.gauss_points(T, X, E.G2)):
        N = shape_values(T, g)
        NN = (N[:, None] * N[None, :])[None, :, :]
        m = m + NN * q["det"][:, None, None]
        S = S + abs(NN) * (q["ddet"] + 3 * abs(q["det"]))[:, None, None]
    return rho * m, abs(rho) * S


def lumped_rows(T, X, rho):
    X = T.arr(X)
    rho = np.broadcast_to(T.arr(rho), (X.shape[0],))[:, None]
    out = 0
    for g, q in enumerate(E.gauss_points(T, X, E.G2)):
        out = out + shape_values(T, g)[None, :] * q["det"][:, None]
    return rho * out


def unit_cube():
    d = (E.SGN[:, None, :] != E.SGN[None, :, :]).sum(axis=2)
    return 2.0 ** (3 - d) / 216.0


def element_scalars(T, j, rho):
    return mass(T, j.xyz[j.conn], np.asarray(rho, dtype=np.float64)[np.asarray(j.elem_mat)])


def dense_mass(j, rho):
    m = np.asarray(element_scalars(E.F64, j, rho)[0], dtype=np.float64)
    return B.dense_reduced(j, B.gather_nodes(j, m)), m


# ---- the pencil ---------------------------------------------------------------------------------------------------------------
MODELS = MR.MODELS
# the modes asked of each model: MR.pick_k's rule on the pencil's own spectrum (the smallest k >= 6 with a relative gap > 1e-3
# behind it), found on the CPU (tests/test_mass.py checks the rule and the restatement's outer counts on every run)
K_MODES = {"cube6": 6, "cube6j": 6, "perforated12": 6, "two_mat": 6}
# outer steps the restatement (exact solves) takes at tol 1e-6, measured on the CPU: the device gets these + 3
RESTATEMENT_OUTER = {"cube6": 15, "cube6j": 15, "perforated12": 16, "two_mat": 14}
_cpu = {}


def normalise(X, Md):
    out = np.empty_like(X)
    for j, x in enumerate(X):
        x = x / np.sqrt(x @ (Md @ x))
        i = int(np.argmax(np.abs(x)))
        out[j] = -x if x[i] < 0 else x
    return out


def eigh_ref(Kd, Md, n_ref=MR.N_REF):
    """(lambda ascending, Phi [N, n_ref] M_c-orthonormal columns) of K phi = lambda M_c phi"""
    return scipy.linalg.eigh(Kd, 0.5 * (Md + Md.T), subset_by_index=[0, min(n_ref, Kd.shape[0]) - 1])


def cpu_pencil(name):
    if name not in _cpu:
        from oracle import pyoracle as O
        from tests import product_ref as P
        j = MR.job(name)
        rc, A = O.assemble(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
        assert rc == 0
        Kd = MR.dense(*P.full_csr(A))
        Md = dense_mass(j, MR.mat_rho(name))[0]
        lam, Phi = eigh_ref(Kd, Md)
        _cpu[name] = dict(Kd=Kd, Md=Md, lam_ref=lam, Phi=Phi)
    return _cpu[name]


def restatement(Kd, Md, k, tol=1e-6, max_outer=100):
    """dict(lam ascending, phi [k, N], rho, outer, converged, block, n_positive): B.restatement on the pencil (M_c, K) -- its mu
    are 1 / lambda -- and the final scaling."""
    r = B.restatement(Kd, Md, k, tol=tol, max_outer=max_outer)
    phi = r["phi"]
    return dict(lam=1.0 / r["mu"], phi=normalise(phi, Md) if phi.shape[0] else phi, rho=r["rho"], outer=r["outer"],
                converged=r["converged"], block=r["block"], n_positive=r["n_positive"])


def orthonormality(phi, Md):
    """max |Phi^T M_c Phi - I| of the rows of phi"""
    return float(np.abs(phi @ Md @ phi.T - np.eye(phi.shape[0])).max())
