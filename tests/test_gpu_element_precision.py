"""The element kernels against the extended-precision reference of tests/element_ref.py, on the conditioning family: k_ke_batch,
the assembled K through k_numeric, the colour scatter and k_numeric_wide, and k_recover.

Every comparison is entrywise |device - reference| <= DEVICE_*_UNITS x 2^-52 x S with the reference's rounding scale S, and
finite.  The bounds are 4 x what the oracle measures over the same family (element_ref.ORACLE_*_UNITS_MEASURED, measured again
by tests/test_element_ref.py on every run); none is chosen here.  Each test prints the worst units it saw: that is the
number to read.  The exact properties at the end (powers of two go through bit for bit) need no reference."""
import os
import re

import numpy as np
import pytest

from stan_amd import problem
from stan_amd.cube import cube_bcs, cube_mesh, revolved_mesh
from tests import element_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_ASSEMBLY_MODE = 5
GROUPS = list(R.family())
FIELDS = ("random", "rigid", "affine")


# ---- k_ke_batch -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GROUPS)
def test_ke_batch_against_the_reference(gpu_ctx, name):
    """One call per (E, nu): the part's elements as HEX8_G2, again as HEX8_G1, and the first once more as HEX8_G1 -- 2 k + 1
    elements, never a multiple of 64, a HEX8_G1 element last."""
    worst = {R.G1: 0.0, R.G2: 0.0}
    for (X, E, nu, K2, S2), (_X, _E, _nu, K1, S1) in zip(R.ke_reference(name, R.G2), R.ke_reference(name, R.G1)):
        k = X.shape[0]
        types = np.array([R.G2] * k + [R.G1] * (k + 1), dtype=np.uint8)
        got = gpu_ctx.ke_hex8_batch(np.concatenate([X, X, X[:1]]), E, nu, types)
        assert got.shape == (2 * k + 1, 24, 24) and (2 * k + 1) % 64 and types[-1] == R.G1
        assert np.array_equal(got[-1], got[k])                       # the same element in another workgroup: the same bits
        worst[R.G2] = max(worst[R.G2], R.units(got[:k], K2, S2))
        worst[R.G1] = max(worst[R.G1], R.units(got[k:2 * k], K1, S1))
    print("k_ke_batch %s: worst %.3f (G2) %.3f (G1) units of 2^-52 S (bound %.2f)" % (name, worst[R.G2], worst[R.G1], R.DEVICE_KE_UNITS))
    assert max(worst.values()) <= R.DEVICE_KE_UNITS


# ---- the assembled K ----------------------------------------------------------------------------------------------------------

def _max_row_blocks_of_the_fast_kernel():
    """STAN_MAX_ROW_BLOCKS (stan_amd/csrc/internal.h): the blocks per row the LDS accumulators of k_numeric take; a wider row
    sends its slice to k_numeric_wide."""
    text = open(os.path.join(ROOT, "stan_amd", "csrc", "internal.h")).read()
    return int(re.search(r"#define\s+STAN_MAX_ROW_BLOCKS\s+(\d+)", text).group(1))


def _mixed(job, seed):
    """Element types and the five materials of element_ref.MIXED_MATERIALS at random."""
    rng = np.random.default_rng(seed)
    ne = job.conn.shape[0]
    job.elem_type = rng.integers(1, 3, ne).astype(np.uint8)
    job.elem_mat = rng.integers(0, len(R.MIXED_MATERIALS), ne).astype(np.int32)
    job.mat_E_nu = np.array(R.MIXED_MATERIALS, dtype=np.float64)
    assert set(job.elem_type) == {R.G1, R.G2} and set(job.elem_mat) == set(range(len(R.MIXED_MATERIALS)))
    return job


TRANSFORMS = {"as_is": lambda x: x, "shift_1e3": lambda x: x + 1e3, "stretch_rot_shift_1e4": R.stretch_rotate_shift}
_models = {}


def _model(mesh, transform):
    """(job, K_ref, S_ref): the 3^3 jittered cube clamped on x = 0, or revolved_mesh(36, 2, 3) clamped on its bottom layer,
    mixed element types and materials, coordinates transformed; the dense reference in longdouble, computed once."""
    key = (mesh, transform)
    if key not in _models:
        if mesh == "cube3":
            xyz, conn = cube_mesh(3, jitter=0.1)
            spc, ld, f = cube_bcs(3)
        else:
            xyz, conn = revolved_mesh(36, 2, 3)
            spc, ld, f = np.nonzero(xyz[:, 2] == 0.0)[0], np.nonzero(xyz[:, 2] == 3.0)[0], np.array([0.0, 10.0, 5.0])
        job = _mixed(problem.make_job(TRANSFORMS[transform](xyz), conn, spc, np.ones((len(spc), 3)), ld, np.tile(f, (len(ld), 1))), 31)
        _models[key] = (job,) + R.model_reference(job)
    return _models[key]


def _dense(K):
    rowptr, col, val = K.to_csr(upper_only=False)
    n = rowptr.shape[0] - 1
    D = np.zeros((n, n))
    D[np.repeat(np.arange(n), np.diff(rowptr)), col] = val
    return D


CASES = [("cube3", t) for t in TRANSFORMS] + [("revolved36", "as_is"), ("revolved36", "shift_1e3")]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("mesh,transform", CASES)
def test_assembled_matrix_against_the_scattered_reference(gpu_ctx, mesh, transform, mode):
    """Mode 0: the row-owner gather, k_numeric (cube3) and k_numeric_wide (revolved36: the axis nodes' rows of 111 blocks are
    wider than the 96 = STAN_MAX_ROW_BLOCKS that k_numeric's LDS takes; 36 thin collapsed sectors meet there); mode 1: the
    colour scatter.  The modes need not agree bit for bit; each meets the reference."""
    job, Kref, Sref = _model(mesh, transform)
    gpu_ctx.set_option(OPT_ASSEMBLY_MODE, mode)
    try:
        K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    finally:
        gpu_ctx.set_option(OPT_ASSEMBLY_MODE, 0)
    info, D, colours = K.info(), _dense(K), gpu_ctx.profile()["assembly_colours"]
    K.free()
    assert (colours >= 8) == (mode == 1)                     # the colour scatter ran in mode 1 and only there
    assert D.shape == Kref.shape and job.n_red <= 700 and np.isfinite(D).all()
    if mesh == "revolved36":
        assert _max_row_blocks_of_the_fast_kernel() == 96 and info["max_row_blocks"] == 3 * (36 + 1) > 96
        assert int((job.conn[:, 0] == job.conn[:, 3]).sum()) == 3 * 36
    else:
        assert info["max_row_blocks"] == 27
    coupled = Sref > 0
    assert not D[~coupled].any() and not Kref[~coupled].any()
    err = np.abs(D.astype(np.longdouble) - Kref)[coupled] / (R.U52 * Sref[coupled])
    print("assembled K %s %s mode %d: worst %.3f units of 2^-52 S (bound %.2f), %d of %d entries coupled" %
          (mesh, transform, mode, float(err.max()), R.DEVICE_KE_UNITS, int(coupled.sum()), coupled.size))
    assert float(err.max()) <= R.DEVICE_KE_UNITS


# ---- k_recover ----------------------------------------------------------------------------------------------------------------

def _recover_disconnected(ctx, X, u, E, nu):
    k = X.shape[0]
    conn = np.arange(8 * k, dtype=np.int32).reshape(k, 8)
    return ctx.recover_hex8(X.reshape(-1, 3), u.reshape(-1, 3), conn, np.zeros(k, np.int32), np.full(k, R.G2, np.uint8),
                            np.array([[E, nu]]))


@pytest.mark.parametrize("name", GROUPS)
def test_recovery_against_the_reference(gpu_ctx, name):
    """The group's elements as disconnected hexes, the first three once more at the end: k + 3 is no multiple of the 8
    elements of a wavefront (the ragged tail).  nu = 0.4999; the random, the rigid and the affine field."""
    worst, bound = {}, {}
    for field in FIELDS:
        X, u, e, s, Se, Ss = R.rec_reference(name, field)
        k = X.shape[0]
        assert (k + 3) % 8
        ge, gs = _recover_disconnected(gpu_ctx, np.concatenate([X, X[:3]]), np.concatenate([u, u[:3]]), *R.REC_MATERIAL)
        t = min(3, k)
        assert np.array_equal(ge[k:], ge[:t]) and np.array_equal(gs[k:], gs[:t])
        ge, gs = ge[:k], gs[:k]
        worst[field], bound[field] = max(R.units(ge, e, Se), R.units(gs, s, Ss)), R.DEVICE_REC_UNITS
        # against the exact answers, through the same scale: the field was rounded once on its way in
        exact = {"rigid": 0.0, "affine": R.AFFINE_STRAIN}.get(field)
        if exact is not None:
            worst[field + "_exact"] = float((np.abs(ge.astype(np.longdouble) - exact) / (R.U52 * Se)).max())
            bound[field + "_exact"] = R.DEVICE_REC_UNITS + R.FIELD_ROUNDING_UNITS
    print("k_recover %s: worst units of 2^-52 S (bound %.2f): %s" % (name, R.DEVICE_REC_UNITS, ", ".join("%s %.3f" % kv for kv in worst.items())))
    for key in worst:
        assert worst[key] <= bound[key], (key, worst)


# ---- exact properties -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-20, 20])
def test_powers_of_two_go_through_bit_for_bit(gpu_ctx, k):
    """On the plain group: coordinates x 2^k and E x 2^k each give K_e x 2^k in the same bits (K_e is of degree one in
    both); under E x 2^k the recovered strain keeps its bits and the stress scales exactly."""
    (X, E, nu, _K, _S), = R.ke_reference("plain", R.G2)
    n = X.shape[0]
    types = np.array([R.G2] * n + [R.G1] * n, dtype=np.uint8)
    XX, f = np.concatenate([X, X]), 2.0 ** k
    base = gpu_ctx.ke_hex8_batch(XX, E, nu, types)
    assert np.isfinite(base).all() and base.any()
    assert np.array_equal(gpu_ctx.ke_hex8_batch(XX * f, E, nu, types), base * f)
    assert np.array_equal(gpu_ctx.ke_hex8_batch(XX, E * f, nu, types), base * f)
    u = R.fields(X)["random"]
    e0, s0 = _recover_disconnected(gpu_ctx, X, u, *R.REC_MATERIAL)
    e1, s1 = _recover_disconnected(gpu_ctx, X, u, R.REC_MATERIAL[0] * f, R.REC_MATERIAL[1])
    assert np.array_equal(e1, e0) and np.array_equal(s1, s0 * f) and s0.any()
