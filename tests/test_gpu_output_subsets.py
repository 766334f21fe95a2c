"""The optional outputs of the load-vector host entries, subset by subset (stan_hip_load_vector_hex8, stan_hip_thermal_load_hex8):
an output asked for carries the bytes of the all-outputs call, an output not asked for is None, an F passed in comes back as a
copy.  Internal forces and result scalars have this in tests/test_gpu_internal_forces.py and tests/test_gpu_result_scalars.py; the
host thermal stress against Results.thermal_stress on a recover_hex8_keep of the same job, mapped whole and compared by
tobytes(), is tests/test_gpu_thermal.py::test_thermal_stress and is not repeated here.

Mesh: problem.cube_job(3, jitter=0.1) -- 27 elements, 64 nodes: interior nodes, more than one gather lane, milliseconds a call."""
import itertools

import numpy as np
import pytest

from stan_amd import problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def job():
    j = problem.cube_job(3, jitter=0.1)
    rng = np.random.default_rng(11)
    j.F_in = rng.standard_normal(j.n_dof - j.n_fixed) * 5.0
    j.mat_body = np.array([[0.3, -0.2, 7.7]])
    j.faces = dict(face_elem=np.array([0, 26], dtype=np.int32), face_id=np.array([0, 5], dtype=np.uint8),   # sorted by 6 e + id
                   face_pressure=np.array([1.5, -0.75]))
    j.disp0 = rng.standard_normal((j.xyz.shape[0], 3)) * 1e-3
    j.mat_alpha = np.array([1.2e-5])
    j.dT = 40.0 * j.xyz[:, 0] + rng.standard_normal(j.xyz.shape[0])   # linear in x plus a nodal perturbation
    return j


def _subsets(names, must=()):
    for on in itertools.product([False, True], repeat=len(names)):
        want = dict(zip(names, on))
        if any(on) and all(want[k] for k in must):
            yield want


def _check(got, ref, want, F_in, F_before):
    """got, ref: the entry's tuples (arrays ..., sums) by the names of `want`, in its order"""
    assert F_in.tobytes() == F_before                                   # the caller's array is unchanged
    for (name, on), g, r in zip(want.items(), got, ref):
        if not on:
            assert g is None, (want, name)
        elif name == "sums":
            assert g.as_dict() == r.as_dict(), (want, name)
        else:
            assert g is not F_in and g.tobytes() == r.tobytes(), (want, name)


def _load_vector(ctx, j, disp0, want):
    return ctx.load_vector_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, mat_body=j.mat_body,
                                disp0=disp0, F=j.F_in if want["F"] else None, F_solve=want["F_solve"],
                                load_full=want["load_full"], sums=want["sums"], **j.faces)


@pytest.mark.parametrize("with_disp0", [False, True])
def test_load_vector_output_subsets(gpu_ctx, job, with_disp0):
    """Without disp0 the 15 non-empty subsets of {F, F_solve, load_full, sums}; with a non-zero disp0 the 8 that contain
    F_solve (the entry refuses disp0 without it).

    F is an input too: F_solve is "(F after the add, or l when F is NULL) - f_int(u0)" (include/stan_hip.h), so a subset
    without F is a call with another input, and its F_solve is held to the all-other-outputs call WITHOUT F; load_full and
    sums do not see F, and those two reference calls must agree on them bit for bit."""
    names = ("F", "F_solve", "load_full", "sums")
    disp0 = job.disp0 if with_disp0 else None
    before = job.F_in.tobytes()
    ref = _load_vector(gpu_ctx, job, disp0, dict.fromkeys(names, True))
    ref_no_F = _load_vector(gpu_ctx, job, disp0, dict(dict.fromkeys(names, True), F=False))
    assert all(r is not None for r in ref) and ref[0].tobytes() != before and np.abs(ref[2]).max() > 0
    assert ref_no_F[0] is None and ref_no_F[1].tobytes() != ref[1].tobytes()
    assert ref_no_F[2].tobytes() == ref[2].tobytes() and ref_no_F[3].as_dict() == ref[3].as_dict()
    if with_disp0:
        assert ref[1].tobytes() != ref[0].tobytes()                     # the prescribed displacements reach F_solve
    else:
        assert ref[1].tobytes() == ref[0].tobytes()                     # "and only then differs"
    cases = list(_subsets(names, must=("F_solve",) if with_disp0 else ()))
    assert len(cases) == (8 if with_disp0 else 15)
    for want in cases:
        _check(_load_vector(gpu_ctx, job, disp0, want), ref if want["F"] else ref_no_F, want, job.F_in, before)


def test_thermal_load_output_subsets(gpu_ctx, job):
    """The 7 non-empty subsets of {F, load_full, sums}."""
    names = ("F", "load_full", "sums")

    def call(want):
        return gpu_ctx.thermal_load_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red,
                                         job.mat_alpha, job.dT, F=job.F_in if want["F"] else None, load_full=want["load_full"],
                                         sums=want["sums"])
    before = job.F_in.tobytes()
    ref = call(dict.fromkeys(names, True))
    assert all(r is not None for r in ref) and ref[0].tobytes() != before and np.abs(ref[1]).max() > 0
    cases = list(_subsets(names))
    assert len(cases) == 7
    for want in cases:
        _check(call(want), ref, want, job.F_in, before)
