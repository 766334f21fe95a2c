"""Distributed loads and prescribed displacements without a GPU: the definitions of tests/loads_ref.py (the reference the
GPU tests hold the kernel to) checked against closed forms and patch tests, stan_host_pressure_faces, BuildDistributedLoads
through host.Db, and the C-ABI's new names.  Figures found when the tests were written are in the docstrings."""
import ctypes
import os
import re

import numpy as np
import pytest

from stan_amd import host
from stan_amd.cube import cube_mesh, revolved_mesh
from tests import forces_ref as R
from tests import loads_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_names_and_records(built_libs):
    """The entry points are exported; LoadSums mirrors stan_load_sums; stan_profile is ABI and keeps its fields (the
    phase times of the load vector have a call of their own, stan_hip_load_vector_times)."""
    from stan_amd import hip
    lib = hip.load()
    for n in ("stan_hip_load_vector_hex8", "stan_hip_load_vector_hex8_dev", "stan_hip_load_vector_times"):
        assert n in hip.EXPORTS and hasattr(lib, n)
    h = open(os.path.join(ROOT, "include", "stan_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+stan_load_sums\s*\{(.*?)\}\s*stan_load_sums\s*;", re.sub(r"/\*.*?\*/", " ", h, flags=re.S), flags=re.S).group(1)
    fields = [(n.strip(), t) for t, n in re.findall(r"(double|int64_t)\s+(\w+(?:\[3\])?)\s*;", body)]
    cmap = {ctypes.c_double: "double", ctypes.c_int64: "int64_t", ctypes.c_double * 3: "double"}
    mine = [(n + ("[3]" if t is ctypes.c_double * 3 else ""), cmap[t]) for n, t in hip.LoadSums._fields_]
    assert mine == fields and ctypes.sizeof(hip.LoadSums) == 80
    assert [n for n, _ in hip.Profile._fields_][-1] == "forces_gather_ms" and callable(hip.Context.load_vector_times)
    assert "stan_host_pressure_faces" in host.EXPORTS and hasattr(host.load(), "stan_host_db_get_distributed_loads")


def test_face_table_and_outward_normals():
    """FACE_NODES is the set of nodes with the face's natural coordinate; on a cube with det J > 0 the surface vector of
    every face points away from the centre and has the face's area."""
    for f in range(6):
        s = 1.0 if f & 1 else -1.0
        assert L.FACE_NODES[f] == [i for i in range(8) if L.S3[f // 2][i] == s]
    xyz, conn = cube_mesh(1, h=2.0)
    m = R.model(xyz, conn)
    for f in range(6):
        l, _, area = L.loads_np(m, L.Case(None, [0], [f], [1.0]))
        force = l[np.asarray(m.node_dof).reshape(-1, 3)].sum(axis=0)          # -p n A
        want = np.zeros(3); want[f // 2] = -(1.0 if f & 1 else -1.0) * 4.0
        assert np.allclose(force, want, rtol=0, atol=1e-14) and abs(area - 4.0) <= 1e-14


def test_body_force_sums_to_b_times_volume():
    """3^3 cube, interior nodes jittered by 0.2, planar boundary: sum f = b V with V = L^3 (27 - 1e-14 found)."""
    m = L.patch_model(3)
    b = np.array([[0.3, -1.1, 2.5]])
    l, vol, _ = L.loads_np(m, L.Case(mat_body=b))
    d = np.asarray(m.node_dof).reshape(-1, 3)
    assert abs(vol - 27.0) <= 1e-12
    for c in range(3):
        assert abs(l[d[:, c]].sum() - b[0, c] * 27.0) <= 1e-12 * 27.0
    l_ref, vol_ref, _ = L.reference(m, L.Case(mat_body=b))
    assert abs(float(vol_ref) - 27.0) <= 1e-15 * 27.0 * 8


def test_pressure_resultants():
    """sum f = -p A on a flat face (9 x 7.5 = 67.5, found to 3e-14), and ~ 0 over the closed free surface of a fully
    jittered (warped) cube (1.4e-14 against |f|_1 = 415 found): the surface vectors of a closed surface add up to zero."""
    m = L.patch_model(3)
    el, fid = L.cube_face(3, 5)
    l, _, area = L.loads_np(m, L.Case(None, el, fid, np.full(el.size, 7.5)))
    d = np.asarray(m.node_dof).reshape(-1, 3)
    assert abs(area - 9.0) <= 1e-13 and abs(l[d[:, 2]].sum() + 67.5) <= 1e-12 and abs(l[d[:, 0]].sum()) <= 1e-12
    mj = R.jittered_cube(3)
    fe, fi = L.free_surface(mj)
    assert fe.size == 54
    l, _, _ = L.loads_np(mj, L.Case(None, fe, fi, np.full(fe.size, 7.5)))
    for c in range(3):
        assert abs(l[d[:, c]].sum()) <= 1e-13 * np.abs(l).sum() and np.abs(l).sum() > 100


def _patch_residual(m, n, p=1000.0):
    E, nu = m.mat_E_nu[0]
    el, fid = L.cube_face(n, 5)
    l, _, _ = L.loads_np(m, L.Case(None, el, fid, np.full(el.size, p)))
    u = m.xyz * np.array([nu * p / E, nu * p / E, -p / E])
    f_ref, _ = R.reference(m, u)
    free = m.red != -1
    return float(np.abs(l - f_ref.astype(np.float64))[free].max()), float(np.abs(l).max())


def test_pressure_patch_test():
    """HEX8_G2, boundary planes planar, symmetry supports, pressure on z = L: with the oracle's element matrices
    load - K u_exact vanishes on every free DOF (5.5e-15 against loads of 8 found for p = 1; here p = 1000).  Distorted
    HEX8_G1 elements do NOT pass (0.15 relative found): one-point integration does not reproduce the constant-stress state
    on a distorted mesh, which is why the patch tests use G2."""
    m = L.patch_model(4)
    res, top = _patch_residual(m, 4)
    assert res <= 1e-12 * top and top > 100
    g1 = L.patch_model(4)
    g1.elem_type = np.full_like(g1.elem_type, 1)
    res1, top1 = _patch_residual(g1, 4)
    assert res1 > 1e-3 * top1


def test_prescribed_displacement_patch_test():
    """u = A x on all boundary nodes: f_int of the linear field vanishes at the interior nodes (1.8e-13 against 336 found),
    so the right-hand side -f_int(u0)|free reproduces the field."""
    m = L.patch_model(4, supports="all")
    A = np.array([[1.0e-3, 2.0e-4, -3.0e-4], [1.5e-4, -7.0e-4, 2.5e-4], [-1.0e-4, 3.0e-4, 5.0e-4]])
    f_ref, _ = R.reference(m, m.xyz @ A.T)
    free = m.red != -1
    assert np.abs(f_ref[free]).max() <= 1e-12 * np.abs(f_ref).max() and free.sum() == 81


def test_pressure_faces():
    xyz, conn = cube_mesh(3)
    nn = xyz.shape[0]
    m = R.model(xyz, conn)
    # free surface from the set "all nodes": interior faces are seen twice and dropped
    fe, fi, fp = host.pressure_faces(nn, conn, np.arange(nn), np.full(nn, 2.0))
    we, wi = L.free_surface(m)
    assert np.array_equal(fe, we) and np.array_equal(fi, wi) and fe.size == 54 and (fp == 2.0).all()
    assert (np.diff(fe.astype(np.int64) * 6 + fi) > 0).all()
    # one face from its four nodes, p = 0.25 x the sum in local face-node order
    nodes = conn[13, L.FACE_NODES[3]]
    fe, fi, fp = host.pressure_faces(nn, conn, nodes, [1.0, 2.0, 4.0, 8.0])
    # (element 13 is the centre element: its face 3 is shared with element 16's face 2 -> interior, dropped)
    assert fe.size == 0
    nodes = conn[26, L.FACE_NODES[1]]
    fe, fi, fp = host.pressure_faces(nn, conn, nodes[::-1], [8.0, 4.0, 2.0, 1.0])
    assert fe.tolist() == [26] and fi.tolist() == [1] and fp.tolist() == [0.25 * (((1.0 + 2.0) + 4.0) + 8.0)]
    # an interior plane's node set gives no face
    plane = np.nonzero(xyz[:, 0] == 1.0)[0]
    assert host.pressure_faces(nn, conn, plane, np.ones(plane.size))[0].size == 0
    # the boundary plane x = 3: nine faces, id 1, ascending
    plane = np.nonzero(xyz[:, 0] == 3.0)[0]
    fe, fi, fp = host.pressure_faces(nn, conn, plane, np.ones(plane.size))
    assert fe.tolist() == L.cube_face(3, 1)[0].tolist() and (fi == 1).all()
    # collapsed faces: the revolved mesh's wedges name the axis node twice; their xi = -1 face has two distinct nodes
    rxyz, rconn = revolved_mesh(36, 2, 3)
    fe, fi, fp = host.pressure_faces(rxyz.shape[0], rconn, np.arange(rxyz.shape[0]), np.ones(rxyz.shape[0]))
    we, wi = L.free_surface(R.model(rxyz, rconn))
    assert np.array_equal(fe, we) and np.array_equal(fi, wi)
    wedge0 = (fe == 0)
    assert 0 not in fi[wedge0].tolist() and len(set(rconn[0, L.FACE_NODES[0]].tolist())) == 2
    # capacity protocol: too small an array is an error, a larger one is fine
    with pytest.raises(host.StanHostError):
        host.pressure_faces(nn, conn, plane, np.ones(plane.size), capacity=8)
    assert host.pressure_faces(nn, conn, plane, np.ones(plane.size), capacity=20)[0].size == 9
    with pytest.raises(host.StanHostError):
        host.pressure_faces(nn, conn, [nn], [1.0])


def _db(n=3, mats=((1, 210000.0, 0.3),)):
    xyz, conn = cube_mesh(n)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    for mid, E, nu in mats:
        d.add_material(mid, "Steel%d" % mid, E, nu)
    d.assign_part(1, mats[0][0], "HEX8_G2")
    fixed = np.nonzero(xyz[:, 0] == 0.0)[0]
    d.add_bc(1, "fix", "SPC", fixed + 1, np.ones((fixed.size, 3)))
    return d, xyz, conn, fixed


def test_build_distributed_loads(tmp_path):
    d, xyz, conn, fixed = _db()
    top = np.nonzero(xyz[:, 0] == 3.0)[0]
    d.add_bc(2, "p", "Pressure", top + 1, np.column_stack([np.full(top.size, 4.0), np.zeros(top.size), np.zeros(top.size)]))
    d.add_bc(3, "g", "BodyForce", [1], [[0.0, 0.0, -9.75]])
    d.add_bc(4, "g2", "BodyForce", [1], [[1.0, 0.0, 0.75]])
    moved = np.tile([0.0, 1e-3, -2e-3], (fixed.size, 1))
    d.add_bc(5, "move", "Displacement", fixed + 1, moved)
    d.add_bc(6, "zero on free", "Displacement", top[:2] + 1, np.zeros((2, 3)))
    d.set_analysis(tol=1e-10)
    d.assign_dof()
    # the file round-trips: the reference's reader ignores Types it does not know, ours keeps them
    path = str(tmp_path / "m.STdb")
    d.write_stdb(path)
    d = host.Db.read_stdb(path)
    d.assign_dof()
    dl = d.distributed_loads()
    assert dl["any"] and np.array_equal(dl["mat_body"], [[1.0, 0.0, -9.0]])
    assert dl["face_elem"].tolist() == L.cube_face(3, 1)[0].tolist() and (dl["face_id"] == 1).all() and (dl["face_p"] == 4.0).all()
    want = np.zeros(xyz.shape); want[fixed] = moved
    assert np.array_equal(dl["disp0"], want) and dl["n_prescribed"] == 2 * fixed.size
    red, n_fixed, F = d.reduction()                      # BuildReductionAndLoads is not changed: no point load here
    assert n_fixed == 3 * fixed.size and not F.any()
    # a model without such BCs
    d0, _, _, _ = _db()
    d0.assign_dof()
    dl0 = d0.distributed_loads()
    assert not dl0["any"] and dl0["mat_body"] is None and dl0["face_elem"] is None and dl0["disp0"] is None


def test_build_distributed_loads_errors():
    d, xyz, conn, fixed = _db()
    d.add_bc(2, "g", "BodyForce", [2], [[0.0, 0.0, -1.0]])          # node 2 exists, material 2 does not
    d.assign_dof()
    with pytest.raises(host.StanHostError) as ei:
        d.distributed_loads()
    assert "material 2" in str(ei.value)
    d, xyz, conn, fixed = _db()
    free_node = int(np.nonzero(xyz[:, 0] == 2.0)[0][0]) + 1
    d.add_bc(2, "move", "Displacement", [free_node], [[0.0, 0.5, 0.0]])
    d.assign_dof()
    with pytest.raises(host.StanHostError) as ei:
        d.distributed_loads()
    assert "node %d" % free_node in str(ei.value)
