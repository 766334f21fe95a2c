"""Thermal loads without a GPU: the definitions of tests/thermal_ref.py (the reference the GPU tests hold the kernel to)
checked against themselves and against the oracle's element matrices, BuildThermalLoads through host.Db, and the C-ABI's new
names.  Figures found when the tests were written are in the docstrings."""
import ctypes
import os
import re

import numpy as np
import pytest

from stan_amd import host
from stan_amd.cube import cube_mesh
from tests import forces_ref as R
from tests import thermal_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_names_and_records(built_libs):
    """The entry points are exported; ThermalSums mirrors stan_thermal_sums; stan_profile is ABI and keeps its fields."""
    from stan_amd import hip
    lib = hip.load()
    for n in ("stan_hip_thermal_load_hex8", "stan_hip_thermal_load_hex8_dev", "stan_hip_thermal_load_times",
              "stan_hip_thermal_stress_hex8", "stan_hip_thermal_stress_hex8_dev", "stan_hip_results_thermal_stress"):
        assert n in hip.EXPORTS and hasattr(lib, n)
    h = open(os.path.join(ROOT, "include", "stan_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+stan_thermal_sums\s*\{(.*?)\}\s*stan_thermal_sums\s*;", re.sub(r"/\*.*?\*/", " ", h, flags=re.S), flags=re.S).group(1)
    fields = [(n.strip(), t) for t, n in re.findall(r"(double|int64_t)\s+(\w+(?:\[3\])?)\s*;", body)]
    cmap = {ctypes.c_double: "double", ctypes.c_int64: "int64_t", ctypes.c_double * 3: "double"}
    mine = [(n + ("[3]" if t is ctypes.c_double * 3 else ""), cmap[t]) for n, t in hip.ThermalSums._fields_]
    assert mine == fields and ctypes.sizeof(hip.ThermalSums) == 72
    assert [n for n, _ in hip.Profile._fields_][-1] == "forces_gather_ms" and callable(hip.Context.thermal_load_times)
    assert "stan_host_db_get_thermal_loads" in host.EXPORTS and hasattr(host.load(), "stan_host_db_get_thermal_loads")


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_reference_load_sums_to_zero(name):
    """sum_a grad N_a = 0, so the load sums to zero by direction over all DOFs.  The reference adds longdouble terms of
    magnitude s: fewer than 256 roundings of 2^-64 each on the way to any entry (found: below one unit of 2^-64 sum s)."""
    m, case = T.cases()[name]
    l, vol, integral = T.reference(m, case)
    s = T.scale(m, case)
    d = np.asarray(m.node_dof).reshape(-1, 3)
    for c in range(3):
        assert abs(float(l[d[:, c]].sum())) <= 256 * 2.0 ** -64 * s[d[:, c]].sum()
    assert float(vol) > 0 and np.abs(l).max() > 0


def test_reference_uniform_dT_is_K_times_free_expansion():
    """Uniform dT, one material, jittered 5^3 cube: l = K (alpha dT x) with K from the oracle's element matrices -- the same
    Gauss rule on both sides.  The oracle forms K_e in fp64: an entry is a sum over 8 points of products of a handful of
    factors, fewer than 64 roundings relative to |K_e| |u_e|, so 64 units of 2^-52 a, a = sum_e |K_e| |u_e| (found: 1.41)."""
    m = R.cases()["cube5"][0]
    alpha, dT = 1.2e-5, 80.0
    case = T.Case([alpha], np.full(m.xyz.shape[0], dT))
    l, _, _ = T.reference(m, case)
    f, a = R.reference(m, alpha * dT * m.xyz)
    worst = float((np.abs(l - f) / (T.U52 * a)).max())
    print("max |l - K alpha dT x| / (2^-52 a) = %.2f" % worst)
    assert worst <= 64 and np.abs(l).max() > 1e3 * T.U52 * a.max()


def test_rho_np():
    """The yardstick of tests/test_gpu_thermal.py, computed and printed here too (found: 30.88, the 31-element strip)."""
    r = T.rho_np(verbose=True)
    assert 1.0 <= r <= 64.0          # a restatement in the kernel's operation form is within tens of units, or it is another form


def test_alpha_zero_elements_and_g1():
    """mixed4: the material that does not expand contributes exact zeros and no volume; a HEX8_G1 element is its one point."""
    m, case = T.cases()["mixed4-cold"]
    fe, vol, _ = T._element_loads(m, case, np.float64)
    cold = case.mat_alpha[m.elem_mat] == 0
    assert cold.any() and not fe[cold].any() and fe[~cold].any()
    _, vol_all, _ = T._element_loads(m, T.cases()["mixed4-rand"][1], np.float64)
    assert 0 < vol < vol_all


# ---- the BC reader ------------------------------------------------------------------------------------------------------
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


def _col0(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.column_stack([v, np.zeros(v.size), np.zeros(v.size)])


def test_build_thermal_loads(tmp_path, built_libs):
    d, xyz, conn, fixed = _db(mats=((1, 210000.0, 0.3), (7, 70000.0, 0.33)))
    top = np.nonzero(xyz[:, 0] == 3.0)[0]
    d.add_bc(2, "load", "PointLoad", top + 1, np.tile([0.0, 0.0, 5.0], (top.size, 1)))
    d.add_bc(3, "hot", "Temperature", top + 1, _col0(np.full(top.size, 40.0)))
    d.add_bc(4, "hotter", "Temperature", top[:3] + 1, _col0([1.0, 2.0, 3.0]))
    d.add_bc(5, "steel", "ThermalExpansion", [1, 7], _col0([1.2e-5, 2.3e-5]))
    d.add_bc(6, "more", "ThermalExpansion", [7], _col0([1.0e-6]))
    d.set_analysis(tol=1e-10)
    d.assign_dof()
    # the file round-trips: the reference's reader ignores Types it does not know, ours keeps them
    path = str(tmp_path / "m.STdb")
    d.write_stdb(path)
    d = host.Db.read_stdb(path)
    d.assign_dof()
    tl = d.thermal_loads()
    want = np.zeros(xyz.shape[0]); want[top] = 40.0; want[top[:3]] += [1.0, 2.0, 3.0]
    assert tl["any"] and np.array_equal(tl["dT"], want)
    assert np.array_equal(tl["mat_alpha"], [1.2e-5, 2.3e-5 + 1.0e-6])
    # the file's other BCs are read as before: BuildReductionAndLoads is not changed, the distributed loads see none of theirs
    red, n_fixed, F = d.reduction()
    assert n_fixed == 3 * fixed.size and F.sum() == 5.0 * top.size and np.count_nonzero(F) == top.size
    assert not d.distributed_loads()["any"]
    # a model with the same SPC and PointLoad BCs and nothing else gives the same reduction and F
    plain, _, _, _ = _db(mats=((1, 210000.0, 0.3), (7, 70000.0, 0.33)))
    plain.add_bc(2, "load", "PointLoad", top + 1, np.tile([0.0, 0.0, 5.0], (top.size, 1)))
    plain.set_analysis(tol=1e-10)
    plain.assign_dof()
    red0, n_fixed0, F0 = plain.reduction()
    assert np.array_equal(red0, red) and n_fixed0 == n_fixed and np.array_equal(F0, F)
    # the reference's reader: the wire schema of the reference in third-party protobuf (tests/stdb_schema.py) parses the file,
    # finds the BCs it knows as they were written and the new ones as BoundaryCondition records of the same schema (it
    # re-encodes to the same bytes: nothing outside the schema)
    pytest.importorskip("google.protobuf")
    from tests import stdb_schema
    raw = open(path, "rb").read()
    msg = stdb_schema.build(False)()
    msg.ParseFromString(raw)
    assert msg.SerializeToString(deterministic=True) == raw
    bcs = {e.key: e.value for e in msg.BCLib}
    assert [bcs[k].Type for k in sorted(bcs)] == ["SPC", "PointLoad", "Temperature", "Temperature", "ThermalExpansion", "ThermalExpansion"]
    assert sorted(e.key for e in bcs[1].NodalValues) == sorted((fixed + 1).tolist())
    assert all(list(e.value.M) == [0.0, 0.0, 5.0] for e in bcs[2].NodalValues) and len(bcs[2].NodalValues) == top.size
    assert {e.key: e.value.M[0] for e in bcs[5].NodalValues} == {1: 1.2e-5, 7: 2.3e-5}
    # an empty set: such BCs without entries, and a model without such BCs
    d1, _, _, _ = _db()
    d1.add_bc(2, "nothing", "Temperature", [], np.zeros((0, 3)))
    d1.assign_dof()
    t1 = d1.thermal_loads()
    assert t1["any"] and not t1["dT"].any() and np.array_equal(t1["mat_alpha"], [0.0])
    d0, _, _, _ = _db()
    d0.assign_dof()
    t0 = d0.thermal_loads()
    assert not t0["any"] and not t0["dT"].any() and not t0["mat_alpha"].any()


def test_build_thermal_loads_errors(built_libs):
    d, xyz, conn, fixed = _db()
    d.add_bc(2, "a", "ThermalExpansion", [2], _col0([1.2e-5]))     # node 2 exists, material 2 does not
    d.assign_dof()
    with pytest.raises(host.StanHostError) as ei:
        d.thermal_loads()
    assert "material 2" in str(ei.value)
    d, xyz, conn, fixed = _db()
    d.add_bc(2, "a", "ThermalExpansion", [1, 1000], _col0([1.2e-5, 2.0e-5]))   # (a material ID beyond the node IDs is kept)
    d.assign_dof()
    with pytest.raises(host.StanHostError) as ei:
        d.thermal_loads()
    assert "material 1000" in str(ei.value)
