"""Result scalars and the .vtu export, the parts that need no GPU: the C-ABI surface, the name table, the writer's file
format (parsed here, byte by byte), and the eigenvalue yardstick the GPU tests hold the device to."""
import ctypes
import os
import re

import numpy as np

from stan_amd.cube import cube_mesh
from tests import scalars_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Part.cs:403-428, typed out
NAMES = ["Displacement X", "Displacement Y", "Displacement Z", "Total Displacement",
         "Stress XX", "Stress YY", "Stress ZZ", "Stress XY", "Stress YZ", "Stress XZ", "Stress P1", "Stress P2", "Stress P3",
         "von Mises Stress",
         "Strain XX", "Strain YY", "Strain ZZ", "Strain XY", "Strain YZ", "Strain XZ", "Strain P1", "Strain P2", "Strain P3",
         "Effective Strain"]
DEFINES = ["DISP_X", "DISP_Y", "DISP_Z", "DISP_TOTAL", "STRESS_XX", "STRESS_YY", "STRESS_ZZ", "STRESS_XY", "STRESS_YZ",
           "STRESS_XZ", "STRESS_P1", "STRESS_P2", "STRESS_P3", "STRESS_VON_MISES", "STRAIN_XX", "STRAIN_YY", "STRAIN_ZZ",
           "STRAIN_XY", "STRAIN_YZ", "STRAIN_XZ", "STRAIN_P1", "STRAIN_P2", "STRAIN_P3", "STRAIN_EFFECTIVE"]


def test_surface_header_exports_methods_and_names(built_libs):
    from stan_amd import hip, host
    h = open(os.path.join(ROOT, "include", "stan_hip.h")).read()
    for f in ("stan_hip_result_scalars_hex8", "stan_hip_results_scalars"):
        assert re.search(r"\bint\s+%s\s*\(" % f, h), f
        assert f in hip.EXPORTS and hasattr(hip.load(), f), f
    assert re.search(r"#define\s+STAN_SCALAR_COUNT\s+24\b", h)
    for s, d in enumerate(DEFINES):
        assert re.search(r"#define\s+STAN_SCALAR_%s\s+%d\b" % (d, s), h), d
    assert callable(hip.Context.result_scalars) and callable(hip.Results.scalars)
    assert [host.scalar_name(s) for s in range(24)] == NAMES == R.NAMES
    assert host.scalar_name(-1) is None and host.scalar_name(24) is None
    hh = open(os.path.join(ROOT, "include", "stan_host.h")).read()
    assert "stan_host_scalar_name" in hh and "stan_host_write_vtu" in hh


def test_vtu_round_trip(built_libs, tmp_path):
    from stan_amd import host
    xyz, conn = cube_mesh(2, jitter=0.1)
    rng = np.random.default_rng(7)
    disp = rng.standard_normal(xyz.shape) * 1e-3
    nn, ne = xyz.shape[0], conn.shape[0]
    pts = [(NAMES[s], rng.standard_normal(nn) * 10.0 ** rng.uniform(-3, 6)) for s in (0, 13, 23)]
    cells = [(p + NAMES[13], rng.standard_normal(ne) * 1e4) for p in ("Max ", "Average ", "Min ")]
    path = str(tmp_path / "cube.vtu")
    host.write_vtu(path, xyz, disp, conn, pts, cells)
    vtk, piece, arr = R.parse_vtu(path)
    assert vtk["type"] == "UnstructuredGrid" and vtk["byte_order"] == "LittleEndian" and vtk["header_type"] == "UInt64"
    assert int(piece["NumberOfPoints"]) == nn == 27 and int(piece["NumberOfCells"]) == ne == 8
    (_, p, at), = arr["Points"]
    assert at["NumberOfComponents"] == "3" and np.array_equal(p.reshape(-1, 3), xyz + disp)     # Part.UpdateNode, exactly
    cel = {n: a for n, a, _ in arr["Cells"]}
    assert np.array_equal(cel["connectivity"].reshape(-1, 8), conn)
    assert np.array_equal(cel["offsets"], 8 * np.arange(1, ne + 1))
    assert cel["types"].dtype == np.uint8 and (cel["types"] == 12).all() and cel["types"].size == ne
    assert [n for n, _, _ in arr["PointData"]] == [n for n, _ in pts]
    assert [n for n, _, _ in arr["CellData"]] == [n for n, _ in cells]
    for (n, a, _), (_, v) in zip(arr["PointData"] + arr["CellData"], pts + cells):
        assert a.dtype == np.dtype("<f4") and np.array_equal(a, v.astype(np.float32)), n
    # no cell arrays, no displacement: still a whole file
    host.write_vtu(path, xyz, None, conn, pts[:1], [])
    _, _, arr = R.parse_vtu(path)
    assert arr["CellData"] == [] and len(arr["PointData"]) == 1 and np.array_equal(arr["Points"][0][1].reshape(-1, 3), xyz)
    # a path that cannot be opened: a negative return, no crash
    lib = host.load()
    rc = lib.stan_host_write_vtu(os.fsencode(str(tmp_path / "no_such_dir" / "x.vtu")), ctypes.c_int64(nn),
                                 xyz.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, ctypes.c_int64(ne),
                                 conn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(0), None, None,
                                 ctypes.c_int32(0), None, None)
    assert rc < 0
    bad = conn.copy(); bad[3, 2] = nn      # a node index out of range is refused, not written
    try:
        host.write_vtu(path, xyz, None, bad, [], [])
        assert False
    except host.StanHostError:
        pass


def test_eigenvalue_yardstick():
    """numpy's eigvalsh against mpmath at 50 digits over the family the GPU tests feed the device: its worst error in
    units of 2^-52 ||S||_F is what scalars_ref.DEVICE_UNITS is derived from (4 x the value measured when the constant was
    written); it must stay under 8 on any host, and the recorded value must stay a fair record of it."""
    fam = R.yardstick_family()
    assert fam.shape == (505, 6)
    worst = R.worst_units(fam, R.principals)
    print("eigvalsh worst error: %.2f units of 2^-52 ||S||_F (recorded: %.2f)" % (worst, R.EIGVALSH_UNITS_MEASURED))
    assert worst < 8
    assert R.DEVICE_UNITS == 4 * R.EIGVALSH_UNITS_MEASURED and R.DEVICE_UNITS < 1e6
    # the family holds what it says: coinciding and near-hydrostatic eigenvalues, and the named special tensors
    w = np.array([R.principals(v) for v in fam])
    gap = np.minimum(w[:, 0] - w[:, 1], w[:, 1] - w[:, 2]) / np.maximum(R.fro(fam), 1e-300)
    assert (gap[300:400] < 1e-5).all() and ((w[400:500, 0] - w[400:500, 2]) / R.fro(fam[400:500]) < 1e-4).all()
    assert not fam[500].any() and np.array_equal(fam[501], [3, 3, 3, 0, 0, 0])


def test_reference_restates_the_quirks():
    """scalars_ref on a hand-made case: a collapsed hex (node listed twice: the first position counts, the element once),
    the shear strain not halved, an unreferenced node left at 0."""
    conn = np.array([[0, 1, 2, 0, 3, 4, 5, 3]])
    disp = np.arange(21, dtype=np.float64).reshape(7, 3)          # node 6 is referenced by no element
    strain = np.zeros((1, 8, 6)); stress = np.zeros((1, 8, 6))
    strain[0, :, 3] = 2.0                                          # pure shear xy = 2 AS STORED: principals +-2, not +-1
    stress[0, 0, 0], stress[0, 3, 0] = 5.0, 7.0                    # corners 0 and 3 are both node 0
    ref = R.Reference(disp, conn, strain, stress)
    assert ref.elist[0] == [(0, 0)] and ref.elist[6] == []
    assert ref.point[4, 0] == 5.0 and (ref.point[:, 6] == 0).all()
    assert np.allclose(ref.point[20:23, 1], [2.0, 0.0, -2.0], atol=1e-15)
    assert np.isclose(ref.point[23, 1], (2.0 / 3.0) * np.sqrt((4 + 4 + 16) / 2.0))
    assert ref.cell[4, 0, 0] == 7.0 and ref.cell[4, 1, 0] == 12.0 / 8 and ref.cell[4, 2, 0] == 0.0
