"""Result scalars on the GPU (stan_hip_result_scalars_hex8 / stan_hip_results_scalars) against tests/scalars_ref.py, the
literal restatement of Part.Load_Scalar, and the console driver's --vtu export.

Bounds (the issue's): the 15 copied scalars (displacement X Y Z, stress and strain components) bit-equal, with their cell
max / average / min and point averages; total displacement within 4 ulp (FMA contraction of the sum of squares);
principals, von Mises and effective strain within scalars_ref.DEVICE_UNITS x 2^-52 x ||S||_F of the eigvalsh-based
reference, ||S||_F the largest tensor norm entering that output; P1 >= P2 >= P3; no NaN / inf."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import problem
from stan_amd.cube import cube_bcs, cube_mesh, revolved_mesh
from tests import scalars_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
ALL = list(range(24))


def row_mesh(n):
    """n hexes in a row along x."""
    xyz = np.array([(i, j, k) for k in range(2) for j in range(2) for i in range(n + 1)], dtype=np.float64)
    m = n + 1
    conn = np.array([[i, i + 1, i + 1 + m, i + m, i + 2 * m, i + 1 + 2 * m, i + 1 + 3 * m, i + 3 * m] for i in range(n)], dtype=np.int32)
    return xyz, conn


def synthetic(n_nodes, conn, first):
    """Displacements and 8x6 blocks for a mesh: the yardstick family tiled over the corners from tensor `first` on (strain)
    and 264 further (stress), so that a mesh of 33 elements carries every tensor of the family once."""
    fam = R.yardstick_family()
    k = np.arange(conn.shape[0] * 8)
    strain = fam[(first + k) % len(fam)].reshape(-1, 8, 6)
    stress = fam[(first + 264 + k) % len(fam)].reshape(-1, 8, 6)
    disp = np.random.default_rng(99).standard_normal((n_nodes, 3)) * 1e-2
    disp[0] = 0.0
    return disp, np.ascontiguousarray(strain), np.ascontiguousarray(stress)


def _mesh(name):
    if name == "one":
        return row_mesh(1) + (497,)       # the five named tensors (zero, diag(3,3,3), uniaxial, pure shear, diag(1,1,-2)) among its corners
    if name == "cube2":
        return cube_mesh(2) + (290,)      # into the coinciding-eigenvalue block; 1, 2, 4 and 8 incidences per node
    if name == "row33":
        return row_mesh(33) + (0,)        # one element past a 32-element workgroup; the whole family
    if name == "orphan":
        xyz, conn = cube_mesh(2)
        return np.vstack([xyz, [[9.0, 9.0, 9.0]]]), conn, 390     # node 27: referenced by no element
    raise KeyError(name)


_refs = {}


def _case(name):
    if name not in _refs:
        xyz, conn, first = _mesh(name)
        disp, strain, stress = synthetic(xyz.shape[0], conn, first)
        _refs[name] = (disp, conn, strain, stress, R.Reference(disp, conn, strain, stress))
    return _refs[name]


@pytest.mark.parametrize("name", ["one", "cube2", "row33", "orphan"])
def test_synthetic_blocks_against_the_reference(gpu_ctx, name):
    disp, conn, strain, stress, ref = _case(name)
    point, cell = gpu_ctx.result_scalars(disp, conn, strain, stress)
    worst = R.check_against(ref, ALL, point, cell)
    print("%s: worst derived-scalar error %.2f units of 2^-52 ||S||_F (bound %.2f)" % (name, worst, R.DEVICE_UNITS))
    if name == "cube2":
        assert sorted(set(len(l) for l in ref.elist)) == [1, 2, 4, 8]
    if name == "orphan":
        assert ref.elist[27] == [] and (point[:, 27] == 0).all() and np.abs(disp[27]).max() > 0


@pytest.fixture(scope="module")
def solved(gpu_ctx):
    """Mesh (d): the 3^3 cube with jittered nodes through assemble -> cg_solve -> recover_hex8_keep."""
    from stan_amd import host
    job = problem.cube_job(3, jitter=0.1)
    K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    U, rep = K.cg_solve(job.F, 1e-12)
    assert rep["terminationtype"] in (1, 7)
    K.free()
    disp = host.nodal_displacements(job.node_dof, job.red, U).reshape(-1, 3)
    res = gpu_ctx.recover_hex8_keep(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    strain, stress = res.map(0, res.n_elem)
    yield job, disp, res, strain, stress, R.Reference(disp, job.conn, strain, stress)
    res.free()


def test_kept_results_of_a_real_solve(gpu_ctx, solved):
    job, disp, res, strain, stress, ref = solved
    point, cell = res.scalars(disp, job.conn)
    worst = R.check_against(ref, ALL, point, cell)
    print("solved 3^3: worst derived-scalar error %.2f units (bound %.2f)" % (worst, R.DEVICE_UNITS))
    assert np.abs(point[13]).max() > 0 and np.abs(cell[23]).max() > 0
    # the host-pointer entry fed the downloaded arrays gives the same bits; so does a second run
    p2, c2 = gpu_ctx.result_scalars(disp, job.conn, strain, stress)
    assert point.tobytes() == p2.tobytes() and cell.tobytes() == c2.tobytes()
    p3, c3 = res.scalars(disp, job.conn)
    assert point.tobytes() == p3.tobytes() and cell.tobytes() == c3.tobytes()


def test_selections_and_optional_outputs(gpu_ctx, solved):
    job, disp, res, strain, stress, ref = solved
    point, cell = res.scalars(disp, job.conn)
    for s in (3, 9, 13, 22):                      # one scalar = that row of all 24 (copied, total, derived from either tensor)
        p1, c1 = res.scalars(disp, job.conn, sel=[s])
        assert p1.shape == (1, point.shape[1]) and p1[0].tobytes() == point[s].tobytes() and c1[0].tobytes() == cell[s].tobytes()
    sel = [23, 4, 10]                             # rows follow the order of the selection
    ps, cs = res.scalars(disp, job.conn, sel=sel)
    R.check_against(ref, sel, ps, cs)
    assert all(ps[k].tobytes() == point[s].tobytes() and cs[k].tobytes() == cell[s].tobytes() for k, s in enumerate(sel))
    p_only, none = res.scalars(disp, job.conn, cell=False)
    assert none is None and p_only.tobytes() == point.tobytes()
    none, c_only = gpu_ctx.result_scalars(disp, job.conn, strain, stress, point=False)
    assert none is None and c_only.tobytes() == cell.tobytes()


def test_revolved_mesh_collapsed_hexes_and_a_high_valence_axis(gpu_ctx):
    """Mesh (e): the axis node is listed twice in each wedge (first position counts, the element once) and has 72
    incident elements -- no per-node buffer can be assumed."""
    xyz, conn = revolved_mesh(36, 2, 3)
    disp, strain, stress = synthetic(xyz.shape[0], conn, 123)
    ref = R.Reference(disp, conn, strain, stress)
    assert max(len(l) for l in ref.elist) == 72 and (conn[0, 0] == conn[0, 3])
    point, cell = gpu_ctx.result_scalars(disp, conn, strain, stress)
    worst = R.check_against(ref, ALL, point, cell)
    print("revolved: worst derived-scalar error %.2f units (bound %.2f)" % (worst, R.DEVICE_UNITS))


def test_argument_errors(gpu_ctx):
    from stan_amd import hip
    disp, conn, strain, stress, ref = _case("cube2")

    def code(**kw):
        with pytest.raises(hip.StanHipError) as ei:
            gpu_ctx.result_scalars(kw.get("disp", disp), kw.get("conn", conn), strain, stress, sel=kw.get("sel"), point=kw.get("point", True),
                                   cell=kw.get("cell", True))
        return ei.value.code
    assert code(sel=[]) == hip.E_ARG                     # n_sel <= 0
    assert code(sel=[24]) == hip.E_ARG and code(sel=[-1]) == hip.E_ARG
    assert code(sel=[13, 4, 13]) == hip.E_ARG            # listed twice
    bad = conn.copy(); bad[5, 6] = disp.shape[0]
    assert code(conn=bad) == hip.E_ARG
    bad[5, 6] = -1
    assert code(conn=bad) == hip.E_ARG
    assert code(point=False, cell=False) == hip.E_ARG    # point or cell may be NULL, not both
    # the context is still usable
    point, _ = gpu_ctx.result_scalars(disp, conn, strain, stress, sel=[13], cell=False)
    assert point[0].tobytes() == gpu_ctx.result_scalars(disp, conn, strain, stress, cell=False)[0][13].tobytes()


def test_multi_device_handle_is_refused(built_libs):
    """Both calls return STAN_E_UNSUPPORTED on a stan_hip_init_multi handle; results kept by such a handle (two chunks) are
    STAN_E_ARG for a single-device context."""
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from stan_amd import hip, problem
job = problem.cube_job(3)
disp = np.random.default_rng(1).standard_normal(job.xyz.shape) * 1e-3
ctx = hip.Context(devices=[0, 0])
blocks = np.zeros((job.conn.shape[0], 8, 6))
for what, call in (("HOST", lambda: ctx.result_scalars(disp, job.conn, blocks, blocks)),):
    try:
        call(); print(what, "NOERROR")
    except hip.StanHipError as e:
        print(what, e.code, "multi-device" in str(e))
res = ctx.recover_hex8_keep(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
try:
    res.scalars(disp, job.conn); print("KEPT NOERROR")
except hip.StanHipError as e:
    print("KEPT", e.code, "multi-device" in str(e))
one = hip.Context(0)
view = hip.Results(one, res.h, res.n_elem)     # the same handle seen through a single-device context
try:
    view.scalars(disp, job.conn); print("FOREIGN NOERROR")
except hip.StanHipError as e:
    print("FOREIGN", e.code)
view.h = None                                  # (res owns it)
one.close(); res.free(); ctx.close()
print("CLOSED")
''' % ROOT
    env = dict(os.environ, STAN_RCCL_LIB=FAKE)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert "HOST -8 True" in lines and "KEPT -8 True" in lines and "FOREIGN -2" in lines and "CLOSED" in lines, p.stdout


def _write_model(path, n):
    from stan_amd import host
    xyz, conn = cube_mesh(n, jitter=0.1)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    d.add_material(1, "Steel", 210000.0, 0.3)
    d.assign_part(1, 1, "HEX8_G2")
    spc, ld, f = cube_bcs(n)
    d.add_bc(1, "fix", "SPC", spc + 1, np.ones((len(spc), 3)))
    d.add_bc(2, "load", "PointLoad", ld + 1, np.tile(f, (len(ld), 1)))
    d.set_analysis(tol=1e-10)
    d.write_stdb(path)
    return xyz, conn


def test_console_driver_vtu(built_libs, tmp_path):
    """stan_solver --vtu on a 4^3 cube: the file against scalars_ref on the results decoded from the written .STdb.  After
    the narrowing to float32 the copied scalars are equal; a derived scalar within the fp64 bound of its reference (orders
    below half a float32 ulp) narrows to the same float32 or, across a rounding boundary, to its neighbour: 1 float32 ulp."""
    import json
    from stan_amd import host
    exe = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
    plain, path = str(tmp_path / "plain.STdb"), str(tmp_path / "model.STdb")
    _write_model(plain, 4)
    xyz, conn = _write_model(path, 4)
    before = open(path, "rb").read()
    # refused before anything is read: several devices, an unknown result name
    for extra, word in ((["--devices", "0,0"], "one device"), (["--vtu-results", "Stress XX,Stress Q9"], "Stress Q9")):
        out = subprocess.run([exe, "--vtu", str(tmp_path / "no")] + extra + [path], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and word in out.stderr, out.stdout + out.stderr
        assert open(path, "rb").read() == before and not os.path.exists(str(tmp_path / "no_001.vtu"))
    out = subprocess.run([exe, plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    out = subprocess.run([exe, "--json", "--vtu", str(tmp_path / "out"), "--vtu-cells", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(path, "rb").read() == open(plain, "rb").read()          # the .STdb does not know about --vtu
    js = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert js["phases_s"]["result_scalars"] > 0 and js["phases_s"]["write_vtu"] > 0
    disp, strain, stress = host.Db.read_stdb(path).results(1)
    ref = R.Reference(disp, conn, strain, stress)
    vtk, piece, arr = R.parse_vtu(str(tmp_path / "out_001.vtu"))
    assert int(piece["NumberOfPoints"]) == xyz.shape[0] and int(piece["NumberOfCells"]) == conn.shape[0]
    assert np.array_equal(arr["Points"][0][1].reshape(-1, 3), xyz + disp.reshape(-1, 3))
    cel = {n: a for n, a, _ in arr["Cells"]}
    assert np.array_equal(cel["connectivity"].reshape(-1, 8), conn) and (cel["types"] == 12).all()
    assert [n for n, _, _ in arr["PointData"]] == R.NAMES
    assert [n for n, _, _ in arr["CellData"]] == [p + n for n in R.NAMES for p in ("Max ", "Average ", "Min ")]

    def same(got, want, s):
        want32 = want.astype(np.float32)
        assert got.dtype == np.dtype("<f4") and np.isfinite(got).all()
        if s in R.COPIED:
            assert np.array_equal(got, want32), R.NAMES[s]
        else:
            assert (np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)).all(), R.NAMES[s]
    for s in range(24):
        same(arr["PointData"][s][1], ref.point[s], s)
        for j in range(3):
            same(arr["CellData"][3 * s + j][1], ref.cell[s, j], s)
    assert np.abs(arr["PointData"][13][1]).max() > 0
    # a selection by name, without cells
    _write_model(path, 4)
    out = subprocess.run([exe, "--vtu", str(tmp_path / "sel"), "--vtu-results", "von Mises Stress,Displacement X", path],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    _, _, arr2 = R.parse_vtu(str(tmp_path / "sel_001.vtu"))
    assert [n for n, _, _ in arr2["PointData"]] == ["von Mises Stress", "Displacement X"] and arr2["CellData"] == []
    assert np.array_equal(arr2["PointData"][0][1], arr["PointData"][13][1]) and np.array_equal(arr2["PointData"][1][1], arr["PointData"][0][1])
