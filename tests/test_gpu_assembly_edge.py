"""Meshes the reference accepts and the assembly's fast paths do not cover (Database.cs:149-176, SolverFunctions.cs:143-173,
Node.cs:202-205 bound neither the elements at a node nor repeats in NList): collapsed hexes, solids of revolution with a
high-valence axis, star meshes, thousands of incidences at one node -- in both assembly modes, sharded, and through
stress recovery.  K_TOL is the fixed bar against the oracle; the conditioning-aware bar (entrywise, in units of an
extended-precision reference's rounding scale, k_numeric_wide and the colour scatter included) lives in
tests/test_gpu_element_precision.py / tests/element_ref.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import problem
from stan_amd.cube import cube_mesh, revolved_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
U_TOL = 1e-6
K_TOL = 1e-13
OPT_ASSEMBLY_MODE = 5
OPT_FOLD = 19
OPT_SELL_SIGMA, OPT_MERIT = 17, 1


def _job(xyz, conn, load=(0.0, 10.0, 5.0)):
    z0 = np.nonzero(xyz[:, 2] == xyz[:, 2].min())[0]
    top = np.nonzero(xyz[:, 2] == xyz[:, 2].max())[0]
    return problem.make_job(xyz, conn, z0, np.ones((len(z0), 3)), top, np.tile(load, (len(top), 1)))


def _check_against_oracle(ctx, oracle, job, mode, cg_eps=1e-10, u_tol=1e-6):
    ctx.set_option(OPT_ASSEMBLY_MODE, mode)
    try:
        K = ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    finally:
        ctx.set_option(OPT_ASSEMBLY_MODE, 0)
    rc, A = oracle.assemble(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    assert rc == 0
    rowptr, col, val = K.to_csr()
    assert np.array_equal(rowptr, A.ridx) and np.array_equal(col, A.idx)          # pattern: bit-equal
    kerr = np.abs(val - A.vals).max() / np.abs(A.vals).max()
    assert kerr <= K_TOL, kerr
    # merit-function stop off on both sides (its type-7 stop lands wherever rounding lets the merit tick up): the residual
    # test is the comparable end state; tolerance: |dU| <= u_tol max|U| (north-star bar 1e-6)
    ctx.set_option(1, 0)
    try:
        U, rep = K.cg_solve(job.F, cg_eps, 50000)
    finally:
        ctx.set_option(1, 1)
    Uo, repo = oracle.cg(A, job.F, cg_eps, 50000, merit_stop=False)
    assert rep["terminationtype"] == repo["terminationtype"] == 1, (rep, repo)
    assert abs(rep["iterations"] - repo["iterations"]) <= max(5, repo["iterations"] // 10), (rep, repo)
    assert np.abs(U - Uo).max() <= u_tol * np.abs(Uo).max()
    info = K.info()
    K.free()
    return info, kerr


@pytest.mark.parametrize("mode", [0, 1])
def test_wedge_collapsed_hex(gpu_ctx, oracle, mode):
    """A hex that lists a node twice (CHEXA wedge: node 4 := node 1, node 8 := node 5) in the middle of a 3^3 cube and
    on its corner: k_numeric's duplicate-node branch (assembly.hip) and k_scatter's (assembly_scatter.hip), which no
    GPU test fed before.  The reference accepts such elements (Node.cs:202-205)."""
    from stan_amd.cube import cube_bcs
    xyz, conn = cube_mesh(3, jitter=0.05)
    for e in (13, 0, 26):
        conn[e, 3], conn[e, 7] = conn[e, 0], conn[e, 4]
    spc, ld, f = cube_bcs(3)                 # (from the grid indices: the jittered coordinates have no exact planes)
    job = problem.make_job(xyz, conn, spc, np.ones((len(spc), 3)), ld, np.tile(f, (len(ld), 1)))
    info, _ = _check_against_oracle(gpu_ctx, oracle, job, mode)
    assert info["n_blocks"] > 0


@pytest.mark.parametrize("mode", [0, 1])
def test_revolved_mesh_with_72_collapsed_hexes_on_the_axis(gpu_ctx, oracle, mode):
    """VERDICT r03 missing 3: a solid of revolution in 5-degree sectors -- 72 collapsed hexes at every axis node, each
    listing it twice: 288 (element, local node) incidences (the fast symbolic kernel takes 64) and a row of 219 blocks
    (the fast numeric kernel's LDS takes 96).  The reference solves it (Database.cs:149-176, SolverFunctions.cs:143-173
    put no bound on the elements at a node); so does the library now: k_symbolic_big, k_fill_cols in chunks,
    k_numeric_wide; the colour scatter with as many colours as it takes."""
    xyz, conn = revolved_mesh(72, 2, 3)
    info, _ = _check_against_oracle(gpu_ctx, oracle, _job(xyz, conn), mode)
    assert info["max_row_blocks"] == 3 * (72 + 1)


@pytest.mark.parametrize("k,rings", [(20, 1), (33, 1), (40, 2), (130, 1)])
def test_star_meshes_beyond_the_old_limits(gpu_ctx, oracle, k, rings):
    """The jobs tests/test_gpu_parity.py used to expect STAN_E_VALENCE for (k = 20: a 123-block row; k = 33: 66
    incidences) and beyond (k = 40; k = 130: 260 incidences, 783 blocks): they assemble, pattern bit-equal, values to
    1e-13, and solve."""
    from stan_amd.cube import star_mesh
    xyz, conn = star_mesh(k, 3, rings)
    info, _ = _check_against_oracle(gpu_ctx, oracle, _job(xyz, conn), 0)
    if rings == 1:
        assert info["max_row_blocks"] == 3 * (2 * k + 1)


def test_a_node_with_thousands_of_incidences(gpu_ctx, oracle):
    """Beyond what the LDS sort of k_symbolic_big holds (3640 incidences): 1000 sectors x 2 layers x 2 listings = 4000
    at the interior axis node -- the global-scratch form of the same sort."""
    xyz, conn = revolved_mesh(1000, 1, 2)
    job = _job(xyz, conn)
    K = gpu_ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    rc, A = oracle.assemble(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    rowptr, col, val = K.to_csr()
    assert np.array_equal(rowptr, A.ridx) and np.array_equal(col, A.idx)
    assert np.abs(val - A.vals).max() <= 1e-12 * np.abs(A.vals).max()    # 4000 terms in one diagonal block
    assert K.info()["max_row_blocks"] == 3 * 1001
    x = np.random.default_rng(3).standard_normal(job.n_red)
    y = K.spmv(x)
    yo = A.to_scipy_full() @ x
    assert np.abs(y - yo).max() <= 1e-11 * np.abs(yo).max()
    K.free()


def test_fuzz_with_five_percent_collapsed_elements(gpu_ctx, oracle):
    """tests/fuzz.py jobs (shuffled wire order, knocked-out elements, two materials, partial SPCs) with 5 % of the
    elements collapsed into wedges: pattern bit-exact, values, CG against the oracle (fuzz.check_job), both modes'
    assembly."""
    from tests import fuzz
    done = 0
    for seed in range(300, 340):
        job = fuzz.random_job(seed, collapse=0.05)
        if job is None or job.has_g1:
            continue
        ncol = int((job.conn[:, 3] == job.conn[:, 0]).sum())
        if ncol == 0:
            continue
        fuzz.check_job(gpu_ctx, oracle, job)
        gpu_ctx.set_option(OPT_ASSEMBLY_MODE, 1)
        try:
            fuzz.check_job(gpu_ctx, oracle, job, cg=False)
        finally:
            gpu_ctx.set_option(OPT_ASSEMBLY_MODE, 0)
        done += 1
    assert done >= 10


def test_shards_of_the_revolved_mesh(built_libs):
    """The slow paths on a rank of a sharded run (halo discovery in k_symbolic_big): device plan == host plan, every
    shard reproduces its rows of the unsharded product bit for bit."""
    from stan_amd import hip
    from tests import fuzz
    xyz, conn = revolved_mesh(72, 2, 3)
    fuzz.check_shards(lambda: hip.Context(0), _job(xyz, conn), 3)


def test_stress_recovery_and_nodal_forces_on_collapsed_hexes(gpu_ctx, oracle):
    """Element.Recovery_Stress / Compute_NodalForces (Element.cs:211-255) on the revolved mesh: the wedge-collapsed hexes
    on the axis list a node twice -- their 8x6 strain / stress blocks (two rows then belong to the same node, each
    extrapolated with its own shape-function row, as the reference does) and the R assembly, where the repeated node
    receives both listings' forces, against the oracle element by element."""
    xyz, conn = revolved_mesh(24, 2, 2)
    job = _job(xyz, conn)
    disp = np.random.default_rng(11).standard_normal(job.xyz.shape) * 1e-3
    strain, stress = gpu_ctx.recover_hex8(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    f, R = gpu_ctx.nodal_forces_hex8(job.xyz, disp, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    fo = np.zeros_like(f)
    E, nu = job.mat_E_nu[0]
    ncollapsed = 0
    for e in range(job.conn.shape[0]):
        rc, eo, so = oracle.recover_hex8(job.xyz[job.conn[e]], E, nu, 2, disp[job.conn[e]].ravel())
        rc2, fo[e] = oracle.nodal_forces_hex8(job.xyz[job.conn[e]], 2, so)
        assert rc == 0 and rc2 == 0
        assert np.abs(strain[e] - eo).max() <= 1e-11 * np.abs(eo).max()
        assert np.abs(stress[e] - so).max() <= 1e-11 * np.abs(so).max()
        ncollapsed += job.conn[e, 0] == job.conn[e, 3]
    assert ncollapsed == 48
    assert np.abs(f - fo).max() <= 1e-11 * np.abs(fo).max()
    Ro = np.zeros(job.n_dof)
    np.add.at(Ro, job.node_dof[job.conn].reshape(-1, 24), fo)
    assert np.abs(R - Ro).max() <= 1e-10 * np.abs(Ro).max()
