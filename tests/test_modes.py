"""The references of the modal analysis (tests/modes_ref.py) on the CPU: the lumped mass adds up to rho * volume, the numpy
restatement of the driver loop (exact inner solves) converges on the model with degenerate pairs, and its eigenvalues meet the
bound the device is held to (tests/test_gpu_modes.py)."""
import numpy as np
import pytest

from tests import modes_ref as R


@pytest.mark.parametrize("name", ["cube6", "two_mat"])
def test_lumped_mass_adds_up_to_rho_times_volume(name):
    """sum_a N_a = 1: the nodal masses add up to sum_m rho_m volume_m.  Every term is positive, so relative errors do not grow:
    a corner weight is 8 products and 7 additions of rounded shape values (< 12 units of 2^-53), a node adds at most 8 of them,
    the pairwise sums over 343 nodes and 216 elements add log2 + 1 each: 64 units cover both sides."""
    j = R.job(name)
    rho = R.mat_rho(name)
    M, mass_node, l, _ = R.lumped_mass(j, rho)
    from tests import loads_ref as L
    want = 0.0
    for m, r in enumerate(rho):     # the volume of material m: the body sum with b = 1 on that material alone
        body = np.zeros((len(rho), 3))
        body[m, 0] = 1.0
        want += r * L.loads_np(j, L.Case(mat_body=body))[1]
    assert abs(mass_node.sum() - want) <= 64 * R.U53 * want
    # by direction: the mass on free DOFs + the mass on supports = the total
    d0 = np.asarray(j.node_dof).reshape(-1, 3)[:, 0]
    red = np.asarray(j.red)
    for c in range(3):
        fixed = red[d0 + c] == -1
        assert abs(mass_node[~fixed].sum() + mass_node[fixed].sum() - want) <= 64 * R.U53 * want
    assert M.shape[0] == j.n_red and (M > 0).all()
    assert abs(M.sum() + sum(mass_node[red[d0 + c] == -1].sum() for c in range(3)) - 3 * want) <= 64 * R.U53 * 3 * want


def test_start_block_is_fixed_and_in_range():
    M = np.linspace(1.0, 2.0, 1000)
    X = R.start_block(M, 5)
    assert np.array_equal(X, R.start_block(M, 5)) and np.array_equal(X[0], M)
    assert (X[1:] >= -0.5).all() and (X[1:] < 0.5).all()
    assert abs(X[1:].mean()) < 0.02 and np.linalg.matrix_rank(X) == 5


def test_restatement_converges_on_the_degenerate_cube(oracle):
    ref = R.reference("cube6")
    k = ref["k"]
    pairs = [c for c in R.clusters(ref["lam"], k) if c[1] - c[0] == 2]
    assert len(pairs) >= 2, "the y and z bending pairs of the clamped cube must be degenerate"
    r = R.restatement(ref["Kd"], ref["M"], k, tol=1e-8, max_outer=100)
    assert r["converged"] and r["outer"] < 100 and (r["rho"] <= 1e-8).all()
    assert (np.abs(r["lam"] - ref["lam"][:k]) <= 2 * 1e-6 * ref["lam"][:k]).all()     # the bound of the GPU test at its tol
    assert (R.rho_host(ref["Kd"], ref["M"], r["lam"], r["phi"]) <= 2e-8).all()
    G = (r["phi"] * ref["M"][None, :]) @ r["phi"].T
    assert np.abs(G - np.eye(k)).max() < 1e-13
    for a, b, gap in R.clusters(ref["lam"], k):
        s = R.sin_max_angle(r["phi"][a:b].T, ref["Phi"][:, a:b], ref["M"])
        assert s <= 2 * (r["rho"][a:b] * r["lam"][a:b]).max() / gap, (a, b, s)
    # the sign rule: the entry of largest magnitude is positive
    for x in r["phi"]:
        assert x[np.argmax(np.abs(x))] > 0


def _density_db(mats):
    from stan_amd import host
    from stan_amd.cube import cube_mesh
    xyz, conn = cube_mesh(3)
    d = host.Db()
    ne = conn.shape[0]
    d.set_mesh(np.arange(1, xyz.shape[0] + 1), xyz, np.arange(1, ne + 1), np.ones(ne), conn + 1, "HEX8_G2")
    for mid, E, nu in mats:
        d.add_material(mid, "Steel%d" % mid, E, nu)
    d.assign_part(1, mats[0][0], "HEX8_G2")
    fixed = np.nonzero(xyz[:, 0] == 0.0)[0]
    d.add_bc(1, "fix", "SPC", fixed + 1, np.ones((fixed.size, 3)))
    return d


def _col0(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.column_stack([v, np.zeros(v.size), np.zeros(v.size)])


def test_density_bc_through_the_host_library(tmp_path, built_libs):
    """The "Density" BoundaryCondition Type: material IDs, component 0 = rho, resolved like "ThermalExpansion"; several entries
    add up, the file round-trips, an unknown material is an error, and the other BCs are read as before."""
    from stan_amd import host
    d = _density_db(((1, 210000.0, 0.3), (7, 70000.0, 0.33)))
    d.add_bc(2, "steel", "Density", [1, 7], _col0([7.85e-9, 2.7e-9]))
    d.add_bc(3, "more", "Density", [7], _col0([1.0e-10]))
    d.assign_dof()
    path = str(tmp_path / "m.STdb")
    d.write_stdb(path)
    d = host.Db.read_stdb(path)
    d.assign_dof()
    got = d.density()
    assert got["any"] and np.array_equal(got["mat_rho"], [7.85e-9, 2.7e-9 + 1.0e-10])
    assert not d.thermal_loads()["any"] and not d.distributed_loads()["any"]
    plain = _density_db(((1, 210000.0, 0.3), (7, 70000.0, 0.33)))
    plain.assign_dof()
    assert not plain.density()["any"] and not plain.density()["mat_rho"].any()
    (red, nf, F), (red0, nf0, F0) = d.reduction(), plain.reduction()
    assert np.array_equal(red, red0) and nf == nf0 and np.array_equal(F, F0)
    bad = _density_db(((1, 210000.0, 0.3),))
    bad.add_bc(2, "a", "Density", [2], _col0([7.85e-9]))     # node 2 exists, material 2 does not
    bad.assign_dof()
    with pytest.raises(host.StanHostError) as ei:
        bad.density()
    assert "material 2" in str(ei.value)
