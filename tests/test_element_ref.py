"""The element reference of tests/element_ref.py, the parts that need no GPU: the longdouble reference against mpmath, the
yardsticks the device bounds derive from (measured on the oracle, on every run), and mutants of the fp64 restatement that
the conditioning-aware bound must catch where the fixed bars of tests/test_gpu_parity.py (1e-13 of max|K_e|, 1e-12 of the
largest strain / stress) let them through."""
import numpy as np
import pytest

from tests import element_ref as R

K_TOL_OLD, REC_TOL_OLD = 1e-13, 1e-12      # tests/test_gpu_parity.py: test_ke_parity, test_stress_recovery_parity
FIELDS = ("random", "rigid", "affine")


def _oracle_ke(oracle, X, E, nu, etype):
    out = np.empty((X.shape[0], 24, 24))
    for k, x in enumerate(X):
        rc, out[k] = oracle.ke_hex8(x, E, nu, etype)
        assert rc == 0
    return out


def _oracle_rec(oracle, X, u, E, nu):
    e, s = np.empty((X.shape[0], 8, 6)), np.empty((X.shape[0], 8, 6))
    for k in range(X.shape[0]):
        rc, e[k], s[k] = oracle.recover_hex8(X[k], E, nu, R.G2, u[k].ravel())
        assert rc == 0
    return e, s


def _ke_units(fn):
    """group -> worst units of fn(X, E, nu, etype) -> K [k, 24, 24] over both element types; and the elements compared."""
    worst, seen = {}, 0
    for name in R.family():
        worst[name] = 0.0
        for etype in (R.G1, R.G2):
            for X, E, nu, K, S in R.ke_reference(name, etype):
                worst[name] = max(worst[name], R.units(fn(X, E, nu, etype), K, S))
                seen += X.shape[0]
    return worst, seen


def _rec_units(fn):
    """group -> worst units of fn(X, u, E, nu) -> (strain, stress) over the three fields; and the elements compared."""
    worst, seen = {}, 0
    for name in R.family():
        worst[name] = 0.0
        for field in FIELDS:
            X, u, e, s, Se, Ss = R.rec_reference(name, field)
            ge, gs = fn(X, u, *R.REC_MATERIAL)
            worst[name] = max(worst[name], R.units(ge, e, Se), R.units(gs, s, Ss))
            seen += X.shape[0]
    return worst, seen


def _show(title, worst):
    print("%s, worst units of 2^-52 S per group: %s" % (title, ", ".join("%s %.3f" % kv for kv in worst.items())))
    return max(worst.values())


def _family_size():
    return sum(X.shape[0] for parts in R.family().values() for X, _E, _nu in parts)


def test_family_has_the_groups_and_is_seeded():
    fam, again = R.family(), R.family()
    assert list(fam) == ["plain", "shift_1e3", "shift_1e6", "aspect_rot", "aspect_rot_shift_1e4", "thin_1e-4", "nu_0.4999",
                         "nu_0", "micro_E_2.1e11", "aspect_rot_shift_union", "materials", "unit_cube"]
    for name in fam:
        assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(fam[name], again[name])), name
    assert [(E, nu) for _X, E, nu in fam["materials"]] == R.MIXED_MATERIALS
    assert np.array_equal(fam["unit_cube"][0][0][0], R.UNIT)
    # every element is a valid one at every Gauss point of both types: the device must not answer STAN_E_DETJ anywhere
    for name, X in R.geometries(fam).items():
        for etype in (R.G1, R.G2):
            for q in R.gauss_points(R.LD, R.LD.arr(X), etype):
                assert (q["det"] > 0).all(), name


def test_longdouble_reference_agrees_with_mpmath():
    """|LD - mpmath at 50 digits| <= 2^-10 units of the scale on elements of every group (K_e of both types, the three
    recovery fields), and the two scales agree: the reference's own error cannot blur the device bounds."""
    import mpmath
    M = R.mp()
    worst = 0.0

    def check(ld, ex, S):
        nonlocal worst
        with mpmath.workdps(50):
            d = abs(R.to_mp(ld) - ex) / (R.U52 * S)
            worst = max(worst, float(max(d.ravel())))

    with mpmath.workdps(50):
        for name, parts in R.family().items():
            for p, (X, E, nu) in enumerate(parts[::2]):                       # materials: nu = 0.3, 0.4999, -0.2
                for k, etype in ((0, R.G2), (X.shape[0] // 2, R.G1), (X.shape[0] - 1, R.G2 if p else R.G1)):
                    x = X[k:k + 1]
                    K, S = R.ke(R.LD, x, E, nu, etype)
                    Km, Sm = R.ke(M, x, E, nu, etype)
                    check(K, Km, Sm)
                    assert float(max((abs(R.to_mp(S) - Sm) / Sm).ravel())) < 1e-6        # (a yardstick: a few digits are enough)
            X = R.geometries()[name]
            for j, field in enumerate(FIELDS):
                k = (j * (X.shape[0] - 1)) // 2
                x, u = X[k:k + 1], R.fields(X)[field][k:k + 1]
                ld, ex = R.recover(R.LD, x, u, *R.REC_MATERIAL), R.recover(M, x, u, *R.REC_MATERIAL)
                check(ld[0], ex[0], ex[2])
                check(ld[1], ex[1], ex[3])
    print("longdouble against mpmath: worst %.2e units of 2^-52 S (bar 2^-10 = %.2e)" % (worst, 2.0 ** -10))
    assert worst <= 2.0 ** -10


def test_yardsticks_are_measured_on_the_oracle(oracle):
    """The oracle's K_e and recovery over the whole family in units of 2^-52 S: within twice what element_ref records (the
    device is held to 4 x the recorded values)."""
    ke_worst, n_ke = _ke_units(lambda X, E, nu, etype: _oracle_ke(oracle, X, E, nu, etype))
    rec_worst, n_rec = _rec_units(lambda X, u, E, nu: _oracle_rec(oracle, X, u, E, nu))
    ke_max, rec_max = _show("oracle K_e", ke_worst), _show("oracle strain / stress", rec_worst)
    print("recorded: K_e %.2f, recovery %.2f; device bounds %.2f / %.2f" %
          (R.ORACLE_KE_UNITS_MEASURED, R.ORACLE_REC_UNITS_MEASURED, R.DEVICE_KE_UNITS, R.DEVICE_REC_UNITS))
    assert n_ke == 2 * _family_size() and n_rec == 3 * _family_size()            # no element left out
    assert ke_max < 2 * R.ORACLE_KE_UNITS_MEASURED and rec_max < 2 * R.ORACLE_REC_UNITS_MEASURED
    assert R.DEVICE_KE_UNITS == 4 * R.ORACLE_KE_UNITS_MEASURED and R.DEVICE_REC_UNITS == 4 * R.ORACLE_REC_UNITS_MEASURED
    # the recorded values are measurements, not allowances: the oracle is not far below them either
    assert ke_max > 0.5 * R.ORACLE_KE_UNITS_MEASURED and rec_max > 0.5 * R.ORACLE_REC_UNITS_MEASURED


def test_fp64_restatement_meets_the_device_bounds_on_every_group():
    ke_worst, n_ke = _ke_units(lambda X, E, nu, etype: R.ke(R.F64, X, E, nu, etype)[0])
    rec_worst, n_rec = _rec_units(lambda X, u, E, nu: R.recover(R.F64, X, u, E, nu)[:2])
    assert n_ke == 2 * _family_size() and n_rec == 3 * _family_size()
    assert _show("fp64 restatement K_e", ke_worst) <= R.DEVICE_KE_UNITS
    assert _show("fp64 restatement strain / stress", rec_worst) <= R.DEVICE_REC_UNITS


def test_rigid_and_affine_fields_have_their_exact_strains():
    """The reference's strain under the rigid field is zero and under the affine one sym(A) (shear as stored), up to the one
    rounding of the field: FIELD_ROUNDING_UNITS of the scale, on every group."""
    for name in R.family():
        for field, exact in (("rigid", 0.0), ("affine", R.AFFINE_STRAIN)):
            _X, _u, e, _s, Se, _Ss = R.rec_reference(name, field)
            assert (abs(e - exact) <= R.FIELD_ROUNDING_UNITS * R.U52 * Se).all(), (name, field)


def test_new_bound_is_ten_times_tighter_than_the_fixed_bar_on_the_plain_group():
    for etype in (R.G1, R.G2):
        for _X, _E, _nu, K, S in R.ke_reference("plain", etype):
            assert (R.DEVICE_KE_UNITS * R.U52 * S <= 1e-14 * abs(K).max(axis=(1, 2), keepdims=True)).all()


# old_ke: what the fixed K_e bar says of the mutant (True: passes it; None: printed only, see the docstring below)
MUTANTS = {
    "gauss_location_1e-13": dict(ke=dict(gl_rel=1e-13), rec=dict(gl_rel=1e-13), old_ke=None),
    "gauss_location_5e-14": dict(ke=dict(gl_rel=5e-14), rec=None, old_ke=True),
    "extrapolation_sqrt3_1e-13": dict(ke=None, rec=dict(s3_rel=1e-13), old_ke=None),
    "no_transpose": dict(ke=dict(transpose=False), rec=None, old_ke=False),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bound_tells_a_mutant_from_the_restatement(oracle, mutant):
    """A subtly wrong fp64 restatement exceeds the device bound on the plain group, where the precision mutants pass the
    fixed bars of the parity tests against the oracle -- the gap the conditioning-aware bar closes.  Measured: a Gauss
    location or a sqrt 3 off by 1e-13 moves strain and stress by 1.9e-13 of the element's largest (fixed bar 1e-12: passes)
    and by 49 / 47 units (bound 4.84: caught).  K_e moves with the Gauss location by 1.34 times its relative error (K_e is
    quadratic in it), so the 1e-13 mutant lands at 1.1e-13 .. 1.34e-13 of max|K_e|, on the fixed 1e-13 bar rather than under
    it, and at 57 units (bound 2.4); the same mutant at 5e-14 is under the fixed bar (6.7e-14) and still at 29 units: that
    one carries the assertion on the fixed K_e bar."""
    m = MUTANTS[mutant]
    if m["ke"] is not None:
        for etype in ((R.G2,) if "gl_rel" in m["ke"] else (R.G1, R.G2)):       # HEX8_G1 has no Gauss location to get wrong
            for X, E, nu, K, S in R.ke_reference("plain", etype):
                Km = R.ke(R.F64, X, E, nu, etype, **m["ke"])[0]
                got = R.units(Km, K, S)
                print("%s: K_e G%d %.1f units (bound %.2f)" % (mutant, etype, got, R.DEVICE_KE_UNITS))
                assert got > R.DEVICE_KE_UNITS
                Ko = _oracle_ke(oracle, X, E, nu, etype)
                old = (np.abs(Km - Ko).max(axis=(1, 2)) / np.abs(Ko).max(axis=(1, 2))).max()
                print("%s: K_e G%d %.2e of max|K_e| against the oracle (fixed bar %.0e)" % (mutant, etype, old, K_TOL_OLD))
                assert m["old_ke"] is None or (old <= K_TOL_OLD) == m["old_ke"]
    if m["rec"] is not None:
        X, u, e, s, Se, Ss = R.rec_reference("plain", "random")
        em, sm = R.recover(R.F64, X, u, *R.REC_MATERIAL, **m["rec"])[:2]
        got = max(R.units(em, e, Se), R.units(sm, s, Ss))
        print("%s: strain / stress %.1f units (bound %.2f)" % (mutant, got, R.DEVICE_REC_UNITS))
        assert got > R.DEVICE_REC_UNITS
        eo, so = _oracle_rec(oracle, X, u, *R.REC_MATERIAL)
        old = max((np.abs(em - eo).max(axis=(1, 2)) / np.abs(eo).max(axis=(1, 2))).max(),
                  (np.abs(sm - so).max(axis=(1, 2)) / np.abs(so).max(axis=(1, 2))).max())
        print("%s: strain / stress %.2e of the element's largest against the oracle (fixed bar %.0e)" % (mutant, old, REC_TOL_OLD))
        assert old <= REC_TOL_OLD


def test_scatter_counts_every_listing():
    """scatter_dense on a 2-element strip with one collapsed hex: the repeated node receives both listings, fixed DOFs drop."""
    from tests import forces_ref
    xyz, conn = forces_ref.strip_mesh(2)
    conn[1, 3], conn[1, 7] = conn[1, 0], conn[1, 4]
    m = forces_ref.model(xyz, conn)
    vals = np.random.default_rng(2).standard_normal((2, 24, 24))
    D = R.scatter_dense(m, vals)
    full = np.zeros((m.n_dof, m.n_dof))
    dof = np.asarray(m.node_dof).reshape(-1, 3)[m.conn].reshape(-1, 24)
    for e in range(2):
        for i in range(24):
            for j in range(24):
                full[dof[e, i], dof[e, j]] += vals[e, i, j]
    free = np.nonzero(np.asarray(m.red) >= 0)[0]
    assert free.size == m.n_red
    assert np.abs(D.astype(np.float64) - full[np.ix_(free, free)]).max() <= 1e-15 * np.abs(full).max() and m.n_fixed > 0
