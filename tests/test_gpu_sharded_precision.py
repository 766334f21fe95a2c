"""Every iterate of the SHARDED CG loop against the long-double CG of tests/product_ref.py, in units of 2^-53: the split product
over the interior and boundary slice lists (cg.hip: launch_product which = 1 / 2), the halo exchange between them (comm.hip,
p2p.hip), the per-rank partial sums combined by an all-reduce or through the mailboxes, the polling of a sharded loop and the
worker threads of multi.hip -- held to the bounds of the one-rank loop (tests/test_gpu_product_precision.py, part C), where the
other sharded tests ask for 1e-4 of max|U| or compare two transports that share everything but the exchange.

Each case is ONE child process (tests/sharded_iterates_worker.py) with its ranks on GPU 0 over the stand-in transport, which
solves with max_its = k for k = 1 .. 22 (FIXED-48: 1 .. 12) in each form and checks nothing; the parent exports the matrix of
the same job from a one-device assembly, unscaled, computes the long-double iterates once per model and load vector and
compares.  Bounds: 4 x the oracle's figures for that model and load vector, 4 x the single-reduction yardstick for the
Chronopoulos-Gear forms -- tests/test_product_ref.py shows that the float64 loop with rank-ordered sums keeps them on 2, 3, 4
and 8 ranks, and that a stale halo, a float32 halo, a rank's partial missing from p . A p and ONE dropped term across a cut do not.
Load case 1 (nonzero in every row) is what catches the dropped term at k = 1.

What runs where (forms: tests/gpu_models.py SHARDED_FORMS; load case 1 with classic, classic_p2p, no_overlap and large):
  cube6 / 2 ranks / sync         every form (fold excepted: the cube folds nothing); both slice lists on both ranks
  perforated12 / 3 / sync        every form, fold included; the middle rank has no interior slice
  cube6 / 3 / async              classic, classic_p2p, separate_reductions, single_reduction, single_reduction_p2p -- and once
                                 more with STAN_P2P_WAIT_MODE 2 (the consuming kernels poll the reductions themselves)
  cube6 / 4 / sync               classic, classic_p2p, no_overlap, large, single_reduction: no rank has an interior slice
  cube6 / 8 / sync               classic, classic_p2p, separate_reductions, single_reduction_p2p, fixed48: ranks 0 and 4 own no row
  perforated12 / 4 / async       classic, classic_p2p, large, fold, single_reduction_p2p

Measured on the device, worst over k, U / residual units, load case 0 (load case 1); a child takes 4 .. 7 s:
  cube6 / 2            classic, classic_p2p, separate_reductions 10.3 / 20.6 (9.6 / 37.9), the same bits; no_overlap 10.3 / 7.7
                       (9.6 / 36.6); large 8.1 / 46.7 (12.6 / 26.7); both single-reduction forms 66.8 / 142.4; fixed48 233.0 /
                       272.8 (bounds 932 / 1061, the one-rank solve reads 233.0 / 267.1)                  bounds 84 / 142 (54 / 217)
  cube6 / 3, both      classic, classic_p2p, separate_reductions 9.4 / 61.6 (9.8 / 23.5); single reduction 33.0 / 73.8 -- wait mode
                       2 gives the figures of the default mode
  cube6 / 4            classic, classic_p2p, no_overlap 7.3 / 96.0 (10.6 / 51.5); large 9.9 / 91.4 (15.8 / 39.3); single_reduction
                       20.7 / 69.5
  cube6 / 8            classic, classic_p2p, separate_reductions 10.7 / 67.3 (12.8 / 47.4); single_reduction_p2p 25.4 / 84.6;
                       fixed48 239.0 / 270.9                                             single reduction: bounds 219 / 380
  perforated12 / 3     classic, classic_p2p 58.8 / 105.5 (14.0 / 21.7); separate_reductions 59.9 / 105.5; no_overlap 56.8 / 103.4
                       (10.5 / 20.4); large 49.5 / 85.6 (9.1 / 18.8); fold 90.8 / 101.3; both single-reduction forms 190.3 / 151.5;
                       fixed48 173.0 / 61.3 (bounds 679 / 190)                    bounds 432 / 346 (130 / 295), 880 / 1299
  perforated12 / 4     classic, classic_p2p 61.9 / 105.5 (15.0 / 23.1); large 55.8 / 85.6 (15.0 / 21.7); fold 68.6 / 101.3;
                       single_reduction_p2p 76.4 / 132.4
-- at or under the float64 restatement with rank-ordered sums (cube6 36 .. 39 / 46 .. 103, perforated12 70 .. 77 / 104 .. 120 in
the classic loop), seven orders under what a float32 halo reads there and ten or more under one dropped term."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stan_amd import hip, host
from tests import product_ref as P
from tests.conftest import fake_rccl_env
from tests.gpu_models import SHARDED_FORMS, SHARDED_PROFILE, model, reduced_reference, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
EVERY = tuple(SHARDED_FORMS)
# (model, nranks, stand-in mode, STAN_P2P_WAIT_MODE, forms)
CASES = [
    ("cube6", 2, "sync", None, tuple(f for f in EVERY if f != "fold")),
    ("perforated12", 3, "sync", None, EVERY),
    ("cube6", 3, "async", None, ("classic", "classic_p2p", "separate_reductions", "single_reduction", "single_reduction_p2p")),
    ("cube6", 3, "async", 2, ("classic", "classic_p2p", "separate_reductions", "single_reduction", "single_reduction_p2p")),
    ("cube6", 4, "sync", None, ("classic", "classic_p2p", "no_overlap", "large", "single_reduction")),
    ("cube6", 8, "sync", None, ("classic", "classic_p2p", "separate_reductions", "single_reduction_p2p", "fixed48")),
    ("perforated12", 4, "async", None, ("classic", "classic_p2p", "large", "fold", "single_reduction_p2p")),
]
PROF = {name: i for i, name in enumerate(SHARDED_PROFILE + ("repacked_streams",))}


def _run(tmp_path, name, nranks, fake_mode, wait_mode, forms):
    out = str(tmp_path / "iterates.npz")
    env = dict(os.environ, STAN_RCCL_LIB=FAKE, **fake_rccl_env(fake_mode))
    env["GPU_MAX_HW_QUEUES"] = str(2 * nranks + 4)
    if wait_mode is not None:
        env["STAN_P2P_WAIT_MODE"] = str(wait_mode)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sharded_iterates_worker.py"), name, str(nranks), out, ",".join(forms)],
                       capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    ok = p.returncode == 0 and p.stdout.strip().endswith("SHARDED_ITERATES_WORKER_OK")
    assert ok, "worker exit code %d\n%s%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return np.load(out)


def _census_serves_the_case(name, nranks, csr, d):
    """The cut is the host plan's, on the device too, and it has what the case is there for (tests/test_product_ref.py reads
    the same off the oracle's pattern)."""
    j = P.job(name)
    rs = host.partition_plan(j.node_index, j.conn, nranks, 0)["row_starts"]
    assert np.array_equal(d["row_begin"], rs[:-1]) and np.array_equal(d["row_end"], rs[1:])
    rank = P.rank_of_rows(j, nranks)
    owners = np.unique(rank)
    assert np.array_equal(np.unique(rank[P.rows_of(csr[0])[P.halo_entries(csr, rank)]]), owners)     # every rank with rows reads a halo
    census = P.slice_census(j, csr, nranks)
    if (name, nranks) == ("cube6", 2):
        assert all(i > 0 and b > 0 for i, b in census), census
    if (name, nranks) == ("cube6", 4):
        assert any(i == 0 and b > 0 for i, b in census), census
    if (name, nranks) == ("cube6", 8):
        assert any(i + b == 0 for i, b in census) and owners.shape[0] < nranks, census
    return census


@pytest.mark.parametrize("name,nranks,fake_mode,wait_mode,forms", CASES,
                         ids=["%s-%d-%s%s" % (c[0], c[1], c[2], "" if c[3] is None else "-wait%d" % c[3]) for c in CASES])
def test_every_iterate_of_the_sharded_loop_against_the_long_double_cg(gpu_ctx, tmp_path, name, nranks, fake_mode, wait_mode, forms):
    """For every form of the case and every k: termination type 5 after exactly k iterations, U finite and of the job's length,
    max|U - U_k| / max|U_k| and |rel_residual / ref - 1| within 4 x the oracle's figures in units of 2^-53 (the single-reduction
    forms: 4 x the float64 restatement of their recurrences).  fixed48: the recurrence's own residual from the profile against
    the long-double CG on the matrix quantised from long-double entries, bound 4 x the float64 loop on the matrix quantised
    from float64 entries, measured on the exported matrix (test_every_iterate_of_a_reduced_precision_solve says why), and the
    profile names the FIXED-48 stream.  classic and classic_p2p are the same bits at every k, and so are the two
    single-reduction forms; the peer-to-peer forms launch no collective and wait on the stream instead; fold reads a folded
    copy (repacked_streams == 1).  The device deals the rows as the host plan does and the cut has what the case is there for."""
    j = P.job(name)
    csr, _probes = model(gpu_ctx, name)
    d = _run(tmp_path, name, nranks, fake_mode, wait_mode, forms)
    census = _census_serves_the_case(name, nranks, csr, d)
    print("%s on %d ranks (%s%s): slices (interior, boundary) %s" % (name, nranks, fake_mode, "" if wait_mode is None else ", wait mode %d" % wait_mode, census))
    assert list(d["forms"]) == list(forms)
    over = []
    for form in forms:
        _opts, prec, kmax, cases = SHARDED_FORMS[form]
        for lc in cases:
            key = "%s_lc%d_" % (form, lc)
            U, rep, rel, prof = d[key + "U"], d[key + "rep"], d[key + "rel"], d[key + "prof"]
            assert U.shape == (kmax, j.n_red) and np.isfinite(U).all() and np.isfinite(rel).all()
            assert np.array_equal(rep, [[5, k] for k in range(1, kmax + 1)]), (form, lc, rep)
            if form == "fixed48":
                Us, rels = reduced_reference(gpu_ctx, name, "fixed48")
                its = P.cg_iterates(P.Scaled(*csr, T=np.float64, quantise=P.quantise_fixed48), j.F, kmax)
                bu = P.DEVICE_CG_FACTOR * max(P.u_units(x, Us[k]) for k, (x, _r) in enumerate(its))
                br = P.DEVICE_CG_FACTOR * max(P.res_units(r, rels[k]) for k, (_x, r) in enumerate(its))
                rel = prof[:, PROF["rel_residual_recurrence"]]
                assert (prof[:, PROF["value_stream"]] == hip.PREC_FIXED48).all(), prof[:, PROF["value_stream"]]
            else:
                Us, rels = reference(gpu_ctx, name, lc)
                bu, br = P.sharded_cg_bounds(name, lc, single_reduction=form.startswith("single_reduction"))
                assert (prof[:, PROF["value_stream"]] == hip.PREC_FP64).all()
            u = [P.u_units(U[k], Us[k]) for k in range(kmax)]
            r = [P.res_units(rel[k], rels[k]) for k in range(kmax)]
            print("sharded cg %s on %d ranks, %s, load case %d: worst over k = 1 .. %d: U %.1f units (bound %.0f), residual %.1f units (bound %.0f)" %
                  (name, nranks, form, lc, kmax, max(u), bu, max(r), br))
            over += [(form, lc, k + 1, u[k], r[k], bu, br) for k in range(kmax) if u[k] > bu or r[k] > br]
            if form.endswith("_p2p"):
                assert (prof[:, PROF["loop_collectives"]] == 0).all() and (prof[:, PROF["loop_stream_waits"]] > 0).all(), form
                twin = form[:-len("_p2p")]
                if twin in forms:
                    assert np.array_equal(U, d["%s_lc%d_U" % (twin, lc)]) and np.array_equal(rel, d["%s_lc%d_rel" % (twin, lc)]), (form, lc)
            else:
                assert (prof[:, PROF["loop_collectives"]] > 0).all() and (prof[:, PROF["loop_stream_waits"]] == 0).all(), form
            if form == "fold":       # (no silent fallback to the padded streams; a later form may report the copy this one left)
                assert (prof[:, PROF["repacked_streams"]] == 1).all(), prof[:, PROF["repacked_streams"]]
    assert not over, over
