"""The frequency response without a GPU: the physics of tests/harmonic_ref.py, reference against
reference, and the console's refusals.

Physics, on modes_ref's cube6j and two_mat with ALL N eigenpairs from scipy.linalg.eigh:
  Y           the full modal sum in long double against the dense complex solve, relative to the largest entry of the solve: what
              the two references agree to (eigh's vectors and the solve are fp64).  The yardstick; printed.
  corrected   k = 8 modes with the static correction, plus the exact remainder sum_{j>k} phi_j p_j (H_j - 1 / lambda_j), against the
              solve within 4 Y: the correction is the static response of the modes left out, nothing else
  plain       the same without the correction, the remainder sum_{j>k} phi_j p_j H_j
  truncation  what the correction buys: the error of k = 8 modes without and with it (printed, and the second must be the smaller)
at w = 0, 0.5 w_1, (w_1 + w_2) / 2 and 1.02 w_1, with Rayleigh damping and with zeta = 0.02 on every mode."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

from tests import harmonic_ref as H
from tests import modes_ref as R

LD = np.longdouble
K_TRUNC = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
_full = {}


def full_basis(name, oracle):
    """dict(Kd, M, F, lam [N], Phi [N, N], us): every eigenpair, and K^-1 F refined twice with long-double residuals; computed once."""
    if name not in _full:
        r = R.reference(name)
        Kd, M = r["Kd"], r["M"]
        F = np.asarray(H.job(name).F, dtype=np.float64)
        lam, Phi = scipy.linalg.eigh(Kd, np.diag(M))
        cho = scipy.linalg.cho_factor(Kd)
        us = scipy.linalg.cho_solve(cho, F).astype(LD)
        Kl = Kd.astype(LD)
        for _ in range(2):
            us = us + scipy.linalg.cho_solve(cho, (F.astype(LD) - Kl @ us).astype(np.float64)).astype(LD)
        _full[name] = dict(Kd=Kd, M=M, F=F, lam=lam, Phi=Phi, us=us)
    return _full[name]


def _cases(b):
    w1, w2 = np.sqrt(b["lam"][0]), np.sqrt(b["lam"][1])
    omega = np.array([0.0, 0.5 * w1, 0.5 * (w1 + w2), 1.02 * w1])
    N = b["lam"].shape[0]
    return omega, (("rayleigh", dict(alpha_R=0.02 * w1, beta_R=0.02 / w1), None), ("modal", dict(zeta=np.full(N, 0.02)), 0.02))


def _remainder(b, omega, kw, k, corrected):
    """sum_{j>=k} phi_j p_j (H_j - 1 / lambda_j) (corrected) or sum_{j>=k} phi_j p_j H_j, H_j = g - i h, in long double"""
    phi, lam = b["Phi"].T.astype(LD), b["lam"].astype(LD)
    p, _ = H.project(phi, b["F"], lam, None, LD)
    g, h = H.transfer(lam, omega, ft=LD, **kw)
    if corrected:
        g = g - (1 / lam)[None, :]
    w_re, w_im = (g * p[None, :])[:, k:], (-h * p[None, :])[:, k:]
    return w_re @ phi[k:], w_im @ phi[k:]


@pytest.mark.parametrize("name", ("cube6j", "two_mat"))
def test_modal_superposition_against_the_direct_solve(oracle, name):
    b = full_basis(name, oracle)
    omega, dampings = _cases(b)
    N = b["lam"].shape[0]
    phi = b["Phi"].T
    for label, kw, zeta in dampings:
        C = None if zeta is None else H.modal_damping_matrix(b["M"], b["lam"], b["Phi"], kw["zeta"])
        kw_k = dict(kw)
        if zeta is not None:
            kw_k["zeta"] = kw["zeta"][:K_TRUNC]
        re_f, im_f = H.modal_sum(phi, b["lam"], b["F"], omega, u_static=None, ft=LD, **kw)
        re_c, im_c = H.modal_sum(phi[:K_TRUNC], b["lam"][:K_TRUNC], b["F"], omega, u_static=b["us"], ft=LD, **kw_k)
        re_p, im_p = H.modal_sum(phi[:K_TRUNC], b["lam"][:K_TRUNC], b["F"], omega, u_static=None, ft=LD, **kw_k)
        rc_re, rc_im = _remainder(b, omega, kw, K_TRUNC, True)
        rp_re, rp_im = _remainder(b, omega, kw, K_TRUNC, False)
        for f, w in enumerate(omega):
            x = H.direct(b["Kd"], b["M"], b["F"], w, kw.get("alpha_R", 0.0), kw.get("beta_R", 0.0), C)
            scale = np.abs(x).max()
            dev = lambda re, im: float(np.abs((re[f].astype(np.float64) + 1j * im[f].astype(np.float64)) - x).max() / scale)
            Y = dev(re_f, im_f)
            corrected, plain = dev(re_c + rc_re, im_c + rc_im), dev(re_p + rp_re, im_p + rp_im)
            t_plain, t_corr = dev(re_p, im_p), dev(re_c, im_c)
            print("%s %s N = %d w = %.6e: Y %.3e, corrected + remainder %.3e, plain + remainder %.3e; truncation at k = %d: plain %.3e, "
                  "corrected %.3e" % (name, label, N, w, Y, corrected, plain, K_TRUNC, t_plain, t_corr))
            # two fp64 references (eigh's vectors, the LU of the complex matrix): far below anything a wrong formula would leave
            assert Y <= 1e-8, (label, f, Y)
            floor = 4 * max(Y, 1e-15)
            assert corrected <= floor and plain <= floor, (label, f, corrected, plain, Y)
            assert t_corr < t_plain or t_plain <= floor, (label, f, t_corr, t_plain)
        # at w = 0 the corrected sum is the static solution itself, whatever k
        assert np.abs(re_c[0] - b["us"]).max() <= 1e-15 * np.abs(b["us"]).max() and not im_c[0].any()


def test_peak_takes_the_lowest_index_on_a_tie():
    re = np.array([[1.0, 0.0], [3.0, 0.0], [3.0, 2.0], [0.0, 2.0]])
    im = np.array([[0.0, 1.0], [4.0, 0.0], [4.0, 0.0], [5.0, 0.0]])
    pk, at = H.peak(re, im)
    assert list(at) == [1, 2] and list(pk) == [5.0, 2.0]


# ---- the console's refusals: argv alone, exit code 2, nothing read --------------------------------------------------------------
P = "{path}"
HM = ["--harmonic", "10,200,20", "--modes", "6"]
REFUSALS = [
    (["--harmonic", "10,200,20", P], "--harmonic needs --modes K: the response is the superposition of the K lowest modes"),
    (HM + ["--transient", "--dt", "1e-3", "--steps", "4", P], "--harmonic, --transient, --explicit and --buckling are four analyses: one per run"),
    (HM + ["--explicit", P], "--harmonic, --transient, --explicit and --buckling are four analyses: one per run"),
    (HM + ["--buckling", "2", P], "--harmonic, --transient, --explicit and --buckling are four analyses: one per run"),
    (HM + ["--modes-shift", "1.0", P],
     "--harmonic needs a supported model: --modes-shift is for a model without supports, which has no static solution to correct with"),
    (["--modal-damping", "0.02", P], "--modal-damping Z belongs to --harmonic"),
    (["--modal-damping", "0.02", "--modes", "6", P], "--modal-damping Z belongs to --harmonic"),
    (["--harmonic", "10,200", "--modes", "6", P], "--harmonic F0,F1,NF takes three numbers: the first and the last frequency in Hz and how many"),
    (["--harmonic", "10,x,3", "--modes", "6", P], "--harmonic F0,F1,NF takes three numbers: the first and the last frequency in Hz and how many"),
    (["--harmonic", "10,200,0", "--modes", "6", P], "--harmonic F0,F1,NF needs NF >= 1, F0 >= 0 and F1 >= F0"),
    (["--harmonic", "10,200,2.5", "--modes", "6", P], "--harmonic F0,F1,NF needs NF >= 1, F0 >= 0 and F1 >= F0"),
    (["--harmonic", "-1,200,3", "--modes", "6", P], "--harmonic F0,F1,NF needs NF >= 1, F0 >= 0 and F1 >= F0"),
    (["--harmonic", "200,10,3", "--modes", "6", P], "--harmonic F0,F1,NF needs NF >= 1, F0 >= 0 and F1 >= F0"),
    (["--harmonic", "0,10,65537", "--modes", "6", P], "--harmonic F0,F1,NF takes at most 65536 frequencies"),
    (HM + ["--rayleigh", "1", P], "--rayleigh A,B takes two numbers"),
    (HM + ["--rayleigh", "-1,0", P], "--rayleigh A,B needs A >= 0 and B >= 0"),
    (HM + ["--modal-damping", "-0.1", P], "--modal-damping Z needs Z >= 0"),
    (HM + ["--vtu-every", "0", P], "--vtu-every E needs E >= 1"),
    (HM + ["--dt", "1e-3", P], "--dt, --steps, --newmark, --load-curve and --solve-eps belong to the time integrators: a frequency response has no steps"),
    (HM + ["--gpus", "2", P], "--harmonic works on one device: the modes, the static solution and the sweep over them live on a single-rank "
                              "context (drop --gpus/--devices)"),
    (HM + ["--devices", "0,0", "--vtu", "{tmp}/o", P],
     "--harmonic works on one device: the modes, the static solution and the sweep over them live on a single-rank context (drop "
     "--gpus/--devices)"),
]
OLD = "--dt, --steps, --newmark, --rayleigh, --load-curve, --probe-node, --solve-eps and --vtu-every belong to --transient"
UNTOUCHED = [["--rayleigh", "0,0", P], ["--probe-node", "3", P], ["--vtu-every", "2", P], ["--rayleigh", "1,1e-6", "--modes", "6", P]]


def _run(args, tmp):
    argv = [a.replace("{path}", os.path.join(tmp, "none.STdb")).replace("{tmp}", tmp) for a in args]
    return subprocess.run([EXE] + argv, capture_output=True, text=True, timeout=60)


def test_console_refusals_of_the_frequency_response(built_libs, tmp_path):
    """Every new refusal has its own text; --rayleigh, --probe-node and --vtu-every without --transient or --harmonic still get the
    sentence they got, byte for byte (tests/golden/console_refusals.json holds it too); --help names the option."""
    tmp = str(tmp_path)
    for args, text in REFUSALS:
        out = _run(args, tmp)
        assert out.returncode == 2 and out.stderr == "stan_solver: " + text + "\n", (args, out.returncode, out.stderr)
        assert "Reading input file" not in out.stdout and not os.listdir(tmp), args
    golden = {json.dumps(c["args"]): c["stderr"] for c in json.load(open(os.path.join(ROOT, "tests", "golden", "console_refusals.json")))}
    for args in UNTOUCHED:
        out = _run(args, tmp)
        assert out.returncode == 2 and out.stderr == "stan_solver: " + OLD + "\n", (args, out.stderr)
        assert golden.get(json.dumps(args), out.stderr) == out.stderr
    assert len({t for _, t in REFUSALS}) == 13
    out = _run(["--help"], tmp)
    assert out.returncode == 0 and "--harmonic F0,F1,NF --modes K [--mass consistent]" in out.stdout and "--modal-damping Z" in out.stdout
    # with --harmonic the three are accepted: the run gets as far as the file, which does not exist
    out = _run(HM + ["--rayleigh", "1,1e-6", "--modal-damping", "0.02", "--probe-node", "3", "--vtu-every", "2", P], tmp)
    assert out.returncode == 1 and "Reading input file" in out.stdout and "ProtoDeserialize" in out.stderr
