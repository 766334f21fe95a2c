"""The slot and window arithmetic of the ring of search directions (stan_amd/csrc/x_ring.h, STAN_OPT_CG_X_RING) checked
on the host: a stand-alone program (tests/x_ring_host/model.cpp, its own main) built with AddressSanitizer and UBSan and run
on the CPU.  It runs a scalar model of the loop with and without the ring for every stop iteration 1 ... 3W + 2, every window
W = 2 ... 16 (and the periods that fall back to W = 10), both kinds of stop, and compares the iterates bit for bit.  Nothing of
it is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_model_matches_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "x_ring_model")
    src = os.path.join(ROOT, "tests", "x_ring_host", "model.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-ffp-contract=off", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
