"""The number format of the lossless 60-bit value stream (stan_amd/csrc/s60.h) checked on the host: a stand-alone program
(tests/stream60_host/roundtrip.cpp, its own main) built with AddressSanitizer and UBSan and run on the CPU.  Nothing of it
is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encode_decode_roundtrip_under_sanitizers(tmp_path):
    exe = str(tmp_path / "s60_roundtrip")
    src = os.path.join(ROOT, "tests", "stream60_host", "roundtrip.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
