"""stan_solver end to end, held to a recorded transcript: for every analysis of the console driver and for the refusals that
need the file, the exit code, stderr, stdout with the times masked and the sha256 of every file the run wrote or left (the
.vtu files and the .STdb).  The models are the console tests' own, from their builders: the 4^3 cubes, and for --buckling the
2 x 2 x 10 column of test_gpu_buckling; nothing new in size.  (--buckling K --solve-eps E is accepted, so it is pinned here
and not among the refusals of tests/test_console_cli.py.)

tests/golden/console_transcripts.json was recorded on an MI355X from the driver as it stood before it was split into
functions:  python -m tests.test_gpu_console_transcript OUT.json , twice in separate processes; the two recordings agreed
byte for byte after the mask.

The mask covers the durations and what is derived from them: the number in "Done in ...s" / "... in ...s" / "Total CPU
time: ... s", and in the JSON line the keys t_* (t_s of the sub-objects among them), phases_s, spmv_ms, spmv_GBs, hbm_frac.
Everything else, the order and the format of the JSON line included, is compared as text.  STAN_HOST_THREADS is set, so
that "host_threads" does not depend on the machine."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
GOLDEN = os.path.join(ROOT, "tests", "golden", "console_transcripts.json")
WHAT = dict(body=[0.0, 0.0, -7.85e-2], p=3.5, move=[1.0e-3, 0.0, -2.0e-3])     # test_console_driver_distributed_loads' own


def _loads(path, distributed=WHAT):
    from tests.test_gpu_loads import _write_model
    _write_model(path, 4, distributed)


def _thermal(path):
    from tests.test_gpu_thermal import _write_model
    _write_model(path, 4, True)


def _modes(path, density=True):
    from tests.test_gpu_modes import _console_db
    _console_db(path, density)


def _transient(path, **kw):
    from tests.test_gpu_transient import _console_db
    _console_db(path, **kw)


def _column(path, **kw):
    from tests.test_gpu_buckling import _console_db
    _console_db(path, **kw)


def _retyped(path, atype):
    """test_gpu_transient's model (loads, supports, density) under another analysis type"""
    from stan_amd import host
    _transient(path)
    d = host.Db.read_stdb(path)
    d.set_analysis(atype=atype, tol=1e-10)
    d.write_stdb(path)


TIP = 125                                   # the last node of x = 4 in the 4^3 cube: what test_gpu_transient's builder returns
STEP = ["--transient", "--dt", "1e-4", "--steps", "2"]
RUNS = {
    # name: (builder, arguments; "{out}" is the .vtu prefix, the .STdb comes last)
    "static_loads": (_loads, ["--reactions", "--json", "--vtu", "{out}", "--vtu-cells"]),
    "static_thermal": (_thermal, ["--reactions", "--json", "--vtu", "{out}", "--vtu-cells"]),
    "static_objects": (lambda p: _loads(p, None), ["--object-results", "--json"]),
    "static_selected_scalars": (lambda p: _loads(p, None), ["--vtu", "{out}", "--vtu-results", "von Mises Stress,Displacement X", "--packed"]),
    "modes_lumped": (_modes, ["--modes", "3", "--json", "--vtu", "{out}"]),
    "modes_consistent_shifted": (lambda p: _transient(p, supports=False),
                                 ["--modes", "3", "--mass", "consistent", "--modes-shift", "1e10", "--json"]),
    "transient": (_transient, ["--transient", "--dt", "1e-4", "--steps", "4", "--probe-node", str(TIP), "--load-curve", "0,0,3e-4,1",
                               "--rayleigh", "10,1e-7", "--json", "--vtu", "{out}", "--vtu-every", "2"]),
    "buckling": (_column, ["--buckling", "2", "--solve-eps", "1e-8", "--json", "--vtu", "{out}"]),
    # the refusals that need the file, and the ends of main() behind the analyses
    "modes_without_density": (lambda p: _modes(p, False), ["--modes", "3"]),
    "transient_without_density": (lambda p: _transient(p, density=False), STEP),
    "buckling_with_temperature": (lambda p: _column(p, temperature=True), ["--buckling", "2"]),
    "buckling_without_supports": (lambda p: _column(p, supports=False), ["--buckling", "2"]),
    "transient_unknown_probe_node": (_transient, STEP + ["--probe-node", "9999"]),
    "transient_moving_support": (lambda p: _transient(p, move=[0.0, 0.01, 0.0]), STEP),
    "modes_without_supports": (lambda p: _transient(p, supports=False), ["--modes", "3"]),
    "modes_on_another_type": (lambda p: _retyped(p, "Modal"), ["--modes", "3"]),
    "transient_on_another_type": (lambda p: _retyped(p, "Modal"), STEP),
    "buckling_on_another_type": (lambda p: _retyped(p, "Modal"), ["--buckling", "2"]),
    "another_type_is_written_back": (lambda p: _retyped(p, "Modal"), ["--json"]),
    "nonlinear_statics": (lambda p: _retyped(p, "Nonlinear_Statics"), []),
}

_TIME = r"[-+0-9.eE]+"


def mask(text):
    text = re.sub(r"( in )%s(s\n)" % _TIME, r"\1<t>\2", text)
    text = re.sub(r"(Total CPU time: )%s( s\n)" % _TIME, r"\1<t>\2", text)
    text = re.sub(r'("(?:t_\w+|spmv_ms|spmv_GBs|hbm_frac)": )%s' % _TIME, r"\1<t>", text)
    return re.sub(r'("phases_s": )\{[^}]*\}', r"\1<t>", text)


def transcript(name, tmp):
    """Run `name` in the fresh directory tmp/name: {returncode, stderr, stdout, files}"""
    build, args = RUNS[name]
    where = os.path.join(tmp, name)
    os.mkdir(where)
    path = os.path.join(where, "m.STdb")
    build(path)
    argv = [a.replace("{out}", os.path.join(where, "out")) for a in args] + [path]
    out = subprocess.run([EXE] + argv, capture_output=True, text=True, timeout=120, env=dict(os.environ, STAN_HOST_THREADS="4"))
    files = {f: hashlib.sha256(open(os.path.join(where, f), "rb").read()).hexdigest() for f in sorted(os.listdir(where))}
    return dict(returncode=out.returncode, stderr=out.stderr.replace(where, "{dir}"), stdout=mask(out.stdout.replace(where, "{dir}")),
                files=files)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_mask_covers_the_durations_and_nothing_else():
    line = ('   K Matrix assembly:           Done in 0.12s\n  NORMAL  (type 1) in 3.40s\n  Total CPU time: 1.50 s\n'
            '{"n_dof": 375, "rel_residual": 1.2e-11, "t_cg_s": 0.01, "spmv_ms": 0.5, "spmv_GBs": 12.0, "hbm_frac": 0.002, "host_threads": 4, '
            '"phases_s": {"read_parse": 0.001, "write_vtu": 0.000100}, "loads": {"n_fixed": 75, "t_s": 0.004}}\n')
    assert mask(line) == ('   K Matrix assembly:           Done in <t>s\n  NORMAL  (type 1) in <t>s\n  Total CPU time: <t> s\n'
                          '{"n_dof": 375, "rel_residual": 1.2e-11, "t_cg_s": <t>, "spmv_ms": <t>, "spmv_GBs": <t>, "hbm_frac": <t>, '
                          '"host_threads": 4, "phases_s": <t>, "loads": {"n_fixed": 75, "t_s": <t>}}\n')


def test_the_fixture_holds_every_run(golden):
    assert sorted(golden) == sorted(RUNS)


@pytest.mark.parametrize("name", list(RUNS))
def test_console_transcript(name, golden, built_libs, tmp_path):
    got, want = transcript(name, str(tmp_path)), golden[name]
    assert got["returncode"] == want["returncode"], got
    assert got["stderr"] == want["stderr"]
    assert got["stdout"] == want["stdout"]
    assert got["files"] == want["files"]


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rec = {name: transcript(name, tmp) for name in RUNS}
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, r in rec.items():
        print("%-32s exit %d, %d files" % (name, r["returncode"], len(r["files"])))
