"""stan_solver's argument checks, pinned text for text: every refusal that main() reaches from argv alone (exit code 2, before
the banner, before the file is opened and before a device is touched) with its exact stderr, the order in which two faults at
once are answered, and the parser's quirks (an option that wants a value but stands last is taken as the path;
--buckling-tol without --buckling is refused by --buckling's own check).

tests/golden/console_refusals.json is a list of {args, returncode, stderr}; in args "{path}" stands for a .STdb that does not
exist and "{tmp}" for the test's empty directory.  It was recorded from the driver as it stood before it was split into
functions:  python -m tests.test_console_cli --record  (the cases are ARGS below; the recorder refuses a case that gets as
far as reading the file)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "stan_amd", "bin", "stan_solver")
GOLDEN = os.path.join(ROOT, "tests", "golden", "console_refusals.json")

P, V = "{path}", "{tmp}/o"
OK = ["--transient", "--dt", "1e-3", "--steps", "4"]
ARGS = [
    # usage: no path at all
    [], ["--json"], ["--modes", "-1"],
    # --vtu / --vtu-results / --reactions
    ["--vtu", V, "--gpus", "2", P], ["--vtu", V, "--devices", "0,1", P],
    ["--vtu", V, "--vtu-results", "Bogus", P], ["--vtu", V, "--vtu-results", "von Mises Stress,von Mises Stress", P],
    ["--vtu", V, "--vtu-results", "von Mises Stress,,Displacement X", P],
    ["--reactions", "--devices", "0,0", P],
    # --modes, --modes-shift, --mass
    ["--modes", "-1", P], ["--modes", "2", "--modes-tol", "-1", P], ["--modes-tol", "1e-3", P],
    ["--modes", "2", "--gpus", "2", P],
    ["--modes-shift", "1.0", P], ["--modes", "3", "--modes-shift", "-1", P], ["--modes", "3", "--modes-shift", "inf", P],
    ["--modes", "3", "--mass", "hrz", P], ["--mass", "hrz", P], ["--mass", "consistent", P],
    # --buckling: its four reasons
    ["--buckling", "0", P], ["--buckling", "2", "--buckling-tol", "-1", P], ["--buckling", "2", "--buckling-tol", "nan", P],
    ["--buckling", "2", "--modes", "2", P], ["--buckling", "2"] + OK + [P],
    ["--buckling", "2", "--solve-eps", "-1", P], ["--buckling", "2", "--solve-eps", "nan", P],
    ["--buckling", "2", "--gpus", "2", P],
    # ... belong to --transient
    ["--dt", "1e-3", P], ["--steps", "4", P], ["--newmark", "0.25,0.5", P], ["--rayleigh", "0,0", P], ["--load-curve", "0,1", P],
    ["--probe-node", "3", P], ["--vtu-every", "2", P], ["--solve-eps", "1e-8", P],
    ["--buckling", "2", "--solve-eps", "1e-8", "--dt", "1e-3", P], ["--buckling", "0", "--solve-eps", "1e-8", P],
    # --transient: its ten reasons
    OK + ["--modes", "3", P],
    OK + ["--newmark", "0.25", P], OK + ["--rayleigh", "1,x", P], OK + ["--load-curve", "0,1,2", P], OK + ["--load-curve", "", P],
    ["--transient", "--steps", "4", P], ["--transient", "--dt", "0", "--steps", "4", P], ["--transient", "--dt", "-1", "--steps", "4", P],
    ["--transient", "--dt", "inf", "--steps", "4", P],
    ["--transient", "--dt", "1e-3", "--steps", "-1", P],
    OK + ["--solve-eps", "-1", P],
    OK + ["--vtu", V, "--vtu-every", "0", P], OK + ["--vtu-every", "0", P],
    OK + ["--rayleigh", "-1,0", P], OK + ["--rayleigh", "0,-1", P],
    OK + ["--newmark", "0.2,0.5", P], OK + ["--newmark", "0.25,0.4", P],
    OK + ["--load-curve", "0,1,2,1,1,0", P], OK + ["--load-curve", "0,nan", P],
    OK + ["--devices", "0,0", P],
    # two faults at once: the first one tested is the one named
    OK + ["--modes", "3", "--devices", "0,0", P],
    ["--buckling", "0", "--modes", "2", P],
    ["--vtu", V, "--gpus", "2", "--vtu-results", "Bogus", P],
    ["--vtu", V, "--vtu-results", "Bogus", "--reactions", "--gpus", "2", P],
    ["--reactions", "--gpus", "2", "--modes", "-1", P],
    ["--modes", "-1", "--mass", "hrz", P],
    ["--modes", "2", "--gpus", "2", "--modes-shift", "-1", P],
    ["--modes-shift", "1", "--mass", "hrz", P],
    ["--mass", "consistent", "--buckling", "0", P],
    ["--buckling", "2", "--modes", "2", "--solve-eps", "-1", P],
    ["--buckling", "2", "--solve-eps", "-1", "--gpus", "2", P],
    ["--buckling", "2", "--gpus", "2", "--dt", "1e-3", P],
    ["--dt", "1e-3", "--modes", "-1", P],
    OK + ["--modes", "3", "--newmark", "0.25", P],
    ["--transient", "--steps", "4", "--newmark", "0.25", P],
    ["--transient", "--dt", "0", "--steps", "-1", P],
    ["--transient", "--dt", "1e-3", "--steps", "-1", "--solve-eps", "-1", P],
    OK + ["--solve-eps", "-1", "--vtu-every", "0", P],
    OK + ["--vtu", V, "--vtu-every", "0", "--rayleigh", "-1,0", P],
    OK + ["--rayleigh", "-1,0", "--newmark", "0.2,0.5", P],
    OK + ["--newmark", "0.2,0.5", "--load-curve", "0,nan", P],
    OK + ["--load-curve", "0,nan", "--gpus", "2", P],
    # the parser: an option that wants a value but stands last is the path (so this is not the usage line) ...
    ["--steps", "4", "--dt"], [P, "--buckling", "0", "--modes"], ["--reactions", "--gpus", "2", "--vtu"],
    # ... and --buckling-tol alone is answered by --buckling's own check
    ["--buckling-tol", "1e-3", P],
]


def _run(args, tmp):
    argv = [a.replace("{path}", os.path.join(tmp, "none.STdb")).replace("{tmp}", tmp) for a in args]
    return subprocess.run([EXE] + argv, capture_output=True, text=True, timeout=60)


def test_console_refusals_are_the_recorded_ones(built_libs, tmp_path):
    cases = json.load(open(GOLDEN))
    assert [c["args"] for c in cases] == ARGS
    for c in cases:
        out = _run(c["args"], str(tmp_path))
        assert out.returncode == c["returncode"] == 2, (c["args"], out.returncode, out.stderr)
        assert out.stderr == c["stderr"], (c["args"], out.stderr, c["stderr"])
        assert "Reading input file" not in out.stdout, c["args"]
        assert not os.listdir(str(tmp_path)), c["args"]


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_console_cli --record"
    rec = []
    with tempfile.TemporaryDirectory() as tmp:
        for args in ARGS:
            out = _run(args, tmp)
            assert out.returncode == 2 and "Reading input file" not in out.stdout and not os.listdir(tmp), (args, out)
            rec.append(dict(args=args, returncode=out.returncode, stderr=out.stderr))
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%d cases -> %s" % (len(rec), GOLDEN))
