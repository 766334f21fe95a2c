"""A multi-device handle names a failing element by its number in the WHOLE model.  Stress recovery cuts the elements into
one contiguous chunk per rank and a rank of a sharded assembly holds a picked subset, so what a rank's device reports is an
index into its own arrays; the host side turns it back (last_bad_element, the error text).  Two ranks on GPU 0 over the RCCL
stand-in, 4^3 = 64 elements: the second rank's chunk is elements 32..63."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import fake_rccl_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")

CHILD = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch
from stan_amd import hip, problem
job = problem.cube_job(4)
assert job.conn.shape[0] == 64
disp = 1e-3 * job.xyz
group, one = hip.Context(devices=[0, 0]), hip.Context(0)
out = {}

def failure(ctx, call):
    try:
        r = call(ctx)
    except hip.StanHipError as e:
        return [e.code, ctx.last_bad_element(), str(e)]
    if hasattr(r, "free"):
        r.free()
    return None

def sound_mesh_still_works():
    eps, sig = one.recover_hex8(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
    K = one.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    K.free()
    return bool(np.isfinite(eps).all() and np.isfinite(sig).all() and np.abs(sig).max() > 0)

# element 40 is HEX8_G1: stress recovery refuses it (the reference throws)
etype = np.array(job.elem_type, dtype=np.uint8).copy()
etype[40] = 1
for name in ("recover_hex8", "recover_hex8_keep"):
    out["g1_" + name] = failure(group, lambda c: getattr(c, name)(job.xyz, disp, job.conn, job.elem_mat, etype, job.mat_E_nu))
out["g1_then_sound"] = sound_mesh_still_works()

# element 50 flattened: det J == 0 there; the device reports the lowest failing index, whichever that is
xyz = job.xyz.copy()
xyz[job.conn[50]] = xyz[job.conn[50]] * [1, 1, 0]
calls = {
    "recover_hex8": lambda c: c.recover_hex8(xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu),
    "recover_hex8_keep": lambda c: c.recover_hex8_keep(xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu),
    "assemble_hex8": lambda c: c.assemble_hex8(xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red),
}
for name, call in calls.items():
    out["detj_" + name] = {"group": failure(group, call), "one": failure(one, call)}
out["detj_then_sound"] = sound_mesh_still_works()
out["codes"] = {"E_UNSUPPORTED": hip.E_UNSUPPORTED, "E_DETJ": hip.E_DETJ}
group.close(); one.close()
print("RESULT " + json.dumps(out))
''' % ROOT


def test_a_group_handle_reports_whole_model_element_numbers(built_libs):
    env = dict(os.environ, STAN_RCCL_LIB=FAKE, **fake_rccl_env("sync", 2))
    p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=180, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    print(json.dumps(out, indent=1))
    codes = out["codes"]
    for name in ("recover_hex8", "recover_hex8_keep"):
        got = out["g1_" + name]
        assert got is not None, name
        code, bad, text = got
        assert code == codes["E_UNSUPPORTED"] and bad == 40 and "element 40" in text, (name, got)
    assert out["g1_then_sound"] is True
    for name in ("recover_hex8", "recover_hex8_keep", "assemble_hex8"):
        group, one = out["detj_" + name]["group"], out["detj_" + name]["one"]
        assert group is not None and one is not None, name
        assert group[0] == one[0] == codes["E_DETJ"], (name, group, one)
        assert one[1] >= 32, (name, one)   # the case is about the SECOND chunk
        assert group[1] == one[1], (name, group, one)
    assert out["detj_then_sound"] is True
