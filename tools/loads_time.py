#!/usr/bin/env python3
"""The load vector (stan_hip_load_vector_hex8_dev) timed at a cube size with the inputs resident in
HBM: the element pass, the node -> (element, corner) lists and the node gather with its reductions by HIP events (the
library's stan_hip_load_vector_times), the whole call by the wall clock.
Load case: gravity on every element, a pressure on the face x = n, and the face x = 0 moved by a given vector.  The call is
timed twice: with body force and pressure only, and with the prescribed displacement as well, which adds one pass of the
internal forces (its phases are reported from forces_*_ms).  The yardstick of the element pass is k_if_elem on the same cube:
run tools/forces_time.py in the same session (profiles/r08/loads_n148.md).
usage: loads_time.py [n=148] [reps=5]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from stan_amd import hip, problem  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 148
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
job = problem.cube_job(n)
dev = torch.device("cuda", 0)
ctx = hip.Context(0)
ctx.set_profiling(True)
ne, nn = job.conn.shape[0], job.xyz.shape[0]
e = np.arange(ne)
face_elem = e[e % n == n - 1].astype(np.int32)                # the elements behind the face x = n: face 1 (xi = +1)
face_id = np.full(face_elem.size, 1, dtype=np.uint8)
face_p = np.full(face_elem.size, 2.5)
body = np.array([[0.0, 0.0, -7.85e-5 * 9.81]])
u0 = np.zeros((nn, 3))
u0[job.xyz[:, 0] == 0.0] = [1.0e-3, 0.0, -2.0e-3]
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_xyz, d_dof, d_conn = up(job.xyz), up(job.node_dof), up(job.conn)
d_mat, d_typ, d_red = up(job.elem_mat), up(job.elem_type), up(job.red)
d_fe, d_fi, d_fp, d_u0 = up(face_elem), up(face_id), up(face_p), up(u0)
d_F = torch.zeros(job.n_red, dtype=torch.float64, device=dev)
d_Fs = torch.empty(job.n_red, dtype=torch.float64, device=dev)
d_l = torch.empty(job.n_dof, dtype=torch.float64, device=dev)
E = np.ascontiguousarray(job.mat_E_nu, dtype=np.float64).reshape(-1, 2)
torch.cuda.synchronize()


def call(with_u0):
    d_F.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = ctx.load_vector_hex8_dev(nn, d_xyz.data_ptr(), d_dof.data_ptr(), ne, d_conn.data_ptr(), d_mat.data_ptr(), d_typ.data_ptr(), E,
                                 job.n_dof, d_red.data_ptr(), body, face_elem.size, d_fe.data_ptr(), d_fi.data_ptr(), d_fp.data_ptr(),
                                 d_u0.data_ptr() if with_u0 else None, d_F.data_ptr(), d_Fs.data_ptr(), d_l.data_ptr())
    return q, (time.perf_counter() - t0) * 1e3


out = {}
for with_u0 in (False, True):
    best = None
    for _ in range(reps + 1):     # the first call pays for the allocations
        q, wall = call(with_u0)
        p, t = ctx.profile(), ctx.load_vector_times()
        cur = dict(elem_ms=t["loads_elem_ms"], list_ms=t["loads_list_ms"], gather_ms=t["loads_gather_ms"], call_wall_ms=wall)
        if with_u0:
            cur.update(forces_elem_ms=p["forces_elem_ms"], forces_list_ms=p["forces_list_ms"], forces_gather_ms=p["forces_gather_ms"])
        best = cur if best is None else {k: min(best[k], cur[k]) for k in cur}
    out["with_prescribed_displacement" if with_u0 else "body_and_pressure"] = best
b = out["body_and_pressure"]
b["elem_bytes"] = ne * (32 + 4 + 24 + 192)      # 8 indices, the material, its share of the coordinates (24 B); 24 doubles out
b["elem_GBs"] = b["elem_bytes"] / b["elem_ms"] / 1e6
print(json.dumps({"n": n, "elements": ne, "nodes": nn, "faces": int(face_elem.size), "reps": reps, "loads": out, "sums": q.as_dict()}))
ctx.close()
