#!/usr/bin/env python3
"""Result scalars (stan_hip_results_scalars) timed at a cube size on results kept on the device:
the cell kernel, the node -> (element, corner) lists and the point kernel by HIP events (the library's profile fields
scalars_cell_ms / scalars_list_ms / scalars_point_ms), and the whole call by the wall clock (uploads of disp and conn,
kernels, download of the selected rows), for all 24 scalars and for von Mises alone.  Algorithmic bytes next to each.
usage: scalars_time.py [n=148] [reps=5]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
from stan_amd import hip, problem  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 148
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
job = problem.cube_job(n)
ctx = hip.Context(0)
ctx.set_profiling(True)
disp = np.random.default_rng(7).standard_normal((job.xyz.shape[0], 3)) * 1e-3
res = ctx.recover_hex8_keep(job.xyz, disp, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu)
ne, nn = job.conn.shape[0], job.xyz.shape[0]
n_inc = 8 * ne     # a cube lists no node twice in an element


def timed(sel, point, cell):
    best = None
    for _ in range(reps + 1):     # the first call pays for the allocations
        t0 = time.perf_counter()
        res.scalars(disp, job.conn, sel=sel, point=point, cell=cell)
        wall = (time.perf_counter() - t0) * 1e3
        p = ctx.profile()
        cur = dict(cell_ms=p["scalars_cell_ms"], list_ms=p["scalars_list_ms"], point_ms=p["scalars_point_ms"], call_wall_ms=wall)
        best = cur if best is None else {k: min(best[k], cur[k]) for k in cur}
    ns = len(sel)
    # cell kernel: per corner 96 B of blocks + 4 B index + 24 B displacement gather; per element ns x 3 doubles out
    best["cell_bytes"] = n_inc * (96 + 4 + 24) + ne * ns * 24
    # point kernel: per incidence 96 B of blocks + 4 B list entry; per node 16 B pointers + 24 B displacement + ns doubles out
    best["point_bytes"] = n_inc * (96 + 4) + nn * (16 + 24 + 8 * ns)
    for k in ("cell", "point"):
        if best[k + "_ms"] > 0:
            best[k + "_GBs"] = best[k + "_bytes"] / best[k + "_ms"] / 1e6
    return best


out = {"n": n, "elements": ne, "nodes": nn, "incidences": n_inc, "reps": reps,
       "all_24_point_and_cell": timed(list(range(24)), True, True),
       "all_24_point_only": timed(list(range(24)), True, False),
       "von_mises_point_and_cell": timed([13], True, True),
       "von_mises_point_only": timed([13], True, False),
       "stress_xx_point_and_cell_no_eigen_solve": timed([4], True, True)}
print(json.dumps(out))
res.free()
ctx.close()
