#!/usr/bin/env python3
"""The thermal load (stan_hip_thermal_load_hex8_dev) timed at a cube size with the inputs resident in
HBM: the element pass k_th_elem, the node -> (element, corner) lists and the node gather with its reductions by HIP events
(stan_hip_thermal_load_times), the whole call by the wall clock.  alpha != 0 on every element, a random dT.
In the same session, as yardsticks of the element pass: k_ld_elem (gravity on every element, stan_hip_load_vector_times) and
k_if_elem (a random displacement field, the forces_* fields of the profile).
The stress pass k_th_stress (stan_hip_thermal_stress_hex8_dev) reads and writes the [n_elem][8][6] array once: its call by the
wall clock against a kernel that only WRITES that array (torch's fill, HIP events; the yardstick of tools/recover_time.py).
The kernel alone: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/thermal_time.py`, in a run of its own.
usage: thermal_time.py [n=148] [reps=5]      (profiles/r09/thermal_n148.md)"""
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
rng = np.random.default_rng(9)
alpha = np.full(job.mat_E_nu.reshape(-1, 2).shape[0], 1.2e-5)
dT = rng.uniform(-50.0, 150.0, nn)
disp = rng.standard_normal((nn, 3)) * 1e-3
body = np.array([[0.0, 0.0, -7.85e-5 * 9.81]])
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_xyz, d_dof, d_conn = up(job.xyz), up(job.node_dof), up(job.conn)
d_mat, d_typ, d_red = up(job.elem_mat), up(job.elem_type), up(job.red)
d_dT, d_disp = up(dT), up(disp)
d_F = torch.zeros(job.n_red, dtype=torch.float64, device=dev)
d_l = torch.empty(job.n_dof, dtype=torch.float64, device=dev)
d_s = torch.zeros(ne * 48, dtype=torch.float64, device=dev)
E = np.ascontiguousarray(job.mat_E_nu, dtype=np.float64).reshape(-1, 2)
mesh = (nn, d_xyz.data_ptr(), d_dof.data_ptr(), ne, d_conn.data_ptr(), d_mat.data_ptr(), d_typ.data_ptr(), E, job.n_dof, d_red.data_ptr())
torch.cuda.synchronize()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = fn()
    return q, (time.perf_counter() - t0) * 1e3     # (every entry returns complete)


def best_of(fn):
    best = None
    for _ in range(reps + 1):     # the first call pays for the allocations
        cur = fn()
        best = cur if best is None else {k: min(best[k], cur[k]) for k in cur}
    return best


def thermal():
    d_F.zero_()
    q, ms = wall(lambda: ctx.thermal_load_hex8_dev(*mesh, alpha, d_dT.data_ptr(), d_F.data_ptr(), d_l.data_ptr()))
    t = ctx.thermal_load_times()
    thermal.sums = q
    return dict(elem_ms=t["thermal_elem_ms"], list_ms=t["thermal_list_ms"], gather_ms=t["thermal_gather_ms"], call_wall_ms=ms)


def gravity():
    d_F.zero_()
    _, ms = wall(lambda: ctx.load_vector_hex8_dev(*mesh, body, d_F=d_F.data_ptr(), d_load_full=d_l.data_ptr()))
    t = ctx.load_vector_times()
    return dict(elem_ms=t["loads_elem_ms"], list_ms=t["loads_list_ms"], gather_ms=t["loads_gather_ms"], call_wall_ms=ms)


def forces():
    _, ms = wall(lambda: ctx.internal_forces_hex8_dev(nn, d_xyz.data_ptr(), d_disp.data_ptr(), d_dof.data_ptr(), ne, d_conn.data_ptr(),
                                                      d_mat.data_ptr(), d_typ.data_ptr(), E, job.n_dof, d_red.data_ptr(),
                                                      d_f_int=d_l.data_ptr(), eq=False))
    p = ctx.profile()
    return dict(elem_ms=p["forces_elem_ms"], list_ms=p["forces_list_ms"], gather_ms=p["forces_gather_ms"], call_wall_ms=ms)


def stress():
    _, ms = wall(lambda: ctx.thermal_stress_hex8_dev(nn, d_dT.data_ptr(), ne, d_conn.data_ptr(), d_mat.data_ptr(), d_typ.data_ptr(), E,
                                                     alpha, d_s.data_ptr()))
    return dict(call_wall_ms=ms)


out = dict(thermal_load=best_of(thermal), gravity_load_k_ld_elem=best_of(gravity), internal_forces_k_if_elem=best_of(forces),
           thermal_stress=best_of(stress))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
d_s.zero_(); torch.cuda.synchronize()
e0.record()
for _ in range(reps):
    d_s.zero_()
e1.record(); torch.cuda.synchronize()
fill_ms = e0.elapsed_time(e1) / reps
s = out["thermal_stress"]
s["bytes_read_and_written"] = ne * 48 * 8 * 2
s["GBs_wall"] = s["bytes_read_and_written"] / (s["call_wall_ms"] * 1e-3) / 1e9
s["write_only_fill_ms"] = fill_ms
s["wall_over_write_only_fill"] = s["call_wall_ms"] / fill_ms
t = out["thermal_load"]
t["elem_bytes"] = ne * (32 + 4 + 1 + 24 + 8 + 192)   # 8 indices, material, type, its share of the coordinates and of dT; 24 doubles out
t["elem_GBs"] = t["elem_bytes"] / t["elem_ms"] / 1e6
print(json.dumps({"n": n, "elements": ne, "nodes": nn, "reps": reps, "times": out, "sums": thermal.sums.as_dict()}))
ctx.close()
