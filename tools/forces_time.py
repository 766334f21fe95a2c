#!/usr/bin/env python3
"""Internal forces (stan_hip_internal_forces_hex8_dev) timed at a cube size with the inputs resident
in HBM: the element pass, the node -> (element, corner) lists and the node gather with its reductions by HIP events (the
library's profile fields forces_elem_ms / forces_list_ms / forces_gather_ms), the whole call by the wall clock; in the same
process k_recover (stan_hip_recover_hex8_dev, as tools/recover_time.py runs it) as the yardstick: the element pass reads
what k_recover reads (224 B per element) and writes 192 B per element where k_recover writes 768 B.  The library records
no events round k_recover, so its time is the wall clock of the synchronising call; the same call on ONE element, timed
the same way, measures what that adds to the kernel (launch, synchronisation, the binding), and the ratio of the element
pass to k_recover is printed both ways: against the raw wall time, which favours the element pass, and with the
one-element call subtracted.
usage: forces_time.py [n=148] [reps=5]"""
import ctypes as C
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
disp = np.random.default_rng(7).standard_normal((job.xyz.shape[0], 3)) * 1e-3
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_xyz, d_disp, d_dof, d_conn = up(job.xyz), up(disp), up(job.node_dof), up(job.conn)
d_mat, d_typ, d_red, d_F = up(job.elem_mat), up(job.elem_type), up(job.red), up(job.F)
ne, nn = job.conn.shape[0], job.xyz.shape[0]
d_fint = torch.empty(job.n_dof, dtype=torch.float64, device=dev)
d_reac = torch.empty(job.n_dof, dtype=torch.float64, device=dev)
d_e = torch.empty(ne * 48, dtype=torch.float64, device=dev)
d_s = torch.empty(ne * 48, dtype=torch.float64, device=dev)
E = np.ascontiguousarray(job.mat_E_nu, dtype=np.float64).reshape(-1, 2)
torch.cuda.synchronize()


def forces():
    return ctx.internal_forces_hex8_dev(nn, d_xyz.data_ptr(), d_disp.data_ptr(), d_dof.data_ptr(), ne, d_conn.data_ptr(),
                                        d_mat.data_ptr(), d_typ.data_ptr(), E, job.n_dof, d_red.data_ptr(), d_F.data_ptr(),
                                        d_fint.data_ptr(), d_reac.data_ptr())


def recover(n_el=ne):
    ctx._chk(ctx.lib.stan_hip_recover_hex8_dev(
        ctx.h, C.c_int64(nn), hip._dev(d_xyz.data_ptr(), C.c_double), hip._dev(d_disp.data_ptr(), C.c_double),
        C.c_int64(n_el), hip._dev(d_conn.data_ptr(), C.c_int32), hip._dev(d_mat.data_ptr(), C.c_int32),
        hip._dev(d_typ.data_ptr(), C.c_uint8), C.c_int32(E.shape[0]), hip._ptr(E, C.c_double),
        hip._dev(d_e.data_ptr(), C.c_double), hip._dev(d_s.data_ptr(), C.c_double)))


best = None
for _ in range(reps + 1):     # the first call pays for the allocations
    t0 = time.perf_counter()
    eq = forces()
    wall = (time.perf_counter() - t0) * 1e3
    p = ctx.profile()
    cur = dict(elem_ms=p["forces_elem_ms"], list_ms=p["forces_list_ms"], gather_ms=p["forces_gather_ms"], call_wall_ms=wall)
    best = cur if best is None else {k: min(best[k], cur[k]) for k in cur}


def wall_ms(fn):
    fn()
    t = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        t = ms if t is None else min(t, ms)
    return t


t_rec = wall_ms(recover)
t_one = wall_ms(lambda: recover(1))     # one element: the call without the kernel's work
n_inc = 8 * ne
best["elem_bytes"] = ne * (224 + 192)                    # 8 indices + its share of coordinates and displacements; 24 doubles out
best["gather_bytes"] = n_inc * (24 + 4) + nn * (16 + 12 + 12 + 24 + 48)      # f_e + list; pointers, DOFs, red, F, f_int + reaction
best["elem_GBs"] = best["elem_bytes"] / best["elem_ms"] / 1e6
best["gather_GBs"] = best["gather_bytes"] / best["gather_ms"] / 1e6
print(json.dumps({"n": n, "elements": ne, "nodes": nn, "incidences": n_inc, "reps": reps, "internal_forces": best,
                  "k_recover_call_wall_ms": t_rec, "k_recover_one_element_call_wall_ms": t_one, "k_recover_bytes": ne * (768 + 224),
                  "elem_pass_events_over_k_recover_wall": best["elem_ms"] / t_rec,
                  "elem_pass_events_over_k_recover_wall_less_one_element_call": best["elem_ms"] / (t_rec - t_one),
                  "equilibrium": eq.as_dict()}))
ctx.close()
