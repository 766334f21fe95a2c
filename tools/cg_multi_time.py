"""M load cases on one K: M calls of cg_solve_dev against one cg_solve_multi_dev (one pass over K per iteration for all
columns).  Bench mode (merit stop off, eps 1e-8), the cube of BASELINE.json, M seeded load vectors: column 0 is the
job's own F, the others standard normal vectors of its norm.  The two forms alternate after a warm-up of each; the clock
is the host's, around work that ends in a device synchronise.  The yardstick is the sequential time of the same run.
usage: cg_multi_time.py SIZE M [REPS=2]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stan_amd import hip, problem

n, M = int(sys.argv[1]), int(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
EPS = 1e-8
ctx = hip.Context(0)
ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
job = problem.cube_job(n)
K = ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
N = job.F.shape[0]
rng = np.random.default_rng(11)
F = np.empty((M, N))
F[0] = job.F
for j in range(1, M):
    g = rng.standard_normal(N)
    F[j] = g * (np.linalg.norm(job.F) / np.linalg.norm(g))
d_F = torch.from_numpy(F).cuda()
d_Us = torch.zeros_like(d_F)
d_Um = torch.zeros_like(d_F)


def sequential():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = [K.cg_solve_dev(d_F[j].data_ptr(), d_Us[j].data_ptr(), EPS) for j in range(M)]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def batched():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = K.cg_solve_multi_dev(d_F.data_ptr(), d_Um.data_ptr(), M, EPS)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


sequential()
batched()
ts, tb = [], []
for _ in range(reps):
    t, rs = sequential()
    ts.append(t)
    t, rb = batched()
    tb.append(t)
Us, Um = d_Us.cpu().numpy(), d_Um.cpu().numpy()
print("cube %d^3, %d DOF, M = %d load cases, eps %g, merit stop off, %d alternating repetitions" % (n, job.n_dof, M, EPS, reps))
print("iterations  sequential:", [r["iterations"] for r in rs], " types", [r["terminationtype"] for r in rs])
print("iterations  batched   :", [r["iterations"] for r in rb], " types", [r["terminationtype"] for r in rb])
print("sequential (M x cg_solve_dev)   : best %.3f s   all %s" % (min(ts), " ".join("%.3f" % t for t in ts)))
print("batched (1 x cg_solve_multi_dev): best %.3f s   all %s" % (min(tb), " ".join("%.3f" % t for t in tb)))
print("ratio sequential / batched: %.2f" % (min(ts) / min(tb)))
print("max|dU| / max|U| between the two answers, per column:",
      " ".join("%.2e" % (np.abs(Us[j] - Um[j]).max() / np.abs(Us[j]).max()) for j in range(M)))
K.free()
ctx.close()
