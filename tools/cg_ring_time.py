"""The ring of search directions (STAN_OPT_CG_X_RING) and the refresh passes on the 60-bit stream (STAN_OPT_CG_REFRESH_60),
each by itself and both together: one process, one resident K, solves that alternate over the four settings of the two
options.  Bench mode (merit stop off, eps 1e-8), the cube of BASELINE.json.  Per solve, from the library's profile (events on
the solve's stream): the whole solve, the time outside the products per iteration ((cg_ms - spmv_ms_total - spmv2_ms_total)
/ iterations: k_step, k_update, the flushes, the reductions), the plain product and the two-product pass per launch.
bench.py cannot select the options; this gives each part's own figures.
usage: cg_ring_time.py SIZE [REPS=3]"""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stan_amd import hip, problem

n = int(sys.argv[1])
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
EPS = 1e-8
FORMS = [(0, 0), (1, 0), (0, 1), (1, 1)]   # (x_ring, refresh_60)
ctx = hip.Context(0)
ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
ctx.set_option(hip.OPT_CG_MERIT_STOP, 0)
ctx.set_profiling(True)
job = problem.cube_job(n)
K = ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
d_F = torch.from_numpy(job.F).cuda()
d_U = {f: torch.zeros_like(d_F) for f in FORMS}


def solve(form):
    ctx.set_option(hip.OPT_CG_X_RING, form[0])
    ctx.set_option(hip.OPT_CG_REFRESH_60, form[1])
    rep = K.cg_solve_dev(d_F.data_ptr(), d_U[form].data_ptr(), EPS)
    p = ctx.profile()
    w, flushes, rstream = ctx.cg_loop_info()
    its = max(rep["iterations"], 1)
    return dict(window=w, flushes=flushes, refresh_stream=rstream, iterations=rep["iterations"], type=rep["terminationtype"],
                rel=rep["rel_residual"], cg_ms=p["cg_ms"],
                other_us_per_it=1e3 * (p["cg_ms"] - p["spmv_ms_total"] - p["spmv2_ms_total"]) / its,
                spmv_ms=p["spmv_ms_total"] / max(p["spmv_launches"], 1), spmv2_ms=p["spmv2_ms_total"] / max(p["spmv2_launches"], 1),
                spmv2_launches=p["spmv2_launches"], value_stream=p["value_stream"])


for form in FORMS:   # warm-up of each: the matrix scaled, its streams built, the ring's block in the pool
    solve(form)
rows = {f: [] for f in FORMS}
for _ in range(reps):
    for form in FORMS:
        rows[form].append(solve(form))
print("cube %d^3, %d DOF, eps %g, merit stop off, %d alternating repetitions" % (n, job.n_dof, EPS, reps))
for form in FORMS:
    for r in rows[form]:
        print("x_ring %d refresh_60 %d  W %2d flushes %4d  its %d type %d rel %s  cg %.2f ms  outside products %.2f us/it  product %.4f ms (stream %d)  two-product %.4f ms x %d (stream %d)"
              % (form + (r["window"], r["flushes"], r["iterations"], r["type"], float(r["rel"]).hex(), r["cg_ms"], r["other_us_per_it"],
                         r["spmv_ms"], r["value_stream"], r["spmv2_ms"], r["spmv2_launches"], r["refresh_stream"])))
for key, unit in (("cg_ms", "ms"), ("other_us_per_it", "us/it"), ("spmv_ms", "ms"), ("spmv2_ms", "ms")):
    base = [r[key] for r in rows[FORMS[0]]]
    for form in FORMS:
        m = [r[key] for r in rows[form]]
        print("%-16s x_ring %d refresh_60 %d: median %.4f spread %.4f   against 0 0: %+.4f %s"
              % ((key,) + form + (statistics.median(m), max(m) - min(m), statistics.median(m) - statistics.median(base), unit)))
ref = rows[FORMS[0]][-1]
same = all(torch.equal(d_U[f], d_U[FORMS[0]]) and rows[f][-1]["iterations"] == ref["iterations"] and rows[f][-1]["rel"] == ref["rel"]
           for f in FORMS)
print("U, iterations and residual of the four forms equal bit for bit:", same)
K.free()
ctx.close()
sys.exit(0 if same else 1)
