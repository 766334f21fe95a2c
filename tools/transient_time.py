#!/usr/bin/env python3
"""Phases of stan_hip_transient at size: the n^3 cube of bench.py (clamped on x) under its own load as a step load, from rest.

    python tools/transient_time.py N STEPS [--dt-over-T1 R ...] [--t1 T1] [--solve-eps E] [--rho R]

T1 is not known at size: it comes from stan_hip_modes with one mode (solve_eps 1e-3, which the outer iteration does not need
tighter: profiles/modes_n148.md), unless --t1 gives it.  One run of STEPS steps per R (default 1/20, 1/200, 1/2000), no damping.
Prints one JSON line: the sizes, T1, the run's own stream rate (stan_hip_stream_bench: what this device gives a read-only sweep
of K's values), and per run sigma, the CG iterations per step (min / mean / max), seconds per step, and the shift pass and the
two step kernels next to their algorithmic bytes over that stream rate:
    shift    K's values read once and written once, the columns read once: n_slots 64 (2 x 72 + 4) bytes
    predict  u, v, a, F, M read, b written: 48 N bytes (no damping: the form without Kw)
    correct  u', u, v, a read, u, v, a written: 56 N bytes"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("steps", type=int)
    ap.add_argument("--dt-over-T1", type=float, nargs="*", default=[1 / 20, 1 / 200, 1 / 2000])
    ap.add_argument("--t1", type=float, default=0.0)
    ap.add_argument("--solve-eps", type=float, default=0.0)
    ap.add_argument("--rho", type=float, default=7.85e-9)
    a = ap.parse_args()
    import torch  # noqa: F401  first: one shared HIP runtime
    from stan_amd import hip, problem
    j = problem.cube_job(a.n)
    ctx = hip.Context(0)
    ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
    ctx.set_profiling(True)
    K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    M, _, sums = ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, [a.rho], mass_node=False)
    info = K.info()
    N = M.shape[0]
    out = dict(n=a.n, N=N, steps=a.steps, solve_eps=a.solve_eps or 1e-6, total_mass=sums.total_mass, n_slots=info["n_slots"])
    T1 = a.t1
    if not T1 > 0:
        t0 = time.perf_counter()
        lam, _, _, mrep = K.modes(M, 1, solve_eps=1e-3)
        T1 = float(2 * np.pi / np.sqrt(lam[0]))
        out.update(modes_wall_s=round(time.perf_counter() - t0, 3), modes_outer=mrep["outer"], modes_cg_iterations=mrep["cg_iterations"])
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    shift_bytes = info["n_slots"] * 64 * (2 * 72 + 4)
    predict_bytes, correct_bytes = 48 * N, 56 * N
    out.update(T1=T1, stream_GBs=round(stream, 1), shift_bytes=shift_bytes, shift_ms_at_stream=shift_bytes / stream / 1e6,
               predict_bytes=predict_bytes, predict_ms_at_stream=predict_bytes / stream / 1e6, correct_bytes=correct_bytes,
               correct_ms_at_stream=correct_bytes / stream / 1e6, runs=[])
    F = np.asarray(j.F, dtype=np.float64)
    for r in a.dt_over_T1:
        t0 = time.perf_counter()
        res = K.transient(M, F, r * T1, a.steps, solve_eps=a.solve_eps)
        wall = time.perf_counter() - t0
        rep = res["report"]
        n = max(rep["steps"], 1)
        out["runs"].append(dict(dt_over_T1=r, dt=r * T1, sigma=rep["sigma"], cg_min=rep["cg_min_iterations"], cg_mean=rep["cg_iterations"] / n,
                                cg_max=rep["cg_max_iterations"], cg_worst_type=rep["cg_worst_type"], wall_s=round(wall, 3),
                                s_per_step=(rep["solve_ms"] + rep["product_ms"] + rep["step_ms"]) / n / 1e3, shift_ms=rep["shift_ms"],
                                solve_ms_per_step=rep["solve_ms"] / n, predict_ms_per_step=rep["predict_ms"] / n,
                                correct_ms_per_step=rep["correct_ms"] / n, u_max=float(np.abs(res["u"]).max())))
    print(json.dumps(out))
    K.free()
    ctx.close()


if __name__ == "__main__":
    main()
