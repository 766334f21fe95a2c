#!/usr/bin/env python3
"""Phases of stan_hip_modes at size: the n^3 cube of bench.py (clamped on x), the K lowest modes.

    python tools/modes_time.py N K [--solve-eps E] [--tol T] [--rho R]

Prints one JSON line: the sizes, outer steps, CG iterations, the stream time in solves / products / block kernels (by events),
the gram and rotate passes next to their algorithmic bytes over the run's own stream rate (stan_hip_stream_bench: what this
device gives a read-only sweep of K's values), and the lowest frequencies."""
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
    ap.add_argument("k", type=int)
    ap.add_argument("--solve-eps", type=float, default=0.0)
    ap.add_argument("--tol", type=float, default=0.0)
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
    t0 = time.perf_counter()
    lam, phi, rho, rep = K.modes(M, a.k, tol=a.tol, solve_eps=a.solve_eps)
    wall = time.perf_counter() - t0
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    N, q, outer = M.shape[0], rep["block"], rep["outer"]
    # algorithmic bytes of one pass: gram reads Z, W and M once; rotate reads them and writes X, KX and the right-hand sides
    gram_bytes = (2 * q + 1) * N * 8
    rot_bytes = (5 * q + 1) * N * 8
    out = dict(n=a.n, N=N, n_modes=a.k, solve_eps=a.solve_eps or 1e-6, tol=a.tol or 1e-6, wall_s=round(wall, 3), total_mass=sums.total_mass,
               stream_GBs=round(stream, 1), gram_ms_per_pass=rep["gram_ms"] / outer, gram_bytes=gram_bytes,
               gram_ms_at_stream=gram_bytes / stream / 1e6, rotate_ms_per_pass=rep["rotate_ms"] / outer, rotate_bytes=rot_bytes,
               rotate_ms_at_stream=rot_bytes / stream / 1e6, frequency_hz=list(np.sqrt(lam) / (2 * np.pi)), rho=list(rho), **rep)
    print(json.dumps(out))
    K.free()
    ctx.close()


if __name__ == "__main__":
    main()
