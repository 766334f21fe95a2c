#!/usr/bin/env python3
"""Linear buckling at size: the n^3 cube of bench.py clamped on x = 0, compressed along x by a point
load on every node of the face x = n; the static solve, G = K_g(U) and the K lowest load factors.

    python tools/buckling_time.py N K [--solve-eps E] [--tol T] [--max-outer M]

Prints one JSON line: the sizes, the static solve, the wall time of stan_hip_geometric_stiffness_hex8_dev with the inputs
resident, its element pass, layout copy, lists and gather by HIP events (stan_hip_geometric_stiffness_times) next to the
algorithmic bytes of the two passes over the run's own stream rate (stan_hip_stream_bench: what this device gives a read-only
sweep of K's values), stan_hip_internal_forces_hex8_dev with its k_if_elem in the same process as the yardstick of the element
pass, outer steps, CG iterations and the stream time in solves / products / block kernels (by events), and the factors."""
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
    ap.add_argument("--max-outer", type=int, default=0)
    a = ap.parse_args()
    import torch
    from stan_amd import hip, problem
    from stan_amd.cube import cube_bcs, cube_mesh
    xyz, conn = cube_mesh(a.n)
    spc, ld, f = cube_bcs(a.n, load=(-50.0, 0.0, 0.0))
    j = problem.make_job(xyz, conn, spc, np.ones((spc.shape[0], 3)), ld, np.tile(f, (ld.shape[0], 1)))
    ctx = hip.Context(0)
    ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
    ctx.set_profiling(True)
    K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    t0 = time.perf_counter()
    U, srep = K.cg_solve(j.F, 1e-8)
    static_s = time.perf_counter() - t0
    full = np.zeros(j.n_dof)
    full[np.asarray(j.red) != -1] = U
    disp = full[np.asarray(j.node_dof).reshape(-1)].reshape(-1, 3)

    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    d_xyz, d_disp, d_dof, d_conn, d_mat, d_type, d_red = (up(x) for x in (j.xyz, disp, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.red))
    nn, ne = j.xyz.shape[0], j.conn.shape[0]
    args = (nn, d_xyz.data_ptr(), d_disp.data_ptr(), d_dof.data_ptr(), ne, d_conn.data_ptr(), d_mat.data_ptr(), d_type.data_ptr(),
            j.mat_E_nu, j.n_dof, d_red.data_ptr())
    torch.cuda.synchronize()
    g_ms = []
    G = None
    for _ in range(3):          # the first call pays the allocations; the pool hands the blocks back to the later ones
        if G is not None:
            G.free()
        t0 = time.perf_counter()
        G = K.geometric_stiffness_dev(*args)
        g_ms.append((time.perf_counter() - t0) * 1e3)
    kg_times = ctx.geometric_stiffness_times()
    d_fint = torch.empty(j.n_dof, dtype=torch.float64, device=dev)
    f_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.internal_forces_hex8_dev(*args, d_f_int=d_fint.data_ptr(), eq=False)
        f_ms.append((time.perf_counter() - t0) * 1e3)
    forces_elem_ms = ctx.profile()["forces_elem_ms"]

    t0 = time.perf_counter()
    fac, phi, rho, rep = ctx.buckling(K, G, a.k, tol=a.tol, max_outer=a.max_outer, solve_eps=a.solve_eps)
    wall = time.perf_counter() - t0
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    info = K.info()
    # algorithmic bytes: the element pass reads 8 (conn) + 48 (xyz, disp) words per element once and writes 36 doubles; the
    # gather reads the 36 doubles of every incidence (8 per node), its column words, and writes the 9-value slots of G
    elem_bytes = ne * (8 * 4 + 48 * 8 + 36 * 8)
    gather_bytes = ne * 8 * 36 * 8 + info["n_slots"] * 64 * (4 + 72)
    out = dict(n=a.n, N=j.n_red, n_modes=a.k, solve_eps=a.solve_eps or 1e-6, tol=a.tol or 1e-6, static_solve_s=round(static_s, 3),
               static_iterations=srep["iterations"], g_build_ms=[round(x, 3) for x in g_ms], forces_call_ms=[round(x, 3) for x in f_ms],
               forces_elem_ms=forces_elem_ms, **kg_times, stream_GBs=round(stream, 1), elem_pass_bytes=elem_bytes,
               elem_pass_ms_at_stream=elem_bytes / stream / 1e6, gather_bytes=gather_bytes,
               gather_ms_at_stream=gather_bytes / stream / 1e6, driver_wall_s=round(wall, 3), factor=list(fac), rho=list(rho), **rep)
    print(json.dumps(out))
    G.free()
    K.free()
    ctx.close()


if __name__ == "__main__":
    main()
