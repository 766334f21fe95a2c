#!/usr/bin/env python3
"""The consistent mass at size: the n^3 cube of bench.py clamped on x = 0.

    python tools/mass_time.py N [--modes K] [--solve-eps E] [--tol T] [--max-outer M]

Prints one JSON line: the sizes; the wall time of stan_hip_consistent_mass_hex8_dev with the inputs resident and its element
pass (k_cm_elem), layout copy, lists and gather by HIP events (stan_hip_consistent_mass_times) next to the same four phases of
stan_hip_geometric_stiffness_hex8_dev (k_kg_elem, the same gather) in the same process; the value pass of stan_hip_matrix_axpy
(k_matrix_axpy) by events next to its algorithmic bytes -- three value arrays -- at the run's own stream rate
(stan_hip_stream_bench: what this device gives a read-only sweep of K's values) and next to k_shift_matrix (shift_ms of a
one-step stan_hip_transient on the lumped mass: two value arrays); with --modes K the K lowest modes on the lumped mass
(stan_hip_modes) against the consistent one (stan_hip_modes_pencil): outer steps, CG iterations, seconds.  Progress lines go to
stderr."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RHO = 7.85e-9


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("--modes", type=int, default=0)
    ap.add_argument("--solve-eps", type=float, default=0.0)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--max-outer", type=int, default=0)
    a = ap.parse_args()
    import torch
    from stan_amd import hip, problem
    from stan_amd.cube import cube_bcs, cube_mesh
    xyz, conn = cube_mesh(a.n)
    spc, ld, f = cube_bcs(a.n)
    j = problem.make_job(xyz, conn, spc, np.ones((spc.shape[0], 3)), ld, np.tile(f, (ld.shape[0], 1)))
    rho = np.array([RHO])
    ctx = hip.Context(0)
    ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
    ctx.set_profiling(True)
    K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    note("assembled: N = %d" % j.n_red)

    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    disp = np.random.default_rng(1).standard_normal(j.xyz.shape) * 1e-3
    d_xyz, d_disp, d_dof, d_conn, d_mat, d_type, d_red = (up(x) for x in (j.xyz, disp, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.red))
    nn, ne = j.xyz.shape[0], j.conn.shape[0]
    tail = (d_dof.data_ptr(), ne, d_conn.data_ptr(), d_mat.data_ptr(), d_type.data_ptr(), j.mat_E_nu, j.n_dof, d_red.data_ptr())
    torch.cuda.synchronize()

    def build(call):          # the first call pays the allocations; the pool hands the blocks back to the later ones
        ms, X = [], None
        for _ in range(3):
            if X is not None:
                X.free()
            t0 = time.perf_counter()
            X = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return X, [round(x, 3) for x in ms]

    G, g_ms = build(lambda: K.geometric_stiffness_dev(nn, d_xyz.data_ptr(), d_disp.data_ptr(), *tail))
    kg_times = ctx.geometric_stiffness_times()
    G.free()
    Mc, m_ms = build(lambda: K.consistent_mass_dev(nn, d_xyz.data_ptr(), rho, *tail))
    cm_times = ctx.consistent_mass_times()
    note("M_c built: %s" % cm_times)

    M, _mn, sums = ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, rho)
    sigma = 4.0 / (1e-4 ** 2)            # a Newmark a0
    S, s_ms = build(lambda: K.axpy(sigma, Mc))
    axpy_ms = ctx.consistent_mass_times()["axpy_ms"]
    S.free()
    tr = K.transient(M, j.F, 1e-4, 1, solve_eps=1e-3)["report"]      # one step: its shift_ms is k_shift_matrix's
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    info = K.info()
    values = info["n_slots"] * 64 * 72          # bytes of one value array
    out = dict(n=a.n, N=j.n_red, n_elem=ne, n_slots=info["n_slots"], mass_build_ms=m_ms, **cm_times, g_build_ms=g_ms, **kg_times,
               axpy_call_ms=s_ms, axpy_bytes=3 * values, stream_GBs=round(stream, 1), axpy_ms_at_stream=3 * values / stream / 1e6,
               shift_ms=tr["shift_ms"], shift_bytes=2 * values, shift_ms_at_stream=2 * values / stream / 1e6,
               total_mass=sums.total_mass)
    out["axpy_ms"] = axpy_ms
    note("axpy %.3f ms, shift %.3f ms, stream %.1f GB/s" % (axpy_ms, tr["shift_ms"], stream))
    if a.modes > 0:
        kw = dict(tol=a.tol, max_outer=a.max_outer, solve_eps=a.solve_eps)
        for name, run in (("lumped", lambda: K.modes(M, a.modes, **kw)), ("consistent", lambda: ctx.modes_pencil(K, Mc, a.modes, **kw))):
            t0 = time.perf_counter()
            lam, _phi, rh, rep = run()
            wall = time.perf_counter() - t0
            out["modes_" + name] = dict(wall_s=round(wall, 3), outer=rep["outer"], converged=rep["converged"], cg_iterations=rep["cg_iterations"],
                                        cg_worst_type=rep["cg_worst_type"], solve_ms=rep["solve_ms"], product_ms=rep["product_ms"],
                                        block_ms=rep["block_ms"], max_rho=rep["max_rho"], frequency_hz=list(np.sqrt(lam) / (2 * np.pi)))
            note("modes %s: %s" % (name, out["modes_" + name]))
        out.update(n_modes=a.modes, solve_eps=a.solve_eps or 1e-6, tol=a.tol or 1e-6)
    print(json.dumps(out), flush=True)
    Mc.free()
    K.free()
    ctx.close()


if __name__ == "__main__":
    main()
