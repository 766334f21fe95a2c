#!/usr/bin/env python3
"""Phases of stan_hip_explicit at size: the n^3 cube of bench.py (clamped on x) under its own load as a step load, from rest.

    python tools/explicit_time.py N STEPS [--dt-scale S] [--t1 T1] [--rho R] [--repeats K]

dt = S * 2 / sqrt(lambda_upper) (S = 0.9, what `stan_solver --explicit --dt auto` would take).  After one warm-up run of 100 steps:
K runs of STEPS steps with profiling off (wall time less the wall time of a run of 0 steps: the loop alone, enqueue-bound or
not), then one run with profiling on (every piece between two events and synchronised: product_ms and update_ms per step hold
some microseconds of launch latency each).  Prints one JSON line: the sizes, the run's own stream rate (stan_hip_stream_bench)
and product time (stan_hip_spmv_bench, the product with its p.Ap sum), both lambdas at n_power 30 and 100, dt, ms per step, the
product's and the update's share, the update pass next to its algorithmic bytes over the stream rate
    update   K u, u_n, u_{n-1}, M, F read, u_{n+1} written: 48 n_pad bytes (the plain form; n_pad = 3 * 64 * slices)
    bound    K's values and columns read once: n_slots 64 (72 + 4) bytes
and, with --t1 (the first period, e.g. from profiles/transient_n148.md), the seconds per period T1.  In the same session, for
comparison: the shift pass of stan_hip_transient (one step at the same dt: its report's shift_ms) next to the row bound, and
--variant-steps V steps of THE SAME LOOP DRIVEN THROUGH stan_spmv_reduced per step -- a throwaway variant that exists only here: it
calls the library's internal stan_spmv_reduced and stan_cd_update_device by their C++ symbol names on torch tensors in the reduced
numbering (what a driver without the resident product entry would have done: two padded vectors allocated, one cleared, expand,
product, compress and a stream synchronisation per step), and reports how far its end state lies from the resident loop's (its
u_{-1} is a torch expression, rounded in another order than k_cd_start's)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def variant_through_spmv_reduced(ctx, K, M, F, dt, steps):
    """The throwaway variant (see the module text): ms per step, and the largest difference of its end state from stan_hip_explicit's."""
    import ctypes as C
    import torch
    lib = ctx.lib
    spmv = getattr(lib, "_Z17stan_spmv_reducedP8stan_ctxP11stan_matrixPKdPd")
    update = getattr(lib, "_Z21stan_cd_update_deviceP8stan_ctxlRK12stan_cd_coefdxPKdS5_S5_PdS5_S5_S6_S6_S6_S6_S6_Px")
    coef = (C.c_double * 6)(dt, dt * dt, 2.0 * dt, 1.0, 1.0, 0.0)      # stan_cd_coef without damping
    dev = torch.device("cuda:0")
    N = M.shape[0]
    Md, Fd = torch.from_numpy(M).to(dev), torch.from_numpy(F).to(dev)
    u, Ku = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    up = (0.5 * dt * dt) * Fd / Md                                       # u_{-1} from rest: (dt2 / 2) a_0, a_0 = F / M
    flag = torch.full((1,), 2 ** 62, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    p = lambda x: C.c_void_p(x.data_ptr())
    null = C.c_void_p(0)

    def step(n):
        nonlocal u, up
        if n > 0:
            rc = spmv(ctx.h, K.k, p(u), p(Ku))
            assert rc == 0, rc
        rc = update(ctx.h, C.c_int64(N), C.byref(coef), C.c_double(1.0), C.c_longlong(n + 1), p(Ku), null, p(u), p(up), p(Md), p(Fd),
                    null, null, null, null, null, p(flag))
        assert rc == 0, rc
        u, up = up, u
    for n in range(min(steps, 20)):       # warm-up, then from rest again
        step(n)
    torch.cuda.synchronize()
    u.zero_(); Ku.zero_(); up.copy_((0.5 * dt * dt) * Fd / Md)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(steps + 1):
        step(n)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    want = K.explicit(M, F, dt, steps)["u"]
    got = up.cpu().numpy()               # after the last swap `up` holds u_{steps}
    return dict(variant_steps=steps, variant_ms_per_step=wall / (steps + 1) * 1e3,
                variant_end_state_max_abs_diff=float(np.abs(got - want).max()), variant_end_state_same_bits=bool(np.array_equal(got, want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("steps", type=int)
    ap.add_argument("--dt-scale", type=float, default=0.9)
    ap.add_argument("--t1", type=float, default=0.0)
    ap.add_argument("--rho", type=float, default=7.85e-9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--variant-steps", type=int, default=0)
    a = ap.parse_args()
    import torch  # noqa: F401  first: one shared HIP runtime
    from stan_amd import hip, problem
    j = problem.cube_job(a.n)
    ctx = hip.Context(0)
    ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
    K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    M, _, sums = ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, [a.rho], mass_node=False)
    info = K.info()
    N = M.shape[0]
    F = np.asarray(j.F, dtype=np.float64)
    n_pad = 3 * 64 * ((info["n_block_rows"] + 63) // 64)
    out = dict(n=a.n, N=N, n_pad=n_pad, steps=a.steps, total_mass=sums.total_mass, n_slots=info["n_slots"])
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    out.update(stream_GBs=round(stream, 1), spmv_bench_ms=K.spmv_bench(20))
    up, p30, dts = K.stable_step(M, 30)
    _, p100, _ = K.stable_step(M, 100)
    dt = a.dt_scale * dts
    out.update(lambda_upper=up, lambda_power_30=p30, lambda_power_100=p100, upper_over_power_30=up / p30, upper_over_power_100=up / p100,
               dt_stable=dts, dt=dt, dt_provably_unstable_above=2.0 / np.sqrt(p100))
    K.explicit(M, F, dt, 100)                                  # warm-up: the pool's blocks, the packed columns
    walls, zero = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); K.explicit(M, F, dt, 0); zero.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); res = K.explicit(M, F, dt, a.steps); walls.append(time.perf_counter() - t0)
    loop = [(w - z) / a.steps * 1e3 for w, z in zip(walls, zero)]
    out.update(wall_s=[round(w, 4) for w in walls], wall_zero_steps_s=[round(z, 4) for z in zero], ms_per_step=[round(x, 5) for x in loop],
               ms_per_step_median=float(np.median(loop)), u_max=float(np.abs(res["u"]).max()))
    ctx.set_profiling(True)
    rep = K.explicit(M, F, dt, a.steps, n_power=30)["report"]
    ctx.set_profiling(False)
    n = a.steps + 1
    update_bytes, bound_bytes = 48 * n_pad, info["n_slots"] * 64 * (72 + 4)
    out.update(product_ms_per_step=rep["product_ms"] / a.steps, update_ms_per_step=rep["update_ms"] / (n + 1), bound_ms=rep["bound_ms"],
               power_ms=rep["power_ms"], power_ms_per_product=rep["power_ms"] / 31, update_bytes=update_bytes,
               update_ms_at_stream=update_bytes / stream / 1e6, bound_bytes=bound_bytes, bound_ms_at_stream=bound_bytes / stream / 1e6)
    ctx.set_profiling(True)
    out.update(shift_ms_same_session=K.transient(M, F, dt, 1)["report"]["shift_ms"])
    ctx.set_profiling(False)
    if a.variant_steps > 0:
        out.update(variant_through_spmv_reduced(ctx, K, M, F, dt, a.variant_steps))
    if a.t1 > 0:
        out.update(T1=a.t1, steps_per_T1=a.t1 / dt, s_per_T1=a.t1 / dt * out["ms_per_step_median"] / 1e3)
    print(json.dumps(out))
    K.free()
    ctx.close()


if __name__ == "__main__":
    main()
