#!/usr/bin/env python3
"""Phases of stan_hip_harmonic at size: the n^3 cube of bench.py (clamped on x) under its own load.

    python tools/harmonic_time.py N K NF [--repeats R] [--snaps S] [--real-modes] [--clock-mhz C]

The entry's time does not depend on the values it is given, so by default Phi [K][N] is a block of random numbers made on the
device and lambda K values spread over two decades (the modes of the 148^3 cube cost minutes of CG solves,
profiles/modes_n148.md); --real-modes takes them from stan_hip_modes and u_static from stan_hip_cg_solve instead.  Everything is
resident: the call is stan_hip_harmonic_dev with profiling on, R times after one warm-up, the medians reported.  One JSON line:
the sizes, the run's own stream rate (stan_hip_stream_bench), the device's clock and compute units as the runtime reports them,
and per phase the stream time by events next to its floor:
    sweep    4 K NF N flop (2 K multiply-adds per frequency and DOF) at the fp64 vector rate CUs x 4 SIMDs x 16 lanes x 2 x clock
             (issued: 4 QT NF N, QT = K rounded up to a multiple of 4), and the bytes of Phi at the stream rate
    project  Phi twice, F, u_static, r: (2 K + 3) N 8 bytes at the stream rate
    snaps    Phi, r, 2 S N doubles written
and what NF passes of the snapshot kind plus a reduction would have moved: NF (K + 1) N 8 bytes read, 2 NF N 8 written and read
again."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rocminfo_gpu_clock_mhz():
    """"Max Clock Freq. (MHz)" of the first GPU agent rocminfo lists (0.0 when it cannot be read): the fallback where the torch
    device properties carry no clock."""
    import re
    import subprocess
    try:
        text = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        return 0.0
    for agent in text.split("Agent ")[1:]:
        if re.search(r"Device Type:\s+GPU", agent):
            m = re.search(r"Max Clock Freq\. \(MHz\):\s+(\d+)", agent)
            if m:
                return float(m.group(1))
    return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("k", type=int)
    ap.add_argument("nf", type=int)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--snaps", type=int, default=2)
    ap.add_argument("--real-modes", action="store_true")
    ap.add_argument("--rho", type=float, default=7.85e-9)
    ap.add_argument("--clock-mhz", type=float, default=0.0)
    a = ap.parse_args()
    import torch  # first: one shared HIP runtime
    from stan_amd import hip, problem
    j = problem.cube_job(a.n)
    ctx = hip.Context(0)
    ctx.set_option(hip.OPT_POOL_MAX_BYTES, -1)
    K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    N = K.info()["n_reduced"]
    ms, nbytes = K.stream_bench(20)
    stream = nbytes / ms / 1e6     # GB/s
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    cus = int(props.multi_processor_count)
    clock_mhz, clock_source = float(getattr(props, "clock_rate", 0)) / 1e3, "device properties"
    if a.clock_mhz > 0:
        clock_mhz, clock_source = a.clock_mhz, "--clock-mhz"
    elif clock_mhz <= 0:
        clock_mhz, clock_source = rocminfo_gpu_clock_mhz(), "rocminfo, Max Clock Freq."
    assert clock_mhz > 0, "neither the device properties nor rocminfo report a clock: pass --clock-mhz"
    F = np.asarray(j.F, dtype=np.float64)
    dF = torch.from_numpy(F).to(dev)
    if a.real_modes:
        M = ctx.lumped_mass_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red, [a.rho], mass_node=False)[0]
        lam, phi, _, mrep = K.modes(M, a.k)
        U = K.cg_solve(F, 1e-10)[0]
        dphi, dus = torch.from_numpy(phi).to(dev), torch.from_numpy(U).to(dev)
        del phi
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        dphi = torch.randn((a.k, N), dtype=torch.float64, device=dev, generator=g)
        dus = torch.randn(N, dtype=torch.float64, device=dev, generator=g)
        lam = np.logspace(8.0, 10.0, a.k)
    K.free()
    dlam = torch.from_numpy(np.ascontiguousarray(lam)).to(dev)
    omega = np.linspace(0.0, 1.2 * np.sqrt(lam[-1]), a.nf)
    snap = np.linspace(0, a.nf - 1, a.snaps).astype(np.int32)
    probe = torch.tensor([0, N // 2, N - 1], dtype=torch.int32, device=dev)
    d_p = torch.empty(a.k, dtype=torch.float64, device=dev)
    d_probe = torch.empty(a.nf * 3 * 2, dtype=torch.float64, device=dev)
    d_snaps = torch.empty(a.snaps * 2 * N, dtype=torch.float64, device=dev)
    d_peak = torch.empty(N, dtype=torch.float64, device=dev)
    d_idx = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    call = lambda: ctx.harmonic_dev(N, a.k, dlam.data_ptr(), dphi.data_ptr(), dF.data_ptr(), omega, d_p.data_ptr(), d_u_static=dus.data_ptr(),
                                    zeta=np.full(a.k, 0.02), n_probe=3, d_probe_dof=probe.data_ptr(), d_probe=d_probe.data_ptr(), snap_freq=snap,
                                    d_snaps=d_snaps.data_ptr(), d_peak=d_peak.data_ptr(), d_peak_idx=d_idx.data_ptr())
    call()                                        # warm-up: the pool's blocks, the code objects
    ctx.set_profiling(True)
    reps = [call() for _ in range(a.repeats)]
    ctx.set_profiling(False)
    med = lambda key: float(np.median([r[key] for r in reps]))
    qt = (a.k + 3) // 4 * 4
    rate = cus * 4 * 16 * 2 * clock_mhz * 1e6     # flop/s
    flop, issued = 4.0 * a.k * a.nf * N, 4.0 * qt * a.nf * N
    phi_bytes, project_bytes = 8.0 * a.k * N, 8.0 * (2 * a.k + 3) * N
    snap_bytes = 8.0 * (a.k + 1 + 2 * a.snaps) * N
    out = dict(n=a.n, N=N, k=a.k, nf=a.nf, qt=qt, real_modes=bool(a.real_modes), stream_GBs=round(stream, 1), compute_units=cus,
               clock_MHz=clock_mhz, clock_source=clock_source, fp64_vector_TFLOPs=rate / 1e12, project_ms=med("project_ms"), sweep_ms=med("sweep_ms"), snap_ms=med("snap_ms"),
               probe_ms=med("probe_ms"), sweep_ms_all=[round(r["sweep_ms"], 4) for r in reps], sweep_flop=flop, sweep_flop_issued=issued,
               sweep_ms_at_fma_rate=flop / rate * 1e3, sweep_ms_issued_at_fma_rate=issued / rate * 1e3,
               sweep_ms_phi_at_stream=phi_bytes / stream / 1e6, project_bytes=project_bytes, project_ms_at_stream=project_bytes / stream / 1e6,
               snap_bytes=snap_bytes, snap_ms_at_stream=snap_bytes / stream / 1e6,
               unfused_bytes=8.0 * a.nf * (a.k + 1) * N + 2 * 16.0 * a.nf * N, peak=reps[-1]["peak"], peak_dof=reps[-1]["peak_dof"],
               peak_freq=reps[-1]["peak_freq"])
    out["sweep_fraction_of_fma_rate"] = out["sweep_ms_at_fma_rate"] / out["sweep_ms"] if out["sweep_ms"] > 0 else 0.0
    out["unfused_ms_at_stream"] = out["unfused_bytes"] / stream / 1e6
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
