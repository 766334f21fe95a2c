"""Generates tests/golden/cg_loop_record.json: what the CG loops of stan_amd/csrc/cg.hip COMPUTE and ENQUEUE, per loop form.

    python tests/golden/make_cg_loop_record.py [--out FILE]          (on a GPU, from the repo root)

A guard for host-side changes of the loop: it says in seconds whether a change moved a bit of the answer or a launch,
collective or stream wait of the loop.  Run by hand at a commit known good; tests/test_gpu_cg_record.py recomputes the
same cases (it imports them from this file) and asserts equality with the committed record.

THE HASHES ARE TIED TO THE COMPILER AND THE DEVICE GENERATION (the kernels' instruction order decides the last bit of
every sum): regenerate the record -- at a commit known good -- when either changes.

Per case:
    U_sha256                                   sha256 of U.tobytes()
    terminationtype, iterations, rel_residual  the report (rel_residual as float.hex())
    PROFILE fields, profiling on               launches, iterations enqueued, collectives, stream waits of the loop; the
                                               value stream, refinement passes, fp64 products, stream format and bytes
Cases: problem.cube_job(n, jitter=0.05), eps 1e-10, on
    n = 6     343 block rows, 6 slices: fewer blocks than the ticket counters of a folded reduction has sub-counters
    n = 14    3375 block rows, 53 slices (a ragged last workgroup), 40 vector blocks: more than sub-counters
each with the small-system product kernel (OPT_SPMV_SMALL 1) and with the large-system kernels (OPT_SPMV_SMALL 0) on
padded (OPT_ROW_FOLDING 0) and folded (1) streams; every loop form of _forms, one option at a time off its default; the
60-bit value stream alone and with each option it shares the choice of kernel and stream with (_stream60_forms: on
every matrix form, so that "inert here" is recorded too); solves on a fresh matrix each (_fresh_forms); and
cg_solve_multi with 7 right-hand sides (groups of 4 + 2 + 1; one of them zero), one record per column.
Only stan_amd's public Python API is used.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "cg_loop_record.json")

EPS = 1e-10
SIZES = (6, 14)
# (name, OPT_SPMV_SMALL, OPT_ROW_FOLDING or None: left alone -- the small-system kernel reads no folded stream)
MATRIX_FORMS = (("small", 1, None), ("large_padded", 0, 0), ("large_folded", 0, 1))
PROFILE_FIELDS = ("loop_kernel_launches", "loop_iterations_enqueued", "loop_collectives", "loop_stream_waits",
                  "value_stream", "refine_passes", "fp64_products", "repacked_streams", "col_slots_packed", "spmv_bytes")
N_RHS = 7
ZERO_COLUMN = 3


def _forms(hip):
    """(name, [(option, value off its default, default)], solve keywords, right-hand side scale)"""
    P = {"mixed": hip.PREC_MIXED, "fixed48": hip.PREC_FIXED48}
    forms = [
        ("default", [], {}, 1.0),
        ("fold_reduce_0", [(hip.OPT_CG_FOLD_REDUCE, 0, 1)], {}, 1.0),
        ("single_reduce_1", [(hip.OPT_CG_SINGLE_REDUCE, 1, 0)], {}, 1.0),
        ("fused_refresh_0", [(hip.OPT_CG_FUSED_REFRESH, 0, 1)], {}, 1.0),
        ("defer_x_0", [(hip.OPT_CG_DEFER_X, 0, 1)], {}, 1.0),
        ("merit_stop_0", [(hip.OPT_CG_MERIT_STOP, 0, 1)], {}, 1.0),
        # (3 is the default: the two bits choose k_update's and k_step's stores one by one)
        ("vec_store_nt_0", [(hip.OPT_VEC_STORE_NT, 0, 3)], {}, 1.0),
        ("vec_store_nt_1", [(hip.OPT_VEC_STORE_NT, 1, 3)], {}, 1.0),
        ("vec_store_nt_2", [(hip.OPT_VEC_STORE_NT, 2, 3)], {}, 1.0),
        ("vec_store_nt_3", [(hip.OPT_VEC_STORE_NT, 3, 3)], {}, 1.0),
        ("packed_columns_0", [(hip.OPT_PACKED_COLUMNS, 0, 1)], {}, 1.0),
        ("spmv_variant_20", [(hip.OPT_SPMV_VARIANT, 20, -1)], {}, 1.0),
        ("spmv_variant_0", [(hip.OPT_SPMV_VARIANT, 0, -1)], {}, 1.0),
    ]
    for prec in ("mixed", "fixed48"):
        for refine in (0, 1, 2):
            forms.append(("%s_refine_%d" % (prec, refine), [(hip.OPT_CG_REFINE, refine, 1)], {"precision_mode": P[prec]}, 1.0))
    forms.append(("max_its_7", [], {"max_its": 7}, 1.0))     # type 5 before the first residual refresh
    forms.append(("zero_rhs", [], {}, 0.0))                  # the first residual test ends it: no iteration
    return forms


def _stream60_forms(hip):
    """The lossless 60-bit value stream (OPT_VALUE_STREAM_60 1) alone and next to every option that decides with it which
    kernel reads which stream, and the two large-system kernel variants alone.  Run BEHIND the forms above (the list only
    grows: the cases in front keep the sequence they were recorded in)."""
    s60 = (hip.OPT_VALUE_STREAM_60, 1, -1)
    forms = [("value_stream_60_1", [s60], {}, 1.0)]
    for v in (12, 9, 0, 20):
        forms.append(("value_stream_60_1_spmv_variant_%d" % v, [s60, (hip.OPT_SPMV_VARIANT, v, -1)], {}, 1.0))
    forms.append(("value_stream_60_1_single_reduce_1", [s60, (hip.OPT_CG_SINGLE_REDUCE, 1, 0)], {}, 1.0))
    forms.append(("value_stream_60_1_fused_refresh_0", [s60, (hip.OPT_CG_FUSED_REFRESH, 0, 1)], {}, 1.0))
    for prec, mode in (("mixed", hip.PREC_MIXED), ("fixed48", hip.PREC_FIXED48)):
        forms.append(("value_stream_60_1_%s_refine_1" % prec, [s60, (hip.OPT_CG_REFINE, 1, 1)], {"precision_mode": mode}, 1.0))
    forms.append(("spmv_variant_9", [(hip.OPT_SPMV_VARIANT, 9, -1)], {}, 1.0))
    forms.append(("spmv_variant_12", [(hip.OPT_SPMV_VARIANT, 12, -1)], {}, 1.0))
    return forms


def _fresh_forms(hip):
    """Solves that must find the matrix as the assembly left it (unscaled, no copy of a stream): a fresh matrix each."""
    s60 = (hip.OPT_VALUE_STREAM_60, 1, -1)
    lazy0 = (hip.OPT_CG_LAZY_SCALING, 0, 1)
    return [
        ("lazy_scaling_0", [lazy0]),                                   # the scaling pass of its own instead of the first product's
        ("fresh_value_stream_60_1", [s60]),                            # the first product scales, then the encoding pass
        ("fresh_value_stream_60_1_lazy_scaling_0", [s60, lazy0]),
        ("fresh_rupdate_1", [(hip.OPT_CG_RUPDATE, 1, 10)]),            # a refresh at iteration 1: no plain first product
    ]


def _solve_record(ctx, K, F, kw):
    U, rep = K.cg_solve(F, EPS, **kw)
    pf = ctx.profile()
    rec = {"U_sha256": hashlib.sha256(U.tobytes()).hexdigest(), "terminationtype": int(rep["terminationtype"]),
           "iterations": int(rep["iterations"]), "rel_residual": float(rep["rel_residual"]).hex()}
    rec.update({f: int(pf[f]) for f in PROFILE_FIELDS})
    return rec


def cases(ctx, n, matrix_form):
    """The records of one size and one matrix form, {case name: record}.  Every option is restored."""
    from stan_amd import hip, problem
    name, small, folding = next(m for m in MATRIX_FORMS if m[0] == matrix_form)
    job = problem.cube_job(n, jitter=0.05)
    args = (job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
    out = {}
    ctx.set_option(hip.OPT_SPMV_SMALL, small)
    if folding is not None:
        ctx.set_option(hip.OPT_ROW_FOLDING, folding)
    ctx.set_profiling(True)

    def solve_with(fname, opts, K, F, kw):
        try:
            for o, v, _ in opts:
                ctx.set_option(o, v)
            out[fname] = _solve_record(ctx, K, F, kw)
        finally:
            for o, _, d in opts:
                ctx.set_option(o, d)

    try:
        K = ctx.assemble_hex8(*args)
        # "default" comes first: the solve that finds the matrix unscaled (the large-system fp64 loop scales it in its
        # first product); "default_scaled_matrix" repeats it on the scaled one
        for fname, opts, kw, fscale in _forms(hip) + [("default_scaled_matrix", [], {}, 1.0)] + _stream60_forms(hip):
            solve_with(fname, opts, K, job.F * fscale, kw)
        # several load cases in one loop: F scaled by 1 .. 7, one column zero
        F2 = np.stack([job.F * float(c + 1) for c in range(N_RHS)])
        F2[ZERO_COLUMN] = 0.0
        U2, reps = K.cg_solve_multi(F2, EPS)
        for c in range(N_RHS):
            out["multi_column_%d" % c] = {
                "U_sha256": hashlib.sha256(U2[c].tobytes()).hexdigest(), "terminationtype": int(reps[c]["terminationtype"]),
                "iterations": int(reps[c]["iterations"]), "rel_residual": float(reps[c]["rel_residual"]).hex()}
        K.free()
        for fname, opts in _fresh_forms(hip):
            K = ctx.assemble_hex8(*args)
            solve_with(fname, opts, K, job.F, {})
            K.free()
    finally:
        ctx.set_profiling(False)
        ctx.set_option(hip.OPT_SPMV_SMALL, 1)
        ctx.set_option(hip.OPT_ROW_FOLDING, -1)
    return out


def key(n, matrix_form):
    return "n%d/%s" % (n, matrix_form)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so one HIP runtime is shared)
    from stan_amd import hip
    ctx = hip.Context(0)
    rec = {}
    try:
        for n in SIZES:
            for m, _, _ in MATRIX_FORMS:
                rec[key(n, m)] = cases(ctx, n, m)
    finally:
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d records to %s" % (sum(len(v) for v in rec.values()), a.out))


if __name__ == "__main__":
    main()
