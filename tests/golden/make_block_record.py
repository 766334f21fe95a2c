"""Generates tests/golden/block_record.json: what the block kernels of stan_amd/csrc/modal.hip and the two block drivers
(api_modal.hip, api_buckling.hip) COMPUTE, bit for bit.

    python tests/golden/make_block_record.py [--out FILE]          (on a GPU, from the repo root)

A guard for changes that must not move a bit: the long-double bounds and the dense eigen-solves of tests/test_gpu_modes.py
and tests/test_gpu_buckling.py let a reordered sum pass, this record does not.  Run by hand at a commit known good;
tests/test_gpu_block_record.py recomputes the same cases (it imports them from this file) and asserts equality with the
committed record.

THE HASHES ARE TIED TO THE COMPILER AND THE DEVICE GENERATION (the kernels' instruction order decides the last bit of
every sum): regenerate the record -- at a commit known good -- when either changes.

Block kernels alone, key "block/N<N>_q<q>": N in BLOCK_N x q in BLOCK_Q, inputs as _block of tests/test_gpu_modes.py makes
them.  N = 4097 has two workgroups of gram partials and crosses the 1024- and 256-row boundaries of the other kernels; the
q reach every width the rotate kernels are built for (8, 16, 24, 32) and both gram kernels (q <= 16 and above).
    gram                              sha256 of A and of B (ctx.block_gram)
    rotate_<aliased|apart>_<mask>     sha256 of X, KX, rhs, rho2 (ctx.block_rotate; in_place or not; mask all clear, all
                                      set, alternating)
    buckling_rotate                   sha256 of X, KX, R, r2, kx2 (ctx.buckling_rotate)
Drivers, key "modes/<model>/<run>" and "buckling/<model>/<run>": K.modes on cube6 and cube6j of tests/modes_ref.py,
ctx.buckling on column20 and cube6j of tests/test_gpu_buckling.py, each at the k and tolerance of its existing test
("as_tested") and with max_outer = 1 ("one_outer"); K.modes on cube6 with k = 12 ("wide": a block of 20 columns, the
rotate kernel of width 24 and the wide gram kernel; the restatement of tests/modes_ref.py converges there in 24 steps).
    lambda | factor, phi, rho         sha256 of each
    every report field whose name does not end in _ms (floats as float.hex())
The drivers are the only cases that reach the start, axpy and normalise kernels.
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
RECORD = os.path.join(HERE, "block_record.json")

BLOCK_N = (1, 65, 4097)
BLOCK_Q = (1, 8, 9, 17, 25, 32)
MODES_MODELS = ("cube6", "cube6j")
BUCKLING_MODELS = ("column20", "cube6j")
WIDE_K = 12


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hashes(names, arrays):
    return {n: _sha(a) for n, a in zip(names, arrays)}


def block_key(N, q):
    return "block/N%d_q%d" % (N, q)


def block_case(ctx, N, q):
    """The block kernels alone on one shape, {call: {output: sha256}}"""
    from tests.test_gpu_modes import _block
    Z, W, M = _block(N, q, 1000 * q + N % 997)
    Y, _, D = _block(N, q, 1000 * q + N % 997 + 1)
    rng = np.random.default_rng(q)
    Q = rng.standard_normal((q, q))
    lam = 10.0 ** rng.uniform(0, 2, q)
    rhs0 = rng.standard_normal((q, N))
    mu = rng.standard_normal(q) * 10.0 ** rng.uniform(-2, 2, q)
    out = {"gram": _hashes(("A", "B"), ctx.block_gram(Z, W, M))}
    masks = (("clear", np.zeros(q, np.uint8)), ("set", np.ones(q, np.uint8)), ("alternating", (np.arange(q) % 2).astype(np.uint8)))
    for in_place in (False, True):
        for mname, mask in masks:
            got = ctx.block_rotate(Z, W, M, Q, lam, mask=mask, in_place=in_place, rhs=rhs0)
            out["rotate_%s_%s" % ("aliased" if in_place else "apart", mname)] = _hashes(("X", "KX", "rhs", "rho2"), got)
    out["buckling_rotate"] = _hashes(("X", "KX", "R", "r2", "kx2"), ctx.buckling_rotate(Z, W, Y, D, Q, mu))
    return out


def _driver_record(first, vectors, rep):
    rec = _hashes((first, "phi", "rho"), vectors)
    for f, v in rep.items():
        if not f.endswith("_ms"):
            rec[f] = float(v).hex() if isinstance(v, float) else int(v)
    return rec


def _mesh_args(j):
    return (j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)


def modes_runs(name):
    """(run, keywords of K.modes) of a model; the k of its existing test comes from the model's reference"""
    from tests.test_gpu_modes import TOL
    runs = [("as_tested", dict(n_modes=None, tol=TOL)), ("one_outer", dict(n_modes=None, tol=TOL, max_outer=1))]
    if name == "cube6":
        runs.append(("wide", dict(n_modes=WIDE_K, tol=TOL)))
    return runs


def modes_cases(ctx, name):
    """{run: record} of K.modes on one model of tests/modes_ref.py"""
    from tests import modes_ref as R
    j = R.job(name)
    K = ctx.assemble_hex8(*_mesh_args(j))
    try:
        M = ctx.lumped_mass_hex8(*_mesh_args(j), R.mat_rho(name))[0]
        k = R.reference(name, R.dense(*K.to_csr(upper_only=False)))["k"]      # as the fixture of tests/test_gpu_modes.py
        out = {}
        for run, kw in modes_runs(name):
            kw = dict(kw, n_modes=kw["n_modes"] or k)
            lam, phi, rho, rep = K.modes(M, **kw)
            out[run] = _driver_record("lambda", (lam, phi, rho), rep)
        return out
    finally:
        K.free()


def buckling_runs():
    return ("as_tested", {}), ("one_outer", dict(max_outer=1))


def buckling_cases(ctx, name):
    """{run: record} of ctx.buckling on one model of tests/test_gpu_buckling.py, set up as its fixture does"""
    from tests import buckling_ref as B
    from tests import test_gpu_buckling as TB
    j = TB._job(name)
    k, tol = TB.CASES[name]
    K = ctx.assemble_hex8(*_mesh_args(j))
    G = None
    try:
        U, rep = K.cg_solve(j.F, 1e-12)
        assert rep["terminationtype"] in (1, 7), rep
        G = K.geometric_stiffness(j.xyz, B.disp_full(j, U), *_mesh_args(j)[1:])
        out = {}
        for run, kw in buckling_runs():
            fac, phi, rho, rep = ctx.buckling(K, G, k, **dict(dict(tol=tol, max_outer=300), **kw))
            out[run] = _driver_record("factor", (fac, phi, rho), rep)
        return out
    finally:
        if G is not None:
            G.free()
        K.free()


def keys():
    out = [block_key(N, q) for N in BLOCK_N for q in BLOCK_Q]
    out += ["modes/%s/%s" % (m, run) for m in MODES_MODELS for run, _ in modes_runs(m)]
    out += ["buckling/%s/%s" % (m, run) for m in BUCKLING_MODELS for run, _ in buckling_runs()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    import torch  # noqa: F401  (first, so one HIP runtime is shared)
    from stan_amd import hip
    ctx = hip.Context(0)
    rec = {}
    try:
        for N in BLOCK_N:
            for q in BLOCK_Q:
                rec[block_key(N, q)] = block_case(ctx, N, q)
        for m in MODES_MODELS:
            rec.update({"modes/%s/%s" % (m, run): r for run, r in modes_cases(ctx, m).items()})
        for m in BUCKLING_MODELS:
            rec.update({"buckling/%s/%s" % (m, run): r for run, r in buckling_cases(ctx, m).items()})
    finally:
        ctx.close()
    assert sorted(rec) == sorted(keys())
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d records to %s (library %s)" % (len(rec), a.out, hip.LIB_PATH))


if __name__ == "__main__":
    main()
