"""What the device tests of the products and of the CG loop share (tests/test_gpu_product_precision.py,
tests/test_gpu_sharded_precision.py, tests/test_gpu_reduced_forms.py, tests/test_gpu_refinement_passes.py,
tests/test_gpu_cg_restart.py): the library's default options and the block that sets some and puts them back, a fresh assembly of a model of tests/product_ref.py on a
one-device context, the matrix it exports with its probes, and the long-double CG on that matrix -- each computed once per
pytest run (product_ref.cached) and left unchanged."""
from stan_amd import hip
from tests import product_ref as P

DEFAULTS = {hip.OPT_CG_MERIT_STOP: 1, hip.OPT_SPMV_VARIANT: -1, hip.OPT_SPMV_SMALL: 1, hip.OPT_PACKED_COLUMNS: 1, hip.OPT_SELL_SIGMA: 1,
            hip.OPT_ROW_FOLDING: -1, hip.OPT_VALUE_STREAM_60: -1, hip.OPT_CG_FOLD_REDUCE: 1, hip.OPT_CG_FUSED_REFRESH: 1,
            hip.OPT_CG_DEFER_X: 1, hip.OPT_CG_SINGLE_REDUCE: 0, hip.OPT_CG_REFINE: 1, hip.OPT_OVERLAP_HALO: 1, hip.OPT_COMM_P2P: 0,
            hip.OPT_CG_RUPDATE: 10, hip.OPT_CG_X_RING: -1}
LARGE = {hip.OPT_SPMV_SMALL: 0}
PADDED = {**LARGE, hip.OPT_ROW_FOLDING: 0}            # the padded streams: left to itself (-1) the library folds where that saves slots


class options:
    """Options set for a block, every one restored to its default behind it -- also when the block fails; profiling on inside."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.ctx.set_profiling(True)
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        try:
            for k in self.opts:
                self.ctx.set_option(k, DEFAULTS[k])
        finally:
            self.ctx.set_profiling(False)


def assemble(ctx, name, sigma=1):
    j = P.job(name)
    ctx.set_option(hip.OPT_SELL_SIGMA, sigma)
    try:
        K = ctx.assemble_hex8(j.xyz, j.node_dof, j.conn, j.elem_mat, j.elem_type, j.mat_E_nu, j.red)
    finally:
        ctx.set_option(hip.OPT_SELL_SIGMA, DEFAULTS[hip.OPT_SELL_SIGMA])
    assert K.info()["scaled"] == 0 and K.info()["sell_sigma"] == sigma
    return K


def model(ctx, name):
    """(csr, probes) of a model: the matrix as a fresh assembly exports it (the exact bits, nothing scaled), the colouring
    computed once per pytest run."""
    def make():
        K = assemble(ctx, name)
        csr = K.to_csr(upper_only=False)
        assert K.info()["scaled"] == 0
        K.free()
        colour = P.colours(csr[0], csr[1], P.cube_grid(name))
        return csr, P.Probes(csr[0], csr[1], colour, P.weights(csr[0].shape[0] - 1))
    return P.cached(("gpu", name), make)


def reference(ctx, name, lc=0):
    """([U_k], [rel_k]), k = 1 .. KMAX: the long-double CG on the exported matrix under load vector lc of product_ref.load_cases."""
    csr, _probes = model(ctx, name)
    return P.cached(("gpu", "cg", name, lc), lambda: P.cg_reference(csr, P.load_cases(name)[lc], P.KMAX))


def reduced_reference(ctx, name, stream):
    """The same under the job's own load vector on the matrix quantised as `stream` quantises it, k = 1 .. KMAX_REDUCED."""
    csr, _probes = model(ctx, name)
    return P.cached(("gpu", "cg", name, stream), lambda: P.cg_reference(csr, P.job(name).F, P.KMAX_REDUCED, quantise=P.QUANTISE[stream]))


# ---- the sharded loop (tests/sharded_iterates_worker.py, tests/test_gpu_sharded_precision.py) -------------------------------------
# form -> (options on top of STAN_OPT_CG_MERIT_STOP 0, precision mode, compared iterates, load cases of product_ref.load_cases)
SHARDED_FORMS = {
    "classic": ({hip.OPT_COMM_P2P: 0}, hip.PREC_FP64, P.KMAX, (0, 1)),                # the split product over k_spmv_small, an all-reduce per sum
    "classic_p2p": ({hip.OPT_COMM_P2P: 1}, hip.PREC_FP64, P.KMAX, (0, 1)),            # mailboxes and arrival counters (p2p.hip)
    "no_overlap": ({hip.OPT_OVERLAP_HALO: 0}, hip.PREC_FP64, P.KMAX, (0, 1)),         # the unsplit product, the exchange in front of it
    "large": ({hip.OPT_SPMV_SMALL: 0, hip.OPT_ROW_FOLDING: 0}, hip.PREC_FP64, P.KMAX, (0, 1)),      # k_spmv on the split lists
    "fold": ({hip.OPT_SPMV_SMALL: 0, hip.OPT_ROW_FOLDING: 1}, hip.PREC_FP64, P.KMAX, (0,)),         # k_spmv_fold on them
    "separate_reductions": ({hip.OPT_CG_FOLD_REDUCE: 0}, hip.PREC_FP64, P.KMAX, (0,)),              # k_reduce publishes the sums
    "single_reduction": ({hip.OPT_CG_SINGLE_REDUCE: 1}, hip.PREC_FP64, P.KMAX, (0,)),
    "single_reduction_p2p": ({hip.OPT_CG_SINGLE_REDUCE: 1, hip.OPT_COMM_P2P: 1}, hip.PREC_FP64, P.KMAX, (0,)),
    "fixed48": ({hip.OPT_CG_REFINE: 0}, hip.PREC_FIXED48, P.KMAX_REDUCED, (0,)),
}
SHARDED_PROFILE = ("value_stream", "loop_collectives", "loop_stream_waits", "rel_residual_recurrence")
