// cg.hip -- Conjugate Gradient on gfx950: replaces SolverFunctions.LinearSolver_CG
// (SolverFunctions.cs:270-330), i.e. alglib.lincgcreate / lincgsetcond /
// lincgsolvesparse / lincgresults of alglib.net 3.16.0 (not vendored in the
// reference; its published algorithm is restated here):
//   * diagonal preconditioner applied as a symmetric scaling  A^ = S K S,
//     s_i = 1/sqrt(K_ii) (1 when K_ii <= 0), b^ = S b, result U = S x^;
//   * x0 = 0; stop when ||r^|| <= EpsF ||b^|| (type 1), after MaxIts > 0 iterations
//     (type 5), when the merit function x'Ax - 2b'x stops decreasing (type 7, previous
//     point returned), p'Ap <= 0 (type -5) or non-finite numbers (type -4);
//   * every 10th iteration the residual is recomputed as b^ - A^ x^ (extra SpMV).
//
// All kernels here are HBM-bound streaming kernels.  The scaling is folded into the
// matrix once per matrix, so an iteration is
//   SpMV (+ fused p.Ap)                      reads the matrix once
//   step  : x' = x + a p, r -= a v, r.r, merit   (one pass, 5 reads 2 writes)
//   update: p = r + b p                          (one pass, 2 reads 1 write)
// plus two 1-block reductions of per-block partial sums (fixed order => the whole solve is
// bit-reproducible).  alpha, beta and every stopping decision live in device memory; the
// host only enqueues iterations and polls a status word every CHUNK iterations, so
// there is no host synchronisation inside an iteration.
// Which product kernel reads which value stream of K (stan_matrix::vs, a table by kind) is decided in ONE place, plan_products:
// a product_plan per solve (per call in cg_entries.inc), which launch_product dispatches on and cg_run reads.
#include <chrono>
#include <cmath>
#include <thread>
#include <type_traits>
#include <utility>

#include "internal.h"
#include "s60.h"
#include "x_ring.h"
#include "p2p_device.h"
#include "fx48.h"

// Cache policy of the vector traffic (measured in round 2, tools/fold_ab.py, profiles/r02/fold_ab_incg_*.txt; the
// compile-time switches behind those runs are the lab build's, lab/lab_hooks.patch): the in-CG penalty of the SpMV is the
// REWRITING of its gather vector between two products, nothing else (a k_step pass in between costs
// nothing).  Rewritten by plain stores the following product ran 1.5 / 1.6 / 2.7 / 3.9 / 11 %
// slower than back to back on five boxes; by non-temporal stores (no load of the line before)
// 1.0 / 1.1 / 1.1 / 1.0 %; non-temporal stores followed by one streaming read of the vector: 0 %
// (but that read costs what it saves).  Agent- / system-scope (write-through) stores: like plain.
// k_update is a read-modify-write of p: a non-temporal store to a line its own plain load has just
// brought into L2 changes nothing, non-temporal loads AND stores recover a part (0.2 % where the
// penalty is 1.6 %).  That is what STAN_OPT_VEC_STORE_NT selects; it never costs anything.
// Writing the new p into the OTHER of two buffers (no line of it in any cache) was tried as well:
// +1.2 % against +1.3 % for the in-place form with non-temporal loads and stores: not built.
// (STAN_OPT_VEC_STORE_NT: bit 0 = k_update stores p non-temporally, bit 1 = k_step stores r so.)
// The vector kernels' own loads -- operands a kernel only reads (v in k_step; r, x in k_update) and operands it rewrites
// in place (r in k_step, p in k_update) -- and the products' stores of y are non-temporal too.

namespace {

#include "cg_reduce_device.inc"   // grid constants, scalar / status slots, block sums, the folded reductions, stopped()

#include "cg_setup_kernels.inc"   // scaling (k_diag_scale, k_diag_get, k_scale_matrix), k_init / k_init_b / k_reduce / k_init_scalars

#include "spmv_kernels.inc"   // the products: k_spmv (one wavefront per slice), k_spmv_small (one workgroup per slice), k_spmv2 (two right-hand sides), k_spmv_fold (folded rows)

#include "cg_vector_kernels.inc"   // the vector kernels of the CG loop: k_step, k_refresh, k_update, k_vec_sr (single-reduction form), result / expand / compress

#include "cg_multi.inc"   // the batched loop (several load cases, one pass over K): k_spmm and the M-column forms of k_init / k_step / k_refresh / k_update / k_result

inline unsigned vec_grid(int64_t n) {
    int64_t b = (n + VEC_T - 1) / VEC_T;
    if (b < 1) b = 1;
    return (unsigned)(b > VEC_BLOCKS ? VEC_BLOCKS : b);
}

// the one-block reduction of np blocks' partial sums (k_reduce), nv = 1 or 2 sums each
inline void launch_reduce(hipStream_t stream, int nv, const double *partial, int np, double *out, p2p_out po, const int64_t *st, int64_t k) {
    if (nv == 2) hipLaunchKernelGGL(k_reduce<2>, dim3(1), dim3(256), 0, stream, partial, np, out, po, st, k);
    else hipLaunchKernelGGL(k_reduce<1>, dim3(1), dim3(256), 0, stream, partial, np, out, po, st, k);
}

// Timed spans of a stream: an event before and one behind each, recorded only when the context profiles; k is the
// iteration a span belongs to.  drain() adds up the spans of iterations <= max_k (those it could measure) and forgets all.
struct span_list {
    const stan_ctx *ctx;
    event_bag *bag;
    std::vector<hipEvent_t> ev;
    std::vector<int64_t> its;
    void mark(hipStream_t s) { ev.push_back(bag->make()); hipEventRecord(ev.back(), s); }
    void begin(hipStream_t s, int64_t k = 0) { if (ctx->profiling) { mark(s); its.push_back(k); } }
    void end(hipStream_t s) { if (ctx->profiling) mark(s); }
    void drain(int64_t max_k, double *ms, int64_t *n) {
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float t = 0;
            if (its[i / 2] <= max_k && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) { *ms += t; (*n)++; }
        }
        ev.clear(); its.clear();
    }
};

// The status polls of a loop that enqueues its iterations in chunks, ahead of the device: behind every chunk the status
// words are copied into one of two pinned slots and an event is recorded; the host then waits for the PREVIOUS chunk's event
// and shows that chunk's words to `stopped` -- one chunk is always queued while the host looks at the one before.
struct chunk_poll {
    static constexpr int64_t hard_cap = 0x7fffffff;   // iteration counter is int32 in the report
    hipEvent_t ev[2] = {nullptr, nullptr};
    int64_t *slot[2] = {nullptr, nullptr};            // pinned
    int chunk_id = 0;
    void setup(event_bag &events, int64_t *pinned, size_t stride) {
        for (int i = 0; i < 2; i++) { ev[i] = events.make(hipEventDisableTiming); slot[i] = pinned + stride * i; }
    }
    // behind a chunk; k: the iteration the next chunk starts with.  wait(event) is the loop's way of waiting on the host.
    template <typename WAIT, typename STOPPED>
    int poll(stan_ctx *ctx, hipStream_t st, const int64_t *status, size_t words, int64_t k, WAIT wait, STOPPED stopped, bool *done) {
        HIPCHK(ctx, hipMemcpyAsync(slot[chunk_id & 1], status, words * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipEventRecord(ev[chunk_id & 1], st));
        if (chunk_id > 0) {
            STANCHK(wait(ev[(chunk_id - 1) & 1]));
            if (stopped(slot[(chunk_id - 1) & 1])) *done = true;
        }
        if (k >= hard_cap) *done = true;
        chunk_id++;
        return STAN_OK;
    }
};

// STAN_OPT_VALUE_STREAM_60 = -1 takes the 60-bit stream above this many block rows -- the small-system kernel's DEFAULT bound,
// whatever STAN_OPT_SPMV_SMALL is set to: a matrix below it lives in the caches and gains nothing from fewer bytes
constexpr int64_t STREAM60_AUTO_ROWS = 150000;

// Which kernel reads which stream of K: filled by plan_products; what a solve learns later enters through the named steps below
struct product_plan {
    // the kernel of a PLAIN product (one right-hand side, not a matrix's first): one workgroup per slice (k_spmv_small), two
    // wavefronts per slice (k_spmv_pair; STAN_OPT_SPMV_VARIANT 20), or one wavefront per slice: k_spmv -- k_spmv_fold where
    // `folding` finds a folded block.  The other products (k_spmv2, k_spmv_first) are wave kernels whatever the form.
    enum { SMALL, PAIR, WAVE } form = WAVE;
    int forced_var = -1;      // k_spmv's VAR of the WAVE form; -1: per stream (var())
    bool folding = false;     // a product of K's own stream of a kind reads the folded block of that kind, where K has one (fold.hip)
    int spb = 4;              // slices per workgroup of a plain product; every other product: 4
    unsigned blocks = 0;      // workgroups of a whole-matrix launch in that form, the most of any form: sizes the partial sums
    int vs = STAN_PREC_FP64;  // the stream the loop's products read on THIS rank (FIXED-48 falls back to fp64 on a rank that owns no
                              // rows or whose shard is not representable: never a base for decisions the ranks must share)
    bool may_lazy_scale = false;   // the loop's first product may scale the matrix on its way (k_spmv_first)
    bool stream60 = false;    // the plain p.Ap products of the fp64 loop read the lossless 60-bit stream (the same bits)
    bool folded = false;      // the loop's stream has a folded block (what the profile reports as repacked) ...
    const stan_colpack *cols = nullptr;   // ... and then the folded layout's packed columns and slots are what the profile's bytes count
    int64_t slots = 0;
    // auto (-1): non-temporal matrix stream + XCD-chunked workgroup mapping (variant 9), with the
    // loop unrolled by 4 for the FIXED-48 stream, whose iterations carry 21 % fewer bytes in
    // flight (variant 12).  One process, one box (tools/fx48_variants.py, min of 3 x 20 launches):
    // fp64 plain 1.181 / nt 1.102 / nt+chunk 1.100 ms; FIXED-48 1.003 / 0.955 / nt+unroll4 0.925;
    // fp32 0.636 / 0.583 / 0.580.
    int var(bool fx) const { return forced_var >= 0 ? forced_var : fx ? 12 : 9; }
    // behind the planning pass of fold.hip (K->fold_state decided, no value touched): a folded copy is made from the SCALED values
    void fold_planned(const stan_matrix *K) { may_lazy_scale = may_lazy_scale && !(folding && K->fold_state == 1); }
    // behind stan_matrix_make_fx48: the FIXED-48 encoder refuses a K that is not SPD-scalable, the fp64 values serve
    void value_stream_built(const stan_matrix *K) { if (vs == STAN_PREC_FIXED48 && !K->vs[vs].padded) vs = STAN_PREC_FP64; }
    // behind the packed columns and the folded copy the solve builds: what the products will find
    void copies_built(const stan_matrix *K) {
        stream60 = stream60 && !K->vs[STAN_VALUE_STREAM_60].refused && !(folding && K->fold_state == 1);
        folded = folding && K->vs[vs].folded != nullptr;   // (whatever the form: a small system reports a copy an earlier solve left)
        cols = folded ? &K->fold_pk : &K->pk;
        slots = folded ? K->nfslots : K->nslots;
    }
    void stream60_unavailable() { stream60 = false; }   // no room for its block, or the encoder refused an entry: the fp64 values serve
};

// precision_mode: the stream the caller asks for; dist: a rank of a sharded matrix; sr: the single-reduction loop
product_plan plan_products(const stan_ctx *ctx, const stan_matrix *K, int precision_mode, bool dist, bool sr) {
    product_plan P;
    const int v = ctx->spmv_variant;
    // k_spmv_small: decided by the GLOBAL number of block rows, so that a shard and the whole matrix sum their rows in the same order
    P.form = v < 0 && K->nb_glob <= ctx->spmv_small_rows ? product_plan::SMALL : v == 20 ? product_plan::PAIR : product_plan::WAVE;
    P.forced_var = v;
    P.folding = ctx->row_folding != 0;
    P.spb = P.form == product_plan::SMALL ? 1 : P.form == product_plan::PAIR ? 2 : 4;
    P.blocks = nblk(K->nslices, P.spb);
    P.vs = precision_mode;
    const bool fp64_one_rank = precision_mode == STAN_PREC_FP64 && !dist && P.form != product_plan::SMALL && K->nslices > 0;
    // The first product of the loop may scale the matrix on its way (k_spmv_first) instead of a pass of its own: the fp64
    // stream of one rank, the large-system kernel in its default variant, no folded copy (fold_planned), a first product
    // that is a plain one (a residual refresh at iteration 1 is a two-product pass).
    P.may_lazy_scale = !K->scaled && ctx->cg_lazy_scaling && fp64_one_rank && v < 0 && ctx->cg_rupdate != 1;
    // The lossless 60-bit stream (s60.h) for the plain products of the classic fp64 loop on one rank, where k_spmv runs them
    // on the padded streams: not the small-system kernel, the pair kernel, the folded copy (copies_built) or the
    // single-reduction loop's DOT = 2 products (they keep the fp64 values, as do k_spmv_first and k_spmv2: the bits are the
    // same either way).  -1 (auto) also wants more than STREAM60_AUTO_ROWS block rows.
    P.stream60 = ctx->value_stream_60 != 0 && fp64_one_rank && !sr && (v < 0 || v == 9 || v == 12) &&
                 (ctx->value_stream_60 > 0 || K->nb_glob > STREAM60_AUTO_ROWS);
    return P;
}

inline colstream colstream_of(const stan_ctx *ctx, const stan_colpack &c, int64_t nslots) {
    return ctx->cols16 && c.cols16 ? make_colstream(c, nslots) : NO_COLSTREAM;
}

// One product, as it is enqueued: y = A x with `dot` sums (k_spmv's DOT), or -- x2 given, dot = 1 -- y = A x and
// y2 = A x2 in one pass over the matrix.
struct product_args {
    const double *x;
    double *y;
    const double *x2;
    double *y2;
    int dot;
    double *partial;
    const int64_t *st;
    int64_t k;
    int kind;           // the value stream (STAN_PREC_*)
    const void *vals;   // nullptr: K's own stream of that kind
    bool vals_folded;   // `vals` is a block for a FOLDED stream (the placement search of fold.hip times its candidates)
    bool first;         // the first product of an unscaled fp64 matrix scales it on the way (k_spmv_first)
};
// the run-time choices of a product -- value stream and DOT -- as the types of f's arguments
template <typename F>
void with_product_types(const stan_matrix *K, const product_args &a, F f) {
    auto by_dot = [&](auto *vals) {
        if (a.dot == 2) f(vals, std::integral_constant<int, 2>());
        else if (a.dot == 1) f(vals, std::integral_constant<int, 1>());
        else f(vals, std::integral_constant<int, 0>());
    };
    const void *vals = a.vals ? a.vals : K->vs[a.kind].padded;
    if (a.kind == STAN_PREC_MIXED) by_dot((const float *)vals);
    else if (a.kind == STAN_PREC_FIXED48) by_dot((const uint32_t *)vals);
    else by_dot((const double *)vals);
}
// the folded form of the value stream `vals` of K, if the product is to read it (fold.hip)
template <typename VT>
const VT *fold_vals(const product_plan &P, const stan_matrix *K, const product_args &a, const VT *vals) {
    if (a.vals_folded) return vals;
    const stan_value_stream &s = K->vs[a.kind];
    return P.folding && (const void *)vals == s.padded ? (const VT *)s.folded : nullptr;
}
// which: 0 = all slices, 1 = interior list, 2 = boundary list (partials offset by the
// interior launch's block count).  Returns the number of partial slots this launch writes.
// `fold`: counter/out of the folded reduction (counter == nullptr: partials only); nblocks and np
// are filled in here (np = this launch's slots + poff: the boundary launch of a split product
// also adds up what the interior launch left).
unsigned launch_product(stan_ctx *ctx, stan_matrix *K, const product_plan &P, const product_args &a, int which = 0,
                        hipStream_t stream = nullptr, fold_args fold = NO_FOLD) {
    if (!stream) stream = ctx->stream;
    const int32_t *slist = which == 1 ? K->d_sl_int : which == 2 ? K->d_sl_bnd : nullptr;
    const int32_t nlist = which == 1 ? K->n_sl_int : which == 2 ? K->n_sl_bnd : K->nslices;
    // the plan's form and slices per workgroup for a single product that is not a matrix's first, k_spmv's for every other
    // (the lossless 60-bit stream belongs to k_spmv alone: the plan picks it only where that kernel would run)
    const bool s60 = a.kind == STAN_VALUE_STREAM_60;
    const bool plain = !a.x2 && !a.first && !s60, small = plain && P.form == product_plan::SMALL, pair = plain && P.form == product_plan::PAIR;
    const int spb = plain ? P.spb : 4;
    const int32_t poff = which == 2 ? (int32_t)nblk(K->n_sl_int, spb) : 0;
    const unsigned grid = nblk(nlist, spb);
    if (grid == 0) return 0;
    fold.nblocks = grid;
    fold.np = (int)grid + poff;
    const colstream cs = colstream_of(ctx, K->pk, K->nslots);
    if (s60) {   // one plain product with its p.Ap sum: k_spmv<s60_t, 1, 9 | 12>, or the fused refresh pass: k_spmv2<s60_t>; nothing else is instantiated for this stream
        const s60_t *vals = (const s60_t *)(a.vals ? a.vals : K->vs[a.kind].padded);
        if (a.x2) {
            hipLaunchKernelGGL((k_spmv2<s60_t>), dim3(grid), dim3(256), 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof, K->d_cols,
                               vals, a.x, a.x2, a.y, a.y2, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);
            return grid;
        }
        auto launch = [&](auto var) {
            hipLaunchKernelGGL((k_spmv<s60_t, 1, decltype(var)::value>), dim3(grid), dim3(256), 0, stream, K->nslices, K->nloc, K->d_slot_ptr,
                               K->d_rowof, K->d_cols, vals, a.x, a.y, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);
        };
        if (P.var(false) == 12) launch(std::integral_constant<int, 12>());
        else launch(std::integral_constant<int, 9>());
        return grid;
    }
    with_product_types(K, a, [&](auto *vals, auto dot_tag) {
        using VT = std::remove_cv_t<std::remove_pointer_t<decltype(vals)>>;
        constexpr int DOT = decltype(dot_tag)::value;
        const dim3 g(grid), b(256);
        const VT *fv = small || pair || a.first ? nullptr : fold_vals(P, K, a, vals);
        const colstream fcs = colstream_of(ctx, K->fold_pk, K->nfslots);
        if constexpr (std::is_same_v<VT, double>)
            if (a.first) {
                hipLaunchKernelGGL(k_spmv_first<DOT>, g, b, 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof, K->d_cols,
                                   K->vals64(), K->d_scale, a.x, a.y, a.partial, a.st, a.k, fold, cs);
                return;
            }
        if constexpr (DOT == 1)
            if (a.x2) {
                if (fv)
                    hipLaunchKernelGGL((k_spmv_fold<VT, 1, 2>), g, b, 0, stream, K->nslices, K->nloc, K->d_fold_ptr, K->d_rowof,
                                       K->d_fold_meta, K->d_fold_cols, fv, a.x, a.x2, a.y, a.y2, a.partial, a.st, a.k, slist, nlist,
                                       poff, fold, fcs);
                else
                    hipLaunchKernelGGL((k_spmv2<VT>), g, b, 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof, K->d_cols,
                                       vals, a.x, a.x2, a.y, a.y2, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);
                return;
            }
        if (small) {   // one workgroup per slice; partials per slice
            hipLaunchKernelGGL((k_spmv_small<VT, DOT>), g, b, 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                               K->d_cols, vals, a.x, a.y, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);
            return;
        }
        if (pair) {   // two wavefronts per slice, two slices per workgroup
            hipLaunchKernelGGL((k_spmv_pair<VT, DOT, true>), g, b, 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                               K->d_cols, vals, a.x, a.y, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);
            return;
        }
        if (fv) {
            hipLaunchKernelGGL((k_spmv_fold<VT, DOT, 1>), g, b, 0, stream, K->nslices, K->nloc, K->d_fold_ptr, K->d_rowof,
                               K->d_fold_meta, K->d_fold_cols, fv, a.x, (const double *)nullptr, a.y, (double *)nullptr, a.partial,
                               a.st, a.k, slist, nlist, poff, fold, fcs);
            return;
        }
#define SPMV_CASE(V)                                                                                                          \
    case V:                                                                                                                   \
        hipLaunchKernelGGL((k_spmv<VT, DOT, V>), g, b, 0, stream, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof, K->d_cols, \
                           vals, a.x, a.y, a.partial, a.st, a.k, slist, nlist, poff, fold, cs);                               \
        break;
        switch (P.var(vstream<VT>::FX)) {
            SPMV_CASE(9) SPMV_CASE(12)
            default:
            SPMV_CASE(0)
        }
#undef SPMV_CASE
    });
    return grid;
}

}  // namespace

// Diagonal scaling of the matrix (once per matrix): A^ = S K S.  First the vector s (ensure_scale_vector), then the values:
// by a pass of its own (ensure_scaled), or -- the fp64 loop on one rank -- by the loop's first product (k_spmv_first,
// cg_run::iterate), which marks the matrix scaled itself.
static int ensure_scale_vector(stan_ctx *ctx, stan_matrix *K) {
    const int64_t npad = (int64_t)K->nslices * 64;
    const int64_t ns = 3 * (npad + K->nhalo);
    if (!K->d_scale) STANCHK(stan_dmalloc(ctx, &K->d_scale, (size_t)ns));
    hipLaunchKernelGGL(k_fill, dim3(vec_grid(ns)), dim3(VEC_T), 0, ctx->stream, K->d_scale, ns, 1.0);
    if (K->nloc > 0)
        hipLaunchKernelGGL(k_diag_scale, dim3(nblk(K->nloc, 256)), dim3(256), 0, ctx->stream, K->nloc,
                           K->d_rowlen, K->d_posof, K->d_slot_ptr, K->d_cols, K->vals64(), K->d_scale);
    if (stan_sharded(ctx)) {
        if (ctx->comm_p2p && ctx->p2p) {
            // Peer to peer, my neighbours write their rows straight into my halo region, which the k_fill above
            // has just initialised: nobody may write before everybody has done that.  One empty reduction
            // (every rank counts itself into every rank's counter, every stream waits for all) orders it; the
            // exchanges inside the CG are ordered by the loop's own reductions.  (Found with the ranks in
            // separate processes, where mapping the peers' vectors delays some ranks by milliseconds: a
            // neighbour's scaling factors arrived before the fill and were overwritten with 1.0.)
            const p2p_out po{stan_p2p_table(ctx), stan_p2p_reduce_slot(ctx), 3, 1};
            launch_reduce(ctx->stream, 1, nullptr, 0, nullptr, po, nullptr, 0);
            STANCHK(stan_p2p_reduce_wait(ctx));
        }
        STANCHK(stan_comm_halo_exchange(ctx, K, K->d_scale));
    }
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
// what changes for the rest of the library once the values carry S K S
static void mark_scaled(stan_ctx *ctx, stan_matrix *K) {
    K->scaled = true;
    // copies of the value stream made before the scaling (stan_hip_spmv_bench on a fresh matrix)
    // hold the unscaled K: a later solve must not iterate on them
    for (int kind = STAN_PREC_FP64 + 1; kind < STAN_NSTREAMS; kind++) {
        stan_dfree(ctx, K->vs[kind].padded);
        K->vs[kind].padded = nullptr;
        K->vs[kind].refused = false;
    }
    stan_matrix_drop_folded_values(ctx, K);
}
static int ensure_scaled(stan_ctx *ctx, stan_matrix *K) {
    if (K->scaled) return STAN_OK;
    STANCHK(ensure_scale_vector(ctx, K));
    if (K->nslices > 0)
        hipLaunchKernelGGL(k_scale_matrix, dim3(nblk(K->nslices, 4)), dim3(256), 0, ctx->stream,
                           K->nslices, K->d_slot_ptr, K->d_rowof, K->d_cols, K->vals64(), K->d_scale);
    HIPCHK(ctx, hipGetLastError());
    mark_scaled(ctx, K);
    return STAN_OK;
}

// the matrix carries S K S from its first solve on -- or from its first export: stan_hip_matrix_to_csr divides the
// scaled values on the way out, whether or not a solve has happened, so an export before a solve and one after it are
// the same bits (rounds 1-4 un-scaled the values in place for an export and re-scaled them for the next solve)
int stan_matrix_ensure_scaled(stan_ctx *ctx, stan_matrix *K) { return ensure_scaled(ctx, K); }

// NOTE on the halo layout: vectors that are gathered by the SpMV (p, x) hold the owned
// block rows first, padded to whole slices, then the halo block columns:
//   [ 3*nslices*64 owned+pad | 3*nhalo ]
// Local column indices >= nloc written by the symbolic phase are relative to nloc, so
// the halo region must start at 3*nloc: the pad only exists for nranks == 1 tails, where
// nhalo == 0.  For nranks > 1 every rank's row count is a multiple of 64 except the last
// rank's; the gather vectors are therefore sized 3*(max(nloc, pad) + nhalo) and the halo
// always sits at 3*nloc.
// Host waits of the loop.  Without peer-to-peer exchanges: the plain blocking calls.  With them the stream may sit in a
// wait for a peer that is gone, and a blocking call would never return (the polling wavefront keeps the queue busy):
// the host polls instead, and after stan_p2p_stall_seconds() without completion releases this rank's waits
// (stan_p2p_release_own), lets the queue drain and reports STAN_E_COMM.  `ev` == nullptr: the whole stream.
static int cg_wait(stan_ctx *ctx, bool p2p, hipStream_t st, hipEvent_t ev) {
    if (!p2p) {
        if (ev) HIPCHK(ctx, hipEventSynchronize(ev));
        else HIPCHK(ctx, hipStreamSynchronize(st));
        return STAN_OK;
    }
    const double bound = stan_p2p_stall_seconds();
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    for (;;) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(st);
        if (e == hipSuccess) return STAN_OK;
        if (e != hipErrorNotReady) { ctx->err = std::string("cg: ") + hipGetErrorString(e); (void)hipGetLastError(); return STAN_E_HIP; }
        (void)hipGetLastError();
        if (++spins > 200) std::this_thread::sleep_for(std::chrono::microseconds(spins > 2000 ? 500 : 50));
        if (ctx->p2p->broken.load()) break;   // somebody else (run_all, another rank's release) gave up already
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > bound) break;
    }
    stan_p2p_release_own(ctx);
    (void)hipStreamSynchronize(st);   // the released waits pass: what was enqueued runs out
    (void)hipGetLastError();
    ctx->err = "cg: peer-to-peer exchange made no progress (a peer rank failed or never arrived); this rank's waits were released";
    return STAN_E_COMM;
}

namespace {

// ---- one solve -------------------------------------------------------------------------------------------
// cg_run holds the state of ONE call of stan_cg_device and is its three parts:
//   setup()    streams and vectors: workspace, scaling, packed columns, value streams, scalars, counters
//   pass()     ONE run of the CG loop on the right-hand side in bh (begin_pass: k_init / k_init_b, first
//              residual test; iterate: chunks of iterations enqueued ahead of a polled status word)
//   finish()   U = S x^, the report, the profile
// and, for the reduced-precision value streams (STAN_PREC_MIXED, STAN_PREC_FIXED48), what lies between two passes:
//   fp64_check()   r_t = b^ - A^64 x^ with the fp64 values (which stay resident next to their copy): the residual
//                  the caller gets REPORTED, and the right-hand side of the next pass when it misses eps
//                  (STAN_OPT_CG_REFINE: iterative refinement; the passes' iterates add up in fp64).
// The fp64 stream makes exactly one pass and no check: alglib's loop as the reference runs it.
struct cg_run {
    stan_ctx *ctx;
    stan_matrix *K;
    const double *d_F;
    double eps_f;
    int32_t max_its;
    int32_t precision_mode;
    double *d_U;

    hipStream_t st_ = nullptr;
    event_bag events;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool dist = false, p2p = false, sr = false, foldr = false, split = false;
    product_plan plan;                // which kernel reads which stream in this solve
    bool lazy_scale = false;          // the values are still K: the loop's first product scales them (k_spmv_first)
    bool reduced = false;             // the caller asked for a reduced-precision stream: fp64 check + refinement (every rank alike)
    uint32_t *pend60 = nullptr;       // the block of plan.stream60, allocated in setup() (the placement search needs the vectors idle); encoded -- and
                                      // handed to K -- in front of the first product that finds the values scaled (product())
    int64_t n60 = 0;                  // plain products enqueued on it
    bool refresh60 = false;           // STAN_OPT_CG_REFRESH_60: where the plain products read that stream the fused refresh passes do too (k_spmv2<s60_t>)
    int refresh_stream = -1;          // the stream the last fused refresh pass read (-1: none ran)
    // STAN_OPT_CG_X_RING (x_ring.h): W + 1 gather-length slots for the directions p_k (slot k mod (W + 1)) and as many doubles for
    // the alphas, taken per solve in setup(); ring_w = 0: the loop as ever (x' formed by k_update every iteration)
    int ring_w = 0;
    double *ring = nullptr, *ring_alpha = nullptr;
    int64_t ring_flushed = 0, n_flush = 0;   // the last term the enqueued flushes cover; flush launches
    double *ring_slot(int64_t j) const { return ring + (int64_t)xring_slot(j, ring_w) * ng; }
    ~cg_run() { if (pend60) stan_dfree(ctx, pend60); }
    int refine = 0;                   // STAN_OPT_CG_REFINE, reduced-precision modes only
    int64_t n3 = 0, npad = 0, ng = 0, dof0 = 0;
    dev_scope bufs{ctx};
    double *xb[2] = {nullptr, nullptr}, *p = nullptr, *r = nullptr, *v = nullptr, *w = nullptr, *bh = nullptr;
    double *partial = nullptr, *sc = nullptr, *sv = nullptr;
    double *xacc = nullptr, *b0 = nullptr;   // refinement: the sum of the passes' iterates, the original b^ (allocated when a second pass starts)
    int64_t *stt = nullptr;
    unsigned long long *tick = nullptr;
    const stan_p2p_dev *p2p_tab = nullptr;
    unsigned vg = 1;
    int64_t its_before_restart = 1;
    int64_t *h_st = nullptr;          // pinned status words
    double *h_sc = nullptr;           // pinned copy of the scalars
    chunk_poll poll;
    // profile: reductions' and halos' exchanges, the products (one right-hand side, two, the fp64 products of a reduced-precision solve)
    span_list red_sp{ctx, &events}, halo_sp{ctx, &events}, spmv_sp{ctx, &events}, spmv2_sp{ctx, &events}, spmv64_sp{ctx, &events};
    int64_t n_coll = 0, n_wait = 0, n_launch = 0, n_enqueued = 0;
    double prof_spmv_ms = 0, prof_spmv2_ms = 0, prof_spmv64_ms = 0;
    int64_t prof_spmv_n = 0, prof_spmv2_n = 0, prof_spmv64_n = 0;
    // result of the last pass
    int pass_type = 0;
    int64_t pass_its = 0;
    const double *xfin = nullptr;

    // Where the sums of a reduction go.  One rank, or RCCL: the local scalars (RCCL all-reduces them in
    // place).  Peer to peer: every rank's mailbox slot `slot`, columns j0.. (+ arrival count when this is
    // the producer that completes the exchange); the consumers then read through a red_src.
    p2p_out p2p_to(int j0, bool signal) {
        return p2p ? p2p_out{p2p_tab, stan_p2p_reduce_slot(ctx), j0, signal ? 1 : 0} : NO_P2P;
    }
    // folded reductions: counter set 0 serves the products, set 1 the vector kernels
    fold_args fold_to(int which, double *out, p2p_out po = NO_P2P) {
        return fold_args{foldr ? tick + FOLD_WORDS * which : nullptr, 0, 0, out, po};
    }
    fold_args vec_fold(double *out, p2p_out po = NO_P2P) {
        fold_args f = fold_to(1, out, po);
        f.nblocks = vg; f.np = (int)vg;
        return f;
    }
    void reduce_if_unfolded(int np, int nv, double *out, p2p_out po = NO_P2P, int64_t k_ = -1) {
        if (foldr || np <= 0) return;
        const int64_t *sk = k_ >= 1 ? stt : nullptr;   // (k_init's sum is formed before the status exists)
        launch_reduce(st_, nv, partial, np, out, po, sk, k_);
    }
    // One exchange point of the sharded loop: RCCL all-reduce of `count` scalars in place, or the stream
    // wait for every rank's arrival; returns where the consumers find the sums.
    int exchange_sums(double *scalars, int count, red_src *rs) {
        *rs = red_src{nullptr, 0, nullptr, 0};
        if (!dist) return STAN_OK;
        red_sp.begin(st_);
        int rc_ = STAN_OK;
        if (p2p) {
            *rs = red_src{stan_p2p_mailbox(ctx, stan_p2p_reduce_slot(ctx)), ctx->nranks, nullptr, 0};
            rc_ = stan_p2p_reduce_wait(ctx, &rs->ctr, &rs->want);   // (wait mode 2: the consumers poll rs->ctr themselves)
            if (!rs->ctr) n_wait++;
        } else {
            rc_ = stan_comm_allreduce_sum_f64(ctx, scalars, (size_t)count);
            n_coll++;
        }
        red_sp.end(st_);
        return rc_;
    }
    int halo(double *x) {
        halo_sp.begin(st_);
        const int rc_ = stan_comm_halo_exchange(ctx, K, x);
        if (p2p && !K->nbr.empty()) n_wait++;
        halo_sp.end(st_);
        return rc_;
    }

    // y = A^ x with `dot` sums (k_spmv's DOT) reduced into out[0..dot) -- or, x2 given and dot = 1, y = A^ x and w = A^ x2
    // in one matrix pass (the fused residual refresh).  x and x2 get their halos filled first when sharded; the sums are
    // folded into the last launch of the product, or formed by k_reduce.  kind: the value stream (the loop's own, or
    // STAN_PREC_FP64 for the check / refresh products of a reduced-precision solve, `extra`: timed apart).
    int product(double *x, double *x2, double *y, int dot, double *out, int64_t k, p2p_out po, int kind, bool extra = false) {
        span_list &span = extra ? spmv64_sp : x2 ? spmv2_sp : spmv_sp;
        if (pend60 && K->scaled) {   // the scaled values -> the 60-bit stream, K's from now on; waits for the encoder's count (the host is a few kernels ahead)
            const int rc = stan_matrix_encode_s60(ctx, K, std::exchange(pend60, nullptr));
            if (!K->vs[STAN_VALUE_STREAM_60].padded) plan.stream60_unavailable();
            STANCHK(rc);
        }
        // the plain products, and -- STAN_OPT_CG_REFRESH_60 -- the fused refresh passes too: then no product inside the loop reads the fp64 block
        const bool s60 = plan.stream60 && !pend60 && (!x2 || refresh60) && dot == 1 && !extra && !lazy_scale && kind == STAN_PREC_FP64;
        if (s60) { kind = STAN_VALUE_STREAM_60; if (!x2) n60++; }
        if (x2) refresh_stream = kind;
        span.begin(st_, k);
        auto go = [&](int which, hipStream_t s, bool last) -> unsigned {
            n_launch++;
            // lazy_scale: the first product of this matrix (one rank, fp64 stream, all slices) scales it on the way
            const product_args a{x, y, x2, x2 ? w : nullptr, dot, partial, stt, k, kind, nullptr, false, lazy_scale};
            const unsigned blocks = launch_product(ctx, K, plan, a, which, s, (dot && last) ? fold_to(0, out, po) : NO_FOLD);
            if (lazy_scale) { lazy_scale = false; mark_scaled(ctx, K); }
            return blocks;
        };
        unsigned parts = 0;
        bool folded = foldr;
        if (split) {
            HIPCHK(ctx, hipEventRecord(ctx->ev_a, st_));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_a, 0));
            parts = go(1, ctx->side, false);
            HIPCHK(ctx, hipEventRecord(ctx->ev_b, ctx->side));
            STANCHK(halo(x));
            if (x2) STANCHK(halo(x2));
            HIPCHK(ctx, hipStreamWaitEvent(st_, ctx->ev_b, 0));
            const unsigned pb = go(2, st_, true);   // adds up the interior launch's partials too
            if (pb == 0) folded = false;            // no boundary slices on this rank: nobody folded
            parts += pb;
        } else {
            if (dist) { STANCHK(halo(x)); if (x2) STANCHK(halo(x2)); }
            parts = go(0, st_, true);
            if (parts == 0) folded = false;
        }
        if (dot && !folded) {
            if (parts > 0 || po.pp) {   // (peer to peer: a rank that owns no rows still sends its zeros)
                launch_reduce(st_, dot, partial, (int)parts, out, po, k >= 1 ? stt : nullptr, k);
                n_launch++;
            } else HIPCHK(ctx, hipMemsetAsync(out, 0, 8 * dot, st_));   // a rank that owns no rows
        }
        span.end(st_);
        return STAN_OK;
    }

    int setup();
    int setup_x_ring();
    void flush_x_ring(int64_t k, int64_t last_enqueued);
    int begin_pass(bool from_F, double eps_pass, bool *done);
    int iterate(double eps_pass, int32_t max_its_pass);
    int pass(bool from_F, double eps_pass, int32_t max_its_pass);
    void account_pass();
    int fp64_check(double *xg, const double *b, double *r2_out);
    int finish(const double *x_result, int type, int64_t its, double rel_rec, double rel64, int passes,
               int32_t *term_out, int32_t *iters_out, double *rel_res_out);
};

// ---- set-up ------------------------------------------------------------------------------------------------
int cg_run::setup() {
    st_ = ctx->stream;
    if (ctx->profiling) {
        ev0 = events.make(); ev1 = events.make();
        hipEventRecord(ev0, st_);
    }
    dist = stan_sharded(ctx);  // exchanges in the loop
    // peer to peer (one-process group handle, STAN_OPT_COMM_P2P): no RCCL call below this line
    p2p = dist && ctx->comm_p2p && ctx->p2p != nullptr;
    if (p2p && ctx->p2p->broken.load()) {   // refused at once: not another collective with a peer that is gone
        ctx->err = "cg: the peer-to-peer exchange of this context is broken (a peer rank failed earlier); start a fresh process";
        return STAN_E_COMM;
    }
    // no hipFree while the peers' streams wait for this rank's future exchanges (stan_ctx::defer_frees): peer to peer, and
    // any transport when ranks of this process share the device
    if (p2p || (dist && ctx->peers_share_device)) ctx->defer_frees = true;
    STANCHK(stan_cg_workspace(ctx, K));   // the context's vectors (the placement search probed with them)
    if (p2p) {
        // my neighbours write their boundary rows straight into these vectors: tell them where they are
        const int64_t ns_ = 3 * ((int64_t)K->nslices * 64 + K->nhalo);
        if (!K->d_scale) STANCHK(stan_dmalloc(ctx, &K->d_scale, (size_t)ns_));
        double *const pub[5] = {ctx->ws.xb[0], ctx->ws.xb[1], ctx->ws.p, ctx->ws.r, K->d_scale};
        STANCHK(stan_p2p_publish_vectors(ctx, K, pub));
    }
    sr = ctx->cg_single_reduce;
    foldr = ctx->cg_fold_reduce;
    plan = plan_products(ctx, K, precision_mode, dist, sr);
    auto folded_copy = [&](int kind, bool plan_only) {   // an optimisation must not fail the solve: without memory the padded streams serve
        const int rc = stan_matrix_make_folded(ctx, K, kind, plan_only);
        if (rc == STAN_E_ALLOC) { stan_matrix_abandon_folding(ctx, K); ctx->err.clear(); }
        return rc == STAN_E_ALLOC ? (int)STAN_OK : rc;
    };
    if (plan.may_lazy_scale) {
        STANCHK(folded_copy(STAN_PREC_FP64, true));   // (decides K->fold_state, touches no value)
        plan.fold_planned(K);
    }
    refresh60 = ctx->cg_refresh_60 > 0 || (ctx->cg_refresh_60 < 0 && K->nb_glob > STREAM60_AUTO_ROWS);
    lazy_scale = plan.may_lazy_scale;
    if (lazy_scale) STANCHK(ensure_scale_vector(ctx, K));
    else STANCHK(ensure_scaled(ctx, K));
    if (ctx->cols16) STANCHK(stan_matrix_make_cols16(ctx, K));
    if (precision_mode == STAN_PREC_MIXED) STANCHK(stan_matrix_make_fp32(ctx, K));
    if (precision_mode == STAN_PREC_FIXED48) STANCHK(stan_matrix_make_fx48(ctx, K));
    reduced = precision_mode != STAN_PREC_FP64;
    refine = reduced ? ctx->cg_refine : 0;
    plan.value_stream_built(K);
    if (plan.form != product_plan::SMALL) STANCHK(folded_copy(plan.vs, false));
    plan.copies_built(K);
    // The block of the 60-bit stream must fit the pool budget and leave a floor of free memory (stan_matrix_alloc_s60
    // decides before it allocates); no room: fp64, and the profile's value_stream says so.
    if (plan.stream60 && !K->vs[STAN_VALUE_STREAM_60].padded) {   // (decided per solve: a matrix without room now may have it at its next solve)
        STANCHK(stan_matrix_alloc_s60(ctx, K, &pend60));
        if (!pend60) plan.stream60_unavailable();
    }

    n3 = 3 * K->nloc;
    npad = (int64_t)K->nslices * 64;
    ng = gather_len(K);
    dof0 = 3 * K->r0;
    xb[0] = ctx->ws.xb[0]; xb[1] = ctx->ws.xb[1]; p = ctx->ws.p; r = ctx->ws.r;
    v = ctx->ws.v; w = ctx->ws.w; bh = ctx->ws.bh;
    if (sr) sv = ctx->ws.sv;
    const size_t npart = 2 * (size_t)(plan.blocks > VEC_BLOCKS ? plan.blocks : VEC_BLOCKS) + 16;
    STANCHK(bufs.alloc(&partial, npart));
    STANCHK(bufs.alloc(&sc, (size_t)S_NSCAL));
    STANCHK(bufs.alloc(&stt, (size_t)T_NSTAT));
    STANCHK(bufs.alloc(&tick, (size_t)(2 * FOLD_WORDS)));   // two ticket-counter sets
    HIPCHK(ctx, hipMemsetAsync(sc, 0, S_NSCAL * 8, st_));
    HIPCHK(ctx, hipMemsetAsync(tick, 0, 2 * FOLD_WORDS * 8, st_));
    HIPCHK(ctx, hipMemsetAsync(xb[0], 0, (size_t)ng * 8, st_));
    HIPCHK(ctx, hipMemsetAsync(xb[1], 0, (size_t)ng * 8, st_));
    HIPCHK(ctx, hipMemsetAsync(p, 0, (size_t)ng * 8, st_));
    if (sr) {
        HIPCHK(ctx, hipMemsetAsync(r, 0, (size_t)ng * 8, st_));
        HIPCHK(ctx, hipMemsetAsync(sv, 0, (size_t)n3 * 8, st_));
    }
    p2p_tab = p2p ? stan_p2p_table(ctx) : nullptr;
    vg = vec_grid(n3);
    its_before_restart = K->n_red > 0 ? K->n_red : 1;   // lincgcreate: ItsBeforeRestart = N (global reduced size)
    STANCHK(setup_x_ring());
    // Sharded SpMV with the halo exchange hidden behind the interior slices: the slices whose
    // rows reference no halo column run on a side stream while the main stream packs, sends
    // and receives; the boundary slices follow on the main stream.  RCCL only ever sees the
    // main stream.
    split = dist && ctx->overlap_halo && K->d_sl_bnd != nullptr;
    if (split && !ctx->side) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_a, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_b, hipEventDisableTiming));
    }
    h_st = ctx->h_status + SS_H_CG_STATUS;  // pinned
    h_sc = (double *)(ctx->h_status + SS_H_CG_SCALARS);
    poll.setup(events, h_st, 8);
    return STAN_OK;
}

// The ring of directions (STAN_OPT_CG_X_RING): where the iteration defers x today -- the classic fp64 loop of one rank, merit
// stop off, fused refresh, a refresh period other than 1 -- and, under -1, only above STREAM60_AUTO_ROWS block rows (a smaller
// system's vectors live in the caches).  The ring is an extra of the solve, W + 1 vectors beside its eight: whether there is
// room is decided before anything is allocated (a parked block that fits, or the block and as much again -- a sixteenth of
// the device at least -- free), a block that cannot be had flushes no parked one, and without it the loop runs as ever.
// ctx->ws is not touched: the products write v and w where the placement search left them.
int cg_run::setup_x_ring() {
    ring_w = 0;
    ctx->prof_x_ring_window = 0;
    ctx->prof_x_ring_flushes = 0;
    const bool applies = precision_mode == STAN_PREC_FP64 && !dist && !sr && ctx->cg_defer_x && !ctx->cg_merit_stop &&
                         ctx->cg_fused_refresh && ctx->cg_rupdate != 1 && n3 > 0;
    if (!applies || ctx->cg_x_ring == 0 || (ctx->cg_x_ring < 0 && K->nb_glob <= STREAM60_AUTO_ROWS)) return STAN_OK;
    const int W = xring_window(ctx->cg_rupdate);
    const size_t bytes = (size_t)(W + 1) * (size_t)ng * 8;
    const stan_pool &pool = ctx->pool;
    bool room = false;
    if (pool.enabled && bytes >= stan_pool::MIN_BYTES)
        for (const stan_pool::blk &b : pool.avail) room = room || (b.cap >= bytes && b.cap <= bytes + bytes / 2);
    if (!room) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return STAN_OK; }
        room = free_b >= bytes + (bytes > total_b / 16 ? bytes : total_b / 16);
    }
    if (!room) return STAN_OK;
    void *blk = nullptr;
    if (stan_dmalloc_bytes(ctx, &blk, bytes, false) != STAN_OK) { ctx->err.clear(); return STAN_OK; }   // (fragmentation: room by the figures, no block)
    bufs.p.push_back(blk);
    ring = (double *)blk;
    STANCHK(bufs.alloc(&ring_alpha, (size_t)(W + 1)));
    ring_w = W;
    // the pad behind the owned rows is gathered like everything else: zero, as p's
    for (int s = 0; s <= W && ng > n3; s++) HIPCHK(ctx, hipMemsetAsync(ring + (int64_t)s * ng + n3, 0, (size_t)(ng - n3) * 8, st_));
    return STAN_OK;
}
// k > 0: the flush in front of iteration k, covering the terms up to k - 1; k == 0: the closing flush behind the loop
void cg_run::flush_x_ring(int64_t k, int64_t last_enqueued) {
    xring_args a;
    a.n3 = n3; a.ng = ng; a.k = k;
    a.first = ring_flushed + 1; a.last = k - 1; a.last_enqueued = last_enqueued;
    a.W = ring_w; a.ring = ring; a.alpha = ring_alpha; a.x = xb[0]; a.st = stt;
    hipLaunchKernelGGL(k_xring_flush, dim3(vg), dim3(VEC_T), 0, st_, a);
    n_launch++; n_flush++;
    if (k > 0) ring_flushed = k - 1;
}

// ---- one pass of the loop ------------------------------------------------------------------------------------
// Right-hand side, x0 = 0, r0 = p0 = b^, ||b^||, first residual test.  from_F: b^ = S F (the caller's load vector);
// otherwise b^ = the vector in r (a refinement pass: the fp64 residual fp64_check left there).
int cg_run::begin_pass(bool from_F, double eps_pass, bool *done) {
    {
        const fold_args f = vec_fold(sc + S_VMV, p2p_to(0, true));
        if (from_F)
            hipLaunchKernelGGL(k_init, dim3(vg), dim3(VEC_T), 0, st_, n3, dof0, K->d_red, d_F, K->d_scale,
                               bh, xb[0], r, ring_w ? ring_slot(1) : p, partial, f);
        else
            hipLaunchKernelGGL(k_init_b, dim3(vg), dim3(VEC_T), 0, st_, n3, (const double *)r, bh, xb[0], r, p, partial, f);
        reduce_if_unfolded((int)vg, 1, sc + S_VMV, p2p_to(0, true));
    }
    red_src rs_b;
    STANCHK(exchange_sums(sc + S_VMV, 1, &rs_b));
    hipLaunchKernelGGL(k_init_scalars, dim3(1), dim3(64), 0, st_, sc, stt, eps_pass, rs_b);
    HIPCHK(ctx, hipGetLastError());
    // status of "iteration 0" (initial residual test)
    HIPCHK(ctx, hipMemcpyAsync(h_st, stt, T_NSTAT * 8, hipMemcpyDeviceToHost, st_));
    STANCHK(cg_wait(ctx, p2p, st_, nullptr));   // (peer to peer: behind the first reduction's wait)
    *done = h_st[T_ITER_A] == 0;
    return STAN_OK;
}

int cg_run::iterate(double eps_pass, int32_t max_its_pass) {
    int64_t k = 1;
    bool done = false;
    int rc = STAN_OK;
    poll.chunk_id = 0;
    red_src rs_sr{nullptr, 0, nullptr, 0}, rs_vmv{nullptr, 0, nullptr, 0}, rs_r2{nullptr, 0, nullptr, 0};
    // STAN_OPT_CG_REFINE = 2 on a reduced-precision stream: the periodic residual recomputation (alglib's
    // ItsBeforeRUpdate) multiplies with the fp64 values -- the recurrence is re-anchored to the true residual
    // ("reliable updates"), so the literal second product replaces the fused two-product pass
    const bool refresh64 = refine >= 2;
    const int kind_refresh = refresh64 ? STAN_PREC_FP64 : plan.vs;
    // ... and then every REFRESH64 iterations instead of every STAN_OPT_CG_RUPDATE: a refresh on the reduced stream in
    // between would undo the anchoring, and the iteration count does not depend on the period (148^3, fp32 copy: 2346
    // iterations with 10, 20 and 50; profiles/r05/mixed_refine_n148.txt) while every fp64 product costs two of the others
    constexpr int REFRESH64 = 50;
    const int rupdate = refresh64 ? (ctx->cg_rupdate > 0 ? REFRESH64 : 0) : ctx->cg_rupdate;
    if (sr) {   // w_0 = A r_0 with gamma_0, delta_0 (merit_0 = 0 sits in the zeroed scalars)
        if (p2p)         // ... or, peer to peer, is sent as this rank's zero into the slot of the first reduction
            launch_reduce(st_, 1, partial, 0, sc + S_SR_MERIT, p2p_to(2, false), nullptr, 0);
        rc = product(r, nullptr, w, 2, sc + S_SR_GAMMA, 0, p2p_to(0, true), plan.vs);
        if (rc == STAN_OK) rc = exchange_sums(sc + S_SR_GAMMA, 3, &rs_sr);
    }
    // a sharded loop polls more often: what runs ahead of the stop are exchanges nobody can cut short
    const int chunk = dist ? CHUNK_DIST : CHUNK;
    if (ring_w) {   // (setup_x_ring: one pass, the classic loop, every refresh a fused one)
        ring_flushed = 0;
        HIPCHK(ctx, hipMemsetAsync(stt + T_FLUSHED, 0, 8, st_));
    }
    while (!done && rc == STAN_OK) {
        // enqueue one chunk of iterations
        for (int c = 0; c < chunk && k < chunk_poll::hard_cap; c++, k++) {
            const bool refresh = rupdate > 0 && (k % rupdate) == 0;
            if (sr) {
                sr_args a;
                a.n3 = n3; a.k = k; a.sc = sc; a.st = stt; a.epsf = eps_pass; a.maxits = max_its_pass;
                a.its_before_restart = its_before_restart; a.merit_stop = ctx->cg_merit_stop ? 1 : 0;
                a.refresh = refresh ? 1 : 0;
                a.xcur = xb[(k - 1) & 1]; a.xnext = xb[k & 1];
                a.r = r; a.p = p; a.s = sv; a.w = w; a.bh = bh; a.partial = partial;
                a.rs = rs_sr;
                // the merit sum rides in the third column of the coming reduction's mailbox slot (no count of its own)
                a.fold = vec_fold(sc + S_SR_MERIT, p2p_to(2, false));
                hipLaunchKernelGGL(k_vec_sr, dim3(vg), dim3(VEC_T), 0, st_, a);
                n_launch++;
                if (!refresh) reduce_if_unfolded((int)vg, 1, sc + S_SR_MERIT, p2p_to(2, false), k);
                else {   // r' = b^ - A^ x' (ALGLIB's periodic residual recomputation), then as usual
                    rc = product(xb[k & 1], nullptr, v, 0, nullptr, k, NO_P2P, kind_refresh, refresh64);
                    if (rc) break;
                    hipLaunchKernelGGL(k_refresh, dim3(vg), dim3(VEC_T), 0, st_, n3, k, (const int64_t *)stt,
                                       bh, v, xb[k & 1], r, partial, vec_fold(sc + S_SR_DELTA, p2p_to(1, false)));
                    n_launch++;
                    reduce_if_unfolded((int)vg, 2, sc + S_SR_DELTA, p2p_to(1, false), k);   // [r.r (rewritten below), merit]
                }
                rc = product(r, nullptr, w, 2, sc + S_SR_GAMMA, k, p2p_to(0, true), plan.vs);
                if (rc) break;
                rc = exchange_sums(sc + S_SR_GAMMA, 3, &rs_sr);
                if (rc) break;
                continue;
            }
            const bool fused = refresh && ctx->cg_fused_refresh && !refresh64;
            // the ring: p_k sits in its slot, x in xb[0], brought up to x_{k-1} in front of the product that multiplies it
            double *const pk = ring_w ? ring_slot(k) : p;
            double *const xprev = ring_w ? xb[0] : xb[(k - 1) & 1];
            if (ring_w && xring_flush_due(k, ring_flushed, ring_w, refresh)) flush_x_ring(k, 0);
            rc = product(pk, fused ? xprev : nullptr, v, 1, sc + S_VMV, k, p2p_to(0, true), plan.vs);
            if (rc) break;
            rc = exchange_sums(sc + S_VMV, 1, &rs_vmv);
            if (rc) break;
            const p2p_out po_r = p2p_to(0, true);   // the slot of r.r / merit (the wait above moved on to it)
            step_args a;
            a.rs_vmv = rs_vmv;
            a.n3 = n3; a.k = k; a.sc = sc; a.st = stt;
            a.xcur = xb[(k - 1) & 1]; a.xnext = xb[k & 1];
            a.r = r; a.p = pk; a.v = v; a.w = w; a.bh = bh; a.partial = partial;
            a.refresh = refresh ? (fused ? 2 : 1) : 0;
            a.merit = ctx->cg_merit_stop ? 1 : 0;
            // x' = x + a p moves into k_update (p is read once for both updates: -79 MB of 714 per
            // iteration at 148^3) unless the merit sum needs x' here or a literal refresh multiplies it
            a.defer_x = (ctx->cg_defer_x && !a.merit && a.refresh != 1) ? 1 : 0;
            a.fold = vec_fold(sc + S_R2NEW, a.refresh == 1 ? NO_P2P : po_r);   // refresh 1: k_refresh forms the sums
            hipLaunchKernelGGL((ctx->vec_store_nt & 2) ? k_step<true> : k_step<false>, dim3(vg), dim3(VEC_T), 0, st_, a);
            n_launch++;
            if (a.refresh == 1) {
                // a -5/-4 stop of this iteration is caught by k_refresh/k_update (ITER_B <= k)
                rc = product(xb[k & 1], nullptr, v, 0, nullptr, k, NO_P2P, kind_refresh, refresh64);
                if (rc) break;
                hipLaunchKernelGGL(k_refresh, dim3(vg), dim3(VEC_T), 0, st_, n3, k,
                                   (const int64_t *)stt, bh, v, xb[k & 1], r, partial, vec_fold(sc + S_R2NEW, po_r));
                n_launch++;
            }
            if (!foldr) { reduce_if_unfolded((int)vg, 2, sc + S_R2NEW, po_r, k); n_launch++; }
            rc = exchange_sums(sc + S_R2NEW, 2, &rs_r2);
            if (rc) break;
            const double *ux = a.defer_x ? a.xcur : nullptr;
            double *uxn = a.defer_x ? a.xnext : nullptr;
            if (ring_w)   // p_{k+1} into the next slot, alpha_k next to the ring; x waits for the flush
                hipLaunchKernelGGL(((ctx->vec_store_nt & 1) ? k_update<true, true> : k_update<false, true>), dim3(vg), dim3(VEC_T), 0, st_, n3, k, sc, stt,
                                   eps_pass, (int64_t)max_its_pass, its_before_restart, 0, r, pk, (const double *)nullptr, (double *)nullptr,
                                   rs_r2, rs_vmv, ring_slot(k + 1), ring_alpha + xring_slot(k, ring_w));
            else
                hipLaunchKernelGGL(((ctx->vec_store_nt & 1) ? k_update<true, false> : k_update<false, false>), dim3(vg), dim3(VEC_T), 0, st_, n3, k, sc, stt,
                                   eps_pass, (int64_t)max_its_pass, its_before_restart, ctx->cg_merit_stop ? 1 : 0, r, p, ux, uxn, rs_r2, rs_vmv,
                                   (double *)nullptr, (double *)nullptr);
            n_launch++;
        }
        if (rc) break;
        // poll: read the status of the PREVIOUS chunk while this one runs
        STANCHK(poll.poll(ctx, st_, stt, T_NSTAT, k, [&](hipEvent_t e) { return cg_wait(ctx, p2p, st_, e); },
                          [](const int64_t *w) { return w[T_TYPE] != 0; }, &done));
        if (dist && (ctx->comm_broken.load() || (ctx->p2p && ctx->p2p->broken.load()))) {
            ctx->err = "cg: a peer rank failed (the exchanges were aborted)";
            rc = STAN_E_COMM;
        }
    }
    n_enqueued += k - 1;
    if (p2p) {   // never a blocking wait on a stream that may sit in front of a peer that is gone
        if (rc == STAN_OK) rc = cg_wait(ctx, true, st_, nullptr);
        else stan_p2p_release_own(ctx);
    }
    hipError_t e = hipStreamSynchronize(st_);
    if (rc) return rc;
    if (e != hipSuccess) { ctx->err = std::string("cg: ") + hipGetErrorString(e); return STAN_E_HIP; }
    if (ring_w) flush_x_ring(0, k - 1);   // the closing flush: x in xb[0] becomes the iterate T_XSEL / T_ITERS name
    HIPCHK(ctx, hipMemcpyAsync(h_st, stt, T_NSTAT * 8, hipMemcpyDeviceToHost, st_));
    HIPCHK(ctx, hipMemcpyAsync(h_sc, sc, S_NSCAL * 8, hipMemcpyDeviceToHost, st_));
    HIPCHK(ctx, hipStreamSynchronize(st_));
    pass_type = (int)h_st[T_TYPE];
    pass_its = h_st[T_ITERS];
    if (pass_type == 0) { pass_type = 5; pass_its = k - 1; h_st[T_XSEL] = (k - 1) & 1; }  // hard cap
    xfin = ring_w ? xb[0] : xb[h_st[T_XSEL] & 1];
    return STAN_OK;
}

int cg_run::pass(bool from_F, double eps_pass, int32_t max_its_pass) {
    bool done = false;
    STANCHK(begin_pass(from_F, eps_pass, &done));
    if (done) {   // the first residual test ended it (b = 0, or eps >= 1): no iteration
        HIPCHK(ctx, hipMemcpyAsync(h_sc, sc, S_NSCAL * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(ctx, hipStreamSynchronize(st_));
        pass_type = (int)h_st[T_TYPE];
        pass_its = h_st[T_ITERS];
        xfin = xb[h_st[T_XSEL] & 1];
        return STAN_OK;
    }
    STANCHK(iterate(eps_pass, max_its_pass));
    account_pass();
    return STAN_OK;
}

// profile: the launch times of the pass that has just ended (its stream is synchronised).  Only launches that did
// work count: the host runs up to two chunks ahead of the status it polls, so a converged solve is followed by a few
// dozen launches that return at once (3-4 us each); averaging those in made the SpMV look ~3 % faster than it is.
void cg_run::account_pass() {
    spmv_sp.drain(pass_its, &prof_spmv_ms, &prof_spmv_n);
    spmv2_sp.drain(pass_its, &prof_spmv2_ms, &prof_spmv2_n);
}

// ---- the fp64 check of a reduced-precision solve ----------------------------------------------------------------
// r_t = b - A^64 xg with the fp64 values of the scaled matrix (xg: a gather vector -- one of the vectors the peers know,
// cg_run::setup -- holding the iterate on the owned rows); r_t stays in r, *r2_out = ||r_t||^2 over all ranks.
int cg_run::fp64_check(double *xg, const double *b, double *r2_out) {
    STANCHK(product(xg, nullptr, v, 0, nullptr, 0, NO_P2P, STAN_PREC_FP64, true));
    const p2p_out po = p2p_to(0, true);
    hipLaunchKernelGGL(k_refresh, dim3(vg), dim3(VEC_T), 0, st_, n3, (int64_t)0, (const int64_t *)stt, b, v,
                       (const double *)xg, r, partial, vec_fold(sc + S_CHK_R2, po));
    n_launch++;
    reduce_if_unfolded((int)vg, 2, sc + S_CHK_R2, po);
    red_src rs;
    STANCHK(exchange_sums(sc + S_CHK_R2, 2, &rs));
    if (rs.mb) hipLaunchKernelGGL(k_land_sums, dim3(1), dim3(64), 0, st_, sc + S_CHK_R2, rs);   // peer to peer: the mailbox's sums into the local scalars
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(h_sc, sc, S_NSCAL * 8, hipMemcpyDeviceToHost, st_));
    STANCHK(cg_wait(ctx, p2p, st_, nullptr));
    *r2_out = h_sc[S_CHK_R2];
    // the check itself (it carries iteration 0) and the refreshes of the pass behind it that did work: the host enqueues up to two
    // chunks past the stop, and a refresh out there returns at once -- counted, it made fp64_products depend on the chunk size
    spmv64_sp.drain(pass_its, &prof_spmv64_ms, &prof_spmv64_n);
    return STAN_OK;
}

// ---- epilogue ------------------------------------------------------------------------------------------------
int cg_run::finish(const double *x_result, int type, int64_t its, double rel_rec, double rel64, int passes,
                   int32_t *term_out, int32_t *iters_out, double *rel_res_out) {
    // U = S x^ on the free DOFs (a rank of a one-process group leaves only ITS entries [u0, u1) of U: the
    // group copies every rank's segment into the caller's buffer, nothing is gathered on the devices)
    if (!dist || ctx->result_segment) {
        hipLaunchKernelGGL(k_result, dim3(vg), dim3(VEC_T), 0, st_, n3, dof0, K->d_red, K->d_scale,
                           x_result, d_U);
    } else {
        double *full;
        STANCHK(bufs.alloc(&full, (size_t)K->n_dof));
        hipLaunchKernelGGL(k_result_full, dim3(vg), dim3(VEC_T), 0, st_, n3, K->d_scale, x_result,
                           full + dof0);
        STANCHK(stan_comm_allgather_rows(ctx, K, full));
        hipLaunchKernelGGL(k_compress, dim3(vec_grid(K->n_dof)), dim3(VEC_T), 0, st_, K->n_dof,
                           K->d_red, full, d_U);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->profiling) hipEventRecord(ev1, st_);
    HIPCHK(ctx, hipStreamSynchronize(st_));

    ctx->prof_x_ring_window = ring_w;
    ctx->prof_x_ring_flushes = n_flush;
    ctx->prof_refresh_stream = refresh_stream;
    if (term_out) *term_out = type;
    if (iters_out) *iters_out = (int32_t)(its > chunk_poll::hard_cap ? chunk_poll::hard_cap : its);
    if (rel_res_out) *rel_res_out = rel64 >= 0 ? rel64 : rel_rec;
    if (!ctx->profiling) return STAN_OK;
    float ms = 0;
    hipEventElapsedTime(&ms, ev0, ev1);
    stan_profile &pf = ctx->prof;
    pf.cg_ms = ms;
    pf.spmv_ms_total = prof_spmv_ms;
    pf.spmv_launches = prof_spmv_n;
    pf.spmv2_ms_total = prof_spmv2_ms;
    pf.spmv2_launches = prof_spmv2_n;
    pf.fp64_products = (int32_t)prof_spmv64_n;
    pf.fp64_products_ms = prof_spmv64_ms;
    pf.iterations = (int32_t)its;
    pf.termination_type = type;
    pf.rel_residual_recurrence = rel_rec;
    pf.rel_residual_fp64 = rel64;
    pf.refine_passes = passes;
    const int stream = n60 > 0 ? (int)STAN_VALUE_STREAM_60 : plan.vs;   // the stream the plain products (what spmv_ms_total times) read
    // bytes of the format actually streamed: a block costs its values and a 4-B column index; a block of a packed slice
    // carries a 2-B column offset instead (+ 4 B per slot for its base, shared by 64 rows)
    // (the folded copy has a packed column stream of its own, one base per slot, and 4 B of plan per row)
    const stan_colpack &c = *plan.cols;
    const bool read_packed = ctx->cols16 && c.cols16;
    const double packed_frac = read_packed && plan.slots > 0 ? (double)c.slots_packed / (double)plan.slots : 0.0;
    pf.spmv_bytes = K->nblocks * (4 * K->vs[stream].dwords + 4) + 3 * K->nloc * 16 + K->nloc * (plan.folded ? 8 : 4)
                    - (int64_t)(packed_frac * (double)K->nblocks * 2.0) + (read_packed ? (c.slots_packed + c.slots_packed2) * 4 : 0);
    pf.repacked_streams = plan.folded ? 1 : 0;
    pf.col_slots_packed = ctx->cols16 && K->pk.cols16 ? K->pk.slots_packed : 0;   // (the padded stream's count even when the products read the folded copy: looks unintended, kept)
    pf.value_stream = stream;
    // vector passes of one classic iteration: k_step reads r, v (+ p, x unless deferred; + b^ for the
    // merit sum) and writes r (+ x); k_update reads r, p (+ x when deferred) and writes p (+ x)
    pf.cg_iteration_vector_bytes = 3 * K->nloc * 8 * ((ctx->cg_defer_x && !ctx->cg_merit_stop ? 8 : 9) + (ctx->cg_merit_stop ? 1 : 0));
    // the ring: k_update reads r, p and writes p (6 passes with k_step's 3), a flush per window reads W directions and x and writes x
    if (ring_w) pf.cg_iteration_vector_bytes = 3 * K->nloc * 8 * (7 * (int64_t)ring_w + 2) / ring_w;
    pf.loop_kernel_launches = n_launch;
    pf.loop_collectives = n_coll;
    pf.loop_stream_waits = n_wait;
    pf.loop_iterations_enqueued = n_enqueued;
    // what the stream spent in the exchanges (RCCL launches, or peer-to-peer waits): events around each
    pf.comm_reduce_ms_total = pf.comm_halo_ms_total = 0;
    pf.comm_reduce_calls = pf.comm_halo_calls = 0;
    red_sp.drain(chunk_poll::hard_cap, &pf.comm_reduce_ms_total, &pf.comm_reduce_calls);
    halo_sp.drain(chunk_poll::hard_cap, &pf.comm_halo_ms_total, &pf.comm_halo_calls);
    return STAN_OK;
}

}  // namespace

int stan_cg_device(stan_ctx *ctx, stan_matrix *K, const double *d_F, double eps_f,
                   int32_t max_its, int32_t precision_mode, double *d_U, int32_t *term_out,
                   int32_t *iters_out, double *rel_res_out) {
    if (precision_mode != STAN_PREC_FP64 && precision_mode != STAN_PREC_MIXED &&
        precision_mode != STAN_PREC_FIXED48) {
        ctx->err = "cg_solve: unknown precision_mode";
        return STAN_E_UNSUPPORTED;
    }
    if (eps_f < 0 || max_its < 0) {
        ctx->err = "cg_solve: eps_f and max_its must be >= 0";
        return STAN_E_ARG;
    }
    if (eps_f == 0 && max_its == 0) eps_f = 1.0e-6;  // lincgsetcond
    // no hipFree while the peers' streams wait for this rank's future exchanges (stan_ctx::defer_frees); the guard
    // outlives the run object, whose buffers are released into the deferred list
    struct free_later { stan_ctx *c; ~free_later() { if (c->defer_frees) { stan_flush_deferred(c); stan_p2p_ipc_trim(c); } } } free_guard{ctx};
    cg_run R{ctx, K, d_F, eps_f, max_its, precision_mode, d_U};
    STANCHK(R.setup());

    constexpr int MAX_PASSES = 8;
    int type = 0, passes = 0;
    int64_t its = 0;
    double bnorm0 = 0, rel_rec = 0, rel64 = -1.0, prev_rel64 = 0, eps_pass = eps_f;
    const double *x_result = nullptr;
    for (;;) {
        const int64_t left = max_its > 0 ? (int64_t)max_its - its : 0;
        STANCHK(R.pass(passes == 0, eps_pass, (int32_t)left));
        passes++;
        its += R.pass_its;
        type = R.pass_type;
        if (passes == 1) bnorm0 = R.h_sc[S_BNORM];
        // ||r|| / ||b|| of the loop's own recurrence, against the ORIGINAL right-hand side (what alglib reports)
        rel_rec = bnorm0 > 0 ? std::sqrt(R.h_sc[S_R2OUT]) / bnorm0 : 0.0;
        x_result = R.xfin;
        if (!R.reduced) break;
        // ---- a reduced-precision mode: what was delivered, in fp64 ----
        double *xg = const_cast<double *>(R.xfin);
        if (passes > 1) {   // the passes' iterates add up: x = x_1 + d_2 + ...; gathered from p (a vector the peers know)
            hipLaunchKernelGGL(k_accumulate, dim3(R.vg), dim3(VEC_T), 0, R.st_, R.n3, R.xacc, R.xfin, R.p);
            xg = R.p;
            x_result = R.xacc;
        }
        double r2 = 0;
        STANCHK(R.fp64_check(xg, passes > 1 ? R.b0 : R.bh, &r2));
        rel64 = bnorm0 > 0 ? std::sqrt(r2) / bnorm0 : 0.0;
        const bool met = rel64 <= eps_f || bnorm0 == 0;
        if (type != 1) break;                       // 5, 7, -4, -5: reported as the loop ended, with the fp64 residual
        if (met) break;
        // the recurrence says converged, the fp64 residual does not: another pass on r_t (iterative refinement) ...
        const bool out_of_its = max_its > 0 && its >= max_its;
        const bool stalled = passes > 1 && !(rel64 < 0.5 * prev_rel64);
        if (R.refine == 0 || passes >= MAX_PASSES || out_of_its || stalled || !std::isfinite(rel64)) {
            type = out_of_its ? 5 : 7;             // ... or the truth: no further progress at this precision (alglib's 7)
            break;
        }
        if (passes == 1) {
            STANCHK(R.bufs.alloc(&R.xacc, (size_t)(R.n3 > 0 ? R.n3 : 1)));
            STANCHK(R.bufs.alloc(&R.b0, (size_t)(R.n3 > 0 ? R.n3 : 1)));
            HIPCHK(ctx, hipMemcpyAsync(R.xacc, R.xfin, (size_t)R.n3 * 8, hipMemcpyDeviceToDevice, R.st_));
            HIPCHK(ctx, hipMemcpyAsync(R.b0, R.bh, (size_t)R.n3 * 8, hipMemcpyDeviceToDevice, R.st_));
        }
        prev_rel64 = rel64;
        eps_pass = eps_f / rel64;                   // ||r|| <= eps ||b0|| with ||b_pass|| = ||r_t|| = rel64 ||b0||
        HIPCHK(ctx, hipMemsetAsync(R.sc, 0, S_NSCAL * 8, R.st_));
        if (R.sr) HIPCHK(ctx, hipMemsetAsync(R.sv, 0, (size_t)R.n3 * 8, R.st_));
    }
    return R.finish(x_result, type, its, rel_rec, rel64, passes, term_out, iters_out, rel_res_out);
}

// ---- several load cases in one loop over a single pass of K (stan_hip_cg_solve_multi) -------------------------------------
// n_rhs right-hand sides are cut into groups of 8, 4, 2, 1 columns, run one after the other; a group is ONE loop of the
// shape of cg_run::iterate on interleaved vectors of its own (cg_multi.inc), whose every kernel serves all live columns.
// One form only: padded BSELL streams (packed columns when the context has them), k_spmm, ensure_scaled before the loop,
// folded reductions, the literal second product on refresh iterations.  One rank, fp64 stream, classic loop.
namespace {

constexpr int MULTI_MAX = 8;   // widest group (k_spmm<8>: register table in DESIGN.md)

struct pinned_words {
    int64_t *p = nullptr;
    ~pinned_words() { if (p) (void)hipHostFree(p); }
};

struct cg_multi_run {
    stan_ctx *ctx;
    stan_matrix *K;
    double eps_f;
    int32_t max_its;
    hipStream_t st_ = nullptr;
    dev_scope bufs{ctx};
    int64_t n3 = 0, ng = 0, pstride = 0, its_before_restart = 1;
    unsigned vg = 1, pg = 0;
    double *xb[2] = {nullptr, nullptr}, *p = nullptr, *r = nullptr, *v = nullptr, *bh = nullptr, *partial = nullptr, *sc = nullptr;
    int64_t *stt = nullptr;
    unsigned long long *tick = nullptr;
    pinned_words host;          // [2][MULTI_MAX][T_NSTAT] poll slots, [MULTI_MAX][T_NSTAT] final status, [MULTI_MAX][S_NSCAL] scalars
    event_bag events;
    chunk_poll poll;

    int setup(int mmax) {
        st_ = ctx->stream;
        STANCHK(ensure_scaled(ctx, K));
        if (ctx->cols16) STANCHK(stan_matrix_make_cols16(ctx, K));
        n3 = 3 * K->nloc;
        ng = gather_len(K);
        vg = vec_grid(n3);
        pg = nblk(K->nslices, 4);
        pstride = 2 * (int64_t)(pg > VEC_BLOCKS ? pg : VEC_BLOCKS) + 16;
        its_before_restart = K->n_red > 0 ? K->n_red : 1;
        const size_t m = (size_t)mmax, g = (size_t)(ng > 0 ? ng : 1), n = (size_t)(n3 > 0 ? n3 : 1);
        for (double **q : {&xb[0], &xb[1], &p}) STANCHK(bufs.alloc(q, g * m));
        for (double **q : {&r, &v, &bh}) STANCHK(bufs.alloc(q, n * m));
        STANCHK(bufs.alloc(&partial, (size_t)pstride * m));
        STANCHK(bufs.alloc(&sc, (size_t)S_NSCAL * m));
        STANCHK(bufs.alloc(&stt, (size_t)T_NSTAT * m));
        STANCHK(bufs.alloc(&tick, (size_t)(2 * FOLD_WORDS)));
        HIPCHK(ctx, hipHostMalloc((void **)&host.p, (size_t)(3 * T_NSTAT + S_NSCAL) * MULTI_MAX * 8, hipHostMallocDefault));
        poll.setup(events, host.p, MULTI_MAX * T_NSTAT);
        return STAN_OK;
    }

    // one group: columns [c0, c0 + M) of F and U
    template <int M>
    int group(const double *d_F, double *d_U, int32_t *term_out, int32_t *iters_out, double *rel_out) {
        const int64_t nr = K->n_red;
        const size_t g = (size_t)(ng > 0 ? ng : 1);
        const int merit = ctx->cg_merit_stop ? 1 : 0, rupdate = ctx->cg_rupdate;
        const colstream cs = colstream_of(ctx, K->pk, K->nslots);
        const fold_args fvec{tick + FOLD_WORDS, vg, (int)vg, nullptr, NO_P2P};   // counter set 1 serves the vector kernels,
        const fold_args fprod{tick, pg, (int)pg, nullptr, NO_P2P};               // set 0 the products
        int64_t *h_st = host.p + 2 * MULTI_MAX * T_NSTAT;
        double *h_sc = (double *)(host.p + 3 * MULTI_MAX * T_NSTAT);
        HIPCHK(ctx, hipMemsetAsync(sc, 0, (size_t)S_NSCAL * M * 8, st_));
        HIPCHK(ctx, hipMemsetAsync(stt, 0, (size_t)T_NSTAT * M * 8, st_));
        HIPCHK(ctx, hipMemsetAsync(tick, 0, 2 * FOLD_WORDS * 8, st_));
        for (double *q : {xb[0], xb[1], p}) HIPCHK(ctx, hipMemsetAsync(q, 0, g * M * 8, st_));
        hipLaunchKernelGGL(k_init_m<M>, dim3(vg), dim3(VEC_T), 0, st_, n3, nr, K->d_red, d_F, K->d_scale, bh, xb[0], r, p, partial,
                           pstride, sc, fvec);
        hipLaunchKernelGGL(k_init_scalars_m<M>, dim3(1), dim3(64), 0, st_, sc, stt, eps_f);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(h_st, stt, (size_t)T_NSTAT * M * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(ctx, hipStreamSynchronize(st_));
        auto all_stopped = [&](const int64_t *w) {
            for (int c = 0; c < M; c++) if (w[c * T_NSTAT + T_TYPE] == 0) return false;
            return true;
        };
        bool done = all_stopped(h_st) || pg == 0;   // the first residual test ended every column (b = 0, or eps >= 1)
        int64_t k = 1;
        poll.chunk_id = 0;
        while (!done) {
            for (int c = 0; c < CHUNK && k < chunk_poll::hard_cap; c++, k++) {
                const bool refresh = rupdate > 0 && (k % rupdate) == 0;
                hipLaunchKernelGGL((k_spmm<M, 1>), dim3(pg), dim3(256), 0, st_, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof, K->d_cols,
                                   K->vals64(), p, v, partial, pstride, sc, stt, k, fprod, cs);
                mstep_args a;
                a.n3 = n3; a.k = k; a.sc = sc; a.st = stt;
                a.xcur = xb[(k - 1) & 1]; a.xnext = xb[k & 1];
                a.r = r; a.p = p; a.v = v; a.bh = bh; a.partial = partial; a.pstride = pstride;
                a.merit = merit; a.refresh = refresh ? 1 : 0; a.fold = fvec;
                hipLaunchKernelGGL(k_step_m<M>, dim3(vg), dim3(VEC_T), 0, st_, a);
                if (refresh) {   // r = b^ - A^ x' from alglib's literal second product
                    hipLaunchKernelGGL((k_spmm<M, 0>), dim3(pg), dim3(256), 0, st_, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                                       K->d_cols, K->vals64(), xb[k & 1], v, partial, pstride, sc, stt, k, NO_FOLD, cs);
                    hipLaunchKernelGGL(k_refresh_m<M>, dim3(vg), dim3(VEC_T), 0, st_, n3, k, sc, (const int64_t *)stt, bh, v, xb[k & 1],
                                       r, partial, pstride, fvec);
                }
                hipLaunchKernelGGL(k_update_m<M>, dim3(vg), dim3(VEC_T), 0, st_, n3, k, sc, stt, eps_f, (int64_t)max_its,
                                   its_before_restart, merit, r, p);
            }
            HIPCHK(ctx, hipGetLastError());
            // poll: read the status of the PREVIOUS chunk while this one runs; done when every column has stopped
            STANCHK(poll.poll(ctx, st_, stt, (size_t)T_NSTAT * M, k, [&](hipEvent_t e) { return cg_wait(ctx, false, st_, e); }, all_stopped, &done));
        }
        HIPCHK(ctx, hipStreamSynchronize(st_));
        HIPCHK(ctx, hipMemcpyAsync(h_st, stt, (size_t)T_NSTAT * M * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(ctx, hipMemcpyAsync(h_sc, sc, (size_t)S_NSCAL * M * 8, hipMemcpyDeviceToHost, st_));
        HIPCHK(ctx, hipStreamSynchronize(st_));
        bool capped = false;
        for (int c = 0; c < M; c++) {
            int64_t *w = h_st + c * T_NSTAT;
            if (w[T_TYPE] == 0) { w[T_TYPE] = 5; w[T_ITERS] = k - 1; w[T_XSEL] = (k - 1) & 1; capped = true; }   // hard cap
        }
        if (capped) HIPCHK(ctx, hipMemcpyAsync(stt, h_st, (size_t)T_NSTAT * M * 8, hipMemcpyHostToDevice, st_));
        hipLaunchKernelGGL(k_result_m<M>, dim3(vg), dim3(VEC_T), 0, st_, n3, nr, K->d_red, K->d_scale, xb[0], xb[1],
                           (const int64_t *)stt, d_U);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st_));
        for (int c = 0; c < M; c++) {
            const int64_t *w = h_st + c * T_NSTAT;
            const double bnorm = h_sc[c * S_NSCAL + S_BNORM];
            if (term_out) term_out[c] = (int32_t)w[T_TYPE];
            if (iters_out) iters_out[c] = (int32_t)(w[T_ITERS] > chunk_poll::hard_cap ? chunk_poll::hard_cap : w[T_ITERS]);
            if (rel_out) rel_out[c] = bnorm > 0 ? std::sqrt(h_sc[c * S_NSCAL + S_R2OUT]) / bnorm : 0.0;
        }
        return STAN_OK;
    }
};

}  // namespace

int stan_cg_multi_device(stan_ctx *ctx, stan_matrix *K, int32_t n_rhs, const double *d_F, double eps_f, int32_t max_its,
                         int32_t precision_mode, double *d_U, int32_t *term_out, int32_t *iters_out, double *rel_res_out) {
    if (stan_sharded(ctx)) {
        ctx->err = "cg_solve_multi: single-rank contexts only (no communicator)";
        return STAN_E_UNSUPPORTED;
    }
    if (precision_mode != STAN_PREC_FP64) {
        ctx->err = "cg_solve_multi: only the fp64 value stream (STAN_PREC_FP64) is supported";
        return STAN_E_UNSUPPORTED;
    }
    if (ctx->cg_single_reduce) {
        ctx->err = "cg_solve_multi: the single-reduction loop (STAN_OPT_CG_SINGLE_REDUCE) is not supported";
        return STAN_E_UNSUPPORTED;
    }
    if (n_rhs <= 0) {
        ctx->err = "cg_solve_multi: n_rhs must be > 0";
        return STAN_E_ARG;
    }
    if (eps_f < 0 || max_its < 0) {
        ctx->err = "cg_solve_multi: eps_f and max_its must be >= 0";
        return STAN_E_ARG;
    }
    if (eps_f == 0 && max_its == 0) eps_f = 1.0e-6;  // lincgsetcond
    cg_multi_run R{ctx, K, eps_f, max_its};
    STANCHK(R.setup(n_rhs >= 8 ? 8 : n_rhs >= 4 ? 4 : n_rhs >= 2 ? 2 : 1));
    const int64_t N = K->n_red;
    for (int32_t c0 = 0; c0 < n_rhs;) {
        const int32_t left = n_rhs - c0;
        const double *F = d_F + (int64_t)c0 * N;
        double *U = d_U + (int64_t)c0 * N;
        int32_t *t = term_out ? term_out + c0 : nullptr, *i = iters_out ? iters_out + c0 : nullptr;
        double *rr = rel_res_out ? rel_res_out + c0 : nullptr;
        if (left >= 8) { STANCHK(R.group<8>(F, U, t, i, rr)); c0 += 8; }
        else if (left >= 4) { STANCHK(R.group<4>(F, U, t, i, rr)); c0 += 4; }
        else if (left >= 2) { STANCHK(R.group<2>(F, U, t, i, rr)); c0 += 2; }
        else { STANCHK(R.group<1>(F, U, t, i, rr)); c0 += 1; }
    }
    return STAN_OK;
}

#include "cg_entries.inc"   // test and bench entries: the products outside a solve
