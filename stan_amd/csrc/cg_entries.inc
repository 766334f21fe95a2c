// cg_entries.inc -- the products OUTSIDE a solve: test helpers (stan_spmv_reduced, stan_matrix_diagonal, stan_spmv_local) and
// the timing entries (stan_spmv_bench_device, stan_stream_bench_device, stan_spmv_probe of the placement search)
// Part of cg.hip (included at its end, at file scope: they need launch_product and the kernels; not a translation unit of
// its own).  Each entry takes its product_plan from plan_products once: the kernel form a solve under the same options launches.

namespace {

// status words for kernels launched outside a solve: never stopped
int alloc_never_stopped(stan_ctx *ctx, dev_scope &b, int64_t **stt, hipStream_t s) {
    STANCHK(b.alloc(stt, (size_t)T_NSTAT));
    const int64_t init[T_NSTAT] = {0x7fffffffffffffffLL, 0x7fffffffffffffffLL, 0, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(*stt, init, sizeof(init), hipMemcpyHostToDevice, s));
    return STAN_OK;
}

// y = A x with K's fp64 values, no sums: the products outside a solve
unsigned launch_plain_product(stan_ctx *ctx, stan_matrix *K, const double *x, double *y, const int64_t *st, int which = 0) {
    const product_args a{x, y, nullptr, nullptr, 0, nullptr, st, 1, STAN_PREC_FP64, nullptr, false, false};
    return launch_product(ctx, K, plan_products(ctx, K, a.kind, stan_sharded(ctx), false), a, which);
}

}  // namespace

// y = K x on the reduced system (test helper; single rank)
int stan_spmv_reduced(stan_ctx *ctx, stan_matrix *K, const double *d_x, double *d_y) {
    if (ctx->nranks != 1) { ctx->err = "spmv: single-rank contexts only"; return STAN_E_UNSUPPORTED; }
    hipStream_t st_ = ctx->stream;
    const int64_t n3 = 3 * K->nloc, npad3 = 3 * (int64_t)K->nslices * 64;
    dev_scope bufs(ctx);
    double *xf, *yf; int64_t *stt;
    STANCHK(bufs.alloc(&xf, (size_t)npad3));
    STANCHK(bufs.alloc(&yf, (size_t)npad3));
    STANCHK(alloc_never_stopped(ctx, bufs, &stt, st_));
    HIPCHK(ctx, hipMemsetAsync(xf, 0, (size_t)npad3 * 8, st_));
    const double *sdiv = K->scaled ? K->d_scale : nullptr;
    // K x = S^-1 (A^ (S^-1 x)) when the matrix already carries its scaling
    hipLaunchKernelGGL(k_expand, dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, n3, (int64_t)0, K->d_red,
                       d_x, sdiv, xf);
    launch_plain_product(ctx, K, xf, yf, stt);
    // compress (and undo the row scaling)
    hipLaunchKernelGGL(k_compress_div, dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, n3, K->d_red, sdiv, yf, d_y);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st_));
    return STAN_OK;
}

// diag[d - red[d]] = K_dd on the free DOFs (single rank)
int stan_matrix_diagonal(stan_ctx *ctx, stan_matrix *K, double *d_diag) {
    if (ctx->nranks != 1) { ctx->err = "matrix_diagonal: single-rank contexts only"; return STAN_E_UNSUPPORTED; }
    hipStream_t st_ = ctx->stream;
    const int64_t n3 = 3 * K->nloc;
    dev_scope bufs(ctx);
    double *full;
    STANCHK(bufs.alloc(&full, (size_t)(n3 > 0 ? n3 : 1)));
    if (K->nloc > 0)
        hipLaunchKernelGGL(k_diag_get, dim3(nblk(K->nloc, 256)), dim3(256), 0, st_, K->nloc, K->d_rowlen, K->d_posof,
                           K->d_slot_ptr, K->d_cols, K->vals64(), K->scaled ? K->d_scale : (const double *)nullptr, full);
    hipLaunchKernelGGL(k_compress_div, dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, n3, K->d_red, (const double *)nullptr, full, d_diag);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st_));
    return STAN_OK;
}

// y_owned = A_local x_local, x_local = [owned rows | halo columns] (plan checks; any rank)
int stan_spmv_local(stan_ctx *ctx, stan_matrix *K, const double *d_x, double *d_y) {
    dev_scope bufs(ctx);
    int64_t *stt;
    STANCHK(alloc_never_stopped(ctx, bufs, &stt, ctx->stream));
    if (K->d_sl_bnd) {  // sharded: interior + boundary lists must cover every slice exactly once
        HIPCHK(ctx, hipMemsetAsync(d_y, 0xff, (size_t)(3 * K->nloc) * 8, ctx->stream));  // NaN
        launch_plain_product(ctx, K, d_x, d_y, stt, 1);
        launch_plain_product(ctx, K, d_x, d_y, stt, 2);
    } else
        launch_plain_product(ctx, K, d_x, d_y, stt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}

// What stan_spmv_bench_device and stan_spmv_probe time: the product with its p.Ap sum, of the value stream `vals` (nullptr:
// K's own of that precision), on the CG's own gather vector and product buffer -- the pair (value block, vector blocks)
// that is timed is the pair the solve will run on -- or, self_block given, on vectors carved out of the front of that
// block (a.x stays nullptr when they do not fit).  The gather vector is filled with ones.
static int timed_product_setup(stan_ctx *ctx, stan_matrix *K, const product_plan &P, int32_t precision, const void *vals, bool vals_folded,
                               void *self_block, size_t self_bytes, dev_scope &bufs, product_args &a) {
    hipStream_t st_ = ctx->stream;
    const int64_t ng = gather_len(K), ngpad = (ng + 511) & ~(int64_t)511;
    STANCHK(stan_cg_workspace(ctx, K));
    double *x = ctx->ws.p, *y = ctx->ws.v, *partial;
    int64_t *stt;
    if (self_block) {
        if ((size_t)(ngpad + 3 * K->nloc) * 8 > self_bytes) return STAN_OK;
        x = (double *)self_block;
        y = x + ngpad;
    }
    STANCHK(bufs.alloc(&partial, 2 * (size_t)P.blocks + 2));
    STANCHK(alloc_never_stopped(ctx, bufs, &stt, st_));
    hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
    a = product_args{x, y, nullptr, nullptr, 1, partial, stt, 1, precision, vals, vals_folded, false};
    return STAN_OK;
}

// `warm` launches, then `groups` groups of `reps` launches back to back, each between two events: the fastest group's ms
// per launch.  (Round 4: single launches between host synchronisations start on an idle device and read 2-3 % under the
// same kernel inside a sequence of kernels.)
template <typename F>
static int timed_launches(stan_ctx *ctx, int warm, int groups, int reps, F launch, float *ms_per_launch) {
    event_bag events;
    for (int i = 0; i < warm; i++) launch();
    float best = 0;
    for (int g = 0; g < groups; g++) {
        hipEvent_t a = events.make(), b = events.make();
        hipEventRecord(a, ctx->stream);
        for (int i = 0; i < reps; i++) launch();
        hipEventRecord(b, ctx->stream);
        HIPCHK(ctx, hipEventSynchronize(b));
        float t = 0;
        hipEventElapsedTime(&t, a, b);
        if (g == 0 || t < best) best = t;
    }
    HIPCHK(ctx, hipGetLastError());
    *ms_per_launch = best / reps;
    return STAN_OK;
}

int stan_spmv_bench_device(stan_ctx *ctx, stan_matrix *K, int32_t precision_mode, int32_t reps,
                           double *avg_ms) {
    if (precision_mode == STAN_PREC_MIXED) STANCHK(stan_matrix_make_fp32(ctx, K));
    if (precision_mode == STAN_PREC_FIXED48) {
        STANCHK(ensure_scaled(ctx, K));
        STANCHK(stan_matrix_make_fx48(ctx, K));
        if (!K->vs[STAN_PREC_FIXED48].padded) { ctx->err = "spmv_bench: matrix not representable in FIXED48"; return STAN_E_UNSUPPORTED; }
    }
    if (precision_mode == STAN_VALUE_STREAM_60) {   // k_spmv on the lossless 60-bit stream of the scaled values
        const stan_value_stream &s60 = K->vs[STAN_VALUE_STREAM_60];
        STANCHK(ensure_scaled(ctx, K));
        if (!s60.padded && !s60.refused && K->nslots > 0) {
            uint32_t *blk = nullptr;
            STANCHK(stan_matrix_alloc_s60(ctx, K, &blk));
            if (!blk) { ctx->err = "spmv_bench: no room for the 60-bit stream within the pool budget and the free-memory floor"; return STAN_E_ALLOC; }
            STANCHK(stan_matrix_encode_s60(ctx, K, blk));
        }
        if (!s60.padded) { ctx->err = "spmv_bench: matrix not representable in the 60-bit stream"; return STAN_E_UNSUPPORTED; }
    }
    dev_scope bufs(ctx);
    product_args pa{};
    const product_plan P = plan_products(ctx, K, precision_mode, stan_sharded(ctx), false);
    STANCHK(timed_product_setup(ctx, K, P, precision_mode, nullptr, false, nullptr, 0, bufs, pa));
    float ms = 0;
    STANCHK(timed_launches(ctx, 3, 1, reps, [&]() { launch_product(ctx, K, P, pa); }, &ms));
    *avg_ms = reps > 0 ? ms : 0;
    return STAN_OK;
}

namespace {
// the 60-bit stream back to doubles through the products' own load9: out[slot][9][64]
__global__ void __launch_bounds__(256)
k_from_s60(int64_t nslots, const s60_t *in, double *out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = t >> 6;
    const int lane = (int)(t & 63);
    if (slot >= nslots) return;
    double a[9];
    load9<true, s60_t>(in + slot * vstream<s60_t>::STRIDE + lane, a);
#pragma unroll
    for (int j = 0; j < 9; j++) out[slot * 9 * 64 + j * 64 + lane] = a[j];
}
}  // namespace

// Test hook of the 60-bit stream (stan_hip_stream60_roundtrip): `n` doubles, laid out as the values of ceil(n / 576) slots
// (padded with zeros), through the encoder of the solve (k_to_s60) and the decoder of the products (load9) on the device;
// *refused = the encoder's count.  Host pointers.
int stan_stream60_roundtrip_device(stan_ctx *ctx, int64_t n, const double *in, double *out, int64_t *refused) {
    hipStream_t st_ = ctx->stream;
    const int64_t nslots = (n + 575) / 576, npad = nslots * 576;
    dev_scope bufs(ctx);
    double *d_in, *d_out;
    uint32_t *d_enc;
    STANCHK(bufs.alloc(&d_in, (size_t)npad));
    STANCHK(bufs.alloc(&d_out, (size_t)npad));
    STANCHK(bufs.alloc(&d_enc, (size_t)nslots * vstream<s60_t>::STRIDE));
    HIPCHK(ctx, hipMemsetAsync(d_in, 0, (size_t)npad * 8, st_));
    HIPCHK(ctx, hipMemcpyAsync(d_in, in, (size_t)n * 8, hipMemcpyHostToDevice, st_));
    STANCHK(stan_stream_encode(ctx, STAN_VALUE_STREAM_60, nslots, d_in, d_enc, refused));
    hipLaunchKernelGGL(k_from_s60, dim3(nblk(nslots * 64, 256)), dim3(256), 0, st_, nslots, (const s60_t *)d_enc, d_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, st_));
    HIPCHK(ctx, hipStreamSynchronize(st_));
    return STAN_OK;
}

// `reps` sweeps of k_value_stream over K's resident fp64 values (see the kernel): average ms per sweep and the bytes one
// sweep reads (the slots' values: padded slots are streamed like real ones, as the product streams them).
int stan_stream_bench_device(stan_ctx *ctx, stan_matrix *K, int32_t reps, double *avg_ms, int64_t *bytes) {
    hipStream_t st_ = ctx->stream;
    *avg_ms = 0;
    *bytes = (int64_t)K->nslots * 64 * 72;
    if (K->nslices <= 0 || !K->vals64()) return STAN_OK;
    const unsigned grid = nblk(K->nslices, 4);
    dev_scope bufs(ctx);
    double *sink;
    STANCHK(bufs.alloc(&sink, (size_t)grid));
    auto one = [&]() { hipLaunchKernelGGL(k_value_stream, dim3(grid), dim3(256), 0, st_, K->nslices, K->d_slot_ptr, K->vals64(), sink); };
    float ms = 0;
    STANCHK(timed_launches(ctx, 3, 1, reps, one, &ms));
    *avg_ms = ms;
    return STAN_OK;
}

// Time of the SpMV of K streaming its values from `vals` -- a block of the stream kind `precision` names (STAN_PREC_*, or
// STAN_VALUE_STREAM_60: the product the loop will launch on it); any contents, only the addresses
// matter --, median of 3 launches after a warm-up.  Used by the allocation-by-trial of placement.hip.  folded: the block is
// a candidate for a FOLDED stream of that kind (fold.hip): the folded kernel is timed on it.
// self_pair: the gather vector and the product are carved out of the FRONT of the candidate block
// itself instead of the context's vectors -- by construction the same-group (slow) pairing, i.e.
// the reference the search compares the real pairing with (profiles/r02/placement_cross_self_n148.txt).
int stan_spmv_probe(stan_ctx *ctx, stan_matrix *K, const void *vals, size_t bytes, int32_t precision,
                    float *ms_out, bool self_pair, bool folded) {
    *ms_out = 0;
    if (K->nslices <= 0) return STAN_OK;
    // self_pair: the block holds no values yet (only addresses matter to the timing).  The gather vector and the product
    // must fit into the candidate: a stream with few slots per slice (or a large halo) has no self-paired reference --
    // *ms_out stays 0, the search then keeps the fastest real pairing (placement.hip)
    dev_scope bufs(ctx);
    product_args pa{};
    const product_plan P = plan_products(ctx, K, precision, stan_sharded(ctx), false);
    STANCHK(timed_product_setup(ctx, K, P, precision, vals, folded, self_pair ? const_cast<void *>(vals) : nullptr, bytes, bufs, pa));
    if (!pa.x) return STAN_OK;
    // one launch to warm up, then two groups of three launches, the faster group counts
    return timed_launches(ctx, 1, 2, 3, [&]() { launch_product(ctx, K, P, pa); }, ms_out);
}

// ---- the product of a loop that keeps its vectors resident (api_explicit.hip) ---------------------------------------------------
// the never-stopped status words such a loop hands to every product it enqueues: a temporary of `tmp`, filled on the stream
int stan_product_status(stan_ctx *ctx, dev_scope &tmp, int64_t **stt) { return alloc_never_stopped(ctx, tmp, stt, ctx->stream); }

// yf = A^ xf: ONE plain fp64 product on the caller's vectors in the padded full numbering (3 * nslices * 64 doubles each, what
// launch_plain_product takes; A^ = S K S once K->scaled), by the plan a solve under the same options gets.  Rows of padding
// are not stored.  Enqueues only: no allocation, no copy, no synchronisation.  Single rank.
int stan_product_full(stan_ctx *ctx, stan_matrix *K, const double *xf, double *yf, const int64_t *stt) {
    if (ctx->nranks != 1) { ctx->err = "product: single-rank contexts only"; return STAN_E_UNSUPPORTED; }
    launch_plain_product(ctx, K, xf, yf, stt);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
