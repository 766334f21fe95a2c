// lab/cg_lab.inc -- LAB ONLY (make lab, -DSTAN_LAB): host-side lab entry points that need cg.hip's kernels
// (slice-range probe of lab/placement_lab.hip, the in-CG penalty experiment of tools/fold_ab.py).  Included at the
// end of cg.hip under STAN_LAB; the product library never compiles this file.
// lab: time the fp64 SpMV over the slices [s0, s1) only, streaming the values from `vals`
// (lab/placement_lab.hip: where inside a block does a slow block lose its time?)
int stan_spmv_probe_range(stan_ctx *ctx, stan_matrix *K, const double *vals, int32_t s0, int32_t s1,
                          int reps, float *ms_out, int variant, double *xy_region, double *y_region) {
    hipStream_t st_ = ctx->stream;
    *ms_out = 0;
    if (s1 <= s0) return STAN_OK;
    const int64_t npad = (int64_t)K->nslices * 64;
    const int64_t ng = 3 * ((npad > K->nloc + K->nhalo ? npad : K->nloc + K->nhalo));
    dev_scope bufs(ctx);
    double *x, *y, *partial; int64_t *stt; int32_t *list;
    if (xy_region) {   // lab: gather vector and product live inside a block the caller chose
        x = xy_region;
        y = y_region ? y_region : xy_region + ((ng + 511) & ~(int64_t)511);
    } else {
        STANCHK(bufs.alloc(&x, (size_t)ng));
        STANCHK(bufs.alloc(&y, (size_t)ng));
    }
    STANCHK(bufs.alloc(&partial, 2 * (size_t)K->nslices + 2));   // k_spmv_small leaves one partial per slice
    STANCHK(bufs.alloc(&stt, (size_t)T_NSTAT));
    STANCHK(bufs.alloc(&list, (size_t)(s1 - s0)));
    std::vector<int32_t> h((size_t)(s1 - s0));
    for (int32_t i = s0; i < s1; i++) h[i - s0] = i;
    int64_t init[T_NSTAT] = {0x7fffffffffffffffLL, 0x7fffffffffffffffLL, 0, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(stt, init, sizeof(init), hipMemcpyHostToDevice, st_));
    HIPCHK(ctx, hipMemcpyAsync(list, h.data(), h.size() * 4, hipMemcpyHostToDevice, st_));
    hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
    HIPCHK(ctx, hipStreamSynchronize(st_));
    const unsigned grid = nblk(s1 - s0, 4);
    event_bag ev;
    hipEvent_t a = ev.make(), b = ev.make();
    for (int r = 0; r < reps + 2; r++) {
        if (r == 2) hipEventRecord(a, st_);
#define LABV(V) case V: hipLaunchKernelGGL((k_spmv<double, 1, V>), dim3(grid), dim3(256), 0, st_, K->nslices, K->nloc, \
                           K->d_slot_ptr, K->d_rowof, K->d_cols, vals, x, y, partial, stt, (int64_t)1, list, s1 - s0, 0,           \
                           NO_FOLD, NO_COLSTREAM); break;
        switch (variant) { LABV(0) LABV(13) LABV(14) LABV(15) LABV(16) LABV(12) default: LABV(9) }
#undef LABV
    }
    hipEventRecord(b, st_);
    HIPCHK(ctx, hipEventSynchronize(b));
    hipEventElapsedTime(ms_out, a, b);
    *ms_out /= reps;
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
__global__ void k_fill_nt(double *p, int64_t n, double v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) __builtin_nontemporal_store(v, p + i);
}
__global__ void k_fill_scope(double *p, int64_t n, double v, int scope) {   // 0: agent-scope (sc1), 1: system-scope stores
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (scope == 0) __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// the rewrite k_update really does: x = r + beta x (read-modify-write of the gather vector)
template <bool LNT, bool SNT>
__global__ void k_rmw(double *x, const double *r, int64_t n, double beta) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double xo = LNT ? __builtin_nontemporal_load(x + i) : x[i];
        const double ro = LNT ? __builtin_nontemporal_load(r + i) : r[i];
        const double v = ro * 0.0 + 1.0 + beta * (xo - 1.0);   // stays 1.0
        if (SNT) __builtin_nontemporal_store(v, x + i); else x[i] = v;
    }
}
// ping-pong form of the same rewrite: xo = r + beta xi into ANOTHER buffer
template <bool LNT, bool SNT>
__global__ void k_pingpong(double *xo, const double *xi, const double *r, int64_t n, double beta) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double xv = LNT ? __builtin_nontemporal_load(xi + i) : xi[i];
        const double ro = LNT ? __builtin_nontemporal_load(r + i) : r[i];
        const double v = ro * 0.0 + 1.0 + beta * (xv - 1.0);
        if (SNT) __builtin_nontemporal_store(v, xo + i); else xo[i] = v;
    }
}
__global__ void k_read_only(const double *p, int64_t n, double *sink) {
    double a = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a += p[i];
    if (a == 0.123456789) sink[0] = a;
}
// lab: what makes the SpMV slower inside the CG than back to back?  mode 0: launches back to back;
// 1: the gather vector is rewritten (k_fill, plain stores like k_update) before every launch;
// 2: plus a k_step-like pass over four other vectors in between; 3: only that pass (x untouched).
// Events bracket each product alone.  out_ms [4].
int stan_spmv_incg_lab(stan_ctx *ctx, stan_matrix *K, int reps, double *out_ms) {
    hipStream_t st_ = ctx->stream;
    STANCHK(stan_cg_workspace(ctx, K));
    const int64_t ng = ctx->ws.ng, n3 = 3 * K->nloc;
    double *x = ctx->ws.p, *y = ctx->ws.v;
    dev_scope bufs(ctx);
    double *partial; int64_t *stt;
    STANCHK(bufs.alloc(&partial, 2 * (size_t)nblk(K->nslices, 4) + 16));
    STANCHK(bufs.alloc(&stt, (size_t)T_NSTAT));
    int64_t init[T_NSTAT] = {0x7fffffffffffffffLL, 0x7fffffffffffffffLL, 0, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(stt, init, sizeof(init), hipMemcpyHostToDevice, st_));
    hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
    for (double *q : {ctx->ws.xb[1], ctx->ws.r, ctx->ws.w})
        hipLaunchKernelGGL(k_fill, dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, q, n3, 0.5);
    hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, ctx->ws.xb[0], ng, 1.0);
    for (int mode = 0; mode < 15; mode++) {
        event_bag ev;
        std::vector<hipEvent_t> e;
        for (int r = 0; r < reps + 2; r++) {
            if (mode == 1 || mode == 2) hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
            if (mode == 2 || mode == 3) {   // the traffic of k_step: x' = x + a p, r -= a v  (reads 4, writes 2)
                step_args a;
                a.n3 = n3; a.k = 1; a.sc = nullptr; a.st = stt; a.xcur = ctx->ws.xb[0]; a.xnext = ctx->ws.xb[1];
                a.r = ctx->ws.r; a.p = ctx->ws.w; a.v = y; a.bh = ctx->ws.bh; a.partial = partial; a.w = ctx->ws.w;
                a.merit = 0; a.refresh = 0; a.defer_x = 0; a.fold = NO_FOLD;
                double *scal; STANCHK(bufs.alloc(&scal, (size_t)S_NSCAL));
                double hs[S_NSCAL] = {0}; hs[S_VMV] = 1.0; hs[S_RHO0] = hs[S_RHO1] = 1e-30;
                HIPCHK(ctx, hipMemcpyAsync(scal, hs, sizeof(hs), hipMemcpyHostToDevice, st_));
                a.sc = scal;
                hipLaunchKernelGGL(k_step<false>, dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, a);
            }
            // 4: rewritten with non-temporal stores; 5: rewritten (plain), then read once front to back
            // by a streaming kernel (does a read pull it into the memory-side cache?); 6: like 5 with nt stores
            if (mode == 4 || mode == 6) hipLaunchKernelGGL(k_fill_nt, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
            if (mode == 5) hipLaunchKernelGGL(k_fill, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0);
            // 9-12: read-modify-write like k_update: plain/plain, plain load + nt store, nt load + nt store, nt load + plain store
            if (mode == 9) hipLaunchKernelGGL((k_rmw<false, false>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, x, ctx->ws.r, n3, 0.5);
            if (mode == 10) hipLaunchKernelGGL((k_rmw<false, true>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, x, ctx->ws.r, n3, 0.5);
            if (mode == 11) hipLaunchKernelGGL((k_rmw<true, true>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, x, ctx->ws.r, n3, 0.5);
            if (mode == 12) hipLaunchKernelGGL((k_rmw<true, false>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, x, ctx->ws.r, n3, 0.5);
            // 7 / 8: rewritten with agent-scope (sc1, write-through) / system-scope stores
            if (mode == 7 || mode == 8) hipLaunchKernelGGL(k_fill_scope, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, x, ng, 1.0, mode - 7);
            if (mode == 5 || mode == 6) hipLaunchKernelGGL(k_read_only, dim3(vec_grid(ng)), dim3(VEC_T), 0, st_, (const double *)x, ng, partial);
            // 13 / 14: the rewrite goes to the OTHER of two buffers (nt load + nt store / plain load + nt store)
            double *xg = x;
            if (mode == 13 || mode == 14) {
                double *xa = (r & 1) ? x : ctx->ws.xb[0], *xi = (r & 1) ? ctx->ws.xb[0] : x;
                if (mode == 13) hipLaunchKernelGGL((k_pingpong<true, true>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, xa, xi, ctx->ws.r, n3, 0.5);
                else hipLaunchKernelGGL((k_pingpong<false, true>), dim3(vec_grid(n3)), dim3(VEC_T), 0, st_, xa, xi, ctx->ws.r, n3, 0.5);
                xg = xa;
            }
            hipEvent_t a0 = ev.make(), b0 = ev.make();
            hipEventRecord(a0, st_);
            hipLaunchKernelGGL((k_spmv<double, 1, 9>), dim3(nblk(K->nslices, 4)), dim3(256), 0, st_, K->nslices, K->nloc,
                               K->d_slot_ptr, K->d_rowof, K->d_cols, K->vals64(), xg, y, partial, stt, (int64_t)1,
                               (const int32_t *)nullptr, K->nslices, 0, NO_FOLD,
                               NO_COLSTREAM);
            hipEventRecord(b0, st_);
            if (r >= 2) { e.push_back(a0); e.push_back(b0); }
        }
        HIPCHK(ctx, hipStreamSynchronize(st_));
        double tot = 0;
        for (size_t i = 0; i + 1 < e.size(); i += 2) { float f = 0; hipEventElapsedTime(&f, e[i], e[i + 1]); tot += f; }
        out_ms[mode] = tot / reps;
    }
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
