// cg_multi.inc -- the kernels of the batched CG (stan_cg_multi_device): M load cases in one loop over ONE pass of K
// Part of cg.hip (included there, inside its anonymous namespace, behind the product and vector kernels whose helpers it
// uses; not a translation unit of its own).  The reference knows one load vector: no counterpart there.
//
// Every column is alglib's loop on its own data, with its own scalars sc[c][S_NSCAL], its own status words
// stt[c][T_NSTAT] and its own stop; the columns share the pass over K and the launches, nothing else.  The loop's
// vectors are INTERLEAVED: element i of column c at [i*M + c] -- the gather of one block column is 3M contiguous doubles,
// a thread of a vector kernel loads and stores M contiguous doubles per element.
// Bits: column c is computed by the expressions of the single solve's kernels (STAN_SPMV_BLOCK, k_step, k_refresh,
// k_update, k_init), element i by the thread and the block that get it there (same grids, same strides), its partial
// sums are added by sum_partials<1> / sum_partials<2> as there -- so every sum of a column has the bits the single
// solve gives it, whatever M is and whatever the other columns hold.  A column that has stopped is frozen: no kernel
// stores to any of its vectors, scalars or status words again.

template <int M> struct colvec { typedef double type __attribute__((ext_vector_type(M))); };
template <> struct colvec<1> { typedef double type; };
// the M columns of one element (q = base + i*M: M*8-byte aligned)
template <int M, bool NT>
__device__ __forceinline__ void ld_cols(const double *q, double o[M]) {
    using V = typename colvec<M>::type;
    V t;
    if constexpr (NT) t = __builtin_nontemporal_load((const V *)q);
    else t = *(const V *)q;
    if constexpr (M == 1) o[0] = t;
    else {
#pragma unroll
        for (int m = 0; m < M; m++) o[m] = t[m];
    }
}
// ALL: every column of the group is live -- one wide store; otherwise only the live columns' words are touched
template <int M, bool NT, bool ALL>
__device__ __forceinline__ void st_cols(double *q, const double o[M], unsigned act) {
    if constexpr (ALL) {
        using V = typename colvec<M>::type;
        V t;
        if constexpr (M == 1) t = o[0];
        else {
#pragma unroll
            for (int m = 0; m < M; m++) t[m] = o[m];
        }
        if constexpr (NT) __builtin_nontemporal_store(t, (V *)q);
        else *(V *)q = t;
    } else {
#pragma unroll
        for (int m = 0; m < M; m++)
            if ((act >> m) & 1u) {
                if constexpr (NT) __builtin_nontemporal_store(o[m], q + m);
                else q[m] = o[m];
            }
    }
}
template <int M> constexpr unsigned ALL_COLS = (1u << M) - 1u;   // every column of the group live

// The folded reduction of M columns: column c's partials lie at partial[c*pstride + i*NV + j]; the block that drew the
// last ticket adds each LIVE column's with sum_partials<NV> (the single solve's order) into sc[c][slot + j].
template <int M, int NV>
__device__ __forceinline__ void fold_finish_cols(const fold_args &f, const double *partial, int64_t pstride, unsigned act,
                                                 double *sc, int slot, double *sh) {
#pragma unroll 1
    for (int c = 0; c < M; c++) {
        if (!((act >> c) & 1u)) continue;   // block-uniform
        double r[NV];
        sum_partials<NV>(partial + c * pstride, f.np, sh, r);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < NV; j++) sc[c * S_NSCAL + slot + j] = r[j];   // read by the NEXT kernel
        }
    }
    if (threadIdx.x <= FOLD_SUB)
        __hip_atomic_store(f.counter + threadIdx.x * FOLD_LINE, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the product: y_c = A x_c for the M interleaved columns, one pass over K ------------------------------------------
// k_spmv<double, DOT, 9> with M accumulator triples per lane: the same slot walk, the block expression of
// STAN_SPMV_BLOCK per column, the same grid and workgroup mapping, one p.Ap partial per column and workgroup.
// refresh = 0: the product of iteration kiter's step (a column is skipped when stopped(st_c, kiter)); the literal
// refresh product has the same rule (a column that k_step has just ended with -5 / -4 is caught by k_refresh_m).
template <int M, int DOT>
__global__ void __launch_bounds__(256)
k_spmm(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
       const int32_t *__restrict__ cols, const double *__restrict__ vals, const double *__restrict__ x,
       double *__restrict__ y, double *partial, int64_t pstride, double *sc, const int64_t *st, int64_t kiter,
       fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < M; c++)
        if (!stopped(st + c * T_NSTAT, kiter)) act |= 1u << c;
    if (!act) return;
    constexpr bool NT = true;
    const int lane = threadIdx.x & 63;
    const int64_t slice = xcd_chunked<32>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    double y0[M], y1[M], y2[M];
#pragma unroll
    for (int m = 0; m < M; m++) y0[m] = y1[m] = y2[m] = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        walk_slots<NT, 2, 9 * 64>(cs, cols, slice, lane, k0, k0, k1, vals, [&](int64_t c, const double *vp) {
            double a[9];
            load9<NT, double>(vp, a);
            double x0[M], x1[M], x2[M];
            ld_cols<M, false>(x + (3 * c) * M, x0);
            ld_cols<M, false>(x + (3 * c + 1) * M, x1);
            ld_cols<M, false>(x + (3 * c + 2) * M, x2);
#pragma unroll
            for (int m = 0; m < M; m++) {
                y0[m] += a[0] * x0[m] + a[1] * x1[m] + a[2] * x2[m];
                y1[m] += a[3] * x0[m] + a[4] * x1[m] + a[5] * x2[m];
                y2[m] += a[6] * x0[m] + a[7] * x1[m] + a[8] * x2[m];
            }
        });
        if (row < nloc) {   // A p is read exactly once, by k_step_m
            if (act == ALL_COLS<M>) {
                st_cols<M, NT, true>(y + (3 * row) * M, y0, act);
                st_cols<M, NT, true>(y + (3 * row + 1) * M, y1, act);
                st_cols<M, NT, true>(y + (3 * row + 2) * M, y2, act);
            } else {
                st_cols<M, NT, false>(y + (3 * row) * M, y0, act);
                st_cols<M, NT, false>(y + (3 * row + 1) * M, y1, act);
                st_cols<M, NT, false>(y + (3 * row + 2) * M, y2, act);
            }
        }
    }
    if (DOT) {
        double d[M];
#pragma unroll
        for (int m = 0; m < M; m++) d[m] = 0;
        if (slice < nslices && row < nloc) {
            double x0[M], x1[M], x2[M];
            ld_cols<M, false>(x + (3 * row) * M, x0);
            ld_cols<M, false>(x + (3 * row + 1) * M, x1);
            ld_cols<M, false>(x + (3 * row + 2) * M, x2);
#pragma unroll
            for (int m = 0; m < M; m++) d[m] = y0[m] * x0[m] + y1[m] * x1[m] + y2[m] * x2[m];
        }
#pragma unroll
        for (int m = 0; m < M; m++) {
            if (!((act >> m) & 1u)) continue;   // block-uniform
            const double t = block_sum(d[m], sh);
            if (threadIdx.x == 0) st_agent(partial + m * pstride + blockIdx.x, t);
        }
        if (fold_arrive(fold, &sh_last)) fold_finish_cols<M, 1>(fold, partial, pstride, act, sc, S_VMV, sh);
    }
}

// ---- k_init for M columns: b^_c = S F_c (free DOFs; F: [..][n_red], column c at F + c*n_red), x0 = 0, r = p = b^ ------
template <int M>
__global__ void __launch_bounds__(VEC_T)
k_init_m(int64_t n3, int64_t n_red, const int32_t *red, const double *F, const double *s, double *bh, double *x0, double *r,
         double *p, double *partial, int64_t pstride, double *sc, fold_args fold) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    double acc[M];
#pragma unroll
    for (int m = 0; m < M; m++) acc[m] = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[i];
        const double si = s[i];
        double b[M], z[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            b[m] = rd == -1 ? 0.0 : si * F[m * n_red + i - rd];
            z[m] = 0.0;
            acc[m] += b[m] * b[m];
        }
        st_cols<M, false, true>(bh + i * M, b, 0);
        st_cols<M, false, true>(x0 + i * M, z, 0);
        st_cols<M, false, true>(r + i * M, b, 0);
        st_cols<M, false, true>(p + i * M, b, 0);
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
        const double t = block_sum(acc[m], sh);
        if (threadIdx.x == 0) st_agent(partial + m * pstride + blockIdx.x, t);
    }
    if (fold_arrive(fold, &sh_last)) fold_finish_cols<M, 1>(fold, partial, pstride, ALL_COLS<M>, sc, S_VMV, sh);
}
// k_init_scalars per column (thread c): bnorm, first residual test, rho, prevmf
template <int M>
__global__ void __launch_bounds__(64) k_init_scalars_m(double *sc_, int64_t *st_, double epsf) {
    if (threadIdx.x >= M) return;
    double *sc = sc_ + threadIdx.x * S_NSCAL;
    int64_t *st = st_ + threadIdx.x * T_NSTAT;
    const double r2 = sc[S_VMV];
    sc[S_BNORM] = sqrt(r2);
    sc[S_RHO0] = r2; sc[S_RHO1] = r2;
    sc[S_PMF0] = 0.0; sc[S_PMF1] = 0.0;
    sc[S_R2OUT] = r2;
    st[T_ITER_A] = 0x7fffffffffffffffLL;
    st[T_ITER_B] = 0x7fffffffffffffffLL;
    st[T_TYPE] = 0; st[T_ITERS] = 0; st[T_XSEL] = 0;
    if (!isfinite(r2)) { st[T_TYPE] = -4; st[T_ITER_A] = 0; }
    else if (sqrt(r2) <= epsf * sqrt(r2)) { st[T_TYPE] = 1; st[T_ITER_A] = 0; }
}

// ---- k_step for M columns ----------------------------------------------------------------------------------------------
struct mstep_args {
    int64_t n3, k;
    double *sc;           // [M][S_NSCAL]
    int64_t *st;          // [M][T_NSTAT]
    const double *xcur;
    double *xnext;
    double *r;
    const double *p, *v, *bh;
    double *partial;      // [M][pstride]: per block r2, merit
    int64_t pstride;
    int merit;            // 0: the merit-function stop is off, skip its sum (and the b^ read)
    int refresh;          // 0: r -= a v and the sums; 1: only x' is formed here (r from the literal second product)
    fold_args fold;
};
template <int M, bool ALL>
__device__ __forceinline__ void step_cols(const mstep_args &a, const double alpha[M], unsigned act, double s_r2[M], double s_mf[M]) {
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < a.n3; i += stride) {
        double pi[M], xc[M], cx[M];
        ld_cols<M, true>(a.p + i * M, pi);
        ld_cols<M, true>(a.xcur + i * M, xc);
#pragma unroll
        for (int m = 0; m < M; m++) cx[m] = xc[m] + alpha[m] * pi[m];
        st_cols<M, true, ALL>(a.xnext + i * M, cx, act);
        if (a.refresh == 0) {
            double ri[M], vi[M], cr[M];
            ld_cols<M, true>(a.r + i * M, ri);
            ld_cols<M, true>(a.v + i * M, vi);
#pragma unroll
            for (int m = 0; m < M; m++) {
                cr[m] = ri[m] - alpha[m] * vi[m];
                s_r2[m] += cr[m] * cr[m];
            }
            st_cols<M, true, ALL>(a.r + i * M, cr, act);
            if (a.merit) {
                double b[M];
                ld_cols<M, false>(a.bh + i * M, b);
#pragma unroll
                for (int m = 0; m < M; m++) s_mf[m] -= (cr[m] + b[m]) * cx[m];
            }
        }
    }
}
template <int M>
__global__ void __launch_bounds__(VEC_T) k_step_m(mstep_args a) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    double alpha[M];
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < M; c++) {
        alpha[c] = 0;
        int64_t *st = a.st + c * T_NSTAT;
        const double *sc = a.sc + c * S_NSCAL;
        if (stopped(st, a.k)) continue;
        const double vmv = sc[S_VMV];
        const double rho = sc[S_RHO0 + (a.k & 1)];
        int bad = 0;
        if (!isfinite(vmv) || vmv <= 0) bad = isfinite(vmv) ? -5 : -4;
        const double al = rho / vmv;
        if (!bad && !isfinite(al)) bad = -4;
        if (bad) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st[T_TYPE] = bad;
                st[T_ITERS] = a.k;
                st[T_XSEL] = (a.k - 1) & 1;  // rx of the previous iteration
                st[T_ITER_B] = a.k;
            }
            continue;
        }
        alpha[c] = al;
        act |= 1u << c;
    }
    if (!act) return;
    double s_r2[M], s_mf[M];
#pragma unroll
    for (int m = 0; m < M; m++) s_r2[m] = s_mf[m] = 0;
    if (act == ALL_COLS<M>) step_cols<M, true>(a, alpha, act, s_r2, s_mf);
    else step_cols<M, false>(a, alpha, act, s_r2, s_mf);
    if (a.refresh != 1) {
#pragma unroll
        for (int m = 0; m < M; m++) {
            if (!((act >> m) & 1u)) continue;   // block-uniform
            const double t0 = block_sum(s_r2[m], sh);
            const double t1 = block_sum(s_mf[m], sh);
            if (threadIdx.x == 0) {
                st_agent(a.partial + m * a.pstride + 2 * blockIdx.x, t0);
                st_agent(a.partial + m * a.pstride + 2 * blockIdx.x + 1, t1);
            }
        }
        if (fold_arrive(a.fold, &sh_last)) fold_finish_cols<M, 2>(a.fold, a.partial, a.pstride, act, a.sc, S_R2NEW, sh);
    }
}

// ---- k_refresh for M columns: r = b^ - A^ cx, merit = sum (mv - 2 b^) cx ------------------------------------------------
template <int M, bool ALL>
__device__ __forceinline__ void refresh_cols(int64_t n3, const double *bh, const double *mv, const double *cx, double *r,
                                             unsigned act, double s_r2[M], double s_mf[M]) {
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        double b[M], m_[M], x[M], cr[M];
        ld_cols<M, false>(bh + i * M, b);
        ld_cols<M, false>(mv + i * M, m_);
        ld_cols<M, false>(cx + i * M, x);
#pragma unroll
        for (int m = 0; m < M; m++) {
            cr[m] = b[m] - m_[m];
            s_r2[m] += cr[m] * cr[m];
            s_mf[m] += (m_[m] - 2 * b[m]) * x[m];
        }
        st_cols<M, true, ALL>(r + i * M, cr, act);
    }
}
template <int M>
__global__ void __launch_bounds__(VEC_T)
k_refresh_m(int64_t n3, int64_t k, double *sc, const int64_t *st_, const double *bh, const double *mv, const double *cx,
            double *r, double *partial, int64_t pstride, fold_args fold) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < M; c++) {
        const int64_t *st = st_ + c * T_NSTAT;
        if (!(st[T_ITER_A] < k || st[T_ITER_B] <= k)) act |= 1u << c;
    }
    if (!act) return;
    double s_r2[M], s_mf[M];
#pragma unroll
    for (int m = 0; m < M; m++) s_r2[m] = s_mf[m] = 0;
    if (act == ALL_COLS<M>) refresh_cols<M, true>(n3, bh, mv, cx, r, act, s_r2, s_mf);
    else refresh_cols<M, false>(n3, bh, mv, cx, r, act, s_r2, s_mf);
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (!((act >> m) & 1u)) continue;   // block-uniform
        const double t0 = block_sum(s_r2[m], sh);
        const double t1 = block_sum(s_mf[m], sh);
        if (threadIdx.x == 0) {
            st_agent(partial + m * pstride + 2 * blockIdx.x, t0);
            st_agent(partial + m * pstride + 2 * blockIdx.x + 1, t1);
        }
    }
    if (fold_arrive(fold, &sh_last)) fold_finish_cols<M, 2>(fold, partial, pstride, act, sc, S_R2NEW, sh);
}

// ---- k_update for M columns: each column's decisions from its own words + p = r + beta p ---------------------------------
template <int M, bool ALL>
__device__ __forceinline__ void update_cols(int64_t n3, const double *r, double *p, const double beta[M], unsigned act) {
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        double po[M], ri[M], pn[M];
        ld_cols<M, true>(p + i * M, po);
        ld_cols<M, true>(r + i * M, ri);
#pragma unroll
        for (int m = 0; m < M; m++) pn[m] = ri[m] + beta[m] * po[m];
        st_cols<M, true, ALL>(p + i * M, pn, act);
    }
}
template <int M>
__global__ void __launch_bounds__(VEC_T)
k_update_m(int64_t n3, int64_t k, double *sc_, int64_t *st_, double epsf, int64_t maxits, int64_t its_before_restart,
           int merit_stop, const double *r, double *p) {
    double beta[M];
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < M; c++) {
        beta[c] = 0;
        double *sc = sc_ + c * S_NSCAL;
        int64_t *st = st_ + c * T_NSTAT;
        if (st[T_ITER_A] < k || st[T_ITER_B] <= k) continue;
        const double r2 = sc[S_R2NEW], merit = sc[S_MERIT];
        const double rho = sc[S_RHO0 + (k & 1)], prevmf = sc[S_PMF0 + (k & 1)];
        const double bnorm = sc[S_BNORM];
        int type = 0;
        int64_t xsel = k & 1;  // cx lives in buffer k&1
        if (sqrt(r2) <= epsf * bnorm) type = 1;
        else if (k >= maxits && maxits > 0) type = 5;
        else if (merit_stop && merit >= prevmf) { type = 7; xsel = (k - 1) & 1; }
        double be = 0;
        const bool restart = (k % its_before_restart) == 0;
        if (!type && !restart) {
            be = r2 / rho;
            if (!isfinite(be)) { type = -4; }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            sc[S_R2OUT] = r2;
            if (type) {
                st[T_TYPE] = type;
                st[T_ITERS] = k;
                st[T_XSEL] = xsel;
                st[T_ITER_A] = k;
            } else {
                sc[S_RHO0 + ((k + 1) & 1)] = r2;
                sc[S_PMF0 + ((k + 1) & 1)] = merit;
            }
        }
        if (type) continue;
        beta[c] = be;
        act |= 1u << c;
    }
    if (!act) return;
    if (act == ALL_COLS<M>) update_cols<M, true>(n3, r, p, beta, act);
    else update_cols<M, false>(n3, r, p, beta, act);
}

// U_c[d - red[d]] = s_d * x^_c,d on the free DOFs, every column from the buffer its own T_XSEL names
template <int M>
__global__ void __launch_bounds__(VEC_T)
k_result_m(int64_t n3, int64_t n_red, const int32_t *red, const double *s, const double *xa, const double *xb,
           const int64_t *st, double *U) {
    unsigned sel = 0;
#pragma unroll
    for (int c = 0; c < M; c++)
        if (st[c * T_NSTAT + T_XSEL] & 1) sel |= 1u << c;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[i];
        if (rd == -1) continue;
        double a[M], b[M];
        ld_cols<M, false>(xa + i * M, a);
        ld_cols<M, false>(xb + i * M, b);
        const double si = s[i];
#pragma unroll
        for (int m = 0; m < M; m++) U[m * n_red + i - rd] = si * (((sel >> m) & 1u) ? b[m] : a[m]);
    }
}
