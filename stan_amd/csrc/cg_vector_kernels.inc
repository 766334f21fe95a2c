// cg_vector_kernels.inc -- the vector kernels of the CG loop: k_step, k_refresh, k_update, k_vec_sr (single-reduction form), result / expand / compress
// Part of cg.hip (included there, inside its anonymous namespace; not a translation unit of its own): split out in
// round 4 so that each piece can be read on its own.  The reference has no counterpart of these kernels beyond the
// calls they replace: alglib.lincgsolvesparse / sparsesmv behind SolverFunctions.LinearSolver_CG (SolverFunctions.cs:270-330).

// ---- CG step kernels ----------------------------------------------------------------------------
__device__ __forceinline__ double vld_ro(const double *q) {
    return __builtin_nontemporal_load(q);
}
__device__ __forceinline__ double vld_rmw(const double *q) {
    return __builtin_nontemporal_load(q);
}

struct step_args {
    int64_t n3;           // 3 * owned block rows
    int64_t k;            // iteration number (1-based)
    double *sc;           // scalars
    int64_t *st;          // status
    const double *xcur;   // rx
    double *xnext;        // cx
    double *r;            // r (in), cr (out)
    const double *p;
    const double *v;      // A^ p
    const double *bh;
    double *partial;      // [blocks][2]: r2, merit
    const double *w;      // A^ x (fused refresh)
    int merit;            // 0: the merit-function stop is off, skip its sum (and the b^ read)
    int refresh;          // 0: r -= a v; 1: only cx is formed here (r from a second SpMV);
                          // 2: fused refresh, r = b^ - (w + a v) with w = A^ x from the same pass
    int defer_x;          // 1: x' = x + a p is formed by k_update (one read of p for both updates); only
                          //    when the merit sum is off and the iteration needs no x' before k_update
    fold_args fold;       // r.r and the merit sum are added up by the last block (-> sc[S_R2NEW..])
    red_src rs_vmv;       // where p.Ap is found (p2p_device.h)
};

template <bool RNT>
__global__ void __launch_bounds__(VEC_T) k_step(step_args a) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    if (stopped(a.st, a.k)) { if (a.refresh != 1) fold_skip(a.fold); return; }
    double vmv_[1];
    red_get<1>(a.sc + S_VMV, a.rs_vmv, vmv_, sh);
    const double vmv = vmv_[0];
    const double rho = a.sc[S_RHO0 + (a.k & 1)];
    int bad = 0;
    if (!isfinite(vmv) || vmv <= 0) bad = isfinite(vmv) ? -5 : -4;
    const double alpha = rho / vmv;
    if (!bad && !isfinite(alpha)) bad = -4;
    if (bad) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.st[T_TYPE] = bad;
            a.st[T_ITERS] = a.k;
            a.st[T_XSEL] = (a.k - 1) & 1;  // rx of the previous iteration
            a.st[T_ITER_B] = a.k;
        }
        if (a.refresh != 1) fold_skip(a.fold);
        return;
    }
    double s_r2 = 0, s_mf = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < a.n3; i += stride) {
        double cx = 0;
        if (!a.defer_x) {
            const double pi = __builtin_nontemporal_load(a.p + i);
            cx = __builtin_nontemporal_load(a.xcur + i) + alpha * pi;
            __builtin_nontemporal_store(cx, a.xnext + i);
        }
        if (a.refresh == 0) {
            const double cr = vld_rmw(a.r + i) - alpha * vld_ro(a.v + i);
            if (RNT) __builtin_nontemporal_store(cr, a.r + i);
            else a.r[i] = cr;
            s_r2 += cr * cr;
            if (a.merit) s_mf -= (cr + a.bh[i]) * cx;
        } else if (a.refresh == 2) {
            const double b = a.bh[i];
            const double mv = a.w[i] + alpha * a.v[i];  // A^ (x + a p)
            const double cr = b - mv;
            if (RNT) __builtin_nontemporal_store(cr, a.r + i);
            else a.r[i] = cr;
            s_r2 += cr * cr;
            if (a.merit) s_mf += (mv - 2 * b) * cx;
        }
    }
    if (a.refresh != 1) {
        const double t0 = block_sum(s_r2, sh);
        const double t1 = block_sum(s_mf, sh);
        if (threadIdx.x == 0) {
            st_agent(a.partial + 2 * blockIdx.x, t0);
            st_agent(a.partial + 2 * blockIdx.x + 1, t1);
        }
        if (a.fold.counter && fold_arrive(a.fold, &sh_last)) fold_finish<2>(a.fold, a.partial, sh);
    }
}

// refresh iterations: r = b^ - A^ cx, merit = sum (mv - 2 b^) cx
__global__ void __launch_bounds__(VEC_T)
k_refresh(int64_t n3, int64_t k, const int64_t *st, const double *bh, const double *mv,
          const double *cx, double *r, double *partial, fold_args fold) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    if (st[T_ITER_A] < k || st[T_ITER_B] <= k) { fold_skip(fold); return; }
    double s_r2 = 0, s_mf = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        const double b = bh[i], m = mv[i];
        const double cr = b - m;
        __builtin_nontemporal_store(cr, r + i);
        s_r2 += cr * cr;
        s_mf += (m - 2 * b) * cx[i];
    }
    const double t0 = block_sum(s_r2, sh);
    const double t1 = block_sum(s_mf, sh);
    if (threadIdx.x == 0) {
        st_agent(partial + 2 * blockIdx.x, t0);
        st_agent(partial + 2 * blockIdx.x + 1, t1);
    }
    if (fold.counter && fold_arrive(fold, &sh_last)) fold_finish<2>(fold, partial, sh);
}

// decisions of the iteration + p = r + beta p
// RING (STAN_OPT_CG_X_RING, x_ring.h): p is p_k in its slot of the ring and stays; p_{k+1} goes to `pnext`, the next slot, and
// alpha_k to `alpha_out`, its place next to the ring.  x is not touched: k_xring_flush forms it once per window.
template <bool PNT, bool RING>
__global__ void __launch_bounds__(VEC_T)
k_update(int64_t n3, int64_t k, double *sc, int64_t *st, double epsf, int64_t maxits,
         int64_t its_before_restart, int merit_stop, const double *r, double *p,
         const double *xcur, double *xnext /* non-null: the deferred x' = x + a p of this iteration */,
         red_src rs_r2, red_src rs_vmv, double *pnext, double *alpha_out) {
    __shared__ double sh[4];
    if (st[T_ITER_A] < k || st[T_ITER_B] <= k) return;
    double t2[2];
    red_get<2>(sc + S_R2NEW, rs_r2, t2, sh);   // r.r, merit sum
    const double r2 = t2[0], merit = t2[1];
    const double rho = sc[S_RHO0 + (k & 1)], prevmf = sc[S_PMF0 + (k & 1)];
    const double bnorm = sc[S_BNORM];
    int type = 0;
    int64_t xsel = k & 1;  // cx lives in buffer k&1
    if (sqrt(r2) <= epsf * bnorm) type = 1;
    else if (k >= maxits && maxits > 0) type = 5;
    else if (merit_stop && merit >= prevmf) { type = 7; xsel = (k - 1) & 1; }
    double beta = 0;
    const bool restart = (k % its_before_restart) == 0;
    if (!type && !restart) {
        beta = r2 / rho;
        if (!isfinite(beta)) { type = -4; }
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
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    // alpha of this iteration, as k_step formed it (same operands, same bits)
    double alpha = 0.0;
    if (RING || xnext) {   // block-uniform
        double v1[1];
        red_get<1>(sc + S_VMV, rs_vmv, v1, sh);
        alpha = rho / v1[0];
    }
    if constexpr (RING) {
        // the term alpha_k p_k is pending from here on, whether the iteration stops (types 1, 5, -4 select x_k) or not
        if (blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
        if (type) return;
        for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
            const double po = PNT ? vld_rmw(p + i) : p[i];
            const double pn = (PNT ? vld_ro(r + i) : r[i]) + beta * po;
            if (PNT) __builtin_nontemporal_store(pn, pnext + i);
            else pnext[i] = pn;
        }
        return;
    }
    if (type) {
        // the iteration that stops (types 1, 5, -4 select x' = buffer k & 1) still owes its x'
        if (xnext && xsel == (k & 1))
            for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride)
                __builtin_nontemporal_store(__builtin_nontemporal_load(xcur + i) + alpha * __builtin_nontemporal_load(p + i), xnext + i);
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride)
    {
        // PNT: p is read, rewritten and not touched again until the next product gathers it: take it
        // past the caches both ways (a non-temporal store to a line a plain load has just brought
        // into L2 only dirties that line: lab modes 9-12 of tools/fold_ab.py)
        const double po = PNT ? vld_rmw(p + i) : p[i];
        const double pn = (PNT ? vld_ro(r + i) : r[i]) + beta * po;
        if (PNT) __builtin_nontemporal_store(pn, p + i);
        else p[i] = pn;
        if (xnext) __builtin_nontemporal_store(vld_ro(xcur + i) + alpha * po, xnext + i);
    }
}

// ---- the iterate from the ring of directions (STAN_OPT_CG_X_RING, x_ring.h) ------------------------
// x += the pending terms alpha_j p_j, j = first ... last, in iteration order: one fused multiply-add per term, as k_update
// forms x' = x + alpha p one iteration at a time.  In front of a refresh iteration k (k > 0): the terms are the host's
// (everything before k ran unless the solve has stopped: then nothing is done), and T_FLUSHED records the last one.
// Closing (k == 0, behind the loop): the terms between T_FLUSHED and the iterate the status words name.
struct xring_args {
    int64_t n3, ng;         // owned length; length of a slot
    int64_t k;              // the iteration this flush stands in front of; 0: the closing flush
    int64_t first, last;    // k > 0: the terms
    int64_t last_enqueued;  // k == 0: the last iteration of the loop (the hard cap's iterate)
    int W;
    const double *ring;     // [W + 1][ng]
    const double *alpha;    // [W + 1]
    double *x;
    int64_t *st;
};
template <int N>
__device__ __forceinline__ void xring_sum(const xring_args &a, int64_t first) {
    const double *q[N];
    double al[N];
#pragma unroll
    for (int m = 0; m < N; m++) {
        const int s = xring_slot(first + m, a.W);
        q[m] = a.ring + (int64_t)s * a.ng;
        al[m] = a.alpha[s];
    }
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < a.n3; i += stride) {
        double pv[N];
#pragma unroll
        for (int m = 0; m < N; m++) pv[m] = __builtin_nontemporal_load(q[m] + i);
        double x = __builtin_nontemporal_load(a.x + i);
#pragma unroll
        for (int m = 0; m < N; m++) x = __builtin_fma(al[m], pv[m], x);
        __builtin_nontemporal_store(x, a.x + i);
    }
}
__global__ void __launch_bounds__(VEC_T) k_xring_flush(xring_args a) {
    int64_t first = a.first, last = a.last;
    if (a.k > 0) {
        if (stopped(a.st, a.k)) return;
    } else {
        first = a.st[T_FLUSHED] + 1;
        last = xring_final_iterate(a.st[T_TYPE], a.st[T_ITERS], a.st[T_XSEL], a.last_enqueued);
    }
    const int64_t n = last - first + 1;   // <= W <= XRING_MAX_W (xring_flush_due)
    if (n <= 0 || n > XRING_MAX_W) return;
    switch ((int)n) {
#define XRING_CASE(N) case N: xring_sum<N>(a, first); break;
        XRING_CASE(1) XRING_CASE(2) XRING_CASE(3) XRING_CASE(4) XRING_CASE(5) XRING_CASE(6) XRING_CASE(7) XRING_CASE(8)
        XRING_CASE(9) XRING_CASE(10) XRING_CASE(11) XRING_CASE(12) XRING_CASE(13) XRING_CASE(14) XRING_CASE(15) XRING_CASE(16)
#undef XRING_CASE
    }
    // (read by the closing flush only: a later kernel)
    if (a.k > 0 && blockIdx.x == 0 && threadIdx.x == 0) a.st[T_FLUSHED] = last;
}

// ---- single-reduction CG (Chronopoulos-Gear), STAN_OPT_CG_SINGLE_REDUCE --------------------------
// Same iterates as the classic loop in exact arithmetic, ONE reduction point per iteration:
//   w_k = A r_k,  gamma_k = r_k.r_k,  delta_k = r_k.w_k          (the SpMV, both sums in its epilogue)
//   beta_k = gamma_k / gamma_{k-1},   p_k.A p_k = delta_k - beta_k gamma_k / alpha_{k-1},
//   alpha_k = gamma_k / p_k.A p_k
//   p = r + beta p,  s = w + beta s (= A p),  x' = x + alpha p,  r' = r - alpha s
// Per iteration: this kernel + one SpMV (+ ONE all-reduce of 3 doubles when sharded) instead of
// SpMV, all-reduce, step, all-reduce, update.  Iteration k's kernel first takes the decisions of
// iteration k-1 (its residual norm and merit value arrived with the last reduction), with the
// codes and the "previous point on type 7" rule of the classic loop.  Rounding differs from the
// classic recurrences (alpha comes from a three-term formula), so iteration counts may differ by
// a few: the default stays the classic loop, which is the oracle's.
struct sr_args {
    int64_t n3, k;
    double *sc;
    int64_t *st;
    double epsf;
    int64_t maxits, its_before_restart;
    int merit_stop;
    int refresh;          // 1: r' comes from b^ - A x' (k_refresh), only p, s, x' are formed here
    const double *xcur;
    double *xnext;
    double *r, *p, *s;
    const double *w, *bh;
    double *partial;      // [blocks] merit partials
    fold_args fold;       // -> sc[S_SR_MERIT]
    red_src rs;           // where gamma, delta, merit of the last reduction are found
};

__global__ void __launch_bounds__(VEC_T) k_vec_sr(sr_args a) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    const int64_t k = a.k;
    if (a.st[T_ITER_A] < k) return;   // stopped by an earlier iteration's decisions
    double t3[3];
    red_get<3>(a.sc + S_SR_GAMMA, a.rs, t3, sh);
    const double gamma = t3[0], delta = t3[1], merit = t3[2];
    const double bnorm = a.sc[S_BNORM];
    int type = 0;
    int64_t its = k - 1, xsel = (k - 1) & 1;
    if (!isfinite(gamma)) type = -4;
    else if (k > 1) {   // decisions of iteration k-1 (x_{k-1} lives in buffer (k-1)&1)
        if (sqrt(gamma) <= a.epsf * bnorm) type = 1;
        else if (k - 1 >= a.maxits && a.maxits > 0) type = 5;
        else if (a.merit_stop && merit >= a.sc[S_PMF0 + ((k - 1) & 1)]) { type = 7; xsel = (k - 2) & 1; }
    }
    double alpha = 0, beta = 0;
    if (!type) {
        const bool restart = k == 1 || ((k - 1) % a.its_before_restart) == 0;
        double pap = delta;
        if (!restart) {
            beta = gamma / a.sc[S_SR_GP0 + ((k - 1) & 1)];
            pap = delta - beta * gamma / a.sc[S_SR_AP0 + ((k - 1) & 1)];
        }
        if (!isfinite(pap) || !isfinite(beta)) type = -4;
        else if (pap <= 0) type = -5;
        else { alpha = gamma / pap; if (!isfinite(alpha)) type = -4; }
        if (type) { its = k; xsel = (k - 1) & 1; }   // as k_step: the previous point, this iteration's number
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.sc[S_R2OUT] = gamma;
        if (type) {
            a.st[T_TYPE] = type;
            a.st[T_ITERS] = its;
            a.st[T_XSEL] = xsel;
            a.st[T_ITER_A] = k - 1;   // this iteration's product and everything later return at once
        } else {
            a.sc[S_SR_GP0 + (k & 1)] = gamma;
            a.sc[S_SR_AP0 + (k & 1)] = alpha;
            a.sc[S_PMF0 + (k & 1)] = merit;
        }
    }
    if (type) return;
    double s_mf = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < a.n3; i += stride) {
        const double ri = a.r[i];
        const double pi = ri + beta * a.p[i];
        const double si = __builtin_nontemporal_load(a.w + i) + beta * a.s[i];
        const double cx = __builtin_nontemporal_load(a.xcur + i) + alpha * pi;
        __builtin_nontemporal_store(pi, a.p + i);
        __builtin_nontemporal_store(si, a.s + i);
        __builtin_nontemporal_store(cx, a.xnext + i);
        if (!a.refresh) {
            const double cr = ri - alpha * si;
            __builtin_nontemporal_store(cr, a.r + i);   // gathered by the product that follows (see STAN_P_NT)
            if (a.merit_stop) s_mf -= (cr + a.bh[i]) * cx;
        }
    }
    if (!a.refresh) {
        const double t = block_sum(s_mf, sh);
        if (threadIdx.x == 0) st_agent(a.partial + blockIdx.x, t);
        if (a.fold.counter && fold_arrive(a.fold, &sh_last)) fold_finish<1>(a.fold, a.partial, sh);
    }
}

// U[d - red[d]] = s_d * x^_d on free DOFs (SolverFunctions.cs:305 lincgresults + un-scaling)
__global__ void k_result(int64_t n3, int64_t dof0, const int32_t *red, const double *s,
                         const double *x, double *U) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[dof0 + i];
        if (rd != -1) U[dof0 + i - rd] = s[i] * x[i];
    }
}
// multi-rank: scaled solution into the global block vector, compressed after the all-gather
__global__ void k_result_full(int64_t n3, const double *s, const double *x, double *full) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride)
        full[i] = s[i] * x[i];
}
__global__ void k_compress(int64_t n_dof, const int32_t *red, const double *full, double *U) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dof; i += stride) {
        const int32_t rd = red[i];
        if (rd != -1) U[i - rd] = full[i];
    }
}
// reduced host-order vector <-> full local vector (for stan_hip_spmv)
__global__ void k_expand(int64_t n3, int64_t dof0, const int32_t *red, const double *in,
                         const double *div, double *out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[dof0 + i];
        double v = rd == -1 ? 0.0 : in[dof0 + i - rd];
        if (div) v /= div[i];
        out[i] = v;
    }
}
__global__ void k_compress_div(int64_t n3, const int32_t *red, const double *s, const double *y,
                               double *out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[i];
        if (rd != -1) out[i - rd] = s ? y[i] / s[i] : y[i];
    }
}
__global__ void k_fill(double *p, int64_t n, double v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
