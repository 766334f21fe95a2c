// cg_setup_kernels.inc -- scaling (k_diag_scale, k_diag_get, k_scale_matrix), k_init / k_init_b / k_reduce / k_init_scalars
// Part of cg.hip (included there, inside its anonymous namespace; not a translation unit of its own): split out in
// round 4 so that each piece can be read on its own.  The reference has no counterpart of these kernels beyond the
// calls they replace: alglib.lincgsolvesparse / sparsesmv behind SolverFunctions.LinearSolver_CG (SolverFunctions.cs:270-330).

// ---- setup kernels ---------------------------------------------------------------------------
// s_i = 1/sqrt(K_ii) if K_ii > 0 else 1 (lincgsolvesparse); one lane per block row
__global__ void k_diag_scale(int64_t nloc, const int32_t *rowlen, const int32_t *posof, const int32_t *slot_ptr,
                             const int32_t *cols, const double *vals, double *s) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nloc) return;
    const int64_t pos = posof[row];   // SELL-C-sigma: where the row sits in the sliced layout
    const int64_t slice = pos >> 6;
    const int lane = (int)(pos & 63);
    const int32_t k0 = slot_ptr[slice];
    double d0 = 0, d1 = 0, d2 = 0;
    for (int k = 0; k < rowlen[row]; k++)
        if (cols[((int64_t)k0 + k) * 64 + lane] == (int32_t)row) {
            const double *v = vals + ((int64_t)k0 + k) * 9 * 64 + lane;
            d0 = v[0 * 64]; d1 = v[4 * 64]; d2 = v[8 * 64];
            break;
        }
    s[3 * row + 0] = d0 > 0 ? 1.0 / sqrt(d0) : 1.0;
    s[3 * row + 1] = d1 > 0 ? 1.0 / sqrt(d1) : 1.0;
    s[3 * row + 2] = d2 > 0 ? 1.0 / sqrt(d2) : 1.0;
}

// d[3 row + m] = K_(3 row + m, 3 row + m) of the UNSCALED matrix (s != nullptr: the values carry S K S, undo it)
__global__ void k_diag_get(int64_t nloc, const int32_t *rowlen, const int32_t *posof, const int32_t *slot_ptr,
                           const int32_t *cols, const double *vals, const double *s, double *d) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nloc) return;
    const int64_t pos = posof[row];
    const int64_t slice = pos >> 6;
    const int lane = (int)(pos & 63);
    const int32_t k0 = slot_ptr[slice];
    double d0 = 0, d1 = 0, d2 = 0;
    for (int k = 0; k < rowlen[row]; k++)
        if (cols[((int64_t)k0 + k) * 64 + lane] == (int32_t)row) {
            const double *v = vals + ((int64_t)k0 + k) * 9 * 64 + lane;
            d0 = v[0 * 64]; d1 = v[4 * 64]; d2 = v[8 * 64];
            break;
        }
    if (s) { d0 /= s[3 * row] * s[3 * row]; d1 /= s[3 * row + 1] * s[3 * row + 1]; d2 /= s[3 * row + 2] * s[3 * row + 2]; }
    d[3 * row] = d0; d[3 * row + 1] = d1; d[3 * row + 2] = d2;
}

// vals[slot][3m+n][lane] *= s[3 row + m] * s[3 col + n]: the scaling pass of its own (several ranks, reduced-precision streams,
// small systems, folded copies, an export before the first solve; the single-GPU fp64 loop scales in its first product:
// k_spmv_first, same expression)
__global__ void __launch_bounds__(256)
k_scale_matrix(int32_t nslices, const int32_t *slot_ptr, const int32_t *rowof, const int32_t *cols, double *vals,
               const double *s) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int64_t row = rowof[slice * 64 + lane];
    const double sr[3] = {s[3 * row], s[3 * row + 1], s[3 * row + 2]};  // s is padded to slices
    for (int32_t k = slot_ptr[slice]; k < slot_ptr[slice + 1]; k++) {
        const int32_t c = cols[(int64_t)k * 64 + lane];
        const double sc[3] = {s[3 * (int64_t)c], s[3 * (int64_t)c + 1], s[3 * (int64_t)c + 2]};
        double *v = vals + (int64_t)k * 9 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) v[(3 * m + n) * 64] *= sr[m] * sc[n];
    }
}

// b^[i] = s_i * F[d - red[d]] on free DOFs, 0 on fixed ones; also x0 = 0, r = p = b^ and
// partial sums of b^.b^ (x0 = 0 => r0 = b^, merit0 = 0).
__global__ void __launch_bounds__(VEC_T)
k_init(int64_t n3, int64_t dof0, const int32_t *red, const double *F, const double *s,
       double *bh, double *x0, double *r, double *p, double *partial, fold_args fold) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    double acc = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        const int32_t rd = red[dof0 + i];
        const double b = rd == -1 ? 0.0 : s[i] * F[dof0 + i - rd];
        bh[i] = b;
        x0[i] = 0.0;
        r[i] = b;
        p[i] = b;
        acc += b * b;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) st_agent(partial + blockIdx.x, t);
    if (fold.counter && fold_arrive(fold, &sh_last)) fold_finish<1>(fold, partial, sh);
}

// A refinement pass (STAN_OPT_CG_REFINE, reduced-precision value streams): the right-hand side is the fp64 residual
// that cg_run::fp64_check left in `src` (which may be r itself); x0 = 0, r = p = b^ = src and the partial sums of b^.b^.
__global__ void __launch_bounds__(VEC_T)
k_init_b(int64_t n3, const double *src, double *bh, double *x0, double *r, double *p, double *partial, fold_args fold) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    double acc = 0;
    const int64_t stride = (int64_t)gridDim.x * VEC_T;
    for (int64_t i = (int64_t)blockIdx.x * VEC_T + threadIdx.x; i < n3; i += stride) {
        const double b = src[i];
        bh[i] = b;
        x0[i] = 0.0;
        r[i] = b;
        p[i] = b;
        acc += b * b;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) st_agent(partial + blockIdx.x, t);
    if (fold.counter && fold_arrive(fold, &sh_last)) fold_finish<1>(fold, partial, sh);
}
// the passes' iterates add up in fp64: xacc += d; the sum also goes to `gather` (a vector the peers know: the
// check product gathers it)
__global__ void k_accumulate(int64_t n3, double *xacc, const double *d, double *gather) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += stride) {
        const double s = xacc[i] + d[i];
        xacc[i] = s;
        gather[i] = s;
    }
}
// peer to peer: the two sums of the fp64 check lie in this rank's mailbox; land them in the local scalars (rank
// order: every rank gets the same bits), where the host reads them
__global__ void __launch_bounds__(64) k_land_sums(double *scalars, red_src rs) {
    __shared__ double sh[4];
    double t[2];
    red_get<2>(scalars, rs, t, sh);
    if (threadIdx.x == 0) { scalars[0] = t[0]; scalars[1] = t[1]; }
}

// out[j] = sum_i partial[i*nv + j]: the unfolded form of the reduction (one 256-thread block, the
// same summation order as fold_finish: both paths give the same bits)
// st != nullptr (the loop's launches, peer to peer): once the solve has stopped -- every rank takes the same decision, but
// not at the same moment -- this launch only COUNTS, like fold_skip: a rank that free-runs through the iterations enqueued
// behind the stop (STAN_P2P_WAIT_MODE=2: stopped consumers do not poll) must not store stale partials into a mailbox slot
// that a slower peer has not read yet (slot R + RING aliases slot R).
template <int NV>
__global__ void __launch_bounds__(256)
k_reduce(const double *partial, int np, double *out, p2p_out po, const int64_t *st, int64_t k) {
    __shared__ double sh[4];
    if (st && po.pp && stopped(st, k)) {
        if (po.signal && (int)threadIdx.x < po.pp->n)
            __hip_atomic_fetch_add(po.pp->sig_red[threadIdx.x][po.slot], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    double r[NV];
    sum_partials<NV>(partial, np, sh, r);   // np == 0 (a rank that owns no rows): zeros
    publish_sums<NV>(out, po, r, sh);
}

// after the b^.b^ reduction: bnorm, first residual test, rho, prevmf
__global__ void __launch_bounds__(64) k_init_scalars(double *sc, int64_t *st, double epsf, red_src rs) {
    __shared__ double sh[4];
    double t[1];
    red_get<1>(sc + S_VMV, rs, t, sh);   // b^.b^ (all ranks' partials when sharded peer to peer)
    if (threadIdx.x != 0) return;
    const double r2 = t[0];
    sc[S_BNORM] = sqrt(r2);
    sc[S_RHO0] = r2; sc[S_RHO1] = r2;  // iteration 1 reads slot 1
    sc[S_PMF0] = 0.0; sc[S_PMF1] = 0.0;
    sc[S_R2OUT] = r2;
    st[T_ITER_A] = 0x7fffffffffffffffLL;
    st[T_ITER_B] = 0x7fffffffffffffffLL;
    st[T_TYPE] = 0; st[T_ITERS] = 0; st[T_XSEL] = 0;
    if (!isfinite(r2)) { st[T_TYPE] = -4; st[T_ITER_A] = 0; }
    else if (sqrt(r2) <= epsf * sqrt(r2)) { st[T_TYPE] = 1; st[T_ITER_A] = 0; }
}
