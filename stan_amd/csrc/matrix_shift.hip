// matrix_shift.hip -- K + sigma diag(M) as a matrix of its own (stan_hip_matrix_shifted): the operator of
// an implicit time step and of a shifted modal analysis.  The result has K's layout (copies of its structure arrays) and its own
// value array, unscaled, with nothing derived: the CG, the products, the placement search, the value streams, row folding and
// the modal driver run on it as on an assembled K.  One device, one rank (the callers refuse the rest).  K is read only.
#include <algorithm>
#include <cmath>

#include "internal.h"

namespace {

// the first entry of M [N] that is not positive and finite
__global__ void __launch_bounds__(256)
k_mass_check(int64_t N, const double *__restrict__ M, long long *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double m = M[i];
    if (!(m > 0.0) || m > 1.7976931348623157e308) atomicMin(bad, (long long)i);
}

// out = the exported values of K with sigma M on the free diagonal: a wavefront per slice, a lane per row, one pass over the
// slice's slots (k_scale_matrix's walk); s non-null: `vals` carries S K S.  The diagonal block of a row is the first of its
// own rowlen blocks whose column is the row (k_diag_get's search); fixed DOFs (fixmask), padding rows and padding slots are
// copied.  M is read one element wide (a caller's pointer); no atomics, nothing of K is written.
__global__ void __launch_bounds__(256)
k_shift_matrix(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
               const int32_t *__restrict__ rowlen, const int32_t *__restrict__ cols, const double *__restrict__ vals,
               const double *__restrict__ s, const int32_t *__restrict__ red, const uint8_t *__restrict__ fixmask, double sigma,
               const double *__restrict__ M, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int64_t row = rowof[slice * 64 + lane];
    const bool live = row < nloc;
    const int32_t len = live ? rowlen[row] : 0;
    const int rfix = live ? fixmask[row] : 7;
    double sr[3] = {1.0, 1.0, 1.0}, sm[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (s) sr[m] = s[3 * row + m];
            const int64_t d = 3 * row + m;
            if (!((rfix >> m) & 1)) sm[m] = M[d - red[d]];
        }
    }
    const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
    bool diag_open = true;   // the row's diagonal block has not been met yet
    for (int32_t k = k0; k < k1; k++) {
        const int32_t c = cols[(int64_t)k * 64 + lane];
        const bool own = k - k0 < len;
        const bool diag = own && diag_open && c == (int32_t)row;
        if (diag) diag_open = false;
        const int cfix = own ? fixmask[c] : 7;
        double sc[3] = {1.0, 1.0, 1.0};
        if (s && own) { sc[0] = s[3 * (int64_t)c]; sc[1] = s[3 * (int64_t)c + 1]; sc[2] = s[3 * (int64_t)c + 2]; }
        const double *v = vals + (int64_t)k * 9 * 64 + lane;
        double *o = out + (int64_t)k * 9 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) {
                double a = v[(3 * m + n) * 64];
                const bool free_entry = own && !((rfix >> m) & 1) && !((cfix >> n) & 1);
                if (free_entry) {
                    if (s) a = stan_unscaled_value(a, sr[m], sc[n]);
                    if (diag && m == n) a = fma(sigma, sm[m], a);
                }
                o[(3 * m + n) * 64] = a;
            }
    }
}

// out = A + sigma B on the layout both have: k_shift_matrix's walk, a wavefront per slice, a lane per row, one pass over the
// slice's slots; sa / sb non-null: that matrix' values carry S K S with its own S.  A free entry is fma(sigma, b, a) on the two
// exported values (stan_unscaled_value); fixed DOFs (fixmask), padding rows and padding slots are copied from A.  Every value of
// va and vb is read once, every value of out written once; no atomics.
__global__ void __launch_bounds__(256)
k_matrix_axpy(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
              const int32_t *__restrict__ rowlen, const int32_t *__restrict__ cols, const uint8_t *__restrict__ fixmask,
              const double *__restrict__ va, const double *__restrict__ sa, double sigma, const double *__restrict__ vb,
              const double *__restrict__ sb, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int64_t row = rowof[slice * 64 + lane];
    const bool live = row < nloc;
    const int32_t len = live ? rowlen[row] : 0;
    const int rfix = live ? fixmask[row] : 7;
    double ar[3] = {1.0, 1.0, 1.0}, br[3] = {1.0, 1.0, 1.0};
    if (live) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (sa) ar[m] = sa[3 * row + m];
            if (sb) br[m] = sb[3 * row + m];
        }
    }
    const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
    for (int32_t k = k0; k < k1; k++) {
        const int32_t c = cols[(int64_t)k * 64 + lane];
        const bool own = k - k0 < len;
        const int cfix = own ? fixmask[c] : 7;
        double ac[3] = {1.0, 1.0, 1.0}, bc[3] = {1.0, 1.0, 1.0};
        if (own) {
#pragma unroll
            for (int n = 0; n < 3; n++) {
                if (sa) ac[n] = sa[3 * (int64_t)c + n];
                if (sb) bc[n] = sb[3 * (int64_t)c + n];
            }
        }
        const double *pa = va + (int64_t)k * 9 * 64 + lane, *pb = vb + (int64_t)k * 9 * 64 + lane;
        double *o = out + (int64_t)k * 9 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) {
                double a = pa[(3 * m + n) * 64];
                double b = pb[(3 * m + n) * 64];
                const bool free_entry = own && !((rfix >> m) & 1) && !((cfix >> n) & 1);
                if (free_entry) {
                    if (sa) a = stan_unscaled_value(a, ar[m], ac[n]);
                    if (sb) b = stan_unscaled_value(b, br[m], bc[n]);
                    a = fma(sigma, b, a);
                }
                o[(3 * m + n) * 64] = a;
            }
    }
}

// "the same layout" of two matrices whose scalars agree: entry i of each structure array of A against B's; a difference raises
// bit 0 of status[SS_ERRBITS].  n = the longest of the five arrays.
__global__ void __launch_bounds__(256)
k_layout_compare(int64_t n, int64_t n_ptr, int64_t n_pad, int64_t n_cols, int64_t n_rows, int64_t n_dof,
                 const int32_t *__restrict__ ptr_a, const int32_t *__restrict__ ptr_b, const int32_t *__restrict__ len_a,
                 const int32_t *__restrict__ len_b, const int32_t *__restrict__ of_a, const int32_t *__restrict__ of_b,
                 const int32_t *__restrict__ cols_a, const int32_t *__restrict__ cols_b, const uint8_t *__restrict__ fix_a,
                 const uint8_t *__restrict__ fix_b, const int32_t *__restrict__ red_a, const int32_t *__restrict__ red_b, int64_t *status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool diff = false;
    if (i < n_ptr) diff = diff || ptr_a[i] != ptr_b[i];
    if (i < n_pad) diff = diff || len_a[i] != len_b[i] || of_a[i] != of_b[i];
    if (i < n_cols) diff = diff || cols_a[i] != cols_b[i];
    if (i < n_rows) diff = diff || fix_a[i] != fix_b[i];
    if (i < n_dof) diff = diff || red_a[i] != red_b[i];
    if (diff) atomicOr((unsigned long long *)&status[SS_ERRBITS], 1ull);
}

template <typename T>
int clone_array(stan_ctx *ctx, T **dst, const T *src, size_t n) {
    STANCHK(stan_dmalloc(ctx, dst, n ? n : 1));
    if (n && src) HIPCHK(ctx, hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    return STAN_OK;
}

}  // namespace

int stan_matrix_clone_layout(stan_ctx *ctx, const stan_matrix *K, stan_matrix **out) {
    stan_matrix *S = new stan_matrix();
    S->ctx = ctx;
    ctx->matrices.push_back(S);
    stan_matrix_guard g{S};
    S->n_dof = K->n_dof; S->n_red = K->n_red; S->nb_glob = K->nb_glob;
    S->r0 = K->r0; S->r1 = K->r1; S->u0 = K->u0; S->u1 = K->u1;
    S->nloc = K->nloc; S->nhalo = K->nhalo; S->nslices = K->nslices; S->nslots = K->nslots; S->nblocks = K->nblocks;
    S->max_row_blocks = K->max_row_blocks; S->n_elem_scanned = K->n_elem_scanned; S->sigma = K->sigma;
    S->row_starts = K->row_starts;
    const size_t npad = (size_t)K->nslices * 64;
    STANCHK(clone_array(ctx, &S->d_slot_ptr, K->d_slot_ptr, (size_t)K->nslices + 1));
    STANCHK(clone_array(ctx, &S->d_rowlen, K->d_rowlen, npad));
    STANCHK(clone_array(ctx, &S->d_rowof, K->d_rowof, npad));
    STANCHK(clone_array(ctx, &S->d_posof, K->d_posof, npad));
    STANCHK(clone_array(ctx, &S->d_cols, K->d_cols, (size_t)K->nslots * 64));
    STANCHK(clone_array(ctx, &S->d_red, K->d_red, (size_t)K->n_dof));
    STANCHK(clone_array(ctx, &S->d_fixmask, K->d_fixmask, (size_t)K->nb_glob));
    // (behind the columns: the allocation by trial times the product itself -- as in the assembly; the packed column stream
    // is a function of the columns alone and is built by the first product that wants it, as K's was)
    STANCHK(stan_matrix_alloc_stream(ctx, S, STAN_PREC_FP64, S->nslots, &S->vs[STAN_PREC_FP64].padded));
    g.ok = true;
    *out = S;
    return STAN_OK;
}

int stan_mass_check_device(stan_ctx *ctx, int64_t N, const double *d_M, int64_t *bad) {
    *bad = -1;
    if (N <= 0) return STAN_OK;
    return stan_first_offender(ctx, bad, [&](long long *slot) {
        hipLaunchKernelGGL(k_mass_check, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, d_M, slot);
    });
}

int stan_matrix_shifted_device(stan_ctx *ctx, stan_matrix *K, double sigma, const double *d_M, stan_matrix **out, double *shift_ms) {
    hipStream_t st = ctx->stream;
    stan_matrix *S = nullptr;
    STANCHK(stan_matrix_clone_layout(ctx, K, &S));
    stan_matrix_guard g{S};   // a failed call gives back what it had allocated
    event_bag evs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->profiling && shift_ms) { e0 = evs.make(); e1 = evs.make(); }
    if (e0) (void)hipEventRecord(e0, st);
    if (K->nslices > 0)
        hipLaunchKernelGGL(k_shift_matrix, dim3(nblk(K->nslices, 4)), dim3(256), 0, st, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                           K->d_rowlen, K->d_cols, K->vals64(), K->scaled ? K->d_scale : (const double *)nullptr, K->d_red,
                           K->d_fixmask, sigma, d_M, S->vals64());
    HIPCHK(ctx, hipGetLastError());
    if (e1) (void)hipEventRecord(e1, st);
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (e1) {
        float t = 0;
        if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) *shift_ms += t;
    }
    g.ok = true;
    *out = S;
    return STAN_OK;
}

int stan_matrix_axpy_device(stan_ctx *ctx, stan_matrix *A, double sigma, stan_matrix *B, stan_matrix **out, double *axpy_ms) {
    auto bad = [&](const char *why, int rc) { ctx->err = std::string("matrix_axpy: ") + why; return rc; };
    hipStream_t st = ctx->stream;
    for (const stan_matrix *X : {A, B})
        if (X->nhalo != 0 || X->r0 != 0 || X->nloc != X->nb_glob) return bad("a matrix is a shard of a larger one", STAN_E_UNSUPPORTED);
    // ---- the same layout: the scalars here, the structure arrays on the device, before anything is allocated
    if (A->n_dof != B->n_dof || A->n_red != B->n_red || A->nb_glob != B->nb_glob || A->nloc != B->nloc || A->nslices != B->nslices ||
        A->nslots != B->nslots || A->nblocks != B->nblocks || A->sigma != B->sigma || A->max_row_blocks != B->max_row_blocks)
        return bad("A and B do not have one layout (their sizes differ)", STAN_E_ARG);
    if (A != B && A->nslices > 0) {
        const int64_t n_ptr = (int64_t)A->nslices + 1, n_pad = (int64_t)A->nslices * 64, n_cols = (int64_t)A->nslots * 64,
                      n_rows = A->nb_glob, n_dof = A->n_dof;
        const int64_t n = std::max(std::max(std::max(n_ptr, n_pad), std::max(n_cols, n_rows)), n_dof);
        HIPCHK(ctx, hipMemsetAsync(ctx->d_status + SS_ERRBITS, 0, 8, st));
        hipLaunchKernelGGL(k_layout_compare, dim3(nblk(n, 256)), dim3(256), 0, st, n, n_ptr, n_pad, n_cols, n_rows, n_dof, A->d_slot_ptr,
                           B->d_slot_ptr, A->d_rowlen, B->d_rowlen, A->d_rowof, B->d_rowof, A->d_cols, B->d_cols, A->d_fixmask, B->d_fixmask,
                           A->d_red, B->d_red, ctx->d_status);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_ERRBITS, ctx->d_status + SS_ERRBITS, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->h_status[SS_ERRBITS])
            return bad("A and B do not have one layout (their patterns, fixed DOFs or reduction maps differ)", STAN_E_ARG);
    }
    stan_matrix *S = nullptr;
    STANCHK(stan_matrix_clone_layout(ctx, A, &S));
    stan_matrix_guard g{S};   // a failed call gives back what it had allocated
    event_bag evs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->profiling && axpy_ms) { e0 = evs.make(); e1 = evs.make(); }
    if (e0) (void)hipEventRecord(e0, st);
    if (A->nslices > 0)
        hipLaunchKernelGGL(k_matrix_axpy, dim3(nblk(A->nslices, 4)), dim3(256), 0, st, A->nslices, A->nloc, A->d_slot_ptr, A->d_rowof,
                           A->d_rowlen, A->d_cols, A->d_fixmask, A->vals64(), A->scaled ? A->d_scale : (const double *)nullptr, sigma,
                           B->vals64(), B->scaled ? B->d_scale : (const double *)nullptr, S->vals64());
    HIPCHK(ctx, hipGetLastError());
    if (e1) (void)hipEventRecord(e1, st);
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (e1) {
        float t = 0;
        if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) *axpy_ms = t;
    }
    g.ok = true;
    *out = S;
    return STAN_OK;
}
