// harmonic.hip -- the kernels of the frequency response by modal superposition (api_harmonic.hip).  A
// block vector is [k][N], one column after the other, k <= STAN_MODAL_QMAX = 32, as in modal.hip.
//   project   p_j = phi_j . F (a term one fused multiply-add, rows ascending per lane, block_sums, the workgroups' partial sums in
//             workgroup order by k_finish_sums), then r = u_s - sum_j phi_j c_j, c_j = p_j / lambda_j formed on the host, j
//             ascending, one fused multiply-add per term: two passes over Phi, because p needs the grid-wide sum first;
//   sweep     one lane per row: the row of Phi and r_d in registers, a loop over the frequencies, HM_FB of them per trip (2 HM_FB
//             independent chains of fused multiply-adds; HM_FB = 4, 1 beyond 24 modes); per frequency f
//                 re = r_d, re = fma(phi_jd, a_jf, re) for j ascending;  im = 0, im = fma(phi_jd, b_jf, im) for j ascending;
//                 amp2 = fma(re, re, im im)
//             and the lane keeps the largest amp2 with the lowest f that attains it (a later f replaces it only when strictly
//             larger); peak = sqrt(amp2).  The table (a_jf, b_jf) is [n_freq][QT] pairs, QT the mode count rounded up to a
//             multiple of 4, zeros beyond k (a padded term is fma(0, 0, x) = x); its address is uniform across the wave, so the
//             loads are scalar loads and the coefficient is the scalar operand of the multiply-add: per frequency the VALU issues
//             the 2 QT multiply-adds and six instructions for the amplitude, the compare and the three selects, nothing else;
//   snapshots the same expressions for a list of frequency indices, stored as (re, im) columns: the bits the sweep computed;
//   probes    the same expressions at a list of DOFs for every frequency, one thread per (frequency, probe).
// All bit-reproducible: no atomics on doubles, every sum in a fixed order.
#include <type_traits>

#include "elem_pass.h"   // block_sums, k_finish_sums

namespace {

constexpr int QMAX = STAN_MODAL_QMAX;
constexpr int HM_ROWS = STAN_HM_ROWS;   // rows per workgroup of the projection and of the peak reduction: 4 per lane
// frequencies per trip of the sweep: 4, or 1 beyond 24 modes.  A trip keeps its table rows in scalar registers: 4 rows of 24 pairs are
// loaded piecewise without a spill, but already 2 rows of 28 pairs made the compiler spill 26 scalar registers to VGPR lanes, with
// v_writelane / v_readlane inside the loop; one row at a time spills nothing (the compiler's resource report), and the two chains of
// a lane (re, im) are covered by the 6 to 7 waves per SIMD
template <int QT> constexpr int HM_FB = QT > 24 ? 1 : 4;

struct hm_cols { double c[QMAX]; };   // p_j / lambda_j, zeros beyond k

// ---- project ---------------------------------------------------------------------------------------------------------------
// grid (row blocks, k): partial[j * gridDim.x + b] = the workgroup's sum of phi_j F over its rows
__global__ void __launch_bounds__(256)
k_hm_dots(int64_t N, const double *__restrict__ Phi, const double *__restrict__ F, double *__restrict__ partial) {
    __shared__ double sh[4][1];
    const int j = blockIdx.y;
    double s[1] = {0.0};
    for (int i = 0; i < HM_ROWS / 256; i++) {
        const int64_t row = (int64_t)blockIdx.x * HM_ROWS + i * 256 + threadIdx.x;
        if (row < N) s[0] = fma(Phi[(int64_t)j * N + row], F[row], s[0]);
    }
    block_sums(s, sh);
    if (threadIdx.x == 0) partial[(int64_t)j * gridDim.x + blockIdx.x] = s[0];
}

// r = u_s - sum_j phi_j c_j, j ascending
__global__ void __launch_bounds__(256)
k_hm_residual(int64_t N, int k, const double *__restrict__ Phi, const double *__restrict__ us, const hm_cols cols, double *__restrict__ r) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    double v = us[row];
    for (int j = 0; j < k; j++) v = fma(-Phi[(int64_t)j * N + row], cols.c[j], v);
    r[row] = v;
}

// ---- the response of one row at FB consecutive table rows --------------------------------------------------------------------
// tab: the table rows of the FB frequencies, QT pairs each (uniform across the wave)
template <int QT, int FB>
__device__ __forceinline__ void hm_response(const double (&phi)[QT], double rd, const double2 *__restrict__ tab, double (&re)[FB],
                                            double (&im)[FB]) {
#pragma unroll
    for (int u = 0; u < FB; u++) { re[u] = rd; im[u] = 0.0; }
#pragma unroll
    for (int j = 0; j < QT; j++)
#pragma unroll
        for (int u = 0; u < FB; u++) {
            const double2 ab = tab[u * QT + j];
            re[u] = fma(phi[j], ab.x, re[u]);
            im[u] = fma(phi[j], ab.y, im[u]);
        }
}

template <int QT>
__device__ __forceinline__ void hm_load_row(int64_t N, int k, int64_t row, const double *__restrict__ Phi, const double *__restrict__ r,
                                            double (&phi)[QT], double &rd) {
#pragma unroll
    for (int j = 0; j < QT; j++) phi[j] = j < k ? Phi[(int64_t)j * N + row] : 0.0;
    rd = r ? r[row] : 0.0;
}

// ---- sweep -------------------------------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256)
k_hm_sweep(int64_t N, int k, int n_freq, const double *__restrict__ Phi, const double *__restrict__ r, const double2 *__restrict__ tab,
           double *__restrict__ peak, int32_t *__restrict__ peak_idx) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    double phi[QT], rd;
    hm_load_row<QT>(N, k, row, Phi, r, phi, rd);
    double best = -1.0;
    int32_t at = 0;
    int f = 0;
    constexpr int FB = HM_FB<QT>;
    for (; f + FB <= n_freq; f += FB) {
        double re[FB], im[FB];
        hm_response<QT, FB>(phi, rd, tab + (int64_t)f * QT, re, im);
#pragma unroll
        for (int u = 0; u < FB; u++) {
            const double a2 = fma(re[u], re[u], im[u] * im[u]);
            if (a2 > best) { best = a2; at = f + u; }
        }
    }
    for (; f < n_freq; f++) {
        double re[1], im[1];
        hm_response<QT, 1>(phi, rd, tab + (int64_t)f * QT, re, im);
        const double a2 = fma(re[0], re[0], im[0] * im[0]);
        if (a2 > best) { best = a2; at = f; }
    }
    peak[row] = sqrt(best);
    peak_idx[row] = at;
}

// ---- snapshots: snaps [n_snap][2][N] -------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256)
k_hm_snap(int64_t N, int k, int n_snap, const int32_t *__restrict__ snap_freq, const double *__restrict__ Phi, const double *__restrict__ r,
          const double2 *__restrict__ tab, double *__restrict__ snaps) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    double phi[QT], rd;
    hm_load_row<QT>(N, k, row, Phi, r, phi, rd);
    for (int s = 0; s < n_snap; s++) {
        double re[1], im[1];
        hm_response<QT, 1>(phi, rd, tab + (int64_t)snap_freq[s] * QT, re, im);
        snaps[(int64_t)(2 * s) * N + row] = re[0];
        snaps[(int64_t)(2 * s + 1) * N + row] = im[0];
    }
}

// ---- probes: probe [n_freq][n_probe][2] -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_hm_probe(int64_t N, int k, int QT, int n_freq, int n_probe, const int32_t *__restrict__ probe_dof, const double *__restrict__ Phi,
           const double *__restrict__ r, const double2 *__restrict__ tab, double *__restrict__ probe) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_freq * n_probe) return;
    const int64_t f = t / n_probe;
    const int64_t d = probe_dof[t - f * n_probe];
    double re = r ? r[d] : 0.0, im = 0.0;
    for (int j = 0; j < QT; j++) {
        const double ph = j < k ? Phi[(int64_t)j * N + d] : 0.0;
        const double2 ab = tab[f * QT + j];
        re = fma(ph, ab.x, re);
        im = fma(ph, ab.y, im);
    }
    probe[2 * t] = re;
    probe[2 * t + 1] = im;
}

// ---- the largest peak, the lowest row on a tie ---------------------------------------------------------------------------------
__device__ __forceinline__ void peak_merge(double &v, long long &i, double v2, long long i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
constexpr long long NO_ROW = 0x7fffffffffffffffLL;
__device__ __forceinline__ void peak_block(double &bv, long long &bi) {   // on thread 0: the workgroup's
    __shared__ double shv[4];
    __shared__ long long shi[4];
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(bv, off, 64);
        const long long i2 = __shfl_xor(bi, off, 64);
        peak_merge(bv, bi, v2, i2);
    }
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = bv; shi[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) peak_merge(bv, bi, shv[w], shi[w]);
}
__global__ void __launch_bounds__(256)
k_hm_peakmax(int64_t N, const double *__restrict__ peak, double *__restrict__ pval, long long *__restrict__ pidx) {
    double bv = -1.0;
    long long bi = NO_ROW;
    for (int i = 0; i < HM_ROWS / 256; i++) {
        const int64_t row = (int64_t)blockIdx.x * HM_ROWS + i * 256 + threadIdx.x;
        if (row < N) peak_merge(bv, bi, peak[row], row);
    }
    peak_block(bv, bi);
    if (threadIdx.x == 0) { pval[blockIdx.x] = bv; pidx[blockIdx.x] = bi; }
}
// one workgroup: out[0] = the value, out_idx[0] = the row, out_idx[1] = peak_idx of that row
__global__ void __launch_bounds__(256)
k_hm_peakmax_finish(int64_t n_blocks, const double *__restrict__ pval, const long long *__restrict__ pidx,
                    const int32_t *__restrict__ peak_idx, double *__restrict__ out, long long *__restrict__ out_idx) {
    double bv = -1.0;
    long long bi = NO_ROW;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) peak_merge(bv, bi, pval[b], pidx[b]);
    peak_block(bv, bi);
    if (threadIdx.x == 0) { out[0] = bv; out_idx[0] = bi; out_idx[1] = bi == NO_ROW ? 0 : peak_idx[bi]; }
}

// f(std::integral_constant<int, QT>): the one dispatch over the widths the row kernels are instantiated for
template <typename F>
void with_hm_qt(int QT, F &&f) {
    switch (QT) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 12: f(std::integral_constant<int, 12>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 20: f(std::integral_constant<int, 20>{}); break;
    case 24: f(std::integral_constant<int, 24>{}); break;
    case 28: f(std::integral_constant<int, 28>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
    }
}

}  // namespace

int stan_harmonic_dots_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_phi, const double *d_F, double *d_partial, double *d_p) {
    hipStream_t st = ctx->stream;
    const int64_t nb = stan_harmonic_blocks(N);
    hipLaunchKernelGGL(k_hm_dots, dim3((unsigned)nb, (unsigned)k), dim3(256), 0, st, N, d_phi, d_F, d_partial);
    hipLaunchKernelGGL(k_finish_sums<256>, dim3((unsigned)k), dim3(256), 0, st, nb, d_partial, d_p);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_harmonic_residual_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_phi, const double *d_us, const double *c, double *d_r) {
    hm_cols cols;
    for (int j = 0; j < QMAX; j++) cols.c[j] = j < k ? c[j] : 0.0;
    hipLaunchKernelGGL(k_hm_residual, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, (int)k, d_phi, d_us, cols, d_r);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_harmonic_sweep_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_freq, const double *d_phi, const double *d_r,
                               const double *d_tab, double *d_peak, int32_t *d_peak_idx) {
    with_hm_qt(stan_harmonic_width(k), [&](auto qt) {
        hipLaunchKernelGGL(k_hm_sweep<decltype(qt)::value>, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, (int)k, (int)n_freq, d_phi, d_r,
                           (const double2 *)d_tab, d_peak, d_peak_idx);
    });
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_harmonic_snap_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_snap, const int32_t *d_snap_freq, const double *d_phi,
                              const double *d_r, const double *d_tab, double *d_snaps) {
    with_hm_qt(stan_harmonic_width(k), [&](auto qt) {
        hipLaunchKernelGGL(k_hm_snap<decltype(qt)::value>, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, (int)k, (int)n_snap, d_snap_freq,
                           d_phi, d_r, (const double2 *)d_tab, d_snaps);
    });
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_harmonic_probe_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_freq, int32_t n_probe, const int32_t *d_probe_dof,
                               const double *d_phi, const double *d_r, const double *d_tab, double *d_probe) {
    const int64_t n = (int64_t)n_freq * n_probe;
    hipLaunchKernelGGL(k_hm_probe, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, N, (int)k, stan_harmonic_width(k), (int)n_freq, (int)n_probe,
                       d_probe_dof, d_phi, d_r, (const double2 *)d_tab, d_probe);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_harmonic_peakmax_device(stan_ctx *ctx, int64_t N, const double *d_peak, const int32_t *d_peak_idx, double *d_pval, long long *d_pidx,
                                 double *d_out, long long *d_out_idx) {
    hipStream_t st = ctx->stream;
    const int64_t nb = stan_harmonic_blocks(N);
    hipLaunchKernelGGL(k_hm_peakmax, dim3((unsigned)nb), dim3(256), 0, st, N, d_peak, d_pval, d_pidx);
    hipLaunchKernelGGL(k_hm_peakmax_finish, dim3(1), dim3(256), 0, st, nb, d_pval, d_pidx, d_peak_idx, d_out, d_out_idx);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
