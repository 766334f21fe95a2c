// modal.hip -- the tall-skinny block kernels of the modal driver (api_modal.hip).  A block vector is
// [q][N], one column after the other (the layout stan_cg_multi_device takes), q <= STAN_MODAL_QMAX = 32; M is the diagonal mass.
//   gram      A = Z^T W and B = Z^T (M o Z) from ONE pass: a workgroup owns GR_ROWS rows, stages them strip by strip (64 rows)
//             through LDS as [row][column] and keeps 2x2 tiles of A and B in registers (VALU fused multiply-adds: the f64 matrix
//             instruction has the vector rate on this chip and would want B's operand M o Z formed first, which costs B its
//             bitwise symmetry);
//   rotate    X = Z Q, KX = W Q, R = KX - (M o X) Lambda, sum R^2 / M per column and the next right-hand sides, one lane per
//             row: the row of Z and of W in registers, Q and Lambda uniform operands;
//   axpy      Z_j = X_j / lambda_j + D_j;
//   normalise column sums of M x^2 and the entry of largest magnitude (lowest index on a tie), then the scaling.
// Behind them the buckling driver's kernels (api_buckling.hip, section 3.12) where its algorithm differs.  What the two sets
// share is written once: block_amax, k_finish_sums (elem_pass.h), k_md_scale and the host halves of the entries.
// All bit-reproducible: no atomics on doubles; a workgroup's sum has a fixed order (rows ascending per wave, the four waves in
// order / block_sums), the workgroups' partial sums are added in workgroup order by one workgroup per value (k_finish_sums).
#include <type_traits>

#include "elem_pass.h"   // block_sums, k_finish_sums

namespace {

constexpr int QMAX = STAN_MODAL_QMAX;
constexpr int GR_STRIP = 64;          // rows per LDS strip
constexpr int GR_ROWS = 4096;         // rows per workgroup of k_md_gram: 64 strips
constexpr int GR_QP = QMAX + 2;       // doubles per LDS row: 16-B aligned pairs, 4 * lane banks apart on the transposing store
constexpr int RT_ROWS = 1024;         // rows per workgroup of k_md_colstats: 4 per lane

// the start block's column j > 0 at row i: a fixed integer hash (the finaliser of splitmix64) mapped to [-0.5, 0.5)
__device__ __forceinline__ double start_entry(int64_t i, int j) {
    unsigned long long h = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull + (unsigned long long)j * 0xD1B54A32D192ED03ull;
    h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 27; h *= 0x94D049BB133111EBull;
    h ^= h >> 31;
    return (double)(h >> 11) * 0x1.0p-53 - 0.5;
}

// rhs = M o X0, and the first row whose mass is not positive and finite
__global__ void __launch_bounds__(256)
k_md_start(int64_t N, int q, const double *__restrict__ M, double *__restrict__ rhs, long long *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double m = M[i];
    if (!(m > 0.0) || m > 1.7976931348623157e308) atomicMin(bad, (long long)i);
    rhs[i] = m * m;
    for (int j = 1; j < q; j++) rhs[(int64_t)j * N + i] = m * start_entry(i, j);
}

// ---- gram ----------------------------------------------------------------------------------------------------------------
// partial [2 q q][gridDim.x]: value v = i * q + j of A, q * q + i * q + j of B, of workgroup b at partial[v * gridDim.x + b].
// NS: tile slots per lane (a lane owns the 2x2 tiles lane, lane + 64, ... of the (qe / 2)^2 tiles, qe = q rounded up to even);
// NC: columns a lane stages per strip (column c = wave + 4 k of row lane).
template <int NS, int NC>
__global__ void __launch_bounds__(256)
k_md_gram(int64_t N, int q, const double *__restrict__ Z, const double *__restrict__ W, const double *__restrict__ M,
          double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double zs[GR_STRIP * GR_QP];
    __shared__ __attribute__((aligned(16))) double ws[GR_STRIP * GR_QP];
    __shared__ double ms[GR_STRIP];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qe = (q + 1) & ~1, nth = qe >> 1, nt = nth * nth;
    const int64_t row0 = (int64_t)blockIdx.x * GR_ROWS;
    const int64_t row1 = row0 + GR_ROWS < N ? row0 + GR_ROWS : N;
    double a[NS][4], b[NS][4];
    int i0[NS], j0[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int tl = lane + 64 * s;
        i0[s] = tl < nt ? 2 * (tl / nth) : -1;
        j0[s] = tl < nt ? 2 * (tl % nth) : 0;
#pragma unroll
        for (int k = 0; k < 4; k++) a[s][k] = b[s][k] = 0.0;
    }
    // the strip in flight: row `lane` of the strip, columns wv, wv + 4, ... (zeros beyond N and beyond q)
    double pz[NC], pw[NC], pm;
    auto fetch = [&](int64_t s0) {
        const int64_t row = s0 + lane;
        const bool in = row < row1;
        pm = in && wv == 0 ? M[row] : 0.0;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const int c = wv + 4 * k;
            const bool on = in && c < q;
            pz[k] = on ? Z[(int64_t)c * N + row] : 0.0;
            pw[k] = on ? W[(int64_t)c * N + row] : 0.0;
        }
    };
    fetch(row0);
    for (int64_t s0 = row0; s0 < row1; s0 += GR_STRIP) {
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const int c = wv + 4 * k;
            if (c < qe) { zs[lane * GR_QP + c] = pz[k]; ws[lane * GR_QP + c] = pw[k]; }
        }
        if (wv == 0) ms[lane] = pm;
        __syncthreads();
        if (s0 + GR_STRIP < row1) fetch(s0 + GR_STRIP);   // in flight behind the arithmetic
        // wave wv: rows wv, wv + 4, ... of the strip, ascending
        for (int r = wv; r < GR_STRIP; r += 4) {
            const double m = ms[r];
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (i0[s] < 0) continue;
                const double zi0 = zs[r * GR_QP + i0[s]], zi1 = zs[r * GR_QP + i0[s] + 1];
                const double zj0 = zs[r * GR_QP + j0[s]], zj1 = zs[r * GR_QP + j0[s] + 1];
                const double wj0 = ws[r * GR_QP + j0[s]], wj1 = ws[r * GR_QP + j0[s] + 1];
                a[s][0] = fma(zi0, wj0, a[s][0]); a[s][1] = fma(zi0, wj1, a[s][1]);
                a[s][2] = fma(zi1, wj0, a[s][2]); a[s][3] = fma(zi1, wj1, a[s][3]);
                b[s][0] = fma(zi0 * zj0, m, b[s][0]); b[s][1] = fma(zi0 * zj1, m, b[s][1]);
                b[s][2] = fma(zi1 * zj0, m, b[s][2]); b[s][3] = fma(zi1 * zj1, m, b[s][3]);
            }
        }
        __syncthreads();
    }
    // the four waves' sums in wave order, on wave 0 (the strips are done with: zs carries the exchange)
#pragma unroll
    for (int s = 0; s < NS; s++) {
        for (int w = 1; w < 4; w++) {
            if (wv == w)
#pragma unroll
                for (int k = 0; k < 4; k++) { zs[k * 64 + lane] = a[s][k]; zs[(4 + k) * 64 + lane] = b[s][k]; }
            __syncthreads();
            if (wv == 0)
#pragma unroll
                for (int k = 0; k < 4; k++) { a[s][k] += zs[k * 64 + lane]; b[s][k] += zs[(4 + k) * 64 + lane]; }
            __syncthreads();
        }
        if (wv == 0 && i0[s] >= 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = i0[s] + (k >> 1), j = j0[s] + (k & 1);
                if (i < q && j < q) {
                    partial[(int64_t)(i * q + j) * gridDim.x + blockIdx.x] = a[s][k];
                    partial[(int64_t)(q * q + i * q + j) * gridDim.x + blockIdx.x] = b[s][k];
                }
            }
        }
    }
}

// ---- rotate + residual ---------------------------------------------------------------------------------------------------
// Q and lambda padded with zeros to QT (QT x QT row-major, QT): a column beyond q multiplies zeros.  partial [q][gridDim.x].
// Z / W may be X / KX: a lane has read its whole row before it stores any of it, and rows are independent.
struct md_cols {
    double lambda[QMAX];
    int32_t dcol[QMAX];
};
template <int QT>
__global__ void __launch_bounds__(256)
k_md_rotate(int64_t N, int q, const double *Z, const double *W, const double *__restrict__ M, const double *__restrict__ Qp,
            const md_cols cols, uint32_t mask, double *X, double *KX, double *__restrict__ rhs, double *__restrict__ partial) {
    __shared__ double sh[4][QT];
    double acc[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) acc[j] = 0.0;
    // one row per lane and no loop over rows: in a loop the loads of Q are hoisted out of it, all QT^2 of them, and spill
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row < N) {
        double z[QT], w[QT];
#pragma unroll
        for (int l = 0; l < QT; l++) {
            z[l] = l < q ? Z[(int64_t)l * N + row] : 0.0;
            w[l] = l < q ? W[(int64_t)l * N + row] : 0.0;
        }
        const double m = M[row];
#pragma unroll
        for (int j = 0; j < QT; j++) {
            if (j >= q) continue;   // uniform
            double x = 0.0, kx = 0.0;
#pragma unroll
            for (int l = 0; l < QT; l++) {
                x = fma(z[l], Qp[l * QT + j], x);
                kx = fma(w[l], Qp[l * QT + j], kx);
            }
            const double lam = cols.lambda[j];
            const double r = kx - (m * x) * lam;
            X[(int64_t)j * N + row] = x;
            KX[(int64_t)j * N + row] = kx;
            acc[j] = r * r / m;
            if (!((mask >> j) & 1u)) rhs[(int64_t)j * N + row] = -r / lam;
        }
    }
    block_sums(acc, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < QT; j++)
            if (j < q) partial[(int64_t)j * gridDim.x + blockIdx.x] = acc[j];
}

// ---- axpy: grid (rows / 256, q) ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_md_axpy(int64_t N, const double *X, const md_cols cols, const double *__restrict__ D, double *Zo) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (row >= N) return;
    double v = X[(int64_t)j * N + row] / cols.lambda[j];
    if (cols.dcol[j] >= 0) v += D[(int64_t)cols.dcol[j] * N + row];
    Zo[(int64_t)j * N + row] = v;
}

// ---- normalise: grid (row blocks, columns) -------------------------------------------------------------------------------
// per column and workgroup: sum M x^2, and the entry of largest magnitude with the lowest index on a tie (value, index)
__device__ __forceinline__ void amax_merge(double &v, long long &i, double v2, long long i2) {
    const double f = fabs(v), f2 = fabs(v2);
    if (f2 > f || (f2 == f && i2 < i)) { v = v2; i = i2; }
}
constexpr long long NO_INDEX = 0x7fffffffffffffffLL;   // the index of "no entry yet": every row's is lower
// The workgroup's (value, index) on thread 0 from the 256 lanes': a 64-lane butterfly, the waves' results handed over through
// shv / shi, the four merged by thread 0.  `barrier` runs between the stores to shv / shi and thread 0's reads and holds the
// workgroup barrier that orders them: __syncthreads(), or block_sums where the kernel sums too.
template <typename Barrier>
__device__ __forceinline__ void block_amax(double &bv, long long &bi, double *shv, long long *shi, Barrier &&barrier) {
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(bv, off, 64);
        const long long i2 = __shfl_xor(bi, off, 64);
        amax_merge(bv, bi, v2, i2);
    }
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = bv; shi[threadIdx.x >> 6] = bi; }
    barrier();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) amax_merge(bv, bi, shv[w], shi[w]);
}
__global__ void __launch_bounds__(256)
k_md_colstats(int64_t N, const double *__restrict__ X, const double *__restrict__ M, double *__restrict__ psum,
              double *__restrict__ pval, long long *__restrict__ pidx) {
    __shared__ double sh[4][1];
    __shared__ double shv[4];
    __shared__ long long shi[4];
    const int j = blockIdx.y;
    double s[1] = {0.0}, bv = 0.0;
    long long bi = NO_INDEX;
    for (int k = 0; k < RT_ROWS / 256; k++) {
        const int64_t row = (int64_t)blockIdx.x * RT_ROWS + k * 256 + threadIdx.x;
        if (row >= N) continue;
        const double x = X[(int64_t)j * N + row];
        s[0] = fma(M[row] * x, x, s[0]);
        amax_merge(bv, bi, x, row);
    }
    block_amax(bv, bi, shv, shi, [&] { block_sums(s, sh); });   // (its barrier orders shv / shi too)
    if (threadIdx.x == 0) {
        const int64_t o = (int64_t)j * gridDim.x + blockIdx.x;
        psum[o] = s[0]; pval[o] = bv; pidx[o] = bi;
    }
}
// the same for a matrix mass (stan_hip_modes_pencil): Y = Mmat X by true products, the sum is x . y, a term one fused multiply-add
__global__ void __launch_bounds__(256)
k_pc_colstats(int64_t N, const double *__restrict__ X, const double *__restrict__ Y, double *__restrict__ psum,
              double *__restrict__ pval, long long *__restrict__ pidx) {
    __shared__ double sh[4][1];
    __shared__ double shv[4];
    __shared__ long long shi[4];
    const int j = blockIdx.y;
    double s[1] = {0.0}, bv = 0.0;
    long long bi = NO_INDEX;
    for (int k = 0; k < RT_ROWS / 256; k++) {
        const int64_t row = (int64_t)blockIdx.x * RT_ROWS + k * 256 + threadIdx.x;
        if (row >= N) continue;
        const double x = X[(int64_t)j * N + row];
        s[0] = fma(Y[(int64_t)j * N + row], x, s[0]);
        amax_merge(bv, bi, x, row);
    }
    block_amax(bv, bi, shv, shi, [&] { block_sums(s, sh); });   // (its barrier orders shv / shi too)
    if (threadIdx.x == 0) {
        const int64_t o = (int64_t)j * gridDim.x + blockIdx.x;
        psum[o] = s[0]; pval[o] = bv; pidx[o] = bi;
    }
}
// one workgroup per column: the partials in block order; scale[j] = +-sqrt(sum M x^2), negative where the largest entry is
__global__ void __launch_bounds__(256)
k_md_colfinish(int64_t n_blocks, const double *__restrict__ psum, const double *__restrict__ pval, const long long *__restrict__ pidx,
               double *__restrict__ scale) {
    __shared__ double sh[4][1];
    __shared__ double shv[4];
    __shared__ long long shi[4];
    const int64_t o = (int64_t)blockIdx.x * n_blocks;
    double s[1] = {0.0}, bv = 0.0;
    long long bi = NO_INDEX;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) {
        s[0] += psum[o + b];
        amax_merge(bv, bi, pval[o + b], pidx[o + b]);
    }
    block_amax(bv, bi, shv, shi, [&] { block_sums(s, sh); });   // (its barrier orders shv / shi too)
    if (threadIdx.x == 0) {
        const double nrm = sqrt(s[0]);
        scale[blockIdx.x] = bv < 0.0 ? -nrm : nrm;
    }
}
__global__ void __launch_bounds__(256)
k_md_scale(int64_t N, const double *__restrict__ X, const double *__restrict__ scale, double *__restrict__ phi) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (row < N) phi[(int64_t)j * N + row] = X[(int64_t)j * N + row] / scale[j];
}

// ---- the buckling driver's block kernels (api_buckling.hip) ---------------------------------------
// the start block: every column j >= 0 is the hash of (row, j)
__global__ void __launch_bounds__(256)
k_bk_start(int64_t N, int q, double *__restrict__ X0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (int j = 0; j < q; j++) X0[(int64_t)j * N + i] = start_entry(i, j);
}
__global__ void __launch_bounds__(256)
k_bk_negate(int64_t n, double *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = -y[i];
}
// X = Z Q: k_md_rotate's shape with one block of operands (Z may be X: a lane has read its whole row before it stores)
template <int QT>
__global__ void __launch_bounds__(256)
k_bk_rotate_x(int64_t N, int q, const double *Z, const double *__restrict__ Qp, double *X) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    double z[QT];
#pragma unroll
    for (int l = 0; l < QT; l++) z[l] = l < q ? Z[(int64_t)l * N + row] : 0.0;
#pragma unroll
    for (int j = 0; j < QT; j++) {
        if (j >= q) continue;   // uniform
        double x = 0.0;
#pragma unroll
        for (int l = 0; l < QT; l++) x = fma(z[l], Qp[l * QT + j], x);
        X[(int64_t)j * N + row] = x;
    }
}
// KX = W Q, R_j = sum_l (mu_j W_l - Y_l) Q_lj, rhs_j = -R_j where bit j of mask is clear, and per column the workgroup's sums
// of R^2 / D and KX^2 / D: partial [2 q][gridDim.x], value j of R, q + j of KX.  The two blocks of operands fill the register
// file, so a column's two sums leave at once: six butterfly stages per wave into LDS, the four waves added in order behind the
// loop (block_sums' order).  W may be KX.
template <int QT>
__global__ void __launch_bounds__(256)
k_bk_residual(int64_t N, int q, const double *W, const double *__restrict__ Y, const double *__restrict__ D,
              const double *__restrict__ Qp, const md_cols cols, uint32_t mask, double *KX, double *__restrict__ rhs,
              double *__restrict__ partial) {
    __shared__ double sh[4][2 * QT];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = row < N;
    double w[QT], y[QT];
#pragma unroll
    for (int l = 0; l < QT; l++) {
        w[l] = in && l < q ? W[(int64_t)l * N + row] : 0.0;
        y[l] = in && l < q ? Y[(int64_t)l * N + row] : 0.0;
    }
    const double dinv = in ? 1.0 / D[row] : 0.0;
#pragma unroll
    for (int j = 0; j < QT; j++) {
        if (j >= q) continue;   // uniform
        const double mu = cols.lambda[j];
        double kx = 0.0, r = 0.0;
#pragma unroll
        for (int l = 0; l < QT; l++) {
            const double ql = Qp[l * QT + j];
            kx = fma(w[l], ql, kx);
            r = fma(fma(mu, w[l], -y[l]), ql, r);
        }
        if (in) {
            KX[(int64_t)j * N + row] = kx;
            if (!((mask >> j) & 1u)) rhs[(int64_t)j * N + row] = -r;
        }
        double s0 = (r * r) * dinv, s1 = (kx * kx) * dinv;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s0 += __shfl_xor(s0, off, 64);
            s1 += __shfl_xor(s1, off, 64);
        }
        if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][j] = s0; sh[threadIdx.x >> 6][QT + j] = s1; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * QT) {
        const int j = threadIdx.x < QT ? threadIdx.x : threadIdx.x - QT;
        if (j < q) {
            double s = sh[0][threadIdx.x];
            for (int wv = 1; wv < 4; wv++) s += sh[wv][threadIdx.x];
            partial[(int64_t)(threadIdx.x < QT ? j : q + j) * gridDim.x + blockIdx.x] = s;
        }
    }
}
// Z_j = mu_j X_j + D_dcol[j] (dcol[j] < 0: mu_j X_j); grid (rows / 256, q)
__global__ void __launch_bounds__(256)
k_bk_axpy(int64_t N, const double *X, const md_cols cols, const double *__restrict__ D, double *Zo) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (row >= N) return;
    const double x = X[(int64_t)j * N + row], mu = cols.lambda[j];
    Zo[(int64_t)j * N + row] = cols.dcol[j] >= 0 ? fma(mu, x, D[(int64_t)cols.dcol[j] * N + row]) : mu * x;
}
// per column and workgroup the entry of largest magnitude (lowest index on a tie): pval / pidx [k][gridDim.x]
__global__ void __launch_bounds__(256)
k_bk_colmax(int64_t N, const double *__restrict__ X, double *__restrict__ pval, long long *__restrict__ pidx) {
    __shared__ double shv[4];
    __shared__ long long shi[4];
    const int j = blockIdx.y;
    double bv = 0.0;
    long long bi = NO_INDEX;
    for (int k = 0; k < RT_ROWS / 256; k++) {
        const int64_t row = (int64_t)blockIdx.x * RT_ROWS + k * 256 + threadIdx.x;
        if (row < N) amax_merge(bv, bi, X[(int64_t)j * N + row], row);
    }
    block_amax(bv, bi, shv, shi, [] { __syncthreads(); });
    if (threadIdx.x == 0) {
        const int64_t o = (int64_t)j * gridDim.x + blockIdx.x;
        pval[o] = bv; pidx[o] = bi;
    }
}
// one workgroup per column: scale[j] = the column's entry of largest magnitude, signed (k_md_scale divides by it)
__global__ void __launch_bounds__(256)
k_bk_colmax_finish(int64_t n_blocks, const double *__restrict__ pval, const long long *__restrict__ pidx, double *__restrict__ scale) {
    __shared__ double shv[4];
    __shared__ long long shi[4];
    const int64_t o = (int64_t)blockIdx.x * n_blocks;
    double bv = 0.0;
    long long bi = NO_INDEX;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) amax_merge(bv, bi, pval[o + b], pidx[o + b]);
    block_amax(bv, bi, shv, shi, [] { __syncthreads(); });
    if (threadIdx.x == 0) scale[blockIdx.x] = bv;
}

// ---- the host halves of the entries: what the two drivers' entries share ---------------------------------------------------
int block_args_check(stan_ctx *ctx, const char *who, int64_t N, int32_t q) {
    if (N <= 0 || q <= 0 || q > QMAX || N > ((int64_t)1 << 31) - 1) {
        ctx->err = std::string(who) + ": N must be in [1, 2^31) and q in [1, 32]";
        return STAN_E_ARG;
    }
    return STAN_OK;
}

// the columns' scalars and corrections as a kernel argument; beyond q no kernel reads them (zeros and "no correction")
void fill_cols(md_cols &cols, int q, const double *scalar, const int32_t *dcol) {
    for (int l = 0; l < QMAX; l++) { cols.lambda[l] = l < q ? scalar[l] : 0.0; cols.dcol[l] = dcol && l < q ? dcol[l] : -1; }
}

// f(std::integral_constant<int, QT>): the one dispatch over the widths the rotate kernels are instantiated for
template <typename F>
void with_qt(int QT, F &&f) {
    if (QT == 8) f(std::integral_constant<int, 8>{});
    else if (QT == 16) f(std::integral_constant<int, 16>{});
    else if (QT == 24) f(std::integral_constant<int, 24>{});
    else f(std::integral_constant<int, 32>{});
}

// What a rotate call sets up: the width QT of its kernels, Q padded with zeros to QT x QT (the host copy outlives the
// stream's), the columns' scalars, and the temporaries of the sums: n_sums values per workgroup of 256 rows.
struct rotate_call {
    int QT = 0; int64_t nb = 0;   // the kernels' width, workgroups of 256 rows
    std::vector<double> Qp;
    md_cols cols;
    dev_scope tmp;
    double *d_Qp = nullptr, *d_partial = nullptr, *d_out = nullptr;
    explicit rotate_call(stan_ctx *ctx) : tmp(ctx) {}
    int prepare(int64_t N, int q, const double *Q, const double *scalar, size_t n_sums) {
        QT = q <= 8 ? 8 : q <= 16 ? 16 : q <= 24 ? 24 : 32;
        nb = nblk(N, 256);
        Qp.assign((size_t)QT * QT, 0.0);
        fill_cols(cols, q, scalar, nullptr);
        for (int l = 0; l < q; l++)
            for (int j = 0; j < q; j++) Qp[(size_t)l * QT + j] = Q[l * q + j];
        STANCHK(tmp.alloc(&d_Qp, Qp.size()));
        STANCHK(tmp.alloc(&d_partial, n_sums * (size_t)nb));
        STANCHK(tmp.alloc(&d_out, n_sums));
        HIPCHK(tmp.ctx, hipMemcpyAsync(d_Qp, Qp.data(), Qp.size() * 8, hipMemcpyHostToDevice, tmp.ctx->stream));
        return STAN_OK;
    }
};

// the tail of the entries with sums: out [n] (host) = the nb workgroups' partials of each value added in workgroup order.
// Synchronises.
int finish_sums(stan_ctx *ctx, int64_t nb, size_t n, const double *d_partial, double *d_out, double *out) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_finish_sums<256>, dim3((unsigned)n), dim3(256), 0, st, nb, d_partial, d_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return STAN_OK;
}

// Z_j = X_j combined with its scalar and its correction by `kernel` (k_md_axpy or k_bk_axpy).  Enqueues only.
int block_axpy(stan_ctx *ctx, const char *who, decltype(&k_md_axpy) kernel, int64_t N, int32_t q, const double *d_X,
               const double *scalar, const int32_t *dcol, const double *d_D, double *d_Z) {
    STANCHK(block_args_check(ctx, who, N, q));
    md_cols cols;
    fill_cols(cols, q, scalar, dcol);
    hipLaunchKernelGGL(kernel, dim3(nblk(N, 256), (unsigned)q), dim3(256), 0, ctx->stream, N, d_X, cols, d_D, d_Z);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

// d_phi = the first k columns of X, column j divided by scale[j].  `enqueue(st, rows, cols, nb, t)` launches the pass over the
// rows (grid `rows`: partials per column and workgroup of RT_ROWS rows) and the one workgroup per column (grid `cols`) that
// leaves scale[j].  with_sums: the modal norm's partial sums are allocated too, in front as ever.  Synchronises.
struct normalise_tmp { double *psum = nullptr, *pval = nullptr, *scale = nullptr; long long *pidx = nullptr; };
template <typename Enqueue>
int block_normalise(stan_ctx *ctx, const char *who, int64_t N, int32_t k, const double *d_X, double *d_phi, bool with_sums,
                    Enqueue &&enqueue) {
    STANCHK(block_args_check(ctx, who, N, k));
    hipStream_t st = ctx->stream;
    const int64_t nb = nblk(N, RT_ROWS);
    dev_scope tmp(ctx);
    normalise_tmp t;
    if (with_sums) STANCHK(tmp.alloc(&t.psum, (size_t)k * (size_t)nb));
    STANCHK(tmp.alloc(&t.pval, (size_t)k * (size_t)nb));
    STANCHK(tmp.alloc(&t.pidx, (size_t)k * (size_t)nb));
    STANCHK(tmp.alloc(&t.scale, (size_t)k));
    enqueue(st, dim3((unsigned)nb, (unsigned)k), dim3((unsigned)k), nb, t);
    hipLaunchKernelGGL(k_md_scale, dim3(nblk(N, 256), (unsigned)k), dim3(256), 0, st, N, d_X, t.scale, d_phi);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    return STAN_OK;
}

}  // namespace

int stan_modal_start_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_M, double *d_rhs, int64_t *bad) {
    STANCHK(block_args_check(ctx, "modes", N, q));
    return stan_first_offender(ctx, bad, [&](long long *slot) {
        hipLaunchKernelGGL(k_md_start, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, (int)q, d_M, d_rhs, slot);
    });
}

int stan_modal_gram_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_M, double *A,
                           double *B) {
    STANCHK(block_args_check(ctx, "block_gram", N, q));
    hipStream_t st = ctx->stream;
    const int64_t nb = nblk(N, GR_ROWS);
    const int nv = 2 * q * q;
    dev_scope tmp(ctx);
    double *d_partial, *d_out;
    STANCHK(tmp.alloc(&d_partial, (size_t)nv * (size_t)nb));
    STANCHK(tmp.alloc(&d_out, (size_t)nv));
    if (q <= 16)
        hipLaunchKernelGGL((k_md_gram<1, 4>), dim3((unsigned)nb), dim3(256), 0, st, N, (int)q, d_Z, d_W, d_M, d_partial);
    else
        hipLaunchKernelGGL((k_md_gram<4, 8>), dim3((unsigned)nb), dim3(256), 0, st, N, (int)q, d_Z, d_W, d_M, d_partial);
    std::vector<double> out((size_t)nv);
    STANCHK(finish_sums(ctx, nb, out.size(), d_partial, d_out, out.data()));
    for (int k = 0; k < q * q; k++) { A[k] = out[(size_t)k]; B[k] = out[(size_t)(q * q + k)]; }
    return STAN_OK;
}

int stan_modal_rotate_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_M,
                             const double *Q, const double *lambda, uint32_t mask, double *d_X, double *d_KX, double *d_rhs,
                             double *rho2) {
    STANCHK(block_args_check(ctx, "block_rotate", N, q));
    hipStream_t st = ctx->stream;
    rotate_call c(ctx);
    STANCHK(c.prepare(N, q, Q, lambda, (size_t)q));
    with_qt(c.QT, [&](auto qt) {
        hipLaunchKernelGGL(k_md_rotate<decltype(qt)::value>, dim3((unsigned)c.nb), dim3(256), 0, st, N, (int)q, d_Z, d_W, d_M, c.d_Qp,
                           c.cols, mask, d_X, d_KX, d_rhs, c.d_partial);
    });
    return finish_sums(ctx, c.nb, (size_t)q, c.d_partial, c.d_out, rho2);
}

int stan_modal_axpy_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_X, const double *lambda, const int32_t *dcol,
                           const double *d_D, double *d_Z) {
    return block_axpy(ctx, "modes", k_md_axpy, N, q, d_X, lambda, dcol, d_D, d_Z);
}

int stan_modal_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, const double *d_M, double *d_phi) {
    return block_normalise(ctx, "modes", N, k, d_X, d_phi, true, [&](hipStream_t st, dim3 rows, dim3 cols, int64_t nb, const normalise_tmp &t) {
        hipLaunchKernelGGL(k_md_colstats, rows, dim3(256), 0, st, N, d_X, d_M, t.psum, t.pval, t.pidx);
        hipLaunchKernelGGL(k_md_colfinish, cols, dim3(256), 0, st, nb, t.psum, t.pval, t.pidx, t.scale);
    });
}

// ---- the buckling driver's block kernels ----------------------------------------------------------------------------------
int stan_pencil_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, const double *d_MX, double *d_phi) {
    return block_normalise(ctx, "modes_pencil", N, k, d_X, d_phi, true, [&](hipStream_t st, dim3 rows, dim3 cols, int64_t nb, const normalise_tmp &t) {
        hipLaunchKernelGGL(k_pc_colstats, rows, dim3(256), 0, st, N, d_X, d_MX, t.psum, t.pval, t.pidx);
        hipLaunchKernelGGL(k_md_colfinish, cols, dim3(256), 0, st, nb, t.psum, t.pval, t.pidx, t.scale);
    });
}

int stan_buckling_start_device(stan_ctx *ctx, int64_t N, int32_t q, double *d_X0) {
    STANCHK(block_args_check(ctx, "buckling", N, q));
    hipLaunchKernelGGL(k_bk_start, dim3(nblk(N, 256)), dim3(256), 0, ctx->stream, N, (int)q, d_X0);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_buckling_negate_device(stan_ctx *ctx, int64_t n, double *d_y) {
    if (n > 0) hipLaunchKernelGGL(k_bk_negate, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, n, d_y);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_buckling_rotate_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_Y,
                                const double *d_D, const double *Q, const double *mu, uint32_t mask, double *d_X, double *d_KX,
                                double *d_rhs, double *r2, double *kx2) {
    STANCHK(block_args_check(ctx, "buckling_rotate", N, q));
    hipStream_t st = ctx->stream;
    rotate_call c(ctx);
    STANCHK(c.prepare(N, q, Q, mu, 2 * (size_t)q));
    with_qt(c.QT, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        const dim3 g((unsigned)c.nb), b(256);
        hipLaunchKernelGGL(k_bk_rotate_x<QT>, g, b, 0, st, N, (int)q, d_Z, c.d_Qp, d_X);
        hipLaunchKernelGGL(k_bk_residual<QT>, g, b, 0, st, N, (int)q, d_W, d_Y, d_D, c.d_Qp, c.cols, mask, d_KX, d_rhs, c.d_partial);
    });
    std::vector<double> out(2 * (size_t)q);
    STANCHK(finish_sums(ctx, c.nb, out.size(), c.d_partial, c.d_out, out.data()));
    for (int j = 0; j < q; j++) { r2[j] = out[(size_t)j]; kx2[j] = out[(size_t)(q + j)]; }
    return STAN_OK;
}

int stan_buckling_axpy_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_X, const double *mu, const int32_t *dcol,
                              const double *d_D, double *d_Z) {
    return block_axpy(ctx, "buckling", k_bk_axpy, N, q, d_X, mu, dcol, d_D, d_Z);
}

int stan_buckling_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, double *d_phi) {
    return block_normalise(ctx, "buckling", N, k, d_X, d_phi, false, [&](hipStream_t st, dim3 rows, dim3 cols, int64_t nb, const normalise_tmp &t) {
        hipLaunchKernelGGL(k_bk_colmax, rows, dim3(256), 0, st, N, d_X, t.pval, t.pidx);
        hipLaunchKernelGGL(k_bk_colmax_finish, cols, dim3(256), 0, st, nb, t.pval, t.pidx, t.scale);
    });
}
