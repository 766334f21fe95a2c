// explicit.hip -- the kernels of the explicit central-difference integrator and of its stable step (api_explicit.hip, DESIGN.md
// section 3.14).  The driver keeps every vector in the product's own padded full numbering (3 * nslices * 64 doubles, index
// 3 * row + m; fixed DOFs and padding carry u = 0, F = 0, M = 1), so a step is a plain vector pass with no index map: a lane
// moves one pair (double2) per vector, STAN_CD_ROWS = 512 entries per workgroup of 256 lanes, an odd n ends in a lane that
// moves one entry (transient.hip's form).  With dt2 = dt dt, two_dt = 2 dt, h = alpha_R dt / 2, om = 1 - h, op = 1 + h (formed
// on the host, stan_cd_make_coef) one update is, per entry and in this order of operations:
//   Ku  = y                      (plain)     y / s      (scaled: K carries S K S, y = A^ (u_n / s))
//   r   = fma(gF, F, -Ku)
//   q   = r / M
//   t   = fma(-om, u_p, 2 u_n)               u_p = u_{n-1}; 2 u_n is exact
//   u'  = fma(dt2, q, t) / op                u_{n+1}, stored over u_p; scaled: xh = u' / s next to it
//   v_n = (u' - u_p) / two_dt                (state form)
//   a_n = ((u' - 2 u_n) + u_p) / dt2         (state form)
//   energies (energy form): the workgroup's sums of 1/2 (M v_n) v_n, 1/2 u_n Ku, gF (F u_n) over the lane's pair, the second
//            product of a pair joined by an fma; v_n formed in registers
//   flag: atomicMin(flag, step) where u' is not finite
// and the start is a_0 = fma(-alpha_R, M v0, fma(gF, F, -Ku)) / M, u_{-1} = fma(dt2 / 2, a_0, fma(-dt, v0, u0)).  Every product
// that feeds a sum is written as an fma, so the library's -ffp-contract=fast has nothing left to choose: every template form of
// the update gives u' the same bits, and a run does not depend on which steps record.  tests/explicit_ref.py restates the lines
// above (its fp64 form rounds the product of an fma once more: inside the bounds the tests derive).
// The stable step: k_row_bound walks K's layout as k_shift_matrix does (a wavefront per slice, a lane per row) and takes the
// largest (sum_j |K_dj|) / M_d over the free DOFs, the sums over the exported values (stan_unscaled_value) of the free entries
// in slot order; the maximum is order-free (an integer atomicMax on the bits of a non-negative double): the same bits twice.
// The power sums have block_sums' fixed order and no atomics on doubles; the two sums of the quotient are carried as pairs hi + lo.
#include <cmath>
#include <cstring>

#include "elem_pass.h"   // block_sums, k_finish_sums

namespace {

constexpr int CD_T = 256;
static_assert(STAN_CD_ROWS == 2 * CD_T, "one pair per lane");

struct pair2 { double x, y; };
// entries 2 i and 2 i + 1 of a 16-byte aligned vector; the second is `pad` beyond n
__device__ __forceinline__ pair2 ld2(const double *__restrict__ p, int64_t i, bool both, double pad = 0.0) {
    if (both) { const double2 t = *reinterpret_cast<const double2 *>(p + 2 * i); return {t.x, t.y}; }
    return {p[2 * i], pad};
}
__device__ __forceinline__ void st2(double *__restrict__ p, int64_t i, bool both, pair2 v) {
    if (both) *reinterpret_cast<double2 *>(p + 2 * i) = make_double2(v.x, v.y);
    else p[2 * i] = v.x;
}
__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the workgroup's three sums into partial[k * gridDim.x + blockIdx.x]
__device__ __forceinline__ void sums_out(double (&s)[3], double *__restrict__ partial) {
    __shared__ double sh[4][3];
    block_sums(s, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; k++) partial[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
}

__global__ void __launch_bounds__(CD_T)
k_cd_expand(int64_t n_dof, int64_t n_pad, const int32_t *__restrict__ red, const double *__restrict__ in, const double *__restrict__ div,
            double fill, double *__restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    if (d >= n_pad) return;
    const int32_t rd = d < n_dof ? red[d] : -1;
    double v = rd == -1 ? fill : in ? in[d - rd] : 0.0;
    if (div) v /= div[d];
    out[d] = v;
}
__global__ void __launch_bounds__(CD_T)
k_cd_compress(int64_t n_dof, const int32_t *__restrict__ red, const double *__restrict__ full, double *__restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    if (d >= n_dof) return;
    const int32_t rd = red[d];
    if (rd != -1) out[d - rd] = full[d];
}
__global__ void __launch_bounds__(CD_T)
k_cd_index(int64_t n_dof, const int32_t *__restrict__ red, int32_t *__restrict__ full_of) {
    const int64_t d = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    if (d >= n_dof) return;
    const int32_t rd = red[d];
    if (rd != -1) full_of[d - rd] = (int32_t)d;
}

__global__ void __launch_bounds__(CD_T)
k_cd_start(int64_t n, stan_cd_coef c, double gF, const double *__restrict__ y, const double *__restrict__ s, const double *__restrict__ u,
           const double *__restrict__ v, const double *__restrict__ M, const double *__restrict__ F, double *__restrict__ a,
           double *__restrict__ up) {
    const int64_t i = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    if (2 * i >= n) return;
    const bool both = 2 * i + 1 < n;
    pair2 ku = ld2(y, i, both);
    if (s) { const pair2 t = ld2(s, i, both, 1.0); ku.x /= t.x; ku.y /= t.y; }
    const pair2 pu = ld2(u, i, both), pv = ld2(v, i, both), m = ld2(M, i, both, 1.0), f = ld2(F, i, both);
    pair2 a0;
    a0.x = fma(-c.alpha_R, m.x * pv.x, fma(gF, f.x, -ku.x)) / m.x;
    a0.y = fma(-c.alpha_R, m.y * pv.y, fma(gF, f.y, -ku.y)) / m.y;
    const double half = c.dt2 / 2.0;
    st2(a, i, both, a0);
    st2(up, i, both, {fma(half, a0.x, fma(-c.dt, pv.x, pu.x)), fma(half, a0.y, fma(-c.dt, pv.y, pu.y))});
}

template <bool SCALED, bool STATE, bool ENERGY>
__global__ void __launch_bounds__(CD_T)
k_cd_update(int64_t n, stan_cd_coef c, double gF, long long step, const double *__restrict__ y, const double *__restrict__ s,
            const double *__restrict__ un, double *__restrict__ up, const double *__restrict__ M, const double *__restrict__ F,
            double *__restrict__ xh, double *__restrict__ v, double *__restrict__ a, double *__restrict__ partial, long long *flag) {
    const int64_t i = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    double e[3] = {0.0, 0.0, 0.0};
    if (2 * i < n) {
        const bool both = 2 * i + 1 < n;
        pair2 ku = ld2(y, i, both), sc = {1.0, 1.0};
        if (SCALED) { sc = ld2(s, i, both, 1.0); ku.x /= sc.x; ku.y /= sc.y; }
        const pair2 u = ld2(un, i, both), p = ld2(up, i, both), m = ld2(M, i, both, 1.0), f = ld2(F, i, both);
        pair2 w;
        w.x = fma(c.dt2, fma(gF, f.x, -ku.x) / m.x, fma(-c.om, p.x, 2.0 * u.x)) / c.op;
        w.y = fma(c.dt2, fma(gF, f.y, -ku.y) / m.y, fma(-c.om, p.y, 2.0 * u.y)) / c.op;
        st2(up, i, both, w);
        if (SCALED) st2(xh, i, both, {w.x / sc.x, w.y / sc.y});
        if (!finite(w.x) || !finite(w.y)) atomicMin(flag, step);
        if (STATE || ENERGY) {
            const pair2 vn = {(w.x - p.x) / c.two_dt, (w.y - p.y) / c.two_dt};
            if (STATE) {
                st2(v, i, both, vn);
                st2(a, i, both, {((w.x - 2.0 * u.x) + p.x) / c.dt2, ((w.y - 2.0 * u.y) + p.y) / c.dt2});
            }
            if (ENERGY) {
                e[0] = 0.5 * fma(m.x * vn.x, vn.x, (m.y * vn.y) * vn.y);
                e[1] = 0.5 * fma(u.x, ku.x, u.y * ku.y);
                e[2] = gF * fma(f.x, u.x, f.y * u.y);
            }
        }
    }
    if (ENERGY) sums_out(e, partial);
}

__global__ void __launch_bounds__(64)
k_cd_probe(int32_t n_probe, const int32_t *__restrict__ probe, const int32_t *__restrict__ full_of, const double *__restrict__ u,
           double *__restrict__ row) {
    const int32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j < n_probe) row[j] = u[full_of[probe[j]]];
}

// the largest (sum_j |K_dj|) / M_d of the slice's free DOFs into *out (the bits of a non-negative double order as integers)
__global__ void __launch_bounds__(256)
k_row_bound(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
            const int32_t *__restrict__ rowlen, const int32_t *__restrict__ cols, const double *__restrict__ vals,
            const double *__restrict__ s, const uint8_t *__restrict__ fixmask, const double *__restrict__ Mf, unsigned long long *out) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int64_t row = rowof[slice * 64 + lane];
    const bool live = row < nloc;
    const int32_t len = live ? rowlen[row] : 0;
    const int rfix = live ? fixmask[row] : 7;
    double sr[3] = {1.0, 1.0, 1.0}, sum[3] = {0.0, 0.0, 0.0};
    if (live && s)
#pragma unroll
        for (int m = 0; m < 3; m++) sr[m] = s[3 * row + m];
    const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
    for (int32_t k = k0; k < k1; k++) {
        if (k - k0 >= len) continue;   // a padding slot of this row
        const int32_t c = cols[(int64_t)k * 64 + lane];
        const int cfix = fixmask[c];
        double sc[3] = {1.0, 1.0, 1.0};
        if (s) { sc[0] = s[3 * (int64_t)c]; sc[1] = s[3 * (int64_t)c + 1]; sc[2] = s[3 * (int64_t)c + 2]; }
        const double *v = vals + (int64_t)k * 9 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) {
                double a = v[(3 * m + n) * 64];
                if (((rfix >> m) & 1) || ((cfix >> n) & 1)) continue;
                if (s) a = stan_unscaled_value(a, sr[m], sc[n]);
                sum[m] += fabs(a);
            }
    }
    double best = 0.0;
    if (live)
#pragma unroll
        for (int m = 0; m < 3; m++)
            if (!((rfix >> m) & 1)) best = fmax(best, sum[m] / Mf[3 * row + m]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
    if (lane == 0) atomicMax(out, (unsigned long long)__double_as_longlong(best));
}

// The two sums of the Rayleigh quotient are carried as unevaluated pairs hi + lo (error-free products and sums: Dekker, Knuth):
// summed plainly, N terms leave the quotient a unit in the last place or two from its value, whichever order adds them; as pairs
// the quotient is the double nearest to what the vectors give.  The order is as fixed as block_sums': six butterfly stages per
// wave, the four waves in order, the workgroups in order.
struct dsum { double hi, lo; };
__device__ __forceinline__ dsum two_prod(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));   // p is the ROUNDED product wherever it is used: no contraction into a later sum
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dsum dsum_add(dsum a, dsum b) {
    const double s = a.hi + b.hi, bb = s - a.hi;
    const double e = ((a.hi - (s - bb)) + (b.hi - bb)) + (a.lo + b.lo);
    const double hi = s + e;
    return {hi, e - (hi - s)};
}
// the block's sum of v on thread 0; sh: one slot per wave
__device__ __forceinline__ dsum block_dsum(dsum v, dsum *sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = dsum_add(v, dsum{__shfl_xor(v.hi, off, 64), __shfl_xor(v.lo, off, 64)});
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) v = dsum_add(v, sh[w]);
    return v;
}

// partial [5][gridDim.x]: x.Kx hi, lo; x.(M x) hi, lo; Kx.Kx / M (the norm of the next iterate: a plain sum)
template <bool SCALED>
__global__ void __launch_bounds__(CD_T)
k_power_sums(int64_t n, const double *__restrict__ y, const double *__restrict__ s, const double *__restrict__ x,
             const double *__restrict__ M, double *__restrict__ partial) {
    __shared__ dsum sh[2][4];
    __shared__ double shc[4][1];
    const int64_t i = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    dsum a = {0.0, 0.0}, b = {0.0, 0.0};
    double c[1] = {0.0};
    if (2 * i < n) {
        const bool both = 2 * i + 1 < n;
        pair2 kx = ld2(y, i, both);
        if (SCALED) { const pair2 t = ld2(s, i, both, 1.0); kx.x /= t.x; kx.y /= t.y; }
        const pair2 px = ld2(x, i, both), m = ld2(M, i, both, 1.0);
        a = dsum_add(two_prod(px.x, kx.x), two_prod(px.y, kx.y));
        b = dsum_add(two_prod(px.x, m.x * px.x), two_prod(px.y, m.y * px.y));
        c[0] = (kx.x * kx.x) / m.x + (kx.y * kx.y) / m.y;
    }
    a = block_dsum(a, sh[0]);
    b = block_dsum(b, sh[1]);
    block_sums(c, shc);
    if (threadIdx.x == 0) {
        const int64_t g = gridDim.x;
        partial[blockIdx.x] = a.hi; partial[g + blockIdx.x] = a.lo;
        partial[2 * g + blockIdx.x] = b.hi; partial[3 * g + blockIdx.x] = b.lo;
        partial[4 * g + blockIdx.x] = c[0];
    }
}
// sums [5] = the workgroups' partial sums in workgroup order: one workgroup; thread t adds blocks t, t + 256, ... in ascending order
__global__ void __launch_bounds__(CD_T)
k_power_finish(int64_t n_blocks, const double *__restrict__ partial, double *__restrict__ sums) {
    __shared__ dsum sh[2][4];
    __shared__ double shc[4][1];
    dsum a = {0.0, 0.0}, b = {0.0, 0.0};
    double c[1] = {0.0};
    for (int64_t k = threadIdx.x; k < n_blocks; k += CD_T) {
        a = dsum_add(a, dsum{partial[k], partial[n_blocks + k]});
        b = dsum_add(b, dsum{partial[2 * n_blocks + k], partial[3 * n_blocks + k]});
        c[0] += partial[4 * n_blocks + k];
    }
    a = block_dsum(a, sh[0]);
    b = block_dsum(b, sh[1]);
    block_sums(c, shc);
    if (threadIdx.x == 0) { sums[0] = a.hi; sums[1] = a.lo; sums[2] = b.hi; sums[3] = b.lo; sums[4] = c[0]; }
}

template <bool SCALED>
__global__ void __launch_bounds__(CD_T)
k_power_next(int64_t n, const double *__restrict__ y, const double *__restrict__ s, const double *__restrict__ M,
             const double *__restrict__ sums, double *__restrict__ x, double *__restrict__ xh) {
    const int64_t i = (int64_t)blockIdx.x * CD_T + threadIdx.x;
    if (2 * i >= n) return;
    const bool both = 2 * i + 1 < n;
    const double nrm = sqrt(sums[4]);
    pair2 kx = ld2(y, i, both), sc = {1.0, 1.0};
    if (SCALED) { sc = ld2(s, i, both, 1.0); kx.x /= sc.x; kx.y /= sc.y; }
    const pair2 m = ld2(M, i, both, 1.0);
    const pair2 z = {(kx.x / m.x) / nrm, (kx.y / m.y) / nrm};
    st2(x, i, both, z);
    if (SCALED) st2(xh, i, both, {z.x / sc.x, z.y / sc.y});
}

int cd_args(stan_ctx *ctx, int64_t n) {
    if (n <= 0 || n > ((int64_t)1 << 31) - 1) { ctx->err = "explicit: n must be in [1, 2^31)"; return STAN_E_ARG; }
    return STAN_OK;
}
unsigned cd_grid(int64_t n) { return (unsigned)stan_cd_blocks(n); }

}  // namespace

int stan_cd_expand_device(stan_ctx *ctx, int64_t n_dof, int64_t n_pad, const int32_t *d_red, const double *in, const double *div,
                          double fill, double *out) {
    STANCHK(cd_args(ctx, n_pad));
    hipLaunchKernelGGL(k_cd_expand, dim3(nblk(n_pad, CD_T)), dim3(CD_T), 0, ctx->stream, n_dof, n_pad, d_red, in, div, fill, out);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_cd_compress_device(stan_ctx *ctx, int64_t n_dof, const int32_t *d_red, const double *full, double *out) {
    STANCHK(cd_args(ctx, n_dof));
    hipLaunchKernelGGL(k_cd_compress, dim3(nblk(n_dof, CD_T)), dim3(CD_T), 0, ctx->stream, n_dof, d_red, full, out);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_cd_index_device(stan_ctx *ctx, int64_t n_dof, const int32_t *d_red, int32_t *full_of) {
    STANCHK(cd_args(ctx, n_dof));
    hipLaunchKernelGGL(k_cd_index, dim3(nblk(n_dof, CD_T)), dim3(CD_T), 0, ctx->stream, n_dof, d_red, full_of);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_cd_start_device(stan_ctx *ctx, int64_t n, const stan_cd_coef &c, double gF, const double *y, const double *s, const double *u,
                         const double *v, const double *M, const double *F, double *a, double *up) {
    STANCHK(cd_args(ctx, n));
    hipLaunchKernelGGL(k_cd_start, dim3(cd_grid(n)), dim3(CD_T), 0, ctx->stream, n, c, gF, y, s, u, v, M, F, a, up);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_cd_update_device(stan_ctx *ctx, int64_t n, const stan_cd_coef &c, double gF, long long step, const double *y, const double *s,
                          const double *un, double *up, const double *M, const double *F, double *xh, double *v, double *a,
                          double *d_partial, double *d_energy, long long *flag) {
    STANCHK(cd_args(ctx, n));
    const dim3 g(cd_grid(n)), t(CD_T);
    hipStream_t st = ctx->stream;
#define CD_UPDATE(S, V, E) hipLaunchKernelGGL((k_cd_update<S, V, E>), g, t, 0, st, n, c, gF, step, y, s, un, up, M, F, xh, v, a, d_partial, flag)
    switch ((s ? 4 : 0) | (v ? 2 : 0) | (d_energy ? 1 : 0)) {
        case 0: CD_UPDATE(false, false, false); break;
        case 1: CD_UPDATE(false, false, true); break;
        case 2: CD_UPDATE(false, true, false); break;
        case 3: CD_UPDATE(false, true, true); break;
        case 4: CD_UPDATE(true, false, false); break;
        case 5: CD_UPDATE(true, false, true); break;
        case 6: CD_UPDATE(true, true, false); break;
        default: CD_UPDATE(true, true, true); break;
    }
#undef CD_UPDATE
    if (d_energy) hipLaunchKernelGGL(k_finish_sums<CD_T>, dim3(3), t, 0, st, (int64_t)g.x, d_partial, d_energy);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_cd_probe_device(stan_ctx *ctx, int32_t n_probe, const int32_t *d_probe, const int32_t *full_of, const double *u, double *row) {
    if (n_probe <= 0) return STAN_OK;
    hipLaunchKernelGGL(k_cd_probe, dim3(nblk(n_probe, 64)), dim3(64), 0, ctx->stream, n_probe, d_probe, full_of, u, row);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_row_bound_device(stan_ctx *ctx, stan_matrix *K, const double *Mf, double *bound) {
    hipStream_t st = ctx->stream;
    unsigned long long *slot = (unsigned long long *)(ctx->d_status + SS_AUX);
    HIPCHK(ctx, hipMemsetAsync(slot, 0, 8, st));
    if (K->nslices > 0)
        hipLaunchKernelGGL(k_row_bound, dim3(nblk(K->nslices, 4)), dim3(256), 0, st, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                           K->d_rowlen, K->d_cols, K->vals64(), K->scaled ? K->d_scale : (const double *)nullptr, K->d_fixmask, Mf, slot);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, slot, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    static_assert(sizeof(double) == sizeof(int64_t), "the slot holds the bits of a double");
    memcpy(bound, ctx->h_status + SS_AUX, 8);
    return STAN_OK;
}

int stan_power_sums_device(stan_ctx *ctx, int64_t n, const double *y, const double *s, const double *x, const double *M,
                           double *d_partial, double *d_sums) {
    STANCHK(cd_args(ctx, n));
    const dim3 g(cd_grid(n)), t(CD_T);
    if (s) hipLaunchKernelGGL(k_power_sums<true>, g, t, 0, ctx->stream, n, y, s, x, M, d_partial);
    else hipLaunchKernelGGL(k_power_sums<false>, g, t, 0, ctx->stream, n, y, s, x, M, d_partial);
    hipLaunchKernelGGL(k_power_finish, dim3(1), t, 0, ctx->stream, (int64_t)g.x, d_partial, d_sums);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_power_next_device(stan_ctx *ctx, int64_t n, const double *y, const double *s, const double *M, const double *d_sums, double *x,
                           double *xh) {
    STANCHK(cd_args(ctx, n));
    const dim3 g(cd_grid(n)), t(CD_T);
    if (s) hipLaunchKernelGGL(k_power_next<true>, g, t, 0, ctx->stream, n, y, s, M, d_sums, x, xh);
    else hipLaunchKernelGGL(k_power_next<false>, g, t, 0, ctx->stream, n, y, s, M, d_sums, x, xh);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}
