// transient.hip -- the step kernels of the implicit Newmark integrator (api_transient.hip).  Bandwidth
// kernels over vectors [N] the drivers own: every base is 16-byte aligned (device allocations; a user's arrays are staged by
// the drivers, which read and write them one element wide or by copies), so a lane moves one pair (double2) per vector and the
// grid is sized from N: STAN_NM_ROWS = 512 entries per workgroup of 256 lanes.  An odd N ends in a lane that moves one entry.
//   start    a_0 = (g F - alpha_R M o v0 - beta_R K v0 - K u0) / M
//   w        w = a1 u + a4 v + a5 a, the operand of the damping product (beta_R != 0 only)
//   predict  b = (g F + M o (p + alpha_R w) + beta_R Kw) / c_K with p = a0 u + a2 v + a3 a; two forms: with Kw and without
//   correct  a' = a0 (u' - u) - a2 v - a3 a, v' = v + dt ((1 - gamma) a + gamma a'), u, v, a replaced in place; with energies:
//            the workgroup's sums of 1/2 v' M v', 1/2 u' (K u'), g F u' from the same pass
//   probe    row[j] = u[probe[j]]
// Bit-reproducible: no atomics on doubles; a workgroup's sum has a fixed order (block_sums), the workgroups' partial sums are
// added in workgroup order by one workgroup per value (k_finish_sums of elem_pass.h, which modal.hip uses too).
#include "elem_pass.h"   // block_sums, k_finish_sums

namespace {

constexpr int NM_T = 256;
static_assert(STAN_NM_ROWS == 2 * NM_T, "one pair per lane");

struct pair2 { double x, y; };
// entries 2 i and 2 i + 1 of a 16-byte aligned vector; the second is 0 beyond N
__device__ __forceinline__ pair2 ld2(const double *__restrict__ p, int64_t i, bool both) {
    if (both) { const double2 t = *reinterpret_cast<const double2 *>(p + 2 * i); return {t.x, t.y}; }
    return {p[2 * i], 0.0};
}
__device__ __forceinline__ void st2(double *__restrict__ p, int64_t i, bool both, pair2 v) {
    if (both) *reinterpret_cast<double2 *>(p + 2 * i) = make_double2(v.x, v.y);
    else p[2 * i] = v.x;
}

__device__ __forceinline__ double nm_p(const stan_newmark_coef &c, double u, double v, double a) { return c.a0 * u + c.a2 * v + c.a3 * a; }
__device__ __forceinline__ double nm_w(const stan_newmark_coef &c, double u, double v, double a) { return c.a1 * u + c.a4 * v + c.a5 * a; }

template <bool V0, bool KV, bool KU>
__global__ void __launch_bounds__(NM_T)
k_nm_start(int64_t N, stan_newmark_coef c, double gF, const double *__restrict__ F, const double *__restrict__ M,
           const double *__restrict__ v0, const double *__restrict__ Kv, const double *__restrict__ Ku, double *__restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    if (2 * i >= N) return;
    const bool both = 2 * i + 1 < N;
    const pair2 f = ld2(F, i, both), m = ld2(M, i, both);
    pair2 r = {gF * f.x, gF * f.y};
    if (V0) { const pair2 t = ld2(v0, i, both); r.x -= c.alpha_R * (m.x * t.x); r.y -= c.alpha_R * (m.y * t.y); }
    if (KV) { const pair2 t = ld2(Kv, i, both); r.x -= c.beta_R * t.x; r.y -= c.beta_R * t.y; }
    if (KU) { const pair2 t = ld2(Ku, i, both); r.x -= t.x; r.y -= t.y; }
    st2(a, i, both, {r.x / m.x, both ? r.y / m.y : 0.0});
}

__global__ void __launch_bounds__(NM_T)
k_nm_w(int64_t N, stan_newmark_coef c, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ a,
       double *__restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    if (2 * i >= N) return;
    const bool both = 2 * i + 1 < N;
    const pair2 pu = ld2(u, i, both), pv = ld2(v, i, both), pa = ld2(a, i, both);
    st2(w, i, both, {nm_w(c, pu.x, pv.x, pa.x), nm_w(c, pu.y, pv.y, pa.y)});
}

template <bool KW>
__global__ void __launch_bounds__(NM_T)
k_nm_predict(int64_t N, stan_newmark_coef c, double gF, const double *__restrict__ u, const double *__restrict__ v,
             const double *__restrict__ a, const double *__restrict__ F, const double *__restrict__ M, const double *__restrict__ Kw,
             double *__restrict__ b) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    if (2 * i >= N) return;
    const bool both = 2 * i + 1 < N;
    const pair2 pu = ld2(u, i, both), pv = ld2(v, i, both), pa = ld2(a, i, both), f = ld2(F, i, both), m = ld2(M, i, both);
    pair2 r;
    r.x = gF * f.x + m.x * (nm_p(c, pu.x, pv.x, pa.x) + c.alpha_R * nm_w(c, pu.x, pv.x, pa.x));
    r.y = gF * f.y + m.y * (nm_p(c, pu.y, pv.y, pa.y) + c.alpha_R * nm_w(c, pu.y, pv.y, pa.y));
    if (KW) { const pair2 t = ld2(Kw, i, both); r.x += c.beta_R * t.x; r.y += c.beta_R * t.y; }
    st2(b, i, both, {r.x / c.c_K, r.y / c.c_K});
}

// the workgroup's three sums into partial[v * gridDim.x + blockIdx.x]
__device__ __forceinline__ void nm_energy_out(double (&s)[3], double *__restrict__ partial) {
    __shared__ double sh[4][3];
    block_sums(s, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; k++) partial[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
}
__device__ __forceinline__ void nm_energy_terms(double (&s)[3], pair2 u, pair2 v, pair2 m, pair2 f, pair2 ku, double gF) {
    s[0] = 0.5 * ((m.x * v.x) * v.x + (m.y * v.y) * v.y);
    s[1] = 0.5 * (u.x * ku.x + u.y * ku.y);
    s[2] = gF * (f.x * u.x + f.y * u.y);
}

template <bool ENERGY>
__global__ void __launch_bounds__(NM_T)
k_nm_correct(int64_t N, stan_newmark_coef c, const double *__restrict__ un, double *__restrict__ u, double *__restrict__ v,
             double *__restrict__ a, const double *__restrict__ M, const double *__restrict__ F, const double *__restrict__ Ku,
             double gF, double *__restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    if (2 * i < N) {
        const bool both = 2 * i + 1 < N;
        const pair2 pn = ld2(un, i, both), pu = ld2(u, i, both), pv = ld2(v, i, both), pa = ld2(a, i, both);
        pair2 an, vn;
        an.x = c.a0 * (pn.x - pu.x) - c.a2 * pv.x - c.a3 * pa.x;
        an.y = c.a0 * (pn.y - pu.y) - c.a2 * pv.y - c.a3 * pa.y;
        vn.x = pv.x + c.dt * ((1.0 - c.gamma) * pa.x + c.gamma * an.x);
        vn.y = pv.y + c.dt * ((1.0 - c.gamma) * pa.y + c.gamma * an.y);
        st2(u, i, both, pn);
        st2(v, i, both, vn);
        st2(a, i, both, an);
        if (ENERGY) nm_energy_terms(s, pn, vn, ld2(M, i, both), ld2(F, i, both), ld2(Ku, i, both), gF);
    }
    if (ENERGY) nm_energy_out(s, partial);
}

__global__ void __launch_bounds__(NM_T)
k_nm_energy(int64_t N, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ M,
            const double *__restrict__ F, const double *__restrict__ Ku, double gF, double *__restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    if (2 * i < N) {
        const bool both = 2 * i + 1 < N;
        nm_energy_terms(s, ld2(u, i, both), ld2(v, i, both), ld2(M, i, both), ld2(F, i, both), ld2(Ku, i, both), gF);
    }
    nm_energy_out(s, partial);
}

__global__ void __launch_bounds__(64)
k_nm_probe(int32_t n_probe, const int32_t *__restrict__ probe, const double *__restrict__ u, double *__restrict__ row) {
    const int32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j < n_probe) row[j] = u[probe[j]];
}
__global__ void __launch_bounds__(64)
k_nm_probe_check(int64_t N, int32_t n_probe, const int32_t *__restrict__ probe, long long *bad) {
    const int32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j < n_probe && (probe[j] < 0 || probe[j] >= N)) atomicMin(bad, (long long)j);
}

int nm_args(stan_ctx *ctx, int64_t N) {
    if (N <= 0 || N > ((int64_t)1 << 31) - 1) { ctx->err = "newmark: N must be in [1, 2^31)"; return STAN_E_ARG; }
    return STAN_OK;
}
unsigned nm_grid(int64_t N) { return (unsigned)stan_newmark_blocks(N); }

}  // namespace

int stan_newmark_start_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, double gF, const double *F, const double *M,
                              const double *v0, const double *Kv0, const double *Ku0, double *a) {
    STANCHK(nm_args(ctx, N));
    const dim3 g(nm_grid(N)), t(NM_T);
    hipStream_t st = ctx->stream;
#define NM_START(V, KV, KU) hipLaunchKernelGGL((k_nm_start<V, KV, KU>), g, t, 0, st, N, c, gF, F, M, v0, Kv0, Ku0, a)
    switch ((v0 ? 4 : 0) | (Kv0 ? 2 : 0) | (Ku0 ? 1 : 0)) {
        case 0: NM_START(false, false, false); break;
        case 1: NM_START(false, false, true); break;
        case 2: NM_START(false, true, false); break;
        case 3: NM_START(false, true, true); break;
        case 4: NM_START(true, false, false); break;
        case 5: NM_START(true, false, true); break;
        case 6: NM_START(true, true, false); break;
        default: NM_START(true, true, true); break;
    }
#undef NM_START
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_w_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, const double *u, const double *v, const double *a, double *w) {
    STANCHK(nm_args(ctx, N));
    hipLaunchKernelGGL(k_nm_w, dim3(nm_grid(N)), dim3(NM_T), 0, ctx->stream, N, c, u, v, a, w);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_predict_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, double gF, const double *u, const double *v,
                                const double *a, const double *F, const double *M, const double *Kw, double *b) {
    STANCHK(nm_args(ctx, N));
    if (Kw) hipLaunchKernelGGL(k_nm_predict<true>, dim3(nm_grid(N)), dim3(NM_T), 0, ctx->stream, N, c, gF, u, v, a, F, M, Kw, b);
    else hipLaunchKernelGGL(k_nm_predict<false>, dim3(nm_grid(N)), dim3(NM_T), 0, ctx->stream, N, c, gF, u, v, a, F, M, Kw, b);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_correct_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, const double *u_new, double *u, double *v,
                                double *a, const double *M, const double *F, const double *Ku, double gF, double *d_partial,
                                double *d_energy) {
    STANCHK(nm_args(ctx, N));
    const unsigned g = nm_grid(N);
    if (d_energy) {
        hipLaunchKernelGGL(k_nm_correct<true>, dim3(g), dim3(NM_T), 0, ctx->stream, N, c, u_new, u, v, a, M, F, Ku, gF, d_partial);
        hipLaunchKernelGGL(k_finish_sums<NM_T>, dim3(3), dim3(NM_T), 0, ctx->stream, (int64_t)g, d_partial, d_energy);
    } else
        hipLaunchKernelGGL(k_nm_correct<false>, dim3(g), dim3(NM_T), 0, ctx->stream, N, c, u_new, u, v, a, M, F, Ku, gF, d_partial);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_energy_device(stan_ctx *ctx, int64_t N, const double *u, const double *v, const double *M, const double *F,
                               const double *Ku, double gF, double *d_partial, double *d_energy) {
    STANCHK(nm_args(ctx, N));
    const unsigned g = nm_grid(N);
    hipLaunchKernelGGL(k_nm_energy, dim3(g), dim3(NM_T), 0, ctx->stream, N, u, v, M, F, Ku, gF, d_partial);
    hipLaunchKernelGGL(k_finish_sums<NM_T>, dim3(3), dim3(NM_T), 0, ctx->stream, (int64_t)g, d_partial, d_energy);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_probe_device(stan_ctx *ctx, int32_t n_probe, const int32_t *d_probe, const double *u, double *row) {
    if (n_probe <= 0) return STAN_OK;
    hipLaunchKernelGGL(k_nm_probe, dim3(nblk(n_probe, 64)), dim3(64), 0, ctx->stream, n_probe, d_probe, u, row);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

int stan_newmark_probe_check_device(stan_ctx *ctx, int64_t N, int32_t n_probe, const int32_t *d_probe, int64_t *bad) {
    *bad = -1;
    if (n_probe <= 0) return STAN_OK;
    return stan_first_offender(ctx, bad, [&](long long *slot) {
        hipLaunchKernelGGL(k_nm_probe_check, dim3(nblk(n_probe, 64)), dim3(64), 0, ctx->stream, N, n_probe, d_probe, slot);
    });
}
