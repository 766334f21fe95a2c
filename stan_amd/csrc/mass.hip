// mass.hip -- the consistent mass M_c of a HEX8 mesh as a matrix on K's layout:
//   m_e[a][b] = rho_m sum_g N_a(q_g) N_b(q_g) det J_g w_g,  the 2 x 2 x 2 rule for BOTH element types
// (as the lumped mass of section 3.10 takes it: a one-point rule would leave M_c singular); the element matrix is m_e (x) I_3,
// one scalar per node pair -- the shape of the geometric stiffness.  No step of the reference.  Two phases, both
// bit-reproducible (no atomics on doubles):
//   element pass  k_cm_elem: 8 lanes per element, one per Gauss point (the layout of elem_pass.h); the 8 Gauss-point terms of an
//                 entry are added by three butterfly stages; the 36 entries of the upper triangle leave per element through
//                 LDS as full lines, [n_elem][36], as k_kg_elem's do;
//   row gather    stan_elem_scalars_matrix (geometric.hip): k_kg_gather itself.
// stan_hip_mass_hex8_batch runs k_cm_elem itself on the batch (its elements' corners numbered 0 .. 8n - 1).
#include <cmath>

#include "elem_pass.h"

namespace {

constexpr double GL = 0.57735026918962576451;   // sqrt(1/3)

// ---- element pass: m36 [n_elem][36] ----------------------------------------------------------------------------------------
// Lane g holds the 8 shape values of its point and t_a = N_a det J_g one node at a time; every index is a compile-time constant
// (no scratch).  Entry i of the triangle stays on lane i % 8 (five registers); rho multiplies the finished sum, as the lumped
// mass multiplies its own (k_ld_elem).  No displacement is loaded; the element's type is not read.
__global__ void __launch_bounds__(256)
k_cm_elem(int64_t n_elem, const double *__restrict__ xyz, const int32_t *__restrict__ conn, const int32_t *__restrict__ elem_mat,
          const double *__restrict__ mat_rho, double *__restrict__ m36, long long *bad_elem) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    const elem_lanes L = elem_lanes_here(n_elem);
    double *rec = lds[L.wv] + L.el * ELEM_REC;
    if (L.valid) elem_load_node<false>(rec, L, conn, xyz, nullptr);
    wave_sync();
    double N[8], sc = 0.0, rho = 0.0;
#pragma unroll
    for (int a = 0; a < 8; a++) N[a] = 0.0;
    if (L.valid) {
        const double px = hex8_sign(HEX8_SX, L.g) * GL, py = hex8_sign(HEX8_SY, L.g) * GL, pz = hex8_sign(HEX8_SZ, L.g) * GL;
        double J[9];
        hex8_jacobian(rec, px, py, pz, J);
        sc = hex8_det3(J);   // det J_g * w, w = 1 (a singular point is reported; its term is zero)
        if (sc == 0.0) atomicMin(bad_elem, (long long)L.e);
        rho = mat_rho[elem_mat[L.e]];
#pragma unroll
        for (int a = 0; a < 8; a++) N[a] = hex8_shape(a, px, py, pz);
    }
    double mine[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 8; a++) {
        const double t = N[a] * sc;
#pragma unroll
        for (int b = a; b < 8; b++) {
            const int i = kg_index(a, b);
            const double v = rho * elem_sum(t * N[b]);
            if ((i & 7) == L.g) mine[i >> 3] = v;
        }
    }
    wave_sync();   // every lane is done with the records
    double *stg = lds[L.wv];   // 8 x 36 = 288 of its 400 doubles
#pragma unroll
    for (int j = 0; j < 5; j++)
        if (8 * j + L.g < KG_N) stg[L.el * KG_N + 8 * j + L.g] = mine[j];
    wave_sync();
    double *dst = m36 + L.e0 * KG_N;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int idx = j * 64 + L.lane;
        if (idx < 8 * KG_N && L.e0 + idx / KG_N < n_elem) dst[idx] = stg[idx];
    }
}

// the first element whose material's density is not positive and finite (elem_mat checked by the caller)
__global__ void __launch_bounds__(256)
k_cm_rho_check(int64_t n_elem, const int32_t *__restrict__ elem_mat, const double *__restrict__ mat_rho, long long *bad) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elem) return;
    const double r = mat_rho[elem_mat[e]];
    if (!(r > 0.0) || r > 1.7976931348623157e308) atomicMin(bad, (long long)e);
}

// the element pass on a device view whose integers have been checked; d_rho [n_mat], d_m36 [n_elem][36]; pt (may be null):
// marks 0 and 1 around the kernel
int cm_elem_pass(stan_ctx *ctx, const stan_mesh &d, const double *d_rho, double *d_m36, phase_timer *pt = nullptr) {
    if (pt) STANCHK(pt->mark(0));
    if (d.n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_cm_elem, dim3(nblk(d.n_elem, 32)), dim3(256), 0, ctx->stream, d.n_elem, d.xyz, d.conn, d.elem_mat, d_rho,
                           d_m36, (long long *)(ctx->d_status + SS_BAD_ELEM));
    if (pt) STANCHK(pt->mark(1));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, ctx->d_status + SS_BAD_ELEM, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the caller's host copy of the densities goes with this call
    return stan_detj_check(ctx, " (consistent mass)");
}

}  // namespace

int stan_mass_batch_device(stan_ctx *ctx, int64_t n, const double *d_xyz8, double rho, double *d_m36) {
    if (n <= 0) return STAN_OK;
    if (n >= (int64_t)1 << 28) { ctx->err = "mass_hex8_batch: more than 2^28 elements"; return STAN_E_ARG; }
    dev_scope tmp(ctx);
    int32_t *d_conn, *d_mat;
    double *d_rho;
    STANCHK(tmp.alloc(&d_conn, (size_t)n * 8));
    STANCHK(tmp.alloc(&d_mat, (size_t)n));
    STANCHK(tmp.alloc(&d_rho, 1));
    STANCHK(stan_elem_batch_iota(ctx, n, d_conn, d_mat));
    HIPCHK(ctx, hipMemcpyAsync(d_rho, &rho, 8, hipMemcpyHostToDevice, ctx->stream));   // (cm_elem_pass synchronises)
    const stan_mesh d{.n_nodes = n * 8, .n_elem = n, .n_mat = 1, .xyz = d_xyz8, .conn = d_conn, .elem_mat = d_mat};
    return cm_elem_pass(ctx, d, d_rho, d_m36);
}

int stan_consistent_mass_device(stan_ctx *ctx, stan_matrix *K, const stan_mesh &d, const double *mat_rho, stan_matrix **out) {
    const char *who = "consistent_mass_hex8";
    dev_scope tmp(ctx);
    STANCHK(stan_elem_scalars_matrix_args(ctx, tmp, who, K, d));
    // ---- the densities of the materials in use, before the element scalars or the matrix are allocated
    double *d_rho;
    STANCHK(tmp.alloc(&d_rho, (size_t)d.n_mat));
    HIPCHK(ctx, hipMemcpyAsync(d_rho, mat_rho, (size_t)d.n_mat * 8, hipMemcpyHostToDevice, ctx->stream));
    int64_t bad_at = -1;
    if (d.n_elem > 0)
        STANCHK(stan_first_offender(ctx, &bad_at, [&](long long *slot) {
            hipLaunchKernelGGL(k_cm_rho_check, dim3(nblk(d.n_elem, 256)), dim3(256), 0, ctx->stream, d.n_elem, d.elem_mat, d_rho, slot);
        }));
    else HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad_at >= 0) {
        ctx->err = std::string(who) + ": the density of the material of element " + std::to_string(bad_at) + " is not positive and finite";
        return STAN_E_ARG;
    }
    // ---- the element scalars (the largest temporary: given back with `tmp`)
    double *d_m36;
    STANCHK(tmp.alloc(&d_m36, (size_t)(d.n_elem > 0 ? d.n_elem : 1) * KG_N));
    for (double &ms : ctx->prof_cm_ms) ms = 0;
    phase_timer pt(ctx, 2);
    STANCHK(cm_elem_pass(ctx, d, d_rho, d_m36, &pt));
    STANCHK(pt.read(0, 1, &ctx->prof_cm_ms[0]));
    return stan_elem_scalars_matrix(ctx, tmp, who, K, d, d_m36, out, ctx->prof_cm_ms + 1);
}
