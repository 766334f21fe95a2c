// recovery.hip -- strain/stress recovery after the solve:
// Element.Recovery_Stress (Element.cs:211-246) + Update_StrainStress (:257-267) with the
// extrapolation table FE_Library.HEX8_ShapeFunctions (FE_Library.cs:105-116, 285-321).
//   eps_g = B_g u_e, sig_g = D eps_g at the 8 Gauss points, then per node
//   value_i = sum_g N[i][g] value_g,  N[i][g] = shape function g at xi = (+-1)/(1/sqrt 3).
// The reference reads the B_g it cached during K_Initial (~10 KB per element); here B_g is
// recomputed from the coordinates (embarrassingly parallel, 8 lanes per element = one per
// Gauss point, node extrapolation through wavefront shuffles).
// Compute_NodalForces (Element.cs:248-255) + the R assembly (Solver.cs:189-196) are the FORCES
// variant of the same kernel: f_e = sum_g B_g^T dS[g] det J_g w, with dS[g] the NODE-extrapolated
// stress of node g exactly as the reference indexes it; R[DOF] accumulates with fp64 atomics
// (the reference's own "+=" under Parallel.ForEach is an unsynchronised race).  The linear-static
// driver discards R (Solver.cs:199), so the console driver does not ask for it.
// HEX8_G1 makes the reference throw (N has one row, indexed by node: Element.cs:242 vs
// FE_Library.cs:77-81): reported as STAN_E_UNSUPPORTED with the element index.
#include "elem_pass.h"

namespace {

// Round 5 (profiles/r05/k_recover_n148_kernel_trace_summary_r05_final.txt): the first form let each of the 8 lanes of an element load all 8 nodes' coordinates
// and displacements itself (56 gathers per lane) and store its 6 + 6 values 48 B apart: 1.73 ms at 148^3 for 3.2 GB =
// 0.23 of the HBM peak, bound by the address pipeline.  Now the element pass of elem_pass.h (lane i loads node i only, the
// element's record goes round through LDS); the node extrapolation value_i = sum_g N[i][g] value_g uses the tensor structure
// of N[i][g] = prod_axis 1/2 (1 + s_i s_g sqrt 3) -- three butterfly stages (x: lane ^ 1, y: lane ^ 3, z: lane ^ 4 in CHEXA
// order) instead of an 8-term sum of shuffles; the results leave through LDS as full 512-B lines.
template <bool FORCES>
__global__ void __launch_bounds__(256)
k_recover(int64_t n_elem, const double *__restrict__ xyz, const double *__restrict__ disp, const int32_t *__restrict__ conn,
          const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const double *__restrict__ mat_lamG,
          double *__restrict__ strain, double *__restrict__ stress, long long *bad_elem, long long *g1_elem,
          const int32_t *__restrict__ node_dof, double *__restrict__ elem_forces, double *R) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    const elem_lanes L = elem_lanes_here(n_elem);
    const int g = L.g;
    const int64_t e = L.e;
    double eps[6] = {0, 0, 0, 0, 0, 0}, sig[6] = {0, 0, 0, 0, 0, 0};
    double o[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, det = 0, px = 0, py = 0, pz = 0;
    bool live = false;  // a HEX8_G2 element of the batch
    int type = 0;
    int64_t nd = 0;
    double *rec = lds[L.wv] + L.el * ELEM_REC;
    if (L.valid) {
        type = elem_type[e];
        nd = elem_load_node<true>(rec, L, conn, xyz, disp);
    }
    wave_sync();
    if (L.valid) {
        if (type != STAN_HEX8_G2) {
            if (g == 0) atomicMin(g1_elem, (long long)e);
        } else {
            live = true;
            det = hex8_gp_setup(rec, type, g, o);
            if (det == 0.0) atomicMin(bad_elem, (long long)e);
            hex8_gauss_point(type, g, px, py, pz);
            hex8_strain(o, rec + 24, px, py, pz, eps);
            const int32_t m = elem_mat[e];
            hex8_stress(mat_lamG[2 * m], mat_lamG[2 * m + 1], eps, sig);
        }
    }
    // node i = this lane's index within the element; N[i][k] = prod over the axes of 1/2 (1 + s_i s_k sqrt 3): a when node
    // and Gauss point lie on the same side of the axis, b otherwise (FE_Library.cs:105-116, 285-321 evaluated at
    // xi = +-sqrt 3); the partner across an axis is lane ^ 1 (xi), ^ 3 (eta), ^ 4 (zeta) in the CHEXA order of HEX8_S*
    const int i = g;
    const double ca = 0.5 * (1.0 + 1.7320508075688772935), cb = 0.5 * (1.0 - 1.7320508075688772935);
    double ne[6], ns[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double a = eps[c], b = sig[c];
        a = ca * a + cb * __shfl_xor(a, 1, 64); b = ca * b + cb * __shfl_xor(b, 1, 64);
        a = ca * a + cb * __shfl_xor(a, 3, 64); b = ca * b + cb * __shfl_xor(b, 3, 64);
        a = ca * a + cb * __shfl_xor(a, 4, 64); b = ca * b + cb * __shfl_xor(b, 4, 64);
        ne[c] = a; ns[c] = b;
    }
    if (strain) {
        // six 512-B lines per array and wave, non-temporal; each staging waits until no lane reads the wave's LDS any more
        wave_sync();
        elem_store_staged<6, true>(lds[L.wv], L, n_elem, ne, strain);
        wave_sync();
        elem_store_staged<6, true>(lds[L.wv], L, n_elem, ns, stress);
    }
    if (FORCES) {
        // lane g: B_g^T ns * det J_g * w (w = 1 for HEX8_G2)
        double mine[3];
        elem_bt_sum(o, live, g, px, py, pz, ns, live ? det : 0.0, mine);
        if (live) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (elem_forces) elem_forces[e * 24 + 3 * i + c] = mine[c];
                if (R) unsafeAtomicAdd(&R[node_dof[3 * nd + c]], mine[c]);
            }
        }
    }
}

}  // namespace

int lamG_buf::alloc(dev_scope &tmp, int32_t n_mat, const double *mat_E_nu) {
    host.resize(2 * (size_t)n_mat);
    for (int m = 0; m < n_mat; m++) stan_lame(mat_E_nu[2 * m], mat_E_nu[2 * m + 1], &host[2 * m], &host[2 * m + 1]);
    return tmp.alloc(&d, host.size());
}

int stan_recover_device(stan_ctx *ctx, const stan_mesh &d, double *d_strain, double *d_stress, double *d_elem_forces, double *d_R) {
    const bool forces = d_elem_forces || d_R;
    const int64_t n_elem = d.n_elem;
    if (n_elem <= 0) return STAN_OK;
    dev_scope tmp(ctx);
    lamG_buf lamG;
    STANCHK(lamG.alloc(tmp, d.n_mat, d.mat_E_nu));
    const double *d_lamG = lamG.d;
    hipStream_t st = ctx->stream;
    long long init[2] = {0x7fffffffffffffffLL, 0x7fffffffffffffffLL};
    hipError_t e1 = lamG.upload(st);
    hipError_t e2 = hipMemcpyAsync(ctx->d_status + SS_BAD_ELEM, init, 16, hipMemcpyHostToDevice, st);
    const dim3 grid((unsigned)((n_elem + 31) / 32)), block(256);   // 8 lanes per element, 8 elements per wave
    if (forces)
        hipLaunchKernelGGL(k_recover<true>, grid, block, 0, st, n_elem, d.xyz, d.disp, d.conn, d.elem_mat,
                           d.elem_type, d_lamG, d_strain, d_stress, (long long *)(ctx->d_status + SS_BAD_ELEM),
                           (long long *)(ctx->d_status + SS_AUX), d.node_dof, d_elem_forces, d_R);
    else
        hipLaunchKernelGGL(k_recover<false>, grid, block, 0, st, n_elem, d.xyz, d.disp, d.conn, d.elem_mat,
                           d.elem_type, d_lamG, d_strain, d_stress, (long long *)(ctx->d_status + SS_BAD_ELEM),
                           (long long *)(ctx->d_status + SS_AUX), nullptr, nullptr, nullptr);
    hipError_t e3 = hipGetLastError();
    hipError_t e4 = hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, ctx->d_status + SS_BAD_ELEM, 16, hipMemcpyDeviceToHost, st);
    hipError_t e5 = hipStreamSynchronize(st);
    for (hipError_t e : {e1, e2, e3, e4, e5})
        if (e != hipSuccess) { ctx->err = std::string("recover: ") + hipGetErrorString(e); return STAN_E_HIP; }
    if (ctx->h_status[SS_AUX] != init[0]) {
        ctx->bad_elem = ctx->h_status[SS_AUX];
        ctx->err = "stress recovery: element " + std::to_string(ctx->bad_elem) +
                   " is HEX8_G1 (the reference throws: N has one row, Element.cs:242)";
        return STAN_E_UNSUPPORTED;
    }
    return stan_detj_check(ctx, "");
}
