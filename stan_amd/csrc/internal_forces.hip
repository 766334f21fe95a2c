// internal_forces.hip -- internal forces, support reactions and the equilibrium sums:
//   f_e = sum_g B_g^T (D (B_g u_e)) det J_g w  with B_g, D, Gauss points and weights of K_Initial (Element.cs:118-155,
//   FE_Library.cs:63-131) -- the GAUSS-POINT stress, not the node-extrapolated one of Compute_NodalForces (recovery.hip
//   keeps that quirk: its R is not K u) -- and HEX8_G1 as the assembly takes it (one point, weight 8);
//   f_int[node_dof[3n+c]] = sum over every (element, corner) that names node n, as the K scatter counts them
//   (SolverFunctions.cs:143-173); reaction = f_int on the fixed DOFs; residual = F - f_int on the free ones.
// Nothing here forms K, reads the sparse layout or scales: the result is an independent witness of assembly and solve.
// Three phases, all bit-reproducible (no atomics on doubles):
//   element pass  k_if_elem: 8 lanes per element, one per Gauss point (the layout of elem_pass.h); the 8 Gauss-point terms
//                 of a node's force are added by three butterfly stages, f_e leaves node-major through LDS as full lines;
//   lists         node -> (element, corner), all corners, ascending (stan_incidence_lists, scalars.hip);
//   node gather   k_if_gather: one lane per node adds its list's entries in order, writes f_int and reaction through
//                 node_dof and forms the block's partial sums of stan_equilibrium in a fixed order; one block finishes
//                 them in block order (the pattern of the CG's reductions).
// The arguments are checked ON THE DEVICE before anything is indexed with them (k_if_check), so the host-pointer entry
// and the device-pointer entry share every check.
#include "elem_pass.h"

namespace {

constexpr int NSUM = 11;  // reaction_sum[3], load_sum[3], fint_sum[3], residual^2, load^2
constexpr long long NONE = 0x7fffffffffffffffLL;

// ---- argument checks: status[SS_ERRBITS] |= IF_*, status[SS_AUX] += fixed DOFs; claim[i] (zeroed) counts the nodes that
// name the DOF triple {3i, 3i+1, 3i+2}: a second one is a layout error, so node_dof is a permutation and the gather's lanes
// write distinct entries --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_if_check(int64_t n_nodes, int64_t n_elem, int64_t n_dof, int32_t n_mat, const int32_t *__restrict__ conn,
           const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const int32_t *__restrict__ node_dof,
           const int32_t *__restrict__ red, int32_t *__restrict__ claim, int64_t *status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bits = 0, nfix = 0;
    if (t < n_elem * 8) {
        const int32_t nd = conn[t];
        if (nd < 0 || nd >= n_nodes) bits |= IF_CONN;
        if ((t & 7) == 0) {
            const int64_t e = t >> 3;
            if (elem_mat[e] < 0 || elem_mat[e] >= n_mat) bits |= IF_MAT;
            if (elem_type[e] != STAN_HEX8_G1 && elem_type[e] != STAN_HEX8_G2) bits |= IF_TYPE;
        }
    }
    if (t < n_nodes) {
        const int32_t d0 = node_dof[3 * t], d1 = node_dof[3 * t + 1], d2 = node_dof[3 * t + 2];
        // Node.cs:218-223 SetDOF: DOF = {3*index, 3*index+1, 3*index+2}
        if (d0 < 0 || d0 % 3 != 0 || d1 != d0 + 1 || d2 != d0 + 2 || (int64_t)d0 + 2 >= n_dof) bits |= IF_DOF;
        else if (atomicAdd(&claim[d0 / 3], 1) != 0) bits |= IF_DOF;   // (n_dof = 3 n_nodes: d0 / 3 < n_nodes)
    }
    if (t < n_dof) {   // by DOF, not by node: the count is the length of F whatever node_dof claims
        const int32_t r = red[t];
        if (r == -1) nfix = 1;
        else if (r < 0 || r > t) bits |= IF_RED;
    }
    if (bits) atomicOr((unsigned long long *)&status[SS_ERRBITS], bits);
    if (nfix) atomicAdd((unsigned long long *)&status[SS_AUX], nfix);
}

// face list (the load vector's): element and face id in range, keys strictly ascending.  Reads the lists by position only.
__global__ void __launch_bounds__(256)
k_ld_check_faces(int64_t n_faces, int64_t n_elem, const int32_t *__restrict__ face_elem, const uint8_t *__restrict__ face_id,
                 int64_t *status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int64_t e = face_elem[t], f = face_id[t];
    bool bad = e < 0 || e >= n_elem || f >= 6;
    if (t > 0 && (int64_t)face_elem[t - 1] * 6 + face_id[t - 1] >= e * 6 + f) bad = true;
    if (bad) atomicOr((unsigned long long *)&status[SS_ERRBITS], (unsigned long long)IF_FACE);
}

// ---- element pass: f_e [n_elem * 24], node-major ------------------------------------------------------------------------
// Lane mapping, record load, Gauss point and the staged store are elem_pass.h's.  The strain / stress loop and the B^T sum
// repeat hex8_strain, hex8_stress and elem_bt_sum word for word: with the helpers called here the backend fuses other
// products of these sums into FMAs (equal opcode counts, other operands) and f_e, so f_int, changes in its last bits.
__global__ void __launch_bounds__(256)
k_if_elem(int64_t n_elem, const double *__restrict__ xyz, const double *__restrict__ disp, const int32_t *__restrict__ conn,
          const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const double *__restrict__ mat_lamG,
          double *__restrict__ fe, long long *bad_elem) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    const elem_lanes L = elem_lanes_here(n_elem);
    double *rec = lds[L.wv] + L.el * ELEM_REC;
    int type = STAN_HEX8_G2;
    if (L.valid) {
        type = elem_type[L.e];
        elem_load_node<true>(rec, L, conn, xyz, disp);
    }
    wave_sync();
    double o[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, sig[6] = {0, 0, 0, 0, 0, 0}, px = 0, py = 0, pz = 0, sc = 0;
    if (L.valid) {
        // HEX8_G1: every lane evaluates the one point (location 0); its weight is 8 on lane 0 and 0 on the others
        const double det = hex8_gp_setup(rec, type, L.g, o);
        if (det == 0.0) atomicMin(bad_elem, (long long)L.e);
        hex8_gauss_point(type, L.g, px, py, pz);
        const double *u = rec + 24;
        double eps[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            double gr[3];
            hex8_grad(o, i, px, py, pz, gr);
            // BL0 rows (Element.cs:316-324): xx, yy, zz, xy, yz, xz
            eps[0] += gr[0] * u[3 * i];
            eps[1] += gr[1] * u[3 * i + 1];
            eps[2] += gr[2] * u[3 * i + 2];
            eps[3] += gr[1] * u[3 * i] + gr[0] * u[3 * i + 1];
            eps[4] += gr[2] * u[3 * i + 1] + gr[1] * u[3 * i + 2];
            eps[5] += gr[2] * u[3 * i] + gr[0] * u[3 * i + 2];
        }
        const int32_t m = elem_mat[L.e];
        const double lam = mat_lamG[2 * m], G = mat_lamG[2 * m + 1];
        const double tr = lam * (eps[0] + eps[1] + eps[2]);
        sig[0] = tr + 2 * G * eps[0];
        sig[1] = tr + 2 * G * eps[1];
        sig[2] = tr + 2 * G * eps[2];
        sig[3] = G * eps[3]; sig[4] = G * eps[4]; sig[5] = G * eps[5];
        sc = det == 0.0 ? 0.0 : o[9];   // det J_g * w (a singular point is reported, its term left out)
    }
    // lane g: B_g^T sig_g * det J_g w for node a, then the sum over the 8 lanes of the element; node a's three components
    // end up on lane a
    double mine[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 8; a++) {
        double gr[3] = {0, 0, 0};
        if (sc != 0.0) hex8_grad(o, a, px, py, pz, gr);
        double f[3];
        f[0] = (gr[0] * sig[0] + gr[1] * sig[3] + gr[2] * sig[5]) * sc;
        f[1] = (gr[1] * sig[1] + gr[0] * sig[3] + gr[2] * sig[4]) * sc;
        f[2] = (gr[2] * sig[2] + gr[1] * sig[4] + gr[0] * sig[5]) * sc;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = elem_sum(f[c]);
            if (a == L.g) mine[c] = v;
        }
    }
    wave_sync();   // every lane is done with the records
    elem_store_staged<3, false>(lds[L.wv], L, n_elem, mine, fe);   // three 512-B lines per wave
}

// ---- node gather + the block's partial sums ----------------------------------------------------------------------------
struct eq_acc {
    double s[NSUM];
    double mx;        // max |F - f_int| over free DOFs (-1: none)
    long long dof;    // where (lowest index on a tie)
};
__device__ __forceinline__ void acc_max(double &mx, long long &dof, double omx, long long odof) {
    if (omx > mx || (omx == mx && odof < dof)) { mx = omx; dof = odof; }
}
// the block's 256 lanes on thread 0: the sums by block_sums; the maximum and its lowest DOF (whatever the order) by a
// butterfly of their own, the waves' results published by the barrier inside block_sums
struct eq_shared {
    double s[4][NSUM + 1];   // a wave's sums, then its maximum
    long long dof[4];
};
__device__ __forceinline__ void eq_block_reduce(eq_acc &a, eq_shared &sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double omx = __shfl_xor(a.mx, off, 64);
        const long long odof = __shfl_xor(a.dof, off, 64);
        acc_max(a.mx, a.dof, omx, odof);
    }
    if ((threadIdx.x & 63) == 0) { sh.s[threadIdx.x >> 6][NSUM] = a.mx; sh.dof[threadIdx.x >> 6] = a.dof; }
    block_sums(a.s, sh.s);
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) acc_max(a.mx, a.dof, sh.s[w][NSUM], sh.dof[w]);
}

template <bool EQ>
__global__ void __launch_bounds__(256)
k_if_gather(int64_t n_nodes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list, const double *__restrict__ fe,
            const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red, const double *__restrict__ F, int64_t n_red,
            double *__restrict__ f_int, double *__restrict__ reaction, double *__restrict__ partial, long long *__restrict__ partial_dof) {
    __shared__ eq_shared sh;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    eq_acc a;
#pragma unroll
    for (int k = 0; k < NSUM; k++) a.s[k] = 0.0;
    a.mx = -1.0; a.dof = NONE;
    if (n < n_nodes) {
        double f[3];
        node_gather(ptr, list, fe, n, f);
        const int64_t d0 = node_dof[3 * n];   // {d0, d0 + 1, d0 + 2}, no other node's (k_if_check)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int64_t d = d0 + c;
            const int32_t r = red[d];
            const bool fixed = r == -1;
            if (f_int) f_int[d] = f[c];
            if (reaction) reaction[d] = fixed ? f[c] : 0.0;
            if (EQ) {
                a.s[6 + c] = f[c];
                if (fixed) a.s[c] = f[c];
                else {
                    const int64_t j = d - r;
                    const double load = F && j < n_red ? F[j] : 0.0;
                    const double res = load - f[c];
                    a.s[3 + c] = load;
                    a.s[9] += res * res;
                    a.s[10] += load * load;
                    acc_max(a.mx, a.dof, fabs(res), (long long)d);
                }
            }
        }
    }
    if (EQ) {
        eq_block_reduce(a, sh);
        if (threadIdx.x == 0) {
            for (int k = 0; k < NSUM; k++) partial[(int64_t)blockIdx.x * (NSUM + 1) + k] = a.s[k];
            partial[(int64_t)blockIdx.x * (NSUM + 1) + NSUM] = a.mx;
            partial_dof[blockIdx.x] = a.dof;
        }
    }
}

// one block: thread t adds the partials of blocks t, t + 256, ... in ascending order, then the block's fixed order
__global__ void __launch_bounds__(256)
k_if_finish(int64_t n_blocks, const double *__restrict__ partial, const long long *__restrict__ partial_dof, double *out, long long *out_dof) {
    __shared__ eq_shared sh;
    eq_acc a;
#pragma unroll
    for (int k = 0; k < NSUM; k++) a.s[k] = 0.0;
    a.mx = -1.0; a.dof = NONE;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) {
#pragma unroll
        for (int k = 0; k < NSUM; k++) a.s[k] += partial[b * (NSUM + 1) + k];
        acc_max(a.mx, a.dof, partial[b * (NSUM + 1) + NSUM], partial_dof[b]);
    }
    eq_block_reduce(a, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k < NSUM; k++) out[k] = a.s[k];
        out[NSUM] = a.mx;
        *out_dof = a.dof;
    }
}

}  // namespace

int stan_elem_args_check(stan_ctx *ctx, dev_scope &tmp, const char *who, const stan_mesh &d, int64_t n_faces,
                         const int32_t *d_face_elem, const uint8_t *d_face_id, int64_t *n_fixed) {
    auto bad = [&](const char *why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    hipStream_t st = ctx->stream;
    int64_t *status = ctx->d_status;
    const long long init[3] = {0, NONE, 0};
    HIPCHK(ctx, hipMemcpyAsync(status + SS_ERRBITS, &init[0], 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(status + SS_BAD_ELEM, &init[1], 16, hipMemcpyHostToDevice, st));   // SS_BAD_ELEM, SS_AUX
    int32_t *d_claim;
    STANCHK(tmp.alloc(&d_claim, (size_t)d.n_nodes));
    HIPCHK(ctx, hipMemsetAsync(d_claim, 0, (size_t)d.n_nodes * 4, st));
    const int64_t n_chk = d.n_elem * 8 > d.n_dof ? d.n_elem * 8 : d.n_dof;   // (n_dof = 3 n_nodes)
    hipLaunchKernelGGL(k_if_check, dim3(nblk(n_chk, 256)), dim3(256), 0, st, d.n_nodes, d.n_elem, d.n_dof, d.n_mat, d.conn, d.elem_mat,
                       d.elem_type, d.node_dof, d.red, d_claim, status);
    if (n_faces > 0)
        hipLaunchKernelGGL(k_ld_check_faces, dim3(nblk(n_faces, 256)), dim3(256), 0, st, n_faces, d.n_elem, d_face_elem, d_face_id, status);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_ERRBITS, status + SS_ERRBITS, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, status + SS_AUX, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int64_t bits = ctx->h_status[SS_ERRBITS];
    *n_fixed = ctx->h_status[SS_AUX];
    if (bits & IF_DOF) return bad("Node.DOF is not {3i,3i+1,3i+2} with 3i < n_dof, or two nodes share one (Node.cs:218-223)", STAN_E_DOF_LAYOUT);
    if (bits & IF_CONN) return bad("node index out of range", STAN_E_ARG);
    if (bits & IF_MAT) return bad("elem_mat out of range", STAN_E_ARG);
    if (bits & IF_TYPE) return bad("element type is neither HEX8_G1 nor HEX8_G2", STAN_E_ARG);
    if (bits & IF_RED) return bad("ndof_reduction entry outside -1 / [0, i]", STAN_E_ARG);
    if (bits & IF_FACE) return bad("face list: element or face id out of range, or face_elem * 6 + face_id not strictly ascending", STAN_E_ARG);
    return STAN_OK;
}

int stan_elem_limits_check(stan_ctx *ctx, const char *who, const stan_mesh &d) {
    auto bad = [&](const char *why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    if (d.n_nodes <= 0 || d.n_elem < 0 || d.n_mat <= 0 || d.n_dof != d.n_nodes * 3) return bad("n_dof must be 3 n_nodes > 0, n_mat > 0", STAN_E_ARG);
    if (d.n_elem >= (int64_t)1 << 28) return bad("more than 2^28 elements", STAN_E_ARG);
    if (d.n_dof > 0x7fffffffLL) return bad("more than 2^31 DOFs", STAN_E_ARG);
    return STAN_OK;
}

int stan_internal_forces_device(stan_ctx *ctx, const stan_mesh &d, const double *d_F, double *d_fint, double *d_reaction,
                                stan_equilibrium *eq) {
    const char *who = "internal_forces_hex8";
    const int64_t n_nodes = d.n_nodes, n_elem = d.n_elem, n_dof = d.n_dof, n_mat = d.n_mat;
    STANCHK(stan_elem_limits_check(ctx, who, d));
    hipStream_t st = ctx->stream;
    ctx->prof.forces_elem_ms = ctx->prof.forces_list_ms = ctx->prof.forces_gather_ms = 0;
    // ---- the checks, before anything is indexed with the caller's integers
    int64_t *status = ctx->d_status;
    dev_scope tmp(ctx);
    int64_t n_fixed;
    STANCHK(stan_elem_args_check(ctx, tmp, who, d, 0, nullptr, nullptr, &n_fixed));
    const int64_t n_red = n_dof - n_fixed;

    phase_timer pt(ctx, 4);   // element pass | lists | gather + reductions
    lamG_buf lamG;
    double *d_fe, *d_partial = nullptr, *d_out = nullptr;
    long long *d_partial_dof = nullptr, *d_out_dof = nullptr;
    const int64_t n_blocks = nblk(n_nodes, 256);
    STANCHK(lamG.alloc(tmp, n_mat, d.mat_E_nu));
    STANCHK(tmp.alloc(&d_fe, (size_t)(n_elem > 0 ? n_elem : 1) * 24));
    if (eq) {
        STANCHK(tmp.alloc(&d_partial, (size_t)n_blocks * (NSUM + 1)));
        STANCHK(tmp.alloc(&d_partial_dof, (size_t)n_blocks));
        STANCHK(tmp.alloc(&d_out, (size_t)NSUM + 1));
        STANCHK(tmp.alloc(&d_out_dof, (size_t)1));
    }
    HIPCHK(ctx, lamG.upload(st));
    STANCHK(pt.mark(0));
    if (n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_if_elem, dim3(nblk(n_elem, 32)), dim3(256), 0, st, n_elem, d.xyz, d.disp, d.conn, d.elem_mat, d.elem_type,
                           lamG.d, d_fe, (long long *)(status + SS_BAD_ELEM));
    STANCHK(pt.mark(1));
    int64_t *d_ptr;
    int32_t *d_list;
    STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d.conn, true, &d_ptr, &d_list));
    STANCHK(pt.mark(2));
    if (eq) {
        hipLaunchKernelGGL(k_if_gather<true>, dim3((unsigned)n_blocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d.node_dof, d.red,
                           d_F, n_red, d_fint, d_reaction, d_partial, d_partial_dof);
        hipLaunchKernelGGL(k_if_finish, dim3(1), dim3(256), 0, st, n_blocks, d_partial, d_partial_dof, d_out, d_out_dof);
    } else {
        hipLaunchKernelGGL(k_if_gather<false>, dim3((unsigned)n_blocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d.node_dof, d.red,
                           d_F, n_red, d_fint, d_reaction, nullptr, nullptr);
    }
    STANCHK(pt.mark(3));
    HIPCHK(ctx, hipGetLastError());
    double out[NSUM + 1];
    long long out_dof = NONE;
    if (eq) {
        HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&out_dof, d_out_dof, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, status + SS_BAD_ELEM, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    STANCHK(pt.read(0, 1, &ctx->prof.forces_elem_ms));
    STANCHK(pt.read(1, 2, &ctx->prof.forces_list_ms));
    STANCHK(pt.read(2, 3, &ctx->prof.forces_gather_ms));
    STANCHK(stan_detj_check(ctx, " (internal forces)"));
    if (eq) {
        for (int c = 0; c < 3; c++) { eq->reaction_sum[c] = out[c]; eq->load_sum[c] = out[3 + c]; eq->fint_sum[c] = out[6 + c]; }
        eq->residual_norm2 = sqrt(out[9]);
        eq->load_norm2 = sqrt(out[10]);
        eq->residual_max = out[NSUM] < 0 ? 0.0 : out[NSUM];
        eq->residual_max_dof = out[NSUM] < 0 ? -1 : (int64_t)out_dof;
        eq->n_fixed = n_fixed;
    }
    return STAN_OK;
}
