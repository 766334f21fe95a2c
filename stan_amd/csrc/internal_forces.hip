// internal_forces.hip -- internal forces, support reactions and the equilibrium sums:
//   f_e = sum_g B_g^T (D (B_g u_e)) det J_g w  with B_g, D, Gauss points and weights of K_Initial (Element.cs:118-155,
//   FE_Library.cs:63-131) -- the GAUSS-POINT stress, not the node-extrapolated one of Compute_NodalForces (recovery.hip
//   keeps that quirk: its R is not K u) -- and HEX8_G1 as the assembly takes it (one point, weight 8);
//   f_int[node_dof[3n+c]] = sum over every (element, corner) that names node n, as the K scatter counts them
//   (SolverFunctions.cs:143-173); reaction = f_int on the fixed DOFs; residual = F - f_int on the free ones.
// Nothing here forms K, reads the sparse layout or scales: the result is an independent witness of assembly and solve.
// Three phases, all bit-reproducible (no atomics on doubles):
//   element pass  k_if_elem: 8 lanes per element, one per Gauss point (the layout of k_recover: lane g loads node g only,
//                 the element's record goes round through LDS, 50 doubles apart); the 8 Gauss-point terms of a node's force
//                 are added by three butterfly stages, f_e leaves node-major through LDS as full lines;
//   lists         node -> (element, corner), all corners, ascending (stan_incidence_lists, scalars.hip);
//   node gather   k_if_gather: one lane per node adds its list's entries in order, writes f_int and reaction through
//                 node_dof and forms the block's partial sums of stan_equilibrium in a fixed order; one block finishes
//                 them in block order (the pattern of the CG's reductions).
// The arguments are checked ON THE DEVICE before anything is indexed with them (k_if_check), so the host-pointer entry
// and the device-pointer entry share every check.
#include "internal.h"
#include "hex8_device.h"

namespace {

constexpr int REC = 50;   // doubles per element record in LDS, as k_recover's (48 + 2: the records of a wave start 36 banks apart, 16-B aligned)
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

__device__ __forceinline__ void wave_sync() {   // wave-local exchange through LDS (as in k_recover)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- element pass: f_e [n_elem * 24], node-major ------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_if_elem(int64_t n_elem, const double *__restrict__ xyz, const double *__restrict__ disp, const int32_t *__restrict__ conn,
          const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const double *__restrict__ mat_lamG,
          double *__restrict__ fe, long long *bad_elem) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * REC];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int el = lane >> 3, g = lane & 7;
    const int64_t e0 = ((int64_t)blockIdx.x * 4 + wv) * 8;   // first element of this wave
    const int64_t e = e0 + el;
    const bool valid = e < n_elem;
    double *rec = lds[wv] + el * REC;
    int type = STAN_HEX8_G2;
    if (valid) {
        type = elem_type[e];
        const int64_t nd = conn[e * 8 + g];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            rec[3 * g + c] = xyz[3 * nd + c];
            rec[24 + 3 * g + c] = disp[3 * nd + c];
        }
    }
    wave_sync();
    double o[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, sig[6] = {0, 0, 0, 0, 0, 0}, px = 0, py = 0, pz = 0, sc = 0;
    if (valid) {
        const double *u = rec + 24;   // coordinates [0, 24), displacements [24, 48)
        // HEX8_G1: every lane evaluates the one point (location 0); its weight is 8 on lane 0 and 0 on the others
        const double det = hex8_gp_setup(rec, type, g, o);
        if (det == 0.0) atomicMin(bad_elem, (long long)e);
        const double gl = hex8_gauss_loc(type);
        px = hex8_sign(HEX8_SX, g) * gl; py = hex8_sign(HEX8_SY, g) * gl; pz = hex8_sign(HEX8_SZ, g) * gl;
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
        const int32_t m = elem_mat[e];
        const double lam = mat_lamG[2 * m], G = mat_lamG[2 * m + 1];
        const double tr = lam * (eps[0] + eps[1] + eps[2]);
        sig[0] = tr + 2 * G * eps[0];
        sig[1] = tr + 2 * G * eps[1];
        sig[2] = tr + 2 * G * eps[2];
        sig[3] = G * eps[3]; sig[4] = G * eps[4]; sig[5] = G * eps[5];
        sc = det == 0.0 ? 0.0 : o[9];   // det J_g * w (a singular point is reported, its term left out)
    }
    // lane g: B_g^T sig_g * det J_g w for node a, then the sum over the 8 lanes of the element (three butterfly stages: a
    // fixed order); node a's three components end up on lane a
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
            double v = f[c];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            if (a == g) mine[c] = v;
        }
    }
    // the wave's 8 x 24 values are contiguous in memory: through LDS, out as three 512-B lines
    double *stg = lds[wv];
    wave_sync();   // every lane is done with the records
#pragma unroll
    for (int c = 0; c < 3; c++) stg[lane * 3 + c] = mine[c];
    wave_sync();
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int idx = j * 64 + lane;
        if (e0 + idx / 24 < n_elem) fe[e0 * 24 + idx] = stg[idx];
    }
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
// sums of the block's 256 lanes in a fixed order (six butterfly stages per wave, then the four waves in order) on thread 0
__device__ __forceinline__ void block_sums(eq_acc &a, double (*sh)[NSUM + 1], long long *shd) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NSUM; k++) a.s[k] += __shfl_xor(a.s[k], off, 64);
        const double omx = __shfl_xor(a.mx, off, 64);
        const long long odof = __shfl_xor(a.dof, off, 64);
        acc_max(a.mx, a.dof, omx, odof);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; k++) sh[wv][k] = a.s[k];
        sh[wv][NSUM] = a.mx;
        shd[wv] = a.dof;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) {
#pragma unroll
            for (int k = 0; k < NSUM; k++) a.s[k] += sh[w][k];
            acc_max(a.mx, a.dof, sh[w][NSUM], shd[w]);
        }
}

template <bool EQ>
__global__ void __launch_bounds__(256)
k_if_gather(int64_t n_nodes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list, const double *__restrict__ fe,
            const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red, const double *__restrict__ F, int64_t n_red,
            double *__restrict__ f_int, double *__restrict__ reaction, double *__restrict__ partial, long long *__restrict__ partial_dof) {
    __shared__ double sh[4][NSUM + 1];
    __shared__ long long shd[4];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    eq_acc a;
#pragma unroll
    for (int k = 0; k < NSUM; k++) a.s[k] = 0.0;
    a.mx = -1.0; a.dof = NONE;
    if (n < n_nodes) {
        double f[3] = {0.0, 0.0, 0.0};
        const int64_t k0 = ptr[n], k1 = ptr[n + 1];
        for (int64_t k = k0; k < k1; k++) {
            const int64_t t = list[k];   // element * 8 + corner
            f[0] += fe[3 * t]; f[1] += fe[3 * t + 1]; f[2] += fe[3 * t + 2];
        }
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
        block_sums(a, sh, shd);
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
    __shared__ double sh[4][NSUM + 1];
    __shared__ long long shd[4];
    eq_acc a;
#pragma unroll
    for (int k = 0; k < NSUM; k++) a.s[k] = 0.0;
    a.mx = -1.0; a.dof = NONE;
    for (int64_t b = threadIdx.x; b < n_blocks; b += 256) {
#pragma unroll
        for (int k = 0; k < NSUM; k++) a.s[k] += partial[b * (NSUM + 1) + k];
        acc_max(a.mx, a.dof, partial[b * (NSUM + 1) + NSUM], partial_dof[b]);
    }
    block_sums(a, sh, shd);
    if (threadIdx.x == 0) {
        for (int k = 0; k < NSUM; k++) out[k] = a.s[k];
        out[NSUM] = a.mx;
        *out_dof = a.dof;
    }
}

}  // namespace

void stan_if_check_enqueue(stan_ctx *ctx, int64_t n_nodes, int64_t n_elem, int64_t n_dof, int32_t n_mat, const int32_t *d_conn,
                           const int32_t *d_elem_mat, const uint8_t *d_elem_type, const int32_t *d_node_dof, const int32_t *d_red,
                           int32_t *d_claim) {
    const int64_t n_chk = n_elem * 8 > n_dof ? n_elem * 8 : n_dof;   // (n_dof = 3 n_nodes)
    hipLaunchKernelGGL(k_if_check, dim3(nblk(n_chk, 256)), dim3(256), 0, ctx->stream, n_nodes, n_elem, n_dof, n_mat, d_conn,
                       d_elem_mat, d_elem_type, d_node_dof, d_red, d_claim, ctx->d_status);
}

int stan_internal_forces_device(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const double *d_disp,
                                const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                const int32_t *d_red, const double *d_F, double *d_fint, double *d_reaction,
                                stan_equilibrium *eq) {
    auto bad = [&](const char *why, int rc) { ctx->err = std::string("internal_forces_hex8: ") + why; return rc; };
    if (n_nodes <= 0 || n_elem < 0 || n_mat <= 0 || n_dof != n_nodes * 3) return bad("n_dof must be 3 n_nodes > 0, n_mat > 0", STAN_E_ARG);
    if (n_elem >= (int64_t)1 << 28) return bad("more than 2^28 elements", STAN_E_ARG);
    if (n_dof > 0x7fffffffLL) return bad("more than 2^31 DOFs", STAN_E_ARG);
    hipStream_t st = ctx->stream;
    ctx->prof.forces_elem_ms = ctx->prof.forces_list_ms = ctx->prof.forces_gather_ms = 0;
    // ---- the checks, before anything is indexed with the caller's integers
    int64_t *status = ctx->d_status;
    const long long init[3] = {0, NONE, 0};
    HIPCHK(ctx, hipMemcpyAsync(status + SS_ERRBITS, &init[0], 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(status + SS_BAD_ELEM, &init[1], 16, hipMemcpyHostToDevice, st));   // SS_BAD_ELEM, SS_AUX
    dev_scope tmp(ctx);
    int32_t *d_claim;
    STANCHK(tmp.alloc(&d_claim, (size_t)n_nodes));
    HIPCHK(ctx, hipMemsetAsync(d_claim, 0, (size_t)n_nodes * 4, st));
    stan_if_check_enqueue(ctx, n_nodes, n_elem, n_dof, n_mat, d_conn, d_elem_mat, d_elem_type, d_node_dof, d_red, d_claim);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_ERRBITS, status + SS_ERRBITS, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, status + SS_AUX, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int64_t bits = ctx->h_status[SS_ERRBITS], n_fixed = ctx->h_status[SS_AUX];
    if (bits & IF_DOF) return bad("Node.DOF is not {3i,3i+1,3i+2} with 3i < n_dof, or two nodes share one (Node.cs:218-223)", STAN_E_DOF_LAYOUT);
    if (bits & IF_CONN) return bad("node index out of range", STAN_E_ARG);
    if (bits & IF_MAT) return bad("elem_mat out of range", STAN_E_ARG);
    if (bits & IF_TYPE) return bad("element type is neither HEX8_G1 nor HEX8_G2", STAN_E_ARG);
    if (bits & IF_RED) return bad("ndof_reduction entry outside -1 / [0, i]", STAN_E_ARG);
    const int64_t n_red = n_dof - n_fixed;

    std::vector<double> lamG(2 * (size_t)n_mat);
    for (int m = 0; m < n_mat; m++) stan_lame(mat_E_nu[2 * m], mat_E_nu[2 * m + 1], &lamG[2 * m], &lamG[2 * m + 1]);
    event_bag evs;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // profiling: element pass | lists | gather + reductions
    if (ctx->profiling)
        for (hipEvent_t &e : ev) e = evs.make();
    double *d_lamG, *d_fe, *d_partial = nullptr, *d_out = nullptr;
    long long *d_partial_dof = nullptr, *d_out_dof = nullptr;
    const int64_t n_blocks = nblk(n_nodes, 256);
    STANCHK(tmp.alloc(&d_lamG, lamG.size()));
    STANCHK(tmp.alloc(&d_fe, (size_t)(n_elem > 0 ? n_elem : 1) * 24));
    if (eq) {
        STANCHK(tmp.alloc(&d_partial, (size_t)n_blocks * (NSUM + 1)));
        STANCHK(tmp.alloc(&d_partial_dof, (size_t)n_blocks));
        STANCHK(tmp.alloc(&d_out, (size_t)NSUM + 1));
        STANCHK(tmp.alloc(&d_out_dof, (size_t)1));
    }
    HIPCHK(ctx, hipMemcpyAsync(d_lamG, lamG.data(), lamG.size() * 8, hipMemcpyHostToDevice, st));
    if (ev[0]) HIPCHK(ctx, hipEventRecord(ev[0], st));
    if (n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_if_elem, dim3(nblk(n_elem, 32)), dim3(256), 0, st, n_elem, d_xyz, d_disp, d_conn, d_elem_mat, d_elem_type,
                           d_lamG, d_fe, (long long *)(status + SS_BAD_ELEM));
    if (ev[1]) HIPCHK(ctx, hipEventRecord(ev[1], st));
    int64_t *d_ptr;
    int32_t *d_list;
    STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d_conn, true, &d_ptr, &d_list));
    if (ev[2]) HIPCHK(ctx, hipEventRecord(ev[2], st));
    if (eq) {
        hipLaunchKernelGGL(k_if_gather<true>, dim3((unsigned)n_blocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d_node_dof, d_red,
                           d_F, n_red, d_fint, d_reaction, d_partial, d_partial_dof);
        hipLaunchKernelGGL(k_if_finish, dim3(1), dim3(256), 0, st, n_blocks, d_partial, d_partial_dof, d_out, d_out_dof);
    } else {
        hipLaunchKernelGGL(k_if_gather<false>, dim3((unsigned)n_blocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d_node_dof, d_red,
                           d_F, n_red, d_fint, d_reaction, nullptr, nullptr);
    }
    if (ev[3]) HIPCHK(ctx, hipEventRecord(ev[3], st));
    HIPCHK(ctx, hipGetLastError());
    double out[NSUM + 1];
    long long out_dof = NONE;
    if (eq) {
        HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&out_dof, d_out_dof, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, status + SS_BAD_ELEM, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    if (ctx->profiling) {
        float ms = 0;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1])); ctx->prof.forces_elem_ms = ms;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[1], ev[2])); ctx->prof.forces_list_ms = ms;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[2], ev[3])); ctx->prof.forces_gather_ms = ms;
    }
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
