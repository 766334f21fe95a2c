// loads.hip -- the load vector of distributed loads and prescribed displacements:
//   body force   f_a = b_m sum_{2x2x2} N_a(q) det J(q)            b_m a force per unit volume of material m; the 2x2x2 rule for
//                                                                 HEX8_G1 elements too (exact: degree <= 3 per variable)
//   pressure     f_a = -p sum_{2x2} N_a(q) n dA(q)                n dA = s (x_beta x x_gamma) on face (axis, s), (beta, gamma)
//                                                                 the cyclic successors of the axis; unit weights, +-1/sqrt 3
//   prescribed   F_solve = F - f_int(u0)|free                     u0 used at the fixed DOFs only (stan_internal_forces_device)
// No J^-1 is formed for the first two: det J == 0 is no error there.  No counterpart in the reference.
// The thermal load and the thermal stress of section 3.9 are at the end of the kernels: one more element pass (k_th_elem) in
// front of the same gather, and one pass over the recovered stress (k_th_stress).
// The lumped mass of section 3.10 is the body term with b = (rho, 0, 0): k_ld_elem as it stands, and a gather of its own
// (k_ms_gather) that keeps component 0 of node_gather's sum -- the bits of load_full at the node's first DOF.
// Faces in CHEXA order:  0 xi=-1 {0,3,4,7}  1 xi=+1 {1,2,5,6}  2 eta=-1 {0,1,4,5}  3 eta=+1 {2,3,6,7}  4 zeta=-1 {0,1,2,3}
// 5 zeta=+1 {4,5,6,7}; the face list is sorted by face_elem * 6 + face_id, strictly.
// Phases, all bit-reproducible (no atomics on doubles):
//   element pass  k_ld_elem: the layout of elem_pass.h (8 lanes per element, lane g loads node g only, coordinates alone);
//                 body term first (lane g = Gauss point g, three butterfly stages), then the element's listed faces
//                 in ascending face id (lanes 0..3 one face point each, lanes 4..7 add zero to the same butterfly); f_e leaves
//                 node-major through LDS as full lines; a wave without any loaded element stores zeros and nothing else;
//   lists         node -> (element, corner), all corners, ascending (stan_incidence_lists);
//   node gather   k_ld_gather: one lane per node adds its list's entries in order and writes load_full, F, F_solve through
//                 node_dof / the reduction map, with the block's partial sums; k_ld_finish adds the partials in block order.
#include "elem_pass.h"

namespace {

constexpr int NGS = 6;     // gather sums: load_sum[3], free_sum[3]
constexpr int NES = 2;     // element sums: volume, area
constexpr double GL = 0.57735026918962576451;   // sqrt(1/3)

// (the face list's check, k_ld_check_faces, sits with k_if_check in internal_forces.hip: stan_elem_args_check runs both)

// ---- element pass: f_e [n_elem * 24], node-major; partial [gridDim.x * 2] = the block's volume and area ------------------
__global__ void __launch_bounds__(256)
k_ld_elem(int64_t n_elem, const double *__restrict__ xyz, const int32_t *__restrict__ conn, const int32_t *__restrict__ elem_mat,
          const double *__restrict__ mat_body, int64_t n_faces, const int32_t *__restrict__ face_elem,
          const uint8_t *__restrict__ face_id, const double *__restrict__ face_p, double *__restrict__ fe,
          double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    __shared__ double sh[4][NES];
    const elem_lanes L = elem_lanes_here(n_elem);
    const int lane = L.lane, g = L.g;
    const int64_t e = L.e;
    const bool valid = L.valid;
    double b[3] = {0, 0, 0};
    int64_t k0 = 0;          // first listed face of this element
    unsigned fmask = 0;      // bit f: face f of this element is listed
    if (valid) {
        if (mat_body) {
            const int32_t m = elem_mat[e];
            b[0] = mat_body[3 * m]; b[1] = mat_body[3 * m + 1]; b[2] = mat_body[3 * m + 2];
        }
        if (n_faces > 0 && g == 0) {   // one lower-bound search per element for key e * 6 in the sorted keys (its lane 0)
            int64_t lo = 0, hi = n_faces;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if ((int64_t)face_elem[mid] < e) lo = mid + 1; else hi = mid;
            }
            k0 = lo;
            for (int64_t k = lo; k < n_faces && k < lo + 6 && (int64_t)face_elem[k] == e; k++) fmask |= 1u << face_id[k];
        }
    }
    if (n_faces > 0) {   // lane 0 of the element hands its result to the other seven (all lanes active here)
        k0 = __shfl(k0, lane & ~7, 64);
        fmask = __shfl(fmask, lane & ~7, 64);
    }
    const bool has_body = b[0] != 0.0 || b[1] != 0.0 || b[2] != 0.0;
    double mine[3] = {0, 0, 0}, acc[NES] = {0, 0};
    if (__any(has_body || fmask != 0)) {   // wave-uniform: a wave without loads stores zeros and does nothing else
        double *rec = lds[L.wv] + L.el * ELEM_REC;
        if (valid) elem_load_node<false>(rec, L, conn, xyz, nullptr);
        wave_sync();
        if (__any(has_body)) {
            // lane g: Gauss point g of the 2x2x2 rule, whatever the element's type
            double w = 0.0;
            const double px = hex8_sign(HEX8_SX, g) * GL, py = hex8_sign(HEX8_SY, g) * GL, pz = hex8_sign(HEX8_SZ, g) * GL;
            if (valid && has_body) {
                double J[9];
                hex8_jacobian(rec, px, py, pz, J);
                w = hex8_det3(J);
                acc[0] = w;
            }
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const double v = elem_sum(hex8_shape(a, px, py, pz) * w);   // sum_q N_a(q) det J(q)
                if (a == g) { mine[0] = b[0] * v; mine[1] = b[1] * v; mine[2] = b[2] * v; }
            }
        }
        for (int f = 0; f < 6; f++) {
            const bool has = (fmask >> f) & 1u;
            if (!__any(has)) continue;   // wave-uniform
            // lanes 0..3 of the element: face point (bit 0 -> beta, bit 1 -> gamma); lanes 4..7 add zero
            const int axis = f >> 1;
            const double s = (f & 1) ? 1.0 : -1.0;
            const double tb = (g & 1) ? GL : -GL, tg = (g & 2) ? GL : -GL;
            const double px = axis == 0 ? s : (axis == 1 ? tg : tb);   // xi:   axis | gamma of eta  | beta of zeta
            const double py = axis == 1 ? s : (axis == 2 ? tg : tb);   // eta:  axis | gamma of zeta | beta of xi
            const double pz = axis == 2 ? s : (axis == 0 ? tg : tb);   // zeta: axis | gamma of xi   | beta of eta
            double n[3] = {0, 0, 0}, p = 0.0;
            if (valid && has && g < 4) {
                double J[9];
                hex8_jacobian(rec, px, py, pz, J);
                // rows beta = axis + 1 and gamma = axis + 2 (mod 3) of J, picked by selects (no runtime-indexed array)
                const double bx = axis == 0 ? J[3] : (axis == 1 ? J[6] : J[0]), cx = axis == 0 ? J[6] : (axis == 1 ? J[0] : J[3]);
                const double by = axis == 0 ? J[4] : (axis == 1 ? J[7] : J[1]), cy = axis == 0 ? J[7] : (axis == 1 ? J[1] : J[4]);
                const double bz = axis == 0 ? J[5] : (axis == 1 ? J[8] : J[2]), cz = axis == 0 ? J[8] : (axis == 1 ? J[2] : J[5]);
                n[0] = s * (by * cz - bz * cy);
                n[1] = s * (bz * cx - bx * cz);
                n[2] = s * (bx * cy - by * cx);
                acc[1] += sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            }
            if (valid && has) p = face_p[k0 + __popc(fmask & ((1u << f) - 1u))];
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const double Na = hex8_shape(a, px, py, pz);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double v = elem_sum(Na * n[c]);   // sum_q N_a(q) n dA(q)
                    if (a == g) mine[c] -= p * v;
                }
            }
        }
        wave_sync();   // every lane is done with the records
    }
    elem_store_staged<3, false>(lds[L.wv], L, n_elem, mine, fe);   // three 512-B lines per wave
    block_sums(acc, sh);
    if (threadIdx.x == 0) {
        partial[(int64_t)blockIdx.x * NES] = acc[0];
        partial[(int64_t)blockIdx.x * NES + 1] = acc[1];
    }
}

// ---- u0 masked to the fixed DOFs (entries at free DOFs count as 0) ------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ld_mask(int64_t n_dof, const double *__restrict__ disp0, const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red,
          double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;   // 3 * node + component
    if (t < n_dof) out[t] = red[node_dof[t]] == -1 ? disp0[t] : 0.0;
}

// ---- node gather + the block's partial sums ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ld_gather(int64_t n_nodes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list, const double *__restrict__ fe,
            const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red, int64_t n_red, const double *__restrict__ fint0,
            double *F, double *F_solve, double *__restrict__ load_full, double *__restrict__ partial) {
    __shared__ double sh[4][NGS];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[NGS] = {0, 0, 0, 0, 0, 0};
    if (n < n_nodes) {
        double l[3];
        node_gather(ptr, list, fe, n, l);
        const int64_t d0 = node_dof[3 * n];   // {d0, d0 + 1, d0 + 2}, no other node's (k_if_check)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int64_t d = d0 + c;
            const int32_t r = red[d];
            if (load_full) load_full[d] = l[c];
            s[c] = l[c];
            if (r == -1) continue;
            s[3 + c] = l[c];
            const int64_t j = d - r;
            if (j >= n_red) continue;   // (a map that is not the count of fixed DOFs before d)
            double v = l[c];
            if (F) { v = F[j] + l[c]; F[j] = v; }
            if (F_solve) F_solve[j] = fint0 ? v - fint0[d] : v;
        }
    }
    block_sums(s, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < NGS; k++) partial[(int64_t)blockIdx.x * NGS + k] = s[k];
}

// one block: thread t adds the partials of blocks t, t + 256, ... in ascending order, then the block's fixed order
__global__ void __launch_bounds__(256)
k_ld_finish(int64_t n_gblocks, const double *__restrict__ gpartial, int64_t n_eblocks, const double *__restrict__ epartial,
            double *out) {
    __shared__ double sh[4][NGS + NES];
    double a[NGS + NES];
#pragma unroll
    for (int k = 0; k < NGS + NES; k++) a[k] = 0.0;
    for (int64_t b = threadIdx.x; b < n_gblocks; b += 256)
#pragma unroll
        for (int k = 0; k < NGS; k++) a[k] += gpartial[b * NGS + k];
    for (int64_t b = threadIdx.x; b < n_eblocks; b += 256)
#pragma unroll
        for (int k = 0; k < NES; k++) a[NGS + k] += epartial[b * NES + k];
    block_sums(a, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < NGS + NES; k++) out[k] = a[k];
}

// ---- thermal loads ------------------------------------------------------------------------------
//   f_a = sum_g B_a(q_g)^T (beta_m dT(q_g) (1,1,1,0,0,0)) det J_g w,  dT(q) = sum_a N_a(q) dT_a,  beta_m = E alpha / (1 - 2 nu)
// at the element's own STIFFNESS rule (HEX8_G1: one point, weight 8), unlike the body force above: with it K u = f_th holds
// term by term for u = alpha dT x.  The element pass is k_th_elem; the node gather and the finishing block are k_ld_gather and
// k_ld_finish as they stand (the element sums are the heated volume and the integral of dT).
// mat_beta [n_mat][2] = {beta, alpha}: an element whose alpha is 0 stores zeros, is not looked at and raises no STAN_E_DETJ.
// Launch bound 4 waves per SIMD: without it the backend hoists all eight gradients (130 VGPRs, 3 waves); with it 70 VGPRs,
// 7 waves, no scratch -- the pass waits on its node gathers, so the waves are worth more than the hoisting.
__global__ void __launch_bounds__(256, 4)
k_th_elem(int64_t n_elem, const double *__restrict__ xyz, const double *__restrict__ dT, const int32_t *__restrict__ conn,
          const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const double *__restrict__ mat_beta,
          double *__restrict__ fe, double *__restrict__ partial, long long *bad_elem) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    __shared__ double sh[4][NES];
    const elem_lanes L = elem_lanes_here(n_elem);
    const int g = L.g;
    int type = STAN_HEX8_G2;
    double beta = 0.0;
    bool hot = false;   // a valid element whose material expands
    if (L.valid) {
        const int32_t m = elem_mat[L.e];
        type = elem_type[L.e];
        beta = mat_beta[2 * m];
        hot = mat_beta[2 * m + 1] != 0.0;
    }
    double mine[3] = {0, 0, 0}, acc[NES] = {0, 0};
    if (__any(hot)) {   // wave-uniform: a wave without a heated element stores zeros and does nothing else
        double *rec = lds[L.wv] + L.el * ELEM_REC;
        if (L.valid) {   // lane g loads node g only: its coordinates, and its dT into the record's displacement slot
            const int64_t nd = elem_load_node<false>(rec, L, conn, xyz, nullptr);
            rec[24 + g] = dT[nd];
        }
        wave_sync();
        double o[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, px = 0, py = 0, pz = 0, s = 0, sc = 0;
        if (hot) {
            // HEX8_G1: every lane evaluates the one point (location 0); its weight is 8 on lane 0 and 0 on the others
            const double det = hex8_gp_setup(rec, type, g, o);
            if (det == 0.0) atomicMin(bad_elem, (long long)L.e);
            hex8_gauss_point(type, g, px, py, pz);
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < 8; a++) t += hex8_shape(a, px, py, pz) * rec[24 + a];   // dT(q)
            sc = det == 0.0 ? 0.0 : o[9];   // det J_g * w (a singular point is reported, its term left out)
            s = beta * t;
            acc[0] = sc;
            acc[1] = t * sc;
        }
        // lane g: B_g^T (s, s, s, 0, 0, 0) * det J_g w for node a = grad N_a * s * sc, then the sum over the 8 lanes of the
        // element; node a's three components end up on lane a.  (elem_bt_sum with the three zero shear terms left out)
#pragma unroll
        for (int a = 0; a < 8; a++) {
            double gr[3] = {0, 0, 0};
            if (sc != 0.0) hex8_grad(o, a, px, py, pz, gr);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double v = elem_sum((gr[c] * s) * sc);
                if (a == g) mine[c] = v;
            }
        }
        wave_sync();   // every lane is done with the records
    }
    elem_store_staged<3, false>(lds[L.wv], L, n_elem, mine, fe);   // three 512-B lines per wave
    block_sums(acc, sh);
    if (threadIdx.x == 0) {
        partial[(int64_t)blockIdx.x * NES] = acc[0];
        partial[(int64_t)blockIdx.x * NES + 1] = acc[1];
    }
}

// ---- thermal stress: sigma[e][i][c] -= beta_m dT[conn[e][i]] for c = xx, yy, zz, one fused multiply-add (one rounding) --------
// One lane per entry of [n_elem][8][6]: the whole array is read and written back as full lines; the shear entries return as
// they came.
__global__ void __launch_bounds__(256)
k_th_stress(int64_t n_entries, const double *__restrict__ dT, const int32_t *__restrict__ conn, const int32_t *__restrict__ elem_mat,
            const double *__restrict__ mat_beta, double *stress) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    double v = stress[t];
    if (t % 6 < 3) v = fma(-mat_beta[2 * elem_mat[t / 48]], dT[conn[t / 6]], v);
    stress[t] = v;
}

// the integers of the thermal stress pass: status[SS_ERRBITS] |= IF_*, status[SS_AUX] = the first HEX8_G1 element
__global__ void __launch_bounds__(256)
k_th_stress_check(int64_t n_nodes, int64_t n_elem, int32_t n_mat, const int32_t *__restrict__ conn, const int32_t *__restrict__ elem_mat,
                  const uint8_t *__restrict__ elem_type, int64_t *status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_elem * 8) return;
    unsigned long long bits = 0;
    if (conn[t] < 0 || conn[t] >= n_nodes) bits |= IF_CONN;
    if ((t & 7) == 0) {
        const int64_t e = t >> 3;
        if (elem_mat[e] < 0 || elem_mat[e] >= n_mat) bits |= IF_MAT;
        if (elem_type[e] == STAN_HEX8_G1) atomicMin((long long *)&status[SS_AUX], (long long)e);
        else if (elem_type[e] != STAN_HEX8_G2) bits |= IF_TYPE;
    }
    if (bits) atomicOr((unsigned long long *)&status[SS_ERRBITS], bits);
}

// ---- lumped mass: the node gather of component 0, checked before anything is stored ---------------
// mass [n_nodes] (a temporary) = node_gather's l[0] with fe from k_ld_elem under mat_body = (rho, 0, 0); partial [gridDim.x][NMS]
// = total | free by direction | fixed by direction; *bad_node = the first node with a free DOF whose mass is not positive.
constexpr int NMS = 7;
__global__ void __launch_bounds__(256)
k_ms_gather(int64_t n_nodes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list, const double *__restrict__ fe,
            const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red, double *__restrict__ mass,
            double *__restrict__ partial, long long *bad_node) {
    __shared__ double sh[4][NMS];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[NMS] = {0, 0, 0, 0, 0, 0, 0};
    if (n < n_nodes) {
        double l[3];
        node_gather(ptr, list, fe, n, l);
        mass[n] = l[0];
        s[0] = l[0];
        const int64_t d0 = node_dof[3 * n];
        bool any_free = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const bool fixed = red[d0 + c] == -1;
            s[(fixed ? 4 : 1) + c] = l[0];
            any_free |= !fixed;
        }
        if (any_free && !(l[0] > 0.0)) atomicMin(bad_node, (long long)n);
    }
    block_sums(s, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < NMS; k++) partial[(int64_t)blockIdx.x * NMS + k] = s[k];
}

// the stores, behind the check: M at the node's free DOFs in the reduced numbering, mass_node in node order
__global__ void __launch_bounds__(256)
k_ms_store(int64_t n_nodes, const double *__restrict__ mass, const int32_t *__restrict__ node_dof, const int32_t *__restrict__ red,
           int64_t n_red, double *__restrict__ M, double *__restrict__ mass_node) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nodes) return;
    const double m = mass[n];
    if (mass_node) mass_node[n] = m;
    if (!M) return;
    const int64_t d0 = node_dof[3 * n];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t d = d0 + c;
        const int32_t r = red[d];
        if (r != -1 && d - r < n_red) M[d - r] = m;
    }
}

// one block: the mass partials in block order, then the element pass's volume
__global__ void __launch_bounds__(256)
k_ms_finish(int64_t n_gblocks, const double *__restrict__ gpartial, int64_t n_eblocks, const double *__restrict__ epartial, double *out) {
    __shared__ double sh[4][NMS + 1];
    double a[NMS + 1];
#pragma unroll
    for (int k = 0; k < NMS + 1; k++) a[k] = 0.0;
    for (int64_t b = threadIdx.x; b < n_gblocks; b += 256)
#pragma unroll
        for (int k = 0; k < NMS; k++) a[k] += gpartial[b * NMS + k];
    for (int64_t b = threadIdx.x; b < n_eblocks; b += 256) a[NMS] += epartial[b * NES];
    block_sums(a, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < NMS + 1; k++) out[k] = a[k];
}

// {beta, alpha} of every material, beta = E alpha / (1 - 2 nu) in fp64 exactly as written
std::vector<double> thermal_beta(int32_t n_mat, const double *mat_E_nu, const double *mat_alpha) {
    std::vector<double> b(2 * (size_t)n_mat);
    for (int32_t m = 0; m < n_mat; m++) {
        const double E = mat_E_nu[2 * m], nu = mat_E_nu[2 * m + 1], alpha = mat_alpha[m];
        b[2 * m] = E * alpha / (1 - 2 * nu);
        b[2 * m + 1] = alpha;
    }
    return b;
}

}  // namespace

int stan_thermal_load_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_alpha, const double *d_dT, double *d_F,
                             double *d_load_full, stan_thermal_sums *sums) {
    const char *who = "thermal_load_hex8";
    const int64_t n_nodes = d.n_nodes, n_elem = d.n_elem, n_dof = d.n_dof, n_mat = d.n_mat;
    auto bad = [&](const char *why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    STANCHK(stan_elem_limits_check(ctx, who, d));
    if (!d_F && !d_load_full && !sums) return bad("none of F / load_full / sums asked for", STAN_E_ARG);
    hipStream_t st = ctx->stream;
    ctx->prof_thermal_ms[0] = ctx->prof_thermal_ms[1] = ctx->prof_thermal_ms[2] = 0;
    // ---- the checks, before anything is indexed with the caller's integers
    dev_scope tmp(ctx);
    int64_t n_fixed;
    STANCHK(stan_elem_args_check(ctx, tmp, who, d, 0, nullptr, nullptr, &n_fixed));
    const int64_t n_red = n_dof - n_fixed;

    phase_timer pt(ctx, 5);   // element pass | lists | (the det J report) | gather + reductions
    const int64_t n_gblocks = nblk(n_nodes, 256), n_eblocks = nblk(n_elem, 32);
    const std::vector<double> beta = thermal_beta((int32_t)n_mat, d.mat_E_nu, mat_alpha);   // outlives the stream's copy
    double *d_beta, *d_fe, *d_gpartial, *d_epartial, *d_out;
    STANCHK(tmp.alloc(&d_beta, beta.size()));
    STANCHK(tmp.alloc(&d_fe, (size_t)(n_elem > 0 ? n_elem : 1) * 24));
    STANCHK(tmp.alloc(&d_gpartial, (size_t)n_gblocks * NGS));
    STANCHK(tmp.alloc(&d_epartial, (size_t)(n_eblocks > 0 ? n_eblocks : 1) * NES));
    STANCHK(tmp.alloc(&d_out, (size_t)NGS + NES));
    HIPCHK(ctx, hipMemcpyAsync(d_beta, beta.data(), beta.size() * 8, hipMemcpyHostToDevice, st));
    STANCHK(pt.mark(0));
    if (n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_th_elem, dim3((unsigned)n_eblocks), dim3(256), 0, st, n_elem, d.xyz, d_dT, d.conn, d.elem_mat, d.elem_type,
                           d_beta, d_fe, d_epartial, (long long *)(ctx->d_status + SS_BAD_ELEM));
    STANCHK(pt.mark(1));
    int64_t *d_ptr;
    int32_t *d_list;
    STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d.conn, true, &d_ptr, &d_list));
    STANCHK(pt.mark(2));
    // det J == 0 in a heated element: known before the gather stores into the caller's arrays
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, ctx->d_status + SS_BAD_ELEM, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    STANCHK(stan_detj_check(ctx, " (thermal load)"));
    STANCHK(pt.mark(3));
    hipLaunchKernelGGL(k_ld_gather, dim3((unsigned)n_gblocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d.node_dof, d.red, n_red,
                       nullptr, d_F, nullptr, d_load_full, d_gpartial);
    if (sums) hipLaunchKernelGGL(k_ld_finish, dim3(1), dim3(256), 0, st, n_gblocks, d_gpartial, n_eblocks, d_epartial, d_out);
    STANCHK(pt.mark(4));
    HIPCHK(ctx, hipGetLastError());
    double out[NGS + NES];
    if (sums) HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    STANCHK(pt.read(0, 1, &ctx->prof_thermal_ms[0]));
    STANCHK(pt.read(1, 2, &ctx->prof_thermal_ms[1]));
    STANCHK(pt.read(3, 4, &ctx->prof_thermal_ms[2]));
    if (sums) {
        for (int c = 0; c < 3; c++) { sums->load_sum[c] = out[c]; sums->free_sum[c] = out[3 + c]; }
        sums->volume = out[NGS];
        sums->dT_integral = out[NGS + 1];
        sums->n_fixed = n_fixed;
    }
    return STAN_OK;
}

int stan_thermal_stress_device(stan_ctx *ctx, const stan_mesh &d, const double *d_dT, const double *mat_alpha, double *d_stress) {
    const int64_t n_nodes = d.n_nodes, n_elem = d.n_elem;
    const int32_t n_mat = d.n_mat;
    auto bad = [&](const char *why, int rc) { ctx->err = std::string("thermal_stress_hex8: ") + why; return rc; };
    if (n_nodes <= 0 || n_elem < 0 || n_mat <= 0) return bad("n_nodes and n_mat must be positive", STAN_E_ARG);
    if (n_elem >= (int64_t)1 << 28) return bad("more than 2^28 elements", STAN_E_ARG);
    if (n_elem == 0) return STAN_OK;
    hipStream_t st = ctx->stream;
    int64_t *status = ctx->d_status;
    const long long init[3] = {0, 0x7fffffffffffffffLL, 0x7fffffffffffffffLL};
    HIPCHK(ctx, hipMemcpyAsync(status + SS_ERRBITS, &init[0], 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(status + SS_BAD_ELEM, &init[1], 16, hipMemcpyHostToDevice, st));   // SS_BAD_ELEM, SS_AUX
    hipLaunchKernelGGL(k_th_stress_check, dim3(nblk(n_elem * 8, 256)), dim3(256), 0, st, n_nodes, n_elem, n_mat, d.conn, d.elem_mat,
                       d.elem_type, status);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_ERRBITS, status + SS_ERRBITS, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, status + SS_AUX, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int64_t bits = ctx->h_status[SS_ERRBITS];
    if (bits & IF_CONN) return bad("node index out of range", STAN_E_ARG);
    if (bits & IF_MAT) return bad("elem_mat out of range", STAN_E_ARG);
    if (bits & IF_TYPE) return bad("element type is neither HEX8_G1 nor HEX8_G2", STAN_E_ARG);
    if (ctx->h_status[SS_AUX] != init[2]) {
        ctx->bad_elem = ctx->h_status[SS_AUX];
        return bad(("element " + std::to_string(ctx->bad_elem) + " is HEX8_G1 (no nodal stress: the recovery refuses it)").c_str(), STAN_E_UNSUPPORTED);
    }
    dev_scope tmp(ctx);
    const std::vector<double> beta = thermal_beta(n_mat, d.mat_E_nu, mat_alpha);   // outlives the stream's copy
    double *d_beta;
    STANCHK(tmp.alloc(&d_beta, beta.size()));
    HIPCHK(ctx, hipMemcpyAsync(d_beta, beta.data(), beta.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_th_stress, dim3(nblk(n_elem * 48, 256)), dim3(256), 0, st, n_elem * 48, d_dT, d.conn, d.elem_mat, d_beta, d_stress);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    return STAN_OK;
}

int stan_load_vector_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_body, int64_t n_faces, const int32_t *d_face_elem,
                            const uint8_t *d_face_id, const double *d_face_pressure, const double *d_disp0, double *d_F,
                            double *d_F_solve, double *d_load_full, stan_load_sums *sums) {
    const char *who = "load_vector_hex8";
    const int64_t n_nodes = d.n_nodes, n_elem = d.n_elem, n_dof = d.n_dof, n_mat = d.n_mat;
    auto bad = [&](const char *why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    STANCHK(stan_elem_limits_check(ctx, who, d));
    if (n_faces < 0 || n_faces > n_elem * 6) return bad("n_faces outside [0, 6 n_elem]", STAN_E_ARG);
    if (!mat_body && n_faces == 0 && !d_disp0) return bad("no body force, no face and no prescribed displacement", STAN_E_ARG);
    if (!d_F && !d_F_solve && !d_load_full && !sums) return bad("none of F / F_solve / load_full / sums asked for", STAN_E_ARG);
    if (d_disp0 && !d_F_solve) return bad("disp0 without F_solve", STAN_E_ARG);
    hipStream_t st = ctx->stream;
    ctx->prof_loads_ms[0] = ctx->prof_loads_ms[1] = ctx->prof_loads_ms[2] = 0;
    // ---- the checks, before anything is indexed with the caller's integers
    dev_scope tmp(ctx);
    int64_t n_fixed;
    STANCHK(stan_elem_args_check(ctx, tmp, who, d, n_faces, d_face_elem, d_face_id, &n_fixed));
    const int64_t n_red = n_dof - n_fixed;

    // ---- prescribed displacements first: f_int(u0 at the fixed DOFs), an error of it leaves every output untouched
    double *d_fint0 = nullptr;
    if (d_disp0) {
        double *d_u0;
        STANCHK(tmp.alloc(&d_u0, (size_t)n_dof));
        STANCHK(tmp.alloc(&d_fint0, (size_t)n_dof));
        hipLaunchKernelGGL(k_ld_mask, dim3(nblk(n_dof, 256)), dim3(256), 0, st, n_dof, d_disp0, d.node_dof, d.red, d_u0);
        HIPCHK(ctx, hipGetLastError());
        stan_mesh at_u0 = d;
        at_u0.disp = d_u0;
        STANCHK(stan_internal_forces_device(ctx, at_u0, nullptr, d_fint0, nullptr, nullptr));
    }

    phase_timer pt(ctx, 4);   // element pass | lists | gather + reductions
    const int64_t n_gblocks = nblk(n_nodes, 256), n_eblocks = nblk(n_elem, 32);
    double *d_body = nullptr, *d_fe, *d_gpartial, *d_epartial, *d_out;
    STANCHK(tmp.alloc(&d_fe, (size_t)(n_elem > 0 ? n_elem : 1) * 24));
    STANCHK(tmp.alloc(&d_gpartial, (size_t)n_gblocks * NGS));
    STANCHK(tmp.alloc(&d_epartial, (size_t)(n_eblocks > 0 ? n_eblocks : 1) * NES));
    STANCHK(tmp.alloc(&d_out, (size_t)NGS + NES));
    if (mat_body) {
        STANCHK(tmp.alloc(&d_body, (size_t)n_mat * 3));
        HIPCHK(ctx, hipMemcpyAsync(d_body, mat_body, (size_t)n_mat * 24, hipMemcpyHostToDevice, st));
    }
    STANCHK(pt.mark(0));
    if (n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_ld_elem, dim3((unsigned)n_eblocks), dim3(256), 0, st, n_elem, d.xyz, d.conn, d.elem_mat, d_body, n_faces,
                           d_face_elem, d_face_id, d_face_pressure, d_fe, d_epartial);
    STANCHK(pt.mark(1));
    int64_t *d_ptr;
    int32_t *d_list;
    STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d.conn, true, &d_ptr, &d_list));
    STANCHK(pt.mark(2));
    hipLaunchKernelGGL(k_ld_gather, dim3((unsigned)n_gblocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d.node_dof, d.red, n_red,
                       d_fint0, d_F, d_F_solve, d_load_full, d_gpartial);
    if (sums) hipLaunchKernelGGL(k_ld_finish, dim3(1), dim3(256), 0, st, n_gblocks, d_gpartial, n_eblocks, d_epartial, d_out);
    STANCHK(pt.mark(3));
    HIPCHK(ctx, hipGetLastError());
    double out[NGS + NES];
    if (sums) HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    for (int k = 0; k < 3; k++) STANCHK(pt.read(k, k + 1, &ctx->prof_loads_ms[k]));
    if (sums) {
        for (int c = 0; c < 3; c++) { sums->load_sum[c] = out[c]; sums->free_sum[c] = out[3 + c]; }
        sums->volume = out[NGS];
        sums->area = out[NGS + 1];
        sums->n_fixed = n_fixed;
        sums->n_faces = n_faces;
    }
    return STAN_OK;
}

int stan_lumped_mass_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_rho, double *d_M, double *d_mass_node,
                            stan_mass_sums *sums) {
    const char *who = "lumped_mass_hex8";
    const int64_t n_nodes = d.n_nodes, n_elem = d.n_elem, n_dof = d.n_dof, n_mat = d.n_mat;
    auto bad = [&](const std::string &why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    STANCHK(stan_elem_limits_check(ctx, who, d));
    if (!d_M && !d_mass_node && !sums) return bad("none of M / mass_node / sums asked for", STAN_E_ARG);
    std::vector<double> body(3 * (size_t)n_mat, 0.0);   // (rho, 0, 0): the body term's b; outlives the stream's copy
    for (int64_t m = 0; m < n_mat; m++) {
        if (!(mat_rho[m] >= 0.0) || !std::isfinite(mat_rho[m])) return bad("density of material " + std::to_string(m) + " is negative or not finite", STAN_E_ARG);
        body[3 * (size_t)m] = mat_rho[m];
    }
    hipStream_t st = ctx->stream;
    // ---- the checks, before anything is indexed with the caller's integers
    dev_scope tmp(ctx);
    int64_t n_fixed;
    STANCHK(stan_elem_args_check(ctx, tmp, who, d, 0, nullptr, nullptr, &n_fixed));
    const int64_t n_red = n_dof - n_fixed;

    const int64_t n_gblocks = nblk(n_nodes, 256), n_eblocks = nblk(n_elem, 32);
    double *d_body, *d_fe, *d_mass, *d_gpartial, *d_epartial, *d_out;
    STANCHK(tmp.alloc(&d_body, body.size()));
    STANCHK(tmp.alloc(&d_fe, (size_t)(n_elem > 0 ? n_elem : 1) * 24));
    STANCHK(tmp.alloc(&d_mass, (size_t)n_nodes));
    STANCHK(tmp.alloc(&d_gpartial, (size_t)n_gblocks * NMS));
    STANCHK(tmp.alloc(&d_epartial, (size_t)(n_eblocks > 0 ? n_eblocks : 1) * NES));
    STANCHK(tmp.alloc(&d_out, (size_t)NMS + 1));
    HIPCHK(ctx, hipMemcpyAsync(d_body, body.data(), body.size() * 8, hipMemcpyHostToDevice, st));
    const long long none = 0x7fffffffffffffffLL;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_status + SS_AUX, &none, 8, hipMemcpyHostToDevice, st));
    if (n_elem > 0)   // the load vector's element pass, no face
        hipLaunchKernelGGL(k_ld_elem, dim3((unsigned)n_eblocks), dim3(256), 0, st, n_elem, d.xyz, d.conn, d.elem_mat, d_body, (int64_t)0,
                           nullptr, nullptr, nullptr, d_fe, d_epartial);
    int64_t *d_ptr;
    int32_t *d_list;
    STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d.conn, true, &d_ptr, &d_list));
    hipLaunchKernelGGL(k_ms_gather, dim3((unsigned)n_gblocks), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_fe, d.node_dof, d.red, d_mass,
                       d_gpartial, (long long *)(ctx->d_status + SS_AUX));
    // a free DOF without mass: known before anything is stored into the caller's arrays
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, ctx->d_status + SS_AUX, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (ctx->h_status[SS_AUX] != none)
        return bad("node " + std::to_string(ctx->h_status[SS_AUX]) + " has a free DOF and no positive mass", STAN_E_ARG);
    if (d_M || d_mass_node)
        hipLaunchKernelGGL(k_ms_store, dim3((unsigned)n_gblocks), dim3(256), 0, st, n_nodes, d_mass, d.node_dof, d.red, n_red, d_M, d_mass_node);
    if (sums) hipLaunchKernelGGL(k_ms_finish, dim3(1), dim3(256), 0, st, n_gblocks, d_gpartial, n_eblocks, d_epartial, d_out);
    HIPCHK(ctx, hipGetLastError());
    double out[NMS + 1];
    if (sums) HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    if (sums) {
        sums->total_mass = out[0];
        for (int c = 0; c < 3; c++) { sums->free_sum[c] = out[1 + c]; sums->fixed_sum[c] = out[4 + c]; }
        sums->volume = out[NMS];
        sums->n_fixed = n_fixed;
    }
    return STAN_OK;
}
