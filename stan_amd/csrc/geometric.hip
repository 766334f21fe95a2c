// geometric.hip -- the geometric (initial-stress) stiffness K_g(U) of linear buckling:
//   s_e[a][b] = sum_g w_g det J_g (grad N_a)^T Sigma_g grad N_b,  Sigma_g the 3x3 tensor of sigma_g = D (B_g u_e)
// with B_g, D, Gauss points and weights of K_Initial (Element.cs:118-155, FE_Library.cs:63-131) and HEX8_G1 as the
// assembly takes it (one point, weight 8); the element matrix is s_e (x) I_3.  No step of the reference.
// Two phases, both bit-reproducible (no atomics on doubles):
//   element pass  k_kg_elem: 8 lanes per element, one per Gauss point (the layout of elem_pass.h); the 8 Gauss-point terms
//                 of an entry are added by three butterfly stages; the 36 entries of the upper triangle leave per element
//                 through LDS as full lines, [n_elem][36];
//   row gather    k_kg_gather: a wavefront per slice of K's layout, a lane per block row; for every slot of the row the
//                 lane walks the (element, local node a) incidences of the row's node in ascending order and adds
//                 s_e[a][b] for b = 0..7 where conn[e][b] is the slot's column; the sum goes to the three diagonal
//                 components of the block, the essential BCs are applied as k_numeric applies them, and every value of
//                 the array -- padding included -- is stored exactly once.
// stan_hip_kg_hex8_batch runs k_kg_elem itself on the batch (its elements' corners numbered 0 .. 8n - 1).
// The row gather with its maps, its host half and the batch numbering serve every matrix of element scalars s_e (x) I_3: the
// consistent mass of mass.hip is built by stan_elem_scalars_matrix too.
#include "elem_pass.h"

namespace {

constexpr long long NONE = 0x7fffffffffffffffLL;

// ---- element pass: s36 [n_elem][36] --------------------------------------------------------------------------------------
// Lane mapping, record load and Gauss point are elem_pass.h's; strain and stress are hex8_strain / hex8_stress.  Lane g holds
// the 8 gradients of its point (24 doubles) and t_a = Sigma_g grad N_a one node at a time; every index is a compile-time
// constant (no scratch).  Entry i of the triangle stays on lane i % 8 (five registers), so a wave's 8 x 36 values go out
// through its LDS as 4.5 lines of 512 B.
__global__ void __launch_bounds__(256)
k_kg_elem(int64_t n_elem, const double *__restrict__ xyz, const double *__restrict__ disp, const int32_t *__restrict__ conn,
          const int32_t *__restrict__ elem_mat, const uint8_t *__restrict__ elem_type, const double *__restrict__ mat_lamG,
          double *__restrict__ s36, long long *bad_elem) {
    __shared__ __attribute__((aligned(16))) double lds[4][8 * ELEM_REC];
    const elem_lanes L = elem_lanes_here(n_elem);
    double *rec = lds[L.wv] + L.el * ELEM_REC;
    int type = STAN_HEX8_G2;
    if (L.valid) {
        type = elem_type[L.e];
        elem_load_node<true>(rec, L, conn, xyz, disp);
    }
    wave_sync();
    double gr[8][3], sig[6] = {0, 0, 0, 0, 0, 0}, sc = 0;
#pragma unroll
    for (int a = 0; a < 8; a++) gr[a][0] = gr[a][1] = gr[a][2] = 0.0;
    if (L.valid) {
        // HEX8_G1: every lane evaluates the one point (location 0); its weight is 8 on lane 0 and 0 on the others
        double o[10], px, py, pz, eps[6];
        const double det = hex8_gp_setup(rec, type, L.g, o);
        if (det == 0.0) atomicMin(bad_elem, (long long)L.e);
        hex8_gauss_point(type, L.g, px, py, pz);
        hex8_strain(o, rec + 24, px, py, pz, eps);
        const int32_t m = elem_mat[L.e];
        hex8_stress(mat_lamG[2 * m], mat_lamG[2 * m + 1], eps, sig);
        sc = det == 0.0 ? 0.0 : o[9];   // det J_g * w (a singular point is reported, its term left out)
        if (sc != 0.0)
#pragma unroll
            for (int a = 0; a < 8; a++) hex8_grad(o, a, px, py, pz, gr[a]);
    }
    double mine[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 8; a++) {
        // t = Sigma grad N_a * det J w; sig: xx, yy, zz, xy, yz, xz
        double t[3];
        t[0] = (sig[0] * gr[a][0] + sig[3] * gr[a][1] + sig[5] * gr[a][2]) * sc;
        t[1] = (sig[3] * gr[a][0] + sig[1] * gr[a][1] + sig[4] * gr[a][2]) * sc;
        t[2] = (sig[5] * gr[a][0] + sig[4] * gr[a][1] + sig[2] * gr[a][2]) * sc;
#pragma unroll
        for (int b = a; b < 8; b++) {
            const int i = kg_index(a, b);
            const double v = elem_sum(t[0] * gr[b][0] + t[1] * gr[b][1] + t[2] * gr[b][2]);
            if ((i & 7) == L.g) mine[i >> 3] = v;
        }
    }
    wave_sync();   // every lane is done with the records
    double *stg = lds[L.wv];   // 8 x 36 = 288 of its 400 doubles
#pragma unroll
    for (int j = 0; j < 5; j++)
        if (8 * j + L.g < KG_N) stg[L.el * KG_N + 8 * j + L.g] = mine[j];
    wave_sync();
    double *dst = s36 + L.e0 * KG_N;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int idx = j * 64 + L.lane;
        if (idx < 8 * KG_N && L.e0 + idx / KG_N < n_elem) dst[idx] = stg[idx];
    }
}

// the element pass on a device view whose integers have been checked; d_s36 [n_elem][36]; pt (may be null): marks 0 and 1
// around the kernel
int kg_elem_pass(stan_ctx *ctx, dev_scope &tmp, const stan_mesh &d, double *d_s36, phase_timer *pt = nullptr) {
    lamG_buf lamG;
    STANCHK(lamG.alloc(tmp, d.n_mat, d.mat_E_nu));
    HIPCHK(ctx, lamG.upload(ctx->stream));
    if (pt) STANCHK(pt->mark(0));
    if (d.n_elem > 0)   // 8 lanes per element, 8 elements per wave, 32 per workgroup
        hipLaunchKernelGGL(k_kg_elem, dim3(nblk(d.n_elem, 32)), dim3(256), 0, ctx->stream, d.n_elem, d.xyz, d.disp, d.conn, d.elem_mat,
                           d.elem_type, lamG.d, d_s36, (long long *)(ctx->d_status + SS_BAD_ELEM));
    if (pt) STANCHK(pt->mark(1));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_BAD_ELEM, ctx->d_status + SS_BAD_ELEM, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // lamG's host copy goes with this call
    return stan_detj_check(ctx, " (geometric stiffness)");
}

}  // namespace

// ---- what every matrix of element scalars s_e (x) I_3 shares (G here, the consistent mass of mass.hip) ---------------------------
// the corners of a batch: element e's corner a is "node" 8 e + a, one material
__global__ void __launch_bounds__(256)
k_kg_iota(int64_t n8, int32_t *__restrict__ conn, int32_t *__restrict__ elem_mat) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n8) return;
    conn[t] = (int32_t)t;
    if ((t & 7) == 0) elem_mat[t >> 3] = 0;
}

// ---- the maps of the gather: block row -> node (node_dof is a permutation: k_if_check) and corner -> block row --------------
__global__ void __launch_bounds__(256)
k_kg_maps(int64_t n_nodes, int64_t n_inc, const int32_t *__restrict__ node_dof, const int32_t *__restrict__ conn,
          int32_t *__restrict__ row_node, int32_t *__restrict__ crow) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_nodes) row_node[node_dof[3 * t] / 3] = (int32_t)t;
    if (t < n_inc) crow[t] = node_dof[3 * (int64_t)conn[t]] / 3;
}

// ---- row gather: k_shift_matrix's walk over the slices -------------------------------------------------------------------
// vals [nslots][9][64].  A row's own slots are its first rowlen; their columns are distinct block rows.  matched counts the
// (incidence, b) pairs that found their column: a row whose count is not 8 x its incidences belongs to another mesh
// (status[SS_ERRBITS] |= 1).
__global__ void __launch_bounds__(256)
k_kg_gather(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
            const int32_t *__restrict__ rowlen, const int32_t *__restrict__ cols, const uint8_t *__restrict__ fixmask,
            const int32_t *__restrict__ row_node, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list,
            const int32_t *__restrict__ crow, const double *__restrict__ s36, double *__restrict__ vals, int64_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int64_t row = rowof[slice * 64 + lane];
    const bool live = row < nloc;
    const int32_t len = live ? rowlen[row] : 0;
    const int rfix = live ? fixmask[row] : 7;
    int64_t p0 = 0, p1 = 0;
    if (live) {
        const int64_t nd = row_node[row];
        p0 = ptr[nd]; p1 = ptr[nd + 1];
    }
    const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
    int64_t matched = 0;
    for (int32_t k = k0; k < k1; k++) {
        const bool own = k - k0 < len;
        const int32_t c = own ? cols[(int64_t)k * 64 + lane] : -1;
        double sum = 0.0;
        if (own) {
            for (int64_t p = p0; p < p1; p++) {   // ascending element, then local node
                const int32_t t = list[p];
                const int64_t e = t >> 3;
                const int a = t & 7;
                const int4 c0 = *(const int4 *)(crow + e * 8), c1 = *(const int4 *)(crow + e * 8 + 4);
                const int32_t cb[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
                for (int b = 0; b < 8; b++)
                    if (cb[b] == c) {
                        const int i = a <= b ? a * 8 - a * (a - 1) / 2 + (b - a) : b * 8 - b * (b - 1) / 2 + (a - b);
                        sum += s36[e * KG_N + i];
                        matched++;
                    }
            }
        }
        const bool diag = own && c == (int32_t)row;
        const int cfix = own ? fixmask[c] : 7;
        double *o = vals + (int64_t)k * 9 * 64 + lane;
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int n = 0; n < 3; n++) {
                double v = 0.0;
                if (own) {
                    if (((rfix >> m) & 1) || ((cfix >> n) & 1)) v = diag && m == n ? 1.0 : 0.0;   // as k_numeric leaves a fixed DOF
                    else if (m == n) v = sum;
                }
                o[(3 * m + n) * 64] = v;
            }
    }
    if (matched != (p1 - p0) * 8) atomicOr((unsigned long long *)&status[SS_ERRBITS], 1ull);
}

int stan_elem_batch_iota(stan_ctx *ctx, int64_t n, int32_t *d_conn, int32_t *d_mat) {
    hipLaunchKernelGGL(k_kg_iota, dim3(nblk(n * 8, 256)), dim3(256), 0, ctx->stream, n * 8, d_conn, d_mat);
    const long long none = NONE;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_status + SS_BAD_ELEM, &none, 8, hipMemcpyHostToDevice, ctx->stream));
    return STAN_OK;
}

int stan_elem_scalars_matrix(stan_ctx *ctx, dev_scope &tmp, const char *who, stan_matrix *K, const stan_mesh &d, const double *d_s36,
                             stan_matrix **out, double ms[3]) {
    hipStream_t st = ctx->stream;
    const int64_t n_inc = d.n_elem * 8;
    phase_timer pt2(ctx, 4);   // layout copy, lists and maps, gather
    // ---- the new matrix: K's structure, its own values, nothing derived (stan_matrix_clone_layout)
    stan_matrix *G = nullptr;
    STANCHK(pt2.mark(0));
    STANCHK(stan_matrix_clone_layout(ctx, K, &G));
    stan_matrix_guard g{G};   // a failed call gives back what it had allocated
    STANCHK(pt2.mark(1));

    // ---- lists and maps, then the gather
    int64_t *d_ptr;
    int32_t *d_list, *d_row_node, *d_crow;
    STANCHK(stan_incidence_lists(ctx, tmp, d.n_nodes, d.n_elem, d.conn, true, &d_ptr, &d_list));
    STANCHK(tmp.alloc(&d_row_node, (size_t)d.n_nodes));
    STANCHK(tmp.alloc(&d_crow, (size_t)(n_inc > 0 ? n_inc : 1)));
    hipLaunchKernelGGL(k_kg_maps, dim3(nblk(n_inc > d.n_nodes ? n_inc : d.n_nodes, 256)), dim3(256), 0, st, d.n_nodes, n_inc, d.node_dof,
                       d.conn, d_row_node, d_crow);
    HIPCHK(ctx, hipMemsetAsync(ctx->d_status + SS_ERRBITS, 0, 8, st));
    STANCHK(pt2.mark(2));
    if (K->nslices > 0)
        hipLaunchKernelGGL(k_kg_gather, dim3(nblk(K->nslices, 4)), dim3(256), 0, st, K->nslices, K->nloc, K->d_slot_ptr, K->d_rowof,
                           K->d_rowlen, K->d_cols, K->d_fixmask, d_row_node, d_ptr, d_list, d_crow, d_s36, G->vals64(), ctx->d_status);
    STANCHK(pt2.mark(3));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_ERRBITS, ctx->d_status + SS_ERRBITS, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    for (int k = 0; k < 3; k++) STANCHK(pt2.read(k, k + 1, &ms[k]));
    if (ctx->h_status[SS_ERRBITS]) {
        ctx->err = std::string(who) + ": an element couples two nodes that K's pattern does not (another mesh)";
        return STAN_E_ARG;
    }
    g.ok = true;
    *out = G;
    return STAN_OK;
}

int stan_elem_scalars_matrix_args(stan_ctx *ctx, dev_scope &tmp, const char *who, stan_matrix *K, const stan_mesh &d) {
    auto bad = [&](const char *why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; };
    STANCHK(stan_elem_limits_check(ctx, who, d));
    if (K->nhalo != 0 || K->r0 != 0 || K->nloc != K->nb_glob) return bad("K is a shard of a larger matrix", STAN_E_UNSUPPORTED);
    if (d.n_nodes != K->nb_glob || d.n_dof != K->n_dof) return bad("the mesh does not have K's block rows", STAN_E_ARG);
    int64_t n_fixed;
    STANCHK(stan_elem_args_check(ctx, tmp, who, d, 0, nullptr, nullptr, &n_fixed));
    if (d.n_dof - n_fixed != K->n_red) return bad("the mesh does not have K's fixed DOFs", STAN_E_ARG);
    return STAN_OK;
}

int stan_kg_batch_device(stan_ctx *ctx, int64_t n, const double *d_xyz8, const double *d_u8, double E, double nu,
                         const uint8_t *d_type, double *d_s36) {
    if (n <= 0) return STAN_OK;
    if (n >= (int64_t)1 << 28) { ctx->err = "kg_hex8_batch: more than 2^28 elements"; return STAN_E_ARG; }
    dev_scope tmp(ctx);
    int32_t *d_conn, *d_mat;
    STANCHK(tmp.alloc(&d_conn, (size_t)n * 8));
    STANCHK(tmp.alloc(&d_mat, (size_t)n));
    STANCHK(stan_elem_batch_iota(ctx, n, d_conn, d_mat));
    const double E_nu[2] = {E, nu};
    const stan_mesh d{.n_nodes = n * 8, .n_elem = n, .n_mat = 1, .xyz = d_xyz8, .disp = d_u8, .conn = d_conn, .elem_mat = d_mat,
                      .elem_type = d_type, .mat_E_nu = E_nu};
    return kg_elem_pass(ctx, tmp, d, d_s36);
}

int stan_geometric_stiffness_device(stan_ctx *ctx, stan_matrix *K, const stan_mesh &d, stan_matrix **out) {
    const char *who = "geometric_stiffness_hex8";
    dev_scope tmp(ctx);
    STANCHK(stan_elem_scalars_matrix_args(ctx, tmp, who, K, d));

    // ---- the element scalars (the largest temporary: given back with `tmp`)
    double *d_s36;
    STANCHK(tmp.alloc(&d_s36, (size_t)(d.n_elem > 0 ? d.n_elem : 1) * KG_N));
    for (double &ms : ctx->prof_kg_ms) ms = 0;
    phase_timer pt(ctx, 2);   // element pass | layout copy, lists and maps, gather: stan_elem_scalars_matrix
    STANCHK(kg_elem_pass(ctx, tmp, d, d_s36, &pt));
    STANCHK(pt.read(0, 1, &ctx->prof_kg_ms[0]));
    return stan_elem_scalars_matrix(ctx, tmp, who, K, d, d_s36, out, ctx->prof_kg_ms + 1);
}
