// api_solve.hip -- the extern "C" surface, part 2 of 5: assembly, the CG solves, products and what a matrix tells about itself.
#include <cstring>

#include "api_stage.h"

namespace {
// A rank of a sharded run only needs the elements that touch its block rows (boundary elements
// are assembled by both owners): they are picked on the host, in element order (the
// accumulation order of a row is the element order, so K keeps its bits), and only they go to
// the device -- neither the upload nor the incidence scan of a rank grows with the ranks of
// the others.  The node arrays stay whole: any node may be a halo column.
struct shard_pick {
    std::vector<int32_t> elems, conn, mat;   // the picked elements by their numbers in the whole model, ascending; their arrays
    std::vector<uint8_t> type;
    stan_mesh mesh;                          // host view: the picked element arrays, everything else as in the whole model
};
int pick_shard_elements(stan_ctx *ctx, const stan_mesh &m, shard_pick *out) {
    const int64_t nb = m.n_dof / 3;
    const int64_t r0 = stan_row_start(nb, ctx->nranks, ctx->rank), r1 = stan_row_start(nb, ctx->nranks, ctx->rank + 1);
    for (int64_t e = 0; e < m.n_elem; e++) {
        bool mine = false;
        for (int a = 0; a < 8; a++) {
            const int32_t nd = m.conn[e * 8 + a];
            if (nd < 0 || nd >= m.n_nodes) {
                ctx->err = "assemble: connectivity references a node index outside [0,n_nodes)";
                return STAN_E_ARG;
            }
            const int64_t row = m.node_dof[3 * (int64_t)nd] / 3;   // a bad DOF layout is caught on the device
            mine |= row >= r0 && row < r1;
        }
        if (mine) out->elems.push_back((int32_t)e);
    }
    const size_t n = out->elems.size();
    out->conn.resize(n * 8); out->mat.resize(n); out->type.resize(n);
    for (size_t i = 0; i < n; i++) {
        memcpy(&out->conn[8 * i], m.conn + 8 * (int64_t)out->elems[i], 8 * sizeof(int32_t));
        out->mat[i] = m.elem_mat[out->elems[i]];
        out->type[i] = m.elem_type[out->elems[i]];
    }
    out->mesh = m;
    out->mesh.n_elem = (int64_t)n;
    out->mesh.conn = out->conn.data(); out->mesh.elem_mat = out->mat.data(); out->mesh.elem_type = out->type.data();
    return STAN_OK;
}
}  // namespace

// ---- the host entry of one context, behind the argument checks of the public entry (a group's ranks start here) ----
int stan_assemble_host(stan_ctx *ctx, const stan_mesh &whole, stan_matrix **outK) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (not mesh_range_check: a foreign element type is STAN_E_UNSUPPORTED here, the connectivity is left to the pick or the device)
    auto bad = [&](const char *why, int64_t e, int rc) { ctx->err = std::string("assemble_hex8: ") + why + " at element " + std::to_string(e); return rc; };
    for (int64_t e = 0; e < whole.n_elem; e++) {
        if (whole.elem_mat[e] < 0 || whole.elem_mat[e] >= whole.n_mat) return bad("elem_mat out of range", e, STAN_E_ARG);
        if (whole.elem_type[e] != STAN_HEX8_G1 && whole.elem_type[e] != STAN_HEX8_G2) return bad("unsupported element type", e, STAN_E_UNSUPPORTED);
    }
    shard_pick pick;
    host_stage st(ctx);   // behind `pick`: the uploads read its vectors
    const bool shard = ctx->nranks > 1 && whole.n_elem > 0;
    if (shard) STANCHK(pick_shard_elements(ctx, whole, &pick));
    mesh_dbufs bufs;
    STANCHK(bufs.upload(st, shard ? pick.mesh : whole));
    const int rc = stan_assemble_device(ctx, bufs.dev, outK);
    if (rc == STAN_OK) (*outK)->n_elem_scanned = bufs.dev.n_elem;
    if (rc == STAN_E_DETJ && shard && ctx->bad_elem >= 0 && ctx->bad_elem < (int64_t)pick.elems.size()) {
        ctx->bad_elem = pick.elems[(size_t)ctx->bad_elem];   // element number of the whole model
        ctx->err = "det J == 0 in element " + std::to_string(ctx->bad_elem) + " (MatrixST.Inverse would throw)";
    }
    return st.finish(rc);   // the uploads are stream-ordered with the assembly
}

extern "C" {

int stan_hip_assemble_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz,
                               const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn,
                               const int32_t *d_elem_mat, const uint8_t *d_elem_type,
                               int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                               const int32_t *d_red, stan_matrix **outK) {
    if (!ctx || !outK || !d_xyz || !d_node_dof || !d_red || !mat_E_nu ||
        (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type)))
        return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "assemble_hex8_dev (device pointers belong to one device)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    return stan_assemble_device(ctx, d, outK);
}

int stan_hip_assemble_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz,
                           const int32_t *node_dof, int64_t n_elem, const int32_t *conn,
                           const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat,
                           const double *mat_E_nu, int64_t n_dof, const int32_t *red,
                           stan_matrix **outK) {
    if (!ctx || !outK || !xyz || !node_dof || !red || !mat_E_nu || n_nodes <= 0 || n_dof <= 0 ||
        n_elem < 0 || (n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        if (ctx) ctx->err = "assemble_hex8: null or empty argument";
        return STAN_E_ARG;
    }
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .node_dof = node_dof,
                      .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red, .mat_E_nu = mat_E_nu};
    return ctx->group ? stan_group_assemble(ctx, m, outK) : stan_assemble_host(ctx, m, outK);
}

void stan_hip_matrix_free(stan_matrix *K) {
    if (!K) return;
    if (!K->parts.empty()) { stan_group_matrix_free(K); return; }
    if (K->ctx) {
        hipSetDevice(K->ctx->device);
        auto &v = K->ctx->matrices;
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] == K) { v.erase(v.begin() + i); break; }
    }
    // the solves that used these buffers have been synchronised by their own calls; the blocks go
    // back to the context's pool (stan_pool) or to the driver
    // (the padded streams first, then the folded copy: the order decides which parked block the next matrix gets)
    auto release = [&](std::initializer_list<void *> blocks) { for (void *q : blocks) stan_dfree(K->ctx, q); };
    release({K->d_slot_ptr, K->d_rowlen, K->d_rowof, K->d_posof, K->d_cols});
    for (const stan_value_stream &s : K->vs) release({s.padded});
    release({K->pk.cols16, K->pk.colbase, K->pk.pair_ptr, K->pk.packed, K->d_red, K->d_fixmask, K->d_scale, K->d_send_rows, K->d_halo_glob,
             K->d_sendbuf, K->d_sl_int, K->d_sl_bnd, K->d_fold_ptr, K->d_fold_meta, K->d_fold_plan, K->d_fold_cols, K->fold_pk.cols16,
             K->fold_pk.colbase, K->fold_pk.pair_ptr, K->fold_pk.packed});
    for (const stan_value_stream &s : K->vs) release({s.folded});
    delete K;
}

int stan_hip_cg_solve_dev(stan_ctx *ctx, stan_matrix *K, const double *d_F, double eps_f,
                          int32_t max_its, int32_t precision_mode, double *d_U,
                          int32_t *termination_type, int32_t *iterations, double *rel_residual) {
    if (!ctx || !K || !d_F || !d_U || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "cg_solve_dev (device pointers belong to one device)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_cg_device(ctx, K, d_F, eps_f, max_its, precision_mode, d_U, termination_type,
                          iterations, rel_residual);
}

int stan_hip_cg_solve(stan_ctx *ctx, stan_matrix *K, const double *F, double eps_f,
                      int32_t max_its, int32_t precision_mode, double *U,
                      int32_t *termination_type, int32_t *iterations, double *rel_residual) {
    if (!ctx || !K || !F || !U || K->ctx != ctx) return STAN_E_ARG;
    if (ctx->group)
        return stan_group_cg_solve(ctx, K, F, eps_f, max_its, precision_mode, U, termination_type, iterations,
                                   rel_residual);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red;
    host_stage st(ctx);
    dbuf<double> dF, dU;
    if (ctx->result_segment && ctx->nranks > 1) {
        // a rank of a one-process group: only ITS entries [u0, u1) of F go up and of U come down -- the ranks
        // share the caller's buffers (disjoint ranges), nothing is gathered on the devices (multi.hip)
        const size_t u0 = (size_t)K->u0, nu = (size_t)(K->u1 - K->u0);
        STANCHK(dF.alloc(st, N ? N : 1));
        STANCHK(dU.alloc(st, N ? N : 1));
        if (nu) STANCHK(st.copy(dF.p + u0, F + u0, nu * 8, hipMemcpyHostToDevice));
        STANCHK(stan_cg_device(ctx, K, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type,
                               iterations, rel_residual));
        if (nu) STANCHK(st.copy(U + u0, dU.p + u0, nu * 8, hipMemcpyDeviceToHost));
        return st.sync();
    }
    STANCHK(dF.upload(st, F, N));
    STANCHK(dU.alloc(st, N, U));
    HIPCHK(ctx, hipMemsetAsync(dU.p, 0, (N ? N : 1) * 8, ctx->stream));
    STANCHK(stan_cg_device(ctx, K, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type,
                           iterations, rel_residual));
    return st.finish(STAN_OK, dU);
}

// Several load cases against one K (cg.hip: stan_cg_multi_device).  One device, one rank: a multi-device handle is refused.
int stan_hip_cg_solve_multi_dev(stan_ctx *ctx, stan_matrix *K, int32_t n_rhs, const double *d_F, double eps_f,
                                int32_t max_its, int32_t precision_mode, double *d_U, int32_t *termination_type,
                                int32_t *iterations, double *rel_residual) {
    if (!ctx || !K || !d_F || !d_U || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "cg_solve_multi_dev");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_cg_multi_device(ctx, K, n_rhs, d_F, eps_f, max_its, precision_mode, d_U, termination_type, iterations,
                                rel_residual);
}

int stan_hip_cg_solve_multi(stan_ctx *ctx, stan_matrix *K, int32_t n_rhs, const double *F, double eps_f, int32_t max_its,
                            int32_t precision_mode, double *U, int32_t *termination_type, int32_t *iterations,
                            double *rel_residual) {
    if (!ctx || !K || !F || !U || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "cg_solve_multi");
    if (n_rhs <= 0) { ctx->err = "cg_solve_multi: n_rhs must be > 0"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)K->n_red * (size_t)n_rhs;
    host_stage st(ctx);
    dbuf<double> dF, dU;
    STANCHK(dF.upload(st, F, n));
    STANCHK(dU.alloc(st, n, U));
    HIPCHK(ctx, hipMemsetAsync(dU.p, 0, (n ? n : 1) * 8, ctx->stream));
    STANCHK(stan_cg_multi_device(ctx, K, n_rhs, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type, iterations,
                                 rel_residual));
    return st.finish(STAN_OK, dU);
}

int stan_hip_matrix_part_info(stan_matrix *K, int32_t part, stan_matrix_info *o) {
    if (!K || !o || part < 0) return STAN_E_ARG;
    if (K->parts.empty()) return part == 0 ? stan_hip_matrix_info(K, o) : STAN_E_ARG;
    if ((size_t)part >= K->parts.size()) return STAN_E_ARG;
    return stan_hip_matrix_info(K->parts[(size_t)part], o);
}

int stan_hip_matrix_info(stan_matrix *K, stan_matrix_info *o) {
    if (!K || !o) return STAN_E_ARG;
    o->n_dof = K->n_dof; o->n_reduced = K->n_red; o->n_block_rows = K->nb_glob;
    o->row_begin = K->r0; o->row_end = K->r1; o->n_halo = K->nhalo; o->n_blocks = K->nblocks;
    o->n_slots = K->nslots;
    o->bytes_matrix = K->nslots * 64 * (9 * 8 + 4);
    o->scaled = (K->parts.empty() ? K->scaled : K->parts[0]->scaled) ? 1 : 0;
    o->max_row_blocks = K->max_row_blocks;
    o->n_elements_on_device = K->n_elem_scanned;
    o->sell_sigma = K->parts.empty() ? K->sigma : K->parts[0]->sigma;
    const stan_matrix *P = K->parts.empty() ? K : K->parts[0];
    o->folded_slots_permille = P->fold_state == 1 && P->nslots > 0 ? (int32_t)(1000 * P->nfslots / P->nslots) : 0;
    return STAN_OK;
}

int stan_hip_ke_hex8_batch(stan_ctx *ctx, int64_t n, const double *xyz8, double E, double nu,
                           const uint8_t *type, double *out) {
    if (!ctx || n < 0 || (n > 0 && (!xyz8 || !type || !out))) return STAN_E_ARG;
    if (ctx->group)
        return stan_group_rank0_call(ctx, [&](stan_ctx *c) { return stan_hip_ke_hex8_batch(c, n, xyz8, E, nu, type, out); });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int64_t e = 0; e < n; e++)
        if (type[e] != STAN_HEX8_G1 && type[e] != STAN_HEX8_G2) {
            ctx->err = "ke_hex8: unsupported element type";
            return STAN_E_UNSUPPORTED;
        }
    host_stage st(ctx);
    dbuf<double> dx, dk; dbuf<uint8_t> dt;
    STANCHK(dx.upload(st, xyz8, (size_t)n * 24));
    STANCHK(dt.upload(st, type, (size_t)n));
    STANCHK(dk.alloc(st, (size_t)n * 576, out));
    STANCHK(stan_ke_batch_device(ctx, n, dx.p, E, nu, dt.p, dk.p));
    return st.finish(STAN_OK, dk);
}

int stan_hip_ke_hex8(stan_ctx *ctx, const double xyz8[24], double E, double nu, int32_t type,
                     double out[576]) {
    uint8_t t = (uint8_t)type;
    if (type != STAN_HEX8_G1 && type != STAN_HEX8_G2) {
        if (ctx) ctx->err = "ke_hex8: unsupported element type";
        return STAN_E_UNSUPPORTED;
    }
    return stan_hip_ke_hex8_batch(ctx, 1, xyz8, E, nu, &t, out);
}

int stan_hip_matrix_to_csr(stan_ctx *ctx, stan_matrix *K, int32_t upper_only, int64_t *nnz,
                           int64_t *rowptr, int32_t *col, double *val) {
    if (!ctx || !K || !nnz || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "matrix_to_csr");
    if (ctx->nranks != 1) { ctx->err = "matrix_to_csr: single-rank contexts only"; return STAN_E_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // export K itself, not S K S.  A matrix no solve has scaled yet is exported AS ASSEMBLED -- the exact bits, and the
    // export changes nothing (round 5 scaled it here as a side effect, which also cost the next solve its lazy-scaling
    // first product: ADVICE r05).  Once a solve has brought it into its scaled form, the values are divided by
    // s_row s_col on the way out: within 1 ulp of the assembled entry ((a t) / t), the matrix again untouched.
    const bool scaled = K->scaled;
    const int64_t nloc = K->nloc;
    std::vector<double> scale((size_t)3 * (size_t)K->nslices * 64);
    std::vector<int32_t> slot_ptr((size_t)K->nslices + 1), rowlen((size_t)K->nslices * 64),
        posof((size_t)K->nslices * 64), cols((size_t)K->nslots * 64), red((size_t)K->n_dof);
    std::vector<double> vals((size_t)K->nslots * 9 * 64);
    host_stage st(ctx);   // behind the vectors: the downloads fill them
    STANCHK(st.copy(slot_ptr.data(), K->d_slot_ptr, slot_ptr.size() * 4, hipMemcpyDeviceToHost));
    if (!rowlen.empty()) STANCHK(st.copy(rowlen.data(), K->d_rowlen, rowlen.size() * 4, hipMemcpyDeviceToHost));
    if (!posof.empty()) STANCHK(st.copy(posof.data(), K->d_posof, posof.size() * 4, hipMemcpyDeviceToHost));
    if (!cols.empty()) STANCHK(st.copy(cols.data(), K->d_cols, cols.size() * 4, hipMemcpyDeviceToHost));
    if (!vals.empty()) STANCHK(st.copy(vals.data(), K->vals64(), vals.size() * 8, hipMemcpyDeviceToHost));
    STANCHK(st.copy(red.data(), K->d_red, red.size() * 4, hipMemcpyDeviceToHost));
    if (scaled && !scale.empty()) STANCHK(st.copy(scale.data(), K->d_scale, scale.size() * 8, hipMemcpyDeviceToHost));
    STANCHK(st.sync());
    int64_t count = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && (!rowptr || !col || !val)) break;
        int64_t q = 0;
        for (int64_t row = 0; row < nloc; row++) {
            const int64_t sl = posof[(size_t)row] >> 6;   // SELL-C-sigma: where the row sits in the sliced layout
            const int lane = (int)(posof[(size_t)row] & 63);
            for (int m = 0; m < 3; m++) {
                const int64_t d = 3 * row + m;
                if (red[d] == -1) continue;
                if (pass == 1) rowptr[d - red[d]] = q;
                for (int k = 0; k < rowlen[row]; k++) {
                    const int64_t slot = (int64_t)slot_ptr[sl] + k;
                    const int32_t c = cols[slot * 64 + lane];
                    for (int n = 0; n < 3; n++) {
                        const int64_t dc = 3 * (int64_t)c + n;
                        if (red[dc] == -1) continue;
                        if (upper_only && dc < d) continue;
                        if (pass == 1) {
                            col[q] = (int32_t)(dc - red[dc]);
                            const double a = vals[(slot * 9 + 3 * m + n) * 64 + lane];
                            val[q] = scaled ? stan_unscaled_value(a, scale[(size_t)d], scale[(size_t)dc]) : a;
                        }
                        q++;
                    }
                }
            }
        }
        if (pass == 0) count = q;
        else rowptr[K->n_red] = q;
    }
    *nnz = count;
    return STAN_OK;
}

int stan_hip_spmv(stan_ctx *ctx, stan_matrix *K, const double *x, double *y) {
    if (!ctx || !K || !x || !y || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "spmv");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red;
    host_stage st(ctx);
    dbuf<double> dx, dy;
    STANCHK(dx.upload(st, x, N));
    STANCHK(dy.alloc(st, N, y));
    STANCHK(stan_spmv_reduced(ctx, K, dx.p, dy.p));
    return st.finish(STAN_OK, dy);
}

int stan_hip_matrix_diagonal(stan_ctx *ctx, stan_matrix *K, double *diag) {
    if (!ctx || !K || !diag || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "matrix_diagonal");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dd;
    STANCHK(dd.alloc(st, (size_t)K->n_red, diag));   // (an empty request is served with one double)
    STANCHK(stan_matrix_diagonal(ctx, K, dd.p));
    return st.finish(STAN_OK, dd);
}

int stan_hip_matrix_plan(stan_ctx *ctx, stan_matrix *K, int64_t *row_starts, int64_t *n_halo,
                         int32_t *halo_glob, int32_t *n_nbr, int32_t *nbr, int64_t *send_off,
                         int32_t *send_rows, int64_t *recv_off) {
    if (!ctx || !K || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "matrix_plan");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (row_starts) for (size_t i = 0; i < K->row_starts.size(); i++) row_starts[i] = K->row_starts[i];
    if (n_halo) *n_halo = K->nhalo;
    if (n_nbr) *n_nbr = (int32_t)K->nbr.size();
    if (nbr) for (size_t i = 0; i < K->nbr.size(); i++) nbr[i] = K->nbr[i];
    if (send_off) { send_off[0] = 0; for (size_t i = 0; i < K->send_off.size(); i++) send_off[i] = K->send_off[i]; }
    if (recv_off) { recv_off[0] = 0; for (size_t i = 0; i < K->recv_off.size(); i++) recv_off[i] = K->recv_off[i]; }
    if (halo_glob && K->nhalo)
        HIPCHK(ctx, hipMemcpy(halo_glob, K->d_halo_glob, (size_t)K->nhalo * 4, hipMemcpyDeviceToHost));
    if (send_rows && !K->send_off.empty() && K->send_off.back())
        HIPCHK(ctx, hipMemcpy(send_rows, K->d_send_rows, (size_t)K->send_off.back() * 4, hipMemcpyDeviceToHost));
    return STAN_OK;
}

int stan_hip_spmv_local(stan_ctx *ctx, stan_matrix *K, const double *x_local, double *y_owned) {
    if (!ctx || !K || !x_local || !y_owned || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "spmv_local");
    if (K->scaled) { ctx->err = "spmv_local: matrix already carries the CG scaling"; return STAN_E_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t npad = (int64_t)K->nslices * 64;
    const int64_t ng = 3 * (npad > K->nloc + K->nhalo ? npad : K->nloc + K->nhalo);
    host_stage st(ctx);
    dbuf<double> dx, dy;
    STANCHK(dx.alloc(st, (size_t)ng));
    STANCHK(dy.alloc(st, (size_t)(3 * npad + 3)));
    HIPCHK(ctx, hipMemsetAsync(dx.p, 0, (size_t)ng * 8, ctx->stream));
    STANCHK(st.copy(dx.p, x_local, (size_t)(3 * (K->nloc + K->nhalo)) * 8, hipMemcpyHostToDevice));
    STANCHK(stan_spmv_local(ctx, K, dx.p, dy.p));
    if (K->nloc) STANCHK(st.copy(y_owned, dy.p, (size_t)(3 * K->nloc) * 8, hipMemcpyDeviceToHost));
    return st.sync();
}

int stan_hip_spmv_bench(stan_ctx *ctx, stan_matrix *K, int32_t precision_mode, int32_t reps,
                        double *avg_ms) {
    if (!ctx || !K || !avg_ms || reps <= 0 || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "spmv_bench");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_spmv_bench_device(ctx, K, precision_mode, reps, avg_ms);
}

int stan_hip_stream60_roundtrip(stan_ctx *ctx, int64_t n, const double *in, double *out, int64_t *refused) {
    if (!ctx || n <= 0 || !in || !out || !refused) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "stream60_roundtrip");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_stream60_roundtrip_device(ctx, n, in, out, refused);
}

int stan_hip_stream_bench(stan_ctx *ctx, stan_matrix *K, int32_t reps, double *avg_ms, int64_t *bytes) {
    if (!ctx || !K || !avg_ms || !bytes || reps <= 0 || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "stream_bench");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_stream_bench_device(ctx, K, reps, avg_ms, bytes);
}

}  // extern "C"
