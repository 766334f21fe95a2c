// api_buckling.hip -- the extern "C" surface of linear buckling: the element scalars of the geometric
// stiffness on a batch (introspection), the assembled matrix G = K_g(U) in K's layout (geometric.hip), and the driver loop of
// stan_hip_buckling over the solver's batched CG (stan_cg_multi_device), its products (stan_spmv_reduced) on K and on G, the
// block kernels of modal.hip and the q x q eigenproblem of api_modal.hip on the host; the stages it has in common with the modal
// driver are block_run's (api_stage.h).  One device, one rank.
#include <algorithm>
#include <cmath>

#include "api_stage.h"

namespace {

int kg_args(stan_ctx *ctx, const char *who, stan_matrix *K, stan_matrix **out, bool null_arg) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, who));
    if (!K || !out || null_arg) { ctx->err = std::string(who) + ": null or empty argument"; return STAN_E_ARG; }
    if (K->ctx != ctx) { ctx->err = std::string(who) + ": K belongs to another context"; return STAN_E_ARG; }
    return STAN_OK;
}

// The driver on device arrays: d_factor / d_rho [k], d_phi [k][N].  With H = -G the k largest positive mu of H x = mu K x by
// block inverse iteration in correction form with a Rayleigh-Ritz step; factor = 1 / mu.
// pencil (stan_hip_modes_pencil, section 3.13): the same loop with H = +G, G a mass matrix, so that 1 / mu are the eigenvalues of
// K phi = lambda G phi, and the vectors scaled to phi^T G phi = 1 by one true product at the end.
int buckling_device(stan_ctx *ctx, bool pencil, stan_matrix *K, stan_matrix *G, int32_t k, double tol, int32_t max_outer, double solve_eps,
                    int32_t solve_max_its, double *d_factor, double *d_phi, double *d_rho, stan_buckling_report *rep) {
    block_run<stan_buckling_report> run(ctx, K, pencil ? "modes_pencil" : "buckling", k, tol, max_outer, solve_eps, solve_max_its);
    STANCHK(run.begin(rep));
    stan_buckling_report &R = run.R;
    piece_timer &pt = run.pt;
    const int64_t N = run.N;
    const int q = run.q;
    hipStream_t st = ctx->stream;
    // the solves run with the merit stop off, as the transient driver's do (its type 7 would leave a correction unfinished)
    merit_off merit(ctx);

    dev_scope tmp(ctx);
    double *Z, *W, *Y, *rhs, *D, *dg;   // [q][N] each (dg: [N], diag K); X lives in Z, K X in W
    const size_t qn = (size_t)q * (size_t)N;
    STANCHK(tmp.alloc(&Z, qn));
    STANCHK(tmp.alloc(&W, qn));
    STANCHK(tmp.alloc(&Y, qn));
    STANCHK(tmp.alloc(&rhs, qn));
    STANCHK(tmp.alloc(&D, qn));
    STANCHK(tmp.alloc(&dg, (size_t)N));

    // out_j = H in_j = -(G in_j), q true products; the negation is exact (pencil: H = G, no negation)
    auto h_products = [&](const double *in, double *out) -> int {
        if (pencil) return run.products(G, in, out);
        return run.products(G, in, out, [&] { return stan_buckling_negate_device(ctx, (int64_t)qn, out); });
    };
    pt.begin();
    STANCHK(stan_buckling_start_device(ctx, N, q, Z));
    pt.end(&R.block_ms);
    STANCHK(h_products(Z, rhs));
    STANCHK(run.solve(q, rhs, Z, "a model without supports?"));
    STANCHK(stan_matrix_diagonal(ctx, K, dg));   // (behind the first solve: K is in the state every later step finds it in)

    std::vector<double> A((size_t)q * q), B((size_t)q * q), unused((size_t)q * q), Qm((size_t)q * q), mu((size_t)q), r2((size_t)q),
        kx2((size_t)q), rho((size_t)q);
    for (;;) {
        R.outer++;
        STANCHK(run.products(K, Z, W));
        STANCHK(h_products(Z, Y));
        pt.begin();   // A = Z^T W, B = Z^T Y: the modal gram pass twice (its second output, Z^T (dg o Z), is not used)
        STANCHK(stan_modal_gram_device(ctx, N, q, Z, W, dg, A.data(), unused.data()));
        STANCHK(stan_modal_gram_device(ctx, N, q, Z, Y, dg, B.data(), unused.data()));
        pt.end(&R.gram_ms);
        for (int i = 0; i < q; i++)
            for (int j = i + 1; j < q; j++) {
                A[(size_t)i * q + j] = A[(size_t)j * q + i] = 0.5 * (A[(size_t)i * q + j] + A[(size_t)j * q + i]);
                B[(size_t)i * q + j] = B[(size_t)j * q + i] = 0.5 * (B[(size_t)i * q + j] + B[(size_t)j * q + i]);
            }
        // B Q = A Q diag(mu) through the Cholesky factor of A = Z^T K Z, mu descending
        if (!stan_small_gen_eig(q, B.data(), A.data(), mu.data(), Qm.data(), true))
            return run.bad("the block lost rank (Z^T K Z is not positive definite)", STAN_E_UNSUPPORTED);
        const bool last = R.outer >= run.max_outer;
        pt.begin();   // the last step needs no right-hand side: every column masked
        STANCHK(stan_buckling_rotate_device(ctx, N, q, Z, W, Y, dg, Qm.data(), mu.data(), last ? 0xffffffffu : 0u, Z, W, rhs, r2.data(),
                                            kx2.data()));
        pt.end(&R.rotate_ms);
        bool done = true;
        R.max_rho = 0.0;
        R.n_positive = 0;
        for (int j = 0; j < q; j++) {
            rho[(size_t)j] = std::sqrt(r2[(size_t)j]) / (std::fabs(mu[(size_t)j]) * std::sqrt(kx2[(size_t)j]));
            if (mu[(size_t)j] > 0.0) R.n_positive++;
            if (j < k) {
                done = done && mu[(size_t)j] > 0.0 && rho[(size_t)j] <= run.tol;
                R.max_rho = std::max(R.max_rho, rho[(size_t)j]);
            }
        }
        R.lowest_negative_factor = mu[(size_t)q - 1] < 0.0 ? 1.0 / mu[(size_t)q - 1] : 0.0;   // mu descends
        R.converged = done ? 1 : 0;
        if (done || last) break;
        // K D = -R for the columns that have not converged (a column is solved again where rho > tol), then
        // Z = X diag(mu) + D: defined for every sign of mu
        int n;
        STANCHK(run.pack(rhs, [&](int j) { return rho[(size_t)j] > run.tol; }, &n));
        if (n > 0) STANCHK(run.solve(n, rhs, D, "a model without supports?"));
        pt.begin();
        STANCHK(stan_buckling_axpy_device(ctx, N, q, Z, mu.data(), run.dcol.data(), D, Z));
        pt.end(&R.block_ms);
    }
    // the first min(k, n_positive) pairs; the rest of the outputs are zeros
    const int kk = std::min<int>(k, R.n_positive);
    std::vector<double> fac((size_t)k, 0.0), rh((size_t)k, 0.0);
    for (int j = 0; j < kk; j++) { fac[(size_t)j] = 1.0 / mu[(size_t)j]; rh[(size_t)j] = rho[(size_t)j]; }
    HIPCHK(ctx, hipMemsetAsync(d_phi, 0, (size_t)k * (size_t)N * 8, st));
    if (pencil && kk > 0) {   // phi_j^T G phi_j = 1: the scale from kk true products
        pt.begin();
        for (int j = 0; j < kk; j++) STANCHK(stan_spmv_reduced(ctx, G, Z + (size_t)j * N, Y + (size_t)j * N));
        pt.end(&R.product_ms);
    }
    pt.begin();
    if (kk > 0) STANCHK(pencil ? stan_pencil_normalise_device(ctx, N, kk, Z, Y, d_phi) : stan_buckling_normalise_device(ctx, N, kk, Z, d_phi));
    pt.end(&R.block_ms);
    return run.finish(fac.data(), rh.data(), d_factor, d_rho);
}

int buckling_args(stan_ctx *ctx, stan_matrix *K, stan_matrix *G, const void *factor, const void *phi, const void *rho,
                  bool pencil = false) {
    if (!ctx) return STAN_E_ARG;
    const std::string who = pencil ? "modes_pencil" : "buckling", G_name = pencil ? "Mmat" : "G";
    STANCHK(block_driver_refused(ctx, who.c_str()));
    if (!K || !G || !factor || !phi || !rho) { ctx->err = who + ": null argument"; return STAN_E_ARG; }
    if (K->ctx != ctx || G->ctx != ctx) { ctx->err = who + ": K or " + G_name + " belongs to another context"; return STAN_E_ARG; }
    if (G->n_dof != K->n_dof || G->n_red != K->n_red || G->nb_glob != K->nb_glob || G->nloc != K->nloc || G->nslices != K->nslices ||
        G->nslots != K->nslots || G->nblocks != K->nblocks || G->sigma != K->sigma) {
        ctx->err = who + ": " + G_name + " does not have K's layout (build it with " +
                   (pencil ? "stan_hip_consistent_mass_hex8" : "stan_hip_geometric_stiffness_hex8") + " on this K)";
        return STAN_E_ARG;
    }
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_buckling_dev(stan_ctx *ctx, stan_matrix *K, stan_matrix *G, int32_t n_modes, double tol, int32_t max_outer,
                          double solve_eps, int32_t solve_max_its, double *d_factor, double *d_phi, double *d_rho, void *rep) {
    STANCHK(buckling_args(ctx, K, G, d_factor, d_phi, d_rho));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return buckling_device(ctx, false, K, G, n_modes, tol, max_outer, solve_eps, solve_max_its, d_factor, d_phi, d_rho, (stan_buckling_report *)rep);
}

int stan_hip_buckling(stan_ctx *ctx, stan_matrix *K, stan_matrix *G, int32_t n_modes, double tol, int32_t max_outer, double solve_eps,
                      int32_t solve_max_its, double *factor, double *phi, double *rho, void *rep) {
    STANCHK(buckling_args(ctx, K, G, factor, phi, rho));
    if (n_modes <= 0 || n_modes > K->n_red) { ctx->err = "buckling: n_modes must be in [1, N]"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red, k = (size_t)n_modes;
    host_stage st(ctx);
    dbuf<double> df, dp, dr;
    STANCHK(df.alloc(st, k, factor));
    STANCHK(dp.alloc(st, k * N, phi));
    STANCHK(dr.alloc(st, k, rho));
    const int rc = buckling_device(ctx, false, K, G, n_modes, tol, max_outer, solve_eps, solve_max_its, df.p, dp.p, dr.p, (stan_buckling_report *)rep);
    return st.finish(rc, df, dp, dr);
}

int stan_hip_modes_pencil_dev(stan_ctx *ctx, stan_matrix *K, stan_matrix *Mmat, int32_t n_modes, double tol, int32_t max_outer,
                              double solve_eps, int32_t solve_max_its, double *d_lambda, double *d_phi, double *d_rho, void *rep) {
    STANCHK(buckling_args(ctx, K, Mmat, d_lambda, d_phi, d_rho, true));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return buckling_device(ctx, true, K, Mmat, n_modes, tol, max_outer, solve_eps, solve_max_its, d_lambda, d_phi, d_rho,
                           (stan_buckling_report *)rep);
}

int stan_hip_modes_pencil(stan_ctx *ctx, stan_matrix *K, stan_matrix *Mmat, int32_t n_modes, double tol, int32_t max_outer,
                          double solve_eps, int32_t solve_max_its, double *lambda, double *phi, double *rho, void *rep) {
    STANCHK(buckling_args(ctx, K, Mmat, lambda, phi, rho, true));
    if (n_modes <= 0 || n_modes > K->n_red) { ctx->err = "modes_pencil: n_modes must be in [1, N]"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red, k = (size_t)n_modes;
    host_stage st(ctx);
    dbuf<double> dl, dp, dr;
    STANCHK(dl.alloc(st, k, lambda));
    STANCHK(dp.alloc(st, k * N, phi));
    STANCHK(dr.alloc(st, k, rho));
    const int rc = buckling_device(ctx, true, K, Mmat, n_modes, tol, max_outer, solve_eps, solve_max_its, dl.p, dp.p, dr.p,
                                   (stan_buckling_report *)rep);
    return st.finish(rc, dl, dp, dr);
}

int stan_hip_buckling_rotate(stan_ctx *ctx, int64_t N, int32_t q, const double *Z, const double *W, const double *Y, const double *D,
                             const double *Q, const double *mu, double *X, double *KX, double *R, double *r2, double *kx2) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(block_driver_refused(ctx, "buckling_rotate"));
    if (!Z || !W || !Y || !D || !Q || !mu || !X || !KX || !R || !r2 || !kx2 || N <= 0 || q <= 0 || q > STAN_MODAL_QMAX) {
        ctx->err = "buckling_rotate: null argument, N <= 0 or q outside [1, 32]";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t qn = (size_t)q * (size_t)N;
    host_stage st(ctx);
    dbuf<double> dZ, dW, dY, dD, dX, dKX, dR;
    STANCHK(dZ.upload(st, Z, qn));
    STANCHK(dW.upload(st, W, qn));
    STANCHK(dY.upload(st, Y, qn));
    STANCHK(dD.upload(st, D, (size_t)N));
    STANCHK(dX.alloc(st, qn, X));
    STANCHK(dKX.alloc(st, qn, KX));
    STANCHK(dR.alloc(st, qn, R));
    int rc = stan_buckling_rotate_device(ctx, N, q, dZ.p, dW.p, dY.p, dD.p, Q, mu, 0u, dX.p, dKX.p, dR.p, r2, kx2);
    if (rc == STAN_OK) rc = stan_buckling_negate_device(ctx, (int64_t)qn, dR.p);   // the kernel stores the right-hand side -R
    return st.finish(rc, dX, dKX, dR);
}

int stan_hip_kg_hex8_batch(stan_ctx *ctx, int64_t n, const double *xyz8, const double *u8, double E, double nu,
                           const uint8_t *type, double *s36) {
    if (!ctx || n < 0 || (n > 0 && (!xyz8 || !u8 || !type || !s36))) return STAN_E_ARG;
    if (ctx->group)
        return stan_group_rank0_call(ctx, [&](stan_ctx *c) { return stan_hip_kg_hex8_batch(c, n, xyz8, u8, E, nu, type, s36); });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int64_t e = 0; e < n; e++)
        if (type[e] != STAN_HEX8_G1 && type[e] != STAN_HEX8_G2) {
            ctx->err = "kg_hex8: unsupported element type";
            return STAN_E_UNSUPPORTED;
        }
    host_stage st(ctx);
    dbuf<double> dx, du, ds; dbuf<uint8_t> dt;
    STANCHK(dx.upload(st, xyz8, (size_t)n * 24));
    STANCHK(du.upload(st, u8, (size_t)n * 24));
    STANCHK(dt.upload(st, type, (size_t)n));
    STANCHK(ds.alloc(st, (size_t)n * 36, s36));
    return st.finish(stan_kg_batch_device(ctx, n, dx.p, du.p, E, nu, dt.p, ds.p), ds);
}

int stan_hip_geometric_stiffness_times(stan_ctx *ctx, double ms[4]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "geometric_stiffness_times");
    for (int k = 0; k < 4; k++) ms[k] = ctx->prof_kg_ms[k];
    return STAN_OK;
}

int stan_hip_geometric_stiffness_hex8_dev(stan_ctx *ctx, stan_matrix *K, int64_t n_nodes, const double *d_xyz, const double *d_disp,
                                          const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn,
                                          const int32_t *d_elem_mat, const uint8_t *d_elem_type, int32_t n_mat,
                                          const double *mat_E_nu, int64_t n_dof, const int32_t *d_red, stan_matrix **out) {
    STANCHK(kg_args(ctx, "geometric_stiffness_hex8", K, out,
                    !d_xyz || !d_disp || !d_node_dof || !d_red || !mat_E_nu || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type))));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz, .disp = d_disp,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    stan_matrix *G = nullptr;
    STANCHK(stan_geometric_stiffness_device(ctx, K, d, &G));
    *out = G;
    return STAN_OK;
}

int stan_hip_geometric_stiffness_hex8(stan_ctx *ctx, stan_matrix *K, int64_t n_nodes, const double *xyz, const double *disp,
                                      const int32_t *node_dof, int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                                      const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                      const int32_t *red, stan_matrix **out) {
    STANCHK(kg_args(ctx, "geometric_stiffness_hex8", K, out,
                    !xyz || !disp || !node_dof || !red || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
                        n_dof != n_nodes * 3 || (n_elem > 0 && (!conn || !elem_mat || !elem_type))));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .disp = disp,
                      .node_dof = node_dof, .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red,
                      .mat_E_nu = mat_E_nu};
    // the checks of stan_hip_internal_forces_hex8, with the element named (the device repeats them for the _dev entry)
    STANCHK(mesh_range_check(ctx, "geometric_stiffness_hex8", true, true, m));
    host_stage st(ctx);
    mesh_dbufs bufs;
    STANCHK(bufs.upload(st, m));
    stan_matrix *G = nullptr;
    // (a refusal of the driver is synchronised too: the uploads are stream-ordered with the kernels)
    const int rc = st.finish(stan_geometric_stiffness_device(ctx, K, bufs.dev, &G));
    if (rc == STAN_OK) *out = G;
    else if (G) stan_hip_matrix_free(G);
    return rc;
}

}  // extern "C"
