// api_mass.hip -- the extern "C" surface of the consistent mass: the element scalars on a batch
// (introspection), the assembled matrix M_c in K's layout (mass.hip) and A + sigma B on a common layout (matrix_shift.hip).
// One device, one rank.
#include <cmath>

#include "api_stage.h"

namespace {

int cm_args(stan_ctx *ctx, const char *who, stan_matrix *K, stan_matrix **out, bool null_arg) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, who));
    if (!K || !out || null_arg) { ctx->err = std::string(who) + ": null or empty argument"; return STAN_E_ARG; }
    if (K->ctx != ctx) { ctx->err = std::string(who) + ": K belongs to another context"; return STAN_E_ARG; }
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_mass_hex8_batch(stan_ctx *ctx, int64_t n, const double *xyz8, double rho, double *m36) {
    if (!ctx || n < 0 || (n > 0 && (!xyz8 || !m36))) return STAN_E_ARG;
    if (ctx->group) return stan_group_rank0_call(ctx, [&](stan_ctx *c) { return stan_hip_mass_hex8_batch(c, n, xyz8, rho, m36); });
    if (!(rho > 0.0) || !std::isfinite(rho)) { ctx->err = "mass_hex8_batch: rho must be positive and finite"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dx, dm;
    STANCHK(dx.upload(st, xyz8, (size_t)n * 24));
    STANCHK(dm.alloc(st, (size_t)n * 36, m36));
    return st.finish(stan_mass_batch_device(ctx, n, dx.p, rho, dm.p), dm);
}

int stan_hip_consistent_mass_times(stan_ctx *ctx, double ms[5]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "consistent_mass_times");
    for (int k = 0; k < 4; k++) ms[k] = ctx->prof_cm_ms[k];
    ms[4] = ctx->prof_axpy_ms;
    return STAN_OK;
}

int stan_hip_consistent_mass_hex8_dev(stan_ctx *ctx, stan_matrix *K, int64_t n_nodes, const double *d_xyz, const double *mat_rho,
                                      const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                      const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                      const int32_t *d_red, stan_matrix **out) {
    STANCHK(cm_args(ctx, "consistent_mass_hex8", K, out,
                    !d_xyz || !d_node_dof || !d_red || !mat_E_nu || !mat_rho || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type))));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz, .node_dof = d_node_dof,
                      .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red, .mat_E_nu = mat_E_nu};
    stan_matrix *M = nullptr;
    STANCHK(stan_consistent_mass_device(ctx, K, d, mat_rho, &M));
    *out = M;
    return STAN_OK;
}

int stan_hip_consistent_mass_hex8(stan_ctx *ctx, stan_matrix *K, int64_t n_nodes, const double *xyz, const double *mat_rho,
                                  const int32_t *node_dof, int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                                  const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof, const int32_t *red,
                                  stan_matrix **out) {
    STANCHK(cm_args(ctx, "consistent_mass_hex8", K, out,
                    !xyz || !node_dof || !red || !mat_E_nu || !mat_rho || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
                        n_dof != n_nodes * 3 || (n_elem > 0 && (!conn || !elem_mat || !elem_type))));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .node_dof = node_dof,
                      .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red, .mat_E_nu = mat_E_nu};
    // the checks of stan_hip_geometric_stiffness_hex8, with the element named (the device repeats them for the _dev entry)
    STANCHK(mesh_range_check(ctx, "consistent_mass_hex8", true, true, m));
    host_stage st(ctx);
    mesh_dbufs bufs;
    STANCHK(bufs.upload(st, m));
    stan_matrix *M = nullptr;
    const int rc = st.finish(stan_consistent_mass_device(ctx, K, bufs.dev, mat_rho, &M));
    if (rc == STAN_OK) *out = M;
    else if (M) stan_hip_matrix_free(M);
    return rc;
}

int stan_hip_matrix_axpy(stan_ctx *ctx, stan_matrix *A, double sigma, stan_matrix *B, stan_matrix **out) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "matrix_axpy"));
    if (!A || !B || !out) { ctx->err = "matrix_axpy: null argument"; return STAN_E_ARG; }
    if (A->ctx != ctx || B->ctx != ctx) { ctx->err = "matrix_axpy: A or B belongs to another context"; return STAN_E_ARG; }
    if (!std::isfinite(sigma)) { ctx->err = "matrix_axpy: sigma must be finite"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    stan_matrix *S = nullptr;
    ctx->prof_axpy_ms = 0;
    STANCHK(stan_matrix_axpy_device(ctx, A, sigma, B, &S, &ctx->prof_axpy_ms));
    *out = S;
    return STAN_OK;
}

}  // extern "C"
