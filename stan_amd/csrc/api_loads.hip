// api_loads.hip -- the extern "C" surface, part 4 of 5: the load vectors of body forces, face pressures, prescribed displacements
// and temperature changes, and the thermal stress correction (loads.hip).  One device, one rank (one_device_refused).
#include "api_stage.h"

namespace {
// the host arrays of the thermal stress pass (m: host view with conn, elem_mat, elem_type) go to the device; d_stress is there
// already, or null: then `stress` goes up and comes back corrected
int thermal_stress_host(stan_ctx *ctx, const stan_mesh &m, const double *dT, const double *mat_alpha, double *stress, double *d_stress) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dt, ds; mesh_dbufs bufs;   // (released: elem_type, elem_mat, conn, stress, dT)
    STANCHK(dt.upload(st, dT, (size_t)m.n_nodes));
    STANCHK(bufs.upload(st, m));
    if (!d_stress) {
        STANCHK(ds.upload(st, stress, (size_t)m.n_elem * 48, stress));
        d_stress = ds.p;
    }
    return st.finish(stan_thermal_stress_device(ctx, bufs.dev, dt.p, mat_alpha, d_stress), ds);
}
}  // namespace

extern "C" {

int stan_hip_load_vector_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const int32_t *d_node_dof,
                                  int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                  const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                  const int32_t *d_red, const double *mat_body, int64_t n_faces,
                                  const int32_t *d_face_elem, const uint8_t *d_face_id, const double *d_face_pressure,
                                  const double *d_disp0, double *d_F, double *d_F_solve, double *d_load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "load_vector_hex8"));
    if (!d_xyz || !d_node_dof || !d_red || !mat_E_nu || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type)) ||
        (n_faces > 0 && (!d_face_elem || !d_face_id || !d_face_pressure))) {
        ctx->err = "load_vector_hex8_dev: null argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    return stan_load_vector_device(ctx, d, mat_body, n_faces, d_face_elem, d_face_id, d_face_pressure, d_disp0, d_F, d_F_solve,
                                   d_load_full, (stan_load_sums *)sums);
}

int stan_hip_load_vector_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const int32_t *node_dof, int64_t n_elem,
                              const int32_t *conn, const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat,
                              const double *mat_E_nu, int64_t n_dof, const int32_t *red, const double *mat_body,
                              int64_t n_faces, const int32_t *face_elem, const uint8_t *face_id, const double *face_pressure,
                              const double *disp0, double *F, double *F_solve, double *load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "load_vector_hex8"));
    if (!xyz || !node_dof || !red || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 || n_dof != n_nodes * 3 || n_faces < 0 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type)) || (n_faces > 0 && (!face_elem || !face_id || !face_pressure))) {
        ctx->err = "load_vector_hex8: null or empty argument, or n_dof != 3 n_nodes";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .node_dof = node_dof,
                      .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red, .mat_E_nu = mat_E_nu};
    // the length of F is fixed by the reduction map alone; every other integer is checked on the device (loads.hip)
    const size_t N = (size_t)(n_dof - count_fixed(m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> dp, dF, dFs, dl; dbuf<int32_t> dfe; dbuf<uint8_t> dfi;
    STANCHK(bufs.upload(st, m));
    if (n_faces > 0) {
        STANCHK(dfe.upload(st, face_elem, (size_t)n_faces));
        STANCHK(dfi.upload(st, face_id, (size_t)n_faces));
        STANCHK(dp.upload(st, face_pressure, (size_t)n_faces));
    }
    if (disp0) STANCHK(bufs.disp.upload(st, disp0, (size_t)n_nodes * 3));   // (behind the face lists: the order of the blocks)
    STANCHK(dF.inout(st, F, N));
    STANCHK(dFs.out(st, F_solve, N));
    STANCHK(dl.out(st, load_full, (size_t)n_dof));
    const int rc = stan_load_vector_device(ctx, bufs.dev, mat_body, n_faces, dfe.p, dfi.p, dp.p, bufs.disp.p, dF.p, dFs.p, dl.p,
                                           (stan_load_sums *)sums);
    return st.finish(rc, dF, dFs, dl);
}

int stan_hip_load_vector_times(stan_ctx *ctx, double ms[3]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "load_vector_times");
    for (int k = 0; k < 3; k++) ms[k] = ctx->prof_loads_ms[k];
    return STAN_OK;
}

// Thermal loads: the load vector of a nodal temperature change, and the stress correction.
int stan_hip_thermal_load_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const int32_t *d_node_dof,
                                   int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                   const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                   const int32_t *d_red, const double *mat_alpha, const double *d_dT, double *d_F,
                                   double *d_load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "thermal_load_hex8"));
    if (!d_xyz || !d_node_dof || !d_red || !mat_E_nu || !mat_alpha || !d_dT || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type))) {
        ctx->err = "thermal_load_hex8_dev: null argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    return stan_thermal_load_device(ctx, d, mat_alpha, d_dT, d_F, d_load_full, (stan_thermal_sums *)sums);
}

int stan_hip_thermal_load_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const int32_t *node_dof, int64_t n_elem,
                               const int32_t *conn, const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat,
                               const double *mat_E_nu, int64_t n_dof, const int32_t *red, const double *mat_alpha,
                               const double *dT, double *F, double *load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "thermal_load_hex8"));
    if (!xyz || !node_dof || !red || !mat_E_nu || !mat_alpha || !dT || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        n_dof != n_nodes * 3 || (n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        ctx->err = "thermal_load_hex8: null or empty argument, or n_dof != 3 n_nodes";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .node_dof = node_dof,
                      .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red, .mat_E_nu = mat_E_nu};
    // the length of F is fixed by the reduction map alone; every other integer is checked on the device (loads.hip)
    const size_t N = (size_t)(n_dof - count_fixed(m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> dt, dF, dl;
    STANCHK(bufs.upload(st, m));
    STANCHK(dt.upload(st, dT, (size_t)n_nodes));
    STANCHK(dF.inout(st, F, N));
    STANCHK(dl.out(st, load_full, (size_t)n_dof));
    return st.finish(stan_thermal_load_device(ctx, bufs.dev, mat_alpha, dt.p, dF.p, dl.p, (stan_thermal_sums *)sums), dF, dl);
}

int stan_hip_thermal_load_times(stan_ctx *ctx, double ms[3]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "thermal_load_times");
    for (int k = 0; k < 3; k++) ms[k] = ctx->prof_thermal_ms[k];
    return STAN_OK;
}

// Lumped mass: the body term with b = rho, per node and at the free DOFs.
int stan_hip_lumped_mass_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const int32_t *d_node_dof,
                                  int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                  const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                  const int32_t *d_red, const double *mat_rho, double *d_M, double *d_mass_node, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "lumped_mass_hex8"));
    if (!d_xyz || !d_node_dof || !d_red || !mat_E_nu || !mat_rho || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type))) {
        ctx->err = "lumped_mass_hex8_dev: null argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    return stan_lumped_mass_device(ctx, d, mat_rho, d_M, d_mass_node, (stan_mass_sums *)sums);
}

int stan_hip_lumped_mass_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const int32_t *node_dof, int64_t n_elem,
                              const int32_t *conn, const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat,
                              const double *mat_E_nu, int64_t n_dof, const int32_t *red, const double *mat_rho, double *M,
                              double *mass_node, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "lumped_mass_hex8"));
    if (!xyz || !node_dof || !red || !mat_E_nu || !mat_rho || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 || n_dof != n_nodes * 3 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        ctx->err = "lumped_mass_hex8: null or empty argument, or n_dof != 3 n_nodes";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .node_dof = node_dof,
                      .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red, .mat_E_nu = mat_E_nu};
    // the length of M is fixed by the reduction map alone; every other integer is checked on the device (loads.hip)
    const size_t N = (size_t)(n_dof - count_fixed(m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> dM, dn;
    STANCHK(bufs.upload(st, m));
    STANCHK(dM.out(st, M, N));
    STANCHK(dn.out(st, mass_node, (size_t)n_nodes));
    return st.finish(stan_lumped_mass_device(ctx, bufs.dev, mat_rho, dM.p, dn.p, (stan_mass_sums *)sums), dM, dn);
}

int stan_hip_thermal_stress_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_dT, int64_t n_elem, const int32_t *d_conn,
                                     const int32_t *d_elem_mat, const uint8_t *d_elem_type, int32_t n_mat,
                                     const double *mat_E_nu, const double *mat_alpha, double *d_stress) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "thermal_stress_hex8"));
    if (!d_dT || !mat_E_nu || !mat_alpha || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type || !d_stress))) {
        ctx->err = "thermal_stress_hex8_dev: null argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_mat = n_mat, .conn = d_conn, .elem_mat = d_elem_mat,
                      .elem_type = d_elem_type, .mat_E_nu = mat_E_nu};
    return stan_thermal_stress_device(ctx, d, d_dT, mat_alpha, d_stress);
}

int stan_hip_thermal_stress_hex8(stan_ctx *ctx, int64_t n_nodes, const double *dT, int64_t n_elem, const int32_t *conn,
                                 const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu,
                                 const double *mat_alpha, double *stress) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "thermal_stress_hex8"));
    if (!dT || !mat_E_nu || !mat_alpha || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type || !stress))) {
        ctx->err = "thermal_stress_hex8: null or empty argument";
        return STAN_E_ARG;
    }
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_mat = n_mat, .conn = conn, .elem_mat = elem_mat,
                      .elem_type = elem_type, .mat_E_nu = mat_E_nu};
    return thermal_stress_host(ctx, m, dT, mat_alpha, stress, nullptr);
}

int stan_hip_results_thermal_stress(stan_ctx *ctx, stan_results *res, int64_t n_nodes, const double *dT, const int32_t *conn,
                                    const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu,
                                    const double *mat_alpha) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "results_thermal_stress"));
    if (!res || !dT || !mat_E_nu || !mat_alpha || n_nodes <= 0 || n_mat <= 0 || (res->n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        ctx->err = "results_thermal_stress: null or empty argument";
        return STAN_E_ARG;
    }
    STANCHK(results_whole_check(ctx, "results_thermal_stress", res));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = res->n_elem, .n_mat = n_mat, .conn = conn, .elem_mat = elem_mat,
                      .elem_type = elem_type, .mat_E_nu = mat_E_nu};
    return thermal_stress_host(ctx, m, dT, mat_alpha, nullptr, res->parts[0].d_stress);
}

}  // extern "C"
