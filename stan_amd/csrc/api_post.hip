// api_post.hip -- the extern "C" surface, part 3 of 5: stress recovery, results kept on the device(s), result scalars, nodal and
// internal forces.
#include "api_stage.h"

namespace {
// pinned staging of one host thread (stan_hip_results_map): grown on demand, released when the thread ends
struct map_stage {
    double *p = nullptr;
    size_t cap = 0;   // doubles
    ~map_stage() { if (p) hipHostFree(p); }
};
thread_local map_stage g_stage;
// m: the elements from e_base on of the whole model (a host view)
int recover_keep_one(stan_ctx *ctx, const stan_mesh &m, int64_t e_base, stan_results::part *out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    STANCHK(mesh_range_check(ctx, "recover_hex8", false, false, m));
    host_stage st(ctx);
    mesh_dbufs bufs;
    STANCHK(bufs.upload(st, m));
    // plain device memory, owned by the results object (it may outlive the context's pool)
    double *de = nullptr, *ds = nullptr;
    const size_t bytes = (size_t)(m.n_elem > 0 ? m.n_elem : 1) * 48 * 8;
    auto both = [&]() {
        if (hipMalloc((void **)&de, bytes) == hipSuccess && hipMalloc((void **)&ds, bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        if (de) hipFree(de);
        de = ds = nullptr;
        return false;
    };
    if (!both()) {
        // the context's pool may hold most of the device parked (stan_solver lets it: STAN_OPT_POOL_MAX_BYTES = -1) while K
        // and the CG's vectors are still live: give the parked blocks back -- what stan_dmalloc_bytes does for a pooled
        // request -- and try once more (400^3 keeps 49 GB of results)
        if (!ctx->pool.avail.empty() && hipStreamSynchronize(ctx->stream) == hipSuccess) {
            ctx->pool.flush();
            (void)both();
        }
        if (!de) {
            ctx->err = "recover_hex8_keep: device allocation of 2 x " + std::to_string(bytes) + " B failed";
            return STAN_E_ALLOC;
        }
    }
    int rc = stan_recover_device(ctx, bufs.dev, de, ds);
    if (rc == STAN_OK && st.sync() != STAN_OK) rc = STAN_E_HIP;
    if (rc != STAN_OK) { hipFree(de); hipFree(ds); return rc; }
    *out = stan_results::part{ctx->device, e_base, e_base + m.n_elem, de, ds};
    return STAN_OK;
}

// Part.Load_Scalar (scalars.hip) with the strain / stress blocks already on the device: argument checks, the uploads of
// disp and conn, the downloads of the selected rows.  `st`: the entry's, which may have uploaded the blocks through it.
int result_scalars(host_stage &st, const char *who, int64_t n_nodes, const double *disp, int64_t n_elem, const int32_t *conn,
                   const double *d_strain, const double *d_stress, int32_t n_sel, const int32_t *sel, double *point, double *cell) {
    stan_ctx *ctx = st.ctx;
    auto bad = [&](const char *why) { ctx->err = std::string(who) + ": " + why; return (int)STAN_E_ARG; };
    if (n_sel <= 0 || n_sel > STAN_SCALAR_COUNT) return bad("n_sel must be 1..24");
    uint32_t seen = 0;
    for (int32_t k = 0; k < n_sel; k++) {
        if (sel[k] < 0 || sel[k] >= STAN_SCALAR_COUNT) return bad("scalar index outside 0..23");
        if (seen & (1u << sel[k])) return bad("scalar index listed twice");
        seen |= 1u << sel[k];
    }
    if (n_elem >= (int64_t)1 << 28) return bad("more than 2^28 elements");
    for (int64_t t = 0; t < n_elem * 8; t++)
        if (conn[t] < 0 || conn[t] >= n_nodes) return bad("node index out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    dbuf<double> du, dp, dcell; dbuf<int32_t> dc;
    STANCHK(du.upload(st, disp, (size_t)n_nodes * 3));
    STANCHK(dc.upload(st, conn, (size_t)n_elem * 8));
    STANCHK(dp.out(st, point, (size_t)n_sel * (size_t)n_nodes));
    STANCHK(dcell.out(st, cell, (size_t)n_sel * 3 * (size_t)n_elem));
    STANCHK(stan_scalars_device(ctx, n_nodes, du.p, n_elem, dc.p, d_strain, d_stress, n_sel, sel, dp.p, dcell.p));
    return st.finish(STAN_OK, dp, dcell);
}

// Compute_NodalForces and the R assembly (recovery.hip) on one context, behind the entry's checks
int nodal_forces_host(stan_ctx *ctx, const stan_mesh &m, double *elem_forces, double *R) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    STANCHK(mesh_range_check(ctx, "nodal_forces_hex8", false, false, m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> df, dR;
    STANCHK(bufs.upload(st, m));
    STANCHK(df.out(st, elem_forces, (size_t)m.n_elem * 24));
    STANCHK(dR.out(st, R, (size_t)m.n_dof));
    if (R) HIPCHK(ctx, hipMemsetAsync(dR.p, 0, (size_t)m.n_dof * 8, ctx->stream));
    STANCHK(stan_recover_device(ctx, bufs.dev, nullptr, nullptr, df.p, dR.p));
    return st.finish(STAN_OK, df, dR);
}
}  // namespace

// the host entry of one context, behind the argument checks of the public entry (a group's ranks start here)
int stan_recover_host(stan_ctx *ctx, const stan_mesh &m, double *strain, double *stress) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    STANCHK(mesh_range_check(ctx, "recover_hex8", false, false, m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> de, ds;
    STANCHK(bufs.upload(st, m));
    STANCHK(de.alloc(st, (size_t)m.n_elem * 48, strain));
    STANCHK(ds.alloc(st, (size_t)m.n_elem * 48, stress));
    STANCHK(stan_recover_device(ctx, bufs.dev, de.p, ds.p));
    return st.finish(STAN_OK, de, ds);
}

extern "C" {

int stan_hip_recover_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz,
                              const double *d_disp, int64_t n_elem, const int32_t *d_conn,
                              const int32_t *d_elem_mat, const uint8_t *d_elem_type,
                              int32_t n_mat, const double *mat_E_nu, double *d_strain,
                              double *d_stress) {
    if (!ctx || !d_xyz || !d_disp || !mat_E_nu || n_mat <= 0 ||
        (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type || !d_strain || !d_stress)))
        return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "recover_hex8_dev (device pointers belong to one device)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_mat = n_mat, .xyz = d_xyz, .disp = d_disp, .conn = d_conn,
                      .elem_mat = d_elem_mat, .elem_type = d_elem_type, .mat_E_nu = mat_E_nu};
    return stan_recover_device(ctx, d, d_strain, d_stress);
}

int stan_hip_recover_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const double *disp,
                          int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                          const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu,
                          double *strain, double *stress) {
    if (!ctx || !xyz || !disp || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type || !strain || !stress)))
        return STAN_E_ARG;
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_mat = n_mat, .xyz = xyz, .disp = disp, .conn = conn,
                      .elem_mat = elem_mat, .elem_type = elem_type, .mat_E_nu = mat_E_nu};
    return ctx->group ? stan_group_recover(ctx, m, strain, stress) : stan_recover_host(ctx, m, strain, stress);
}

// ---- results kept on the device(s): struct stan_results of api_stage.h ------------------------------------------------------
int stan_hip_recover_hex8_keep(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const double *disp,
                               int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                               const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu, stan_results **out) {
    if (!ctx || !out || !xyz || !disp || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type)))
        return STAN_E_ARG;
    *out = nullptr;
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_mat = n_mat, .xyz = xyz, .disp = disp, .conn = conn,
                      .elem_mat = elem_mat, .elem_type = elem_type, .mat_E_nu = mat_E_nu};
    stan_results *res = new stan_results();
    res->n_elem = n_elem;
    int rc = STAN_OK;
    if (ctx->group) {
        const int n = stan_group_size(ctx);
        res->parts.assign((size_t)n, stan_results::part{0, 0, 0, nullptr, nullptr});
        rc = stan_group_ctx_call_ranked(ctx, [&](stan_ctx *c, int r) {
            const int64_t e0 = n_elem * r / n, e1 = n_elem * (r + 1) / n;
            res->parts[(size_t)r] = stan_results::part{c->device, e0, e0, nullptr, nullptr};
            if (e1 <= e0) return (int)STAN_OK;
            const int e = recover_keep_one(c, m.chunk(e0, e1), e0, &res->parts[(size_t)r]);
            stan_chunk_bad_element(ctx, c, e, e0);
            return e;
        });
    } else {
        res->parts.assign(1, stan_results::part{ctx->device, 0, 0, nullptr, nullptr});
        if (n_elem > 0) rc = recover_keep_one(ctx, m, 0, &res->parts[0]);
    }
    if (rc != STAN_OK) { stan_hip_results_free(res); return rc; }
    *out = res;
    return STAN_OK;
}

int stan_hip_results_map(stan_results *res, int64_t e0, int64_t e1, const double **strain, const double **stress) {
    if (!res || !strain || !stress || e0 < 0 || e1 < e0 || e1 > res->n_elem) return STAN_E_ARG;
    const size_t n = (size_t)(e1 - e0) * 48;
    map_stage &st = g_stage;
    if (st.cap < 2 * n) {
        if (st.p) hipHostFree(st.p);
        st.p = nullptr; st.cap = 0;
        const size_t want = 2 * n > (size_t)1 << 16 ? 2 * n : (size_t)1 << 16;
        if (hipHostMalloc((void **)&st.p, want * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); st.p = nullptr; return STAN_E_ALLOC; }
        st.cap = want;
    }
    for (const stan_results::part &pt : res->parts) {
        const int64_t a = e0 > pt.e0 ? e0 : pt.e0, b = e1 < pt.e1 ? e1 : pt.e1;
        if (b <= a) continue;
        if (hipSetDevice(pt.device) != hipSuccess) return STAN_E_HIP;
        const size_t off = (size_t)(a - e0) * 48, cnt = (size_t)(b - a) * 48 * 8;
        // blocking copies on the null stream of the calling thread: the kernel that produced the data was
        // synchronised by stan_hip_recover_hex8_keep, the library's own streams are non-blocking
        if (hipMemcpy(st.p + off, pt.d_strain + (size_t)(a - pt.e0) * 48, cnt, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(st.p + n + off, pt.d_stress + (size_t)(a - pt.e0) * 48, cnt, hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return STAN_E_HIP;
        }
    }
    *strain = st.p;
    *stress = st.p + n;
    return STAN_OK;
}

void stan_hip_results_free(stan_results *res) {
    if (!res) return;
    for (stan_results::part &pt : res->parts) {
        if (!pt.d_strain && !pt.d_stress) continue;
        hipSetDevice(pt.device);
        if (pt.d_strain) hipFree(pt.d_strain);
        if (pt.d_stress) hipFree(pt.d_stress);
    }
    delete res;
}

int stan_hip_result_scalars_hex8(stan_ctx *ctx, int64_t n_nodes, const double *disp, int64_t n_elem, const int32_t *conn,
                                 const double *strain, const double *stress, int32_t n_sel, const int32_t *sel,
                                 double *point, double *cell) {
    if (!ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "result_scalars_hex8 (a node on a chunk boundary has incidences on two devices)");
    if (!disp || !sel || n_nodes <= 0 || n_elem < 0 || (!point && !cell) || (n_elem > 0 && (!conn || !strain || !stress))) {
        ctx->err = "result_scalars_hex8: null or empty argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> de, ds;
    STANCHK(de.upload(st, strain, (size_t)n_elem * 48));
    STANCHK(ds.upload(st, stress, (size_t)n_elem * 48));
    return result_scalars(st, "result_scalars_hex8", n_nodes, disp, n_elem, conn, de.p, ds.p, n_sel, sel, point, cell);
}

int stan_hip_results_scalars(stan_ctx *ctx, stan_results *res, int64_t n_nodes, const double *disp, const int32_t *conn,
                             int32_t n_sel, const int32_t *sel, double *point, double *cell) {
    if (!ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "results_scalars (a node on a chunk boundary has incidences on two devices)");
    if (!res || !disp || !sel || n_nodes <= 0 || (!point && !cell) || (res->n_elem > 0 && !conn)) {
        ctx->err = "results_scalars: null or empty argument";
        return STAN_E_ARG;
    }
    STANCHK(results_whole_check(ctx, "results_scalars", res));
    host_stage st(ctx);
    return result_scalars(st, "results_scalars", n_nodes, disp, res->n_elem, conn, res->parts[0].d_strain,
                          res->parts[0].d_stress, n_sel, sel, point, cell);
}

int stan_hip_nodal_forces_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const double *disp,
                               const int32_t *node_dof, int64_t n_elem, const int32_t *conn,
                               const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat,
                               const double *mat_E_nu, int64_t n_dof, double *elem_forces, double *R) {
    if (!ctx || !xyz || !disp || !node_dof || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        n_dof != n_nodes * 3 || (!elem_forces && !R) || (n_elem > 0 && (!conn || !elem_mat || !elem_type)))
        return STAN_E_ARG;
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .disp = disp,
                      .node_dof = node_dof, .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .mat_E_nu = mat_E_nu};
    if (ctx->group)   // R is an all-element sum: one device (rank 0); its error text follows the handle
        return stan_group_rank0_call(ctx, [&](stan_ctx *c) { return nodal_forces_host(c, m, elem_forces, R); });
    return nodal_forces_host(ctx, m, elem_forces, R);
}

// f_int = sum_e int B^T D B u_e dV, reactions and the equilibrium sums (internal_forces.hip).  One device, one rank
// (one_device_refused).
int stan_hip_internal_forces_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const double *d_disp,
                                      const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn,
                                      const int32_t *d_elem_mat, const uint8_t *d_elem_type, int32_t n_mat,
                                      const double *mat_E_nu, int64_t n_dof, const int32_t *d_red, const double *d_F,
                                      double *d_f_int, double *d_reaction, void *eq) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "internal_forces_hex8"));
    if (!d_xyz || !d_disp || !d_node_dof || !d_red || !mat_E_nu || (!d_f_int && !d_reaction && !eq) ||
        (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type))) {
        ctx->err = "internal_forces_hex8_dev: null argument, or none of f_int / reaction / eq asked for";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh d{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = d_xyz, .disp = d_disp,
                      .node_dof = d_node_dof, .conn = d_conn, .elem_mat = d_elem_mat, .elem_type = d_elem_type, .red = d_red,
                      .mat_E_nu = mat_E_nu};
    return stan_internal_forces_device(ctx, d, d_F, d_f_int, d_reaction, (stan_equilibrium *)eq);
}

int stan_hip_internal_forces_hex8(stan_ctx *ctx, int64_t n_nodes, const double *xyz, const double *disp,
                                  const int32_t *node_dof, int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                                  const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                  const int32_t *red, const double *F, double *f_int, double *reaction, void *eq) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(one_device_refused(ctx, "internal_forces_hex8"));
    if (!xyz || !disp || !node_dof || !red || !mat_E_nu || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 || n_dof != n_nodes * 3 ||
        (!f_int && !reaction && !eq) || (n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        ctx->err = "internal_forces_hex8: null or empty argument, or none of f_int / reaction / eq asked for";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const stan_mesh m{.n_nodes = n_nodes, .n_elem = n_elem, .n_dof = n_dof, .n_mat = n_mat, .xyz = xyz, .disp = disp,
                      .node_dof = node_dof, .conn = conn, .elem_mat = elem_mat, .elem_type = elem_type, .red = red,
                      .mat_E_nu = mat_E_nu};
    // the checks of stan_hip_nodal_forces_hex8, with the element named (the device repeats them for the _dev entry)
    STANCHK(mesh_range_check(ctx, "internal_forces_hex8", true, true, m));
    const size_t N = (size_t)(n_dof - count_fixed(m));
    host_stage st(ctx);
    mesh_dbufs bufs; dbuf<double> dF, dfi, dre;
    STANCHK(bufs.upload(st, m));
    if (F) STANCHK(dF.upload(st, F, N));
    STANCHK(dfi.out(st, f_int, (size_t)n_dof));
    STANCHK(dre.out(st, reaction, (size_t)n_dof));
    // (a refusal of the driver is synchronised too: the uploads are stream-ordered with the kernels)
    return st.finish(stan_internal_forces_device(ctx, bufs.dev, dF.p, dfi.p, dre.p, (stan_equilibrium *)eq), dfi, dre);
}

}  // extern "C"
