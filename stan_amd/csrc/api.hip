// api.hip -- the extern "C" surface of libstan_hip.so declared in include/stan_hip.h.
#include <cstring>

#include "internal.h"


namespace {
thread_local std::string g_err;  // errors raised before a context exists

template <typename T>
struct dbuf {  // RAII device buffer filled from host memory
    T *p = nullptr;
    stan_ctx *owner = nullptr;
    ~dbuf() { stan_dfree(owner, p); }
    int upload(stan_ctx *ctx, const T *h, size_t n) {
        owner = ctx;
        STANCHK(stan_dmalloc(ctx, &p, n));
        if (n) HIPCHK(ctx, hipMemcpyAsync(p, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return STAN_OK;
    }
    int alloc(stan_ctx *ctx, size_t n) { owner = ctx; return stan_dmalloc(ctx, &p, n); }
};

// the device copies of a mesh's host arrays: upload() takes the host view and yields the device view `dev`; an array the
// entry does not have (a null pointer) is skipped and stays null.  The blocks are allocated in the order of upload()'s lines
// and given back in the reverse order of the members: elem_type, red, elem_mat, conn, node_dof, disp, xyz.
struct mesh_dbufs {
    dbuf<double> xyz, disp;
    dbuf<int32_t> node_dof, conn, elem_mat, red;
    dbuf<uint8_t> elem_type;
    stan_mesh dev;
    int upload(stan_ctx *ctx, const stan_mesh &h) {
        if (h.xyz) STANCHK(xyz.upload(ctx, h.xyz, (size_t)h.n_nodes * 3));
        if (h.disp) STANCHK(disp.upload(ctx, h.disp, (size_t)h.n_nodes * 3));
        if (h.node_dof) STANCHK(node_dof.upload(ctx, h.node_dof, (size_t)h.n_nodes * 3));
        if (h.conn) STANCHK(conn.upload(ctx, h.conn, (size_t)h.n_elem * 8));
        if (h.elem_mat) STANCHK(elem_mat.upload(ctx, h.elem_mat, (size_t)h.n_elem));
        if (h.elem_type) STANCHK(elem_type.upload(ctx, h.elem_type, (size_t)h.n_elem));
        if (h.red) STANCHK(red.upload(ctx, h.red, (size_t)h.n_dof));
        dev = h;   // the counts and mat_E_nu
        dev.xyz = xyz.p; dev.disp = disp.p; dev.node_dof = node_dof.p; dev.conn = conn.p;
        dev.elem_mat = elem_mat.p; dev.elem_type = elem_type.p; dev.red = red.p;
        return STAN_OK;
    }
};

// host range checks of a host view's integers, in element order: material, type (with_type), the 8 nodes; then node_dof when
// given.  "<who>: <what>", with " at element N" appended when at_element.
int mesh_range_check(stan_ctx *ctx, const char *who, bool at_element, bool with_type, const stan_mesh &m) {
    auto bad = [&](const char *why, int64_t e, int rc) {
        ctx->err = std::string(who) + ": " + why + (at_element && e >= 0 ? " at element " + std::to_string(e) : std::string());
        return rc;
    };
    for (int64_t e = 0; e < m.n_elem; e++) {
        if (m.elem_mat[e] < 0 || m.elem_mat[e] >= m.n_mat) return bad("elem_mat out of range", e, STAN_E_ARG);
        if (with_type && m.elem_type[e] != STAN_HEX8_G1 && m.elem_type[e] != STAN_HEX8_G2) return bad("unsupported element type", e, STAN_E_ARG);
        for (int a = 0; a < 8; a++)
            if (m.conn[e * 8 + a] < 0 || m.conn[e * 8 + a] >= m.n_nodes) return bad("node index out of range", e, STAN_E_ARG);
    }
    if (m.node_dof)
        for (int64_t k = 0; k < m.n_dof; k++)
            if (m.node_dof[k] < 0 || m.node_dof[k] >= m.n_dof) return bad("DOF out of range", -1, STAN_E_DOF_LAYOUT);
    return STAN_OK;
}

// the fixed DOFs of a reduction map: the reduced vectors (F, U) have n_dof minus this many entries
int64_t count_fixed(const stan_mesh &m) {
    int64_t n_fixed = 0;
    for (int64_t k = 0; k < m.n_dof; k++) n_fixed += m.red[k] == -1;
    return n_fixed;
}

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

void stan_set_global_error(const std::string &msg) { g_err = msg; }

// ---- the host entries of one context, behind the argument checks of the public entries (a group's ranks start here) ----
int stan_assemble_host(stan_ctx *ctx, const stan_mesh &whole, stan_matrix **outK) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (not mesh_range_check: a foreign element type is STAN_E_UNSUPPORTED here, the connectivity is left to the pick or the device)
    auto bad = [&](const char *why, int64_t e, int rc) { ctx->err = std::string("assemble_hex8: ") + why + " at element " + std::to_string(e); return rc; };
    for (int64_t e = 0; e < whole.n_elem; e++) {
        if (whole.elem_mat[e] < 0 || whole.elem_mat[e] >= whole.n_mat) return bad("elem_mat out of range", e, STAN_E_ARG);
        if (whole.elem_type[e] != STAN_HEX8_G1 && whole.elem_type[e] != STAN_HEX8_G2) return bad("unsupported element type", e, STAN_E_UNSUPPORTED);
    }
    shard_pick pick;
    const bool shard = ctx->nranks > 1 && whole.n_elem > 0;
    if (shard) STANCHK(pick_shard_elements(ctx, whole, &pick));
    mesh_dbufs bufs;
    STANCHK(bufs.upload(ctx, shard ? pick.mesh : whole));
    const int rc = stan_assemble_device(ctx, bufs.dev, outK);
    if (rc == STAN_OK) (*outK)->n_elem_scanned = bufs.dev.n_elem;
    if (rc == STAN_E_DETJ && shard && ctx->bad_elem >= 0 && ctx->bad_elem < (int64_t)pick.elems.size()) {
        ctx->bad_elem = pick.elems[(size_t)ctx->bad_elem];   // element number of the whole model
        ctx->err = "det J == 0 in element " + std::to_string(ctx->bad_elem) + " (MatrixST.Inverse would throw)";
    }
    // the uploads above are stream-ordered with the assembly; the host vectors must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

int stan_recover_host(stan_ctx *ctx, const stan_mesh &m, double *strain, double *stress) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    STANCHK(mesh_range_check(ctx, "recover_hex8", false, false, m));
    mesh_dbufs bufs; dbuf<double> de, ds;
    STANCHK(bufs.upload(ctx, m));
    STANCHK(de.alloc(ctx, (size_t)m.n_elem * 48));
    STANCHK(ds.alloc(ctx, (size_t)m.n_elem * 48));
    STANCHK(stan_recover_device(ctx, bufs.dev, de.p, ds.p));
    if (m.n_elem) {
        HIPCHK(ctx, hipMemcpyAsync(strain, de.p, (size_t)m.n_elem * 48 * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(stress, ds.p, (size_t)m.n_elem * 48 * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}

extern "C" {

int stan_hip_init(int device, stan_ctx **out) {
    if (!out) return STAN_E_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || device < 0 || device >= n) {
        g_err = std::string("stan_hip_init: no usable HIP device (") +
                (e != hipSuccess ? hipGetErrorString(e) : "device ordinal out of range") + ")";
        return STAN_E_HIP;
    }
    stan_ctx *c = new stan_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&c->h_status, 64 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&c->d_status, 64 * sizeof(int64_t)) != hipSuccess) {
        g_err = "stan_hip_init: stream / status allocation failed";
        delete c;
        return STAN_E_HIP;
    }
    c->own_stream = true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) c->pool.max_bytes = total_b / 2;
    *out = c;
    return STAN_OK;
}

void stan_hip_destroy(stan_ctx *ctx) {
    if (!ctx) return;
    if (ctx->group) { stan_group_destroy(ctx); return; }
    hipSetDevice(ctx->device);
    if (ctx->p2p && ctx->p2p->ipc) stan_p2p_ipc_release(ctx);   // (a group's resources belong to the group)
    {
        void *comm = nullptr;
        { std::lock_guard<std::mutex> lk(ctx->comm_mu); comm = ctx->comm; ctx->comm = nullptr; }
        if (comm && ctx->nccl.CommDestroy) ctx->nccl.CommDestroy(comm);
    }
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->side) hipStreamDestroy(ctx->side);
    if (ctx->ev_a) hipEventDestroy(ctx->ev_a);
    if (ctx->ev_b) hipEventDestroy(ctx->ev_b);
    // matrices that outlive their context keep working memory-wise: they are detached and their
    // buffers go straight back to the driver when they are freed
    for (stan_matrix *K : ctx->matrices) K->ctx = nullptr;
    stan_cg_workspace_free(ctx);
    ctx->pool.flush();
    if (ctx->h_status) hipHostFree(ctx->h_status);
    if (ctx->d_status) hipFree(ctx->d_status);
    delete ctx;
}

const char *stan_hip_last_error(stan_ctx *ctx) {
    if (ctx && ctx->group) return stan_group_last_error(ctx);
    return ctx ? ctx->err.c_str() : g_err.c_str();
}
int64_t stan_hip_last_bad_element(stan_ctx *ctx) { return ctx ? ctx->bad_elem : -1; }

int stan_hip_set_stream(stan_ctx *ctx, void *hip_stream) {
    if (!ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "set_stream");
    hipSetDevice(ctx->device);
    // parked blocks of the pool are reused in stream order: drain the old stream before switching
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    ctx->own_stream = false;
    ctx->stream = (hipStream_t)hip_stream;
    if (!hip_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    }
    return STAN_OK;
}

int stan_hip_set_option(stan_ctx *ctx, int32_t option, int64_t value) {
    if (!ctx) return STAN_E_ARG;
    if (ctx->group && option == STAN_OPT_COMM_P2P) return stan_group_set_p2p(ctx, value != 0);
    if (ctx->group)
        return stan_group_ctx_call(ctx, [&](stan_ctx *c) { return stan_hip_set_option(c, option, value); });
    if (option == STAN_OPT_COMM_P2P) {
        // one process per GPU: the ranks map each other's mailboxes, counters and vectors through HIP IPC; the
        // handles travel over the communicator, so EVERY rank must make this call (it is a collective)
        if (value != 0) {
            if (ctx->nranks < 2 || !ctx->comm) { ctx->err = "STAN_OPT_COMM_P2P: needs a communicator of several ranks (stan_hip_comm_init) or a handle of stan_hip_init_multi"; return STAN_E_UNSUPPORTED; }
            HIPCHK(ctx, hipSetDevice(ctx->device));
            STANCHK(stan_p2p_ipc_setup(ctx));
        }
        ctx->comm_p2p = value != 0 && ctx->p2p != nullptr;
        return STAN_OK;
    }
    if (option == STAN_OPT_CG_MERIT_STOP) ctx->cg_merit_stop = value != 0;
    else if (option == STAN_OPT_CG_RUPDATE && value >= 0 && value < (1 << 30)) ctx->cg_rupdate = (int)value;
    else if (option == STAN_OPT_ASSEMBLY_MODE && (value == 0 || value == 1)) ctx->assembly_mode = (int)value;
    else if (option == STAN_OPT_CG_FUSED_REFRESH) ctx->cg_fused_refresh = value != 0;
    else if (option == STAN_OPT_CG_SINGLE_REDUCE) ctx->cg_single_reduce = value != 0;
    else if (option == STAN_OPT_CG_FOLD_REDUCE) ctx->cg_fold_reduce = value != 0;
    else if (option == STAN_OPT_CG_REFINE && value >= 0 && value <= 2) ctx->cg_refine = (int)value;
    else if (option == STAN_OPT_CG_LAZY_SCALING) ctx->cg_lazy_scaling = value != 0;
    else if (option == STAN_OPT_VEC_STORE_NT && value >= 0 && value <= 3) ctx->vec_store_nt = (int)value;
    else if (option == STAN_OPT_PACKED_COLUMNS) ctx->cols16 = value != 0;
    else if (option == STAN_OPT_CG_DEFER_X) ctx->cg_defer_x = value != 0;
    else if (option == STAN_OPT_SPMV_SMALL && value >= 0) ctx->spmv_small_rows = value == 1 ? 150000 : value;
    else if (option == STAN_OPT_POOL) {
        ctx->pool.enabled = value != 0;
        if (!ctx->pool.enabled) {
            hipSetDevice(ctx->device);
            hipStreamSynchronize(ctx->stream);
            ctx->pool.flush();
        }
    }
    else if (option == STAN_OPT_POOL_MAX_BYTES && value >= -1) {
        hipSetDevice(ctx->device);
        if (value == -1) {   // "this process owns the device": nine tenths of what is free now
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); ctx->err = "set_option: hipMemGetInfo failed"; return STAN_E_HIP; }
            value = (int64_t)(free_b - free_b / 10 + ctx->pool.bytes_avail);   // (parked blocks are not "free" to the driver)
        }
        ctx->pool.max_bytes = (size_t)value;
        hipStreamSynchronize(ctx->stream);  // parked blocks may still be in use by queued work
        while (!ctx->pool.avail.empty() && ctx->pool.bytes_avail > ctx->pool.max_bytes) {
            hipFree(ctx->pool.avail.front().p);
            ctx->pool.bytes_avail -= ctx->pool.avail.front().cap;
            ctx->pool.avail.erase(ctx->pool.avail.begin());
        }
    }
    else if (option == STAN_OPT_VALUE_STREAM_60 && value >= -1 && value <= 1) ctx->value_stream_60 = (int)value;
    else if (option == STAN_OPT_OVERLAP_HALO) ctx->overlap_halo = value != 0;
    else if (option == STAN_OPT_SELL_SIGMA && value >= 1 && value <= 32) ctx->sell_sigma = (int)value;
    else if (option == STAN_OPT_PLACEMENT_TRIES && value >= 1 && value <= 64) ctx->placement_tries = (int)value;
    else if (option == STAN_OPT_PLACEMENT_MAX_BYTES && value >= 0) ctx->placement_max_bytes = value;
    else if (option == STAN_OPT_ROW_FOLDING && value >= -1 && value <= 1) ctx->row_folding = (int)value;
    else if (option == STAN_OPT_SPMV_VARIANT && (value == -1 || value == 0 || value == 9 || value == 12 || value == 20))
        ctx->spmv_variant = (int)value;
    else { ctx->err = "set_option: unknown option or bad value"; return STAN_E_ARG; }
    return STAN_OK;
}

int stan_hip_pool_info(stan_ctx *ctx, int64_t *bytes_parked, int64_t *blocks_parked) {
    if (!ctx) return STAN_E_ARG;
    if (ctx->group) ctx = stan_group_rank0(ctx);
    if (bytes_parked) *bytes_parked = (int64_t)ctx->pool.bytes_avail;
    if (blocks_parked) *blocks_parked = (int64_t)ctx->pool.avail.size();
    return STAN_OK;
}

// which transport the sharded CG of this context will use (bench.py prints it next to a multi-GPU line)
int stan_hip_comm_info(stan_ctx *ctx, int32_t *rccl_version, int32_t *comm_ranks, int32_t *comm_rank, int32_t *p2p) {
    if (!ctx) return STAN_E_ARG;
    stan_ctx *c = ctx->group ? stan_group_rank0(ctx) : ctx;
    int v = 0, n = 0, r = 0;
    stan_comm_info(c, &v, &n, &r);
    if (rccl_version) *rccl_version = v;
    if (comm_ranks) *comm_ranks = n;
    if (comm_rank) *comm_rank = r;
    if (p2p) *p2p = (c->p2p && c->comm_p2p) ? 1 : 0;
    return STAN_OK;
}

// which FILE the RCCL entry points of this context were resolved from (empty before comm_init)
int stan_hip_comm_library(stan_ctx *ctx, char *path, int64_t capacity, int32_t *reused) {
    if (!ctx || (capacity > 0 && !path) || capacity < 0) return STAN_E_ARG;
    stan_ctx *c = ctx->group ? stan_group_rank0(ctx) : ctx;
    std::string p;
    int r = 0;
    stan_comm_library(c, &p, &r);
    if (capacity > 0) {
        const size_t n = p.size() < (size_t)capacity - 1 ? p.size() : (size_t)capacity - 1;
        memcpy(path, p.data(), n);
        path[n] = 0;
    }
    if (reused) *reused = r;
    return STAN_OK;
}

int stan_hip_set_profiling(stan_ctx *ctx, int32_t enabled) {
    if (!ctx) return STAN_E_ARG;
    if (ctx->group)
        return stan_group_ctx_call(ctx, [&](stan_ctx *c) { return stan_hip_set_profiling(c, enabled); });
    ctx->profiling = enabled != 0;
    return STAN_OK;
}
int stan_hip_get_profile_rank(stan_ctx *ctx, int32_t rank, stan_profile *out) {
    if (!ctx || !out || rank < 0) return STAN_E_ARG;
    if (ctx->group) {
        if (rank >= stan_group_size(ctx)) return STAN_E_ARG;
        return stan_hip_get_profile(stan_group_rank(ctx, rank), out);
    }
    if (rank != 0) return STAN_E_ARG;
    return stan_hip_get_profile(ctx, out);
}
int stan_hip_device_info(stan_ctx *ctx, int32_t rank, int32_t *hip_ordinal, char bus_id[32]) {
    if (!ctx || rank < 0) return STAN_E_ARG;
    stan_ctx *c = ctx;
    if (ctx->group) {
        if (rank >= stan_group_size(ctx)) return STAN_E_ARG;
        c = stan_group_rank(ctx, rank);
    } else if (rank != 0) return STAN_E_ARG;
    if (hip_ordinal) *hip_ordinal = c->device;
    if (bus_id) {
        bus_id[0] = 0;
        if (hipDeviceGetPCIBusId(bus_id, 32, c->device) != hipSuccess) { (void)hipGetLastError(); bus_id[0] = 0; }
    }
    return STAN_OK;
}
int stan_hip_get_profile(stan_ctx *ctx, stan_profile *out) {
    if (!ctx || !out) return STAN_E_ARG;
    if (ctx->group) ctx = stan_group_rank0(ctx);   // rank 0's timings; spmv_bytes is that shard's
    *out = ctx->prof;
    out->assembly_colours = ctx->prof_colours;
    out->placement_candidates = ctx->prof_placement_candidates;
    out->placement_ms_best = ctx->prof_placement_ms_best;
    out->placement_ms_worst = ctx->prof_placement_ms_worst;
    out->placement_moved_vectors = ctx->prof_placement_moved_vectors;
    return STAN_OK;
}

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
    dbuf<double> dF, dU;
    if (ctx->result_segment && ctx->nranks > 1) {
        // a rank of a one-process group: only ITS entries [u0, u1) of F go up and of U come down -- the ranks
        // share the caller's buffers (disjoint ranges), nothing is gathered on the devices (multi.hip)
        const size_t u0 = (size_t)K->u0, nu = (size_t)(K->u1 - K->u0);
        STANCHK(dF.alloc(ctx, N ? N : 1));
        STANCHK(dU.alloc(ctx, N ? N : 1));
        if (nu) HIPCHK(ctx, hipMemcpyAsync(dF.p + u0, F + u0, nu * 8, hipMemcpyHostToDevice, ctx->stream));
        STANCHK(stan_cg_device(ctx, K, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type,
                               iterations, rel_residual));
        if (nu) HIPCHK(ctx, hipMemcpyAsync(U + u0, dU.p + u0, nu * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return STAN_OK;
    }
    STANCHK(dF.upload(ctx, F, N));
    STANCHK(dU.alloc(ctx, N));
    HIPCHK(ctx, hipMemsetAsync(dU.p, 0, (N ? N : 1) * 8, ctx->stream));
    STANCHK(stan_cg_device(ctx, K, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type,
                           iterations, rel_residual));
    if (N) HIPCHK(ctx, hipMemcpyAsync(U, dU.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
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
    dbuf<double> dF, dU;
    STANCHK(dF.upload(ctx, F, n));
    STANCHK(dU.alloc(ctx, n));
    HIPCHK(ctx, hipMemsetAsync(dU.p, 0, (n ? n : 1) * 8, ctx->stream));
    STANCHK(stan_cg_multi_device(ctx, K, n_rhs, dF.p, eps_f, max_its, precision_mode, dU.p, termination_type, iterations,
                                 rel_residual));
    if (n) HIPCHK(ctx, hipMemcpyAsync(U, dU.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}

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

// ---- results kept on the device(s) (stan_hip_recover_hex8_keep) ------------------------------------------------------
}  // extern "C"
struct stan_results {
    struct part { int device; int64_t e0, e1; double *d_strain, *d_stress; };
    std::vector<part> parts;
    int64_t n_elem = 0;
};
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
    mesh_dbufs bufs;
    STANCHK(bufs.upload(ctx, m));
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
    if (rc == STAN_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = STAN_E_HIP;
    if (rc != STAN_OK) { hipFree(de); hipFree(ds); return rc; }
    *out = stan_results::part{ctx->device, e_base, e_base + m.n_elem, de, ds};
    return STAN_OK;
}
}  // namespace
extern "C" {

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

}  // extern "C"
namespace {
// Part.Load_Scalar (scalars.hip) with the strain / stress blocks already on the device: argument checks, the uploads of
// disp and conn, the downloads of the selected rows
int result_scalars(stan_ctx *ctx, const char *who, int64_t n_nodes, const double *disp, int64_t n_elem, const int32_t *conn,
                   const double *d_strain, const double *d_stress, int32_t n_sel, const int32_t *sel, double *point, double *cell) {
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
    STANCHK(du.upload(ctx, disp, (size_t)n_nodes * 3));
    STANCHK(dc.upload(ctx, conn, (size_t)n_elem * 8));
    const size_t np = (size_t)n_sel * (size_t)n_nodes, nc = (size_t)n_sel * 3 * (size_t)n_elem;
    if (point) STANCHK(dp.alloc(ctx, np));
    if (cell) STANCHK(dcell.alloc(ctx, nc));
    STANCHK(stan_scalars_device(ctx, n_nodes, du.p, n_elem, dc.p, d_strain, d_stress, n_sel, sel, point ? dp.p : nullptr,
                                cell ? dcell.p : nullptr));
    if (point) HIPCHK(ctx, hipMemcpyAsync(point, dp.p, np * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (cell && nc) HIPCHK(ctx, hipMemcpyAsync(cell, dcell.p, nc * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}
// Compute_NodalForces and the R assembly (recovery.hip) on one context, behind the entry's checks
int nodal_forces_host(stan_ctx *ctx, const stan_mesh &m, double *elem_forces, double *R) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    STANCHK(mesh_range_check(ctx, "nodal_forces_hex8", false, false, m));
    mesh_dbufs bufs; dbuf<double> df, dR;
    STANCHK(bufs.upload(ctx, m));
    if (elem_forces) STANCHK(df.alloc(ctx, (size_t)m.n_elem * 24));
    if (R) {
        STANCHK(dR.alloc(ctx, (size_t)m.n_dof));
        HIPCHK(ctx, hipMemsetAsync(dR.p, 0, (size_t)m.n_dof * 8, ctx->stream));
    }
    STANCHK(stan_recover_device(ctx, bufs.dev, nullptr, nullptr, elem_forces ? df.p : nullptr, R ? dR.p : nullptr));
    if (elem_forces && m.n_elem)
        HIPCHK(ctx, hipMemcpyAsync(elem_forces, df.p, (size_t)m.n_elem * 24 * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (R) HIPCHK(ctx, hipMemcpyAsync(R, dR.p, (size_t)m.n_dof * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}
}  // namespace
extern "C" {

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
    dbuf<double> de, ds;
    STANCHK(de.upload(ctx, strain, (size_t)n_elem * 48));
    STANCHK(ds.upload(ctx, stress, (size_t)n_elem * 48));
    return result_scalars(ctx, "result_scalars_hex8", n_nodes, disp, n_elem, conn, de.p, ds.p, n_sel, sel, point, cell);
}

int stan_hip_results_scalars(stan_ctx *ctx, stan_results *res, int64_t n_nodes, const double *disp, const int32_t *conn,
                             int32_t n_sel, const int32_t *sel, double *point, double *cell) {
    if (!ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "results_scalars (a node on a chunk boundary has incidences on two devices)");
    if (!res || !disp || !sel || n_nodes <= 0 || (!point && !cell) || (res->n_elem > 0 && !conn)) {
        ctx->err = "results_scalars: null or empty argument";
        return STAN_E_ARG;
    }
    if (res->parts.size() != 1 || res->parts[0].device != ctx->device || res->parts[0].e0 != 0 ||
        res->parts[0].e1 != res->n_elem) {
        ctx->err = "results_scalars: the results are not held, whole, on this context's device";
        return STAN_E_ARG;
    }
    return result_scalars(ctx, "results_scalars", n_nodes, disp, res->n_elem, conn, res->parts[0].d_strain,
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

// f_int = sum_e int B^T D B u_e dV, reactions and the equilibrium sums (internal_forces.hip).  One device, one rank: a node on
// a chunk boundary would have incidences on two devices.
static int internal_forces_refused(stan_ctx *ctx, const char *entry = "internal_forces_hex8") {
    STAN_NO_GROUP(ctx, std::string(entry) + " (a node on a chunk boundary has incidences on two devices)");
    if (stan_sharded(ctx)) {
        ctx->err = std::string(entry) + ": not available on a context with a communicator";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

int stan_hip_internal_forces_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const double *d_disp,
                                      const int32_t *d_node_dof, int64_t n_elem, const int32_t *d_conn,
                                      const int32_t *d_elem_mat, const uint8_t *d_elem_type, int32_t n_mat,
                                      const double *mat_E_nu, int64_t n_dof, const int32_t *d_red, const double *d_F,
                                      double *d_f_int, double *d_reaction, void *eq) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx));
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
    STANCHK(internal_forces_refused(ctx));
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
    mesh_dbufs bufs; dbuf<double> dF, dfi, dre;
    STANCHK(bufs.upload(ctx, m));
    if (F) STANCHK(dF.upload(ctx, F, N));
    if (f_int) STANCHK(dfi.alloc(ctx, (size_t)n_dof));
    if (reaction) STANCHK(dre.alloc(ctx, (size_t)n_dof));
    const int rc = stan_internal_forces_device(ctx, bufs.dev, F ? dF.p : nullptr, f_int ? dfi.p : nullptr, reaction ? dre.p : nullptr,
                                               (stan_equilibrium *)eq);
    if (rc == STAN_OK) {
        if (f_int) HIPCHK(ctx, hipMemcpyAsync(f_int, dfi.p, (size_t)n_dof * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (reaction) HIPCHK(ctx, hipMemcpyAsync(reaction, dre.p, (size_t)n_dof * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    // the uploads above are stream-ordered with the kernels; the host arrays must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

// The load vector of body forces, face pressures and prescribed displacements (loads.hip).  One device, one rank, for the
// reason the internal forces give.
int stan_hip_load_vector_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const int32_t *d_node_dof,
                                  int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                  const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                  const int32_t *d_red, const double *mat_body, int64_t n_faces,
                                  const int32_t *d_face_elem, const uint8_t *d_face_id, const double *d_face_pressure,
                                  const double *d_disp0, double *d_F, double *d_F_solve, double *d_load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx, "load_vector_hex8"));
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
    STANCHK(internal_forces_refused(ctx, "load_vector_hex8"));
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
    mesh_dbufs bufs; dbuf<double> dp, dF, dFs, dl; dbuf<int32_t> dfe; dbuf<uint8_t> dfi;
    STANCHK(bufs.upload(ctx, m));
    if (n_faces > 0) {
        STANCHK(dfe.upload(ctx, face_elem, (size_t)n_faces));
        STANCHK(dfi.upload(ctx, face_id, (size_t)n_faces));
        STANCHK(dp.upload(ctx, face_pressure, (size_t)n_faces));
    }
    if (disp0) STANCHK(bufs.disp.upload(ctx, disp0, (size_t)n_nodes * 3));   // (behind the face lists: the order of the blocks)
    if (F) STANCHK(dF.upload(ctx, F, N));
    if (F_solve) STANCHK(dFs.alloc(ctx, N));
    if (load_full) STANCHK(dl.alloc(ctx, (size_t)n_dof));
    const int rc = stan_load_vector_device(ctx, bufs.dev, mat_body, n_faces, dfe.p, dfi.p, dp.p, bufs.disp.p, F ? dF.p : nullptr,
                                           F_solve ? dFs.p : nullptr, load_full ? dl.p : nullptr, (stan_load_sums *)sums);
    if (rc == STAN_OK) {
        if (F && N) HIPCHK(ctx, hipMemcpyAsync(F, dF.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (F_solve && N) HIPCHK(ctx, hipMemcpyAsync(F_solve, dFs.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (load_full) HIPCHK(ctx, hipMemcpyAsync(load_full, dl.p, (size_t)n_dof * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    // the uploads above are stream-ordered with the kernels; the host arrays must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

int stan_hip_load_vector_times(stan_ctx *ctx, double ms[3]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "load_vector_times");
    for (int k = 0; k < 3; k++) ms[k] = ctx->prof_loads_ms[k];
    return STAN_OK;
}

// Thermal loads (loads.hip): the load vector of a nodal temperature change, and the stress correction.  One device, one rank,
// for the reason the internal forces give.
int stan_hip_thermal_load_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_xyz, const int32_t *d_node_dof,
                                   int64_t n_elem, const int32_t *d_conn, const int32_t *d_elem_mat,
                                   const uint8_t *d_elem_type, int32_t n_mat, const double *mat_E_nu, int64_t n_dof,
                                   const int32_t *d_red, const double *mat_alpha, const double *d_dT, double *d_F,
                                   double *d_load_full, void *sums) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx, "thermal_load_hex8"));
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
    STANCHK(internal_forces_refused(ctx, "thermal_load_hex8"));
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
    mesh_dbufs bufs; dbuf<double> dt, dF, dl;
    STANCHK(bufs.upload(ctx, m));
    STANCHK(dt.upload(ctx, dT, (size_t)n_nodes));
    if (F) STANCHK(dF.upload(ctx, F, N));
    if (load_full) STANCHK(dl.alloc(ctx, (size_t)n_dof));
    const int rc = stan_thermal_load_device(ctx, bufs.dev, mat_alpha, dt.p, F ? dF.p : nullptr, load_full ? dl.p : nullptr,
                                            (stan_thermal_sums *)sums);
    if (rc == STAN_OK) {
        if (F && N) HIPCHK(ctx, hipMemcpyAsync(F, dF.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (load_full) HIPCHK(ctx, hipMemcpyAsync(load_full, dl.p, (size_t)n_dof * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    // the uploads above are stream-ordered with the kernels; the host arrays must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}

int stan_hip_thermal_load_times(stan_ctx *ctx, double ms[3]) {
    if (!ctx || !ms) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "thermal_load_times");
    for (int k = 0; k < 3; k++) ms[k] = ctx->prof_thermal_ms[k];
    return STAN_OK;
}

int stan_hip_thermal_stress_hex8_dev(stan_ctx *ctx, int64_t n_nodes, const double *d_dT, int64_t n_elem, const int32_t *d_conn,
                                     const int32_t *d_elem_mat, const uint8_t *d_elem_type, int32_t n_mat,
                                     const double *mat_E_nu, const double *mat_alpha, double *d_stress) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx, "thermal_stress_hex8"));
    if (!d_dT || !mat_E_nu || !mat_alpha || (n_elem > 0 && (!d_conn || !d_elem_mat || !d_elem_type || !d_stress))) {
        ctx->err = "thermal_stress_hex8_dev: null argument";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stan_thermal_stress_device(ctx, n_nodes, d_dT, n_elem, d_conn, d_elem_mat, d_elem_type, n_mat, mat_E_nu, mat_alpha, d_stress);
}
}  // extern "C"
namespace {
// the host arrays of the thermal stress pass go to the device; d_stress is there already, or null: then `stress` goes up and
// comes back corrected
int thermal_stress_host(stan_ctx *ctx, int64_t n_nodes, const double *dT, int64_t n_elem, const int32_t *conn, const int32_t *elem_mat,
                        const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu, const double *mat_alpha, double *stress,
                        double *d_stress) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    dbuf<double> dt, ds; dbuf<int32_t> dc, dm; dbuf<uint8_t> dty;
    STANCHK(dt.upload(ctx, dT, (size_t)n_nodes));
    STANCHK(dc.upload(ctx, conn, (size_t)n_elem * 8));
    STANCHK(dm.upload(ctx, elem_mat, (size_t)n_elem));
    STANCHK(dty.upload(ctx, elem_type, (size_t)n_elem));
    if (!d_stress) {
        STANCHK(ds.upload(ctx, stress, (size_t)n_elem * 48));
        d_stress = ds.p;
    }
    const int rc = stan_thermal_stress_device(ctx, n_nodes, dt.p, n_elem, dc.p, dm.p, dty.p, n_mat, mat_E_nu, mat_alpha, d_stress);
    if (rc == STAN_OK && ds.p && n_elem)
        HIPCHK(ctx, hipMemcpyAsync(stress, ds.p, (size_t)n_elem * 48 * 8, hipMemcpyDeviceToHost, ctx->stream));
    // the uploads above are stream-ordered with the kernels; the host arrays must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return rc;
}
}  // namespace
extern "C" {

int stan_hip_thermal_stress_hex8(stan_ctx *ctx, int64_t n_nodes, const double *dT, int64_t n_elem, const int32_t *conn,
                                 const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu,
                                 const double *mat_alpha, double *stress) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx, "thermal_stress_hex8"));
    if (!dT || !mat_E_nu || !mat_alpha || n_nodes <= 0 || n_mat <= 0 || n_elem < 0 ||
        (n_elem > 0 && (!conn || !elem_mat || !elem_type || !stress))) {
        ctx->err = "thermal_stress_hex8: null or empty argument";
        return STAN_E_ARG;
    }
    return thermal_stress_host(ctx, n_nodes, dT, n_elem, conn, elem_mat, elem_type, n_mat, mat_E_nu, mat_alpha, stress, nullptr);
}

int stan_hip_results_thermal_stress(stan_ctx *ctx, stan_results *res, int64_t n_nodes, const double *dT, const int32_t *conn,
                                    const int32_t *elem_mat, const uint8_t *elem_type, int32_t n_mat, const double *mat_E_nu,
                                    const double *mat_alpha) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(internal_forces_refused(ctx, "results_thermal_stress"));
    if (!res || !dT || !mat_E_nu || !mat_alpha || n_nodes <= 0 || n_mat <= 0 || (res->n_elem > 0 && (!conn || !elem_mat || !elem_type))) {
        ctx->err = "results_thermal_stress: null or empty argument";
        return STAN_E_ARG;
    }
    if (res->parts.size() != 1 || res->parts[0].device != ctx->device || res->parts[0].e0 != 0 ||
        res->parts[0].e1 != res->n_elem) {
        ctx->err = "results_thermal_stress: the results are not held, whole, on this context's device";
        return STAN_E_ARG;
    }
    return thermal_stress_host(ctx, n_nodes, dT, res->n_elem, conn, elem_mat, elem_type, n_mat, mat_E_nu, mat_alpha, nullptr,
                               res->parts[0].d_stress);
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
    dbuf<double> dx, dk; dbuf<uint8_t> dt;
    STANCHK(dx.upload(ctx, xyz8, (size_t)n * 24));
    STANCHK(dt.upload(ctx, type, (size_t)n));
    STANCHK(dk.alloc(ctx, (size_t)n * 576));
    STANCHK(stan_ke_batch_device(ctx, n, dx.p, E, nu, dt.p, dk.p));
    if (n) HIPCHK(ctx, hipMemcpyAsync(out, dk.p, (size_t)n * 576 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
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
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(slot_ptr.data(), K->d_slot_ptr, slot_ptr.size() * 4, hipMemcpyDeviceToHost, st));
    if (!rowlen.empty()) HIPCHK(ctx, hipMemcpyAsync(rowlen.data(), K->d_rowlen, rowlen.size() * 4, hipMemcpyDeviceToHost, st));
    if (!posof.empty()) HIPCHK(ctx, hipMemcpyAsync(posof.data(), K->d_posof, posof.size() * 4, hipMemcpyDeviceToHost, st));
    if (!cols.empty()) HIPCHK(ctx, hipMemcpyAsync(cols.data(), K->d_cols, cols.size() * 4, hipMemcpyDeviceToHost, st));
    if (!vals.empty()) HIPCHK(ctx, hipMemcpyAsync(vals.data(), K->vals64(), vals.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(red.data(), K->d_red, red.size() * 4, hipMemcpyDeviceToHost, st));
    if (scaled && !scale.empty()) HIPCHK(ctx, hipMemcpyAsync(scale.data(), K->d_scale, scale.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
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
                            val[q] = scaled ? a / (scale[(size_t)d] * scale[(size_t)dc]) : a;
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
    dbuf<double> dx, dy;
    STANCHK(dx.upload(ctx, x, N));
    STANCHK(dy.alloc(ctx, N));
    STANCHK(stan_spmv_reduced(ctx, K, dx.p, dy.p));
    if (N) HIPCHK(ctx, hipMemcpyAsync(y, dy.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
}

int stan_hip_matrix_diagonal(stan_ctx *ctx, stan_matrix *K, double *diag) {
    if (!ctx || !K || !diag || K->ctx != ctx) return STAN_E_ARG;
    STAN_NO_GROUP(ctx, "matrix_diagonal");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red;
    dbuf<double> dd;
    STANCHK(dd.alloc(ctx, N ? N : 1));
    STANCHK(stan_matrix_diagonal(ctx, K, dd.p));
    if (N) HIPCHK(ctx, hipMemcpyAsync(diag, dd.p, N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return STAN_OK;
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
    dbuf<double> dx, dy;
    STANCHK(dx.alloc(ctx, (size_t)ng));
    STANCHK(dy.alloc(ctx, (size_t)(3 * npad + 3)));
    HIPCHK(ctx, hipMemsetAsync(dx.p, 0, (size_t)ng * 8, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dx.p, x_local, (size_t)(3 * (K->nloc + K->nhalo)) * 8, hipMemcpyHostToDevice, ctx->stream));
    STANCHK(stan_spmv_local(ctx, K, dx.p, dy.p));
    if (K->nloc) HIPCHK(ctx, hipMemcpy(y_owned, dy.p, (size_t)(3 * K->nloc) * 8, hipMemcpyDeviceToHost));
    return STAN_OK;
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
