// api_stage.h -- what the api*.hip files share: the staging of a host entry's arrays (host_stage, dbuf, mesh_dbufs), the host
// checks of a host view, the refusals several entries repeat, and the kept results.  Not part of the C ABI.
#pragma once

#include "internal.h"

// The stream side of one host entry.  Declared before the entry's device buffers (and behind any host memory of the entry's
// own that a copy reads or fills: it is drained before that memory goes).  Every copy from or to host memory goes through
// copy(), the straight path ends in finish() or sync(), and a return on any other path drains the stream here once a copy
// has been queued: the host arrays outlive their copies on EVERY way out.
struct host_stage {
    stan_ctx *ctx;
    bool queued = false;
    explicit host_stage(stan_ctx *c) : ctx(c) {}
    host_stage(const host_stage &) = delete; host_stage &operator=(const host_stage &) = delete;
    ~host_stage() { if (queued) (void)hipStreamSynchronize(ctx->stream); }
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        queued = true;
        HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
        return STAN_OK;
    }
    int sync() {   // the one synchronisation of the straight path
        queued = false;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return STAN_OK;
    }
    // the tail of an entry: rc is its driver's code; the downloads of `bufs` when that is STAN_OK, sync() either way
    template <typename... B>
    int finish(int rc, B &...bufs) {
        int e = STAN_OK;
        if (rc == STAN_OK) ((e = e == STAN_OK ? bufs.fetch() : e), ...);
        STANCHK(e);
        STANCHK(sync());
        return rc;
    }
};

template <typename T>
struct dbuf {  // RAII device buffer of a host entry: filled from host memory, fetched back to it, or both
    T *p = nullptr;
    host_stage *st = nullptr;
    T *back = nullptr;   // where fetch() copies the n entries to; null: nowhere
    size_t n = 0;
    ~dbuf() { if (st) stan_dfree(st->ctx, p); }
    int alloc(host_stage &s, size_t count, T *fetch_to = nullptr) {
        st = &s; n = count; back = fetch_to;
        return stan_dmalloc(s.ctx, &p, count);
    }
    int upload(host_stage &s, const T *h, size_t count, T *fetch_to = nullptr) {
        STANCHK(alloc(s, count, fetch_to));
        return count ? s.copy(p, h, count * sizeof(T), hipMemcpyHostToDevice) : (int)STAN_OK;
    }
    // an optional output / an optional array that goes up and comes back: nothing is allocated for a null `h`, p stays null
    int out(host_stage &s, T *h, size_t count) { return h ? alloc(s, count, h) : (int)STAN_OK; }
    int inout(host_stage &s, T *h, size_t count) { return h ? upload(s, h, count, h) : (int)STAN_OK; }
    int fetch() { return back && n ? st->copy(back, p, n * sizeof(T), hipMemcpyDeviceToHost) : (int)STAN_OK; }
};

// the device copies of a mesh's host arrays: upload() takes the host view and yields the device view `dev`; an array the
// entry does not have (a null pointer) is skipped and stays null.  The blocks are allocated in the order of upload()'s lines
// and given back in the reverse order of the members: elem_type, red, elem_mat, conn, node_dof, disp, xyz.
struct mesh_dbufs {
    dbuf<double> xyz, disp;
    dbuf<int32_t> node_dof, conn, elem_mat, red;
    dbuf<uint8_t> elem_type;
    stan_mesh dev;
    int upload(host_stage &s, const stan_mesh &h) {
        if (h.xyz) STANCHK(xyz.upload(s, h.xyz, (size_t)h.n_nodes * 3));
        if (h.disp) STANCHK(disp.upload(s, h.disp, (size_t)h.n_nodes * 3));
        if (h.node_dof) STANCHK(node_dof.upload(s, h.node_dof, (size_t)h.n_nodes * 3));
        if (h.conn) STANCHK(conn.upload(s, h.conn, (size_t)h.n_elem * 8));
        if (h.elem_mat) STANCHK(elem_mat.upload(s, h.elem_mat, (size_t)h.n_elem));
        if (h.elem_type) STANCHK(elem_type.upload(s, h.elem_type, (size_t)h.n_elem));
        if (h.red) STANCHK(red.upload(s, h.red, (size_t)h.n_dof));
        dev = h;   // the counts and mat_E_nu
        dev.xyz = xyz.p; dev.disp = disp.p; dev.node_dof = node_dof.p; dev.conn = conn.p;
        dev.elem_mat = elem_mat.p; dev.elem_type = elem_type.p; dev.red = red.p;
        return STAN_OK;
    }
};

// host range checks of a host view's integers, in element order: material, type (with_type), the 8 nodes; then node_dof when
// given.  "<who>: <what>", with " at element N" appended when at_element.
inline int mesh_range_check(stan_ctx *ctx, const char *who, bool at_element, bool with_type, const stan_mesh &m) {
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
inline int64_t count_fixed(const stan_mesh &m) {
    int64_t n_fixed = 0;
    for (int64_t k = 0; k < m.n_dof; k++) n_fixed += m.red[k] == -1;
    return n_fixed;
}

// One device, one rank (internal forces, load vectors, thermal loads): a node on a chunk boundary would have incidences on
// two devices.
inline int one_device_refused(stan_ctx *ctx, const char *entry) {
    STAN_NO_GROUP(ctx, std::string(entry) + " (a node on a chunk boundary has incidences on two devices)");
    if (stan_sharded(ctx)) {
        ctx->err = std::string(entry) + ": not available on a context with a communicator";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

// ---- what the drivers over the CG share (api_modal.hip, api_transient.hip) ------------------------------------------------------
// stream time of a driver's phases, by one event pair around each piece (profiling on; every piece ends synchronised)
struct piece_timer {
    stan_ctx *ctx;
    event_bag evs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit piece_timer(stan_ctx *c) : ctx(c) {
        if (ctx->profiling) { e0 = evs.make(); e1 = evs.make(); }
    }
    void begin() { if (e0) (void)hipEventRecord(e0, ctx->stream); }
    void end(double *acc) {
        if (!e0) return;
        float t = 0;
        (void)hipEventRecord(e1, ctx->stream);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) *acc += t;
    }
};

// the q x q eigenproblem of the block drivers, on the host (api_modal.hip): A Q = B Q Lambda, B = L L^T, cyclic Jacobi
bool stan_small_gen_eig(int q, const double *A, const double *B, double *lambda, double *Q, bool descending = false);

// One device, one rank (the modal and the buckling driver and their block helpers): the solves are the batched CG's (a
// single-rank context), the block kernels and their sums run on it
inline int block_driver_refused(stan_ctx *ctx, const char *entry) {
    STAN_NO_GROUP(ctx, std::string(entry) + " (the block solves and the block kernels run on one device)");
    if (stan_sharded(ctx)) {
        ctx->err = std::string(entry) + ": not available on a context with a communicator (the block sums are not reduced over ranks)";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

inline int worse_type(int a, int b) {   // negative < 5 < 7 < 1
    auto rank = [](int t) { return t < 0 ? 0 : t == 5 ? 1 : t == 7 ? 2 : 3; };
    if (a == 0) return b;
    return rank(b) < rank(a) || (rank(b) == rank(a) && b < a) ? b : a;
}

// ---- results kept on the device(s) (stan_hip_recover_hex8_keep, api_post.hip) ------------------------------------------------
struct stan_results {
    struct part { int device; int64_t e0, e1; double *d_strain, *d_stress; };
    std::vector<part> parts;
    int64_t n_elem = 0;
};

// an entry that works on the kept blocks in place needs them in one part, on its context's device
inline int results_whole_check(stan_ctx *ctx, const char *who, const stan_results *res) {
    if (res->parts.size() == 1 && res->parts[0].device == ctx->device && res->parts[0].e0 == 0 && res->parts[0].e1 == res->n_elem)
        return STAN_OK;
    ctx->err = std::string(who) + ": the results are not held, whole, on this context's device";
    return STAN_E_ARG;
}
