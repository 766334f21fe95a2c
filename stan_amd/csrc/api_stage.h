// api_stage.h -- what the api*.hip files share: the staging of a host entry's arrays (host_stage, dbuf, mesh_dbufs), the host
// checks of a host view, the refusals several entries repeat, and the kept results.  Not part of the C ABI.
#pragma once

#include <algorithm>
#include <cmath>

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

// ---- what the drivers over the CG share (api_modal.hip, api_transient.hip, api_buckling.hip) ------------------------------------
// the report as far as the call got, on every way out (to == null: nobody asked, or not yet)
template <typename Rep>
struct report_out {
    Rep *to; const Rep &from;
    ~report_out() { if (to) *to = from; }
};

// A driver's solves run with ALGLIB's merit stop off (its type 7 would leave a step or a correction unfinished); the caller's
// setting comes back on every way out
struct merit_off {
    stan_ctx *c; bool was;
    explicit merit_off(stan_ctx *x) : c(x), was(x->cg_merit_stop) { c->cg_merit_stop = false; }
    ~merit_off() { c->cg_merit_stop = was; }
};

// The load curve of the time integrators at x: piecewise linear through the n points (t ascending, g), constant before the first
// and after the last point; the segment is that of the LAST point with t <= x (a repeated t is a jump); no point: 1.  The
// expression of api_transient.hip's curve_at, which the explicit driver shares through this copy.
inline double stan_curve_at(int n, const double *t, const double *g, double x) {
    if (n == 0) return 1.0;
    if (x <= t[0]) return g[0];
    if (x >= t[n - 1]) return g[n - 1];
    const int i = (int)(std::upper_bound(t, t + n, x) - t) - 1;
    return g[i] + (g[i + 1] - g[i]) * ((x - t[i]) / (t[i + 1] - t[i]));
}

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

// What a run of a block driver carries (modes_device, buckling_device; Rep is stan_modes_report or stan_buckling_report, which
// name the shared fields alike) and the stages that are the same in both.  The loops themselves are the drivers': they differ
// in every line that matters (the pencil, the norm, the order, the stop test).
template <typename Rep>
struct block_run {
    stan_ctx *ctx; stan_matrix *K;
    const char *who;                  // the driver's name: the prefix of its error texts
    int64_t N; int32_t k; int q = 0;  // rows, pairs asked for, columns of the block
    double tol, solve_eps; int32_t max_outer, solve_max_its;
    Rep R{};
    report_out<Rep> report{nullptr, R};
    piece_timer pt;
    std::vector<int32_t> term, its, dcol;   // [q]: of the last solve; a column's place among the packed right-hand sides

    block_run(stan_ctx *c, stan_matrix *Km, const char *name, int32_t n_modes, double tol_, int32_t max_outer_, double solve_eps_,
              int32_t solve_max_its_)
        : ctx(c), K(Km), who(name), N(Km->n_red), k(n_modes), tol(tol_), solve_eps(solve_eps_), max_outer(max_outer_),
          solve_max_its(solve_max_its_), pt(c) {}
    int bad(const std::string &why, int rc) { ctx->err = std::string(who) + ": " + why; return rc; }
    // the argument checks, the block size and the defaults; from here on `rep` gets the report on every way out
    int begin(Rep *rep) {
        if (k <= 0 || k > N) return bad("n_modes must be in [1, N]", STAN_E_ARG);
        if (!(tol >= 0) || !(solve_eps >= 0) || !std::isfinite(tol) || !std::isfinite(solve_eps) || max_outer < 0 || solve_max_its < 0)
            return bad("tol, solve_eps, max_outer and solve_max_its must be >= 0", STAN_E_ARG);
        const int64_t q64 = std::min<int64_t>(N, std::min<int64_t>(2 * (int64_t)k, (int64_t)k + 8));
        if (q64 > STAN_MODAL_QMAX) return bad("the block of min(2 n_modes, n_modes + 8) columns exceeds 32", STAN_E_ARG);
        q = (int)q64;
        if (tol == 0) tol = 1e-6;
        if (max_outer == 0) max_outer = 100;
        if (solve_eps == 0 && solve_max_its == 0) solve_eps = 1e-6;   // lincgsetcond
        report.to = rep;
        R.block = q;
        term.resize((size_t)q); its.resize((size_t)q); dcol.resize((size_t)q);
        return STAN_OK;
    }
    // n columns of `F` -> `U` through the batched CG; a column that ends with -5 / -4 ends the call (hint: what the driver
    // says about a K that is not positive definite)
    int solve(int n, const double *F, double *U, const std::string &hint) {
        pt.begin();
        STANCHK(stan_cg_multi_device(ctx, K, n, F, solve_eps, solve_max_its, STAN_PREC_FP64, U, term.data(), its.data(), nullptr));
        pt.end(&R.solve_ms);
        for (int c = 0; c < n; c++) {
            R.cg_iterations += its[(size_t)c];
            R.cg_worst_type = worse_type(R.cg_worst_type, term[(size_t)c]);
        }
        if (R.cg_worst_type < 0)
            return bad("a CG column ended with termination type " + std::to_string(R.cg_worst_type) + " (K is not positive definite: " + hint + ")",
                       STAN_E_UNSUPPORTED);
        return STAN_OK;
    }
    // out_j = A in_j, q true products, and what `then` enqueues behind them, as one piece of product_ms
    template <typename Then>
    int products(stan_matrix *A, const double *in, double *out, Then &&then) {
        pt.begin();
        for (int j = 0; j < q; j++) STANCHK(stan_spmv_reduced(ctx, A, in + (size_t)j * N, out + (size_t)j * N));
        STANCHK(then());
        pt.end(&R.product_ms);
        return STAN_OK;
    }
    int products(stan_matrix *A, const double *in, double *out) {
        return products(A, in, out, [] { return (int)STAN_OK; });
    }
    // the right-hand sides of the columns j with again(j) packed side by side (a column's CG does not depend on its
    // neighbours): dcol[j] = the column's place, -1 for the others; *n = how many
    template <typename Again>
    int pack(double *rhs, Again &&again, int *n_out) {
        int n = 0;
        for (int j = 0; j < q; j++) {
            dcol[(size_t)j] = -1;
            if (!again(j)) continue;
            if (n != j) HIPCHK(ctx, hipMemcpyAsync(rhs + (size_t)n * N, rhs + (size_t)j * N, (size_t)N * 8, hipMemcpyDeviceToDevice, ctx->stream));
            dcol[(size_t)j] = n++;
        }
        *n_out = n;
        return STAN_OK;
    }
    // the tail: the block pieces' times folded, the two k-vectors out
    int finish(const double *values, const double *rho, double *d_values, double *d_rho) {
        hipStream_t st = ctx->stream;
        R.block_ms += R.gram_ms + R.rotate_ms;
        HIPCHK(ctx, hipMemcpyAsync(d_values, values, (size_t)k * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_rho, rho, (size_t)k * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return STAN_OK;
    }
};

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
