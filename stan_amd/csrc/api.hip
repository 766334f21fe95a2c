// api.hip -- the extern "C" surface of libstan_hip.so declared in include/stan_hip.h, part 1 of 5: a context's life-cycle, options
// and reports.  (api_solve.hip, api_post.hip, api_loads.hip, api_modal.hip: the other parts; api_stage.h: what they share.)
#include <cstring>

#include "internal.h"

namespace {
thread_local std::string g_err;  // errors raised before a context exists
}  // namespace

void stan_set_global_error(const std::string &msg) { g_err = msg; }

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
    else if (option == STAN_OPT_CG_X_RING && value >= -1 && value <= 1) ctx->cg_x_ring = (int)value;
    else if (option == STAN_OPT_CG_REFRESH_60 && value >= -1 && value <= 1) ctx->cg_refresh_60 = (int)value;
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

int stan_hip_cg_loop_info(stan_ctx *ctx, int32_t *x_ring_window, int64_t *x_ring_flushes, int32_t *refresh_stream) {
    if (!ctx) return STAN_E_ARG;
    if (ctx->group) ctx = stan_group_rank0(ctx);
    if (x_ring_window) *x_ring_window = ctx->prof_x_ring_window;
    if (x_ring_flushes) *x_ring_flushes = ctx->prof_x_ring_flushes;
    if (refresh_stream) *refresh_stream = ctx->prof_refresh_stream;
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

}  // extern "C"
