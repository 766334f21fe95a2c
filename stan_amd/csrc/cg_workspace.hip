// cg_workspace.hip -- the context's CG vectors (stan_cg_ws, internal.h) and the moves the placement search makes with
// them (placement.hip).  Launches no kernel.
#include "internal.h"

// Vectors of the CG for a matrix of K's sizes, owned by the context (see stan_cg_ws).
int stan_cg_workspace(stan_ctx *ctx, const stan_matrix *K) {
    const int64_t ng = gather_len(K);
    const int64_t n3 = 3 * K->nloc > 0 ? 3 * K->nloc : 1;
    stan_cg_ws &ws = ctx->ws;
    if (ws.p && ws.ng >= ng && ws.n3 >= n3 && ws.ng <= ng + ng / 2 + 64) return STAN_OK;
    stan_cg_workspace_free(ctx);
    for (int i = 0; i < stan_cg_ws::NVEC; i++) STANCHK(stan_dmalloc(ctx, ws.vec(i).q, (size_t)(ws.vec(i).gather ? (ng > 0 ? ng : 1) : n3)));
    ws.ng = ng; ws.n3 = n3;
    return STAN_OK;
}
void stan_cg_workspace_free(stan_ctx *ctx) {
    stan_cg_ws &ws = ctx->ws;
    if (ws.vw_owner) {   // v, w carved out of one block (placement.hip, second stage): plain device memory, not the pool's
        stan_dfree(ctx, ws.vw_owner);
        ws.vw_owner = ws.v = ws.w = nullptr;
        ctx->prof_placement_moved_vectors = 0;   // the next matrix of another size searches afresh
    }
    for (int i = 0; i < stan_cg_ws::NVEC; i++) {
        double **q = ws.vec(i).q;
        if (*q) stan_dfree(ctx, *q);
        *q = nullptr;
    }
    ws.ng = ws.n3 = 0;
}

// Last resort of the placement search (placement.hip): no value candidate was clear of the vectors'
// group, and all of them are still allocated -- so NEW vectors, allocated now, lie beyond them.
// They are taken straight from the driver (a parked pool block would be the old memory again); the
// caller probes with them and keeps them (commit) or not.
int stan_cg_workspace_move(stan_ctx *ctx, const stan_matrix *K, bool commit, stan_cg_ws *saved) {
    stan_cg_ws &ws = ctx->ws;
    if (saved && !commit && saved->p == nullptr) {          // step 1: swap fresh vectors in, keep the old ones in *saved
        if (!ws.p) return STAN_OK;
        *saved = ws;
        stan_cg_ws nw;   // (nw.vw_owner stays null: eight blocks of their own)
        nw.ng = ws.ng; nw.n3 = ws.n3;
        bool ok = true;
        for (int i = 0; i < stan_cg_ws::NVEC && ok; i++)
            ok = hipMalloc((void **)nw.vec(i).q, (size_t)(nw.vec(i).gather ? (nw.ng > 0 ? nw.ng : 1) : nw.n3) * 8) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (int i = 0; i < stan_cg_ws::NVEC; i++) if (*nw.vec(i).q) hipFree(*nw.vec(i).q);
            saved->p = nullptr;
            return STAN_OK;   // no memory for it: keep what we have
        }
        ws = nw;
        (void)K;
        return STAN_OK;
    }
    if (!saved || saved->p == nullptr) return STAN_OK;
    // step 2: keep the new vectors (release the old ones for real) or go back to the old ones
    stan_cg_ws &drop = commit ? *saved : ws;
    stan_cg_ws keep = commit ? ws : *saved;
    if (drop.vw_owner) { ctx->pool.live.erase((void *)drop.vw_owner); hipFree(drop.vw_owner); drop.vw_owner = drop.v = drop.w = nullptr; }
    for (int i = 0; i < stan_cg_ws::NVEC; i++) {
        double *q = *drop.vec(i).q;
        if (!q) continue;
        ctx->pool.live.erase((void *)q);
        hipFree(q);
    }
    ws = keep;
    if (commit && ctx->pool.enabled)   // the new blocks are pooled-class blocks from now on (a carved v, w pair is not: its owner is plain memory)
        for (int i = 0; i < stan_cg_ws::NVEC; i++) {
            double **q = ws.vec(i).q;
            const size_t bytes = (size_t)(ws.vec(i).gather ? ws.ng : ws.n3) * 8;
            const bool carved = ws.vw_owner && (q == &ws.v || q == &ws.w);
            if (*q && !carved && bytes >= stan_pool::MIN_BYTES) ctx->pool.live[(void *)*q] = bytes;
        }
    saved->p = nullptr;
    return STAN_OK;
}

// Round 4 (tools/lab/spmv_steps_lab.cpp, profiles/r04/spmv_steps/): what makes a pairing slow is the vector the product
// WRITES lying in the memory group of the values it reads -- the gather vector's place does not matter.  So the cheap move is
// the two product buffers v and w alone, CARVED out of a block the caller has placed (a fresh small allocation would land in
// whatever hole the allocator finds, not behind the caller's spacers).  set: v, w point into `block` (saved[] takes the old
// v, w, owner) or, with block == nullptr, back to saved[]; adopt: the carved pair stays, `block` becomes its owner and the
// saved pair is released.
static int64_t vw_stride(const stan_cg_ws &ws) { return ((ws.n3 > 0 ? ws.n3 : 1) + 511) & ~(int64_t)511; }
size_t stan_cg_products_bytes(const stan_ctx *ctx) { return (size_t)(2 * vw_stride(ctx->ws)) * 8; }
void stan_cg_products_set(stan_ctx *ctx, double *block, double *saved[3]) {
    stan_cg_ws &ws = ctx->ws;
    if (block) {
        saved[0] = ws.v; saved[1] = ws.w; saved[2] = ws.vw_owner;
        ws.v = block; ws.w = block + vw_stride(ws);
    } else {
        ws.v = saved[0]; ws.w = saved[1]; ws.vw_owner = saved[2];
    }
}
void stan_cg_products_adopt(stan_ctx *ctx, double *block, size_t bytes, double *saved[3]) {
    stan_cg_ws &ws = ctx->ws;
    if (saved[2]) { ctx->pool.live.erase((void *)saved[2]); hipFree(saved[2]); }
    else for (int i = 0; i < 2; i++) if (saved[i]) { ctx->pool.live.erase((void *)saved[i]); hipFree(saved[i]); }
    ws.v = block; ws.w = block + vw_stride(ws); ws.vw_owner = block;
    // NOT a pooled block: 1-4 GB that hold 2 x n3 doubles would sit in the pool for the context's life once
    // the workspace is re-sized, matching no later request; stan_cg_workspace_free gives it straight back to the driver
    (void)bytes;
    saved[0] = saved[1] = saved[2] = nullptr;
}
