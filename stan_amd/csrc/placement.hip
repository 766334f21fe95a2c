// placement.hip -- where a big device block lands physically decides how fast it streams.
//
// Measured on MI355X (tools/placement_probe*.py, profiles/r02/PLACEMENT.md): the SAME SpMV over the
// SAME 6.4 GB matrix takes 1.02 ms from one hipMalloc'ed block and 1.15 ms from the next one, steadily,
// for the life of the block; moving the data inside a block (offsets of 256 B ... 4 MB) changes nothing,
// and asking for a physically contiguous block (hipExtMallocWithFlags, hipDeviceMallocContiguous) does
// not remove the lottery either, nor does rounding the sizes to 2 MB (all tried with lab hooks that are
// no longer in the tree).  For a given sequence of allocations the outcome repeats from process to
// process: it is a property of the addresses the allocator hands out -- more precisely (round 2) of the
// PAIR (value block, vector blocks): the sweep is ~8 % slower exactly when the matrix stream and the
// vectors it gathers from / writes to lie in the same group of device memory.  The column array's
// placement does not matter (eight fresh copies of cols under one value array: 1.112-1.121 ms).
// So the value stream of K is allocated by SEARCH (stan_dmalloc_streamed below; ON by default:
// STAN_OPT_PLACEMENT_TRIES = 16 candidates at most, bench.py asks for 32, 1 = plain allocation): the
// SpMV itself is timed on each candidate (the column indices exist by then; the values are whatever
// the block holds, only the addresses matter) with the context's own vectors and with vectors carved
// out of the candidate; the first candidate that is 3 % faster than its own reference is kept.
// Candidates that are not clear stay allocated while the search goes on, within a BYTE BUDGET
// (STAN_OPT_PLACEMENT_MAX_BYTES, default a quarter of the free device memory when the search starts)
// and above a free-memory floor of four block sizes.  (A plain front-to-back read of the block,
// k_probe below, tells the bad blocks from the rest but does not rank the rest:
// tools/placement_probe3.py.)  Costs ~10 ms per candidate once per context and size -- the block pool
// keeps the chosen block for the following assemblies.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "internal.h"

namespace {

constexpr int64_t PROBE_RUN = 15552;  // doubles per wavefront run = 27 slots x 9 x 64 (124 416 B)

__global__ void __launch_bounds__(256)
k_probe(const double *__restrict__ p, int64_t n, double *sink) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t b0 = wave * PROBE_RUN;
    if (b0 >= n) return;
    const int64_t b1 = b0 + PROBE_RUN < n ? b0 + PROBE_RUN : n;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int64_t i = b0 + lane;
    for (; i + 192 < b1; i += 256) {
        a0 += __builtin_nontemporal_load(p + i);
        a1 += __builtin_nontemporal_load(p + i + 64);
        a2 += __builtin_nontemporal_load(p + i + 128);
        a3 += __builtin_nontemporal_load(p + i + 192);
    }
    for (; i < b1; i += 64) a0 += __builtin_nontemporal_load(p + i);
    const double s = (a0 + a1) + (a2 + a3);
    if (s == 0.1234567890123) sink[0] = s;  // keeps the loads alive; practically never taken
}

}  // namespace

// time of one front-to-back read of the block (median of 3 after 1 warm-up), in ms
int stan_probe_block(stan_ctx *ctx, const void *p, size_t bytes, float *ms_out) {
    const int64_t n = (int64_t)(bytes / 8);
    *ms_out = 0;
    if (n <= 0) return STAN_OK;
    const int64_t waves = (n + PROBE_RUN - 1) / PROBE_RUN;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    event_bag ev;
    float t[3] = {0, 0, 0};
    for (int r = 0; r < 4; r++) {
        hipEvent_t a = ev.make(), b = ev.make();
        hipEventRecord(a, ctx->stream);
        hipLaunchKernelGGL(k_probe, dim3(grid), dim3(256), 0, ctx->stream, (const double *)p, n,
                           (double *)(ctx->d_status + SS_AUX));
        hipEventRecord(b, ctx->stream);
        HIPCHK(ctx, hipEventSynchronize(b));
        if (r > 0) hipEventElapsedTime(&t[r - 1], a, b);
    }
    HIPCHK(ctx, hipGetLastError());
    const float lo = t[0] < t[1] ? t[0] : t[1], hi = t[0] < t[1] ? t[1] : t[0];
    *ms_out = t[2] < lo ? lo : (t[2] > hi ? hi : t[2]);
    return STAN_OK;
}

// Allocation by search for a block that will be streamed many times (see the header comment and
// profiles/r02/PLACEMENT.md).  Round 2 measurements: what a block streams in is a property of the
// PAIR (value block, vector blocks) for the life of both: the sweep takes ~4-8 % longer exactly
// when the two lie in the same group of device memory (groups: runs of tens of GB of consecutive
// allocations), whichever group that is; it does not depend on the walk order of the kernel, on
// the allocation size class or flags, on translation cost or on the moment.  So every candidate is
// timed twice: with the context's vectors (the pairing the solve will run) and with the vectors
// carved out of the candidate ITSELF (by construction the same-group pairing: the slow reference).
// A candidate whose real pairing is 3 % faster than its own reference is clear of the vectors'
// group and is taken at once -- usually the first or second; otherwise it STAYS allocated, so that
// the allocator has to move on to other memory, and the next one is tried, up to `tries`
// candidates, the byte budget of held candidates (ctx->placement_max_bytes; 0 = a quarter of the free
// memory at the start of the search) or a free-memory floor of four block sizes; then the fastest real
// pairing is kept.
// A hipMalloc of 6.4 GB takes 0.3 ms and a probe four launches: ~10 ms per candidate at 148^3,
// once per context and size (the pool keeps the winner).
int stan_dmalloc_streamed(stan_ctx *ctx, void **p, size_t bytes,
                          const std::function<int(const void *, float *, bool)> &probe, bool second_copy) {
    const int tries = ctx->placement_tries;
    const bool may_flush = !second_copy;
    if (tries <= 1 || bytes < ((size_t)256 << 20) || !probe) return stan_dmalloc_bytes(ctx, p, bytes, may_flush);
    // inside a peer-to-peer solve nothing may call hipFree (stan_ctx::defer_frees): no candidates to give back
    if (ctx->defer_frees) return stan_dmalloc_bytes(ctx, p, bytes, may_flush);
    // a parked block of the right size was chosen by an earlier search: take it
    for (const stan_pool::blk &b : ctx->pool.avail)
        if (b.cap >= bytes && b.cap <= bytes + bytes / 2) return stan_dmalloc_bytes(ctx, p, bytes, may_flush);
    const bool trace = getenv("STAN_PLACEMENT_TRACE") != nullptr;   // one line per probe on stderr
    std::vector<void *> cand;
    std::vector<float> ms, tself;
    float worst = 0;
    bool clear = false;
    // this library lives inside a foreign host process: the candidates held during the search never
    // add up to more than the budget (the first candidate is always allowed: it is the allocation itself)
    size_t budget = (size_t)ctx->placement_max_bytes;
    {
        size_t free0 = 0, total0 = 0;
        if (budget == 0 && hipMemGetInfo(&free0, &total0) == hipSuccess) budget = free0 / 4;
    }
    // Round 6: WHICH clear candidate.  One box, five consecutive processes, every candidate timed (STAN_PLACEMENT_TRACE=all,
    // profiles/r06/placement_all_candidates_five_processes.txt): the 32 blocks an allocator hands out fall on LEVELS that repeat
    // from process to process -- 1.00 / 1.01-1.02 / 1.036 / 1.065 / 1.08-1.10 ms against self-paired references of 1.08-1.12 --
    // and "3 % faster than its own reference" also accepts the middle ones: the driver-command process of the end-of-round
    // session kept a 1.061-ms pairing (5 % clear) and solved at 1.040 ms per product where the process before it had got
    // 1.005 ms from its first candidate and solved at 1.010 (6.32 against 6.49 M DOF/s: the gap between the driver's lines of
    // rounds 2-5 and the builder's).  So: a candidate that is 7 % clear (the top levels) ends the search at once, as before; a
    // merely clear one is remembered and up to EXTRA more are timed for a better one; the fastest clear pairing is kept.
    // STAN_PLACEMENT_TRACE=all (diagnosis only): every candidate the bounds allow is timed and printed; =first: the rule of
    // rounds 2-5 (the first clear candidate ends the search), for A/B runs.
    const bool time_all = trace && strcmp(getenv("STAN_PLACEMENT_TRACE"), "all") == 0;
    const bool first_rule = trace && strcmp(getenv("STAN_PLACEMENT_TRACE"), "first") == 0;
    constexpr float CLEAR = 0.97f, TOP = 0.93f;
    constexpr int EXTRA = 8;
    int extra = 0;
    bool stop = false;
    for (int i = 0; i < tries && (!stop || time_all); i++) {
        size_t free_b = 0, total_b = 0;
        if (i > 0 && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 4 * bytes)) break;
        if (i > 0 && budget > 0 && (cand.size() + 1) * bytes > budget) break;
        // (Groups come in runs of up to 150 GB of consecutive allocations: one box needed 24 candidates.
        // Longer strides -- spacers of 1, 2, 4 ... block sizes in front of the next candidate -- were
        // tried and dropped: a hipMalloc / hipFree of 50-200 GB takes seconds on this stack, 24 blocks
        // of 6.4 GB a quarter of a second.)
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        float t = 0, t_self = 0;
        int rc = probe(q, &t, false);
        if (rc == STAN_OK) rc = probe(q, &t_self, true);
        if (rc) { hipFree(q); for (void *c : cand) hipFree(c); return rc; }
        cand.push_back(q);
        ms.push_back(t);
        tself.push_back(t_self);
        if (trace) fprintf(stderr, "[stan placement] candidate %d at %p (%.2f GB): %.4f ms with the context's vectors, %.4f ms self-paired\n", i, q, bytes / 1e9, t, t_self);
        if (t_self > worst) worst = t_self;
        if (t > worst) worst = t;
        // (t_self == 0: the candidate is too small to hold its own reference)
        if (clear && !stop && ++extra >= EXTRA) stop = true;            // enough looked at behind a merely clear one
        if (t_self > 0 && t <= CLEAR * t_self) {
            clear = true;
            if (t <= TOP * t_self || first_rule) stop = true;
        }
    }
    if (cand.empty()) return stan_dmalloc_bytes(ctx, p, bytes, may_flush);  // reports the allocation failure
    size_t ibest = 0;   // the fastest real pairing: among the clear ones if there is one (a pairing that is fast but not clear of
    bool have = false;  // its own reference has a fast reference too: nothing the vectors' place would change)
    for (size_t i = 0; i < cand.size(); i++) {
        const bool clear_i = tself[i] > 0 && ms[i] <= CLEAR * tself[i];
        if (clear && !clear_i) continue;
        if (!have || ms[i] < ms[ibest]) { ibest = i; have = true; }
    }
    // A second copy of a matrix's values (second_copy) takes the best candidate and leaves the vectors alone: they were
    // placed for the fp64 values, which the first and the refresh products of the same loop go on streaming, and moving
    // them for this block would undo that pairing unchecked.  prof_placement_moved_vectors keeps describing the vectors.
    if (!second_copy) ctx->prof_placement_moved_vectors = 0;
    if (!second_copy && !clear && cand.size() >= 2) {
        // Every candidate shares the vectors' group and they are all still allocated: vectors
        // allocated NOW lie beyond them.  Move the vectors instead of the values, if that pairing
        // is clear of the chosen candidate's own reference.
        stan_cg_ws saved;
        float t_new = 0, t_self = 0;
        int rc = stan_cg_workspace_move(ctx, nullptr, false, &saved);
        if (rc == STAN_OK && saved.p) {
            rc = probe(cand[ibest], &t_new, false);
            if (rc == STAN_OK) rc = probe(cand[ibest], &t_self, true);
            const bool better = rc == STAN_OK && t_self > 0 && t_new <= 0.97f * t_self && t_new < ms[ibest];
            stan_cg_workspace_move(ctx, nullptr, better, &saved);
            if (better) { ms[ibest] = t_new; ctx->prof_placement_moved_vectors = 1; }
        }
    }
    for (size_t i = 0; i < cand.size(); i++)
        if (i != ibest) hipFree(cand[i]);
    // Second stage (round 4).  The pairing is slow when the vectors the product WRITES (v, w) share a group with the values;
    // where the gather vector lies does not matter (tools/lab/spmv_steps_lab.cpp `sweep`: 1.004 or 1.127 ms by the place of
    // y alone; at 400^3 20.1 or 21.1-21.3 ms; boxes with three and four levels exist).  So, when the first stage found nothing
    // clear -- a block too large to have rivals has had no search at all (400^3: 125 GB) -- blocks of
    // free / 48 (1-4 GB) are allocated one after the other and held, the real pairing is timed with v and w carved out of the
    // front of each, and the best place is kept if it beats the pairing so far by 1 % and the candidate's self-paired
    // reference by 3 %.  (v and w are carved, not re-allocated: a fresh small allocation goes into whatever hole the
    // allocator knows -- seen: the same address behind every held block -- and the chosen block is kept as it is.)
    // ~5 ms per block at 148^3, once per context and size.  STAN_PLACEMENT_TRACE=1 prints every probe; =sweep keeps nothing.
    const bool sweep = trace && strcmp(getenv("STAN_PLACEMENT_TRACE"), "sweep") == 0;
    const bool force2 = trace && strcmp(getenv("STAN_PLACEMENT_TRACE"), "stage2") == 0;   // tests: enter, and adopt the best block whatever it gains
    // Only when the first stage did not end on a clear pairing.  (A thorough form -- the first stage going on until a pairing
    // is 7 % clear, this stage always walking its blocks -- found probes of 1.00-1.02 ms where the ordinary search keeps
    // 1.02-1.03, and the solves ran no faster: 1.020-1.043 ms per product in the CG against 1.021-1.027, four runs each on
    // one box.  With the probe timing launches back to back, twelve alternating runs each: five more candidates after the
    // first clear one change nothing (1.032-1.035 ms either way; the 1.00 ms pairings of a box come with the process, not with
    // the search); this stage walking its blocks after every search, keeping nothing, makes the solve 1 % SLOWER (1.013-1.016
    // against 1.004-1.007 ms: what is allocated afterwards lands elsewhere) -- profiles/r04/placement/extra_candidates_and_always_stage2_ab.txt.)
    if (!second_copy && (sweep || force2 || (!clear && !ctx->prof_placement_moved_vectors)) && tself[ibest] > 0 && ctx->ws.v && ctx->ws.w) {
        std::vector<void *> blocks;
        std::vector<float> tb;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const size_t vw = stan_cg_products_bytes(ctx);
        size_t sp_bytes = free_b / 48;
        if (sp_bytes < ((size_t)1 << 30)) sp_bytes = (size_t)1 << 30;
        if (sp_bytes > ((size_t)4 << 30)) sp_bytes = (size_t)4 << 30;
        if (sp_bytes < vw) sp_bytes = vw;
        const float bar = 0.97f * tself[ibest] < 0.99f * ms[ibest] ? 0.97f * tself[ibest] : 0.99f * ms[ibest];
        double *saved[3];
        int rc = STAN_OK;
        for (int i = 0; i < 40 && i < 2 * tries; i++) {
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < sp_bytes + 2 * vw + total_b / 16) break;
            if (budget > 0 && (blocks.size() + 1) * sp_bytes > budget) break;
            void *q = nullptr;
            if (hipMalloc(&q, sp_bytes) != hipSuccess) { (void)hipGetLastError(); break; }
            float t_new = 0;
            stan_cg_products_set(ctx, (double *)q, saved);
            rc = probe(cand[ibest], &t_new, false);
            stan_cg_products_set(ctx, nullptr, saved);
            if (trace) fprintf(stderr, "[stan placement] stage 2, block %d (%.2f GB at %p): v, w inside -> %.4f ms (so far %.4f, reference %.4f)\n", i, sp_bytes / 1e9, q, t_new, ms[ibest], tself[ibest]);
            blocks.push_back(q);
            tb.push_back(rc == STAN_OK ? t_new : 1e30f);
            if (rc) break;
        }
        size_t jb = 0;
        for (size_t j = 1; j < blocks.size(); j++) if (tb[j] < tb[jb]) jb = j;
        const bool take = !sweep && rc == STAN_OK && !blocks.empty() && (tb[jb] <= bar || force2);
        if (take) {
            // The pair stays in the block it was timed in (1-4 GB for 2 x 79 MB at 148^3).  Giving the block back and
            // taking a right-sized one -- even one that comes back at the same ADDRESS -- gets other physical memory: seen
            // 1.0023 ms in the probe and 1.033 / 1.112 ms afterwards.
            stan_cg_products_set(ctx, (double *)blocks[jb], saved);
            stan_cg_products_adopt(ctx, (double *)blocks[jb], sp_bytes, saved);
            if (trace) fprintf(stderr, "[stan placement] stage 2: block %zu chosen: %.4f ms\n", jb, tb[jb]);
            ms[ibest] = tb[jb];
            ctx->prof_placement_moved_vectors = 2;
        }
        for (size_t j = 0; j < blocks.size(); j++) if (!take || j != jb) hipFree(blocks[j]);
    }
    *p = cand[ibest];
    if (ctx->pool.enabled) ctx->pool.live[*p] = bytes;
    ctx->prof_placement_ms_best = ms[ibest];
    ctx->prof_placement_ms_worst = worst;
    ctx->prof_placement_candidates = (int)cand.size();
    return STAN_OK;
}
