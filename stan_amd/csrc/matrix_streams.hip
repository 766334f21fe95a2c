// matrix_streams.hip -- the copies of a matrix's streams the products may read instead of the assembled ones, made once per
// matrix: the fp32 and FIXED-48 value streams (STAN_PREC_MIXED, STAN_PREC_FIXED48), the lossless 60-bit stream of the fp64
// solve (STAN_OPT_VALUE_STREAM_60, s60.h) and the packed column stream (struct
// colstream of spmv_kernels.inc; fold.hip packs the folded copy's columns through stan_pack_columns too).  The reference has
// no counterpart: alglib.sparsesmv behind SolverFunctions.LinearSolver_CG (SolverFunctions.cs:270-330) reads one CRS matrix.
#include <algorithm>

#include "internal.h"
#include "fx48.h"
#include "s60.h"
static_assert(S60_ROWS == 17, "stan_matrix::vs: dwords per slot of the 60-bit stream");

namespace {

__global__ void k_to_fp32(const double *in, float *out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (float)in[i];
}

// scaled fp64 values -> FIXED-48 stream (see vstream<uint32_t>); *bad counts the entries
// with |a| >= 2 (not representable: the matrix was not SPD-scalable)
__global__ void __launch_bounds__(256)
k_to_fx48(int64_t nslots, const double *vals, uint32_t *out, unsigned long long *bad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = t >> 6;
    const int lane = (int)(t & 63);
    if (slot >= nslots) return;
    const double *v = vals + slot * 9 * 64 + lane;
    uint32_t *o = out + slot * 14 * 64 + lane;
    uint32_t hi[10];
    int nbad = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const double a = v[j * 64] * FX48_ONE;
        long long q = 0;
        if (!(fabs(a) < 140737488355328.0)) nbad++;  // also catches NaN
        else q = __double2ll_rn(a);
        if (q >= 140737488355328LL) { q = 0; nbad++; }
        const unsigned long long u = (unsigned long long)(q + 140737488355328LL);
        o[j * 64] = (uint32_t)u;
        hi[j] = (uint32_t)(u >> 32);
    }
    hi[9] = 0;
#pragma unroll
    for (int m = 0; m < 5; m++) o[(9 + m) * 64] = hi[2 * m] | (hi[2 * m + 1] << 16);
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// scaled fp64 values -> the lossless 60-bit stream (s60.h; vstream<s60_t>); *bad counts the refused entries.  One lane per
// block row of a slot, like k_to_fx48: every load and store is a contiguous wave access; both sides are touched once.
__global__ void __launch_bounds__(256)
k_to_s60(int64_t nslots, const double *vals, uint32_t *out, unsigned long long *bad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t slot = t >> 6;
    const int lane = (int)(t & 63);
    if (slot >= nslots) return;
    const double *v = vals + slot * 9 * 64 + lane;
    uint32_t *o = out + slot * S60_ROWS * 64 + lane;
    uint32_t hi[9], w[8];
    int nbad = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        uint32_t lo;
        if (!s60_encode((uint64_t)__double_as_longlong(__builtin_nontemporal_load(v + j * 64)), &lo, &hi[j])) nbad++;
        __builtin_nontemporal_store(lo, o + j * 64);
    }
    s60_pack_high(hi, w);
#pragma unroll
    for (int m = 0; m < 8; m++) __builtin_nontemporal_store(w[m], o + (9 + m) * 64);
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// packed column stream (struct colstream): one wavefront per slice.  Mode of a slice (ok[slice]):
//   1  every slot's 64 columns (padding entries = the row's own column included) lie within 2^16 of the slot's smallest:
//      one base per slot (round 2);
//   2  (round 4) the slice mixes rows of different length -- the k-th neighbour of a short row (a node on the surface
//      of the mesh) plays another part than the k-th neighbour of its 27-neighbour slice mates and, once a breadth-first
//      level is wider than 2^16 rows (200^3: 120 k), lies further away than an offset reaches.  Two bases per slot: A
//      for the rows of the slice's full width, B for the shorter ones (cmask[slice]: one bit per lane); a padding
//      entry (zero values) takes offset 0 from its class's base.  63.9 % -> 99.8 % of the slots at 200^3 / 400^3,
//      98.4 % -> 99.9 % at 148^3 (profiles/r04/packed_columns_ab_two_bases_n148_n200.txt, packed_columns_simulation.txt);
//   0  neither: the slice keeps the int32 stream.
// rowof == nullptr (the folded copy's stream, whose lanes carry foreign pieces): modes 0 / 1 only.
__global__ void __launch_bounds__(256)
k_pack_cols(int32_t nslices, int64_t nloc, const int32_t *slot_ptr, const int32_t *cols, const int32_t *rowof, const int32_t *rowlen,
            const int32_t *pair_ptr, uint32_t *packed, int32_t *base, int32_t *base2, unsigned long long *cmask, uint8_t *ok) {
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;
    const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
    int32_t len = k1 - k0;   // without row lengths every entry counts as live and every lane as class A
    if (rowof) {
        const int64_t row = rowof[slice * 64 + lane];
        len = row < nloc ? rowlen[row] : 0;
    }
    const bool cls_b = len < k1 - k0;
    const int32_t BIG = 0x7fffffff;
    auto wmin = [](int32_t v) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
        return v;
    };
    auto wmax = [](int32_t v) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
        return v;
    };
    bool fits1 = true, fits2 = rowof != nullptr;
    for (int32_t k = k0; k < k1; k++) {
        const int32_t c = cols[(int64_t)k * 64 + lane];
        const bool live = k - k0 < len;
        fits1 = fits1 && (wmax(c) - wmin(c)) < 65536;
        if (fits2) {
            const int32_t mna = wmin(live && !cls_b ? c : BIG), mxa = wmax(live && !cls_b ? c : -1);
            const int32_t mnb = wmin(live && cls_b ? c : BIG), mxb = wmax(live && cls_b ? c : -1);
            fits2 = (mxa < 0 || mxa - mna < 65536) && (mxb < 0 || mxb - mnb < 65536);
        }
    }
    const int mode = fits1 ? 1 : fits2 ? 2 : 0;
    uint32_t *out = packed + (int64_t)pair_ptr[slice] * 64 + lane;
    uint32_t lo = 0;
    for (int32_t k = k0; k < k1; k++) {
        const int32_t c = cols[(int64_t)k * 64 + lane];
        uint32_t dlt;
        if (mode == 2) {
            const bool live = k - k0 < len;
            int32_t mna = wmin(live && !cls_b ? c : BIG);         // (BIG only if slice widths were ever padded beyond the longest row)
            int32_t mnb = wmin(live && cls_b ? c : BIG);
            if (mnb == BIG) mnb = mna;                            // no short row reaches this slot: its padding points at A's base
            if (mna == BIG) mna = mnb == BIG ? 0 : mnb;           // no class-A lane alive in this slot: never a base of 0x7fffffff
            if (mnb == BIG) mnb = mna;
            if (lane == 0) { base[k] = mna; base2[k] = mnb; }
            dlt = live ? (uint32_t)(c - (cls_b ? mnb : mna)) & 0xffffu : 0u;
        } else {
            const int32_t mn = wmin(c);
            if (lane == 0) { base[k] = mn; base2[k] = mn; }
            dlt = (uint32_t)(c - mn) & 0xffffu;
        }
        if (((k - k0) & 1) == 0) lo = dlt;
        else { *out = lo | (dlt << 16); out += 64; }
    }
    if ((k1 - k0) & 1) *out = lo;
    const unsigned long long mb = __ballot(cls_b);
    if (lane == 0) {
        ok[slice] = (uint8_t)mode;
        cmask[slice] = mode == 2 ? mb : 0ULL;
    }
}
__global__ void k_pair_counts(int32_t nslices, const int32_t *slot_ptr, int32_t *cnt) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nslices) cnt[s] = (slot_ptr[s + 1] - slot_ptr[s] + 1) >> 1;
}
__global__ void k_count_ok(int32_t nslices, const uint8_t *ok, const int32_t *slot_ptr, unsigned long long *out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nslices && ok[s]) atomicAdd(out, (unsigned long long)(slot_ptr[s + 1] - slot_ptr[s]));           // packed slots
    if (s < nslices && ok[s] == 2) atomicAdd(out + 1, (unsigned long long)(slot_ptr[s + 1] - slot_ptr[s]));  // ... with two bases
}

}  // namespace

// A block for `slots` slots of a value stream of K, allocated by trial (placement.hip) with the very product that will stream it
int stan_matrix_alloc_stream(stan_ctx *ctx, stan_matrix *K, int32_t kind, int64_t slots, void **out, bool folded, bool second_copy) {
    const size_t bytes = (size_t)slots * K->vs[kind].dwords * 64 * 4;
    return stan_dmalloc_streamed(ctx, out, bytes, [&, bytes](const void *q, float *ms, bool self) {
        return stan_spmv_probe(ctx, K, q, bytes, kind, ms, self, folded);
    }, second_copy);
}
// The encoding pass of the FIXED-48 or the 60-bit stream over scaled values; *bad = the entries it refused.  Synchronises the stream.
int stan_stream_encode(stan_ctx *ctx, int32_t kind, int64_t nslots, const double *d_vals, uint32_t *d_out, int64_t *bad) {
    unsigned long long *d_bad = (unsigned long long *)(ctx->d_status + SS_COUNTER);
    *bad = 0;
    if (nslots <= 0) return STAN_OK;
    HIPCHK(ctx, hipMemsetAsync(d_bad, 0, 8, ctx->stream));
    hipLaunchKernelGGL(kind == STAN_PREC_FIXED48 ? k_to_fx48 : k_to_s60, dim3((unsigned)nblk(nslots * 64, 256)), dim3(256), 0, ctx->stream, nslots, d_vals, d_out, d_bad);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_COUNTER, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *bad = ctx->h_status[SS_COUNTER];
    return STAN_OK;
}

int stan_matrix_make_fp32(stan_ctx *ctx, stan_matrix *K) {
    stan_value_stream &s = K->vs[STAN_PREC_MIXED];
    if (s.padded) return STAN_OK;
    const int64_t n = K->nslots * 9 * 64;
    STANCHK(stan_matrix_alloc_stream(ctx, K, STAN_PREC_MIXED, K->nslots, &s.padded));
    const unsigned blocks = std::min(std::max(nblk(n, 256), 1u), 2048u);   // (four times the grid of the CG's vector kernels)
    hipLaunchKernelGGL(k_to_fp32, dim3(blocks * 4), dim3(256), 0, ctx->stream, K->vals64(), (float *)s.padded, n);
    HIPCHK(ctx, hipGetLastError());
    return STAN_OK;
}

// FIXED-48 copy of the scaled values.  Returns STAN_OK with no block (and the stream marked refused) when some
// entry is not representable (K not SPD): the caller then streams the fp64 values.
int stan_matrix_make_fx48(stan_ctx *ctx, stan_matrix *K) {
    stan_value_stream &s = K->vs[STAN_PREC_FIXED48];
    if (s.padded || s.refused) return STAN_OK;
    if (K->nslots == 0) return STAN_OK;
    void *out;
    int64_t bad = 0;
    STANCHK(stan_matrix_alloc_stream(ctx, K, STAN_PREC_FIXED48, K->nslots, &out));
    STANCHK(stan_stream_encode(ctx, STAN_PREC_FIXED48, K->nslots, K->vals64(), (uint32_t *)out, &bad));
    if (bad != 0) { stan_dfree(ctx, out); s.refused = true; return STAN_OK; }
    s.padded = out;
    return STAN_OK;
}

// The lossless 60-bit stream of the scaled values (STAN_OPT_VALUE_STREAM_60), in two steps, because a solve that scales K
// with its first product (k_spmv_first) has the values only after its vectors are in use: the block -- from the pool, or by
// the placement search, which times the very product that will stream it on the very block that is kept -- and the
// encoding pass, which ends with the count of refused entries on the host.
//
// The block is a SECOND copy of the values (17/18 of the fp64 block, which stays) for the life of the matrix, and nothing
// needs it: so whether there is room is decided BEFORE anything is allocated, and "no" costs nothing -- no hipMalloc that
// fails, no flush of the parked blocks.  A parked block that fits is room (it is device memory this context holds
// anyway).  Otherwise
//  - pool budget: what this matrix gives back to the pool when it is freed -- its fp64 values, its columns and this block,
//    those of the pool's size class -- must fit into STAN_OPT_POOL_MAX_BYTES together; beyond it the pool would return the
//    oldest of them, the fp64 values, to the driver at every stan_hip_matrix_free, and the next assembly would pay a
//    hipMalloc of that size (seconds at 400^3, see stan_pool);
//  - free-memory floor: after the block is taken, as much again stays free as it takes (one more stream of the matrix --
//    the folded copy, a reduced-precision stream -- or the arrays of a recovery still fit), and never less than a
//    sixteenth of the device, the floor of the placement search's second stage.
// Both are figures of the moment (hipMemGetInfo counts every process on the device).  At 148^3 the block is 6.0 GB next
// to 6.4 + 0.4 GB; at 400^3 126 + 7 + 119 GB exceed the default pool budget (half of 288 GB) and, with the budget of a
// process that owns the device, the floor: 2 x 119 GB are not free beside 133 GB.
static bool s60_room(stan_ctx *ctx, const stan_matrix *K, size_t bytes) {
    const stan_pool &pool = ctx->pool;
    if (pool.enabled && bytes >= stan_pool::MIN_BYTES)
        for (const stan_pool::blk &b : pool.avail)
            if (b.cap >= bytes && b.cap <= bytes + bytes / 2) return true;
    if (pool.enabled) {
        const size_t own[3] = {(size_t)K->nslots * 9 * 64 * 8, (size_t)K->nslots * 64 * 4, bytes};
        size_t parked = 0;
        for (size_t b : own) parked += b >= stan_pool::MIN_BYTES ? b : 0;
        if (bytes >= stan_pool::MIN_BYTES && parked > pool.max_bytes) return false;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    const size_t floor_b = bytes > total_b / 16 ? bytes : total_b / 16;
    return free_b >= bytes + floor_b;
}
int stan_matrix_alloc_s60(stan_ctx *ctx, stan_matrix *K, uint32_t **out) {
    const size_t bytes = (size_t)K->nslots * S60_ROWS * 64 * 4;
    *out = nullptr;
    if (!s60_room(ctx, K, bytes)) return STAN_OK;
    const int rc = stan_matrix_alloc_stream(ctx, K, STAN_VALUE_STREAM_60, K->nslots, (void **)out, false, true);
    if (rc == STAN_E_ALLOC) { ctx->err.clear(); *out = nullptr; return STAN_OK; }   // (fragmentation: room by the figures, no block)
    return rc;
}
// K's scaled values into `blk` (stan_matrix_alloc_s60's), which becomes K's 60-bit stream -- or, an entry refused, goes back:
// the matrix then streams fp64 for good
int stan_matrix_encode_s60(stan_ctx *ctx, stan_matrix *K, uint32_t *blk) {
    stan_value_stream &s = K->vs[STAN_VALUE_STREAM_60];
    int64_t refused = 0;
    const int rc = stan_stream_encode(ctx, STAN_VALUE_STREAM_60, K->nslots, K->vals64(), blk, &refused);
    if (rc != STAN_OK || refused != 0) { stan_dfree(ctx, blk); s.refused = rc == STAN_OK; return rc; }
    s.padded = blk;
    return STAN_OK;
}

// Packed column stream of K (struct colstream), built once per matrix; the int32 columns stay (the
// assembly, scaling and export kernels use them).
int stan_matrix_make_cols16(stan_ctx *ctx, stan_matrix *K) {
    if (K->pk.cols16 || K->nslices <= 0) return STAN_OK;
    return stan_pack_columns(ctx, K->nslices, K->nslots, K->d_slot_ptr, K->d_cols, &K->pk, K->nloc, K->d_rowof, K->d_rowlen);
}
// the same for any sliced column stream (the folded copy of fold.hip has its own: no row lengths, so no two-base slices);
// out->cols16 stays nullptr when the pair index would not fit an int32
int stan_pack_columns(stan_ctx *ctx, int32_t nslices, int64_t nslots, const int32_t *d_slot_ptr, const int32_t *d_cols, stan_colpack *out,
                      int64_t nloc, const int32_t *d_rowof, const int32_t *d_rowlen) {
    hipStream_t st_ = ctx->stream;
    dev_scope bufs(ctx);
    int32_t *cnt; int64_t *ptr64;
    STANCHK(bufs.alloc(&cnt, (size_t)nslices + 1));
    STANCHK(bufs.alloc(&ptr64, (size_t)nslices + 2));
    hipLaunchKernelGGL(k_pair_counts, dim3(nblk(nslices, 256)), dim3(256), 0, st_, nslices, d_slot_ptr, cnt);
    STANCHK(stan_scan_total(ctx, cnt, ptr64, nslices, SS_H_NSLOTS));
    HIPCHK(ctx, hipStreamSynchronize(st_));
    const int64_t npairs = ctx->h_status[SS_H_NSLOTS];
    if (npairs >= ((int64_t)1 << 31)) return STAN_OK;   // pair index is int32: keep the plain columns
    STANCHK(stan_slot_ptr_narrow(ctx, ptr64, nslices, &out->pair_ptr));
    // one allocation: [n] base, [n] base2, [nslices] cmask (64-bit words), n = max(nslots, 1): make_colstream
    const size_t nb_ = (size_t)(nslots > 0 ? nslots : 1);
    STANCHK(stan_dmalloc(ctx, &out->colbase, 2 * nb_ + 2 * (size_t)nslices + 2));
    STANCHK(stan_dmalloc(ctx, &out->packed, (size_t)nslices));
    uint32_t *packed;
    STANCHK(stan_dmalloc(ctx, &packed, (size_t)(npairs > 0 ? npairs : 1) * 64));
    int32_t *b2_ = out->colbase + nb_;
    unsigned long long *cm_ = (unsigned long long *)(out->colbase + 2 * nb_);
    if (((uintptr_t)cm_ & 7) != 0) cm_ = (unsigned long long *)((uintptr_t)cm_ + 4);   // (never: 2 n ints from an aligned block)
    hipLaunchKernelGGL(k_pack_cols, dim3(nblk(nslices, 4)), dim3(256), 0, st_, nslices, nloc, d_slot_ptr, d_cols, d_rowof, d_rowlen,
                       out->pair_ptr, packed, out->colbase, b2_, cm_, out->packed);
    unsigned long long *d_cnt = (unsigned long long *)(ctx->d_status + SS_COUNTER);   // two words: SS_COUNTER, SS_H_ERRCOPY
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 16, st_));
    hipLaunchKernelGGL(k_count_ok, dim3(nblk(nslices, 256)), dim3(256), 0, st_, nslices, out->packed, d_slot_ptr, d_cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_COUNTER, d_cnt, 16, hipMemcpyDeviceToHost, st_));
    HIPCHK(ctx, hipStreamSynchronize(st_));
    out->slots_packed = ctx->h_status[SS_COUNTER];
    out->slots_packed2 = ctx->h_status[SS_COUNTER + 1];
    out->cols16 = packed;
    return STAN_OK;
}
