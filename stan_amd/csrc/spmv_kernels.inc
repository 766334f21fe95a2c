// spmv_kernels.inc -- the products: k_spmv (one wavefront per slice), k_spmv_small (one workgroup per slice), k_spmv2 (two right-hand sides), k_spmv_fold (folded rows)
// Part of cg.hip (included there, inside its anonymous namespace; not a translation unit of its own): split out in
// round 4 so that each piece can be read on its own.  The reference has no counterpart of these kernels beyond the
// calls they replace: alglib.lincgsolvesparse / sparsesmv behind SolverFunctions.LinearSolver_CG (SolverFunctions.cs:270-330).

// ---- SpMV --------------------------------------------------------------------------------------
// y = A x over BSELL-64.  One wavefront per slice, one lane per block row: every load of
// the value stream is a contiguous 512-B (fp64) / 256-B (fp32) wave access; x is gathered
// (24 B per block, L2 / Infinity-Cache resident: neighbouring rows share columns).
// DOT = 1: also the per-block partial of x_own . y  (p.Ap of the CG); DOT = 2: the partials of
// x_own . x_own and x_own . y (r.r and r.Ar of the single-reduction CG); the block that finishes
// last adds the partials up (fold_args).
// VAR selects the kernel variant:
//   0   plain loads, identity workgroup mapping (the reference point of the A/B runs)
//   9   non-temporal loads for the once-read matrix stream (keeps x in L2 / MALL) + XCD-chunked
//       workgroup mapping (below)                                   -- default for fp64 / fp32
//   12  = 9 with the block loop unrolled by 4                       -- default for FIXED-48
// (The other A/B variants of rounds 1-2 -- mappings, unroll depths, register caps, a timing-only kernel -- live in the lab
// build: lab/lab_hooks.patch, `make lab`.)
// NT must be a compile-time choice: with a run-time flag, `nt ? __builtin_nontemporal_load(p) : *p`
// is two loads of one address that the optimiser merges into ONE plain load inside this helper,
// before it is inlined anywhere -- the non-temporal hint never reached the ISA (no `nt` bit on any
// global_load of the first builds; found by reading the disassembly).
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// Value streams of the matrix.  double / float: vals[slot][9][64].
// uint32_t = FIXED-48 (STAN_PREC_FIXED48): after the Jacobi scaling every entry of an SPD matrix
// satisfies |a_ij| <= sqrt(a_ii a_jj) = 1, so no exponent is needed: q = rint(a * 2^46) as a
// signed 48-bit integer (absolute error <= 2^-47 = 7.1e-15 of the unit diagonal), stored
// offset-binary u = q + 2^47 as vals48[slot][14][64] dwords: rows 0..8 the low 32 bits of the
// nine entries, rows 9..13 the high 16 bits packed two per dword.  60 B per block instead of
// 76 B.  Decoding is one integer op and one exact fp64 subtraction per entry: the bits
// 0x43300000'00000000 | u are the double 2^52 + u.  The 2^-46 is applied to the three
// gathered x values instead of the nine entries (powers of two commute with rounding), so
// the arithmetic is the fp64 product with the quantised matrix.
// s60_t = the lossless 60-bit stream of the scaled fp64 values (s60.h; STAN_OPT_VALUE_STREAM_60): vals60[slot][17][64]
// dwords, rows 0..8 the low 32 bits of the nine entries, rows 9..16 their nine 28-bit high parts (sign, 7-bit exponent
// code, 20 mantissa bits) back to back.  68 B per block instead of 72 B; decoding is integer work only -- a funnel shift
// or a mask, one add, one select per entry -- and yields the stored double bit for bit, so a product of this stream IS the
// fp64 product.  (A tag type of its own: uint32_t is FIXED-48's.)
struct s60_t { uint32_t w; };
template <typename VT> struct vstream { static constexpr int STRIDE = 9 * 64; static constexpr bool FX = false, P60 = false; };
template <> struct vstream<uint32_t> { static constexpr int STRIDE = 14 * 64; static constexpr bool FX = true, P60 = false; };
template <> struct vstream<s60_t> { static constexpr int STRIDE = S60_ROWS * 64; static constexpr bool FX = false, P60 = true; };

template <bool NT, typename VT>
__device__ __forceinline__ void load9(const VT *vp, double a[9]) {
    if constexpr (vstream<VT>::FX) {
        uint32_t lo[9], hw[5];
#pragma unroll
        for (int j = 0; j < 9; j++) lo[j] = ld_stream<NT>(vp + j * 64);
#pragma unroll
        for (int m = 0; m < 5; m++) hw[m] = ld_stream<NT>(vp + (9 + m) * 64);
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const uint32_t h = (j & 1) ? (hw[j >> 1] >> 16) : (hw[j >> 1] & 0xffffu);
            a[j] = __hiloint2double((int)(0x43300000u | h), (int)lo[j]) - FX48_BIAS;
        }
    } else if constexpr (vstream<VT>::P60) {
        uint32_t lo[9], hw[8];
#pragma unroll
        for (int j = 0; j < 9; j++) lo[j] = ld_stream<NT>(&vp[j * 64].w);
#pragma unroll
        for (int m = 0; m < 8; m++) hw[m] = ld_stream<NT>(&vp[(9 + m) * 64].w);
#pragma unroll
        for (int j = 0; j < 9; j++) a[j] = __longlong_as_double((long long)s60_decode(lo[j], s60_high(hw, j)));
    } else {
#pragma unroll
        for (int j = 0; j < 9; j++) a[j] = (double)ld_stream<NT>(vp + j * 64);
    }
}

// Packed column stream (round 2): the block-column indices of a slot are, in reference (BFS) DOF
// order, within a few thousand of each other across the 64 rows of a slice, so a slot stores its
// smallest column once (a wave-uniform scalar) and every lane a 16-bit offset, two slots per
// dword: 2 B per block instead of 4 (74 B instead of 76 with fp64 values: -2.6 % of the SpMV's
// bytes, lossless, same products in the same order -> same bits).  Slices whose offsets do not fit
// (the ragged last slice, rows coupling owned and halo columns far apart) keep the int32 stream.
struct colstream {
    const uint32_t *packed;   // [pair][64]: offset of slot 2j in the low half, of slot 2j+1 in the high half
    const int32_t *base;      // [slot] smallest column of the slot
    const int32_t *pair_ptr;  // [nslices + 1] first pair of every slice
    const uint8_t *ok;        // [nslices] 0 = int32 columns, 1 = packed, one base per slot, 2 = packed, two bases (k_pack_cols)
    const int32_t *base2;     // [slot] mode 2: the base of the slice's SHORTER rows (base: of its full-width rows)
    const unsigned long long *cmask;   // [nslices] mode 2: bit l = lane l holds a shorter row
};
constexpr colstream NO_COLSTREAM = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
// the arrays behind `base` (one allocation, stan_pack_columns): [nslots] base, [nslots] base2, [nslices] cmask
inline colstream make_colstream(const stan_colpack &c, int64_t nslots) {
    const int64_t n = nslots > 0 ? nslots : 1;
    return colstream{c.cols16, c.colbase, c.pair_ptr, c.packed, c.colbase + n, (const unsigned long long *)(c.colbase + 2 * n)};
}

// ---- the pieces every product kernel shares -------------------------------------------------------------------------
// XCD-chunked workgroup mapping (CH = 0: identity).  Workgroups go round-robin to the 8 XCDs; here every window of 8*CH
// consecutive workgroups is dealt so that each XCD gets CH CONSECUTIVE ones: an XCD's L2 then holds the x window of one
// contiguous run of rows while the chip as a whole still sweeps the matrix front to back.
template <int CH>
__device__ __forceinline__ int64_t xcd_chunked(int64_t bid) {
    if constexpr (CH > 0) {
        const int64_t win = 8 * CH, grp = bid / win, within = bid - grp * win;
        if ((grp + 1) * win <= (int64_t)gridDim.x)   // the ragged tail keeps the identity mapping
            bid = grp * win + (within & 7) * CH + (within >> 3);
    }
    return bid;
}
// position `pos` of a launch -> slice: itself, or through the interior / boundary list (past its end: no slice)
__device__ __forceinline__ int64_t slice_at(int64_t pos, const int32_t *__restrict__ slist, int32_t nlist, int32_t nslices) {
    if (slist) pos = pos < nlist ? (int64_t)slist[pos] : (int64_t)nslices;
    return pos;
}
// SELL-C-sigma: position -> block row (nloc: none, a padding position or no slice)
__device__ __forceinline__ int64_t row_at(int64_t slice, int32_t nslices, const int32_t *__restrict__ rowof, int lane, int64_t nloc) {
    return slice < nslices ? (int64_t)rowof[slice * 64 + lane] : nloc;
}
// the three values of block row `row`; non-temporal where the matrix stream is: A p is read exactly once, by k_step
template <bool NT>
__device__ __forceinline__ void store_row(double *__restrict__ y, int64_t row, double y0, double y1, double y2) {
    if (NT) {
        __builtin_nontemporal_store(y0, y + 3 * row); __builtin_nontemporal_store(y1, y + 3 * row + 1);
        __builtin_nontemporal_store(y2, y + 3 * row + 2);
    } else { y[3 * row] = y0; y[3 * row + 1] = y1; y[3 * row + 2] = y2; }
}
// The dot products fused into a product (DOT as in k_spmv).  dot_terms: the row's terms d = x_row . y_row and, DOT = 2,
// e = x_row . x_row.  dot_reduce (every thread of the block; rows without terms bring zeros): the block's sums to
// partial[blockIdx.x + poff] -- DOT = 2: the pair [sum e, sum d] -- as agent-scope stores, then the ticket of the folded
// reduction; the block that draws the last one adds all partials up (fold_arrive / fold_finish, cg_reduce_device.inc).
template <int DOT>
__device__ __forceinline__ void dot_terms(const double *__restrict__ x, int64_t row, double y0, double y1, double y2, double &d, double &e) {
    const double x0 = x[3 * row], x1 = x[3 * row + 1], x2 = x[3 * row + 2];
    d = y0 * x0 + y1 * x1 + y2 * x2;
    if (DOT == 2) e = x0 * x0 + x1 * x1 + x2 * x2;
}
template <int DOT>
__device__ __forceinline__ void dot_reduce(double d, double e, double *partial, int32_t poff, const fold_args &fold, double *sh, int *sh_last) {
    const double t = block_sum(d, sh);
    if (DOT == 2) {
        const double u = block_sum(e, sh);
        if (threadIdx.x == 0) {
            st_agent(partial + 2 * (int64_t)(blockIdx.x + poff), u);
            st_agent(partial + 2 * (int64_t)(blockIdx.x + poff) + 1, t);
        }
    } else if (threadIdx.x == 0) st_agent(partial + blockIdx.x + poff, t);
    if (fold.counter && fold_arrive(fold, sh_last)) fold_finish<(DOT == 2 ? 2 : 1)>(fold, partial, sh);
}
// The walk of one wavefront over the slots [ka, kb) of `slice` (whose first slot is k0; ka - k0 even), one lane per block
// row: body(c, vp) for every slot, c the lane's block column, vp its entry of the value stream `vals` ([slot][STRIDE], a
// carried pointer).  Packed slices (colstream) two slots per trip -- unrolling that further costs 40 VGPRs --, int32
// columns one slot per trip, unrolled UNR times.
template <bool NT, int UNR, int STRIDE, typename V, typename BODY>
__device__ __forceinline__ void walk_slots(const colstream &cs, const int32_t *__restrict__ cols, int64_t slice, int lane,
                                           int32_t k0, int32_t ka, int32_t kb, V *__restrict__ vals, BODY body) {
    const int32_t *cp = cols + (int64_t)ka * 64 + lane;
    V *vp = vals + (int64_t)ka * STRIDE + lane;
    const int pmode = cs.packed ? (int)cs.ok[slice] : 0;   // wave-uniform: 0 int32 columns, 1 / 2 packed (k_pack_cols)
    if (pmode != 0) {   // one loop for both packed modes: a one-base slice has cmask 0 and base2 = base
        // two bases per slot: the lane's class picks (a select between two scalars)
        const uint32_t *cq = cs.packed + ((int64_t)cs.pair_ptr[slice] + ((ka - k0) >> 1)) * 64 + lane;
        const int32_t *bp = cs.base + __builtin_amdgcn_readfirstlane(ka);
        const int32_t *bq = cs.base2 + __builtin_amdgcn_readfirstlane(ka);
        const bool cb = (cs.cmask[slice] >> lane) & 1ull;
        int32_t k = ka;
#pragma unroll 1
        for (; k + 1 < kb; k += 2) {
            const uint32_t wd = ld_stream<NT>(cq);
            // four scalar loads and two selects of VALUES: written as `cb ? bq[0] : bp[0]` the select lands on the
            // pointer and the bases arrive through a per-lane vector load (+0.6 %, tools/lab/spmv_steps_lab.cpp S35)
            const int32_t b0 = bp[0], b1 = bp[1], q0 = bq[0], q1 = bq[1];
            const int64_t c = (int64_t)(cb ? q0 : b0) + (int64_t)(wd & 0xffffu);
            const int64_t c2 = (int64_t)(cb ? q1 : b1) + (int64_t)(wd >> 16);
            body(c, vp);
            body(c2, vp + STRIDE);
            cq += 64;
            bp += 2;
            bq += 2;
            vp += 2 * STRIDE;
        }
        if (k < kb) {
            const int32_t b0 = bp[0], q0 = bq[0];
            const int64_t c = (int64_t)(cb ? q0 : b0) + (int64_t)(ld_stream<NT>(cq) & 0xffffu);
            body(c, vp);
        }
    } else {
#pragma unroll UNR
        for (int32_t k = ka; k < kb; k++) {
            const int64_t c = ld_stream<NT>(cp);
            body(c, vp);
            cp += 64;
            vp += STRIDE;
        }
    }
}

// One row of a block on the 60-bit stream: y + (a0 x0 + a1 x1 + a2 x2) as the kernels of the fp64 stream compute it.
// The library is compiled with fused multiply-adds allowed, and WHICH of the two products of a0 x0 + a1 x1 stays a rounded
// multiplication of its own is then the compiler's choice: a1 x1 in every k_spmv of the fp64 stream -- but for entries
// that come out of integer registers it chose a0 x0 in two rows of three, and a solve on the lossless stream ended
// 1e-8 away from the fp64 one.  So the operations are spelled out here; no product feeds an addition, nothing is left
// to fuse.  (tests/test_gpu_stream60.py compares solves bit for bit, k_spmv<s60_t, 1, 9> against k_spmv<double, 1, 9> and
// <.., 12> against <.., 12>: a compiler that changes its mind about either fp64 kernel shows there.)
__device__ __forceinline__ double s60_row(double a0, double a1, double a2, double x0, double x1, double x2, double y) {
    double t = a1 * x1;
    t = __builtin_fma(a0, x0, t);
    t = __builtin_fma(a2, x2, t);
    return y + t;
}

#define STAN_SPMV_BLOCK(C, VP)                                                        \
    {                                                                                 \
        double a[9];                                                                  \
        load9<NT, VT>(VP, a);                                                         \
        double x0 = x[3 * (C)], x1 = x[3 * (C) + 1], x2 = x[3 * (C) + 2];             \
        if (vstream<VT>::FX) { x0 *= FX48_INV; x1 *= FX48_INV; x2 *= FX48_INV; }      \
        if constexpr (vstream<VT>::P60) {                                             \
            y0 = s60_row(a[0], a[1], a[2], x0, x1, x2, y0);                           \
            y1 = s60_row(a[3], a[4], a[5], x0, x1, x2, y1);                           \
            y2 = s60_row(a[6], a[7], a[8], x0, x1, x2, y2);                           \
        } else {                                                                      \
            y0 += a[0] * x0 + a[1] * x1 + a[2] * x2;                                  \
            y1 += a[3] * x0 + a[4] * x1 + a[5] * x2;                                  \
            y2 += a[6] * x0 + a[7] * x1 + a[8] * x2;                                  \
        }                                                                             \
    }

template <typename VT, int DOT, int VAR>
__global__ void __launch_bounds__(256)
k_spmv(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
       const int32_t *__restrict__ cols, const VT *__restrict__ vals,
       const double *__restrict__ x, double *__restrict__ y, double *partial,
       const int64_t *st, int64_t kiter, const int32_t *__restrict__ slist, int32_t nlist,
       int32_t poff, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    if (stopped(st, kiter)) { fold_skip(fold); return; }
    constexpr bool NT = VAR != 0;
    constexpr int UNR = VAR == 12 ? 4 : 2;
    constexpr int CH = VAR != 0 ? 32 : 0;
    const int lane = threadIdx.x & 63;
    int64_t bid = blockIdx.x;
    bid = xcd_chunked<CH>(bid);
    const int64_t slice = slice_at(bid * 4 + (threadIdx.x >> 6), slist, nlist, nslices);
    double y0 = 0, y1 = 0, y2 = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        walk_slots<NT, UNR, vstream<VT>::STRIDE>(cs, cols, slice, lane, k0, k0, k1, vals,
                                                 [&](int64_t c, const VT *vp) { STAN_SPMV_BLOCK(c, vp) });
        if (row < nloc) store_row<NT>(y, row, y0, y1, y2);
    }
    if (DOT) {
        double d = 0, e = 0;
        if (slice < nslices && row < nloc) dot_terms<DOT>(x, row, y0, y1, y2, d, e);
        dot_reduce<DOT>(d, e, partial, poff, fold, sh, &sh_last);
    }
}

// ---- two wavefronts per slice (round 6: a RANK'S SHARD of the headline cube is a mid-size system) ---------------------
// At 150 k ... 1.1 M block rows (60^3 ... 100^3, or one of 8 ranks' rows of 148^3) k_spmv has 2 400 ... 16 000 wavefronts for
// 1024 SIMDs and runs for 85 ... 330 us: 0.66 ... 0.78 of the HBM peak against 0.82 at 148^3 (profiles/r05/
// spmv_small_kernel_limit_n60_n80_n100.txt); k_spmv_small's four waves per slice with plain loads are slower still there.
// This is the form in between: k_spmv's loop (packed columns two slots per trip, XCD-chunked mapping, NT as a template
// parameter) with the slots of a slice split between TWO wavefronts at an even slot, the second wave's sums handed over
// through LDS and added in a fixed order (first half + second half: deterministic, NOT the one-wave order).  A workgroup
// = 2 slices.  MEASURED (profiles/r06/spmv_pair_kernel_n60_n72_n80_n100.txt, whole bench steps): 60^3 x1.09, 72^3 x1.00,
// 80^3 x1.05, 100^3 x1.01 against k_spmv; with plain instead of non-temporal loads 0.92-1.00 everywhere (that form was
// removed again).  The bar set for making it the choice of a size class -- +5 % at 72^3, one rank's share of 148^3 on 8
// GPUs -- is NOT met: it stays an explicit option (STAN_OPT_SPMV_VARIANT 20), never chosen by the library.
template <typename VT, int DOT, bool NT>
__global__ void __launch_bounds__(256)
k_spmv_pair(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
            const int32_t *__restrict__ cols, const VT *__restrict__ vals,
            const double *__restrict__ x, double *__restrict__ y, double *partial,
            const int64_t *st, int64_t kiter, const int32_t *__restrict__ slist, int32_t nlist,
            int32_t poff, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    __shared__ double acc[2][3][64];
    if (stopped(st, kiter)) { fold_skip(fold); return; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, sl = w >> 1, half = w & 1;
    const int64_t slice = slice_at(xcd_chunked<32>(blockIdx.x) * 2 + sl, slist, nlist, nslices);
    double y0 = 0, y1 = 0, y2 = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        int32_t mid = k0 + ((((k1 - k0) + 1) / 2 + 1) & ~1);   // an EVEN number of slots for the first wave: packed pairs stay whole
        if (mid > k1) mid = k1;
        const int32_t ka = half ? mid : k0, kb = half ? k1 : mid;
        walk_slots<NT, 2, vstream<VT>::STRIDE>(cs, cols, slice, lane, k0, ka, kb, vals,
                                               [&](int64_t c, const VT *vp) { STAN_SPMV_BLOCK(c, vp) });
    }
    if (half) { acc[sl][0][lane] = y0; acc[sl][1][lane] = y1; acc[sl][2][lane] = y2; }
    __syncthreads();
    double d = 0, e = 0;
    if (!half && slice < nslices && row < nloc) {
        y0 += acc[sl][0][lane]; y1 += acc[sl][1][lane]; y2 += acc[sl][2][lane];
        store_row<NT>(y, row, y0, y1, y2);
        if (DOT) dot_terms<DOT>(x, row, y0, y1, y2, d, e);
    }
    if (DOT) dot_reduce<DOT>(d, e, partial, poff, fold, sh, &sh_last);
}

// ---- the yardstick of the product's roofline --------------------------------------------------------------------------
// K's fp64 value stream read the way k_spmv reads it -- one wavefront per slice, the XCD-chunked workgroup mapping,
// non-temporal 8-byte loads, two slots per trip -- and NOTHING ELSE: no column words, no gather of x, no product vector
// stored (one double per workgroup leaves, so that the loads are not dropped).  What this kernel reaches on K's resident
// values is what the memory system gives a read-only sweep of that block on THIS device; bench.py reports it as
// `roofline.stream_GBs` and the product's rate against it as `frac_of_stream` (stan_hip_stream_bench).  Round 4 measured
// the same with a lab program on a synthetic operator (tools/lab/spmv_steps_lab.cpp S0: 7.2 TB/s).
__global__ void __launch_bounds__(256)
k_value_stream(int32_t nslices, const int32_t *__restrict__ slot_ptr, const double *__restrict__ vals, double *sink) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63;
    const int64_t slice = xcd_chunked<32>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    double s0 = 0, s1 = 0, s2 = 0;
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        const double *vp = vals + (int64_t)k0 * vstream<double>::STRIDE + lane;
        int32_t k = k0;
        for (; k + 1 < k1; k += 2) {
            double a[9], b[9];
            load9<true, double>(vp, a);
            load9<true, double>(vp + vstream<double>::STRIDE, b);
            s0 += a[0] + a[1] + a[2] + b[0] + b[1] + b[2];
            s1 += a[3] + a[4] + a[5] + b[3] + b[4] + b[5];
            s2 += a[6] + a[7] + a[8] + b[6] + b[7] + b[8];
            vp += 2 * vstream<double>::STRIDE;
        }
        if (k < k1) {
            double a[9];
            load9<true, double>(vp, a);
            s0 += a[0] + a[1] + a[2]; s1 += a[3] + a[4] + a[5]; s2 += a[6] + a[7] + a[8];
        }
    }
    const double t = block_sum(s0 + s1 + s2, sh);
    if (threadIdx.x == 0) sink[blockIdx.x] = t;
}

// ---- the FIRST product of a matrix: scale on the fly -----------------------------------------------------------------
// alglib's lincg iterates on S K S (cg.hip); rounds 1-4 brought the assembled K into that form with a pass of its own
// (k_scale_matrix: 6.4 GB read + 6.4 GB written at 148^3, 2.7 ms) before the first iteration.  The first product of the
// loop reads every value anyway: this variant of k_spmv (fp64 values, non-temporal stream, XCD-chunked mapping, both
// column streams) multiplies each block by s_row s_col -- the expression of k_scale_matrix, so the stored values and
// every later product keep their bits --, writes it back and multiplies with the scaled block.  One read of K saved,
// one kernel less (VERDICT r04 item 8: k_scale_matrix gone from the single-GPU fp64 trace).  s is padded to whole
// slices with 1.0 (a padding entry is a zero block whose column is its row).
template <int DOT>
__global__ void __launch_bounds__(256)
k_spmv_first(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
             const int32_t *__restrict__ cols, double *__restrict__ vals, const double *__restrict__ s,
             const double *__restrict__ x, double *__restrict__ y, double *partial,
             const int64_t *st, int64_t kiter, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    // (never skipped: the scaling must happen even when the solve has stopped at its first residual test -- the caller
    // only launches it for a solve that iterates)
    (void)st; (void)kiter;
    const int lane = threadIdx.x & 63;
    const int64_t slice = xcd_chunked<32>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    double y0 = 0, y1 = 0, y2 = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        const double sr0 = s[3 * row], sr1 = s[3 * row + 1], sr2 = s[3 * row + 2];
#define STAN_SPMV_FIRST_BLOCK(C, VP)                                                                   \
    {                                                                                                  \
        double a[9];                                                                                   \
        load9<true, double>(VP, a);                                                                    \
        const double sc0_ = s[3 * (C)], sc1_ = s[3 * (C) + 1], sc2_ = s[3 * (C) + 2];                  \
        a[0] *= sr0 * sc0_; a[1] *= sr0 * sc1_; a[2] *= sr0 * sc2_;                                    \
        a[3] *= sr1 * sc0_; a[4] *= sr1 * sc1_; a[5] *= sr1 * sc2_;                                    \
        a[6] *= sr2 * sc0_; a[7] *= sr2 * sc1_; a[8] *= sr2 * sc2_;                                    \
        _Pragma("unroll") for (int j = 0; j < 9; j++) __builtin_nontemporal_store(a[j], (VP) + j * 64); \
        const double x0 = x[3 * (C)], x1 = x[3 * (C) + 1], x2 = x[3 * (C) + 2];                        \
        y0 += a[0] * x0 + a[1] * x1 + a[2] * x2;                                                       \
        y1 += a[3] * x0 + a[4] * x1 + a[5] * x2;                                                       \
        y2 += a[6] * x0 + a[7] * x1 + a[8] * x2;                                                       \
    }
        walk_slots<true, 1, 9 * 64>(cs, cols, slice, lane, k0, k0, k1, vals,
                                    [&](int64_t c, double *vp) { STAN_SPMV_FIRST_BLOCK(c, vp) });
#undef STAN_SPMV_FIRST_BLOCK
        if (row < nloc) store_row<true>(y, row, y0, y1, y2);
    }
    if (DOT) {
        double d = 0, e = 0;
        if (slice < nslices && row < nloc) dot_terms<DOT>(x, row, y0, y1, y2, d, e);
        dot_reduce<DOT>(d, e, partial, 0, fold, sh, &sh_last);
    }
}

// ---- SpMV for SMALL systems -----------------------------------------------------------------------
// Below ~150 k block rows the chip is not filled by one wavefront per slice (46 875 DOF: 245 slices
// on 1024 SIMDs), and a wavefront walking its 27 slots is a chain of dependent memory round trips:
// k_spmv takes 19 us there, two thirds of an iteration (rocprofv3, tools/small_sizes.py).  Here a
// slice belongs to a WORKGROUP: its four wavefronts take every fourth slot, the four partial rows are
// added through LDS in a fixed order (wave 0 + 1 + 2 + 3: deterministic; another order than k_spmv's,
// so the choice between the two depends on the GLOBAL row count only -- every shard of a sharded
// matrix and the unsharded matrix use the same kernel and keep producing the same bits).  Plain
// loads: a matrix of this size stays in the L2s / the memory-side cache from one product to the next.
template <typename VT, int DOT>
__global__ void __launch_bounds__(256)
k_spmv_small(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
             const int32_t *__restrict__ cols, const VT *__restrict__ vals,
             const double *__restrict__ x, double *__restrict__ y, double *partial,
             const int64_t *st, int64_t kiter, const int32_t *__restrict__ slist, int32_t nlist,
             int32_t poff, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    __shared__ double acc[3][4][64];
    if (stopped(st, kiter)) { fold_skip(fold); return; }
    constexpr bool NT = false;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t slice = slice_at(blockIdx.x, slist, nlist, nslices);
    double y0 = 0, y1 = 0, y2 = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
        const int pmode = cs.packed ? (int)cs.ok[slice] : 0;   // 0 int32 columns, 1 / 2 packed (one / two bases per slot)
        const bool packed = pmode != 0;
        const bool cb = pmode == 2 && ((cs.cmask[slice] >> lane) & 1ull);   // this lane's row takes the slot's second base
        const int64_t pp = packed ? (int64_t)cs.pair_ptr[slice] : 0;
        for (int32_t k = k0 + w; k < k1; k += 4) {
            int64_t c;
            if (packed) {
                const uint32_t wd = cs.packed[(pp + ((k - k0) >> 1)) * 64 + lane];
                const int32_t b0 = cs.base[k], q0 = cs.base2[k];
                c = (int64_t)(cb ? q0 : b0) + (int64_t)(((k - k0) & 1) ? (wd >> 16) : (wd & 0xffffu));
            } else
                c = cols[(int64_t)k * 64 + lane];
            const VT *vp = vals + (int64_t)k * vstream<VT>::STRIDE + lane;
            STAN_SPMV_BLOCK(c, vp)
        }
    }
    acc[0][w][lane] = y0; acc[1][w][lane] = y1; acc[2][w][lane] = y2;
    __syncthreads();
    double d = 0, e = 0;
    if (w == 0) {
        y0 = ((acc[0][0][lane] + acc[0][1][lane]) + acc[0][2][lane]) + acc[0][3][lane];
        y1 = ((acc[1][0][lane] + acc[1][1][lane]) + acc[1][2][lane]) + acc[1][3][lane];
        y2 = ((acc[2][0][lane] + acc[2][1][lane]) + acc[2][2][lane]) + acc[2][3][lane];
        if (slice < nslices && row < nloc) {
            store_row<NT>(y, row, y0, y1, y2);
            if (DOT) dot_terms<DOT>(x, row, y0, y1, y2, d, e);
        }
    }
    if (DOT) dot_reduce<DOT>(d, e, partial, poff, fold, sh, &sh_last);
}

// Two right-hand sides in ONE pass over the matrix: y = A x and y2 = A x2 (+ the x.y partial).
// Used on the residual-refresh iterations: r = b - A(x + a p) = b - (A x + a A p), so the
// refresh needs A x next to the A p every iteration needs -- one matrix stream instead of two.
// 128-VGPR budget (4 waves per SIMD): with the default target the four gathers of a trip (x and x2 of two slots) were
// issued one by one, each behind a wait for earlier data
// VT = s60_t (STAN_OPT_CG_REFRESH_60): the same pass on the lossless 60-bit stream.  In the gfx950 code of k_spmv2<double>
// every one of its row sums -- six per block, in each of the walk's block bodies (two per packed trip and the odd slot, two
// per int32-column trip and its remainder) -- keeps a1 x1 (a1 u1) as the rounded multiplication and fuses a0 x0, then
// a2 x2, onto it, as k_spmv does: s60_row spells exactly that out, for every position alike.
template <typename VT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_spmv2(int32_t nslices, int64_t nloc, const int32_t *__restrict__ slot_ptr, const int32_t *__restrict__ rowof,
        const int32_t *__restrict__ cols, const VT *__restrict__ vals,
        const double *__restrict__ x, const double *__restrict__ x2, double *__restrict__ y,
        double *__restrict__ y2, double *partial, const int64_t *st, int64_t kiter,
        const int32_t *__restrict__ slist, int32_t nlist, int32_t poff, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    if (stopped(st, kiter)) { fold_skip(fold); return; }
    const int lane = threadIdx.x & 63;
    int64_t bid = blockIdx.x;
    bid = xcd_chunked<32>(bid);
    const int64_t slice = slice_at(bid * 4 + (threadIdx.x >> 6), slist, nlist, nslices);
    double y0 = 0, y1 = 0, yy2 = 0, z0 = 0, z1 = 0, z2 = 0;
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    if (slice < nslices) {
        const int32_t k0 = slot_ptr[slice], k1 = slot_ptr[slice + 1];
#define STAN_SPMV2_BLOCK(C, VP)                                                       \
    {                                                                                 \
        double a[9];                                                                  \
        load9<true, VT>(VP, a);                                                       \
        double x0 = x[3 * (C)], x1 = x[3 * (C) + 1], xx2 = x[3 * (C) + 2];            \
        double u0 = x2[3 * (C)], u1 = x2[3 * (C) + 1], u2 = x2[3 * (C) + 2];          \
        if (vstream<VT>::FX) {                                                        \
            x0 *= FX48_INV; x1 *= FX48_INV; xx2 *= FX48_INV;                          \
            u0 *= FX48_INV; u1 *= FX48_INV; u2 *= FX48_INV;                           \
        }                                                                             \
        if constexpr (vstream<VT>::P60) {                                             \
            y0 = s60_row(a[0], a[1], a[2], x0, x1, xx2, y0);                          \
            y1 = s60_row(a[3], a[4], a[5], x0, x1, xx2, y1);                          \
            yy2 = s60_row(a[6], a[7], a[8], x0, x1, xx2, yy2);                        \
            z0 = s60_row(a[0], a[1], a[2], u0, u1, u2, z0);                           \
            z1 = s60_row(a[3], a[4], a[5], u0, u1, u2, z1);                           \
            z2 = s60_row(a[6], a[7], a[8], u0, u1, u2, z2);                           \
        } else {                                                                      \
            y0 += a[0] * x0 + a[1] * x1 + a[2] * xx2;                                 \
            y1 += a[3] * x0 + a[4] * x1 + a[5] * xx2;                                 \
            yy2 += a[6] * x0 + a[7] * x1 + a[8] * xx2;                                \
            z0 += a[0] * u0 + a[1] * u1 + a[2] * u2;                                  \
            z1 += a[3] * u0 + a[4] * u1 + a[5] * u2;                                  \
            z2 += a[6] * u0 + a[7] * u1 + a[8] * u2;                                  \
        }                                                                             \
    }
        walk_slots<true, 2, vstream<VT>::STRIDE>(cs, cols, slice, lane, k0, k0, k1, vals,
                                                 [&](int64_t c, const VT *vp) { STAN_SPMV2_BLOCK(c, vp) });
#undef STAN_SPMV2_BLOCK
        if (row < nloc) {   // both products are read exactly once, by k_step
            store_row<true>(y, row, y0, y1, yy2);
            store_row<true>(y2, row, z0, z1, z2);
        }
    }
    double d = 0, e = 0;
    if (slice < nslices && row < nloc) dot_terms<1>(x, row, y0, y1, yy2, d, e);
    dot_reduce<1>(d, e, partial, poff, fold, sh, &sh_last);
}


// ---- folded rows (STAN_OPT_ROW_FOLDING, fold.hip) ---------------------------------------------------------
// The streams of fold.hip: padded-slot layout ([slot][ROWS][64]) with W ~ blocks/64 slots per slice; slots
// < own[lane] hold the lane's own row, the slots behind them a piece of ONE longer row of the slice (or zeros).
// Two accumulators per lane; the foreign ones go through LDS and each folded row adds its helpers' sums in a
// fixed order (descending lane).  NRHS = 1: k_spmv (DOT as there); NRHS = 2: k_spmv2.
template <typename VT, int DOT, int NRHS>
// at most 5 waves per SIMD (96 VGPRs): with the default target of 6 (80 VGPRs) the scheduler issues the gathers of a
// trip's second slot only after the first slot's data has arrived -- one more dependent round trip per trip
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, (NRHS == 2 ? 4 : 5))))
k_spmv_fold(int32_t nslices, int64_t nloc, const int32_t *__restrict__ fold_ptr, const int32_t *__restrict__ rowof,
            const uint32_t *__restrict__ meta, const int32_t *__restrict__ cols, const VT *__restrict__ vals,
            const double *__restrict__ x, const double *__restrict__ x2, double *__restrict__ y, double *__restrict__ y2,
            double *partial, const int64_t *st, int64_t kiter, const int32_t *__restrict__ slist, int32_t nlist,
            int32_t poff, fold_args fold, colstream cs) {
    __shared__ double sh[4];
    __shared__ int sh_last;
    __shared__ double fsh[4][3 * NRHS][64];
    if (stopped(st, kiter)) { fold_skip(fold); return; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t bid = blockIdx.x;
    bid = xcd_chunked<32>(bid);
    const int64_t slice = slice_at(bid * 4 + w, slist, nlist, nslices);
    double y0 = 0, y1 = 0, yy2 = 0, z0 = 0, z1 = 0, z2 = 0;     // own row
    double f0 = 0, f1 = 0, f2 = 0, g0 = 0, g1 = 0, g2 = 0;      // the piece of a longer row this lane carries
    const int64_t row = row_at(slice, nslices, rowof, lane, nloc);
    uint32_t m = 0;
    if (slice < nslices) {
        m = meta[slice * 64 + lane];
        const int32_t own = (int32_t)(m & 0xffffu);
        const int32_t k0 = fold_ptr[slice], k1 = fold_ptr[slice + 1];
        const int32_t *cp = cols + (int64_t)k0 * 64 + lane;
        const VT *vp = vals + (int64_t)k0 * vstream<VT>::STRIDE + lane;
// LOAD then MATH for both slots of a trip: with the two accumulator sets the scheduler otherwise
// issued the gathers of a trip's SECOND slot only after the first slot's data had arrived (one more dependent round
// trip per trip: the folded kernel was 3-6 % slower than k_spmv at equal slot counts).
#define STAN_FOLD_LOAD(S, C, VP)                                                                \
        double a##S[9];                                                                         \
        load9<true, VT>(VP, a##S);                                                              \
        double x0##S = x[3 * (C)], x1##S = x[3 * (C) + 1], x2##S = x[3 * (C) + 2];              \
        double u0##S = 0, u1##S = 0, u2##S = 0;                                                 \
        if (NRHS == 2) { u0##S = x2[3 * (C)]; u1##S = x2[3 * (C) + 1]; u2##S = x2[3 * (C) + 2]; }
#define STAN_FOLD_MATH(S, KL)                                                                   \
    {                                                                                           \
        if (vstream<VT>::FX) { x0##S *= FX48_INV; x1##S *= FX48_INV; x2##S *= FX48_INV; }       \
        const double t0 = a##S[0] * x0##S + a##S[1] * x1##S + a##S[2] * x2##S;                  \
        const double t1 = a##S[3] * x0##S + a##S[4] * x1##S + a##S[5] * x2##S;                  \
        const double t2 = a##S[6] * x0##S + a##S[7] * x1##S + a##S[8] * x2##S;                  \
        const bool mine = (KL) < own;                                                           \
        y0 += mine ? t0 : 0.0; y1 += mine ? t1 : 0.0; yy2 += mine ? t2 : 0.0;                   \
        f0 += mine ? 0.0 : t0; f1 += mine ? 0.0 : t1; f2 += mine ? 0.0 : t2;                    \
        if (NRHS == 2) {                                                                        \
            if (vstream<VT>::FX) { u0##S *= FX48_INV; u1##S *= FX48_INV; u2##S *= FX48_INV; }   \
            const double s0 = a##S[0] * u0##S + a##S[1] * u1##S + a##S[2] * u2##S;              \
            const double s1 = a##S[3] * u0##S + a##S[4] * u1##S + a##S[5] * u2##S;              \
            const double s2 = a##S[6] * u0##S + a##S[7] * u1##S + a##S[8] * u2##S;              \
            z0 += mine ? s0 : 0.0; z1 += mine ? s1 : 0.0; z2 += mine ? s2 : 0.0;                \
            g0 += mine ? 0.0 : s0; g1 += mine ? 0.0 : s1; g2 += mine ? 0.0 : s2;                \
        }                                                                                       \
    }
        if (cs.packed && cs.ok[slice] == 1) {   // wave-uniform: the folded copy has its own packed column stream (modes 0 / 1)
            const uint32_t *cq = cs.packed + (int64_t)cs.pair_ptr[slice] * 64 + lane;
            const int32_t *bp = cs.base + __builtin_amdgcn_readfirstlane(k0);
            int32_t k = k0;
            // the packed offsets of a trip are loaded one trip ahead: both gathers of a trip can go out with its values
            uint32_t wd = __builtin_nontemporal_load(cq);
            for (; k + 1 < k1; k += 2) {
                const uint32_t wn = __builtin_nontemporal_load(k + 2 < k1 ? cq + 64 : cq);
                const int64_t c = (int64_t)bp[0] + (int64_t)(wd & 0xffffu);
                const int64_t c2 = (int64_t)bp[1] + (int64_t)(wd >> 16);
                STAN_FOLD_LOAD(A, c, vp)
                STAN_FOLD_LOAD(B, c2, vp + vstream<VT>::STRIDE)
                STAN_FOLD_MATH(A, k - k0)
                STAN_FOLD_MATH(B, k - k0 + 1)
                cq += 64;
                bp += 2;
                vp += 2 * vstream<VT>::STRIDE;
                wd = wn;
            }
            if (k < k1) {
                const int64_t c = (int64_t)bp[0] + (int64_t)(wd & 0xffffu);
                STAN_FOLD_LOAD(A, c, vp)
                STAN_FOLD_MATH(A, k - k0)
            }
        } else {
            int32_t k = k0;
            for (; k + 1 < k1; k += 2) {
                const int64_t c = __builtin_nontemporal_load(cp), c2 = __builtin_nontemporal_load(cp + 64);
                STAN_FOLD_LOAD(A, c, vp)
                STAN_FOLD_LOAD(B, c2, vp + vstream<VT>::STRIDE)
                STAN_FOLD_MATH(A, k - k0)
                STAN_FOLD_MATH(B, k - k0 + 1)
                cp += 128;
                vp += 2 * vstream<VT>::STRIDE;
            }
            if (k < k1) {
                const int64_t c = __builtin_nontemporal_load(cp);
                STAN_FOLD_LOAD(A, c, vp)
                STAN_FOLD_MATH(A, k - k0)
            }
        }
#undef STAN_FOLD_LOAD
#undef STAN_FOLD_MATH
    }
    // The exchange is wave-local (a slice is one wavefront): the LDS executes one wave's instructions in order, so
    // the reads below see the writes above without a workgroup barrier -- the four slices of a workgroup do not
    // wait for each other here; a slice without folded rows skips it altogether.
    const int nh = (int)(m >> 24);
    if (__any(nh > 0)) {
        fsh[w][0][lane] = f0; fsh[w][1][lane] = f1; fsh[w][2][lane] = f2;
        if (NRHS == 2) { fsh[w][3][lane] = g0; fsh[w][4][lane] = g1; fsh[w][5][lane] = g2; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int hfirst = (int)((m >> 16) & 0xffu);
        for (int h = 0; h < nh; h++) {   // a folded row: own part + its pieces, last lane first
            const int j = hfirst - h;
            y0 += fsh[w][0][j]; y1 += fsh[w][1][j]; yy2 += fsh[w][2][j];
            if (NRHS == 2) { z0 += fsh[w][3][j]; z1 += fsh[w][4][j]; z2 += fsh[w][5][j]; }
        }
    }
    if (slice < nslices && row < nloc) {
        store_row<true>(y, row, y0, y1, yy2);
        if (NRHS == 2) store_row<true>(y2, row, z0, z1, z2);
    }
    if (DOT) {
        double d = 0, e = 0;
        if (slice < nslices && row < nloc) dot_terms<DOT>(x, row, y0, y1, yy2, d, e);
        dot_reduce<DOT>(d, e, partial, poff, fold, sh, &sh_last);
    }
}
