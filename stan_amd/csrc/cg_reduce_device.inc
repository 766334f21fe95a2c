// cg_reduce_device.inc -- what every kernel of the CG shares: grid constants, the scalar / status slots, block sums, the folded reductions (fold_args, fold_arrive / fold_finish / fold_skip), stopped()
// Part of cg.hip (included there first, inside its anonymous namespace; not a translation unit of its own).

constexpr int VEC_BLOCKS = 2048;  // grid of the streaming vector kernels (8 blocks per CU; 1024 ... 16384 measured: profiles/r04/vector_grid_ab_in_cg.txt)
constexpr int VEC_T = 256;
constexpr int CHUNK = 32;         // iterations enqueued between two status polls
constexpr int CHUNK_DIST = 8;     // ... of a sharded loop

// device scalar slots (double)
enum { S_BNORM = 0, S_VMV = 1, S_R2NEW = 2, S_MERIT = 3, S_RHO0 = 4, S_RHO1 = 5, S_PMF0 = 6,
       S_PMF1 = 7, S_R2OUT = 8,
       // single-reduction loop: the three sums of one iteration are contiguous (ONE all-reduce)
       S_SR_GAMMA = 9, S_SR_DELTA = 10, S_SR_MERIT = 11, S_SR_GP0 = 12, S_SR_GP1 = 13, S_SR_AP0 = 14,
       S_SR_AP1 = 15,
       // fp64 check of a reduced-precision solve: ||b - A64 x||^2 and the merit sum of the same pass
       S_CHK_R2 = 16, S_CHK_MF = 17, S_NSCAL = 24 };
// device status slots (int64)
enum { T_ITER_A = 0, T_ITER_B = 1, T_TYPE = 2, T_ITERS = 3, T_XSEL = 4,
       T_FLUSHED = 5,   // STAN_OPT_CG_X_RING: the last term alpha_j p_j the iterate holds (k_xring_flush)
       T_NSTAT = 8 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// block sum (256 threads), valid in thread 0; fixed combination order
__device__ __forceinline__ double block_sum(double v, double *sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- reductions folded into their producers ("last block done") --------------------------------
// Every block of a producing kernel leaves its partial sum(s) in `partial`, then takes a ticket;
// the block that draws the last ticket adds ALL partials in a fixed order (independent of which
// block that is: the result is bit-reproducible) and writes the scalar.  That removes the two
// one-block k_reduce launches per iteration from the stream (2 x (4.5 us + a kernel boundary) at
// 148^3; more where it matters: the sharded loop, whose per-rank kernels are 8 x shorter).
// Hand-off across XCDs (their L2s are not coherent, MI355X_MICROARCH.md "inter-workgroup
// visibility", first row of the table of measured forms): the partial is an agent-scope store
// (sc1, write-through), the storing lane waits for it (vmcnt(0)) before its agent-scope add to
// the one unsharded counter, the block whose add returned the last ticket reads every partial
// with agent-scope (sc1) loads after a workgroup barrier behind that add.
// STAN_OPT_CG_FOLD_REDUCE = 0 restores the separate k_reduce launches (same order: same bits).
__device__ __forceinline__ void st_agent(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// r[j] = sum_i partial[i*NV + j] over np blocks by one 256-thread block, all NV sums in ONE pass
// over the partials (their loads overlap), fixed order; valid in thread 0
template <int NV>
__device__ __forceinline__ void sum_partials(const double *partial, int np, double *sh, double r[NV]) {
    constexpr int W = 16 / NV;   // loads in flight per thread: the last block's latency adds to the kernel
    double a[NV][W];
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
        for (int q = 0; q < W; q++) a[j][q] = 0;
    int i = threadIdx.x;
    for (; i + (W - 1) * 256 < np; i += W * 256) {
#pragma unroll
        for (int q = 0; q < W; q++)
#pragma unroll
            for (int j = 0; j < NV; j++) a[j][q] += ld_agent(partial + (int64_t)(i + q * 256) * NV + j);
    }
    for (; i < np; i += 256)
#pragma unroll
        for (int j = 0; j < NV; j++) a[j][0] += ld_agent(partial + (int64_t)i * NV + j);
#pragma unroll
    for (int j = 0; j < NV; j++) {
#pragma unroll
        for (int w = W / 2; w > 0; w >>= 1)   // fixed pairwise tree
#pragma unroll
            for (int q = 0; q < w; q++) a[j][q] += a[j][q + w];
        r[j] = block_sum(a[j][0], sh);
    }
}
// Tickets are two-level: block b first counts itself into sub-counter b % FOLD_SUB (a 128-B line
// of its own), the last arrival of a sub-counter counts that sub-counter into the top counter, the
// last arrival there finishes.  One flat counter cost k_step +10 us (rocprofv3, 148^3): its 2048
// blocks end together and 2048 adds to ONE address are served one after the other at the memory
// side; with 32 sub-counters the longest queue is 64.
constexpr int FOLD_SUB = 32;
constexpr int FOLD_LINE = 16;                               // uint64 per 128-B line
constexpr int FOLD_WORDS = (1 + FOLD_SUB) * FOLD_LINE;      // one counter set: top + sub-counters
struct fold_args {
    unsigned long long *counter;  // counter set (zero between kernels); nullptr: no fold
    unsigned nblocks;             // tickets this launch hands out (its grid size)
    int np;                       // partials to add (>= nblocks: earlier launches may have left some)
    double *out;                  // [NV] results
    p2p_out po;                   // sharded, peer to peer: the sums go to every rank's mailbox instead (p2p_device.h)
};
constexpr p2p_out NO_P2P = {nullptr, 0, 0, 0};
constexpr fold_args NO_FOLD = {nullptr, 0, 0, nullptr, NO_P2P};
// the finished sums r[0..NV) (valid in thread 0) to where the consumer will look for them
template <int NV>
__device__ __forceinline__ void publish_sums(double *out, const p2p_out &po, const double r[NV], double *sh) {
    if (po.pp) { p2p_publish<NV>(po, r, sh); return; }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; j++) out[j] = r[j];  // read by the NEXT kernel: a plain store will do
    }
}
// Thread 0 of every block calls this after storing its partials with st_agent(); true (in every
// thread) for the block that arrived last.  `sh_last` is one int of LDS.
__device__ __forceinline__ bool fold_arrive(const fold_args &f, int *sh_last) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU
        const unsigned sub = blockIdx.x % FOLD_SUB;
        const unsigned in_sub = (f.nblocks - sub + FOLD_SUB - 1) / FOLD_SUB;     // blocks b with b % SUB == sub
        const unsigned nsub = f.nblocks < (unsigned)FOLD_SUB ? f.nblocks : (unsigned)FOLD_SUB;
        int last = 0;
        unsigned long long t = __hip_atomic_fetch_add(f.counter + (1 + sub) * FOLD_LINE, 1ULL, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        if (t == (unsigned long long)in_sub - 1) {
            t = __hip_atomic_fetch_add(f.counter, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = t == (unsigned long long)nsub - 1;
        }
        *sh_last = last;
    }
    __syncthreads();
    return *sh_last != 0;
}
template <int NV>
__device__ __forceinline__ void fold_finish(const fold_args &f, const double *partial, double *sh) {
    double r[NV];
    sum_partials<NV>(partial, f.np, sh, r);
    publish_sums<NV>(f.out, f.po, r, sh);
    // every ticket of this launch has been drawn: clear the set for the next one
    if (threadIdx.x <= FOLD_SUB)
        __hip_atomic_store(f.counter + threadIdx.x * FOLD_LINE, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A producing kernel that returns without doing its work (the solve has stopped; every rank takes the same
// decision) still owes its peers the arrival count of its reduction: their streams wait for it.
__device__ __forceinline__ void fold_skip(const fold_args &f) {
    if (f.counter && f.po.pp && f.po.signal && blockIdx.x == 0 && (int)threadIdx.x < f.po.pp->n)
        __hip_atomic_fetch_add(f.po.pp->sig_red[threadIdx.x][f.po.slot], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ bool stopped(const int64_t *st, int64_t k) {
    return st[T_ITER_A] < k || st[T_ITER_B] < k;
}
