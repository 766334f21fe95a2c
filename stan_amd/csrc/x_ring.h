// x_ring.h -- slot and window arithmetic of the ring of search directions (STAN_OPT_CG_X_RING), shared by the host loop
// that enqueues the kernels (cg.hip: cg_run::iterate) and the kernel that sums the pending terms (cg_vector_kernels.inc:
// k_xring_flush).  With the merit stop off nothing reads the iterate between two residual refreshes, so the loop keeps the
// directions p_j and the step lengths alpha_j of a window in a ring of W + 1 slots and forms
//   x_last = fma(alpha_last, p_last, ... fma(alpha_first, p_first, x_{first-1}) ...)
// once per window, in iteration order: the same fused multiply-adds in the same order as one per iteration, the same bits.
// Three questions are answered here: which slot holds p_j, which terms a flush in front of iteration k sums, and which
// terms the closing flush sums for the status words a solve ended with.
// Plain C++ as well as HIP: the host-side check of this arithmetic compiles this file with a sanitizer.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XRING_FN __host__ __device__ __forceinline__
#else
#define XRING_FN inline
#endif

constexpr int XRING_MAX_W = 16;   // longest window: the flush kernel holds one load per term in flight

// W: the refresh period (STAN_OPT_CG_RUPDATE) where a window of that length fits, 10 where there is no refresh or a longer period
XRING_FN int xring_window(int64_t rupdate) { return rupdate >= 2 && rupdate <= XRING_MAX_W ? (int)rupdate : 10; }

// p_j, the direction iteration j multiplies, and alpha_j live in slot j mod (W + 1): while iteration k writes p_{k+1} the
// ring still holds p_{k-W+1} ... p_k, the most that can be pending (xring_flush_due)
XRING_FN int xring_slot(int64_t j, int W) { return (int)(j % (W + 1)); }

// A flush in front of iteration k sums the terms flushed + 1 ... k - 1 (flushed: the last term summed so far, 0 at the
// start).  It is due when iteration k refreshes the residual -- its product multiplies x_{k-1} -- and when the slot
// iteration k writes (p_{k+1}) still holds a pending term (p_{k-W}).
XRING_FN bool xring_flush_due(int64_t k, int64_t flushed, int W, bool refresh) { return refresh || k - flushed > W; }

// The iterate a solve returns, from its status words: T_TYPE, T_ITERS, T_XSEL (the parity of the iterate's number: types 1,
// 5 and a -4 of k_update select x_k, a -5 / -4 stop of k_step selects x_{k-1}); type 0: the hard cap of the iteration
// counter ended the loop, every enqueued iteration ran.  The closing flush sums the terms flushed + 1 ... this.
XRING_FN int64_t xring_final_iterate(int64_t type, int64_t iters, int64_t xsel, int64_t last_enqueued) {
    if (type == 0) return last_enqueued;
    return ((iters ^ xsel) & 1) == 0 ? iters : iters - 1;
}
