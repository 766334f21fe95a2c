// internal.h -- shared declarations of libstan_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/stan_hip.h"

#define STAN_SLICE 64      // block rows per ELL slice == wavefront width
#define STAN_MAX_INCIDENT 64  // (element,local node) pairs per node of the FAST symbolic kernel (one lane each); more: k_symbolic_big
#define STAN_MAX_ROW_BLOCKS 96 // slice width (blocks per row) of the FAST numeric kernel's LDS accumulators; wider slices: k_numeric_wide

// HIP call guard: records the error on the context and returns STAN_E_HIP.
#define HIPCHK(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);            \
            return (e_ == hipErrorOutOfMemory) ? STAN_E_ALLOC : STAN_E_HIP;            \
        }                                                                              \
    } while (0)

#define STANCHK(call)                 \
    do {                              \
        int rc_ = (call);             \
        if (rc_ != STAN_OK) return rc_; \
    } while (0)

// RCCL entry points, resolved with dlopen at comm_init (no link-time dependency so the
// library loads on a host without RCCL / without a GPU).
struct rccl_api {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, const void *, int) = nullptr;  // ncclUniqueId by value
    int (*CommDestroy)(void *) = nullptr;
    int (*CommAbort)(void *) = nullptr;   // optional: frees ranks blocked in a collective (multi.hip)
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;          // optional
    int (*CommCount)(void *, int *) = nullptr;   // optional
    int (*CommUserRank)(void *, int *) = nullptr;
    std::string path;      // the file the entry points live in (dladdr)
    bool reused = false;   // it was already mapped in this process (RTLD_NOLOAD): no second RCCL next to the host's
};

// Device blocks of 8 MB and more are kept by the context when they are freed and handed out again
// to the next request they fit (best fit, at most 1.5x the size asked for): on this stack a
// hipMalloc of tens of GB right after the hipFree of as much takes 0.4-1.8 s, erratically -- at
// 200^3 more than the whole assembly (12 + 32 ms) and 10-25 % of a step (tools/alloc_probe.py).
// Reuse is ordered by the context's stream, so no synchronisation is needed; a failed hipMalloc
// flushes the pool and retries; STAN_OPT_POOL = 0 flushes and disables; destroy frees everything.
struct stan_pool {
    static constexpr size_t MIN_BYTES = 8u << 20;
    static constexpr size_t MAX_BLOCKS = 64;   // parked blocks; one assemble + solve parks ~30
    size_t max_bytes = (size_t)64 << 30;       // parked bytes (STAN_OPT_POOL_MAX_BYTES; init: half the device); oldest go first
    struct blk { void *p; size_t cap; };
    std::vector<blk> avail;
    std::unordered_map<void *, size_t> live;  // pooled-class blocks currently handed out
    bool enabled = true;
    size_t bytes_avail = 0;
    void flush() {
        for (blk &b : avail) hipFree(b.p);
        avail.clear();
        bytes_avail = 0;
    }
};

// events owned by one call: destroyed on every exit path
struct event_bag {
    std::vector<hipEvent_t> ev;
    hipEvent_t make(unsigned flags = hipEventDefault) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, flags) == hipSuccess) ev.push_back(e);
        return e;
    }
    ~event_bag() { for (hipEvent_t e : ev) hipEventDestroy(e); }
};

// Slots of stan_ctx::d_status (device) and ::h_status (pinned host mirror), 64 x int64 each.
// Device and host copies of a slot are not always the same quantity: the host side also parks
// scan totals it copies back (SS_H_*).
enum stan_status_slot {
    SS_ERRBITS = 0,      // device: ERR_* bit mask raised by the assembly kernels
    SS_H_NINC = 1,       // host: total node-element incidences
    SS_H_NHALO = 2,      // host: halo block columns of this rank
    SS_H_NSLOTS = 3,     // host: ELL slots (slot_ptr total)
    SS_H_NBLOCKS = 4,    // host: blocks, followed by
    SS_H_MAXROW = 5,     //       the longest row (copied as a pair from SS_WIDTH_SUM / SS_WIDTH_MAX)
    SS_H_COUNT_A = 6,    // host: scan totals (boundary slices, send rows ...)
    SS_H_COUNT_B = 7,    // host: scan totals (interior slices)
    SS_BAD_ELEM = 8,     // min element index with det J == 0 (LLONG_MAX = none)
    SS_AUX = 9,          // fixed-DOF count (assembly) / first HEX8_G1 element (recovery)
    SS_COUNTER = 10,     // FIXED-48 overflow count; colouring: elements still uncoloured (host)
    SS_H_ERRCOPY = 11,   // host: copy of SS_ERRBITS during the colouring rounds
    SS_MAXDEG = 12,      // device + host: most (element, local node) incidences of one owned row when > STAN_MAX_INCIDENT, else 0
    SS_NGIANT = 13,      // device + host: rows whose symbolic sort does not fit the LDS allotment (global scratch)
    SS_NBIG = 14,        // device + host: rows with more than STAN_MAX_INCIDENT incidences (k_symbolic_big's grid)
    SS_WIDTH_SUM = 16,   // device: sum of row lengths, followed by
    SS_WIDTH_MAX = 17,   //         the longest row (k_slice_width)
    SS_H_CG_STATUS = 16, // host: two 8-word copies of the CG status words (chunk polling)
    SS_H_CG_SCALARS = 40 // host: the CG scalars at the end of a solve
};

// Vectors of the CG, kept by the context between solves (cg_workspace.hip: stan_cg_workspace).  They are
// allocated BEFORE the value stream of K is placed by search, and the search's probe multiplies
// with exactly these buffers: whether a block streams fast depends on the PAIR (value block,
// vector block) -- profiles/r02/PLACEMENT.md -- so the pair that is timed is the pair that runs.
struct stan_cg_ws {
    int64_t ng = 0, n3 = 0;        // capacities: gather-sized (owned + pad + halo) / owned-sized, in doubles
    double *xb[2] = {nullptr, nullptr}, *p = nullptr, *r = nullptr;   // ng each
    double *v = nullptr, *w = nullptr, *bh = nullptr, *sv = nullptr;  // n3 each
    double *vw_owner = nullptr;    // non-null: v and w are carved out of this one block (placement.hip, second stage): it is what gets freed
    // the eight vectors, i = 0 .. NVEC - 1 in the order they are allocated: where the pointer is kept, and which capacity it has
    static constexpr int NVEC = 8;
    struct slot { double **q; bool gather; };
    slot vec(int i) {
        double **const all[NVEC] = {&xb[0], &xb[1], &p, &r, &v, &w, &bh, &sv};
        return slot{all[i], i < 4};
    }
};

// ---- peer-to-peer exchanges of the one-process multi-GPU handle (p2p.hip) ---------------------
// All devices of a group handle live in ONE address space, so the sharded CG needs no RCCL launch
// in its loop: the block that finishes a reduction stores its partial sums into EVERY rank's
// mailbox and then counts itself into every rank's arrival counter; the consumer's stream waits
// for the count (a one-wave polling kernel, or hipStreamWaitValue64: p2p.hip) and the consuming kernel adds the
// partials of all ranks in rank order (the result is the same on every rank, bit for bit, and
// the same as a rank-ordered all-reduce gives).  Halo rows are written straight into the
// neighbour's gather vector, followed by the same kind of count.
constexpr int STAN_P2P_RING = 4;    // mailbox slots / counters in rotation (a rank is never two exchanges ahead)
constexpr int STAN_P2P_MAXR = 16;   // ranks of a group that can exchange peer to peer
struct stan_p2p_dev {               // device-resident, one copy per rank
    int32_t n, me;
    double *mbox[STAN_P2P_MAXR];    // rank q's mailbox [RING][n][4] doubles, fine-grained device memory of q
    unsigned long long *sig_red[STAN_P2P_MAXR][STAN_P2P_RING];   // reduction arrivals at rank q
    unsigned long long *sig_halo[STAN_P2P_MAXR][STAN_P2P_RING];  // halo arrivals at rank q
};
struct stan_p2p {                   // host side, shared by the ranks of a group (owned by multi.hip)
    int n = 0;
    int wait_mode = 1;              // STAN_P2P_WAIT_MODE: 1 (default) a one-wave polling kernel; 0 hipStreamWaitValue64; 2 reductions polled by the consuming kernel itself
    struct rank_res {
        int device = 0;
        double *mbox = nullptr;
        unsigned long long *sig_red[STAN_P2P_RING] = {}, *sig_halo[STAN_P2P_RING] = {};
        stan_p2p_dev *d_dev = nullptr;       // this rank's device copy of the table
        unsigned long long *d_tick = nullptr; // ticket counter of the halo-pack kernel (device)
        int64_t red_calls = 0, halo_calls = 0;   // exchanges so far (identical on every rank)
        unsigned long long red_expect[STAN_P2P_RING] = {}, halo_expect[STAN_P2P_RING] = {};   // arrivals each counter must have reached
        // published at the start of a solve (host barrier behind it): where my neighbours write
        double *vec[5] = {};                 // xb0, xb1, p, r, scale
        int64_t nloc = 0;
        std::vector<int> nbr;
        std::vector<int64_t> recv_off;
    };
    std::vector<rank_res> rk;
    // process-per-GPU form (stan_p2p_ipc_setup): this process owns ONE rank; the other ranks' mailboxes,
    // counters and vectors are device memory of other processes mapped through HIP IPC handles, which the
    // ranks exchange over the RCCL communicator they already have (no change to the host application)
    bool ipc = false;
    int ipc_me = -1;
    void *ipc_block = nullptr;                     // own mailbox + counters: one fine-grained allocation, one handle
    std::vector<void *> ipc_peer_block;            // mapped blocks of the peers
    std::unordered_map<std::string, void *> ipc_open;   // vectors of peers mapped so far, by handle bytes
    std::unordered_set<std::string> ipc_live;           // ... of which the peers published these in the current solve
    // host barrier of the worker threads (abortable)
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    long generation = 0;
    std::atomic<bool> broken{false};
};
int stan_p2p_create(stan_p2p **out, const std::vector<int> &devices, std::string *err);   // called with no worker running
int stan_p2p_rank_setup(stan_p2p *pp, int rank, std::string *err);    // from rank's own thread (its device current)
int stan_p2p_rank_finish(stan_p2p *pp, int rank, std::string *err);   // after every rank's setup: uploads the table
void stan_p2p_rank_release(stan_p2p *pp, int rank);
void stan_p2p_destroy(stan_p2p *pp);
void stan_p2p_abort(stan_p2p *pp);                 // frees every stream wait and every host barrier
void stan_p2p_dump(stan_p2p *pp, FILE *f);         // call counts, expected and actual arrivals of every counter
int stan_p2p_barrier(stan_p2p *pp);                // STAN_E_COMM when aborted / timed out
// Host waits of a peer-to-peer solve are BOUNDED: a stream of this rank that makes no progress for
// stan_p2p_stall_seconds() (a peer died or never published) gets its waits released -- the IPC form releases the
// counters this rank waits on (its own memory), the one-process form every rank's -- the exchange is marked broken
// and the solve returns STAN_E_COMM instead of blocking in hipStreamSynchronize with a spinning queue.
double stan_p2p_stall_seconds();                   // STAN_P2P_STALL_S, default 120
void stan_p2p_release_own(stan_ctx *ctx);          // RELEASE_ALL into this rank's own arrival counters + broken
struct stan_ctx;
int stan_p2p_ipc_setup(stan_ctx *ctx);             // collective over the context's RCCL communicator
void stan_p2p_ipc_release(stan_ctx *ctx);
void stan_p2p_ipc_trim(stan_ctx *ctx);             // end of a solve: close the mappings no peer published this time
struct stan_matrix;
int stan_p2p_reduce_slot(stan_ctx *ctx);           // mailbox slot / counter of this rank's NEXT reduction
int stan_p2p_reduce_wait(stan_ctx *ctx, const unsigned long long **ctr = nullptr, unsigned long long *want = nullptr);   // the wait for it (advances the slot): enqueued, or (wait mode 2, ctr / want given) left to the consuming kernel
const stan_p2p_dev *stan_p2p_table(stan_ctx *ctx);
const double *stan_p2p_mailbox(stan_ctx *ctx, int slot);
int stan_p2p_publish_vectors(stan_ctx *ctx, const stan_matrix *K, double *const vec[5]);
int stan_p2p_halo_exchange(stan_ctx *ctx, stan_matrix *K, double *d_vec);

struct stan_matrix;
struct stan_group;   // multi.hip: one process, several GPUs
struct stan_ctx {
    stan_group *group = nullptr;  // set on the handle stan_hip_init_multi returns: the calls fan out
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    int64_t bad_elem = -1;
    // communicator
    int rank = 0, nranks = 1;
    void *comm = nullptr;      // guarded by comm_mu: the group's host thread may abort it (multi.hip)
    std::mutex comm_mu;
    std::atomic<bool> comm_broken{false};  // the communicator was aborted after a peer failed: no further collectives
    rccl_api nccl;
    stan_p2p *p2p = nullptr;   // set on the rank contexts of a group whose devices can reach each other
    bool comm_p2p = false;     // STAN_OPT_COMM_P2P: the CG's reductions and halo exchanges go peer to peer
    bool result_segment = false;  // group rank: the solve leaves only this rank's own entries of U (no gather)
    // hipFree waits for EVERY stream of the device.  Inside a peer-to-peer solve the other ranks' streams hold
    // waits for exchanges this rank has not issued yet; when ranks share a device (the test topology) a hipFree
    // in the middle of the solve therefore never returns (found as a stall in 7 of 32 runs: the stall dump showed
    // every expectation of the stuck ranks met -- they sat in the hipFree of a temporary).  Blocks released
    // during such a solve are kept and freed when it has ended (stan_cg_device).
    bool defer_frees = false;
    bool peers_share_device = false;   // group rank whose device also carries another rank of the process (multi.hip): frees deferred on every transport
    std::vector<void *> deferred;
    // solver options (include/stan_hip.h STAN_OPT_*)
    bool cg_merit_stop = true;
    int cg_rupdate = 10;
    bool cg_fused_refresh = true;  // A x and A p of a refresh iteration in one matrix pass
    bool cg_single_reduce = false; // Chronopoulos-Gear loop: one reduction point per iteration
    int64_t spmv_small_rows = 150000;   // systems of at most this many block rows: one workgroup per slice (k_spmv_small); 0 = never
    bool cg_defer_x = true;        // merit stop off: x' = x + a p is formed by k_update (one read of p)
    bool cols16 = true;            // SpMV reads the packed column stream where a slice allows it
    int vec_store_nt = 3;          // bit 0: p (k_update), bit 1: r (k_step) leave through non-temporal stores
    bool cg_fold_reduce = true;    // reductions finished by the producing kernel's last block
    bool cg_lazy_scaling = true;   // STAN_OPT_CG_LAZY_SCALING: the first product of the loop brings K into its scaled form (k_spmv_first)
    int cg_refine = 1;             // STAN_OPT_CG_REFINE: reduced-precision streams -- 0 fp64 check only, 1 + refinement passes, 2 + fp64 refresh products
    bool overlap_halo = true;  // interior SpMV on a side stream while the halo is exchanged
    hipStream_t side = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int assembly_mode = 0;     // 0 row-owner gather (default), 1 element-wave colour scatter
    int row_folding = -1;      // STAN_OPT_ROW_FOLDING: -1 = products read the folded streams (fold.hip) when they save > 5 % of the slots; 1 always; 0 never
    int sell_sigma = 1;        // SELL-C-sigma: rows sorted by length inside windows of this many slices (1: inside each slice only)
    int placement_tries = 16;  // > 1: allocate the value stream by search (placement.hip); blocks >= 256 MB only
    int64_t placement_max_bytes = 0;  // bytes of candidates the search may hold at once; 0 = a quarter of the free memory
    float prof_placement_ms_best = 0, prof_placement_ms_worst = 0;
    int prof_placement_candidates = 0;
    int prof_placement_moved_vectors = 0;   // 1: the search ended by re-allocating the CG's vectors
    int prof_colours = 0;
    int spmv_variant = -1; // -1 = auto (plan_products picks per value stream); >= 0: A/B lab
    int value_stream_60 = -1;  // STAN_OPT_VALUE_STREAM_60: -1 = the fp64 loop of a large system on one rank streams the 60-bit values; 1 always where k_spmv runs; 0 never
    int cg_x_ring = -1;        // STAN_OPT_CG_X_RING: where k_update defers x, x is formed once per refresh window from a ring of directions (x_ring.h); -1 = above 150 000 block rows; 1 always there; 0 never
    int prof_x_ring_window = 0;        // last solve: the ring's window W (0: the loop formed x every iteration) ...
    int64_t prof_x_ring_flushes = 0;   // ... and the flush launches it enqueued (stan_hip_cg_loop_info)
    int cg_refresh_60 = -1;    // STAN_OPT_CG_REFRESH_60: where the plain products of a solve read the 60-bit stream its fused refresh passes do too; -1 = above 150 000 block rows; 1 always there; 0 never
    int prof_refresh_stream = -1;      // last solve: the value stream its fused refresh passes read (-1: none ran)
    // profiling
    bool profiling = false;
    stan_profile prof{};
    double prof_loads_ms[3] = {0, 0, 0};   // last load-vector call: element pass | lists | gather (stan_hip_load_vector_times)
    double prof_thermal_ms[3] = {0, 0, 0}; // last thermal-load call, the same phases (stan_hip_thermal_load_times)
    double prof_cm_ms[4] = {0, 0, 0, 0};   // last consistent-mass call, the same four phases (stan_hip_consistent_mass_times)
    double prof_axpy_ms = 0;               // last stan_hip_matrix_axpy: the value pass
    double prof_kg_ms[4] = {0, 0, 0, 0};   // last geometric-stiffness call: element pass | layout copy | lists and maps | gather (stan_hip_geometric_stiffness_times)
    stan_pool pool;
    stan_cg_ws ws;
    std::vector<stan_matrix *> matrices;  // alive matrices of this context (detached when it is destroyed)
    // small pinned host + device scratch for status words
    int64_t *h_status = nullptr;  // pinned, 64 words
    int64_t *d_status = nullptr;  // device, 64 words
};
// a rank of a sharded matrix: halo exchanges and all-reduces belong to every product and reduction
inline bool stan_sharded(const stan_ctx *ctx) { return ctx->comm != nullptr || ctx->nranks > 1; }

// A value stream of K.  Kinds: STAN_PREC_FP64 (the assembled values, scaled in place), STAN_PREC_MIXED (fp32 copy),
// STAN_PREC_FIXED48 and STAN_VALUE_STREAM_60 (copies of the SCALED values; s60.h: 17 rows); layout [slot][dwords][64].
constexpr int STAN_NSTREAMS = 4;
struct stan_value_stream {
    int dwords;               // dwords per slot and lane
    void *padded = nullptr;   // [nslots] slots
    void *folded = nullptr;   // [nfslots] slots, built on demand (fold.hip); the 60-bit stream has none
    bool refused = false;     // some scaled entry is outside the format's range (FIXED-48: |a_ij| >= 2, K not SPD; 60-bit: also below 2^-126 or not finite): fp64 is streamed
};
// A packed column stream (struct colstream of spmv_kernels.inc, stan_pack_columns): of the padded layout, and of the folded one
struct stan_colpack {
    uint32_t *cols16 = nullptr;   // [pair][64]
    int32_t *colbase = nullptr;   // [slots] smallest column of each slot (+ second bases and class masks: make_colstream)
    int32_t *pair_ptr = nullptr;  // [nslices+1]
    uint8_t *packed = nullptr;    // [nslices] mode of the slice (k_pack_cols): 0 = not in the packed stream
    int64_t slots_packed = 0;     // ELL slots of packed slices (modes 1 and 2) ...
    int64_t slots_packed2 = 0;    // ... of which in two-base slices (4 B more per slot: the second base)
};

struct stan_matrix {
    stan_ctx *ctx = nullptr;
    std::vector<stan_matrix *> parts;  // group matrix (multi.hip): the shard of each device
    int64_t n_dof = 0, n_red = 0;
    int64_t nb_glob = 0;  // global block rows
    int64_t r0 = 0, r1 = 0;  // owned block rows
    int64_t u0 = 0, u1 = 0;  // group shard: this rank's entries [u0, u1) of the reduced vectors
    int64_t nloc = 0, nhalo = 0;
    int32_t nslices = 0;
    int64_t nslots = 0;      // total k-slots (each = 64 rows x one block)
    int64_t nblocks = 0;     // structural blocks on this rank
    int32_t max_row_blocks = 0;
    int64_t n_elem_scanned = 0;  // elements this rank holds on the device (sharded host entry: its subset)
    int32_t *d_slot_ptr = nullptr;  // [nslices+1]
    int32_t *d_rowlen = nullptr;    // [nslices*64] blocks per row (by local row)
    int32_t *d_rowof = nullptr;     // [nslices*64] SELL-C-sigma: position in the sliced layout -> local block row
    int32_t *d_posof = nullptr;     // [nslices*64] local block row -> position (slice = pos / 64, lane = pos % 64)
    int sigma = 1;                  // sorting window in slices the matrix was built with
    int32_t *d_cols = nullptr;      // [nslots][64] local block-column index
    stan_colpack pk;                // packed column stream of d_cols
    stan_value_stream vs[STAN_NSTREAMS] = {{9 * 2}, {9}, {14}, {17}};   // the value streams by kind; [STAN_PREC_FP64].padded: the assembled values
    double *vals64() const { return (double *)vs[STAN_PREC_FP64].padded; }   // [nslots][9][64]
    // Folded copy of the streams (fold.hip, STAN_OPT_ROW_FOLDING): long rows lend their tails to the idle slots of
    // the short rows of their slice; padded-slot layout with ~blocks/64 slots per slice.
    int32_t *d_fold_ptr = nullptr;      // [nslices + 1] first folded slot of every slice
    uint32_t *d_fold_meta = nullptr;    // [nslices * 64] own slots (16 bits) | first helper lane << 16 | helper lanes << 24
    int4 *d_fold_plan = nullptr;        // [nslices * 64] own slots, owner lane (-1), offset in the owner's row, slots taken
    int32_t *d_fold_cols = nullptr;     // [nfslots][64]
    stan_colpack fold_pk;               // packed column stream of d_fold_cols (one base per slot)
    int64_t nfslots = 0;
    bool fold_cols_filled = false;
    int fold_state = 0;                 // 0: not examined, 1: planned, -1: not applicable / abandoned (no memory), -2: declined by the auto threshold (> 95 % of the slots)
    int32_t *d_red = nullptr;       // [n_dof] nDOF_reduction
    uint8_t *d_fixmask = nullptr;   // [nb_glob] bit m = DOF m of the node fixed
    double *d_scale = nullptr;      // [3*(nloc+nhalo)] s_i = 1/sqrt(K_ii)
    bool scaled = false;
    // halo plan (all index lists on device, counts on host)
    std::vector<int> nbr;             // neighbour ranks
    std::vector<int64_t> send_off;    // [nbr+1] offsets into d_send_rows
    std::vector<int64_t> recv_off;    // [nbr+1] offsets into the halo region (block cols)
    int32_t *d_send_rows = nullptr;   // local block rows to pack, grouped by neighbour
    int32_t *d_halo_glob = nullptr;   // [nhalo] global block index of each halo column
    double *d_sendbuf = nullptr;      // [3*send_total]
    std::vector<int64_t> row_starts;  // [nranks+1] partition
    // slices whose rows reference no halo column (interior) / at least one (boundary)
    int32_t *d_sl_int = nullptr, *d_sl_bnd = nullptr;
    int32_t n_sl_int = 0, n_sl_bnd = 0;
};

// contiguous block-row partition of the sharded system, cut on slice (64-row) boundaries:
// rank r owns [row_start(r), row_start(r+1)) of the nb block rows (reference DOF order)
static inline int64_t stan_row_start(int64_t nb, int nranks, int r) {
    if (r >= nranks) return nb;
    const int64_t nsl = (nb + 63) / 64;
    const int64_t s = nsl * r / nranks * 64;
    return s > nb ? nb : s;
}

// ---- the mesh, as every layer below the C ABI passes it on ---------------------------------------------------------------
// A view: plain pointers and counts, nothing owned.  ONE type for both sides of the upload -- a HOST view holds the caller's
// arrays (a public entry builds it behind its checks), a DEVICE view their copies in device memory (mesh_dbufs of api_stage.h makes
// it, a _dev entry builds it from its arguments, the stan_*_device drivers take it); mat_E_nu is a host array in both.
// May be null: disp, node_dof and red where the entry has no such array (n_dof is 0 where it is not passed either); conn,
// elem_mat and elem_type only where n_elem == 0.  Built with designated initialisers, so that no array is passed by position.
struct stan_mesh {
    int64_t n_nodes = 0, n_elem = 0, n_dof = 0;
    int32_t n_mat = 0;
    const double *xyz = nullptr, *disp = nullptr;   // [n_nodes][3]
    const int32_t *node_dof = nullptr;              // [n_nodes][3]
    const int32_t *conn = nullptr;                  // [n_elem][8]
    const int32_t *elem_mat = nullptr;              // [n_elem]
    const uint8_t *elem_type = nullptr;             // [n_elem]
    const int32_t *red = nullptr;                   // [n_dof]
    const double *mat_E_nu = nullptr;               // [n_mat][2], host
    // the elements [e0, e1) of a mesh that has some: the element arrays start at e0, the node arrays stay whole
    stan_mesh chunk(int64_t e0, int64_t e1) const {
        stan_mesh c = *this;
        c.n_elem = e1 - e0; c.conn = conn + 8 * e0; c.elem_mat = elem_mat + e0; c.elem_type = elem_type + e0;
        return c;
    }
};

// ---- scan.hip -------------------------------------------------------------------------------
// out[i] = sum_{j<i} in[j] (int32 in, int64 out), out has n+1 entries (out[n] = total).
int stan_scan_exclusive(stan_ctx *ctx, const int32_t *d_in, int64_t *d_out, int64_t n);
// ... and the total on its way to the pinned h_status[slot] (valid after the caller's next synchronisation).
int stan_scan_total(stan_ctx *ctx, const int32_t *d_in, int64_t *d_out, int64_t n, int slot);
// Flags -> the ascending list of the flagged indices: stan_scan_total(d_flag -> d_rank), a synchronisation (one may serve
// several lists), then collect: reads the count, allocates *out (a temporary of `tmp`, or the caller's) and fills it.
struct dev_scope;
int stan_compact_collect(stan_ctx *ctx, const int32_t *d_flag, const int64_t *d_rank, int64_t n, int slot, int32_t **out, int64_t *count, dev_scope *tmp = nullptr);
int stan_compact_flags(stan_ctx *ctx, const int32_t *d_flag, int64_t *d_rank, int64_t n, int slot, int32_t **out, int64_t *count, dev_scope *tmp = nullptr);   // all three
// Widths -> int32 slot pointers: stan_scan_total(d_width -> d_ptr64), then (behind a synchronisation when the total
// must be checked first) narrow: allocates *d_ptr32[n + 1], the caller's, and fills it.
int stan_slot_ptr_narrow(stan_ctx *ctx, const int64_t *d_ptr64, int64_t n, int32_t **d_ptr32);

// ---- assembly.hip ---------------------------------------------------------------------------
int stan_assemble_device(stan_ctx *ctx, const stan_mesh &d, stan_matrix **outK);   // d: device view with node_dof and red
int stan_ke_batch_device(stan_ctx *ctx, int64_t n, const double *d_xyz8, double E, double nu,
                         const uint8_t *d_type, double *d_out);

// ---- assembly_scatter.hip ---------------------------------------------------------------------
int stan_assemble_colour_scatter(stan_ctx *ctx, stan_matrix *K, int64_t n_elem, const int32_t *d_conn,
                                 const int32_t *d_perm, const double *d_xyz, const int32_t *d_elem_mat,
                                 const uint8_t *d_elem_type, const double *d_lamG, const int64_t *d_ptr,
                                 const int32_t *d_list, long long *d_bad);

// ---- cg.hip ---------------------------------------------------------------------------------
int stan_cg_device(stan_ctx *ctx, stan_matrix *K, const double *d_F, double eps_f,
                   int32_t max_its, int32_t precision_mode, double *d_U, int32_t *term,
                   int32_t *iters, double *rel_res);
// n_rhs load vectors, one loop over a single pass of K per group of columns (cg.hip, cg_multi.inc); d_F, d_U: [n_rhs][n_red]
int stan_cg_multi_device(stan_ctx *ctx, stan_matrix *K, int32_t n_rhs, const double *d_F, double eps_f, int32_t max_its,
                         int32_t precision_mode, double *d_U, int32_t *term, int32_t *iters, double *rel_res);
int stan_spmv_reduced(stan_ctx *ctx, stan_matrix *K, const double *d_x, double *d_y);
// The product of a loop that keeps its vectors resident (cg_entries.inc): yf = A^ xf on caller-held vectors in the padded full
// numbering (3 * nslices * 64 doubles; index 3 * row + m; A^ = S K S once K->scaled), ONE plain fp64 product by the plan a
// solve gets; rows of padding are not stored.  Enqueues only.  stt: the status words of stan_product_status (a temporary of
// `tmp`, filled on the stream), made once per loop.  Single rank.
int stan_product_status(stan_ctx *ctx, dev_scope &tmp, int64_t **stt);
int stan_product_full(stan_ctx *ctx, stan_matrix *K, const double *xf, double *yf, const int64_t *stt);
int stan_matrix_diagonal(stan_ctx *ctx, stan_matrix *K, double *d_diag);
int stan_spmv_bench_device(stan_ctx *ctx, stan_matrix *K, int32_t precision_mode, int32_t reps,
                           double *avg_ms);
int stan_stream_bench_device(stan_ctx *ctx, stan_matrix *K, int32_t reps, double *avg_ms, int64_t *bytes);
int stan_spmv_local(stan_ctx *ctx, stan_matrix *K, const double *d_x, double *d_y);
int stan_matrix_make_fp32(stan_ctx *ctx, stan_matrix *K);
// ---- fold.hip -------------------------------------------------------------------------------
int stan_matrix_make_folded(stan_ctx *ctx, stan_matrix *K, int32_t stream_kind, bool plan_only = false);
void stan_matrix_drop_folded_values(stan_ctx *ctx, stan_matrix *K);
void stan_matrix_abandon_folding(stan_ctx *ctx, stan_matrix *K);
int stan_matrix_make_fx48(stan_ctx *ctx, stan_matrix *K);
int stan_matrix_alloc_stream(stan_ctx *ctx, stan_matrix *K, int32_t kind, int64_t slots, void **out, bool folded = false, bool second_copy = false);   // folded: a block of the folded layout; second_copy: see stan_dmalloc_streamed
int stan_matrix_alloc_s60(stan_ctx *ctx, stan_matrix *K, uint32_t **out);   // a block for K's 60-bit stream, allocated by search like K's values; *out = nullptr (STAN_OK): no room within the budgets
int stan_stream_encode(stan_ctx *ctx, int32_t kind, int64_t nslots, const double *d_vals, uint32_t *d_out, int64_t *refused);   // FIXED-48 or 60-bit; synchronises the stream
int stan_matrix_encode_s60(stan_ctx *ctx, stan_matrix *K, uint32_t *blk);   // blk becomes K's 60-bit stream, or -- an entry refused -- is freed
int stan_stream60_roundtrip_device(stan_ctx *ctx, int64_t n, const double *in, double *out, int64_t *refused);   // cg_entries.inc
int stan_matrix_make_cols16(stan_ctx *ctx, stan_matrix *K);
int stan_pack_columns(stan_ctx *ctx, int32_t nslices, int64_t nslots, const int32_t *d_slot_ptr, const int32_t *d_cols, stan_colpack *out,
                      int64_t nloc = 0, const int32_t *d_rowof = nullptr, const int32_t *d_rowlen = nullptr);
int stan_matrix_ensure_scaled(stan_ctx *ctx, stan_matrix *K);   // S K S in place (once per matrix)
// length of a gather vector of K (NOTE on the halo layout, cg.hip): the owned rows padded to whole slices, or the owned
// rows and the halo columns behind them, whichever is longer
inline int64_t gather_len(const stan_matrix *K) {
    const int64_t npad = (int64_t)K->nslices * 64;
    return 3 * (npad > K->nloc + K->nhalo ? npad : K->nloc + K->nhalo);
}
int stan_cg_workspace(stan_ctx *ctx, const stan_matrix *K);  // (re)allocates ctx->ws for K's sizes
void stan_cg_workspace_free(stan_ctx *ctx);
int stan_cg_workspace_move(stan_ctx *ctx, const stan_matrix *K, bool commit, stan_cg_ws *saved);
size_t stan_cg_products_bytes(const stan_ctx *ctx);   // bytes of a block that holds v and w
void stan_cg_products_set(stan_ctx *ctx, double *block, double *saved[3]);   // v, w carved out of `block` (nullptr: back to saved[]); placement.hip, second stage
void stan_cg_products_adopt(stan_ctx *ctx, double *block, size_t bytes, double *saved[3]);   // keep the carved pair for good, release the saved one

// ---- recovery.hip ---------------------------------------------------------------------------
// d: device view with disp (and node_dof when forces are asked for).  Strain / stress (both or neither), the element nodal
// forces and their sum R over the DOFs: outputs that are null are not computed.
int stan_recover_device(stan_ctx *ctx, const stan_mesh &d, double *d_strain, double *d_stress, double *d_elem_forces = nullptr,
                        double *d_R = nullptr);

// ---- scalars.hip ----------------------------------------------------------------------------
// Part.Load_Scalar on device arrays; sel: n_sel distinct indices in [0, STAN_SCALAR_COUNT), d_conn checked by the caller;
// d_point [n_sel][n_nodes] / d_cell [n_sel][3][n_elem], either may be null.  Synchronises the stream.
int stan_scalars_device(stan_ctx *ctx, int64_t n_nodes, const double *d_disp, int64_t n_elem, const int32_t *d_conn,
                        const double *d_strain, const double *d_stress, int32_t n_sel, const int32_t *sel, double *d_point,
                        double *d_cell);

// node -> (element, corner) lists in ascending element * 8 + corner: first corners only (the point scalars) or every corner
// (internal_forces.hip); ptr / list are temporaries of `tmp`, the work is enqueued on the context's stream
int stan_incidence_lists(stan_ctx *ctx, dev_scope &tmp, int64_t n_nodes, int64_t n_elem, const int32_t *d_conn, bool all_corners,
                         int64_t **ptr_out, int32_t **list_out);

// ---- internal_forces.hip --------------------------------------------------------------------
// f_int = sum_e int B^T D B u_e dV gathered per node, reactions and the equilibrium sums (stan_hip_internal_forces_hex8);
// d: device view with every array; eq is host memory; d_F, d_fint, d_reaction, eq may be null.  Checks its arguments on
// the device before anything is indexed with them.  Synchronises the stream.
int stan_internal_forces_device(stan_ctx *ctx, const stan_mesh &d, const double *d_F, double *d_fint, double *d_reaction,
                                stan_equilibrium *eq);
// Its argument check, shared with loads.hip: resets the status words, runs k_if_check (and k_ld_check_faces when
// n_faces > 0) with a zeroed claim array out of `tmp`, synchronises, and turns the first IF_* bit raised -- tested in the
// order DOF, CONN, MAT, TYPE, RED, FACE -- into "<who>: <what>" and its return code; *n_fixed = the fixed DOFs of the map.
enum stan_if_bits { IF_CONN = 1, IF_MAT = 2, IF_TYPE = 4, IF_DOF = 8, IF_RED = 16, IF_FACE = 32 };
int stan_elem_args_check(stan_ctx *ctx, dev_scope &tmp, const char *who, const stan_mesh &d, int64_t n_faces,
                         const int32_t *d_face_elem, const uint8_t *d_face_id, int64_t *n_fixed);
// The limits of the drivers that take every array, on the host, before it: n_dof = 3 n_nodes > 0 and n_mat > 0, fewer than
// 2^28 elements, at most 2^31 - 1 DOFs; "<who>: <what>", STAN_E_ARG.
int stan_elem_limits_check(stan_ctx *ctx, const char *who, const stan_mesh &d);

// ---- loads.hip ------------------------------------------------------------------------------
// Consistent nodal loads of body forces and face pressures, and the right-hand side for prescribed displacements
// (stan_hip_load_vector_hex8); d: device view with node_dof and red (its disp is not read: the prescribed displacements are
// d_disp0); mat_body and sums are host memory.  Checks its arguments on the device before anything is indexed with them.
// Synchronises the stream.
int stan_load_vector_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_body, int64_t n_faces, const int32_t *d_face_elem,
                            const uint8_t *d_face_id, const double *d_face_pressure, const double *d_disp0, double *d_F,
                            double *d_F_solve, double *d_load_full, stan_load_sums *sums);
// The thermal load of a nodal temperature change d_dT [n_nodes] (stan_hip_thermal_load_hex8); d as above; mat_alpha [n_mat]
// and sums are host memory.  The same checks; det J == 0 in a heated element is found before any output is stored.
int stan_thermal_load_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_alpha, const double *d_dT, double *d_F,
                             double *d_load_full, stan_thermal_sums *sums);
// d_stress [n_elem][8][6] loses beta_m dT at its corner's node in xx, yy, zz (stan_hip_thermal_stress_hex8); d: device view
// with conn, elem_mat and elem_type (no node array but d_dT); the integers are checked on the device first.  Synchronises
// the stream.
int stan_thermal_stress_device(stan_ctx *ctx, const stan_mesh &d, const double *d_dT, const double *mat_alpha, double *d_stress);
// The row-sum lumped mass (stan_hip_lumped_mass_hex8): the body term of the load vector with b = (rho, 0, 0), its component 0
// per node; d as above; mat_rho [n_mat] and sums are host memory; d_M [n_red], d_mass_node [n_nodes], either may be null.  The
// same checks; a free DOF without positive mass is found before any output is stored.
int stan_lumped_mass_device(stan_ctx *ctx, const stan_mesh &d, const double *mat_rho, double *d_M, double *d_mass_node,
                            stan_mass_sums *sums);

// ---- modal.hip ------------------------------------------------------------------------------
// The tall-skinny block kernels of the modal driver (api_modal.hip) and, below, of the buckling driver; a block vector is
// [q][N], q <= STAN_MODAL_QMAX.  All enqueue on the context's stream; those with host outputs synchronise it.  The two sets
// differ in their kernels; the host halves of the rotate, axpy and normalise entries are one routine each inside modal.hip.
constexpr int STAN_MODAL_QMAX = 32;
// d_rhs [q][N] = M o X0 with X0's column 0 = M and column j > 0 the hash of (row, j); *bad = the first row whose M is not
// positive and finite (-1: none).  Synchronises.
int stan_modal_start_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_M, double *d_rhs, int64_t *bad);
// A = Z^T W, B = Z^T (M o Z), host arrays [q*q] row-major.  Synchronises.
int stan_modal_gram_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_M, double *A,
                           double *B);
// X = Z Q, KX = W Q, R = KX - (M o X) diag(lambda), rho2 [q] (host) = sum R^2 / M, d_rhs column j = -R_j / lambda_j where bit j
// of mask is clear.  Q [q*q] row-major and lambda [q] are host arrays.  d_X / d_KX may be d_Z / d_W.  Synchronises.
int stan_modal_rotate_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_M,
                             const double *Q, const double *lambda, uint32_t mask, double *d_X, double *d_KX, double *d_rhs,
                             double *rho2);
// Z_j = X_j / lambda_j + D_dcol[j] (dcol[j] < 0: no correction).  d_Z may be d_X.  Enqueues only.
int stan_modal_axpy_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_X, const double *lambda, const int32_t *dcol,
                           const double *d_D, double *d_Z);
// d_phi [k][N] = the first k columns of X, each scaled to M-norm 1 with its entry of largest magnitude positive.  Synchronises.
int stan_modal_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, const double *d_M, double *d_phi);

// The block kernels of the buckling driver (api_buckling.hip); block vectors as above.
// d_X0 [q][N]: column j >= 0 = the hash of (row, j) of stan_modal_start_device's columns j > 0.  Enqueues only.
int stan_buckling_start_device(stan_ctx *ctx, int64_t N, int32_t q, double *d_X0);
// y = -y, n entries (exact).  Enqueues only.
int stan_buckling_negate_device(stan_ctx *ctx, int64_t n, double *d_y);
// X = Z Q in one launch; KX = W Q, R_j = sum_l (mu_j W_l - Y_l) Q_lj, d_rhs column j = -R_j where bit j of mask is clear,
// r2 [q] = sum R^2 / D and kx2 [q] = sum KX^2 / D (host) in another.  Q [q*q] row-major and mu [q] are host arrays.  d_X / d_KX
// may be d_Z / d_W.  Synchronises.
int stan_buckling_rotate_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_Z, const double *d_W, const double *d_Y,
                                const double *d_D, const double *Q, const double *mu, uint32_t mask, double *d_X, double *d_KX,
                                double *d_rhs, double *r2, double *kx2);
// Z_j = fma(mu_j, X_j, D_dcol[j]) (dcol[j] < 0: mu_j X_j).  d_Z may be d_X.  Enqueues only.
int stan_buckling_axpy_device(stan_ctx *ctx, int64_t N, int32_t q, const double *d_X, const double *mu, const int32_t *dcol,
                              const double *d_D, double *d_Z);
// d_phi [k][N] = the first k columns of X, each divided by its entry of largest magnitude (the lowest index on a tie): that
// entry becomes exactly +1.  Synchronises.
int stan_buckling_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, double *d_phi);
// The pencil driver's (stan_hip_modes_pencil): d_phi [k][N] = the first k columns of X, each divided by sqrt(X_j . MX_j), d_MX
// [k][N] = Mmat X by true products, with its entry of largest magnitude positive (the lowest index on a tie).  Synchronises.
int stan_pencil_normalise_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_X, const double *d_MX, double *d_phi);

// ---- matrix_shift.hip -----------------------------------------------------------------------
// The value stan_hip_matrix_to_csr exports for an entry a of a matrix that carries S K S, s_row and s_col its two scaling
// factors: the export and the shift pass share this one expression.
__host__ __device__ static inline double stan_unscaled_value(double a, double s_row, double s_col) { return a / (s_row * s_col); }
// *bad = the first index of d_M [N] whose entry is not positive and finite (-1: none).  Synchronises.
int stan_mass_check_device(stan_ctx *ctx, int64_t N, const double *d_M, int64_t *bad);
// *out = a new matrix of the context holding K + sigma diag(M) on the free DOFs (stan_hip_matrix_shifted_dev): K's structure
// arrays copied, its own value array by stan_matrix_alloc_stream, unscaled, nothing derived.  K is read only.  sigma and d_M
// checked by the caller; shift_ms (may be null) gets the stream time of the value pass when profiling is on.  Synchronises.
int stan_matrix_shifted_device(stan_ctx *ctx, stan_matrix *K, double sigma, const double *d_M, stan_matrix **out, double *shift_ms = nullptr);
// What the builders of a second matrix on K's layout share (the shifted matrix, the geometric stiffness): *out = a new matrix of
// the context with copies of K's structure arrays (enqueued on the context's stream), its own value array by
// stan_matrix_alloc_stream -- not yet filled -- unscaled, nothing derived.  A failure gives back what it had allocated.
int stan_matrix_clone_layout(stan_ctx *ctx, const stan_matrix *K, stan_matrix **out);
struct stan_matrix_guard {   // frees a matrix under construction unless the call gets to ok = true
    stan_matrix *k; bool ok = false;
    ~stan_matrix_guard() { if (!ok) stan_hip_matrix_free(k); }
};

// ---- geometric.hip --------------------------------------------------------------------------
// d_s36 [n][36] = the upper triangle of the element scalars s_e of the geometric stiffness (stan_hip_kg_hex8_batch), by the
// element pass of stan_geometric_stiffness_device itself; d_xyz8, d_u8 [n][24]; d_type checked by the caller.  Synchronises.
int stan_kg_batch_device(stan_ctx *ctx, int64_t n, const double *d_xyz8, const double *d_u8, double E, double nu,
                         const uint8_t *d_type, double *d_s36);
// *out = a new matrix of the context holding K_g(disp) in K's layout (stan_hip_geometric_stiffness_hex8_dev): K's structure
// arrays copied, its own value array by stan_matrix_alloc_stream, unscaled, nothing derived.  d: device view with every
// array, checked on the device before anything is indexed with it.  K is read only (its values are not read at all).
// Synchronises.
int stan_geometric_stiffness_device(stan_ctx *ctx, stan_matrix *K, const stan_mesh &d, stan_matrix **out);
// What the matrices of element scalars s_e (x) I_3 on K's layout share (G above, the consistent mass of mass.hip).
// The checks before anything is indexed: the limits, K whole on this device, the mesh's counts against K's, the integers on the
// device (stan_elem_args_check with a claim array out of `tmp`), the fixed DOFs against K's; "<who>: <what>".
int stan_elem_scalars_matrix_args(stan_ctx *ctx, dev_scope &tmp, const char *who, stan_matrix *K, const stan_mesh &d);
// *out = a new matrix by stan_matrix_clone_layout whose values are the ordered row gather of d_s36 [n_elem][36] (the upper
// triangles, kg_index's order): the node -> (element, corner) lists, the row maps, k_kg_gather, the status check (a mesh that
// couples two nodes K's pattern does not: STAN_E_ARG, the matrix given back).  ms [3] (profiling on): layout copy | lists and
// maps | gather.  The lists and maps are temporaries of `tmp`.  Synchronises.
int stan_elem_scalars_matrix(stan_ctx *ctx, dev_scope &tmp, const char *who, stan_matrix *K, const stan_mesh &d, const double *d_s36,
                             stan_matrix **out, double ms[3]);
// the connectivity of a batch (element e's corner a is "node" 8 e + a, material 0; d_conn [8 n], d_mat [n]) and the reset of the
// det J word.  Enqueues only.
int stan_elem_batch_iota(stan_ctx *ctx, int64_t n, int32_t *d_conn, int32_t *d_mat);

// ---- mass.hip -------------------------------------------------------------------------------
// d_m36 [n][36] = the upper triangle of the element scalars m_e of the consistent mass (stan_hip_mass_hex8_batch), by the element
// pass of stan_consistent_mass_device itself; d_xyz8 [n][24]; rho checked by the caller.  Synchronises.
int stan_mass_batch_device(stan_ctx *ctx, int64_t n, const double *d_xyz8, double rho, double *d_m36);
// *out = a new matrix of the context holding the consistent mass M_c in K's layout (stan_hip_consistent_mass_hex8_dev), built as
// stan_geometric_stiffness_device builds G.  d: device view with every array but disp; mat_rho [n_mat] is host memory.  K is
// read only (its values are not read at all).  Synchronises.
int stan_consistent_mass_device(stan_ctx *ctx, stan_matrix *K, const stan_mesh &d, const double *mat_rho, stan_matrix **out);
// *out = a new matrix of the context holding A + sigma B (stan_hip_matrix_axpy, matrix_shift.hip): A and B whole matrices of this
// context on one layout, compared on the host (the scalars) and on the device (the structure arrays) before anything is
// allocated; axpy_ms (may be null) gets the stream time of the value pass when profiling is on.  Synchronises.
int stan_matrix_axpy_device(stan_ctx *ctx, stan_matrix *A, double sigma, stan_matrix *B, stan_matrix **out, double *axpy_ms = nullptr);

// ---- transient.hip --------------------------------------------------------------------------
// The Newmark step kernels of the transient driver (api_transient.hip).  Every vector is [N] in
// memory the caller of these functions owns, 16-byte aligned (the drivers stage a user's arrays); all enqueue on the context's
// stream and none synchronises.
struct stan_newmark_coef { double a0, a1, a2, a3, a4, a5, alpha_R, beta_R, c_K, dt, gamma; };
constexpr int STAN_NM_ROWS = 512;   // entries per workgroup of the step kernels: one pair per lane
inline int64_t stan_newmark_blocks(int64_t N) { return (N + STAN_NM_ROWS - 1) / STAN_NM_ROWS; }
// a_0 = (gF F - alpha_R M o v0 - beta_R Kv0 - Ku0) / M; v0, Kv0, Ku0 may be null (the term is left out)
int stan_newmark_start_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, double gF, const double *F, const double *M,
                              const double *v0, const double *Kv0, const double *Ku0, double *a);
// w = a1 u + a4 v + a5 a (the operand of the damping product)
int stan_newmark_w_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, const double *u, const double *v, const double *a, double *w);
// b = (gF F + M o (p + alpha_R w) + beta_R Kw) / c_K; Kw null: without the beta_R term
int stan_newmark_predict_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, double gF, const double *u, const double *v,
                                const double *a, const double *F, const double *M, const double *Kw, double *b);
// u, v, a <- u_new, v', a' in place.  d_energy non-null: [3] = 1/2 v'.M v', 1/2 u'.Ku, gF F.u' from the same pass, through
// d_partial [3][stan_newmark_blocks(N)] and one finishing workgroup per value (workgroup order)
int stan_newmark_correct_device(stan_ctx *ctx, int64_t N, const stan_newmark_coef &c, const double *u_new, double *u, double *v,
                                double *a, const double *M, const double *F, const double *Ku, double gF, double *d_partial,
                                double *d_energy);
// the same three sums of a state that no step made (step 0)
int stan_newmark_energy_device(stan_ctx *ctx, int64_t N, const double *u, const double *v, const double *M, const double *F,
                               const double *Ku, double gF, double *d_partial, double *d_energy);
// row[j] = u[probe[j]], j < n_probe
int stan_newmark_probe_device(stan_ctx *ctx, int32_t n_probe, const int32_t *d_probe, const double *u, double *row);
// *bad = the first j whose probe[j] is outside [0, N) (-1: none).  Synchronises.
int stan_newmark_probe_check_device(stan_ctx *ctx, int64_t N, int32_t n_probe, const int32_t *d_probe, int64_t *bad);

// ---- explicit.hip ---------------------------------------------------------------------------
// The kernels of the explicit driver (api_explicit.hip): the central-difference update, the maps
// between the reduced numbering and the padded full one the driver keeps its vectors in, the row bound and the power sums of
// the stable step.  Vectors are 16-byte aligned memory of the caller of these functions; all enqueue on the context's stream
// and, unless said otherwise, none synchronises.
struct stan_cd_coef { double dt, dt2, two_dt, om, op, alpha_R; };   // dt, dt dt, 2 dt, 1 - h, 1 + h with h = alpha_R dt / 2
inline stan_cd_coef stan_cd_make_coef(double dt, double alpha_R) {
    const double h = alpha_R * dt / 2.0;
    return stan_cd_coef{dt, dt * dt, 2.0 * dt, 1.0 - h, 1.0 + h, alpha_R};
}
constexpr int STAN_CD_ROWS = 512;   // entries per workgroup of the vector kernels: one pair per lane
inline int64_t stan_cd_blocks(int64_t n) { return (n + STAN_CD_ROWS - 1) / STAN_CD_ROWS; }
// out[d] = `fill` at a fixed DOF (red[d] == -1) and in the padding n_dof <= d < n_pad, else in[d - red[d]] (in null: 0), divided
// by div[d] where div is given: k_expand's mapping
int stan_cd_expand_device(stan_ctx *ctx, int64_t n_dof, int64_t n_pad, const int32_t *d_red, const double *in, const double *div,
                          double fill, double *out);
// out[d - red[d]] = full[d] on the free DOFs; full_of[d - red[d]] = d
int stan_cd_compress_device(stan_ctx *ctx, int64_t n_dof, const int32_t *d_red, const double *full, double *out);
int stan_cd_index_device(stan_ctx *ctx, int64_t n_dof, const int32_t *d_red, int32_t *full_of);
// a = (gF F - Ku - alpha_R (M v)) / M and up = (u - dt v) + (dt2 / 2) a, Ku = y (s null) or y / s
int stan_cd_start_device(stan_ctx *ctx, int64_t n, const stan_cd_coef &c, double gF, const double *y, const double *s, const double *u,
                         const double *v, const double *M, const double *F, double *a, double *up);
// One central-difference update (the expressions: explicit.hip's header).  y: the product of the step (K u_n, or A^ (u_n / s)
// with s given); up holds u_{n-1} and receives u_{n+1}; xh (s given) receives u_{n+1} / s; v, a non-null: v_n and a_n are
// stored; d_energy non-null: [3] = 1/2 v_n.M v_n, 1/2 u_n.K u_n, gF F.u_n through d_partial [3][stan_cd_blocks(n)]; flag: the
// lowest `step` at which an entry of u_{n+1} is not finite (atomicMin on an integer)
int stan_cd_update_device(stan_ctx *ctx, int64_t n, const stan_cd_coef &c, double gF, long long step, const double *y, const double *s,
                          const double *un, double *up, const double *M, const double *F, double *xh, double *v, double *a,
                          double *d_partial, double *d_energy, long long *flag);
// row[j] = u[full_of[probe[j]]]
int stan_cd_probe_device(stan_ctx *ctx, int32_t n_probe, const int32_t *d_probe, const int32_t *full_of, const double *u, double *row);
// *bound (host) = max over the free DOFs d of (sum_j |K_dj|) / Mf[d], K_dj the exported values over the free columns; Mf in
// the full numbering.  K is read only.  Synchronises.
int stan_row_bound_device(stan_ctx *ctx, stan_matrix *K, const double *Mf, double *bound);
// the sums of one power step: d_sums [5] = x.Kx as hi, lo; x.(M x) as hi, lo (unevaluated pairs: error-free products and sums);
// Kx.Kx / M, with Kx = y or y / s, through d_partial [5][stan_cd_blocks(n)]
int stan_power_sums_device(stan_ctx *ctx, int64_t n, const double *y, const double *s, const double *x, const double *M,
                           double *d_partial, double *d_sums);
// x = (Kx / M) / sqrt(d_sums[4]), xh (s given) = x / s
int stan_power_next_device(stan_ctx *ctx, int64_t n, const double *y, const double *s, const double *M, const double *d_sums, double *x,
                           double *xh);

// ---- harmonic.hip ---------------------------------------------------------------------------
// The kernels of the frequency response (api_harmonic.hip); the expressions: harmonic.hip's header.  Phi is
// [k][N], the table d_tab [n_freq][stan_harmonic_width(k)] pairs (a, b) with zeros beyond k, d_r [N] or null (then r = 0).  All
// enqueue on the context's stream and none synchronises.
constexpr int STAN_HM_ROWS = 1024;   // rows per workgroup of the projection and of the peak reduction
inline int64_t stan_harmonic_blocks(int64_t N) { return (N + STAN_HM_ROWS - 1) / STAN_HM_ROWS; }
inline int stan_harmonic_width(int k) { return (k + 3) & ~3; }   // the table's pairs per frequency: k rounded up to a multiple of 4
// d_p [k] = Phi^T F through d_partial [k][stan_harmonic_blocks(N)]
int stan_harmonic_dots_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_phi, const double *d_F, double *d_partial, double *d_p);
// d_r = d_us - sum_j phi_j c[j], c [k] host
int stan_harmonic_residual_device(stan_ctx *ctx, int64_t N, int32_t k, const double *d_phi, const double *d_us, const double *c, double *d_r);
int stan_harmonic_sweep_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_freq, const double *d_phi, const double *d_r,
                               const double *d_tab, double *d_peak, int32_t *d_peak_idx);
// d_snaps [n_snap][2][N] at the table rows d_snap_freq [n_snap]
int stan_harmonic_snap_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_snap, const int32_t *d_snap_freq, const double *d_phi,
                              const double *d_r, const double *d_tab, double *d_snaps);
// d_probe [n_freq][n_probe][2]
int stan_harmonic_probe_device(stan_ctx *ctx, int64_t N, int32_t k, int32_t n_freq, int32_t n_probe, const int32_t *d_probe_dof,
                               const double *d_phi, const double *d_r, const double *d_tab, double *d_probe);
// d_out[0] = the largest entry of d_peak, d_out_idx[0] = its row (the lowest on a tie), d_out_idx[1] = d_peak_idx of that row;
// d_pval / d_pidx [stan_harmonic_blocks(N)]
int stan_harmonic_peakmax_device(stan_ctx *ctx, int64_t N, const double *d_peak, const int32_t *d_peak_idx, double *d_pval, long long *d_pidx,
                                 double *d_out, long long *d_out_idx);

// ---- comm.cpp -------------------------------------------------------------------------------
int stan_comm_allreduce_sum_f64(stan_ctx *ctx, double *d_buf, size_t count);
int stan_comm_info(stan_ctx *ctx, int *version, int *count, int *rank);
int stan_comm_library(stan_ctx *ctx, std::string *path, int *reused);
int stan_comm_allgather_bytes(stan_ctx *ctx, const void *mine, size_t bytes, void *all);   // host buffers, [nranks*bytes] out
// exchange: pack rows listed in K->d_send_rows from d_vec (3 doubles per block row) and
// receive into d_vec + 3*nloc (halo region).
int stan_comm_halo_exchange(stan_ctx *ctx, stan_matrix *K, double *d_vec);
int stan_comm_allgather_rows(stan_ctx *ctx, stan_matrix *K, double *d_full_blockvec);
void stan_comm_abort(stan_ctx *ctx);

// device memory helpers (see stan_pool)
// may_flush = false: a block the caller can do without (an optional second copy of a matrix's values) -- a failed hipMalloc
// leaves the parked blocks where they are
static inline int stan_dmalloc_bytes(stan_ctx *ctx, void **p, size_t bytes, bool may_flush = true) {
    *p = nullptr;
    if (bytes == 0) bytes = 8;
    stan_pool &pool = ctx->pool;
    const bool pooled = pool.enabled && bytes >= stan_pool::MIN_BYTES;
    if (pooled) {
        int best = -1;
        for (int i = 0; i < (int)pool.avail.size(); i++) {
            const size_t cap = pool.avail[i].cap;
            if (cap >= bytes && cap <= bytes + bytes / 2 && (best < 0 || cap < pool.avail[best].cap)) best = i;
        }
        if (best >= 0) {
            *p = pool.avail[best].p;
            pool.live[*p] = pool.avail[best].cap;
            pool.bytes_avail -= pool.avail[best].cap;
            pool.avail.erase(pool.avail.begin() + best);
            return STAN_OK;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess && may_flush && !pool.avail.empty()) {  // make room and try once more
        (void)hipGetLastError();
        pool.flush();
        e = hipMalloc(p, bytes);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        ctx->err = std::string("hipMalloc(") + std::to_string(bytes) + " B): " + hipGetErrorString(e);
        return STAN_E_ALLOC;
    }
    if (pooled) pool.live[*p] = bytes;
    return STAN_OK;
}
template <typename T>
static inline int stan_dmalloc(stan_ctx *ctx, T **p, size_t count) {
    return stan_dmalloc_bytes(ctx, (void **)p, count * sizeof(T));
}
static inline void stan_dfree(stan_ctx *ctx, void *p) {
    if (!p) return;
    if (ctx) {
        auto it = ctx->pool.live.find(p);
        if (it != ctx->pool.live.end()) {
            const size_t cap = it->second;
            ctx->pool.live.erase(it);
            if (ctx->pool.enabled) {
                ctx->pool.avail.push_back({p, cap});
                ctx->pool.bytes_avail += cap;
                // a host cycling through many sizes, or one sharing the GPU with another
                // allocator: drop the oldest parked blocks beyond the block / byte budget
                while (!ctx->defer_frees && !ctx->pool.avail.empty() &&
                       (ctx->pool.avail.size() > stan_pool::MAX_BLOCKS || ctx->pool.bytes_avail > ctx->pool.max_bytes)) {
                    hipFree(ctx->pool.avail.front().p);
                    ctx->pool.bytes_avail -= ctx->pool.avail.front().cap;
                    ctx->pool.avail.erase(ctx->pool.avail.begin());
                }
                return;
            }
        }
        if (ctx->defer_frees) { ctx->deferred.push_back(p); return; }   // (see stan_ctx::defer_frees)
    }
    hipFree(p);
}
static inline void stan_flush_deferred(stan_ctx *ctx) {
    ctx->defer_frees = false;
    for (void *q : ctx->deferred) hipFree(q);
    ctx->deferred.clear();
}
// device temporaries of one call: given back to the context in the order of allocation, on every exit path
struct dev_scope {
    stan_ctx *ctx;
    std::vector<void *> p;
    explicit dev_scope(stan_ctx *c) : ctx(c) {}
    dev_scope(const dev_scope &) = delete; dev_scope &operator=(const dev_scope &) = delete;
    ~dev_scope() { for (void *q : p) stan_dfree(ctx, q); }
    template <typename T>
    int alloc(T **q, size_t n) {
        const int rc = stan_dmalloc(ctx, q, n);
        if (rc == STAN_OK) p.push_back((void *)*q);
        return rc;
    }
};
// the events around a call's phases: mark(k) records event k on the context's stream, read(a, b, &ms) after the stream is
// synchronised; with profiling off no event is created, mark does nothing and read leaves *ms alone
struct phase_timer {
    stan_ctx *ctx;
    event_bag evs;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    phase_timer(stan_ctx *c, int n_marks) : ctx(c) {   // n_marks <= 5
        for (int k = 0; ctx->profiling && k < n_marks; k++) ev[k] = evs.make();
    }
    int mark(int k) {
        if (ev[k]) HIPCHK(ctx, hipEventRecord(ev[k], ctx->stream));
        return STAN_OK;
    }
    int read(int a, int b, double *ms) {
        float t = 0;
        if (!ctx->profiling) return STAN_OK;
        HIPCHK(ctx, hipEventElapsedTime(&t, ev[a], ev[b]));
        *ms = t;
        return STAN_OK;
    }
};
// lambda and G of every material (stan_lame) in a temporary of `tmp`; the object outlives the stream's copy (recovery.hip)
struct lamG_buf {
    std::vector<double> host;
    double *d = nullptr;
    int alloc(dev_scope &tmp, int32_t n_mat, const double *mat_E_nu);
    hipError_t upload(hipStream_t st) const { return hipMemcpyAsync(d, host.data(), host.size() * 8, hipMemcpyHostToDevice, st); }
};
// the det J == 0 report of the element kernels (the caller has copied h_status[SS_BAD_ELEM] back and synchronised)
static inline int stan_detj_check(stan_ctx *ctx, const char *why) {
    if (ctx->h_status[SS_BAD_ELEM] == 0x7fffffffffffffffLL) return STAN_OK;
    ctx->bad_elem = ctx->h_status[SS_BAD_ELEM];
    ctx->err = "det J == 0 in element " + std::to_string(ctx->bad_elem) + why;
    return STAN_E_DETJ;
}
static inline unsigned nblk(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }   // blocks of t threads over n items
// The round trip of a check on the device: the slot d_status[SS_AUX] starts at "none", `enqueue(slot)` launches on the context's
// stream the kernel that takes atomicMin(slot, index) at every index it refuses, the slot comes back; *first = the lowest such
// index (-1: none).  Synchronises.
template <typename F>
static inline int stan_first_offender(stan_ctx *ctx, int64_t *first, F &&enqueue) {
    hipStream_t st = ctx->stream;
    const long long none = 0x7fffffffffffffffLL;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_status + SS_AUX, &none, 8, hipMemcpyHostToDevice, st));
    enqueue((long long *)(ctx->d_status + SS_AUX));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, ctx->d_status + SS_AUX, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *first = ctx->h_status[SS_AUX] == none ? -1 : ctx->h_status[SS_AUX];
    return STAN_OK;
}

// ---- multi.hip: fan-out of the public entry points for a group handle ------------------------
void stan_set_global_error(const std::string &msg);   // api.hip: errors raised before a context exists
void stan_group_destroy(stan_ctx *lead);
const char *stan_group_last_error(stan_ctx *lead);
int stan_group_ctx_call(stan_ctx *lead, const std::function<int(stan_ctx *)> &fn);
int stan_group_ctx_call_ranked(stan_ctx *lead, const std::function<int(stan_ctx *, int)> &fn);   // fn(rank context, rank) on every worker
int stan_group_assemble(stan_ctx *lead, const stan_mesh &m, stan_matrix **outK);   // m: host view, as in stan_assemble_host
void stan_group_matrix_free(stan_matrix *K);
int stan_group_cg_solve(stan_ctx *lead, stan_matrix *K, const double *F, double eps_f, int32_t max_its,
                        int32_t precision_mode, double *U, int32_t *termination_type, int32_t *iterations,
                        double *rel_residual);
int stan_group_recover(stan_ctx *lead, const stan_mesh &m, double *strain, double *stress);   // one chunk of m per rank
// a rank's STAN_E_DETJ / STAN_E_UNSUPPORTED over the chunk from element e0 on: lead->bad_elem and the rank's text name the whole model's element
void stan_chunk_bad_element(stan_ctx *lead, stan_ctx *c, int rc, int64_t e0);
// api_solve.hip, api_post.hip: the host entries of ONE context behind their argument checks (the public entries and the group's ranks call them)
int stan_assemble_host(stan_ctx *ctx, const stan_mesh &m, stan_matrix **outK);
int stan_recover_host(stan_ctx *ctx, const stan_mesh &m, double *strain, double *stress);
int stan_group_set_p2p(stan_ctx *lead, bool on);
int stan_group_rank0_call(stan_ctx *lead, const std::function<int(stan_ctx *)> &fn);
stan_ctx *stan_group_rank0(stan_ctx *lead);
stan_ctx *stan_group_rank(stan_ctx *lead, int r);
int stan_group_size(stan_ctx *lead);
// entry points that have no meaning for a group handle (device pointers, single-rank helpers)
#define STAN_NO_GROUP(ctx, what)                                                                   \
    do {                                                                                           \
        if ((ctx) && (ctx)->group) {                                                               \
            (ctx)->err = std::string(what) + ": not available on a multi-device handle";           \
            return STAN_E_UNSUPPORTED;                                                             \
        }                                                                                          \
    } while (0)

// placement.hip
int stan_probe_block(stan_ctx *ctx, const void *p, size_t bytes, float *ms_out);
// second_copy: an optional further stream of a matrix whose own values are placed already -- the search leaves the CG's
// vectors where they are (they are paired with the values) and a failure does not flush the pool
int stan_dmalloc_streamed(stan_ctx *ctx, void **p, size_t bytes,
                          const std::function<int(const void *, float *, bool)> &probe, bool second_copy = false);
int stan_spmv_probe(stan_ctx *ctx, stan_matrix *K, const void *vals, size_t bytes, int32_t precision,
                    float *ms_out, bool self_pair = false, bool folded = false);   // folded: `vals` is a block for a FOLDED stream (fold.hip)
