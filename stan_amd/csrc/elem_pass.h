// elem_pass.h -- the skeleton shared by the element passes after the solve: k_recover (recovery.hip), k_if_elem
// (internal_forces.hip) and k_ld_elem (loads.hip), with the block reduction and the node gather of their second phases.
// block_sums and the kernel that finishes a two-pass sum (k_finish_sums) also serve modal.hip and transient.hip.
//
// Layout (round 5): a workgroup of 256 lanes = 4 waves, a wave = 8 elements, an element = 8 lanes.
// Lane g of an element is its Gauss point g AND its local node g: it loads node g only (3 coordinates, 3 displacements: 7
// gathers with the connectivity entry, where every lane loading all 8 nodes was 56 and bound by the address pipeline) and
// the element's 48 values go round through LDS, one record per element:
//     rec[0, 24)  coordinates, node-major        rec[24, 48)  displacements, node-major        rec[48, 50)  padding
// The exchange is wave-local (wave_sync); sums over an element's 8 lanes are three butterfly stages (elem_sum: a fixed
// order, bit-reproducible); what a wave produces is contiguous in memory (8 elements x 8 nodes x NV values), so it is staged
// in the wave's LDS and leaves as full 512-B lines (elem_store_staged).
#pragma once

#include "internal.h"
#include "hex8_device.h"

// doubles per element record in LDS.  48 + 2: the 8 records of a wave start 50 doubles = 100 banks = 36 banks (mod 64) apart
// -- no bank conflicts between the 8 elements of a wave -- and a record stays 16-B aligned: the
// reads pair up into ds_read_b128.
constexpr int ELEM_REC = 50;

// The element scalars of geometric.hip and mass.hip, one per node pair: the upper triangle of the symmetric 8 x 8, row-major:
// (a, b), a <= b, at a * 8 - a (a - 1) / 2 + b - a
constexpr int KG_N = 36;
__host__ __device__ constexpr int kg_index(int a, int b) {
    return (a <= b ? a * 8 - a * (a - 1) / 2 + (b - a) : b * 8 - b * (b - 1) / 2 + (a - b));
}

// wave-local exchange through LDS: the LDS executes one wave's instructions in order (as in k_spmv_fold), so a wave-level
// fence is all that the lanes of one wave need between a write and another lane's read
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct elem_lanes {
    int wv, lane;   // wave of the workgroup, lane of the wave
    int el, g;      // element of the wave, Gauss point = local node of the element
    int64_t e0, e;  // first element of this wave, this lane's element
    bool valid;     // e < n_elem
};
__device__ __forceinline__ elem_lanes elem_lanes_here(int64_t n_elem) {   // grid: nblk(n_elem, 32) workgroups of 256
    elem_lanes L;
    L.wv = threadIdx.x >> 6; L.lane = threadIdx.x & 63;
    L.el = L.lane >> 3; L.g = L.lane & 7;
    L.e0 = ((int64_t)blockIdx.x * 4 + L.wv) * 8;
    L.e = L.e0 + L.el;
    L.valid = L.e < n_elem;
    return L;
}

// lane g of a valid element loads node g into the element's record (DISP: with its displacements); returns the node
template <bool DISP>
__device__ __forceinline__ int64_t elem_load_node(double *rec, const elem_lanes &L, const int32_t *__restrict__ conn,
                                                  const double *__restrict__ xyz, const double *__restrict__ disp) {
    const int64_t nd = conn[L.e * 8 + L.g];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        rec[3 * L.g + c] = xyz[3 * nd + c];
        if (DISP) rec[24 + 3 * L.g + c] = disp[3 * nd + c];
    }
    return nd;
}

// natural coordinates of Gauss point g of `type` (HEX8_G1: every g is the one point at the origin)
__device__ __forceinline__ void hex8_gauss_point(int type, int g, double &px, double &py, double &pz) {
    const double gl = hex8_gauss_loc(type);
    px = hex8_sign(HEX8_SX, g) * gl; py = hex8_sign(HEX8_SY, g) * gl; pz = hex8_sign(HEX8_SZ, g) * gl;
}

// eps = B u at the Gauss point whose {J^-1, c} is o (hex8_gp_setup); u: the record's 24 displacements
__device__ __forceinline__ void hex8_strain(const double *o, const double *u, double px, double py, double pz, double eps[6]) {
#pragma unroll
    for (int c = 0; c < 6; c++) eps[c] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double gr[3];
        hex8_grad(o, i, px, py, pz, gr);
        // BL0 rows (Element.cs:316-324): xx, yy, zz, xy, yz, xz
        eps[0] += gr[0] * u[3 * i];
        eps[1] += gr[1] * u[3 * i + 1];
        eps[2] += gr[2] * u[3 * i + 2];
        eps[3] += gr[1] * u[3 * i] + gr[0] * u[3 * i + 1];
        eps[4] += gr[2] * u[3 * i + 1] + gr[1] * u[3 * i + 2];
        eps[5] += gr[2] * u[3 * i] + gr[0] * u[3 * i + 2];
    }
}
// sig = D eps, D isotropic.  Apart from hex8_strain so that the material is read after the strain loop, where it was: its
// two values would otherwise be live across the loop (8 VGPRs, a wave per SIMD less in k_recover)
__device__ __forceinline__ void hex8_stress(double lam, double G, const double eps[6], double sig[6]) {
    const double tr = lam * (eps[0] + eps[1] + eps[2]);
    sig[0] = tr + 2 * G * eps[0];
    sig[1] = tr + 2 * G * eps[1];
    sig[2] = tr + 2 * G * eps[2];
    sig[3] = G * eps[3]; sig[4] = G * eps[4]; sig[5] = G * eps[5];
}

// sum over the 8 lanes of an element (three butterfly stages: a fixed order)
__device__ __forceinline__ double elem_sum(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

// lane g: (B_g^T s) * sc for each node a, summed over the element's 8 lanes; node a's three components end up on lane a
// (mine).  Every lane of the wave takes part in the sums; `with_grad` false leaves the gradient, so the term, at zero.
__device__ __forceinline__ void elem_bt_sum(const double *o, bool with_grad, int g, double px, double py, double pz,
                                            const double s[6], double sc, double mine[3]) {
    mine[0] = mine[1] = mine[2] = 0.0;
#pragma unroll
    for (int a = 0; a < 8; a++) {
        double gr[3] = {0, 0, 0};
        if (with_grad) hex8_grad(o, a, px, py, pz, gr);
        double f[3];
        f[0] = (gr[0] * s[0] + gr[1] * s[3] + gr[2] * s[5]) * sc;
        f[1] = (gr[1] * s[1] + gr[0] * s[3] + gr[2] * s[4]) * sc;
        f[2] = (gr[2] * s[2] + gr[1] * s[4] + gr[0] * s[5]) * sc;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = elem_sum(f[c]);
            if (a == g) mine[c] = v;
        }
    }
}

// The wave's 8 x 8 x NV values of an [n_elem][8][NV] array are contiguous in memory: lane -> stg[lane * NV ..], then out
// as NV 512-B lines; the ragged tail of the last wave stops at n_elem.  stg: the wave's LDS, which no lane still reads
// (the caller's wave_sync).  NT: non-temporal stores (results that this pass does not read again).
template <int NV, bool NT>
__device__ __forceinline__ void elem_store_staged(double *stg, const elem_lanes &L, int64_t n_elem, const double (&v)[NV],
                                                  double *__restrict__ out) {
#pragma unroll
    for (int c = 0; c < NV; c++) stg[L.lane * NV + c] = v[c];
    wave_sync();
    double *dst = out + L.e0 * (8 * NV);
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int idx = j * 64 + L.lane;
        if (L.e0 + idx / (8 * NV) < n_elem) {
            if (NT) __builtin_nontemporal_store(stg[idx], dst + idx);
            else dst[idx] = stg[idx];
        }
    }
}

// sums of the block's 256 lanes in a fixed order (six butterfly stages per wave, then the four waves in order) on thread 0
template <int N, int W>
__device__ __forceinline__ void block_sums(double (&s)[N], double (*sh)[W]) {   // W >= N: a row may hold more than the sums
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < N; k++) s[k] += __shfl_xor(s[k], off, 64);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; k++) sh[wv][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++)
#pragma unroll
            for (int k = 0; k < N; k++) s[k] += sh[w][k];
}
// The second pass of a two-pass sum (modal.hip, transient.hip): out[v] = the sum of partial[v][0 .. n_blocks) in block order.
// One workgroup of T lanes per value: thread t adds blocks t, t + T, ... in ascending order, then the workgroup's fixed order.
// A kernel defined in a header is emitted only in the translation units that instantiate it.
template <int T>
__global__ void __launch_bounds__(T)
k_finish_sums(int64_t n_blocks, const double *__restrict__ partial, double *__restrict__ out) {
    static_assert(T == 256, "block_sums adds the four waves of 256 lanes");
    __shared__ double sh[4][1];
    double s[1] = {0.0};
    const double *p = partial + (int64_t)blockIdx.x * n_blocks;
    for (int64_t b = threadIdx.x; b < n_blocks; b += T) s[0] += p[b];
    block_sums(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// node gather: f = the sum of fe[3t .. 3t + 2] over node n's list entries t = element * 8 + corner, in list order
__device__ __forceinline__ void node_gather(const int64_t *__restrict__ ptr, const int32_t *__restrict__ list,
                                            const double *__restrict__ fe, int64_t n, double f[3]) {
    f[0] = f[1] = f[2] = 0.0;
    const int64_t k0 = ptr[n], k1 = ptr[n + 1];
    for (int64_t k = k0; k < k1; k++) {
        const int64_t t = list[k];
        f[0] += fe[3 * t]; f[1] += fe[3 * t + 1]; f[2] += fe[3 * t + 2];
    }
}
