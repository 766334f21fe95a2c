// scalars.hip -- result scalars for post-processing: Part.Load_Scalar (Part.cs:231-528).
// From an element's 8x6 strain and stress blocks (recovery.hip) and the nodal displacements, 24 scalars per
// (element, local node) corner (Part.cs:272-297, 318-379):
//    0-3   displacement X, Y, Z, total          4-9   stress xx yy zz xy yz xz     10-12 stress P1 >= P2 >= P3
//   13     von Mises stress                     14-19 strain components            20-22 strain principals
//   23     effective strain = 2/3 of the von Mises expression on the strain principals
// (the shear strain enters the tensor as stored, not halved -- the reference's choice, kept), then
//   cell scalars  (:386-388): max, average, min over the element's 8 corners, the average summed in node order 0..7;
//   point scalars (:431-519): average over the node's incident elements in element order, each element once, its corner
//                             the FIRST local position that names the node (NList.IndexOf in a collapsed hex).
// Everything is bit-reproducible: the point scalars are a GATHER over a node -> (element, corner) list in ascending
// element order, never atomics on doubles.  The list is built here: integer counts (atomic, order-free), an exclusive
// scan (scan.hip), an unordered fill and a rank sort of every node's segment -- no per-node buffer of fixed size, so
// the axis node of a revolved mesh with dozens of incidences takes the same path as a cube's corner.
// The point kernel RECOMPUTES the two eigen-solves of an incidence instead of reading derived values the cell kernel
// could leave behind: a temporary of P1-P3 and von Mises for both tensors is 64 B written and 64 B read per corner on
// top of the 96 B both forms read; recomputing moves nothing (DESIGN.md 3.6 has the byte count).
// Eigenvalues: cyclic Jacobi, 6 fixed sweeps over (0,1), (0,2), (1,2), the 3x3 in named registers (no LDS, no
// scratch); the tensor is first scaled by a power of two so that no intermediate overflows, and von Mises is formed
// before scaling back: finite input never gives NaN.  The trigonometric closed form loses 8e-9 relative when two
// eigenvalues nearly coincide and is not used.
#include "internal.h"

namespace {

struct scal_sel {
    uint32_t mask;    // bit s: scalar s is selected
    int8_t row[STAN_SCALAR_COUNT];   // its row in the output arrays
};

constexpr uint32_t SIG_EIG = 0xFu << STAN_SCALAR_STRESS_P1, EPS_EIG = 0xFu << STAN_SCALAR_STRAIN_P1;

// one Jacobi rotation that annihilates a_pq; r is the third index
__device__ inline void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    // t = sign(theta) / (|theta| + sqrt(theta^2 + 1)): a huge theta gives t = 0, not inf / inf
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double p = arp, q = arq;
    arp = p - s * (q + tau * p);
    arq = q + s * (p - tau * q);
}

// v = {xx, yy, zz, xy, yz, xz}: P1 >= P2 >= P3 and sqrt(((P1-P2)^2 + (P2-P3)^2 + (P3-P1)^2) / 2)
__device__ inline void principal(double xx, double yy, double zz, double xy, double yz, double xz,
                                 double &P1, double &P2, double &P3, double &vm) {
    const double m = fmax(fmax(fmax(fabs(xx), fabs(yy)), fmax(fabs(zz), fabs(xy))), fmax(fabs(yz), fabs(xz)));
    if (m == 0.0) { P1 = P2 = P3 = vm = 0.0; return; }
    const int ex = __builtin_amdgcn_frexp_exp(m);   // m = f 2^ex, f in [0.5, 1): the scaled entries are at most 1
    xx = ldexp(xx, -ex); yy = ldexp(yy, -ex); zz = ldexp(zz, -ex);
    xy = ldexp(xy, -ex); yz = ldexp(yz, -ex); xz = ldexp(xz, -ex);
#pragma unroll
    for (int sweep = 0; sweep < 6; sweep++) {
        jacobi_rotate(xx, yy, xy, xz, yz);   // (0,1), r = 2
        jacobi_rotate(xx, zz, xz, xy, yz);   // (0,2), r = 1
        jacobi_rotate(yy, zz, yz, xy, xz);   // (1,2), r = 0
    }
    const double hi = fmax(xx, yy), lo = fmin(xx, yy);
    const double p1 = fmax(hi, zz), mid = fmin(hi, zz);
    const double p2 = fmax(lo, mid), p3 = fmin(lo, mid);
    const double a = p1 - p2, b = p2 - p3, c = p3 - p1;
    vm = ldexp(sqrt((a * a + b * b + c * c) / 2.0), ex);
    P1 = ldexp(p1, ex); P2 = ldexp(p2, ex); P3 = ldexp(p3, ex);
}

// the 24 values of one corner; only what `mask` selects is computed (uniform branches), the rest stays 0
__device__ inline void corner_values(uint32_t mask, const double u[3], const double eps[6], const double sig[6],
                                     double v[STAN_SCALAR_COUNT]) {
#pragma unroll
    for (int s = 0; s < STAN_SCALAR_COUNT; s++) v[s] = 0.0;
    v[0] = u[0]; v[1] = u[1]; v[2] = u[2];
    if (mask & (1u << STAN_SCALAR_DISP_TOTAL)) v[3] = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
#pragma unroll
    for (int c = 0; c < 6; c++) { v[STAN_SCALAR_STRESS_XX + c] = sig[c]; v[STAN_SCALAR_STRAIN_XX + c] = eps[c]; }
    if (mask & SIG_EIG)
        principal(sig[0], sig[1], sig[2], sig[3], sig[4], sig[5], v[10], v[11], v[12], v[13]);
    if (mask & EPS_EIG) {
        principal(eps[0], eps[1], eps[2], eps[3], eps[4], eps[5], v[20], v[21], v[22], v[23]);
        v[23] = (2.0 / 3.0) * v[23];
    }
}

__device__ inline void load_row(const double *__restrict__ p, double out[6]) {   // 48-B rows: 16-B aligned
    const double2 *q = reinterpret_cast<const double2 *>(p);
    const double2 a = q[0], b = q[1], c = q[2];
    out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y; out[4] = c.x; out[5] = c.y;
}

// ---- cell scalars: 8 lanes per element, one per local node (the layout of k_recover) ---------------------------------
__global__ void __launch_bounds__(256)
k_scalars_cell(int64_t n_elem, const int32_t *__restrict__ conn, const double *__restrict__ disp,
               const double *__restrict__ strain, const double *__restrict__ stress, scal_sel sel, double *__restrict__ cell) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t >> 3;
    const int i = (int)(t & 7), lane = threadIdx.x & 63, base = lane & ~7;
    const bool valid = e < n_elem;
    double u[3] = {0, 0, 0}, eps[6] = {0, 0, 0, 0, 0, 0}, sig[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
        const int64_t nd = conn[t];
        u[0] = disp[3 * nd]; u[1] = disp[3 * nd + 1]; u[2] = disp[3 * nd + 2];
        load_row(strain + t * 6, eps);
        load_row(stress + t * 6, sig);
    }
    double v[STAN_SCALAR_COUNT];
    corner_values(sel.mask, u, eps, sig, v);
#pragma unroll
    for (int s = 0; s < STAN_SCALAR_COUNT; s++) {
        if (!(sel.mask & (1u << s))) continue;
        // corner 0..7 in order: the sum is LINQ's Average, max and min keep the first of equals (Part.cs:386-388)
        double x = __shfl(v[s], base, 64);
        double sum = 0.0 + x, mx = x, mn = x;   // (LINQ's sum starts at 0: eight times -0.0 average to +0.0)
#pragma unroll
        for (int k = 1; k < 8; k++) {
            x = __shfl(v[s], base + k, 64);
            sum += x;
            mx = x > mx ? x : mx;
            mn = x < mn ? x : mn;
        }
        if (valid && i < 3)
            cell[((int64_t)sel.row[s] * 3 + i) * n_elem + e] = i == 0 ? mx : i == 1 ? sum / 8.0 : mn;
    }
}

// ---- point scalars: one lane per node walks its (element, corner) list in ascending element order ---------------------
__global__ void __launch_bounds__(256)
k_scalars_point(int64_t n_nodes, const int64_t *__restrict__ ptr, const int32_t *__restrict__ list,
                const double *__restrict__ disp, const double *__restrict__ strain, const double *__restrict__ stress,
                scal_sel sel, double *__restrict__ point) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nodes) return;
    const int64_t k0 = ptr[n], k1 = ptr[n + 1];
    const double u[3] = {disp[3 * n], disp[3 * n + 1], disp[3 * n + 2]};
    double acc[STAN_SCALAR_COUNT];
#pragma unroll
    for (int s = 0; s < STAN_SCALAR_COUNT; s++) acc[s] = 0.0;
    for (int64_t k = k0; k < k1; k++) {
        const int64_t t = list[k];   // element * 8 + corner
        double eps[6], sig[6], v[STAN_SCALAR_COUNT];
        load_row(strain + t * 6, eps);
        load_row(stress + t * 6, sig);
        corner_values(sel.mask, u, eps, sig, v);
#pragma unroll
        for (int s = 0; s < STAN_SCALAR_COUNT; s++)
            if (sel.mask & (1u << s)) acc[s] += v[s];
    }
    const double cnt = (double)(k1 - k0);
#pragma unroll
    for (int s = 0; s < STAN_SCALAR_COUNT; s++)
        if (sel.mask & (1u << s))   // a node no element references: 0 (the reference would divide by zero)
            point[(int64_t)sel.row[s] * n_nodes + n] = k1 > k0 ? acc[s] / cnt : 0.0;
}

// ---- node -> (element, corner) lists -----------------------------------------------------------------------------------
// first corners only (the point scalars): corner a of element e counts when no earlier corner of e names the same node
// (EList holds an element once, Database.cs:149-158; NList.IndexOf finds the first position); all corners (the internal
// forces, internal_forces.hip): every corner counts, as the K scatter counts them
__device__ inline bool first_corner(const int32_t *__restrict__ conn, int64_t t, int32_t nd) {
    const int64_t e8 = t & ~(int64_t)7;
    for (int64_t j = e8; j < t; j++)
        if (conn[j] == nd) return false;
    return true;
}
__global__ void k_scal_count(int64_t n_inc, const int32_t *__restrict__ conn, bool all_corners, int32_t *cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_inc) return;
    const int32_t nd = conn[t];
    if (all_corners || first_corner(conn, t, nd)) atomicAdd(&cnt[nd], 1);
}
__global__ void k_scal_fill(int64_t n_inc, const int32_t *__restrict__ conn, bool all_corners, const int64_t *__restrict__ ptr,
                            int32_t *cursor, int32_t *unsorted) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_inc) return;
    const int32_t nd = conn[t];
    if (all_corners || first_corner(conn, t, nd)) unsorted[ptr[nd] + atomicAdd(&cursor[nd], 1)] = (int32_t)t;
}
// the entries of a segment are distinct: the rank of one among its segment is its place in ascending order
__global__ void k_scal_rank(const int64_t *__restrict__ ptr, int64_t n_nodes, const int32_t *__restrict__ conn,
                            const int32_t *__restrict__ unsorted, int32_t *__restrict__ list) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ptr[n_nodes]) return;
    const int32_t v = unsorted[p];
    const int32_t nd = conn[v];
    const int64_t k0 = ptr[nd], k1 = ptr[nd + 1];
    int64_t r = 0;
    for (int64_t k = k0; k < k1; k++) r += unsorted[k] < v;
    list[k0 + r] = v;
}

}  // namespace

// ptr [n_nodes + 1], list [ptr[n_nodes]] = element * 8 + corner, every node's segment ascending: temporaries of `tmp`,
// enqueued on the context's stream (the caller synchronises before `tmp` goes).  d_conn entries are in [0, n_nodes).
int stan_incidence_lists(stan_ctx *ctx, dev_scope &tmp, int64_t n_nodes, int64_t n_elem, const int32_t *d_conn, bool all_corners,
                         int64_t **ptr_out, int32_t **list_out) {
    hipStream_t st = ctx->stream;
    const int64_t n_inc = n_elem * 8;
    int32_t *d_cnt, *d_unsorted, *d_list;
    int64_t *d_ptr;
    STANCHK(tmp.alloc(&d_cnt, (size_t)n_nodes));
    STANCHK(tmp.alloc(&d_ptr, (size_t)n_nodes + 1));
    STANCHK(tmp.alloc(&d_unsorted, (size_t)(n_inc > 0 ? n_inc : 1)));
    STANCHK(tmp.alloc(&d_list, (size_t)(n_inc > 0 ? n_inc : 1)));
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, (size_t)n_nodes * 4, st));
    if (n_inc > 0) hipLaunchKernelGGL(k_scal_count, dim3(nblk(n_inc, 256)), dim3(256), 0, st, n_inc, d_conn, all_corners, d_cnt);
    STANCHK(stan_scan_exclusive(ctx, d_cnt, d_ptr, n_nodes));
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, (size_t)n_nodes * 4, st));
    if (n_inc > 0) {
        hipLaunchKernelGGL(k_scal_fill, dim3(nblk(n_inc, 256)), dim3(256), 0, st, n_inc, d_conn, all_corners, d_ptr, d_cnt, d_unsorted);
        hipLaunchKernelGGL(k_scal_rank, dim3(nblk(n_inc, 256)), dim3(256), 0, st, d_ptr, n_nodes, d_conn, d_unsorted, d_list);
    }
    *ptr_out = d_ptr;
    *list_out = d_list;
    return STAN_OK;
}

// d_conn entries are in [0, n_nodes) (the callers check on the host); sel: n_sel distinct indices in [0, 24)
int stan_scalars_device(stan_ctx *ctx, int64_t n_nodes, const double *d_disp, int64_t n_elem, const int32_t *d_conn,
                        const double *d_strain, const double *d_stress, int32_t n_sel, const int32_t *sel, double *d_point,
                        double *d_cell) {
    scal_sel ss{};
    for (int32_t k = 0; k < n_sel; k++) { ss.mask |= 1u << sel[k]; ss.row[sel[k]] = (int8_t)k; }
    hipStream_t st = ctx->stream;
    const int64_t n_inc = n_elem * 8;
    phase_timer pt(ctx, 5);   // cell kernel [0, 1] | list [2, 3] | point kernel [3, 4]
    ctx->prof.scalars_cell_ms = ctx->prof.scalars_list_ms = ctx->prof.scalars_point_ms = 0;
    if (d_cell && n_elem > 0) {
        STANCHK(pt.mark(0));
        hipLaunchKernelGGL(k_scalars_cell, dim3(nblk(n_inc, 256)), dim3(256), 0, st, n_elem, d_conn, d_disp, d_strain, d_stress,
                           ss, d_cell);
        STANCHK(pt.mark(1));
    }
    if (d_point) {
        dev_scope tmp(ctx);
        int32_t *d_list;
        int64_t *d_ptr;
        STANCHK(pt.mark(2));
        STANCHK(stan_incidence_lists(ctx, tmp, n_nodes, n_elem, d_conn, false, &d_ptr, &d_list));
        STANCHK(pt.mark(3));
        hipLaunchKernelGGL(k_scalars_point, dim3(nblk(n_nodes, 256)), dim3(256), 0, st, n_nodes, d_ptr, d_list, d_disp, d_strain,
                           d_stress, ss, d_point);
        STANCHK(pt.mark(4));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));   // the temporaries go back to the context behind the kernels
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (d_cell && n_elem > 0) STANCHK(pt.read(0, 1, &ctx->prof.scalars_cell_ms));
    if (d_point) {
        STANCHK(pt.read(2, 3, &ctx->prof.scalars_list_ms));
        STANCHK(pt.read(3, 4, &ctx->prof.scalars_point_ms));
    }
    return STAN_OK;
}
