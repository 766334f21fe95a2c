// api_modal.hip -- the extern "C" surface, part 5 of 5: the modal analysis.  The driver loop of stan_hip_modes (block inverse iteration in
// correction form with a Rayleigh-Ritz step) over the solver's batched CG (stan_cg_multi_device), its
// products (stan_spmv_reduced) and the block kernels of modal.hip; the q x q eigenproblem on the host; the two block helpers.
// One device, one rank (block_driver_refused, api_stage.h).  What the loop shares with the buckling driver's (the checks and
// defaults, the solves, the products, the packing, the tail) is block_run of api_stage.h.
#include <algorithm>
#include <cmath>

#include "api_stage.h"

// A Q = B Q Lambda for symmetric A and symmetric positive definite B, q x q row-major: B = L L^T, C = L^-1 A L^-T, cyclic
// Jacobi on C (C = V Theta V^T), Lambda = Theta ascending (descending: descending; stably either way), Q = L^-T V: Q^T B Q = I.
// false: B is not positive definite.  Shared with the buckling driver (api_stage.h).
bool stan_small_gen_eig(int q, const double *A, const double *B, double *lambda, double *Q, bool descending) {
    std::vector<double> L((size_t)q * q, 0.0), Cm((size_t)q * q), V((size_t)q * q, 0.0), T((size_t)q * q);
    auto at = [q](std::vector<double> &m, int i, int j) -> double & { return m[(size_t)i * q + j]; };
    for (int j = 0; j < q; j++) {
        double d = B[j * q + j];
        for (int k = 0; k < j; k++) d -= at(L, j, k) * at(L, j, k);
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        at(L, j, j) = std::sqrt(d);
        for (int i = j + 1; i < q; i++) {
            double s = 0.5 * (B[i * q + j] + B[j * q + i]);
            for (int k = 0; k < j; k++) s -= at(L, i, k) * at(L, j, k);
            at(L, i, j) = s / at(L, j, j);
        }
    }
    // T = L^-1 Asym (forward substitution, column by column), C = T L^-T = (L^-1 T^T)^T
    for (int c = 0; c < q; c++)
        for (int i = 0; i < q; i++) {
            double s = 0.5 * (A[i * q + c] + A[c * q + i]);
            for (int k = 0; k < i; k++) s -= at(L, i, k) * at(T, k, c);
            at(T, i, c) = s / at(L, i, i);
        }
    for (int r = 0; r < q; r++)       // row r of T is a right-hand side: C[r][.] = L^-1 T[r][.]^T
        for (int i = 0; i < q; i++) {
            double s = at(T, r, i);
            for (int k = 0; k < i; k++) s -= at(L, i, k) * at(Cm, r, k);
            at(Cm, r, i) = s / at(L, i, i);
        }
    for (int i = 0; i < q; i++)
        for (int j = i + 1; j < q; j++) at(Cm, i, j) = at(Cm, j, i) = 0.5 * (at(Cm, i, j) + at(Cm, j, i));
    for (int i = 0; i < q; i++) at(V, i, i) = 1.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < q; i++) {
            diag += at(Cm, i, i) * at(Cm, i, i);
            for (int j = i + 1; j < q; j++) off += at(Cm, i, j) * at(Cm, i, j);
        }
        if (off == 0.0 || off <= 1e-40 * diag) break;
        for (int p = 0; p < q - 1; p++)
            for (int r = p + 1; r < q; r++) {
                const double apr = at(Cm, p, r);
                if (apr == 0.0) continue;
                const double theta = (at(Cm, r, r) - at(Cm, p, p)) / (2.0 * apr);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < q; k++) {   // columns p, r
                    const double akp = at(Cm, k, p), akr = at(Cm, k, r);
                    at(Cm, k, p) = c * akp - s * akr;
                    at(Cm, k, r) = s * akp + c * akr;
                }
                for (int k = 0; k < q; k++) {   // rows p, r
                    const double apk = at(Cm, p, k), ark = at(Cm, r, k);
                    at(Cm, p, k) = c * apk - s * ark;
                    at(Cm, r, k) = s * apk + c * ark;
                }
                at(Cm, p, r) = at(Cm, r, p) = 0.0;
                for (int k = 0; k < q; k++) {
                    const double vkp = at(V, k, p), vkr = at(V, k, r);
                    at(V, k, p) = c * vkp - s * vkr;
                    at(V, k, r) = s * vkp + c * vkr;
                }
            }
    }
    std::vector<int> order((size_t)q);
    for (int i = 0; i < q; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return descending ? at(Cm, x, x) > at(Cm, y, y) : at(Cm, x, x) < at(Cm, y, y); });
    for (int j = 0; j < q; j++) {
        const int src = order[(size_t)j];
        lambda[j] = at(Cm, src, src);
        for (int i = q - 1; i >= 0; i--) {   // L^T y = v (back substitution)
            double s = at(V, i, src);
            for (int k = i + 1; k < q; k++) s -= at(L, k, i) * Q[k * q + j];
            Q[i * q + j] = s / at(L, i, i);
        }
    }
    return true;
}

namespace {

// the driver on device arrays: d_M [N], d_lambda / d_rho [k], d_phi [k][N]
int modes_device(stan_ctx *ctx, stan_matrix *K, const double *d_M, int32_t k, double tol, int32_t max_outer, double solve_eps,
                 int32_t solve_max_its, double *d_lambda, double *d_phi, double *d_rho, stan_modes_report *rep) {
    // what every refusal of a K that is not positive definite ends with: the way such a model is analysed
    const std::string free_hint = "a model without supports?  Analyse the shifted problem K + sigma M: stan_hip_matrix_shifted, stan_solver --modes-shift SIGMA";
    block_run<stan_modes_report> run(ctx, K, "modes", k, tol, max_outer, solve_eps, solve_max_its);
    STANCHK(run.begin(rep));
    stan_modes_report &R = run.R;
    piece_timer &pt = run.pt;
    const int64_t N = run.N;
    const int q = run.q;

    dev_scope tmp(ctx);
    double *Z, *W, *rhs, *D;   // [q][N] each; X lives in Z, K X in W
    const size_t qn = (size_t)q * (size_t)N;
    STANCHK(tmp.alloc(&Z, qn));
    STANCHK(tmp.alloc(&W, qn));
    STANCHK(tmp.alloc(&rhs, qn));
    STANCHK(tmp.alloc(&D, qn));
    int64_t bad_row;
    pt.begin();
    STANCHK(stan_modal_start_device(ctx, N, q, d_M, rhs, &bad_row));
    pt.end(&R.block_ms);
    if (bad_row >= 0) return run.bad("M[" + std::to_string(bad_row) + "] is not positive and finite", STAN_E_ARG);
    STANCHK(run.solve(q, rhs, Z, free_hint));

    std::vector<double> A((size_t)q * q), B((size_t)q * q), Qm((size_t)q * q), lam((size_t)q), rho2((size_t)q), rho((size_t)q);
    for (;;) {
        R.outer++;
        STANCHK(run.products(K, Z, W));
        pt.begin();
        STANCHK(stan_modal_gram_device(ctx, N, q, Z, W, d_M, A.data(), B.data()));
        pt.end(&R.gram_ms);
        if (!stan_small_gen_eig(q, A.data(), B.data(), lam.data(), Qm.data()))
            return run.bad("the block lost rank (Z^T M Z is not positive definite: " + free_hint + ")", STAN_E_UNSUPPORTED);
        for (int j = 0; j < q; j++)
            if (!(lam[(size_t)j] > 0.0))
                return run.bad("Ritz value " + std::to_string(j) + " is not positive (K is not positive definite: " + free_hint + ")", STAN_E_UNSUPPORTED);
        const bool last = R.outer >= run.max_outer;
        pt.begin();   // the last step needs no right-hand side: every column masked
        STANCHK(stan_modal_rotate_device(ctx, N, q, Z, W, d_M, Qm.data(), lam.data(), last ? 0xffffffffu : 0u, Z, W, rhs, rho2.data()));
        pt.end(&R.rotate_ms);
        bool done = true;
        R.max_rho = 0.0;
        for (int j = 0; j < q; j++) {
            rho[(size_t)j] = std::sqrt(rho2[(size_t)j]) / lam[(size_t)j];
            if (j < k) {
                done = done && rho[(size_t)j] <= run.tol;
                R.max_rho = std::max(R.max_rho, rho[(size_t)j]);
            }
        }
        R.converged = done ? 1 : 0;
        if (done || last) break;
        // K D = -R Lambda^-1 for the columns that have not converged (a column is left out where rho <= tol), then
        // Z = X Lambda^-1 + D
        int n;
        STANCHK(run.pack(rhs, [&](int j) { return !(rho[(size_t)j] <= run.tol); }, &n));
        STANCHK(run.solve(n, rhs, D, free_hint));
        pt.begin();
        STANCHK(stan_modal_axpy_device(ctx, N, q, Z, lam.data(), run.dcol.data(), D, Z));
        pt.end(&R.block_ms);
    }
    pt.begin();
    STANCHK(stan_modal_normalise_device(ctx, N, k, Z, d_M, d_phi));
    pt.end(&R.block_ms);
    return run.finish(lam.data(), rho.data(), d_lambda, d_rho);
}

int modes_args(stan_ctx *ctx, stan_matrix *K, const void *M, const void *lambda, const void *phi, const void *rho) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(block_driver_refused(ctx, "modes"));
    if (!K || !M || !lambda || !phi || !rho) { ctx->err = "modes: null argument"; return STAN_E_ARG; }
    if (K->ctx != ctx) { ctx->err = "modes: K belongs to another context"; return STAN_E_ARG; }
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_modes_dev(stan_ctx *ctx, stan_matrix *K, const double *d_M, int32_t n_modes, double tol, int32_t max_outer,
                       double solve_eps, int32_t solve_max_its, double *d_lambda, double *d_phi, double *d_rho, void *rep) {
    STANCHK(modes_args(ctx, K, d_M, d_lambda, d_phi, d_rho));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return modes_device(ctx, K, d_M, n_modes, tol, max_outer, solve_eps, solve_max_its, d_lambda, d_phi, d_rho, (stan_modes_report *)rep);
}

int stan_hip_modes(stan_ctx *ctx, stan_matrix *K, const double *M, int32_t n_modes, double tol, int32_t max_outer, double solve_eps,
                   int32_t solve_max_its, double *lambda, double *phi, double *rho, void *rep) {
    STANCHK(modes_args(ctx, K, M, lambda, phi, rho));
    if (n_modes <= 0 || n_modes > K->n_red) { ctx->err = "modes: n_modes must be in [1, N]"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red, k = (size_t)n_modes;
    host_stage st(ctx);
    dbuf<double> dM, dl, dp, dr;
    STANCHK(dM.upload(st, M, N));
    STANCHK(dl.alloc(st, k, lambda));
    STANCHK(dp.alloc(st, k * N, phi));
    STANCHK(dr.alloc(st, k, rho));
    const int rc = modes_device(ctx, K, dM.p, n_modes, tol, max_outer, solve_eps, solve_max_its, dl.p, dp.p, dr.p, (stan_modes_report *)rep);
    return st.finish(rc, dl, dp, dr);
}

int stan_hip_block_gram(stan_ctx *ctx, int64_t N, int32_t q, const double *Z, const double *W, const double *M, double *A, double *B) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(block_driver_refused(ctx, "block_gram"));
    if (!Z || !W || !M || !A || !B || N <= 0 || q <= 0 || q > STAN_MODAL_QMAX) { ctx->err = "block_gram: null argument, N <= 0 or q outside [1, 32]"; return STAN_E_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dZ, dW, dM;
    STANCHK(dZ.upload(st, Z, (size_t)q * (size_t)N));
    STANCHK(dW.upload(st, W, (size_t)q * (size_t)N));
    STANCHK(dM.upload(st, M, (size_t)N));
    return st.finish(stan_modal_gram_device(ctx, N, q, dZ.p, dW.p, dM.p, A, B));
}

int stan_hip_block_rotate(stan_ctx *ctx, int64_t N, int32_t q, const double *Z, const double *W, const double *M, const double *Q,
                          const double *lambda, const uint8_t *mask, int32_t in_place, double *X, double *KX, double *rhs,
                          double *rho2) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(block_driver_refused(ctx, "block_rotate"));
    if (!Z || !W || !M || !Q || !lambda || !X || !KX || !rhs || !rho2 || N <= 0 || q <= 0 || q > STAN_MODAL_QMAX) {
        ctx->err = "block_rotate: null argument, N <= 0 or q outside [1, 32]";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint32_t bits = 0;
    for (int j = 0; mask && j < q; j++) bits |= mask[j] ? 1u << j : 0u;
    const size_t qn = (size_t)q * (size_t)N;
    host_stage st(ctx);
    dbuf<double> dZ, dW, dM, dX, dKX, dR;
    STANCHK(dZ.upload(st, Z, qn, in_place ? X : nullptr));
    STANCHK(dW.upload(st, W, qn, in_place ? KX : nullptr));
    STANCHK(dM.upload(st, M, (size_t)N));
    if (!in_place) {
        STANCHK(dX.alloc(st, qn, X));
        STANCHK(dKX.alloc(st, qn, KX));
    }
    STANCHK(dR.upload(st, rhs, qn, rhs));
    const int rc = stan_modal_rotate_device(ctx, N, q, dZ.p, dW.p, dM.p, Q, lambda, bits, in_place ? dZ.p : dX.p, in_place ? dW.p : dKX.p,
                                            dR.p, rho2);
    return st.finish(rc, dZ, dW, dX, dKX, dR);
}

}  // extern "C"
