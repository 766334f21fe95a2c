// api_harmonic.hip -- the extern "C" surface of the frequency response: the steady-state response to a
// harmonic load by modal superposition with a static correction.  The driver checks every argument before the first launch,
// projects the load on the modes (two passes over Phi, harmonic.hip), forms the coefficient table on the host in fp64 and runs the
// fused sweep, the snapshots and the probes on it.  With Phi^T M Phi = I the response needs neither K nor M: one entry serves the
// lumped mass and the consistent mass alike.  One device, one rank.
#include <algorithm>
#include <cmath>

#include "api_stage.h"

namespace {

struct hm_run {   // what both entries check on the host and hand to the driver
    int64_t N;
    int32_t k, n_freq, n_probe, n_snap;
    std::vector<double> lambda;      // [k], host
    std::vector<double> g, h;        // [n_freq][k]: d / D and e / D of the table, formed before anything is launched
    const int32_t *snap_freq;        // [n_snap], host
};

int harmonic_refused(stan_ctx *ctx) {
    STAN_NO_GROUP(ctx, "harmonic (the projection's sums and the sweep run on one device)");
    if (stan_sharded(ctx)) {
        ctx->err = "harmonic: not available on a context with a communicator (the projection's sums are not reduced over ranks)";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

// the host checks of both entries that need no array in device memory
int harmonic_args(stan_ctx *ctx, int64_t N, int32_t n_modes, const void *lambda, const void *phi, const void *F, double alpha_R,
                  double beta_R, const double *zeta, int32_t n_freq, const double *omega, int32_t n_probe, const void *probe_dof,
                  const void *probe, int32_t n_snap, const int32_t *snap_freq, const void *snaps, const void *p, const void *peak,
                  const void *peak_idx) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(harmonic_refused(ctx));
    auto bad = [&](const std::string &why) { ctx->err = "harmonic: " + why; return STAN_E_ARG; };
    if (N <= 0 || N > ((int64_t)1 << 31) - 1) return bad("N must be in [1, 2^31)");
    if (n_modes <= 0 || n_modes > STAN_MODAL_QMAX) return bad("n_modes must be in [1, 32]");
    if (n_freq <= 0 || n_freq > 65536) return bad("n_freq must be in [1, 65536]");
    if (n_probe < 0 || n_snap < 0) return bad("n_probe and n_snap must be >= 0");
    if (!lambda || !phi || !F || !omega || !p) return bad("null argument");
    if (!peak != !peak_idx) return bad("peak and peak_idx go together");
    if (n_probe > 0 && probe && !probe_dof) return bad("null probe_dof");
    if (n_snap > 0 && snaps && !snap_freq) return bad("null snap_freq");
    if (!(alpha_R >= 0) || !std::isfinite(alpha_R) || !(beta_R >= 0) || !std::isfinite(beta_R))
        return bad("alpha_R and beta_R must be >= 0 and finite");
    for (int j = 0; zeta && j < n_modes; j++)
        if (!(zeta[j] >= 0) || !std::isfinite(zeta[j])) return bad("zeta[" + std::to_string(j) + "] must be >= 0 and finite");
    for (int f = 0; f < n_freq; f++)
        if (!(omega[f] >= 0) || !std::isfinite(omega[f])) return bad("omega[" + std::to_string(f) + "] must be >= 0 and finite");
    for (int s = 0; snaps && s < n_snap; s++)
        if (snap_freq[s] < 0 || snap_freq[s] >= n_freq) return bad("snap_freq[" + std::to_string(s) + "] is outside [0, n_freq)");
    return STAN_OK;
}

// lambda on the host: its check and the table's two factors per (frequency, mode), in this order of operations:
//   c = fma(2 zeta_j, sqrt(lambda_j), fma(beta_R, lambda_j, alpha_R));  d = fma(-w, w, lambda_j);  e = w c;  D = fma(d, d, e e);
//   g = d / D;  h = e / D                                  (the table is a = p_j g, b = -(p_j h) once p is known)
int harmonic_table(stan_ctx *ctx, double alpha_R, double beta_R, const double *zeta, const double *omega, hm_run *P) {
    auto bad = [&](const std::string &why) { ctx->err = "harmonic: " + why; return STAN_E_ARG; };
    const int k = P->k;
    for (int j = 0; j < k; j++)
        if (!(P->lambda[(size_t)j] > 0) || !std::isfinite(P->lambda[(size_t)j])) return bad("lambda[" + std::to_string(j) + "] is not positive and finite");
    P->g.resize((size_t)P->n_freq * k); P->h.resize((size_t)P->n_freq * k);
    for (int f = 0; f < P->n_freq; f++)
        for (int j = 0; j < k; j++) {
            const double lam = P->lambda[(size_t)j], w = omega[f];
            const double c = std::fma(2.0 * (zeta ? zeta[j] : 0.0), std::sqrt(lam), std::fma(beta_R, lam, alpha_R));
            const double d = std::fma(-w, w, lam), e = w * c;
            const double D = std::fma(d, d, e * e);
            if (D == 0.0 || !std::isfinite(D))
                return bad("the denominator of frequency " + std::to_string(f) + " and mode " + std::to_string(j) +
                           " is zero or not finite (an undamped load on a resonance?)");
            P->g[(size_t)f * k + j] = d / D;
            P->h[(size_t)f * k + j] = e / D;
        }
    return STAN_OK;
}

// The driver on device arrays.  Every check is made and every temporary allocated before the first kernel that stores an output.
int harmonic_device(stan_ctx *ctx, const hm_run &P, const double *d_phi, const double *d_F, const double *d_us, const int32_t *d_probe_dof,
                    double *d_probe, double *d_snaps, double *d_p, double *d_peak, int32_t *d_peak_idx, stan_harmonic_report *rep) {
    stan_harmonic_report R{};
    report_out<stan_harmonic_report> report{rep, R};   // first: written on every way out behind the argument checks
    R.n_modes = P.k; R.n_freq = P.n_freq; R.peak_dof = -1; R.peak_freq = -1; R.static_correction = d_us ? 1 : 0;
    const int64_t N = P.N;
    const int k = P.k, QT = stan_harmonic_width(k);
    const bool probes = P.n_probe > 0 && d_probe, snaps = P.n_snap > 0 && d_snaps;
    hipStream_t st = ctx->stream;
    piece_timer pt(ctx);

    if (probes) {
        int64_t bad_at;
        STANCHK(stan_newmark_probe_check_device(ctx, N, P.n_probe, d_probe_dof, &bad_at));
        if (bad_at >= 0) { ctx->err = "harmonic: probe_dof[" + std::to_string(bad_at) + "] is outside [0, N)"; return STAN_E_ARG; }
    }
    const int64_t nb = stan_harmonic_blocks(N);
    dev_scope tmp(ctx);
    double *partial, *r = nullptr, *tab, *pval = nullptr, *top = nullptr;
    long long *pidx = nullptr, *top_idx = nullptr;
    int32_t *d_snap_freq = nullptr;
    STANCHK(tmp.alloc(&partial, (size_t)k * (size_t)nb));
    if (d_us) STANCHK(tmp.alloc(&r, (size_t)N));
    STANCHK(tmp.alloc(&tab, 2 * (size_t)P.n_freq * (size_t)QT));
    if (snaps) STANCHK(tmp.alloc(&d_snap_freq, (size_t)P.n_snap));
    if (d_peak) {
        STANCHK(tmp.alloc(&pval, (size_t)nb)); STANCHK(tmp.alloc(&pidx, (size_t)nb));
        STANCHK(tmp.alloc(&top, 1)); STANCHK(tmp.alloc(&top_idx, 2));
    }

    // project: p, then r
    std::vector<double> p((size_t)k), c((size_t)k);
    pt.begin();
    STANCHK(stan_harmonic_dots_device(ctx, N, k, d_phi, d_F, partial, d_p));
    HIPCHK(ctx, hipMemcpyAsync(p.data(), d_p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int j = 0; j < k; j++) c[(size_t)j] = p[(size_t)j] / P.lambda[(size_t)j];
    if (d_us) STANCHK(stan_harmonic_residual_device(ctx, N, k, d_phi, d_us, c.data(), r));
    pt.end(&R.project_ms);

    // the table, [n_freq][QT] pairs, zeros beyond k; the host copy outlives the stream's (the synchronisation at the end)
    std::vector<double> table(2 * (size_t)P.n_freq * (size_t)QT, 0.0);
    for (int f = 0; f < P.n_freq; f++)
        for (int j = 0; j < k; j++) {
            table[2 * ((size_t)f * QT + j)] = p[(size_t)j] * P.g[(size_t)f * k + j];
            table[2 * ((size_t)f * QT + j) + 1] = -(p[(size_t)j] * P.h[(size_t)f * k + j]);
        }
    HIPCHK(ctx, hipMemcpyAsync(tab, table.data(), table.size() * 8, hipMemcpyHostToDevice, st));
    if (snaps) HIPCHK(ctx, hipMemcpyAsync(d_snap_freq, P.snap_freq, (size_t)P.n_snap * 4, hipMemcpyHostToDevice, st));

    if (d_peak) {
        pt.begin();
        STANCHK(stan_harmonic_sweep_device(ctx, N, k, P.n_freq, d_phi, r, tab, d_peak, d_peak_idx));
        STANCHK(stan_harmonic_peakmax_device(ctx, N, d_peak, d_peak_idx, pval, pidx, top, top_idx));
        pt.end(&R.sweep_ms);
    }
    if (snaps) {
        pt.begin();
        STANCHK(stan_harmonic_snap_device(ctx, N, k, P.n_snap, d_snap_freq, d_phi, r, tab, d_snaps));
        pt.end(&R.snap_ms);
    }
    if (probes) {
        pt.begin();
        STANCHK(stan_harmonic_probe_device(ctx, N, k, P.n_freq, P.n_probe, d_probe_dof, d_phi, r, tab, d_probe));
        pt.end(&R.probe_ms);
    }
    double top_h = 0.0;
    long long top_idx_h[2] = {-1, -1};
    if (d_peak) {
        HIPCHK(ctx, hipMemcpyAsync(&top_h, top, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(top_idx_h, top_idx, 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (d_peak) {
        // no row at all: every entry of peak is NaN (phi or F not finite) and none compares larger than another
        const bool none = top_idx_h[0] < 0 || top_idx_h[0] >= N;
        R.peak = none ? std::nan("") : top_h;
        R.peak_dof = none ? -1 : (int64_t)top_idx_h[0];
        R.peak_freq = none ? -1 : (int32_t)top_idx_h[1];
    }
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_harmonic_dev(stan_ctx *ctx, int64_t N, int32_t n_modes, const double *d_lambda, const double *d_phi, const double *d_F,
                          const double *d_u_static, double alpha_R, double beta_R, const double *zeta, int32_t n_freq, const double *omega,
                          int32_t n_probe, const int32_t *d_probe_dof, double *d_probe, int32_t n_snap, const int32_t *snap_freq,
                          double *d_snaps, double *d_p, double *d_peak, int32_t *d_peak_idx, void *rep) {
    STANCHK(harmonic_args(ctx, N, n_modes, d_lambda, d_phi, d_F, alpha_R, beta_R, zeta, n_freq, omega, n_probe, d_probe_dof, d_probe, n_snap,
                          snap_freq, d_snaps, d_p, d_peak, d_peak_idx));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hm_run P{N, n_modes, n_freq, n_probe, n_snap, std::vector<double>((size_t)n_modes), {}, {}, snap_freq};
    HIPCHK(ctx, hipMemcpyAsync(P.lambda.data(), d_lambda, (size_t)n_modes * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    STANCHK(harmonic_table(ctx, alpha_R, beta_R, zeta, omega, &P));
    return harmonic_device(ctx, P, d_phi, d_F, d_u_static, d_probe_dof, d_probe, d_snaps, d_p, d_peak, d_peak_idx, (stan_harmonic_report *)rep);
}

int stan_hip_harmonic(stan_ctx *ctx, int64_t N, int32_t n_modes, const double *lambda, const double *phi, const double *F,
                      const double *u_static, double alpha_R, double beta_R, const double *zeta, int32_t n_freq, const double *omega,
                      int32_t n_probe, const int32_t *probe_dof, double *probe, int32_t n_snap, const int32_t *snap_freq, double *snaps,
                      double *p, double *peak, int32_t *peak_idx, void *rep) {
    STANCHK(harmonic_args(ctx, N, n_modes, lambda, phi, F, alpha_R, beta_R, zeta, n_freq, omega, n_probe, probe_dof, probe, n_snap, snap_freq,
                          snaps, p, peak, peak_idx));
    hm_run P{N, n_modes, n_freq, n_probe, n_snap, std::vector<double>(lambda, lambda + n_modes), {}, {}, snap_freq};
    STANCHK(harmonic_table(ctx, alpha_R, beta_R, zeta, omega, &P));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N, k = (size_t)n_modes;
    const bool probes = n_probe > 0 && probe, with_snaps = n_snap > 0 && snaps;
    host_stage st(ctx);
    dbuf<double> dphi, dF, dus, dpr, dsn, dp, dpk;
    dbuf<int32_t> dpd, dpi;
    STANCHK(dphi.upload(st, phi, k * n));
    STANCHK(dF.upload(st, F, n));
    if (u_static) STANCHK(dus.upload(st, u_static, n));
    if (probes) {
        STANCHK(dpd.upload(st, probe_dof, (size_t)n_probe));
        STANCHK(dpr.alloc(st, 2 * (size_t)n_freq * (size_t)n_probe, probe));
    }
    if (with_snaps) STANCHK(dsn.alloc(st, 2 * (size_t)n_snap * n, snaps));
    STANCHK(dp.alloc(st, k, p));
    STANCHK(dpk.out(st, peak, n));
    STANCHK(dpi.out(st, peak_idx, n));
    const int rc = harmonic_device(ctx, P, dphi.p, dF.p, dus.p, dpd.p, dpr.p, dsn.p, dp.p, dpk.p, dpi.p, (stan_harmonic_report *)rep);
    return st.finish(rc, dpr, dsn, dp, dpk, dpi);
}

}  // extern "C"
