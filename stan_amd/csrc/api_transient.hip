// api_transient.hip -- the extern "C" surface of the transient dynamics: the driver loop of stan_hip_transient (implicit Newmark
// steps) over the shifted matrix K + sigma M (matrix_shift.hip), the solver's CG (stan_cg_device), its
// products (stan_spmv_reduced) and the step kernels of transient.hip; the load curve on the host; the two step helpers.
// One device, one rank (transient_refused).
#include <algorithm>
#include <cmath>

#include "api_stage.h"

namespace {

struct nm_run {   // what both entries check on the host and hand to the driver
    double dt, beta_N, gamma, alpha_R, beta_R, solve_eps;
    int32_t n_steps, n_curve, solve_max_its, n_probe, snap_every;
    const double *curve_t, *curve_g;
};

// the piecewise-linear curve at x: constant before the first and after the last point; the segment is that of the LAST point
// with t <= x (a repeated t is a jump); no point: 1
double curve_at(const nm_run &P, double x) {
    const int n = P.n_curve;
    if (n == 0) return 1.0;
    if (x <= P.curve_t[0]) return P.curve_g[0];
    if (x >= P.curve_t[n - 1]) return P.curve_g[n - 1];
    const int i = (int)(std::upper_bound(P.curve_t, P.curve_t + n, x) - P.curve_t) - 1;
    const double t0 = P.curve_t[i], t1 = P.curve_t[i + 1];
    return P.curve_g[i] + (P.curve_g[i + 1] - P.curve_g[i]) * ((x - t0) / (t1 - t0));
}

stan_newmark_coef make_coef(double dt, double beta_N, double gamma, double alpha_R, double beta_R) {
    stan_newmark_coef c;
    c.a0 = 1.0 / (beta_N * dt * dt);
    c.a1 = gamma / (beta_N * dt);
    c.a2 = 1.0 / (beta_N * dt);
    c.a3 = 1.0 / (2.0 * beta_N) - 1.0;
    c.a4 = gamma / beta_N - 1.0;
    c.a5 = dt * (gamma / (2.0 * beta_N) - 1.0);
    c.alpha_R = alpha_R; c.beta_R = beta_R;
    c.c_K = 1.0 + c.a1 * beta_R;
    c.dt = dt; c.gamma = gamma;
    return c;
}

// One device, one rank: the shift pass walks one rank's rows, the solves are a single-rank context's, the step kernels' sums are
// not reduced over ranks
int transient_refused(stan_ctx *ctx, const char *entry) {
    STAN_NO_GROUP(ctx, std::string(entry) + " (the shifted matrix, its solves and the step kernels run on one device)");
    if (stan_sharded(ctx)) {
        ctx->err = std::string(entry) + ": not available on a context with a communicator (the shift pass and the step sums are one rank's)";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

// the host checks of both entries; fills P (defaults applied)
int transient_args(stan_ctx *ctx, stan_matrix *K, const void *M, const void *F, double dt, int32_t n_steps, double beta_N, double gamma,
                   double alpha_R, double beta_R, int32_t n_curve, const double *curve_t, const double *curve_g, double solve_eps,
                   int32_t solve_max_its, int32_t n_probe, const void *probe_dof, const void *probe_u, int32_t snap_every,
                   const void *u_end, const void *v_end, const void *a_end, nm_run *P) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(transient_refused(ctx, "transient"));
    auto bad = [&](const char *why) { ctx->err = std::string("transient: ") + why; return STAN_E_ARG; };
    if (!K || !M || !F || !u_end || !v_end || !a_end) return bad("null argument");
    if (K->ctx != ctx) return bad("K belongs to another context");
    if (!(dt > 0) || !std::isfinite(dt)) return bad("dt must be positive and finite");
    if (n_steps < 0 || n_curve < 0 || n_probe < 0 || snap_every < 0 || solve_max_its < 0) return bad("n_steps, n_curve, n_probe, snap_every and solve_max_its must be >= 0");
    if (!(solve_eps >= 0) || !std::isfinite(solve_eps)) return bad("solve_eps must be >= 0");
    if (!(alpha_R >= 0) || !(beta_R >= 0) || !std::isfinite(alpha_R) || !std::isfinite(beta_R)) return bad("alpha_R and beta_R must be >= 0");
    if (beta_N == 0 && gamma == 0) { beta_N = 0.25; gamma = 0.5; }
    if (!std::isfinite(beta_N) || !std::isfinite(gamma) || !(gamma >= 0.5) || !(beta_N >= (gamma + 0.5) * (gamma + 0.5) / 4))
        return bad("the Newmark parameters must satisfy gamma >= 1/2 and beta_N >= (gamma + 1/2)^2 / 4");
    if (n_curve > 0 && (!curve_t || !curve_g)) return bad("null load curve");
    for (int i = 0; i < n_curve; i++) {
        if (!std::isfinite(curve_t[i]) || !std::isfinite(curve_g[i])) return bad("a load curve value is not finite");
        if (i > 0 && curve_t[i] < curve_t[i - 1]) return bad("the load curve's t must not descend");
    }
    if (n_probe > 0 && (!probe_dof || !probe_u)) return bad("null probe argument");
    if ((int64_t)n_probe * ((int64_t)n_steps + 1) > ((int64_t)1 << 40)) return bad("probe table too large");
    if (solve_eps == 0 && solve_max_its == 0) solve_eps = 1e-6;   // lincgsetcond
    *P = nm_run{dt, beta_N, gamma, alpha_R, beta_R, solve_eps, n_steps, n_curve, solve_max_its, n_probe, snap_every, curve_t, curve_g};
    return STAN_OK;
}

int64_t snap_count(const nm_run &P, const double *snaps) { return snaps && P.snap_every > 0 ? P.n_steps / P.snap_every + 1 : 0; }

// The driver on device arrays.  The inputs are copied into vectors of the driver's own (16-byte aligned, what the step kernels
// take; a caller's pointer is only read by copies and by the one-element-wide shift pass), the outputs are collected in
// tables of its own and copied out at the end of a run that succeeded: an error leaves the caller's outputs untouched.
int transient_device(stan_ctx *ctx, stan_matrix *K, const double *d_Min, const double *d_Fin, const double *d_u0, const double *d_v0,
                     const nm_run &P, const int32_t *d_probe, double *d_probe_u, double *d_snaps, double *d_energy, double *d_u_end,
                     double *d_v_end, double *d_a_end, stan_transient_report *rep) {
    auto bad = [&](const std::string &why, int rc) { ctx->err = "transient: " + why; return rc; };
    const int64_t N = K->n_red;
    if (N <= 0) return bad("the matrix has no free DOF", STAN_E_ARG);
    const size_t n = (size_t)N, nb = n * 8;
    stan_transient_report R{};
    report_out<stan_transient_report> report{rep, R};
    const stan_newmark_coef c = make_coef(P.dt, P.beta_N, P.gamma, P.alpha_R, P.beta_R);
    R.sigma = (c.a0 + c.a1 * P.alpha_R) / c.c_K;
    if (!std::isfinite(R.sigma) || !std::isfinite(c.a0)) return bad("dt is too small: 1 / (beta_N dt^2) is not finite", STAN_E_ARG);
    piece_timer pt(ctx);
    hipStream_t st = ctx->stream;
    const bool damped_K = P.beta_R != 0.0;

    int64_t bad_at;
    STANCHK(stan_mass_check_device(ctx, N, d_Min, &bad_at));
    if (bad_at >= 0) return bad("M[" + std::to_string(bad_at) + "] is not positive and finite", STAN_E_ARG);
    STANCHK(stan_newmark_probe_check_device(ctx, N, P.n_probe, d_probe, &bad_at));
    if (bad_at >= 0) return bad("probe_dof[" + std::to_string(bad_at) + "] is outside [0, N)", STAN_E_ARG);

    const int64_t n_snap = snap_count(P, d_snaps);
    const size_t n_rows = (size_t)P.n_steps + 1;
    dev_scope tmp(ctx);
    double *M, *F, *u, *v, *a, *b, *un, *w = nullptr, *Kx = nullptr, *t_probe = nullptr, *t_energy = nullptr, *partial = nullptr, *t_snaps = nullptr;
    STANCHK(tmp.alloc(&M, n)); STANCHK(tmp.alloc(&F, n));
    STANCHK(tmp.alloc(&u, n)); STANCHK(tmp.alloc(&v, n)); STANCHK(tmp.alloc(&a, n));
    STANCHK(tmp.alloc(&b, n)); STANCHK(tmp.alloc(&un, n));
    if (damped_K) STANCHK(tmp.alloc(&w, n));
    if (damped_K || d_energy) STANCHK(tmp.alloc(&Kx, n));
    if (P.n_probe > 0) STANCHK(tmp.alloc(&t_probe, n_rows * (size_t)P.n_probe));
    if (d_energy) {
        STANCHK(tmp.alloc(&t_energy, n_rows * 3));
        STANCHK(tmp.alloc(&partial, 3 * (size_t)stan_newmark_blocks(N)));
    }
    if (n_snap > 0) STANCHK(tmp.alloc(&t_snaps, (size_t)n_snap * 3 * n));
    HIPCHK(ctx, hipMemcpyAsync(M, d_Min, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(F, d_Fin, nb, hipMemcpyDeviceToDevice, st));
    if (d_u0) HIPCHK(ctx, hipMemcpyAsync(u, d_u0, nb, hipMemcpyDeviceToDevice, st));
    else HIPCHK(ctx, hipMemsetAsync(u, 0, nb, st));
    if (d_v0) HIPCHK(ctx, hipMemcpyAsync(v, d_v0, nb, hipMemcpyDeviceToDevice, st));
    else HIPCHK(ctx, hipMemsetAsync(v, 0, nb, st));

    // The steps' solves run with ALGLIB's merit stop off, as under STAN_OPT_CG_MERIT_STOP 0: that stop is there for the static
    // solve's parity with the reference, which has no transient analysis; its type 7 ("no further progress": near 1e-7 on
    // these systems, and now and then above 1e-6 on a stiffness-dominated step) would end a run that the loop can finish.
    merit_off merit(ctx);
    stan_matrix *S = nullptr;
    struct shifted_guard {   // freed on every way out
        stan_matrix *&s;
        ~shifted_guard() { if (s) stan_hip_matrix_free(s); }
    } sg{S};
    STANCHK(stan_matrix_shifted_device(ctx, K, R.sigma, M, &S, &R.shift_ms));

    auto product = [&](const double *x, double *y) -> int {
        pt.begin();
        STANCHK(stan_spmv_reduced(ctx, K, x, y));
        pt.end(&R.product_ms);
        return STAN_OK;
    };
    auto record = [&](int32_t step) -> int {   // the probes and the snapshot of the state after `step`
        if (t_probe) STANCHK(stan_newmark_probe_device(ctx, P.n_probe, d_probe, u, t_probe + (size_t)step * (size_t)P.n_probe));
        if (n_snap > 0 && step % P.snap_every == 0) {
            double *row = t_snaps + (size_t)(step / P.snap_every) * 3 * n;
            HIPCHK(ctx, hipMemcpyAsync(row, u, nb, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(row + n, v, nb, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(row + 2 * n, a, nb, hipMemcpyDeviceToDevice, st));
        }
        return STAN_OK;
    };

    // the start: a_0 from the equation of motion at t = 0 (the products in b and un, which the first step overwrites)
    const double g0 = curve_at(P, 0.0);
    const double *Kv0 = nullptr, *Ku0 = nullptr;
    if (d_v0 && damped_K) { STANCHK(product(v, b)); Kv0 = b; }
    if (d_u0) { STANCHK(product(u, un)); Ku0 = un; }
    pt.begin();
    STANCHK(stan_newmark_start_device(ctx, N, c, g0, F, M, d_v0 && P.alpha_R != 0.0 ? v : nullptr, Kv0, Ku0, a));
    pt.end(&R.step_ms);
    if (d_energy) {
        STANCHK(product(u, Kx));
        pt.begin();
        STANCHK(stan_newmark_energy_device(ctx, N, u, v, M, F, Kx, g0, partial, t_energy));
        pt.end(&R.step_ms);
    }
    STANCHK(record(0));

    R.cg_min_iterations = P.n_steps > 0 ? INT32_MAX : 0;
    for (int32_t step = 1; step <= P.n_steps; step++) {
        const double gF = curve_at(P, (double)step * P.dt);
        if (damped_K) {
            pt.begin();
            STANCHK(stan_newmark_w_device(ctx, N, c, u, v, a, w));
            pt.end(&R.step_ms);
            STANCHK(product(w, Kx));
        }
        pt.begin();
        STANCHK(stan_newmark_predict_device(ctx, N, c, gF, u, v, a, F, M, damped_K ? Kx : nullptr, b));
        pt.end(&R.predict_ms);
        int32_t term = 0, its = 0;
        pt.begin();
        HIPCHK(ctx, hipMemsetAsync(un, 0, nb, st));
        STANCHK(stan_cg_device(ctx, S, b, P.solve_eps, P.solve_max_its, STAN_PREC_FP64, un, &term, &its, nullptr));
        pt.end(&R.solve_ms);
        R.cg_iterations += its;
        R.cg_min_iterations = std::min(R.cg_min_iterations, its);
        R.cg_max_iterations = std::max(R.cg_max_iterations, its);
        R.cg_worst_type = worse_type(R.cg_worst_type, term);
        if (term == 5 || term == 7 || term == -5 || term == -4) {
            R.failed_step = step;
            return bad("the solve of step " + std::to_string(step) + " ended with termination type " + std::to_string(term), STAN_E_UNSUPPORTED);
        }
        if (d_energy) STANCHK(product(un, Kx));
        pt.begin();
        STANCHK(stan_newmark_correct_device(ctx, N, c, un, u, v, a, M, F, Kx, gF, partial, d_energy ? t_energy + 3 * (size_t)step : nullptr));
        pt.end(&R.correct_ms);
        STANCHK(record(step));
        R.steps = step;
    }

    R.step_ms += R.predict_ms + R.correct_ms;
    // the run succeeded: the outputs leave the driver's tables
    if (t_probe) HIPCHK(ctx, hipMemcpyAsync(d_probe_u, t_probe, n_rows * (size_t)P.n_probe * 8, hipMemcpyDeviceToDevice, st));
    if (t_energy) HIPCHK(ctx, hipMemcpyAsync(d_energy, t_energy, n_rows * 24, hipMemcpyDeviceToDevice, st));
    if (t_snaps) HIPCHK(ctx, hipMemcpyAsync(d_snaps, t_snaps, (size_t)n_snap * 3 * nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_u_end, u, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_v_end, v, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_a_end, a, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return STAN_OK;
}

int shifted_args(stan_ctx *ctx, stan_matrix *K, double sigma, const void *M, stan_matrix **out) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(transient_refused(ctx, "matrix_shifted"));
    if (!K || !M || !out) { ctx->err = "matrix_shifted: null argument"; return STAN_E_ARG; }
    if (K->ctx != ctx) { ctx->err = "matrix_shifted: K belongs to another context"; return STAN_E_ARG; }
    if (!(sigma >= 0) || !std::isfinite(sigma)) { ctx->err = "matrix_shifted: sigma must be >= 0 and finite"; return STAN_E_ARG; }
    return STAN_OK;
}

int shifted_checked(stan_ctx *ctx, stan_matrix *K, double sigma, const double *d_M, stan_matrix **out) {
    int64_t bad_at;
    STANCHK(stan_mass_check_device(ctx, K->n_red, d_M, &bad_at));   // before anything is allocated
    if (bad_at >= 0) { ctx->err = "matrix_shifted: M[" + std::to_string(bad_at) + "] is not positive and finite"; return STAN_E_ARG; }
    stan_matrix *S = nullptr;
    STANCHK(stan_matrix_shifted_device(ctx, K, sigma, d_M, &S));
    *out = S;
    return STAN_OK;
}

int helper_args(stan_ctx *ctx, const char *who, int64_t N, bool null_arg) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(transient_refused(ctx, who));
    if (null_arg || N <= 0) { ctx->err = std::string(who) + ": null argument or N <= 0"; return STAN_E_ARG; }
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_matrix_shifted_dev(stan_ctx *ctx, stan_matrix *K, double sigma, const double *d_M, stan_matrix **out) {
    STANCHK(shifted_args(ctx, K, sigma, d_M, out));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return shifted_checked(ctx, K, sigma, d_M, out);
}

int stan_hip_matrix_shifted(stan_ctx *ctx, stan_matrix *K, double sigma, const double *M, stan_matrix **out) {
    STANCHK(shifted_args(ctx, K, sigma, M, out));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dM;
    STANCHK(dM.upload(st, M, (size_t)K->n_red));
    return st.finish(shifted_checked(ctx, K, sigma, dM.p, out));
}

int stan_hip_transient_dev(stan_ctx *ctx, stan_matrix *K, const double *d_M, const double *d_F, const double *d_u0,
                           const double *d_v0, double dt, int32_t n_steps, double beta_N, double gamma, double alpha_R,
                           double beta_R, int32_t n_curve, const double *curve_t, const double *curve_g, double solve_eps,
                           int32_t solve_max_its, int32_t n_probe, const int32_t *d_probe_dof, double *d_probe_u,
                           int32_t snap_every, double *d_snaps, double *d_energy, double *d_u_end, double *d_v_end,
                           double *d_a_end, void *rep) {
    nm_run P;
    STANCHK(transient_args(ctx, K, d_M, d_F, dt, n_steps, beta_N, gamma, alpha_R, beta_R, n_curve, curve_t, curve_g, solve_eps,
                           solve_max_its, n_probe, d_probe_dof, d_probe_u, snap_every, d_u_end, d_v_end, d_a_end, &P));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return transient_device(ctx, K, d_M, d_F, d_u0, d_v0, P, d_probe_dof, d_probe_u, d_snaps, d_energy, d_u_end, d_v_end, d_a_end,
                            (stan_transient_report *)rep);
}

int stan_hip_transient(stan_ctx *ctx, stan_matrix *K, const double *M, const double *F, const double *u0, const double *v0,
                       double dt, int32_t n_steps, double beta_N, double gamma, double alpha_R, double beta_R, int32_t n_curve,
                       const double *curve_t, const double *curve_g, double solve_eps, int32_t solve_max_its, int32_t n_probe,
                       const int32_t *probe_dof, double *probe_u, int32_t snap_every, double *snaps, double *energy,
                       double *u_end, double *v_end, double *a_end, void *rep) {
    nm_run P;
    STANCHK(transient_args(ctx, K, M, F, dt, n_steps, beta_N, gamma, alpha_R, beta_R, n_curve, curve_t, curve_g, solve_eps,
                           solve_max_its, n_probe, probe_dof, probe_u, snap_every, u_end, v_end, a_end, &P));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)K->n_red, rows = (size_t)n_steps + 1;
    host_stage st(ctx);
    dbuf<double> dM, dF, du0, dv0, dpu, dsn, den, due, dve, dae;
    dbuf<int32_t> dpd;
    STANCHK(dM.upload(st, M, N));
    STANCHK(dF.upload(st, F, N));
    if (u0) STANCHK(du0.upload(st, u0, N));
    if (v0) STANCHK(dv0.upload(st, v0, N));
    if (n_probe > 0) {
        STANCHK(dpd.upload(st, probe_dof, (size_t)n_probe));
        STANCHK(dpu.alloc(st, rows * (size_t)n_probe, probe_u));
    }
    STANCHK(dsn.out(st, snap_every > 0 ? snaps : nullptr, (size_t)snap_count(P, snaps) * 3 * N));
    STANCHK(den.out(st, energy, rows * 3));
    STANCHK(due.alloc(st, N, u_end));
    STANCHK(dve.alloc(st, N, v_end));
    STANCHK(dae.alloc(st, N, a_end));
    const int rc = transient_device(ctx, K, dM.p, dF.p, du0.p, dv0.p, P, dpd.p, dpu.p, dsn.p, den.p, due.p, dve.p, dae.p,
                                    (stan_transient_report *)rep);
    return st.finish(rc, dpu, dsn, den, due, dve, dae);
}

int stan_hip_newmark_predict(stan_ctx *ctx, int64_t N, const double *u, const double *v, const double *a, const double *F,
                             const double *M, const double *Kw, const double *coef, double gF, double *w, double *b) {
    STANCHK(helper_args(ctx, "newmark_predict", N, !u || !v || !a || !F || !M || !coef || !b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    stan_newmark_coef c{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], 1.0 + coef[1] * coef[7], 0.0, 0.0};
    const size_t n = (size_t)N;
    host_stage st(ctx);
    dbuf<double> du, dv, da, dF, dM, dK, dw, db;
    STANCHK(du.upload(st, u, n)); STANCHK(dv.upload(st, v, n)); STANCHK(da.upload(st, a, n));
    STANCHK(dF.upload(st, F, n)); STANCHK(dM.upload(st, M, n));
    if (Kw) STANCHK(dK.upload(st, Kw, n));
    STANCHK(dw.out(st, w, n));
    STANCHK(db.alloc(st, n, b));
    if (w) STANCHK(stan_newmark_w_device(ctx, N, c, du.p, dv.p, da.p, dw.p));
    return st.finish(stan_newmark_predict_device(ctx, N, c, gF, du.p, dv.p, da.p, dF.p, dM.p, dK.p, db.p), dw, db);
}

int stan_hip_newmark_correct(stan_ctx *ctx, int64_t N, const double *u_new, double *u, double *v, double *a, const double *coef,
                             double dt, double gamma, const double *M, const double *F, const double *Ku, double gF,
                             double *energy) {
    STANCHK(helper_args(ctx, "newmark_correct", N, !u_new || !u || !v || !a || !coef || (energy && (!M || !F || !Ku))));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    stan_newmark_coef c{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], 1.0 + coef[1] * coef[7], dt, gamma};
    const size_t n = (size_t)N;
    host_stage st(ctx);
    dbuf<double> dn, du, dv, da, dM, dF, dK, dpart, den;
    STANCHK(dn.upload(st, u_new, n));
    STANCHK(du.upload(st, u, n, u)); STANCHK(dv.upload(st, v, n, v)); STANCHK(da.upload(st, a, n, a));
    if (energy) {
        STANCHK(dM.upload(st, M, n)); STANCHK(dF.upload(st, F, n)); STANCHK(dK.upload(st, Ku, n));
        STANCHK(dpart.alloc(st, 3 * (size_t)stan_newmark_blocks(N)));
        STANCHK(den.alloc(st, 3, energy));
    }
    return st.finish(stan_newmark_correct_device(ctx, N, c, dn.p, du.p, dv.p, da.p, dM.p, dF.p, dK.p, gF, dpart.p, den.p), du, dv, da, den);
}

}  // extern "C"
