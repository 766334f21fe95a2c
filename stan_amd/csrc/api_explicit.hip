// api_explicit.hip -- the extern "C" surface of the explicit dynamics: the driver loop of
// stan_hip_explicit (central-difference steps: one product of K and one vector pass each, explicit.hip), the stable step
// (stan_hip_stable_step: the row bound and the power iteration), the update kernel on host arrays.  The loop keeps every vector
// in the product's padded full numbering (stan_product_full of cg_entries.inc) and enqueues launches only; the load curve is
// evaluated on the host.  One device, one rank (explicit_refused).
#include <algorithm>
#include <cmath>

#include "api_stage.h"

namespace {

struct cd_run {   // what both entries check on the host and hand to the driver
    double dt, alpha_R;
    int32_t n_steps, n_curve, n_probe, snap_every, energy_every, n_power;
    const double *curve_t, *curve_g;
};

double curve_at(const cd_run &P, double x) { return stan_curve_at(P.n_curve, P.curve_t, P.curve_g, x); }

// One device, one rank: the loop's product is a single rank's, the row bound walks one rank's rows, the sums are not reduced
// over ranks
int explicit_refused(stan_ctx *ctx, const char *entry) {
    STAN_NO_GROUP(ctx, std::string(entry) + " (the resident product, the row bound and the step sums run on one device)");
    if (stan_sharded(ctx)) {
        ctx->err = std::string(entry) + ": not available on a context with a communicator (the product and the sums are one rank's)";
        return STAN_E_UNSUPPORTED;
    }
    return STAN_OK;
}

// K whole on this device, with a free DOF: the full numbering is then the DOF numbering (3 * row + m)
int whole_matrix(stan_ctx *ctx, const char *who, const stan_matrix *K) {
    if (K->nhalo != 0 || K->r0 != 0 || K->nloc != K->nb_glob || K->n_dof != 3 * K->nloc) {
        ctx->err = std::string(who) + ": the matrix is a shard of a larger one";
        return STAN_E_UNSUPPORTED;
    }
    if (K->n_red <= 0 || K->nslices <= 0) { ctx->err = std::string(who) + ": the matrix has no free DOF"; return STAN_E_ARG; }
    return STAN_OK;
}
inline int64_t pad3(const stan_matrix *K) { return 3 * (int64_t)K->nslices * 64; }
inline const double *scale_of(const stan_matrix *K) { return K->scaled ? K->d_scale : nullptr; }

// lambda_upper (always) and lambda_power (n_power > 0) of M^-1 K; Mf: the mass in the full numbering.  The power iteration:
// x_0 = the hash column stan_buckling_start_device(N, 1) gives (reduced numbering), then n_power times x <- (K x / M) / sqrt(Kx.Kx / M)
// -- M-norm 1 -- and lambda_power = x.Kx / x.Mx of the last x, the two sums carried as pairs hi + lo: n_power + 1 products.
// Synchronises.
int stable_device(stan_ctx *ctx, stan_matrix *K, const double *Mf, int32_t n_power, double *upper, double *power, double *bound_ms,
                  double *power_ms) {
    const int64_t n = pad3(K), N = K->n_red;
    hipStream_t st = ctx->stream;
    piece_timer pt(ctx);
    pt.begin();
    STANCHK(stan_row_bound_device(ctx, K, Mf, upper));
    pt.end(bound_ms);
    *power = 0.0;
    if (n_power <= 0) return STAN_OK;
    const double *s = scale_of(K);
    dev_scope tmp(ctx);
    double *x0, *x, *xh = nullptr, *y, *partial, *sums;
    int64_t *stt;
    STANCHK(tmp.alloc(&x0, (size_t)N)); STANCHK(tmp.alloc(&x, (size_t)n)); STANCHK(tmp.alloc(&y, (size_t)n));
    if (s) STANCHK(tmp.alloc(&xh, (size_t)n));
    STANCHK(tmp.alloc(&partial, 5 * (size_t)stan_cd_blocks(n))); STANCHK(tmp.alloc(&sums, 5));
    STANCHK(stan_product_status(ctx, tmp, &stt));
    pt.begin();
    HIPCHK(ctx, hipMemsetAsync(y, 0, (size_t)n * 8, st));   // the product leaves the padding alone
    STANCHK(stan_buckling_start_device(ctx, N, 1, x0));
    STANCHK(stan_cd_expand_device(ctx, K->n_dof, n, K->d_red, x0, nullptr, 0.0, x));
    if (s) STANCHK(stan_cd_expand_device(ctx, K->n_dof, n, K->d_red, x0, s, 0.0, xh));
    for (int32_t it = 0; it <= n_power; it++) {
        STANCHK(stan_product_full(ctx, K, s ? xh : x, y, stt));
        STANCHK(stan_power_sums_device(ctx, n, y, s, x, Mf, partial, sums));
        if (it < n_power) STANCHK(stan_power_next_device(ctx, n, y, s, Mf, sums, x, xh));
    }
    double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    HIPCHK(ctx, hipMemcpyAsync(h, sums, 40, hipMemcpyDeviceToHost, st));
    pt.end(power_ms);
    HIPCHK(ctx, hipStreamSynchronize(st));
    *power = (double)(((long double)h[0] + h[1]) / ((long double)h[2] + h[3]));   // the pairs hi + lo, rounded once
    return STAN_OK;
}

// the host checks of both entries; fills P
int explicit_args(stan_ctx *ctx, stan_matrix *K, const void *M, const void *F, double dt, int32_t n_steps, double alpha_R,
                  int32_t n_curve, const double *curve_t, const double *curve_g, int32_t n_probe, const void *probe_dof,
                  const void *probe_u, int32_t snap_every, int32_t energy_every, const void *energy, const void *u_end,
                  const void *v_end, const void *a_end, int32_t n_power, cd_run *P) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(explicit_refused(ctx, "explicit"));
    auto bad = [&](const char *why) { ctx->err = std::string("explicit: ") + why; return STAN_E_ARG; };
    if (!K || !M || !F || !u_end || !v_end || !a_end) return bad("null argument");
    if (K->ctx != ctx) return bad("K belongs to another context");
    if (!(dt > 0) || !std::isfinite(dt)) return bad("dt must be positive and finite");
    if (n_steps < 0 || n_curve < 0 || n_probe < 0 || snap_every < 0 || energy_every < 0 || n_power < 0)
        return bad("n_steps, n_curve, n_probe, snap_every, energy_every and n_power must be >= 0");
    if (!(alpha_R >= 0) || !std::isfinite(alpha_R)) return bad("alpha_R must be >= 0");
    if (n_curve > 0 && (!curve_t || !curve_g)) return bad("null load curve");
    for (int i = 0; i < n_curve; i++) {
        if (!std::isfinite(curve_t[i]) || !std::isfinite(curve_g[i])) return bad("a load curve value is not finite");
        if (i > 0 && curve_t[i] < curve_t[i - 1]) return bad("the load curve's t must not descend");
    }
    if (n_probe > 0 && (!probe_dof || !probe_u)) return bad("null probe argument");
    if (energy_every > 0 && !energy) return bad("null energy argument");
    if ((int64_t)n_probe * ((int64_t)n_steps + 1) > ((int64_t)1 << 40)) return bad("probe table too large");
    *P = cd_run{dt, alpha_R, n_steps, n_curve, n_probe, snap_every, energy_every, n_power, curve_t, curve_g};
    return STAN_OK;
}

int64_t snap_count(const cd_run &P, const double *snaps) { return snaps && P.snap_every > 0 ? P.n_steps / P.snap_every + 1 : 0; }
int64_t energy_count(const cd_run &P) { return P.energy_every > 0 ? P.n_steps / P.energy_every + 1 : 0; }

// The driver on device arrays.  The inputs are expanded once into vectors of the driver's own in the padded full numbering (fixed
// DOFs and padding: u = 0, F = 0, M = 1), the outputs are compressed into tables of its own where a step records them and copied
// out at the end of a run that succeeded: an error leaves the caller's outputs untouched.
int explicit_device(stan_ctx *ctx, stan_matrix *K, const double *d_Min, const double *d_Fin, const double *d_u0, const double *d_v0,
                    const cd_run &P, const int32_t *d_probe, double *d_probe_u, double *d_snaps, double *d_energy, double *d_u_end,
                    double *d_v_end, double *d_a_end, stan_explicit_report *rep) {
    auto bad = [&](const std::string &why, int rc) { ctx->err = "explicit: " + why; return rc; };
    stan_explicit_report R{};
    report_out<stan_explicit_report> report{rep, R};   // first: written on every way out behind the argument checks
    STANCHK(whole_matrix(ctx, "explicit", K));
    const int64_t N = K->n_red, n = pad3(K), n_dof = K->n_dof;
    const size_t nb = (size_t)N * 8;
    const stan_cd_coef c = stan_cd_make_coef(P.dt, P.alpha_R);
    if (!(c.dt2 > 0) || !(c.op > 0) || !std::isfinite(c.op)) return bad("dt is too small or alpha_R dt too large: dt^2 or 1 + alpha_R dt / 2 is not positive and finite", STAN_E_ARG);
    piece_timer pt(ctx);
    hipStream_t st = ctx->stream;

    int64_t bad_at;
    STANCHK(stan_mass_check_device(ctx, N, d_Min, &bad_at));
    if (bad_at >= 0) return bad("M[" + std::to_string(bad_at) + "] is not positive and finite", STAN_E_ARG);
    STANCHK(stan_newmark_probe_check_device(ctx, N, P.n_probe, d_probe, &bad_at));
    if (bad_at >= 0) return bad("probe_dof[" + std::to_string(bad_at) + "] is outside [0, N)", STAN_E_ARG);

    const double *s = scale_of(K);
    const int64_t n_snap = snap_count(P, d_snaps), n_en = energy_count(P);
    const size_t n_rows = (size_t)P.n_steps + 1;
    dev_scope tmp(ctx);
    double *M, *F, *un, *up, *y, *v, *a, *xh = nullptr, *t_probe = nullptr, *t_energy = nullptr, *partial = nullptr, *t_snaps = nullptr, *t_end;
    int32_t *full_of = nullptr;
    int64_t *stt;
    long long *flag;
    STANCHK(tmp.alloc(&M, (size_t)n)); STANCHK(tmp.alloc(&F, (size_t)n));
    STANCHK(tmp.alloc(&un, (size_t)n)); STANCHK(tmp.alloc(&up, (size_t)n)); STANCHK(tmp.alloc(&y, (size_t)n));
    STANCHK(tmp.alloc(&v, (size_t)n)); STANCHK(tmp.alloc(&a, (size_t)n));
    if (s) STANCHK(tmp.alloc(&xh, (size_t)n));
    STANCHK(tmp.alloc(&t_end, 3 * (size_t)N));
    STANCHK(tmp.alloc(&flag, 1));
    if (P.n_probe > 0) {
        STANCHK(tmp.alloc(&t_probe, n_rows * (size_t)P.n_probe));
        STANCHK(tmp.alloc(&full_of, (size_t)N));
    }
    if (n_en > 0) {
        STANCHK(tmp.alloc(&t_energy, (size_t)n_en * 3));
        STANCHK(tmp.alloc(&partial, 3 * (size_t)stan_cd_blocks(n)));
    }
    if (n_snap > 0) STANCHK(tmp.alloc(&t_snaps, (size_t)n_snap * 3 * (size_t)N));
    STANCHK(stan_product_status(ctx, tmp, &stt));
    STANCHK(stan_cd_expand_device(ctx, n_dof, n, K->d_red, d_Min, nullptr, 1.0, M));
    STANCHK(stan_cd_expand_device(ctx, n_dof, n, K->d_red, d_Fin, nullptr, 0.0, F));
    STANCHK(stan_cd_expand_device(ctx, n_dof, n, K->d_red, d_u0, nullptr, 0.0, un));
    STANCHK(stan_cd_expand_device(ctx, n_dof, n, K->d_red, d_v0, nullptr, 0.0, v));
    if (s) STANCHK(stan_cd_expand_device(ctx, n_dof, n, K->d_red, d_u0, s, 0.0, xh));
    if (full_of) STANCHK(stan_cd_index_device(ctx, n_dof, K->d_red, full_of));
    HIPCHK(ctx, hipMemsetAsync(y, 0, (size_t)n * 8, st));   // the product leaves the padding alone; K u0 = 0 without a u0
    const long long none = 0x7fffffffffffffffLL;
    HIPCHK(ctx, hipMemcpyAsync(flag, &none, 8, hipMemcpyHostToDevice, st));

    // the stable step: what the matrix itself says about dt
    STANCHK(stable_device(ctx, K, M, P.n_power, &R.lambda_upper, &R.lambda_power, &R.bound_ms, &R.power_ms));
    R.dt_stable = 2.0 / std::sqrt(R.lambda_upper);
    if (P.n_power > 0 && P.dt > 2.0 / std::sqrt(R.lambda_power)) {
        char buf[256];
        snprintf(buf, sizeof buf, "dt = %.17g is unstable: it exceeds 2 / sqrt(lambda_power) = %.17g, and lambda_power = %.17g is a lower bound of lambda_max",
                 P.dt, 2.0 / std::sqrt(R.lambda_power), R.lambda_power);
        return bad(buf, STAN_E_ARG);
    }

    auto product = [&]() -> int {
        pt.begin();
        STANCHK(stan_product_full(ctx, K, s ? xh : un, y, stt));
        pt.end(&R.product_ms);
        return STAN_OK;
    };
    auto flag_check = [&]() -> int {   // synchronises
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_status + SS_AUX, flag, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (ctx->h_status[SS_AUX] == none) return STAN_OK;
        R.first_nonfinite_step = (int32_t)std::min<int64_t>(ctx->h_status[SS_AUX], INT32_MAX);
        return bad("u of step " + std::to_string(ctx->h_status[SS_AUX]) + " has an entry that is not finite", STAN_E_UNSUPPORTED);
    };

    // the start: a_0 from the equation of motion at t = 0 and u_{-1}; y = K u0 serves step 0 too
    if (d_u0) STANCHK(product());
    pt.begin();
    STANCHK(stan_cd_start_device(ctx, n, c, curve_at(P, 0.0), y, s, un, v, M, F, a, up));
    pt.end(&R.update_ms);

    // step n: u_{n+1} from u_n, u_{n-1} and K u_n, which closes v_n and a_n: one update more than n_steps
    for (int32_t step = 0; step <= P.n_steps; step++) {
        const double gF = curve_at(P, (double)step * P.dt);
        if (step > 0) STANCHK(product());
        if (t_probe) STANCHK(stan_cd_probe_device(ctx, P.n_probe, d_probe, full_of, un, t_probe + (size_t)step * (size_t)P.n_probe));
        const bool snap = n_snap > 0 && step % P.snap_every == 0, last = step == P.n_steps;
        const bool state = step > 0 && (snap || last);   // step 0 keeps v0 and the start's a_0
        double *en = n_en > 0 && step % P.energy_every == 0 ? t_energy + 3 * (size_t)(step / P.energy_every) : nullptr;
        pt.begin();
        STANCHK(stan_cd_update_device(ctx, n, c, gF, (long long)step + 1, y, s, un, up, M, F, xh, state ? v : nullptr, state ? a : nullptr,
                                      partial, en, flag));
        pt.end(&R.update_ms);
        R.steps = step;
        if (snap || last) {
            double *row = last ? t_end : t_snaps + (size_t)(step / P.snap_every) * 3 * (size_t)N;
            STANCHK(stan_cd_compress_device(ctx, n_dof, K->d_red, un, row));
            STANCHK(stan_cd_compress_device(ctx, n_dof, K->d_red, v, row + N));
            STANCHK(stan_cd_compress_device(ctx, n_dof, K->d_red, a, row + 2 * N));
            if (snap && last) HIPCHK(ctx, hipMemcpyAsync(t_snaps + (size_t)(step / P.snap_every) * 3 * (size_t)N, t_end, 3 * nb, hipMemcpyDeviceToDevice, st));
            STANCHK(flag_check());
        }
        std::swap(un, up);   // up now holds u_n, un holds u_{n+1}
    }

    // the run succeeded: the outputs leave the driver's tables
    if (t_probe) HIPCHK(ctx, hipMemcpyAsync(d_probe_u, t_probe, n_rows * (size_t)P.n_probe * 8, hipMemcpyDeviceToDevice, st));
    if (t_energy) HIPCHK(ctx, hipMemcpyAsync(d_energy, t_energy, (size_t)n_en * 24, hipMemcpyDeviceToDevice, st));
    if (t_snaps) HIPCHK(ctx, hipMemcpyAsync(d_snaps, t_snaps, (size_t)n_snap * 3 * nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_u_end, t_end, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_v_end, t_end + N, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_a_end, t_end + 2 * N, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return STAN_OK;
}

int stable_args(stan_ctx *ctx, stan_matrix *K, const void *M, int32_t n_power, const void *lu, const void *lp, const void *dts) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(explicit_refused(ctx, "stable_step"));
    if (!K || !M || !lu || !lp || !dts) { ctx->err = "stable_step: null argument"; return STAN_E_ARG; }
    if (K->ctx != ctx) { ctx->err = "stable_step: K belongs to another context"; return STAN_E_ARG; }
    if (n_power < 0) { ctx->err = "stable_step: n_power must be >= 0"; return STAN_E_ARG; }
    return STAN_OK;
}

int stable_checked(stan_ctx *ctx, stan_matrix *K, const double *d_M, int32_t n_power, double *upper, double *power, double *dt_stable) {
    STANCHK(whole_matrix(ctx, "stable_step", K));
    int64_t bad_at;
    STANCHK(stan_mass_check_device(ctx, K->n_red, d_M, &bad_at));
    if (bad_at >= 0) { ctx->err = "stable_step: M[" + std::to_string(bad_at) + "] is not positive and finite"; return STAN_E_ARG; }
    dev_scope tmp(ctx);
    double *Mf, lu = 0, lp = 0, ms[2] = {0, 0};
    STANCHK(tmp.alloc(&Mf, (size_t)pad3(K)));
    STANCHK(stan_cd_expand_device(ctx, K->n_dof, pad3(K), K->d_red, d_M, nullptr, 1.0, Mf));
    STANCHK(stable_device(ctx, K, Mf, n_power, &lu, &lp, &ms[0], &ms[1]));
    *upper = lu; *power = lp; *dt_stable = 2.0 / std::sqrt(lu);
    return STAN_OK;
}

}  // namespace

extern "C" {

int stan_hip_stable_step_dev(stan_ctx *ctx, stan_matrix *K, const double *d_M, int32_t n_power, double *lambda_upper,
                             double *lambda_power, double *dt_stable) {
    STANCHK(stable_args(ctx, K, d_M, n_power, lambda_upper, lambda_power, dt_stable));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return stable_checked(ctx, K, d_M, n_power, lambda_upper, lambda_power, dt_stable);
}

int stan_hip_stable_step(stan_ctx *ctx, stan_matrix *K, const double *M, int32_t n_power, double *lambda_upper, double *lambda_power,
                         double *dt_stable) {
    STANCHK(stable_args(ctx, K, M, n_power, lambda_upper, lambda_power, dt_stable));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    host_stage st(ctx);
    dbuf<double> dM;
    STANCHK(dM.upload(st, M, (size_t)K->n_red));
    return st.finish(stable_checked(ctx, K, dM.p, n_power, lambda_upper, lambda_power, dt_stable));
}

int stan_hip_explicit_dev(stan_ctx *ctx, stan_matrix *K, const double *d_M, const double *d_F, const double *d_u0, const double *d_v0,
                          double dt, int32_t n_steps, double alpha_R, int32_t n_curve, const double *curve_t, const double *curve_g,
                          int32_t n_probe, const int32_t *d_probe_dof, double *d_probe_u, int32_t snap_every, double *d_snaps,
                          int32_t energy_every, double *d_energy, double *d_u_end, double *d_v_end, double *d_a_end, int32_t n_power,
                          void *rep) {
    cd_run P;
    STANCHK(explicit_args(ctx, K, d_M, d_F, dt, n_steps, alpha_R, n_curve, curve_t, curve_g, n_probe, d_probe_dof, d_probe_u, snap_every,
                          energy_every, d_energy, d_u_end, d_v_end, d_a_end, n_power, &P));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return explicit_device(ctx, K, d_M, d_F, d_u0, d_v0, P, d_probe_dof, d_probe_u, d_snaps, d_energy, d_u_end, d_v_end, d_a_end,
                           (stan_explicit_report *)rep);
}

int stan_hip_explicit(stan_ctx *ctx, stan_matrix *K, const double *M, const double *F, const double *u0, const double *v0, double dt,
                      int32_t n_steps, double alpha_R, int32_t n_curve, const double *curve_t, const double *curve_g, int32_t n_probe,
                      const int32_t *probe_dof, double *probe_u, int32_t snap_every, double *snaps, int32_t energy_every, double *energy,
                      double *u_end, double *v_end, double *a_end, int32_t n_power, void *rep) {
    cd_run P;
    STANCHK(explicit_args(ctx, K, M, F, dt, n_steps, alpha_R, n_curve, curve_t, curve_g, n_probe, probe_dof, probe_u, snap_every,
                          energy_every, energy, u_end, v_end, a_end, n_power, &P));
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
    STANCHK(den.out(st, energy_every > 0 ? energy : nullptr, (size_t)energy_count(P) * 3));
    STANCHK(due.alloc(st, N, u_end));
    STANCHK(dve.alloc(st, N, v_end));
    STANCHK(dae.alloc(st, N, a_end));
    const int rc = explicit_device(ctx, K, dM.p, dF.p, du0.p, dv0.p, P, dpd.p, dpu.p, dsn.p, den.p, due.p, dve.p, dae.p,
                                   (stan_explicit_report *)rep);
    return st.finish(rc, dpu, dsn, den, due, dve, dae);
}

int stan_hip_central_update(stan_ctx *ctx, int64_t N, const double *y, const double *s, const double *u, const double *u_prev,
                            const double *M, const double *F, double dt, double alpha_R, double gF, int64_t step, double *u_next,
                            double *u_next_scaled, double *v, double *a, double *energy, int64_t *first_nonfinite) {
    if (!ctx) return STAN_E_ARG;
    STANCHK(explicit_refused(ctx, "central_update"));
    if (!y || !u || !u_prev || !M || !F || !u_next || (s && !u_next_scaled) || !v != !a || N <= 0) {
        ctx->err = "central_update: null argument, v without a, or N <= 0";
        return STAN_E_ARG;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)N;
    const long long none = 0x7fffffffffffffffLL;
    long long found = none;
    host_stage st(ctx);
    dbuf<double> dy, ds, du, dp, dM, dF, dxh, dv, da, dpart, den;
    dbuf<long long> dflag;
    STANCHK(dy.upload(st, y, n));
    if (s) { STANCHK(ds.upload(st, s, n)); STANCHK(dxh.alloc(st, n, u_next_scaled)); }
    STANCHK(du.upload(st, u, n)); STANCHK(dp.upload(st, u_prev, n, u_next));
    STANCHK(dM.upload(st, M, n)); STANCHK(dF.upload(st, F, n));
    STANCHK(dv.out(st, v, n)); STANCHK(da.out(st, a, n));
    if (energy) {
        STANCHK(dpart.alloc(st, 3 * (size_t)stan_cd_blocks(N)));
        STANCHK(den.alloc(st, 3, energy));
    }
    STANCHK(dflag.upload(st, &none, 1, &found));
    const int rc = st.finish(stan_cd_update_device(ctx, N, stan_cd_make_coef(dt, alpha_R), gF, (long long)step, dy.p, ds.p, du.p, dp.p, dM.p,
                                                   dF.p, dxh.p, dv.p, da.p, dpart.p, den.p, dflag.p),
                             dp, dxh, dv, da, den, dflag);
    if (rc == STAN_OK && first_nonfinite) *first_nonfinite = found == none ? 0 : (int64_t)found;
    return rc;
}

}  // extern "C"
