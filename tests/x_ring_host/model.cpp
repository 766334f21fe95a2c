// The slot and window arithmetic of the ring of search directions (stan_amd/csrc/x_ring.h, STAN_OPT_CG_X_RING) checked on
// the host: a scalar model of the CG loop's bookkeeping -- one double stands for a vector -- run with x formed every
// iteration and with x formed from the ring, for every stop iteration, every window and both kinds of stop.  Built with
// -fsanitize=address,undefined by tests/test_x_ring_host.py; nothing of it is loaded into Python.
//
// What the model keeps of the loop (cg.hip: cg_run::iterate, cg_vector_kernels.inc): the host enqueues iterations ahead of
// the device and knows nothing of a stop; every kernel of iteration k looks at the status words first (ITER_A, ITER_B) and
// returns at once when the solve has stopped; k_step stops with the previous iterate (ITER_B = k, x_{k-1}), k_update with
// this one (ITER_A = k, x_k); the ring's slots are REALLY overwritten, so a term summed after its slot was reused shows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>

#include "../../stan_amd/csrc/x_ring.h"

namespace {

constexpr int64_t NEVER = INT64_MAX;
enum stop_kind { IN_UPDATE = 0, IN_STEP = 1 };

struct status {
    int64_t iter_a = NEVER, iter_b = NEVER, type = 0, iters = 0, xsel = 0, flushed = 0;
};
bool stopped(const status &t, int64_t k) { return t.iter_a < k || t.iter_b < k; }

// the numbers of iteration j: any doubles will do, as long as the order of the sums matters
double alpha_of(int64_t j) { return 1.0 / 3.0 + 1e-3 * (double)(j * 7919 % 101); }
double p_of(int64_t j) { return std::ldexp(1.0 + (double)(j * 104729 % 1009) / 1009.0, (int)(j % 40) - 20) * ((j & 1) ? -1.0 : 1.0); }

uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

// x formed every iteration, in the buffer k & 1 (k_update with xnext); returns the iterate the status names
double run_plain(int64_t stop_at, stop_kind kind, int64_t enqueued, status *out) {
    double xb[2] = {0.0, 0.0};
    status t;
    for (int64_t k = 1; k <= enqueued; k++) {
        // k_step
        if (!stopped(t, k) && k == stop_at && kind == IN_STEP) { t.type = -5; t.iters = k; t.xsel = (k - 1) & 1; t.iter_b = k; }
        // k_update
        if (t.iter_a < k || t.iter_b <= k) continue;
        xb[k & 1] = std::fma(alpha_of(k), p_of(k), xb[(k - 1) & 1]);
        if (k == stop_at && kind == IN_UPDATE) { t.type = 1; t.iters = k; t.xsel = k & 1; t.iter_a = k; }
    }
    *out = t;
    if (t.type == 0) return xb[enqueued & 1];   // the hard cap
    return xb[t.xsel & 1];
}

struct ring_model {
    int W;
    std::vector<double> p, alpha;   // W + 1 slots
    double x = 0.0;
    status t;
    int64_t flushed_host = 0, flushes = 0;
    int errors = 0;
    explicit ring_model(int w) : W(w), p((size_t)w + 1, NAN), alpha((size_t)w + 1, NAN) {}

    // k_xring_flush: k > 0 in front of iteration k (terms from the host), k == 0 the closing one (terms from the status)
    void flush(int64_t k, int64_t first, int64_t last, int64_t last_enqueued) {
        flushes++;
        if (k > 0) {
            if (stopped(t, k)) return;
        } else {
            first = t.flushed + 1;
            last = xring_final_iterate(t.type, t.iters, t.xsel, last_enqueued);
        }
        const int64_t n = last - first + 1;
        if (n <= 0) return;
        if (n > XRING_MAX_W || n > W) { errors++; return; }
        for (int64_t j = first; j <= last; j++) {
            const int s = xring_slot(j, W);
            if (s < 0 || s > W) { errors++; return; }
            x = std::fma(alpha[(size_t)s], p[(size_t)s], x);
        }
        if (k > 0) t.flushed = last;
    }

    double run(int64_t stop_at, stop_kind kind, int64_t enqueued, int64_t rupdate, const std::vector<double> &x_ref) {
        p[(size_t)xring_slot(1, W)] = p_of(1);   // k_init
        for (int64_t k = 1; k <= enqueued; k++) {
            const bool refresh = rupdate > 0 && k % rupdate == 0;
            if (xring_flush_due(k, flushed_host, W, refresh)) {
                flush(k, flushed_host + 1, k - 1, 0);
                flushed_host = k - 1;
            }
            // the product of a refresh iteration multiplies x_{k-1}
            if (refresh && !stopped(t, k) && bits(x) != bits(x_ref[(size_t)(k - 1)])) errors++;
            // the product reads p_k from its slot
            if (!stopped(t, k) && bits(p[(size_t)xring_slot(k, W)]) != bits(p_of(k))) errors++;
            // k_step
            if (!stopped(t, k) && k == stop_at && kind == IN_STEP) { t.type = -5; t.iters = k; t.xsel = (k - 1) & 1; t.iter_b = k; }
            // k_update
            if (t.iter_a < k || t.iter_b <= k) continue;
            alpha[(size_t)xring_slot(k, W)] = alpha_of(k);
            if (k == stop_at && kind == IN_UPDATE) { t.type = 1; t.iters = k; t.xsel = k & 1; t.iter_a = k; continue; }
            p[(size_t)xring_slot(k + 1, W)] = p_of(k + 1);
        }
        flush(0, 0, 0, enqueued);
        return x;
    }
};

}  // namespace

int main() {
    long cases = 0, bad = 0;
    // the refresh periods: every window 2 ... 16 as its own period, no refresh, and periods beyond the longest window (W = 10)
    std::vector<int64_t> periods;
    for (int64_t r = 2; r <= XRING_MAX_W; r++) periods.push_back(r);
    for (int64_t r : {0, 17, 20, 21, 22, 33}) periods.push_back(r);
    for (int64_t rupdate : periods) {
        const int W = xring_window(rupdate);
        if (W < 2 || W > XRING_MAX_W || (rupdate >= 2 && rupdate <= XRING_MAX_W && W != rupdate)) { std::printf("bad window %d for period %ld\n", W, (long)rupdate); return 1; }
        const int64_t last_stop = 3 * W + 2;
        for (int kind = 0; kind < 2; kind++)
            for (int64_t stop_at = 1; stop_at <= last_stop + 1; stop_at++)      // last_stop + 1: no stop, the hard cap ends the loop
                for (int64_t ahead : {(int64_t)0, (int64_t)1, (int64_t)W, (int64_t)64}) {   // the host's run-ahead behind the stop
                    const bool capped = stop_at > last_stop;
                    const int64_t enqueued = capped ? last_stop : stop_at + ahead;
                    // the iterates x_0 ... of the plain recurrence: what a refresh product must find
                    std::vector<double> x_ref((size_t)enqueued + 1, 0.0);
                    for (int64_t j = 1; j <= enqueued; j++) x_ref[(size_t)j] = std::fma(alpha_of(j), p_of(j), x_ref[(size_t)(j - 1)]);
                    status tp;
                    const double xp = run_plain(stop_at, (stop_kind)kind, enqueued, &tp);
                    ring_model R(W);
                    const double xr = R.run(stop_at, (stop_kind)kind, enqueued, rupdate, x_ref);
                    cases++;
                    const bool same_status = tp.type == R.t.type && tp.iters == R.t.iters && tp.xsel == R.t.xsel;
                    if (bits(xp) != bits(xr) || R.errors || !same_status) {
                        if (bad++ < 10)
                            std::printf("differs: period %ld W %d kind %d stop %ld enqueued %ld: plain %a ring %a errors %d\n", (long)rupdate, W,
                                        kind, (long)stop_at, (long)enqueued, xp, xr, R.errors);
                    }
                }
    }
    if (bad) { std::printf("FAILED %ld of %ld cases\n", bad, cases); return 1; }
    std::printf("ok %ld cases\n", cases);
    return 0;
}
