// main_solver.cpp -- native console driver: `stan_solver <model.STdb>`.
// Reproduces Solver.Main / SolverLinearStatics / ExportOutput (Solver.cs:18-217, 454-462)
// on top of the two C-ABI libraries: read STdb -> materials -> AssignDOF -> BC tables ->
// assemble on the GPU -> CG on the GPU -> displacements -> stress recovery on the GPU ->
// overwrite the input file with the results (Result_StepNo = 1).
// Differences kept on purpose: no console-window sizing in the banner
// (SolverFunctions.cs:18-20 throws when stdout is redirected) and no 10 s sleep at exit
// (Solver.cs:67-68).  LinSolver "Cholesky"/"LU" (SolverFunctions.cs:332-516) are outside the GPU
// hot path: K is exported as the upper CRS the reference holds and solved on the CPU (direct.cpp).
//
// In the order of a run: CliOptions (all that argv sets: ParseArgs, then Refusal before anything is read -- a run that gets further
// overwrites its input), Prepared (what every analysis starts from: ReadModel, BuildTables, Assemble, BuildLoads), RunModes /
// RunTransient / RunExplicit / RunHarmonic / RunBuckling / RunStatics, main().  The extra switches (never stored in the STdb) are described where they are carried out.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stan_hip.h"
#include "../../include/stan_host.h"
#include "model.h"
#include "solver_functions.h"

using namespace stan;
using clk = std::chrono::steady_clock;
static double secs(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

static int fail(const char *what, const std::string &msg) {
    fprintf(stderr, "\n  ERROR in %s: %s\n", what, msg.c_str());
    return 1;
}

// a run that is refused: before anything is computed or written
static int refuse(const std::string &why) {
    fprintf(stderr, "stan_solver: %s\n", why.c_str());
    return 2;
}

static const char *const kUsage =
    "usage: stan_solver [--device N | --gpus N | --devices a,b,..] [--p2p] [--mixed|--fixed48] "
    "[--no-merit-stop] [--packed] [--object-results] [--json] [--vtu PREFIX [--vtu-results \"name,..\"] [--vtu-cells]] [--reactions] [--modes K [--modes-tol T] [--modes-shift SIGMA] [--mass lumped|consistent]] "
    "[--buckling K [--buckling-tol T] [--solve-eps E] [--vtu PREFIX]] "
    "[--transient --dt DT --steps N [--newmark B,G] [--rayleigh A,B] [--load-curve t0,g0,t1,g1,...] [--probe-node ID] "
    "[--solve-eps E] [--vtu PREFIX [--vtu-every K]]] <model.STdb>\n";

// what --help prints behind kUsage (kUsage itself is pinned text: tests/golden/console_refusals.json)
static const char *const kExplicitUsage =
    "       stan_solver --explicit --steps N [--dt DT | --dt auto] [--dt-scale S] [--rayleigh A,0] [--load-curve t0,g0,t1,g1,...] "
    "[--probe-node ID] [--json] [--vtu PREFIX [--vtu-every K]] <model.STdb>\n"
    "         --dt auto     dt = S * 2 / sqrt(lambda_upper), lambda_upper the Gershgorin row bound of M^-1 K: stable by proof\n"
    "         --dt-scale S  default 0.9: the usual convention of explicit codes, not a measured value\n";

static const char *const kHarmonicUsage =
    "       stan_solver --harmonic F0,F1,NF --modes K [--mass consistent] [--modes-tol T] [--rayleigh A,B] [--modal-damping Z] "
    "[--probe-node ID] [--json] [--vtu PREFIX [--vtu-every E]] <model.STdb>\n"
    "         --harmonic F0,F1,NF  the steady-state response to the file's loads times e^{i w t} at NF frequencies, linearly spaced\n"
    "                              from F0 to F1 in Hz (NF = 1: F0), by superposition of the K lowest modes with a static correction\n"
    "         --modal-damping Z    the damping ratio of every mode, on top of --rayleigh A,B\n";

// ---- options ------------------------------------------------------------------------------------------------------------------
// --device N, --gpus N (devices 0..N-1) or --devices a,b,c (several GPUs from this ONE process: stan_hip_init_multi, rows of K
// sharded, RCCL inside the CG), --mixed, --fixed48, --no-merit-stop, --packed, --placement-tries N (default 16; 1 = plain
// allocation), --p2p (several GPUs: the CG exchanges peer to peer instead of over RCCL, STAN_OPT_COMM_P2P), --object-results
// (store the results in the Node / Element objects before the export, as the reference does, instead of encoding them from the
// flat arrays: same bytes), --json (one JSON line with sizes, iterations, device and host phase times and the SpMV's HBM rate);
// --vtu, --reactions: RunStatics; --modes, --modes-shift, --mass: RunModes; --buckling: RunBuckling; --transient: RunTransient;
// --explicit (with --dt auto, --dt-scale): RunExplicit; --harmonic (with --modal-damping): RunHarmonic; --help: the usage lines.
struct CliOptions {
    std::string path;
    int device = 0, precision = STAN_PREC_FP64, placement_tries = 16;
    bool merit_stop = true, packed = false, json = false, object_results = false, p2p = false;
    std::vector<int> devices;
    bool vtu = false, vtu_cells = false, reactions = false;
    std::string vtu_prefix, vtu_results, vtu_results_why;   // (why: what ParseScalarNames has against vtu_results)
    std::vector<int32_t> vtu_sel;
    int modes = 0;
    double modes_tol = 0.0, modes_shift = 0.0;
    std::string mass_kind = "lumped";
    int buckling = 0;
    double buckling_tol = 0.0, solve_eps = 0.0;
    bool buckling_arg = false, have_solve_eps = false;
    bool transient = false, transient_arg = false, bad_list = false;
    SolverFunctions::TransientRun run;
    int probe_node = 0, vtu_every = 1;
    bool have_probe = false;
    bool explicit_run = false, explicit_arg = false, dt_auto = false, help = false;   // --explicit; --dt auto / --dt-scale seen
    double dt_scale = 0.9;
    bool harmonic = false, harmonic_bad = false, have_modal_damping = false, time_arg = false;   // --harmonic; an option of the time integrators seen
    double f0 = 0, f1 = 0, n_freq = 0, modal_damping = -1;                                        // (n_freq as given: checked in Refusal)
    bool several_devices() const { return devices.size() > 1; }
};

// "a,b,c" -> doubles; false when an item is not a number
static bool NumberList(const char *text, std::vector<double> *out) {
    out->clear();
    for (const char *p = text; *p;) {
        char *end = nullptr;
        const double x = strtod(p, &end);
        if (end == p) return false;
        out->push_back(x);
        p = end;
        if (*p == ',') p++;
        else if (*p) return false;
    }
    return true;
}

// argv -> options.  A word that is no switch is the path, the last one wins; so is a switch that wants a value and stands last.
static CliOptions ParseArgs(int argc, char **argv) {
    CliOptions o;
    SolverFunctions::TransientRun &run = o.run;
    std::vector<double> list;
    for (int i = 1; i < argc; i++) {
        auto flag = [&](const char *name) { return !strcmp(argv[i], name); };
        auto value = [&](const char *name) { return flag(name) && i + 1 < argc; };
        // the value as `list`: `count` numbers, or (0) pairs of them; else bad_list
        auto numbers = [&](size_t count) {
            o.transient_arg = true;
            const bool ok = NumberList(argv[++i], &list) && (count ? list.size() == count : !list.empty() && list.size() % 2 == 0);
            if (!ok) o.bad_list = true;
            return ok;
        };
        if (value("--device")) o.device = atoi(argv[++i]);
        else if (value("--gpus")) {
            o.devices.clear();
            for (int d = 0, n = atoi(argv[++i]); d < n; d++) o.devices.push_back(d);
        } else if (value("--devices")) {
            o.devices.clear();
            for (const char *p = argv[++i]; *p;) {
                o.devices.push_back(atoi(p));
                while (*p && *p != ',') p++;
                if (*p == ',') p++;
            }
        }
        else if (value("--placement-tries")) o.placement_tries = atoi(argv[++i]);
        else if (flag("--mixed")) o.precision = STAN_PREC_MIXED;
        else if (flag("--fixed48")) o.precision = STAN_PREC_FIXED48;
        else if (flag("--no-merit-stop")) o.merit_stop = false;
        else if (flag("--packed")) o.packed = true;
        else if (flag("--json")) o.json = true;
        else if (flag("--object-results")) o.object_results = true;
        else if (flag("--p2p")) o.p2p = true;
        else if (value("--vtu")) { o.vtu = true; o.vtu_prefix = argv[++i]; }
        else if (value("--vtu-results")) o.vtu_results = argv[++i];
        else if (flag("--vtu-cells")) o.vtu_cells = true;
        else if (flag("--reactions")) o.reactions = true;
        else if (value("--modes")) o.modes = atoi(argv[++i]);
        else if (value("--modes-tol")) o.modes_tol = atof(argv[++i]);
        else if (value("--modes-shift")) o.modes_shift = atof(argv[++i]);
        else if (value("--mass")) o.mass_kind = argv[++i];
        else if (flag("--transient")) o.transient = true;
        else if (flag("--help")) o.help = true;
        else if (flag("--explicit")) o.explicit_run = true;
        else if (value("--harmonic")) {
            o.harmonic = true;
            if (NumberList(argv[++i], &list) && list.size() == 3) { o.f0 = list[0]; o.f1 = list[1]; o.n_freq = list[2]; }
            else o.harmonic_bad = true;
        }
        else if (value("--modal-damping")) { o.have_modal_damping = true; o.modal_damping = atof(argv[++i]); }
        else if (value("--dt-scale")) { o.transient_arg = o.explicit_arg = o.time_arg = true; o.dt_scale = atof(argv[++i]); }
        else if (value("--dt") && !strcmp(argv[i + 1], "auto")) { o.transient_arg = o.explicit_arg = o.dt_auto = o.time_arg = true; i++; }
        else if (value("--dt")) { o.transient_arg = o.time_arg = true; run.dt = atof(argv[++i]); }
        else if (value("--steps")) { o.transient_arg = o.time_arg = true; run.n_steps = atoi(argv[++i]); }
        else if (value("--buckling")) { o.buckling_arg = true; o.buckling = atoi(argv[++i]); }
        else if (value("--buckling-tol")) { o.buckling_arg = true; o.buckling_tol = atof(argv[++i]); }
        else if (value("--solve-eps")) { o.have_solve_eps = true; o.solve_eps = run.solve_eps = atof(argv[++i]); }
        else if (value("--probe-node")) { o.transient_arg = o.have_probe = true; o.probe_node = atoi(argv[++i]); }
        else if (value("--vtu-every")) { o.transient_arg = true; o.vtu_every = atoi(argv[++i]); }
        else if (value("--newmark")) { o.time_arg = true; if (numbers(2)) { run.beta_N = list[0]; run.gamma = list[1]; } }
        else if (value("--rayleigh")) { if (numbers(2)) { run.alpha_R = list[0]; run.beta_R = list[1]; } }
        else if (value("--load-curve")) {
            o.time_arg = true;
            if (numbers(0))
                for (size_t k = 0; k < list.size(); k += 2) { run.curve_t.push_back(list[k]); run.curve_g.push_back(list[k + 1]); }
        }
        else o.path = argv[i];
    }
    if (o.vtu) SolverFunctions::ParseScalarNames(o.vtu_results, &o.vtu_sel, &o.vtu_results_why);
    if (o.have_solve_eps && !o.buckling) o.transient_arg = o.time_arg = true;   // --solve-eps belongs to --buckling, else to --transient
    run.snap_every = o.vtu ? o.vtu_every : 0;
    return o;
}

static const char *const kDropDevices = "drop --gpus/--devices";

// "... works on one device": `what` names the option (or the BCs) with its verb, `reason` what a multi-device handle lacks
static std::string OneDevice(const char *what, const char *reason, const char *or_else = "") {
    return std::string(what) + " on one device: " + reason + " (" + kDropDevices + or_else + ")";
}

// What is wrong with the options, or nothing: the tests in their fixed order, each with its own text
// (tests/golden/console_refusals.json).  Everything here needs argv alone.
static std::string Refusal(const CliOptions &o) {
    const SolverFunctions::TransientRun &run = o.run;
    const bool several = o.several_devices();
    if (o.have_modal_damping && !o.harmonic) return "--modal-damping Z belongs to --harmonic";
    if (o.harmonic) {   // first: each of these has a text of its own, whatever else the line holds
        if (o.harmonic_bad) return "--harmonic F0,F1,NF takes three numbers: the first and the last frequency in Hz and how many";
        if (!(o.n_freq >= 1) || o.n_freq != std::floor(o.n_freq) || !(o.f0 >= 0) || !(o.f1 >= o.f0) || !std::isfinite(o.f1))
            return "--harmonic F0,F1,NF needs NF >= 1, F0 >= 0 and F1 >= F0";
        if (o.n_freq > 65536) return "--harmonic F0,F1,NF takes at most 65536 frequencies";
        if (o.transient || o.explicit_run || o.buckling_arg) return "--harmonic, --transient, --explicit and --buckling are four analyses: one per run";
        if (o.modes == 0 && o.modes_tol == 0) return "--harmonic needs --modes K: the response is the superposition of the K lowest modes";
        if (o.modes_shift != 0)
            return "--harmonic needs a supported model: --modes-shift is for a model without supports, which has no static solution to correct with";
        if (o.bad_list) return "--rayleigh A,B takes two numbers";
        if (o.time_arg) return "--dt, --steps, --newmark, --load-curve and --solve-eps belong to the time integrators: a frequency response has no steps";
        if (!(run.alpha_R >= 0) || !(run.beta_R >= 0) || !std::isfinite(run.alpha_R) || !std::isfinite(run.beta_R))
            return "--rayleigh A,B needs A >= 0 and B >= 0";
        if (o.have_modal_damping && (!(o.modal_damping >= 0) || !std::isfinite(o.modal_damping))) return "--modal-damping Z needs Z >= 0";
        if (o.vtu_every < 1) return "--vtu-every E needs E >= 1";
        if (several)
            return OneDevice("--harmonic works", "the modes, the static solution and the sweep over them live on a single-rank context");
    }
    if (o.vtu && several)
        return OneDevice("--vtu works", "the result scalars average over all elements at a node, and a multi-device handle holds them in chunks",
                         ", or export in a second run");
    if (o.vtu && !o.vtu_results_why.empty()) return "--vtu-results: " + o.vtu_results_why;
    if (o.reactions && several)
        return OneDevice("--reactions works", "the internal forces add up all elements at a node, and a multi-device handle holds them in chunks");
    if (o.modes < 0 || o.modes_tol < 0 || (o.modes == 0 && o.modes_tol != 0))
        return "--modes K needs K > 0, --modes-tol T needs T >= 0 and --modes";
    if (o.modes && several)
        return OneDevice("--modes works", "the lumped mass adds up all elements at a node, and the block solves run on a single-rank context");
    if (o.modes_shift != 0 && (!o.modes || !(o.modes_shift > 0) || !std::isfinite(o.modes_shift)))
        return "--modes-shift SIGMA needs SIGMA > 0 and --modes";
    if (o.mass_kind != "lumped" && o.mass_kind != "consistent") return "--mass takes lumped or consistent, not \"" + o.mass_kind + "\"";
    if (o.mass_kind == "consistent" && !o.modes) return "--mass consistent needs --modes";
    if (o.buckling_arg) {
        if (o.buckling <= 0 || !(o.buckling_tol >= 0)) return "--buckling K needs K > 0, --buckling-tol T needs T >= 0 and --buckling";
        if (o.modes || o.transient) return "--buckling, --modes and --transient are three analyses: one per run";
        if (!(o.solve_eps >= 0)) return "--solve-eps E needs E >= 0";
        if (several)
            return OneDevice("--buckling works",
                             "the geometric stiffness adds up all elements at a node, and the block solves run on a single-rank context");
    }
    if (o.explicit_arg && !o.explicit_run) return "--dt auto and --dt-scale belong to --explicit";
    if (o.explicit_run) {
        if (o.modes || o.transient || o.buckling_arg) return "--explicit, --transient, --modes and --buckling are four analyses: one per run";
        if (o.bad_list) return "--rayleigh A,0 takes two numbers, --load-curve t0,g0,t1,g1,... an even count of them";
        if (!o.dt_auto && (!(run.dt > 0) || !std::isfinite(run.dt))) return "--explicit needs --dt DT with DT > 0, or --dt auto";
        if (o.dt_auto && run.dt != 0) return "--dt DT and --dt auto are two steps: one per run";
        if (!(o.dt_scale > 0) || !std::isfinite(o.dt_scale)) return "--dt-scale S needs S > 0";
        if (run.n_steps < 0) return "--steps N needs N >= 0";
        if (o.vtu_every < 1) return "--vtu-every K needs K >= 1";
        if (run.beta_N != 0 || run.gamma != 0 || o.have_solve_eps) return "--newmark and --solve-eps belong to --transient: an explicit step has no solve";
        if (run.beta_R != 0)
            return "--explicit takes --rayleigh A,0 only: beta_R, the stiffness-proportional damping, is a different, lagged scheme in an explicit step";
        if (!(run.alpha_R >= 0) || !std::isfinite(run.alpha_R)) return "--rayleigh A,0 needs A >= 0";
        for (size_t k = 0; k < run.curve_t.size(); k++)
            if (!std::isfinite(run.curve_t[k]) || !std::isfinite(run.curve_g[k]) || (k > 0 && run.curve_t[k] < run.curve_t[k - 1]))
                return "--load-curve needs finite values and times that do not descend";
        if (several)
            return OneDevice("--explicit works", "the lumped mass adds up all elements at a node, and the resident product and the step sums run "
                                                 "on a single-rank context");
        return "";
    }
    if (!o.transient && !o.harmonic && o.transient_arg)
        return "--dt, --steps, --newmark, --rayleigh, --load-curve, --probe-node, --solve-eps and --vtu-every belong to --transient";
    if (o.transient) {
        if (o.modes) return "--transient and --modes are two analyses: one per run";
        if (o.bad_list) return "--newmark B,G and --rayleigh A,B take two numbers, --load-curve t0,g0,t1,g1,... an even count of them";
        if (!(run.dt > 0) || !std::isfinite(run.dt)) return "--transient needs --dt DT with DT > 0";
        if (run.n_steps < 0) return "--steps N needs N >= 0";
        if (!(run.solve_eps >= 0)) return "--solve-eps E needs E >= 0";
        if (o.vtu_every < 1) return "--vtu-every K needs K >= 1";
        if (!(run.alpha_R >= 0) || !(run.beta_R >= 0)) return "--rayleigh A,B needs A >= 0 and B >= 0";
        if (!(run.beta_N == 0 && run.gamma == 0) && (!(run.gamma >= 0.5) || !(run.beta_N >= (run.gamma + 0.5) * (run.gamma + 0.5) / 4)))
            return "--newmark B,G needs G >= 1/2 and B >= (G + 1/2)^2 / 4 (unconditional stability)";
        for (size_t k = 0; k < run.curve_t.size(); k++)
            if (!std::isfinite(run.curve_t[k]) || !std::isfinite(run.curve_g[k]) || (k > 0 && run.curve_t[k] < run.curve_t[k - 1]))
                return "--load-curve needs finite values and times that do not descend";
        if (several)
            return OneDevice("--transient works", "the lumped mass adds up all elements at a node, and the shifted matrix and its solves run "
                                                  "on a single-rank context");
    }
    return "";
}

// ... and what is wrong with the file for the analysis that was asked for: --modes and --transient need the densities, all three
// the static analysis they replace or start from; the stress state of --buckling is sigma = D B u, a thermal part is out of scope
static std::string FileRefusal(const CliOptions &o, const Database &DB) {
    const std::string analysis = o.harmonic ? "--harmonic" : o.modes ? "--modes" : o.transient ? "--transient" : o.explicit_run ? "--explicit" : o.buckling ? "--buckling" : "";
    if (analysis.empty()) return "";
    if (!o.buckling && !HasDensity(DB))
        return analysis + " needs a \"Density\" boundary condition (material IDs, component 0 = rho): the file has none";
    if (DB.AnalysisLib.Type != "Linear_Statics") return analysis + " works on a Linear_Statics file";
    if (o.buckling)
        for (const auto &kv : DB.BCLib.Items())
            if (kv.second.Type == "Temperature")
                return "--buckling takes mechanical loads only: the file has a \"Temperature\" boundary condition (thermal pre-stress is "
                       "out of scope)";
    return "";
}

// ---- the prepared model ---------------------------------------------------------------------------------------------------------
// host phase times of this run (--json): the path around the GPU hot path is host work, and at scale most of the wall clock
// 
struct PhaseTimes {
    double read = 0, dof = 0, bc = 0, hot = 0, disp = 0, recover = 0, store = 0, write = 0, scalars = 0, vtu = 0, react = 0;
    double thermal = 0, loads = 0;
};

struct Prepared {
    Database DB;
    SparseMatrixHandle K;   // (behind DB: freed first)
    stan_matrix_info minfo{};
    int64_t n_nodes = 0, n_fixed = 0;
    std::vector<int32_t> nDOF_reduction;
    // F: the external load on the free DOFs; with distributed loads the right-hand side is F_rhs = F - f_int(u0)
    std::vector<double> F, F_rhs;
    bool dist_loads = false, thermal = false;
    DistributedLoads dl;
    stan_load_sums lsum{};
    ThermalLoads thermal_bc;
    stan_thermal_sums tsum{};
    std::vector<double> thermal_full;   // the thermal load over all DOFs: the supports exert f_int - this
    PhaseTimes t;
    clk::time_point t_wall, t_total, t_hot;   // the starts of the run, of the analysis and of "flatten_upload_assemble_solve"
    const std::vector<double> &F_solve() const { return dist_loads ? F_rhs : F; }
};

static const char *const kSeparator = "  ========================================================== ";

static void ClosingBanner(const Prepared &m) { printf("\n%s\n  Total CPU time: %.2f s\n%s\n", kSeparator, secs(m.t_total), kSeparator); }

// read, the refusals that need the file, AssignDOF (Solver.cs:23-50)
static int ReadModel(const SolverFunctions &Functions, const CliOptions &o, Prepared *m) {
    std::string err;
    printf("   Reading input file: ");  // Solver.cs:23-41
    fflush(stdout);
    auto t0 = clk::now();
    if (!Functions.ProtoDeserialize(o.path, &m->DB, &err)) return fail("ProtoDeserialize", err);
    m->t.read = secs(t0);
    printf("     Done\n");
    const std::string why = FileRefusal(o, m->DB);
    if (!why.empty()) return refuse(why);

    printf("   DoF ordering: ");  // Solver.cs:44-47
    fflush(stdout);
    t0 = clk::now();
    if (int rc = m->DB.AssignDOF()) return fail("AssignDOF", "code " + std::to_string(rc) +
                                                " (disconnected mesh or unknown node ID)");
    m->t.dof = secs(t0);
    printf("           Done\n");
    fputs(m->DB.Database_Summary().c_str(), stdout);  // Solver.cs:50
    return 0;
}

// Fix_DOF / nDOF_reduction / F (Solver.cs:104-152), and what of the file's BCs one device alone can do
static int BuildTables(const CliOptions &o, Prepared *m) {
    std::string err;
    const auto t0 = clk::now();
    if (BuildReductionAndLoads(m->DB, &m->nDOF_reduction, &m->n_fixed, &m->F, &err)) return fail("boundary conditions", err);
    m->dist_loads = HasDistributedLoads(m->DB);
    if (m->dist_loads && o.several_devices())
        return fail("boundary conditions", OneDevice("Pressure / BodyForce / Displacement work", "the load vector adds up all elements at a "
                                                     "node, and a multi-device handle holds them in chunks"));
    m->thermal = HasThermalLoads(m->DB);
    if (m->thermal && o.several_devices())
        return fail("boundary conditions", OneDevice("Temperature / ThermalExpansion work", "the thermal load adds up all elements at a "
                                                     "node, and a multi-device handle holds them in chunks"));
    m->t.bc = secs(t0);
    m->n_nodes = (int64_t)m->DB.NodeLib.Count();
    if (o.buckling && m->n_fixed == 0)   // before anything is assembled: K of a model without supports is not positive definite
        return refuse("--buckling needs a supported model: the file fixes no DOF");
    return 0;
}

static void Assemble(const SolverFunctions &Functions, Prepared *m) {
    m->t_hot = clk::now();
    Functions.ParallelAssembly_K(m->DB, m->nDOF_reduction, 1, "Initial", &m->K);  // Solver.cs:157
    stan_hip_matrix_info(m->K.K, &m->minfo);
}

// The loads that the reference ignores, with their console blocks; one device only.
// The Types "Temperature" and "ThermalExpansion"  give the thermal load from stan_hip_thermal_load_hex8,
// added to F in front of the distributed loads (their F - f_int(u0) then holds this load too): a block "Thermal loads:", the
// recovered stress less beta dT, the reactions of --reactions as f_int - l, a "thermal" object with --json.
// A file whose BCLib holds the Types "Pressure", "BodyForce" or "Displacement" (loads.cpp) gets their consistent nodal loads from
// stan_hip_load_vector_hex8: a block "Distributed loads:", the solve with F - f_int(u0), u0 written into the displacements at the
// fixed DOFs, a "loads" object with --json.  F becomes the whole external load, F_rhs the right-hand side.
static int BuildLoads(const SolverFunctions &Functions, Prepared *m) {
    std::string err;
    if (m->thermal) {
        const auto t0 = clk::now();
        if (BuildThermalLoads(m->DB, m->K.flat, &m->thermal_bc, &err)) return fail("boundary conditions", err);
        Functions.Thermal_Load(m->K, m->nDOF_reduction, m->thermal_bc, &m->F, &m->thermal_full, &m->tsum);
        m->t.thermal = secs(t0);
        const stan_thermal_sums &s = m->tsum;
        printf("   Thermal loads:\n");
        printf("     Total:              X %14.6e   Y %14.6e   Z %14.6e\n", s.load_sum[0], s.load_sum[1], s.load_sum[2]);
        printf("     On free DOFs:       X %14.6e   Y %14.6e   Z %14.6e\n", s.free_sum[0], s.free_sum[1], s.free_sum[2]);
        printf("     Heated volume: %.6e   mean dT: %.6e\n", s.volume, s.volume != 0 ? s.dT_integral / s.volume : 0.0);
    }
    if (m->dist_loads) {
        const auto t0 = clk::now();
        const DistributedLoads &dl = m->dl;
        stan_load_sums &s = m->lsum;
        if (BuildDistributedLoads(m->DB, m->K.flat, m->nDOF_reduction, &m->dl, &err)) return fail("boundary conditions", err);
        if (dl.mat_body.empty() && dl.face_elem.empty() && dl.disp0.empty()) {   // such BCs, but nothing in them (a Pressure
            m->F_rhs = m->F;                                                     // set that forms no boundary face, an empty
            s.n_fixed = m->n_fixed;                                              // BodyForce): the block with zeros
        } else Functions.Load_Vector(m->K, m->nDOF_reduction, dl, &m->F, &m->F_rhs, &s);
        m->t.loads = secs(t0);
        printf("   Distributed loads:\n");
        printf("     Total:              X %14.6e   Y %14.6e   Z %14.6e\n", s.load_sum[0], s.load_sum[1], s.load_sum[2]);
        printf("     On free DOFs:       X %14.6e   Y %14.6e   Z %14.6e\n", s.free_sum[0], s.free_sum[1], s.free_sum[2]);
        printf("     Loaded volume: %.6e   loaded area: %.6e (%lld faces)   prescribed DOFs: %lld\n", s.volume, s.area,
               (long long)s.n_faces, (long long)dl.n_prescribed);
    }
    return 0;
}

// ---- what the analyses share ----------------------------------------------------------------------------------------------------
// the JSON line of an analysis that replaces the static solve: {head, "name": {
static void JsonHead(const Prepared &m, const char *name) {
    printf("{\"n_gpus\": 1, \"n_dof\": %d, \"n_reduced\": %lld, \"t_wall_s\": %.3f, \"%s\": {", m.DB.nDOF, (long long)m.minfo.n_reduced,
           secs(m.t_wall), name);
}

// [x, ...] and , "name": [x, ...] -- %.17g: the doubles round-trip
static void JsonNumbers(const double *x, size_t n) {
    printf("[");
    for (size_t j = 0; j < n; j++) printf("%s%.17g", j ? ", " : "", x[j]);
    printf("]");
}
static void JsonArray(const char *name, const double *x, size_t n) {
    printf(", \"%s\": ", name);
    JsonNumbers(x, n);
}

// PREFIX_mode_NNN.vtu / PREFIX_buckle_NNN.vtu for the first `count` columns of phi [.][n_reduced]
static void ExportShapes(const SolverFunctions &Functions, const CliOptions &o, Prepared &m, const SolverFunctions::ShapeKind &kind,
                         const std::vector<double> &phi, int count) {
    const size_t N = (size_t)m.minfo.n_reduced;
    for (int j = 0; j < count; j++)
        Functions.Export_Shape_Vtu(m.K, Functions.Nodal_Vector(m.K, &phi[(size_t)j * N], m.nDOF_reduction), o.vtu_prefix, kind, j + 1);
    const char *p = o.vtu_prefix.c_str();
    if (count > 0) printf("   VTU export: %s_%s_001.vtu ... %s_%s_%03d.vtu\n", p, kind.stem, p, kind.stem, count);
}

// ---- the analyses ---------------------------------------------------------------------------------------------------------------
// --modes K [--modes-tol T] runs the modal analysis INSTEAD of the static solve and never writes the
// STdb: the lumped mass from the "Density" BCs (material IDs, component 0 = rho) and the K lowest natural frequencies from
// stan_hip_modes; a block "Natural frequencies:", with --json a "modes" object, with --vtu PREFIX one PREFIX_mode_NNN.vtu per
// mode (point arrays "Mode Shape X" / "Y" / "Z" and "Magnitude").  One device only; a file without a "Density" entry is refused.
// --modes-shift SIGMA (a model without supports): the modes of K + SIGMA M (stan_hip_matrix_shifted), printed as lambda = mu - SIGMA;
// rho is then the convergence measure of the shifted problem, "shift" in the JSON object.
// --mass consistent (default lumped, the path above) runs on the consistent mass M_c:
// stan_hip_consistent_mass_hex8 on K's layout and stan_hip_modes_pencil, under --modes-shift on stan_hip_matrix_axpy(K, SIGMA, M_c); the
// block "Natural frequencies:" names the mass and the "modes" object carries "mass": "consistent".
// Runs before the loads are built: it needs none of them.
static int RunModes(const SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    std::string err;
    MassDensity md;
    if (BuildDensity(m.DB, m.K.flat, &md, &err)) return fail("boundary conditions", err);
    std::vector<double> lambda, phi, rho;
    stan_mass_sums msum{};
    stan_modes_report rep{};
    const bool consistent = o.mass_kind == "consistent";
    Functions.Modes(m.K, m.nDOF_reduction, md, consistent ? SolverFunctions::MASS_CONSISTENT : SolverFunctions::MASS_LUMPED, o.modes,
                    o.modes_tol, &lambda, &phi, &rho, &msum, &rep, o.modes_shift);
    const double two_pi = 6.283185307179586476925;
    const size_t n = (size_t)o.modes;
    std::vector<double> hz(n);   // (a rigid-body mode of a shifted run has lambda = 0 up to the tolerance, on either side: its frequency is 0)
    for (size_t j = 0; j < n; j++) hz[j] = lambda[j] > 0 ? std::sqrt(lambda[j]) / two_pi : 0.0;
    printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
    printf("   Natural frequencies: (%sblock %d, %d outer steps, %lld CG iterations, %s)\n", consistent ? "consistent mass, " : "",
           rep.block, rep.outer, (long long)rep.cg_iterations, rep.converged ? "converged" : "NOT converged");
    if (o.modes_shift > 0)
        printf("     shift %.8e: the modes of K + shift M, lambda = mu - shift; rho is the convergence measure of the shifted\n"
               "     problem, relative to mu\n", o.modes_shift);
    printf("     mode            lambda    frequency [Hz]           rho\n");
    for (size_t j = 0; j < n; j++) printf("     %4d  %16.8e  %16.8e  %12.3e\n", (int)j + 1, lambda[j], hz[j], rho[j]);
    if (o.vtu) ExportShapes(Functions, o, m, SolverFunctions::MODE_SHAPE, phi, o.modes);
    ClosingBanner(m);
    if (o.json) {
        JsonHead(m, "modes");
        printf("\"n_modes\": %d, \"block\": %d, \"outer\": %d, \"converged\": %d, \"cg_iterations\": %lld, \"total_mass\": %.17g", o.modes,
               rep.block, rep.outer, rep.converged, (long long)rep.cg_iterations, msum.total_mass);
        if (consistent) printf(", \"mass\": \"consistent\"");
        if (o.modes_shift > 0) printf(", \"shift\": %.17g", o.modes_shift);   // rho: of the shifted problem
        JsonArray("lambda", lambda.data(), n);
        JsonArray("frequency_hz", hz.data(), n);
        JsonArray("rho", rho.data(), n);
        printf("}}\n");
    }
    return 0;
}

// the probe of --probe-node: the free DOFs of one node, by its ID, and their directions; false: the file has no such node
static bool ProbeDofs(const CliOptions &o, const Prepared &m, std::vector<int32_t> *dof, int dir[3]) {
    int64_t node = -1;
    for (int64_t n = 0; n < m.n_nodes && node < 0; n++)
        if (m.DB.NodeLib.Items()[(size_t)n].first == o.probe_node) node = n;
    if (node < 0) return false;
    for (int c = 0; c < 3; c++) {
        const int32_t d = m.K.flat.node_dof[(size_t)(3 * node + c)];
        if (m.nDOF_reduction[(size_t)d] == -1) continue;
        dir[dof->size()] = c;
        dof->push_back(d - m.nDOF_reduction[(size_t)d]);
    }
    return true;
}

// --transient --dt DT --steps N [--newmark B,G] [--rayleigh A,B] [--load-curve t0,g0,t1,g1,...] [--probe-node ID] [--solve-eps E]
//  integrates M a + C v + K u = g(t) F from rest by stan_hip_transient INSTEAD of the static solve and never
// writes the STdb: F is the model's own load (PointLoad, distributed and thermal loads), g = 1 without a curve (a step load), the
// supports homogeneous (a non-zero "Displacement" is refused); a block "Transient:", with --json a "transient" object, with
// --vtu PREFIX [--vtu-every K] PREFIX_step_NNNN.vtu every K steps (point arrays "Displacement", "Velocity", "Acceleration" X / Y / Z).
// One device only; a file without a "Density" entry is refused.
static int RunTransient(const SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    for (double x : m.dl.disp0)
        if (x != 0.0) return refuse("--transient takes homogeneous supports only: the file prescribes a non-zero \"Displacement\"");
    SolverFunctions::TransientRun run = o.run;
    int probe_dir[3] = {0, 0, 0};
    if (o.have_probe && !ProbeDofs(o, m, &run.probe_dof, probe_dir))
        return refuse("--probe-node " + std::to_string(o.probe_node) + ": the file has no such node");
    std::string err;
    MassDensity md;
    if (BuildDensity(m.DB, m.K.flat, &md, &err)) return fail("boundary conditions", err);
    std::vector<double> probe_u, snaps, energy;
    stan_mass_sums msum{};
    stan_transient_report rep{};
    Functions.Transient(m.K, m.nDOF_reduction, md, m.F_solve(), run, &probe_u, &snaps, &energy, &msum, &rep);
    const size_t np = run.probe_dof.size(), N = (size_t)m.minfo.n_reduced;
    const double bN = run.beta_N == 0 && run.gamma == 0 ? 0.25 : run.beta_N, gm = run.beta_N == 0 && run.gamma == 0 ? 0.5 : run.gamma;
    const double mean_its = rep.steps > 0 ? (double)rep.cg_iterations / rep.steps : 0.0;
    printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
    printf("   Transient: (%d steps of dt %.6e, Newmark beta %g gamma %g, Rayleigh alpha %g beta %g)\n", rep.steps, run.dt, bN, gm,
           run.alpha_R, run.beta_R);
    printf("     sigma of K + sigma M: %.8e\n", rep.sigma);
    printf("     CG iterations per step: min %d  mean %.1f  max %d\n", rep.cg_min_iterations, mean_its, rep.cg_max_iterations);
    if (np) {
        printf("     Probe node %d:\n       step                 t", o.probe_node);
        for (size_t q = 0; q < np; q++) printf("                u%c", "xyz"[probe_dir[q]]);
        printf("\n");
        for (int s = 0; s <= run.n_steps; s++) {
            printf("     %6d  %16.8e", s, (double)s * run.dt);
            for (size_t q = 0; q < np; q++) printf("  %16.8e", probe_u[(size_t)s * np + q]);
            printf("\n");
        }
    }
    const double *ef = &energy[(size_t)run.n_steps * 3];
    printf("     Final energies: kinetic %.8e  strain %.8e  external %.8e\n", ef[0], ef[1], ef[2]);
    if (o.vtu) {
        int last = 0;
        for (int s = 0; s <= run.n_steps; s += o.vtu_every) {
            Functions.Export_Step_Vtu(m.K, m.nDOF_reduction, &snaps[(size_t)(s / o.vtu_every) * 3 * N], N, o.vtu_prefix, s);
            last = s;
        }
        printf("   VTU export: %s_step_0000.vtu ... %s_step_%04d.vtu\n", o.vtu_prefix.c_str(), o.vtu_prefix.c_str(), last);
    }
    ClosingBanner(m);
    if (o.json) {
        JsonHead(m, "transient");
        printf("\"steps\": %d, \"dt\": %.17g, \"beta_N\": %.17g, \"gamma\": %.17g, \"alpha_R\": %.17g, \"beta_R\": %.17g, \"sigma\": %.17g, "
               "\"cg_iterations\": %lld, \"cg_min_iterations\": %d, \"cg_max_iterations\": %d, \"cg_worst_type\": %d, \"total_mass\": %.17g",
               rep.steps, run.dt, bN, gm, run.alpha_R, run.beta_R, rep.sigma, (long long)rep.cg_iterations, rep.cg_min_iterations,
               rep.cg_max_iterations, rep.cg_worst_type, msum.total_mass);
        JsonArray("energy_final", ef, 3);
        if (np) {
            printf(", \"probe_node\": %d, \"probe_direction\": [", o.probe_node);
            for (size_t q = 0; q < np; q++) printf("%s%d", q ? ", " : "", probe_dir[q]);
            printf("], \"probe_u\": [");
            for (int s = 0; s <= run.n_steps; s++) {
                printf("%s", s ? ", " : "");
                JsonNumbers(&probe_u[(size_t)s * np], np);
            }
            printf("]");
        }
        printf("}}\n");
    }
    return 0;
}

// --explicit --steps N [--dt DT | --dt auto] [--dt-scale S] [--rayleigh A,0] [--load-curve ...] [--probe-node ID] (DESIGN.md section
// 3.14) integrates M a + alpha_R M v + K u = g(t) F from rest by stan_hip_explicit INSTEAD of the static solve and never writes the
// STdb: the load, the curve, the supports, the probe and the .vtu files as for --transient; --dt auto is S * 2 / sqrt(lambda_upper), S
// = 0.9 unless --dt-scale gives it.  A block "Explicit:", with --json an "explicit" object.  One device only; a file without a
// "Density" entry is refused.
static int RunExplicit(const SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    for (double x : m.dl.disp0)
        if (x != 0.0) return refuse("--explicit takes homogeneous supports only: the file prescribes a non-zero \"Displacement\"");
    SolverFunctions::ExplicitRun run;
    run.dt_auto = o.dt_auto; run.dt = o.run.dt; run.dt_scale = o.dt_scale; run.alpha_R = o.run.alpha_R; run.n_steps = o.run.n_steps;
    run.snap_every = o.run.snap_every; run.curve_t = o.run.curve_t; run.curve_g = o.run.curve_g;
    int probe_dir[3] = {0, 0, 0};
    if (o.have_probe && !ProbeDofs(o, m, &run.probe_dof, probe_dir))
        return refuse("--probe-node " + std::to_string(o.probe_node) + ": the file has no such node");
    std::string err;
    MassDensity md;
    if (BuildDensity(m.DB, m.K.flat, &md, &err)) return fail("boundary conditions", err);
    std::vector<double> probe_u, snaps, energy;
    stan_mass_sums msum{};
    stan_explicit_report rep{};
    Functions.Explicit(m.K, m.nDOF_reduction, md, m.F_solve(), &run, &probe_u, &snaps, &energy, &msum, &rep);
    const size_t np = run.probe_dof.size(), N = (size_t)m.minfo.n_reduced;
    printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
    printf("   Explicit: (%d steps of dt %.6e%s, central differences, Rayleigh alpha %g)\n", rep.steps, run.dt,
           run.dt_auto ? " = dt-scale x dt_stable" : "", run.alpha_R);
    printf("     dt_stable = 2 / sqrt(lambda_upper): %.8e\n", rep.dt_stable);
    printf("     lambda_upper (row bound): %.8e   lambda_power (%d iterations, a lower bound): %.8e\n", rep.lambda_upper, run.n_power,
           rep.lambda_power);
    if (np) {
        printf("     Probe node %d:\n       step                 t", o.probe_node);
        for (size_t q = 0; q < np; q++) printf("                u%c", "xyz"[probe_dir[q]]);
        printf("\n");
        for (int s = 0; s <= run.n_steps; s++) {
            printf("     %6d  %16.8e", s, (double)s * run.dt);
            for (size_t q = 0; q < np; q++) printf("  %16.8e", probe_u[(size_t)s * np + q]);
            printf("\n");
        }
    }
    const double *ef = &energy[energy.size() - 3];
    printf("     Final energies: kinetic %.8e  strain %.8e  external %.8e\n", ef[0], ef[1], ef[2]);
    if (o.vtu) {
        int last = 0;
        for (int s = 0; s <= run.n_steps; s += o.vtu_every) {
            Functions.Export_Step_Vtu(m.K, m.nDOF_reduction, &snaps[(size_t)(s / o.vtu_every) * 3 * N], N, o.vtu_prefix, s);
            last = s;
        }
        printf("   VTU export: %s_step_0000.vtu ... %s_step_%04d.vtu\n", o.vtu_prefix.c_str(), o.vtu_prefix.c_str(), last);
    }
    ClosingBanner(m);
    if (o.json) {
        JsonHead(m, "explicit");
        printf("\"steps\": %d, \"dt\": %.17g, \"dt_auto\": %d, \"dt_scale\": %.17g, \"dt_stable\": %.17g, \"lambda_upper\": %.17g, "
               "\"lambda_power\": %.17g, \"n_power\": %d, \"alpha_R\": %.17g, \"first_nonfinite_step\": %d, \"total_mass\": %.17g",
               rep.steps, run.dt, run.dt_auto ? 1 : 0, run.dt_scale, rep.dt_stable, rep.lambda_upper, rep.lambda_power, run.n_power,
               run.alpha_R, rep.first_nonfinite_step, msum.total_mass);
        JsonArray("energy_final", ef, 3);
        if (np) {
            printf(", \"probe_node\": %d, \"probe_direction\": [", o.probe_node);
            for (size_t q = 0; q < np; q++) printf("%s%d", q ? ", " : "", probe_dir[q]);
            printf("], \"probe_u\": [");
            for (int s = 0; s <= run.n_steps; s++) {
                printf("%s", s ? ", " : "");
                JsonNumbers(&probe_u[(size_t)s * np], np);
            }
            printf("]");
        }
        printf("}}\n");
    }
    return 0;
}

// --harmonic F0,F1,NF --modes K [--mass consistent] [--modes-tol T] [--rayleigh A,B] [--modal-damping Z] [--probe-node ID] (DESIGN.md
// section 3.15) finds the steady-state response to the file's loads times e^{i w t} at NF frequencies from F0 to F1 Hz and never writes
// the STdb: the modes exactly as --modes finds them (on the assembled K, before any solve has scaled it), the static solve of the
// file's loads for the static correction, then stan_hip_harmonic_dev on what stayed in device memory (SolverFunctions::HarmonicResident).  A block "Frequency response:", with --json a "harmonic" object,
// with --vtu PREFIX PREFIX_peak.vtu ("Peak Amplitude", "Peak Frequency") and PREFIX_freq_NNNN.vtu ("Displacement Re" / "Im") for every
// E-th frequency.  One device only; a file without a "Density" entry is refused.
static int RunHarmonic(SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    for (double x : m.dl.disp0)
        if (x != 0.0) return refuse("--harmonic takes homogeneous supports only: the file prescribes a non-zero \"Displacement\"");
    SolverFunctions::HarmonicRun run;
    run.alpha_R = o.run.alpha_R; run.beta_R = o.run.beta_R; run.zeta = o.have_modal_damping ? o.modal_damping : -1.0;
    run.snap_every = o.vtu ? o.vtu_every : 0;
    int probe_dir[3] = {0, 0, 0};
    if (o.have_probe && !ProbeDofs(o, m, &run.probe_dof, probe_dir))
        return refuse("--probe-node " + std::to_string(o.probe_node) + ": the file has no such node");
    const double two_pi = 6.283185307179586476925;
    const int nf = (int)o.n_freq;
    std::vector<double> hz((size_t)nf);
    for (int f = 0; f < nf; f++) hz[(size_t)f] = nf == 1 ? o.f0 : o.f0 + (o.f1 - o.f0) * ((double)f / (double)(nf - 1));
    for (double x : hz) run.omega.push_back(two_pi * x);
    std::string err;
    MassDensity md;
    if (BuildDensity(m.DB, m.K.flat, &md, &err)) return fail("boundary conditions", err);

    std::vector<double> lambda, p, probe, snaps, peak;
    std::vector<int32_t> peak_idx;
    stan_mass_sums msum{};
    stan_modes_report mrep{};
    stan_harmonic_report rep{};
    const bool consistent = o.mass_kind == "consistent";
    Functions.HarmonicResident(m.K, m.nDOF_reduction, md, consistent ? SolverFunctions::MASS_CONSISTENT : SolverFunctions::MASS_LUMPED,
                               o.modes, o.modes_tol, m.F_solve(), m.DB.AnalysisLib, run, &lambda, &p, &probe, &snaps, &peak, &peak_idx, &msum,
                               &mrep, &rep);
    printf("   CG iterations: %d, scaled relative residual %.3e\n", Functions.last_iterations, Functions.last_rel_residual);

    const size_t k = (size_t)o.modes, np = run.probe_dof.size(), N = (size_t)m.minfo.n_reduced;
    std::vector<double> mode_hz(k), ratio(k);   // the damping ratio of mode j: c_j / (2 sqrt(lambda_j))
    for (size_t j = 0; j < k; j++) {
        const double w = std::sqrt(lambda[j]);
        mode_hz[j] = w / two_pi;
        ratio[j] = (run.alpha_R + run.beta_R * lambda[j]) / (2.0 * w) + (run.zeta >= 0 ? run.zeta : 0.0);
    }
    // the largest amplitude: its reduced DOF as node ID and direction
    int peak_node = 0, peak_dir = 0;
    for (int64_t n = 0; n < m.n_nodes && rep.peak_dof >= 0; n++)
        for (int c = 0; c < 3; c++) {
            const int32_t d = m.K.flat.node_dof[(size_t)(3 * n + c)];
            if (m.nDOF_reduction[(size_t)d] != -1 && d - m.nDOF_reduction[(size_t)d] == rep.peak_dof) {
                peak_node = m.DB.NodeLib.Items()[(size_t)n].first;
                peak_dir = c;
            }
        }
    const double peak_hz = rep.peak_freq >= 0 ? hz[(size_t)rep.peak_freq] : 0.0;
    const double deg = 360.0 / two_pi;
    printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
    printf("   Frequency response: (%d frequencies from %.6e to %.6e Hz, %d modes%s, static correction)\n", nf, hz.front(), hz.back(),
           o.modes, consistent ? ", consistent mass" : "");
    printf("     modes: block %d, %d outer steps, %lld CG iterations, %s\n", mrep.block, mrep.outer, (long long)mrep.cg_iterations,
           mrep.converged ? "converged" : "NOT converged");
    printf("     damping: Rayleigh alpha %g beta %g, modal ratio %g\n", run.alpha_R, run.beta_R, run.zeta >= 0 ? run.zeta : 0.0);
    printf("     mode    frequency [Hz]      modal load p   damping ratio\n");
    for (size_t j = 0; j < k; j++) printf("     %4d  %16.8e  %16.8e  %14.6e\n", (int)j + 1, mode_hz[j], p[j], ratio[j]);
    printf("     Largest amplitude: %.8e at node %d, direction %c, at %.8e Hz\n", rep.peak, peak_node, "XYZ"[peak_dir], peak_hz);
    if (np) {
        printf("     Probe node %d:\n      index    frequency [Hz]", o.probe_node);
        for (size_t q = 0; q < np; q++) printf("              |u%c|    phase(u%c) [deg]", "xyz"[probe_dir[q]], "xyz"[probe_dir[q]]);
        printf("\n");
        for (int f = 0; f < nf; f++) {
            printf("     %6d  %16.8e", f, hz[(size_t)f]);
            for (size_t q = 0; q < np; q++) {
                const double re = probe[((size_t)f * np + q) * 2], im = probe[((size_t)f * np + q) * 2 + 1];
                printf("  %16.8e  %16.8e", std::hypot(re, im), std::atan2(im, re) * deg);
            }
            printf("\n");
        }
    }
    if (o.vtu) {
        Functions.Export_Peak_Vtu(m.K, m.nDOF_reduction, peak.data(), peak_idx.data(), hz, o.vtu_prefix);
        int last = 0;
        for (int f = 0; f < nf; f += o.vtu_every) {
            Functions.Export_Freq_Vtu(m.K, m.nDOF_reduction, &snaps[(size_t)(f / o.vtu_every) * 2 * N], N, o.vtu_prefix, f);
            last = f;
        }
        printf("   VTU export: %s_peak.vtu, %s_freq_0000.vtu ... %s_freq_%04d.vtu\n", o.vtu_prefix.c_str(), o.vtu_prefix.c_str(),
               o.vtu_prefix.c_str(), last);
    }
    ClosingBanner(m);
    if (o.json) {
        JsonHead(m, "harmonic");
        printf("\"n_modes\": %d, \"n_freq\": %d, \"f0_hz\": %.17g, \"f1_hz\": %.17g, \"alpha_R\": %.17g, \"beta_R\": %.17g, \"modal_damping\": %.17g, "
               "\"static_cg_iterations\": %d, \"modes_converged\": %d, \"total_mass\": %.17g, \"peak\": %.17g, \"peak_node\": %d, "
               "\"peak_direction\": %d, \"peak_frequency_hz\": %.17g, \"peak_frequency_index\": %d",
               o.modes, nf, o.f0, o.f1, run.alpha_R, run.beta_R, run.zeta >= 0 ? run.zeta : 0.0, Functions.last_iterations, mrep.converged,
               msum.total_mass, rep.peak, peak_node, peak_dir, peak_hz, rep.peak_freq);
        if (consistent) printf(", \"mass\": \"consistent\"");
        JsonArray("lambda", lambda.data(), k);
        JsonArray("mode_frequency_hz", mode_hz.data(), k);
        JsonArray("modal_load", p.data(), k);
        JsonArray("damping_ratio", ratio.data(), k);
        JsonArray("frequency_hz", hz.data(), (size_t)nf);
        if (np) {
            printf(", \"probe_node\": %d, \"probe_direction\": [", o.probe_node);
            for (size_t q = 0; q < np; q++) printf("%s%d", q ? ", " : "", probe_dir[q]);
            printf("], \"probe_re_im\": [");   // [n_freq][n_probe][2]
            for (int f = 0; f < nf; f++) {
                printf("%s[", f ? ", " : "");
                for (size_t q = 0; q < np; q++) {
                    printf("%s", q ? ", " : "");
                    JsonNumbers(&probe[((size_t)f * np + q) * 2], 2);
                }
                printf("]");
            }
            printf("]");
        }
        printf("}}\n");
    }
    return 0;
}

// --buckling K [--buckling-tol T] [--solve-eps E] runs the static solve under the model's own loads, builds
// G = K_g(U) (stan_hip_geometric_stiffness_hex8) and finds the K lowest positive load factors (stan_hip_buckling): a block
// "Buckling load factors:", with --json a "buckling" object, with --vtu PREFIX one PREFIX_buckle_NNN.vtu per factor; the STdb is
// never written.  Refused before anything is computed: several devices, a "Temperature" boundary condition, no supports.
static int RunBuckling(SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    const std::vector<double> U = Functions.LinearSolver_CG(m.K, m.F_solve(), m.DB.AnalysisLib);
    printf("   CG iterations: %d, scaled relative residual %.3e\n", Functions.last_iterations, Functions.last_rel_residual);
    std::vector<double> disp = Functions.Nodal_Vector(m.K, U.data(), m.nDOF_reduction);
    if (m.dist_loads && !m.dl.disp0.empty())   // the solved field is U on top of the prescribed u0
        for (size_t k = 0; k < disp.size(); k++) disp[k] += m.dl.disp0[k];
    std::vector<double> factor, phi, rho;
    stan_buckling_report rep{};
    Functions.Buckling(m.K, m.nDOF_reduction, disp, o.buckling, o.buckling_tol, o.solve_eps, &factor, &phi, &rho, &rep);
    const int found = rep.n_positive < o.buckling ? rep.n_positive : o.buckling;
    printf("   Buckling load factors: (block %d, %d outer steps, %lld CG iterations, %s)\n", rep.block, rep.outer,
           (long long)rep.cg_iterations, rep.converged ? "converged" : "NOT converged");
    printf("     mode            factor           rho\n");
    for (int j = 0; j < found; j++) printf("     %4d  %16.8e  %12.3e\n", j + 1, factor[(size_t)j], rho[(size_t)j]);
    if (found < o.buckling) printf("     only %d positive factors in the block of %d\n", rep.n_positive, rep.block);
    if (rep.lowest_negative_factor != 0)
        printf("     lowest negative factor (the load reversed): %.8e\n", rep.lowest_negative_factor);
    if (o.vtu) ExportShapes(Functions, o, m, SolverFunctions::BUCKLING_SHAPE, phi, found);
    ClosingBanner(m);
    if (o.json) {
        JsonHead(m, "buckling");
        printf("\"n_modes\": %d, \"block\": %d, \"outer\": %d, \"converged\": %d, \"n_positive\": %d, \"cg_iterations\": %lld, "
               "\"static_cg_iterations\": %d, \"lowest_negative_factor\": %.17g",
               o.buckling, rep.block, rep.outer, rep.converged, rep.n_positive, (long long)rep.cg_iterations, Functions.last_iterations,
               rep.lowest_negative_factor);
        JsonArray("factor", factor.data(), (size_t)found);
        JsonArray("rho", rho.data(), (size_t)found);
        printf("}}\n");
    }
    return 0;
}

// --reactions (after the solve: support reactions and applied load by axis, the out-of-balance norm of F - f_int(U) against |F| and
// the largest out-of-balance force with its node, from stan_hip_internal_forces_hex8 -- no step of the reference, nothing of it
// reaches the STdb; with --json an "equilibrium" object, with --vtu the point arrays "Reaction Force X / Y / Z"; one device only).
// f_int(U) element by element, never through K; the displacement vector carries 0 at the fixed DOFs
static void Reactions(const SolverFunctions &Functions, const CliOptions &o, Prepared &m, const std::vector<double> &disp,
                      stan_equilibrium *eq_out, std::vector<double> *reaction) {
    stan_equilibrium &eq = *eq_out;
    const std::vector<int32_t> &node_dof = m.K.flat.node_dof;
    const auto t0 = clk::now();
    Functions.Equilibrium(m.K, disp, m.F, m.nDOF_reduction, nullptr, o.vtu || m.thermal ? reaction : nullptr, &eq);
    if (m.thermal)   // the supports exert f_int - l at the fixed DOFs: the arrays, and the sums by direction in node order
        for (int64_t n = 0; n < m.n_nodes; n++)
            for (int c = 0; c < 3; c++) {
                const size_t d = (size_t)node_dof[(size_t)(3 * n + c)];
                if (m.nDOF_reduction[d] != -1) continue;
                (*reaction)[d] -= m.thermal_full[d];
                eq.reaction_sum[c] -= m.thermal_full[d];
            }
    m.t.react = secs(t0);
    int64_t node = -1;
    for (int64_t n = 0; n < m.n_nodes && eq.residual_max_dof >= 0; n++)
        if (node_dof[(size_t)(3 * n)] == (int32_t)(eq.residual_max_dof - eq.residual_max_dof % 3)) { node = n; break; }
    printf("   Equilibrium check (internal forces of the solved displacements):\n");
    printf("     Support reactions:  X %14.6e   Y %14.6e   Z %14.6e\n", eq.reaction_sum[0], eq.reaction_sum[1], eq.reaction_sum[2]);
    printf("     Applied load:       X %14.6e   Y %14.6e   Z %14.6e\n", eq.load_sum[0], eq.load_sum[1], eq.load_sum[2]);
    printf("     Out of balance:     |F - f_int| = %.3e, %.3e of |F|\n", eq.residual_norm2,
           eq.load_norm2 > 0 ? eq.residual_norm2 / eq.load_norm2 : 0.0);
    if (node >= 0)
        printf("     Largest:            %.3e at node %d, direction %c\n", eq.residual_max, m.DB.NodeLib.Items()[(size_t)node].first,
               "XYZ"[eq.residual_max_dof % 3]);
}

// Solver.cs:81-90 (initialise step 0/1), :203-210 (update), Main :56: every node / element object is initialised and updated with
// the results, then ExportOutput serialises the objects.  By default the writer takes the results from the flat arrays instead
// (Database::ResultView: the same bytes without 13 million small heap objects); --object-results walks the reference's object path
// (tests/test_gpu_parity.py compares the files).
static void StoreResults(const CliOptions &o, Prepared &m, const std::vector<double> &disp, const std::vector<double> &strain,
                         const std::vector<double> &stress) {
    if (!o.object_results) {
        m.DB.results.disp = disp.data();
        stan_results *res = m.K.results;
        m.DB.results.fetch = [res](size_t e0, size_t e1, const double **sn, const double **ss) {
            return stan_hip_results_map(res, (int64_t)e0, (int64_t)e1, sn, ss) == STAN_OK;
        };
        return;
    }
    auto &nodes = m.DB.NodeLib.Items();
    ParallelRanges(nodes.size(), [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            Node &n = nodes[i].second;
            n.Initialize_StepZero();
            n.Initialize_NewDisp(1);
            for (int d = 0; d < 3; d++) n.dU_buffer[d] = disp[3 * i + (size_t)d];
            n.Update_Displacement(1);
        }
    });
    auto &elems = m.DB.ElemLib.Items();
    ParallelRanges(elems.size(), [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            Element &e = elems[i].second;
            e.Initialize_StepZero();
            e.Initialize_Increment(1);
            memcpy(e.Strain[1].M.data(), &strain[48 * i], 48 * sizeof(double));
            memcpy(e.Stress[1].M.data(), &stress[48 * i], 48 * sizeof(double));
        }
    });
}

// one machine-readable line per run (metrics/logging), after the export
static void StaticsJson(const SolverFunctions &Functions, const CliOptions &o, const Prepared &m, const stan_profile &pr,
                        const stan_equilibrium &eq) {
    const PhaseTimes &t = m.t;
    const double spmv_ms = pr.spmv_launches ? pr.spmv_ms_total / (double)pr.spmv_launches : 0;
    const double wall = secs(m.t_wall), dev = (pr.assemble_ms + pr.cg_ms) * 1e-3;
    printf("{\"n_gpus\": %d, \"n_dof\": %d, \"n_reduced\": %lld, \"blocks_3x3\": %lld, \"cg_iterations\": %d, "
           "\"termination_type\": %d, \"rel_residual\": %.3e, \"t_assembly_s\": %.4f, \"t_cg_s\": %.4f, "
           "\"spmv_ms\": %.4f, \"spmv_GBs\": %.1f, \"hbm_frac\": %.3f, "
           "\"host_threads\": %d, \"t_wall_s\": %.3f, \"t_device_assembly_plus_cg_s\": %.4f, "
           "\"phases_s\": {\"read_parse\": %.3f, \"assign_dof\": %.3f, \"bc_tables\": %.3f, "
           "\"flatten_upload_assemble_solve\": %.3f, \"displacements\": %.3f, \"stress_recovery\": %.3f, "
           "\"store_results\": %.3f, \"serialize_write\": %.3f, \"result_scalars\": %.6f, \"write_vtu\": %.6f}",
           o.several_devices() ? (int)o.devices.size() : 1, m.DB.nDOF, (long long)m.minfo.n_reduced, (long long)m.minfo.n_blocks,
           Functions.last_iterations, Functions.last_termination_type, Functions.last_rel_residual, Functions.last_assembly_s,
           Functions.last_cg_s, spmv_ms, spmv_ms > 0 ? pr.spmv_bytes / spmv_ms / 1e6 : 0.0,
           spmv_ms > 0 ? pr.spmv_bytes / spmv_ms / 1e6 / 8000.0 : 0.0,
           // (the two .vtu phases to the microsecond: on a small model they take less than the 0.5 ms that %.3f shows as 0)
           HostThreads(), wall, dev, t.read, t.dof, t.bc, t.hot, t.disp, t.recover, t.store, t.write, t.scalars, t.vtu);
    if (o.reactions)   // %.17g: the doubles round-trip
        printf(", \"equilibrium\": {\"reaction_sum\": [%.17g, %.17g, %.17g], \"load_sum\": [%.17g, %.17g, %.17g], "
               "\"fint_sum\": [%.17g, %.17g, %.17g], \"residual_norm2\": %.17g, \"load_norm2\": %.17g, \"residual_max\": %.17g, "
               "\"residual_max_dof\": %lld, \"n_fixed\": %lld, \"t_s\": %.3f}",
               eq.reaction_sum[0], eq.reaction_sum[1], eq.reaction_sum[2], eq.load_sum[0], eq.load_sum[1], eq.load_sum[2],
               eq.fint_sum[0], eq.fint_sum[1], eq.fint_sum[2], eq.residual_norm2, eq.load_norm2, eq.residual_max,
               (long long)eq.residual_max_dof, (long long)eq.n_fixed, t.react);
    if (m.dist_loads) {
        const stan_load_sums &s = m.lsum;
        printf(", \"loads\": {\"load_sum\": [%.17g, %.17g, %.17g], \"free_sum\": [%.17g, %.17g, %.17g], \"volume\": %.17g, "
               "\"area\": %.17g, \"n_faces\": %lld, \"n_fixed\": %lld, \"n_prescribed\": %lld, \"t_s\": %.3f}",
               s.load_sum[0], s.load_sum[1], s.load_sum[2], s.free_sum[0], s.free_sum[1], s.free_sum[2], s.volume, s.area,
               (long long)s.n_faces, (long long)s.n_fixed, (long long)m.dl.n_prescribed, t.loads);
    }
    if (m.thermal) {
        const stan_thermal_sums &s = m.tsum;
        printf(", \"thermal\": {\"load_sum\": [%.17g, %.17g, %.17g], \"free_sum\": [%.17g, %.17g, %.17g], \"volume\": %.17g, "
               "\"dT_integral\": %.17g, \"mean_dT\": %.17g, \"n_fixed\": %lld, \"t_s\": %.3f}",
               s.load_sum[0], s.load_sum[1], s.load_sum[2], s.free_sum[0], s.free_sum[1], s.free_sum[2], s.volume, s.dT_integral,
               s.volume != 0 ? s.dT_integral / s.volume : 0.0, (long long)s.n_fixed, t.thermal);
    }
    printf("}\n");
}

// The static solve (Solver.cs:157-217) and ExportOutput: the input path is overwritten with the results (Solver.cs:454-462).
// --vtu PREFIX (after the solve, PREFIX_001.vtu with the point scalars of Part.Load_Scalar as Part.ExportGrid exports them;
// --vtu-results "name,name,..." picks them by the reference's result strings, default all 24; --vtu-cells adds their Max / Average /
// Min cell arrays; one device only).
static int RunStatics(SolverFunctions &Functions, const CliOptions &o, Prepared &m) {
    std::vector<double> U((size_t)(m.DB.nDOF - m.n_fixed), 0.0);
    const std::string &ls = m.DB.AnalysisLib.LinSolver;
    if ((ls == "Cholesky" || ls == "LU") && o.several_devices())
        return fail("solver selection", std::string("the direct solvers run on one device's export of K: ") + kDropDevices);
    if (ls == "CG") {  // Solver.cs:162
        U = Functions.LinearSolver_CG(m.K, m.F_solve(), m.DB.AnalysisLib);
        printf("   CG iterations: %d, scaled relative residual %.3e\n", Functions.last_iterations, Functions.last_rel_residual);
    } else if (ls == "Cholesky") U = Functions.LinearSolver_Cholesky(m.K, m.F_solve());  // Solver.cs:163: CPU fallback (direct.cpp)
    else if (ls == "LU") U = Functions.LinearSolver_LU(m.K, m.F_solve());                // Solver.cs:164
    // (any other string: the reference leaves U = 0, Solver.cs:160-164)
    m.t.hot = secs(m.t_hot);   // flatten + context + upload + assembly + solve + download

    // U = Include_BC_DOF(U, nDOF_reduction); node.dU_buffer[d] = U[DOF[d]] (Solver.cs:168-178)
    auto t0 = clk::now();
    std::vector<double> disp = Functions.Nodal_Vector(m.K, U.data(), m.nDOF_reduction);
    if (!m.dl.disp0.empty())   // the supports' own displacement, before recovery, reactions, .vtu and the export
        for (size_t k = 0; k < disp.size(); k++)
            if (m.nDOF_reduction[(size_t)m.K.flat.node_dof[k]] == -1) disp[k] = m.dl.disp0[k];
    m.t.disp = secs(t0);

    printf("   Stress recovery: ");  // Solver.cs:183
    fflush(stdout);
    t0 = clk::now();
    std::vector<double> strain, stress;
    // the flat-array export takes the element results from the device chunk by chunk while it encodes (the
    // download overlaps the encoding and the file writes); --object-results needs them as whole host arrays
    if (o.object_results) Functions.Recovery_Stress(m.K, disp, &strain, &stress);
    else Functions.Recovery_Stress_Keep(m.K, disp);
    if (m.thermal) Functions.Thermal_Stress(m.K, m.thermal_bc, o.object_results ? &stress : nullptr);   // before .vtu, scalars and export
    m.t.recover = secs(t0);
    printf("            Done\n");
    stan_profile pr{};
    if (o.json) stan_hip_get_profile(m.K.ctx, &pr);
    stan_equilibrium eq{};
    std::vector<double> reaction;
    if (o.reactions) Reactions(Functions, o, m, disp, &eq, &reaction);
    // the .vtu takes its scalars from the results while they are still on the device (the STdb export frees them)
    if (o.vtu) {
        Functions.Export_Vtu(m.K, disp, o.object_results ? &strain : nullptr, o.object_results ? &stress : nullptr, o.vtu_prefix,
                             o.vtu_sel, o.vtu_cells, &m.t.scalars, &m.t.vtu, o.reactions ? &reaction : nullptr);
        printf("   VTU export: %s_001.vtu\n", o.vtu_prefix.c_str());
    }
    t0 = clk::now();
    StoreResults(o, m, disp, strain, stress);
    m.t.store = secs(t0);
    ClosingBanner(m);
    m.DB.AnalysisLib.Result_StepNo = 1;
    t0 = clk::now();
    std::string err;
    if (!Functions.ProtoSerialize(m.DB, o.path, o.packed, &err)) return fail("ExportOutput", err);
    m.t.write = secs(t0);
    if (o.json) StaticsJson(Functions, o, m, pr, eq);
    return 0;
}

int main(int argc, char **argv) {
    const CliOptions o = ParseArgs(argc, argv);
    if (o.help) {
        fputs(kUsage, stdout);
        fputs(kExplicitUsage, stdout);
        fputs(kHarmonicUsage, stdout);
        return 0;
    }
    if (o.path.empty()) {  // Path = path[0] -> IndexOutOfRangeException in the reference
        fputs(kUsage, stderr);
        return 2;
    }
    const std::string why = Refusal(o);
    if (!why.empty()) return refuse(why);

    SolverOptions opt;
    opt.device = o.device; opt.devices = o.devices; opt.precision = o.precision; opt.placement_tries = o.placement_tries;
    opt.merit_stop = o.merit_stop; opt.profile = o.json; opt.p2p = o.p2p;
    SolverFunctions Functions(opt);  // Solver.cs:16
    Functions.Welcome_Messsage();
    Functions.Prewarm();             // the device context comes up while the file is read

    Prepared m;
    m.t_wall = clk::now();
    if (int rc = ReadModel(Functions, o, &m)) return rc;

    if (m.DB.AnalysisLib.Type == "Linear_Statics") try {  // Solver.cs:53-57, SolverLinearStatics :72-217
        m.t_total = clk::now();
        printf("\n%s\n        LINEAR STATIC ANALYSIS \n%s\n", kSeparator, kSeparator);
        if (int rc = BuildTables(o, &m)) return rc;
        Assemble(Functions, &m);
        if (o.harmonic) {   // (--modes K belongs to it)
            if (int rc = BuildLoads(Functions, &m)) return rc;
            return RunHarmonic(Functions, o, m);
        }
        if (o.modes) return RunModes(Functions, o, m);   // before the loads are built
        if (int rc = BuildLoads(Functions, &m)) return rc;
        if (o.transient) return RunTransient(Functions, o, m);
        if (o.explicit_run) return RunExplicit(Functions, o, m);
        if (o.buckling) return RunBuckling(Functions, o, m);
        return RunStatics(Functions, o, m);
    } catch (const std::exception &e) {  // the C# lets these escape Main as unhandled exceptions
        return fail("SolverLinearStatics", e.what());
    } else if (m.DB.AnalysisLib.Type == "Nonlinear_Statics") {
        return fail("analysis type", "Nonlinear_Statics is unreachable from the GUI "
                                     "(MainWindow.xaml.cs:444) and outside the hot path");
    }

    // ExportOutput: overwrite the input path (Solver.cs:454-462) -- also when the analysis type is not one
    // this driver solves (Main writes the file back regardless)
    std::string err;
    if (!Functions.ProtoSerialize(m.DB, o.path, o.packed, &err)) return fail("ExportOutput", err);
    return 0;
}
