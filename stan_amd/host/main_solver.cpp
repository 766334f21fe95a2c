// main_solver.cpp -- native console driver: `stan_solver <model.STdb>`.
// Reproduces Solver.Main / SolverLinearStatics / ExportOutput (Solver.cs:18-217, 454-462)
// on top of the two C-ABI libraries: read STdb -> materials -> AssignDOF -> BC tables ->
// assemble on the GPU -> CG on the GPU -> displacements -> stress recovery on the GPU ->
// overwrite the input file with the results (Result_StepNo = 1).
// Differences kept on purpose: no console-window sizing in the banner
// (SolverFunctions.cs:18-20 throws when stdout is redirected) and no 10 s sleep at exit
// (Solver.cs:67-68).  LinSolver "Cholesky"/"LU" (SolverFunctions.cs:332-516) are outside the GPU
// hot path: K is exported as the upper CRS the reference holds and solved on the CPU (direct.cpp).
// Extra switches (never stored in the STdb): --device N, --gpus N (devices 0..N-1) or --devices a,b,c
// (several GPUs from this ONE process: stan_hip_init_multi, rows of K sharded, RCCL inside the CG),
// --mixed, --fixed48, --no-merit-stop, --packed, --placement-tries N (default 16; 1 = plain allocation),
// --p2p (several GPUs: the CG exchanges peer to peer instead of over RCCL, STAN_OPT_COMM_P2P),
// --object-results (store the results in the Node / Element objects before the export, as the reference does,
// instead of encoding them from the flat arrays: same bytes), --json (one JSON line with sizes, iterations,
// device and host phase times and the SpMV's HBM rate), --vtu PREFIX (after the solve, PREFIX_001.vtu with the point
// scalars of Part.Load_Scalar as Part.ExportGrid exports them; --vtu-results "name,name,..." picks them by the reference's
// result strings, default all 24; --vtu-cells adds their Max / Average / Min cell arrays; one device only), --reactions
// (after the solve: support reactions and applied load by axis, the out-of-balance norm of F - f_int(U) against |F| and the
// largest out-of-balance force with its node, from stan_hip_internal_forces_hex8 -- no step of the reference, nothing of it
// reaches the STdb; with --json an "equilibrium" object, with --vtu the point arrays "Reaction Force X / Y / Z"; one device
// only).  A file whose BCLib holds the Types "Pressure", "BodyForce" or "Displacement" (loads.cpp; the reference ignores them)
// gets their consistent nodal loads from stan_hip_load_vector_hex8: a block "Distributed loads:", the solve with
// F - f_int(u0), u0 written into the displacements at the fixed DOFs, a "loads" object with --json; one device only.
// The Types "Temperature" and "ThermalExpansion"  give the thermal load from stan_hip_thermal_load_hex8,
// added to F in front of the distributed loads: a block "Thermal loads:", the recovered stress less beta dT, the reactions of
// --reactions as f_int - l, a "thermal" object with --json; one device only.
// --modes K [--modes-tol T] runs the modal analysis INSTEAD of the static solve and never writes the
// STdb: the lumped mass from the "Density" BCs (material IDs, component 0 = rho) and the K lowest natural frequencies from
// stan_hip_modes; a block "Natural frequencies:", with --json a "modes" object, with --vtu PREFIX one PREFIX_mode_NNN.vtu per
// mode (point arrays "Mode Shape X" / "Y" / "Z" and "Magnitude").  One device only; a file without a "Density" entry is refused.
// --buckling K [--buckling-tol T] [--solve-eps E] runs the static solve under the model's own loads, builds
// G = K_g(U) (stan_hip_geometric_stiffness_hex8) and finds the K lowest positive load factors (stan_hip_buckling): a block
// "Buckling load factors:", with --json a "buckling" object, with --vtu PREFIX one PREFIX_buckle_NNN.vtu per factor; the STdb is
// never written.  Refused before anything is computed: several devices, a "Temperature" boundary condition, no supports.
// --modes-shift SIGMA (a model without supports): the modes of K + SIGMA M (stan_hip_matrix_shifted), printed as lambda = mu - SIGMA;
// rho is then the convergence measure of the shifted problem, "shift" in the JSON object.
// --mass consistent (with --modes; default lumped, the path above) runs on the consistent mass M_c:
// stan_hip_consistent_mass_hex8 on K's layout and stan_hip_modes_pencil, under --modes-shift on stan_hip_matrix_axpy(K, SIGMA, M_c); the
// block "Natural frequencies:" names the mass and the "modes" object carries "mass": "consistent".
// --transient --dt DT --steps N [--newmark B,G] [--rayleigh A,B] [--load-curve t0,g0,t1,g1,...] [--probe-node ID] [--solve-eps E]
//  integrates M a + C v + K u = g(t) F from rest by stan_hip_transient INSTEAD of the static solve and never
// writes the STdb: F is the model's own load (PointLoad, distributed and thermal loads), g = 1 without a curve (a step load), the
// supports homogeneous (a non-zero "Displacement" is refused); a block "Transient:", with --json a "transient" object, with
// --vtu PREFIX [--vtu-every K] PREFIX_step_NNNN.vtu every K steps (point arrays "Displacement", "Velocity", "Acceleration" X / Y / Z).
// One device only; a file without a "Density" entry is refused.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/stan_hip.h"
#include "../../include/stan_host.h"
#include "model.h"
#include "solver_functions.h"

using namespace stan;
using clk = std::chrono::steady_clock;
static double secs(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

// fn(i0, i1) over [0, n) on the host threads of libstan_host (STAN_HOST_THREADS)
template <typename F>
static void parallel_ranges(size_t n, F fn) {
    const size_t nt = (size_t)HostThreads();
    if (nt <= 1 || n < 4096) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back([=] { fn(n * t / nt, n * (t + 1) / nt); });
    for (std::thread &x : th) x.join();
}

static int fail(const char *what, const std::string &msg) {
    fprintf(stderr, "\n  ERROR in %s: %s\n", what, msg.c_str());
    return 1;
}

int main(int argc, char **argv) {
    std::string path;
    int device = 0, precision = STAN_PREC_FP64, placement_tries = 16;
    bool merit_stop = true, packed = false, json = false, object_results = false, p2p = false;
    std::vector<int> devices;
    std::string vtu_prefix, vtu_results;
    bool vtu = false, vtu_cells = false, reactions = false;
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
    // "a,b,c" -> doubles; false when an item is not a number
    auto number_list = [](const char *text, std::vector<double> *out) {
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
    };
    std::vector<double> list;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) {
            devices.clear();
            for (int d = 0, n = atoi(argv[++i]); d < n; d++) devices.push_back(d);
        } else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {
            devices.clear();
            for (const char *p = argv[++i]; *p;) {
                devices.push_back(atoi(p));
                while (*p && *p != ',') p++;
                if (*p == ',') p++;
            }
        }
        else if (!strcmp(argv[i], "--placement-tries") && i + 1 < argc) placement_tries = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--mixed")) precision = STAN_PREC_MIXED;
        else if (!strcmp(argv[i], "--fixed48")) precision = STAN_PREC_FIXED48;
        else if (!strcmp(argv[i], "--no-merit-stop")) merit_stop = false;
        else if (!strcmp(argv[i], "--packed")) packed = true;
        else if (!strcmp(argv[i], "--json")) json = true;
        else if (!strcmp(argv[i], "--object-results")) object_results = true;
        else if (!strcmp(argv[i], "--p2p")) p2p = true;
        else if (!strcmp(argv[i], "--vtu") && i + 1 < argc) { vtu = true; vtu_prefix = argv[++i]; }
        else if (!strcmp(argv[i], "--vtu-results") && i + 1 < argc) vtu_results = argv[++i];
        else if (!strcmp(argv[i], "--vtu-cells")) vtu_cells = true;
        else if (!strcmp(argv[i], "--reactions")) reactions = true;
        else if (!strcmp(argv[i], "--modes") && i + 1 < argc) modes = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--modes-tol") && i + 1 < argc) modes_tol = atof(argv[++i]);
        else if (!strcmp(argv[i], "--modes-shift") && i + 1 < argc) modes_shift = atof(argv[++i]);
        else if (!strcmp(argv[i], "--mass") && i + 1 < argc) mass_kind = argv[++i];
        else if (!strcmp(argv[i], "--transient")) transient = true;
        else if (!strcmp(argv[i], "--dt") && i + 1 < argc) { transient_arg = true; run.dt = atof(argv[++i]); }
        else if (!strcmp(argv[i], "--steps") && i + 1 < argc) { transient_arg = true; run.n_steps = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--buckling") && i + 1 < argc) { buckling_arg = true; buckling = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--buckling-tol") && i + 1 < argc) { buckling_arg = true; buckling_tol = atof(argv[++i]); }
        else if (!strcmp(argv[i], "--solve-eps") && i + 1 < argc) { have_solve_eps = true; solve_eps = run.solve_eps = atof(argv[++i]); }
        else if (!strcmp(argv[i], "--probe-node") && i + 1 < argc) { transient_arg = have_probe = true; probe_node = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--vtu-every") && i + 1 < argc) { transient_arg = true; vtu_every = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--newmark") && i + 1 < argc) {
            transient_arg = true;
            if (number_list(argv[++i], &list) && list.size() == 2) { run.beta_N = list[0]; run.gamma = list[1]; }
            else bad_list = true;
        } else if (!strcmp(argv[i], "--rayleigh") && i + 1 < argc) {
            transient_arg = true;
            if (number_list(argv[++i], &list) && list.size() == 2) { run.alpha_R = list[0]; run.beta_R = list[1]; }
            else bad_list = true;
        } else if (!strcmp(argv[i], "--load-curve") && i + 1 < argc) {
            transient_arg = true;
            if (number_list(argv[++i], &list) && !list.empty() && list.size() % 2 == 0)
                for (size_t k = 0; k < list.size(); k += 2) { run.curve_t.push_back(list[k]); run.curve_g.push_back(list[k + 1]); }
            else bad_list = true;
        }
        else path = argv[i];
    }
    if (path.empty()) {  // Path = path[0] -> IndexOutOfRangeException in the reference
        fprintf(stderr, "usage: stan_solver [--device N | --gpus N | --devices a,b,..] [--p2p] [--mixed|--fixed48] "
                        "[--no-merit-stop] [--packed] [--object-results] [--json] [--vtu PREFIX [--vtu-results \"name,..\"] [--vtu-cells]] [--reactions] [--modes K [--modes-tol T] [--modes-shift SIGMA] [--mass lumped|consistent]] "
                        "[--buckling K [--buckling-tol T] [--solve-eps E] [--vtu PREFIX]] "
                        "[--transient --dt DT --steps N [--newmark B,G] [--rayleigh A,B] [--load-curve t0,g0,t1,g1,...] [--probe-node ID] "
                        "[--solve-eps E] [--vtu PREFIX [--vtu-every K]]] <model.STdb>\n");
        return 2;
    }
    // --vtu is checked before anything is read: the input file is overwritten by a run that gets further
    std::vector<int32_t> vtu_sel;
    if (vtu) {
        std::string why;
        if (devices.size() > 1) {
            fprintf(stderr, "stan_solver: --vtu works on one device: the result scalars average over all elements at a node, "
                            "and a multi-device handle holds them in chunks (drop --gpus/--devices, or export in a second run)\n");
            return 2;
        }
        if (!SolverFunctions::ParseScalarNames(vtu_results, &vtu_sel, &why)) {
            fprintf(stderr, "stan_solver: --vtu-results: %s\n", why.c_str());
            return 2;
        }
    }
    if (reactions && devices.size() > 1) {
        fprintf(stderr, "stan_solver: --reactions works on one device: the internal forces add up all elements at a node, and a "
                        "multi-device handle holds them in chunks (drop --gpus/--devices)\n");
        return 2;
    }
    if (modes < 0 || modes_tol < 0 || (modes == 0 && modes_tol != 0)) {
        fprintf(stderr, "stan_solver: --modes K needs K > 0, --modes-tol T needs T >= 0 and --modes\n");
        return 2;
    }
    if (modes && devices.size() > 1) {
        fprintf(stderr, "stan_solver: --modes works on one device: the lumped mass adds up all elements at a node, and the block "
                        "solves run on a single-rank context (drop --gpus/--devices)\n");
        return 2;
    }
    if (modes_shift != 0 && (!modes || !(modes_shift > 0) || !std::isfinite(modes_shift))) {
        fprintf(stderr, "stan_solver: --modes-shift SIGMA needs SIGMA > 0 and --modes\n");
        return 2;
    }
    if (mass_kind != "lumped" && mass_kind != "consistent") {
        fprintf(stderr, "stan_solver: --mass takes lumped or consistent, not \"%s\"\n", mass_kind.c_str());
        return 2;
    }
    if (mass_kind == "consistent" && !modes) {
        fprintf(stderr, "stan_solver: --mass consistent needs --modes\n");
        return 2;
    }
    // --buckling, checked before anything is read as well
    if (buckling_arg) {
        const char *why = nullptr;
        if (buckling <= 0 || !(buckling_tol >= 0)) why = "--buckling K needs K > 0, --buckling-tol T needs T >= 0 and --buckling";
        else if (modes || transient) why = "--buckling, --modes and --transient are three analyses: one per run";
        else if (!(solve_eps >= 0)) why = "--solve-eps E needs E >= 0";
        else if (devices.size() > 1)
            why = "--buckling works on one device: the geometric stiffness adds up all elements at a node, and the block solves run "
                  "on a single-rank context (drop --gpus/--devices)";
        if (why) {
            fprintf(stderr, "stan_solver: %s\n", why);
            return 2;
        }
    }
    if (have_solve_eps && !buckling) transient_arg = true;
    // --transient, checked before anything is read as well
    if (!transient && transient_arg) {
        fprintf(stderr, "stan_solver: --dt, --steps, --newmark, --rayleigh, --load-curve, --probe-node, --solve-eps and --vtu-every belong to --transient\n");
        return 2;
    }
    if (transient) {
        const char *why = nullptr;
        if (modes) why = "--transient and --modes are two analyses: one per run";
        else if (bad_list) why = "--newmark B,G and --rayleigh A,B take two numbers, --load-curve t0,g0,t1,g1,... an even count of them";
        else if (!(run.dt > 0) || !std::isfinite(run.dt)) why = "--transient needs --dt DT with DT > 0";
        else if (run.n_steps < 0) why = "--steps N needs N >= 0";
        else if (!(run.solve_eps >= 0)) why = "--solve-eps E needs E >= 0";
        else if (vtu_every < 1) why = "--vtu-every K needs K >= 1";
        else if (!(run.alpha_R >= 0) || !(run.beta_R >= 0)) why = "--rayleigh A,B needs A >= 0 and B >= 0";
        else if (!(run.beta_N == 0 && run.gamma == 0) &&
                 (!(run.gamma >= 0.5) || !(run.beta_N >= (run.gamma + 0.5) * (run.gamma + 0.5) / 4)))
            why = "--newmark B,G needs G >= 1/2 and B >= (G + 1/2)^2 / 4 (unconditional stability)";
        for (size_t k = 0; !why && k < run.curve_t.size(); k++)
            if (!std::isfinite(run.curve_t[k]) || !std::isfinite(run.curve_g[k]) || (k > 0 && run.curve_t[k] < run.curve_t[k - 1]))
                why = "--load-curve needs finite values and times that do not descend";
        if (!why && devices.size() > 1)
            why = "--transient works on one device: the lumped mass adds up all elements at a node, and the shifted matrix and its "
                  "solves run on a single-rank context (drop --gpus/--devices)";
        if (why) {
            fprintf(stderr, "stan_solver: %s\n", why);
            return 2;
        }
        run.snap_every = vtu ? vtu_every : 0;
    }
    SolverOptions opt;
    opt.device = device; opt.devices = devices; opt.precision = precision; opt.placement_tries = placement_tries; opt.merit_stop = merit_stop; opt.profile = json;
    opt.p2p = p2p;
    SolverFunctions Functions(opt);  // Solver.cs:16
    Functions.Welcome_Messsage();
    Functions.Prewarm();             // the device context comes up while the file is read

    // host phase times of this run (--json): the path around the GPU hot path is host work, and at scale most
    // of the wall clock
    double t_read = 0, t_dof = 0, t_bc = 0, t_disp = 0, t_recover = 0, t_store = 0, t_write = 0, t_hot = 0, t_scalars = 0, t_vtu = 0, t_react = 0;
    const auto t_wall = clk::now();
    printf("   Reading input file: ");  // Solver.cs:23-41
    fflush(stdout);
    Database DB;
    std::string err;
    auto t0 = clk::now();
    if (!Functions.ProtoDeserialize(path, &DB, &err)) return fail("ProtoDeserialize", err);
    t_read = secs(t0);
    printf("     Done\n");
    // --modes is checked before anything is computed or written: it needs the densities, and the static analysis it replaces
    if (modes && !HasDensity(DB)) {
        fprintf(stderr, "stan_solver: --modes needs a \"Density\" boundary condition (material IDs, component 0 = rho): the file has none\n");
        return 2;
    }
    if (modes && DB.AnalysisLib.Type != "Linear_Statics") {
        fprintf(stderr, "stan_solver: --modes works on a Linear_Statics file\n");
        return 2;
    }
    if (transient && !HasDensity(DB)) {   // the same, for the same reason
        fprintf(stderr, "stan_solver: --transient needs a \"Density\" boundary condition (material IDs, component 0 = rho): the file has none\n");
        return 2;
    }
    if (transient && DB.AnalysisLib.Type != "Linear_Statics") {
        fprintf(stderr, "stan_solver: --transient works on a Linear_Statics file\n");
        return 2;
    }

    if (buckling && DB.AnalysisLib.Type != "Linear_Statics") {
        fprintf(stderr, "stan_solver: --buckling works on a Linear_Statics file\n");
        return 2;
    }
    if (buckling)   // the stress state is sigma = D B u: a thermal part is out of scope
        for (const auto &kv : DB.BCLib.Items())
            if (kv.second.Type == "Temperature") {
                fprintf(stderr, "stan_solver: --buckling takes mechanical loads only: the file has a \"Temperature\" boundary condition "
                                "(thermal pre-stress is out of scope)\n");
                return 2;
            }

    printf("   DoF ordering: ");  // Solver.cs:44-47
    fflush(stdout);
    t0 = clk::now();
    if (int rc = DB.AssignDOF()) return fail("AssignDOF", "code " + std::to_string(rc) +
                                             " (disconnected mesh or unknown node ID)");
    t_dof = secs(t0);
    printf("           Done\n");
    fputs(DB.Database_Summary().c_str(), stdout);  // Solver.cs:50

    if (DB.AnalysisLib.Type == "Linear_Statics") try {  // Solver.cs:53-57, SolverLinearStatics :72-217
        const auto t_total = clk::now();
        const char *separator = "  ========================================================== ";
        printf("\n%s\n        LINEAR STATIC ANALYSIS \n%s\n", separator, separator);

        // Fix_DOF / nDOF_reduction / F (Solver.cs:104-152)
        std::vector<int32_t> nDOF_reduction;
        std::vector<double> F;
        int64_t n_fixed = 0;
        t0 = clk::now();
        if (BuildReductionAndLoads(DB, &nDOF_reduction, &n_fixed, &F, &err)) return fail("boundary conditions", err);
        const bool dist_loads = HasDistributedLoads(DB);
        if (dist_loads && devices.size() > 1)
            return fail("boundary conditions", "Pressure / BodyForce / Displacement work on one device: the load vector adds up all "
                                               "elements at a node, and a multi-device handle holds them in chunks (drop --gpus/--devices)");
        const bool thermal = HasThermalLoads(DB);
        if (thermal && devices.size() > 1)
            return fail("boundary conditions", "Temperature / ThermalExpansion work on one device: the thermal load adds up all "
                                               "elements at a node, and a multi-device handle holds them in chunks (drop --gpus/--devices)");
        t_bc = secs(t0);
        const int64_t n_nodes = (int64_t)DB.NodeLib.Count();
        if (buckling && n_fixed == 0) {   // before anything is assembled: K of a model without supports is not positive definite
            fprintf(stderr, "stan_solver: --buckling needs a supported model: the file fixes no DOF\n");
            return 2;
        }

        t0 = clk::now();
        SparseMatrixHandle K;
        Functions.ParallelAssembly_K(DB, nDOF_reduction, 1, "Initial", &K);  // Solver.cs:157
        stan_matrix_info minfo;
        stan_hip_matrix_info(K.K, &minfo);

        if (modes) {   // the modal analysis instead of the static solve: nothing of it reaches the STdb
            MassDensity md;
            if (BuildDensity(DB, K.flat, &md, &err)) return fail("boundary conditions", err);
            std::vector<double> lambda, phi, rho;
            stan_mass_sums msum{};
            stan_modes_report rep{};
            const bool consistent = mass_kind == "consistent";
            if (consistent) Functions.ModesConsistent(K, nDOF_reduction, md, modes, modes_tol, &lambda, &phi, &rho, &msum, &rep, modes_shift);
            else Functions.Modes(K, nDOF_reduction, md, modes, modes_tol, &lambda, &phi, &rho, &msum, &rep, modes_shift);
            const double two_pi = 6.283185307179586476925;
            // (a rigid-body mode of a shifted run has lambda = 0 up to the tolerance, on either side: its frequency is 0)
            auto hz = [&](double l) { return l > 0 ? std::sqrt(l) / two_pi : 0.0; };
            printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
            printf("   Natural frequencies: (%sblock %d, %d outer steps, %lld CG iterations, %s)\n", consistent ? "consistent mass, " : "",
                   rep.block, rep.outer, (long long)rep.cg_iterations, rep.converged ? "converged" : "NOT converged");
            if (modes_shift > 0)
                printf("     shift %.8e: the modes of K + shift M, lambda = mu - shift; rho is the convergence measure of the shifted\n"
                       "     problem, relative to mu\n", modes_shift);
            printf("     mode            lambda    frequency [Hz]           rho\n");
            for (int j = 0; j < modes; j++)
                printf("     %4d  %16.8e  %16.8e  %12.3e\n", j + 1, lambda[(size_t)j], hz(lambda[(size_t)j]), rho[(size_t)j]);
            if (vtu) {
                const size_t N = (size_t)minfo.n_reduced;
                std::vector<double> shape((size_t)n_nodes * 3);
                for (int j = 0; j < modes; j++) {
                    const std::vector<double> full = Functions.Include_BC_DOF(
                        std::vector<double>(phi.begin() + (ptrdiff_t)((size_t)j * N), phi.begin() + (ptrdiff_t)((size_t)(j + 1) * N)), nDOF_reduction);
                    for (size_t k = 0; k < shape.size(); k++) shape[k] = full[(size_t)K.flat.node_dof[k]];
                    Functions.Export_Mode_Vtu(K, shape, vtu_prefix, j + 1);
                }
                printf("   VTU export: %s_mode_001.vtu ... %s_mode_%03d.vtu\n", vtu_prefix.c_str(), vtu_prefix.c_str(), modes);
            }
            printf("\n%s\n  Total CPU time: %.2f s\n%s\n", separator, secs(t_total), separator);
            if (json) {   // %.17g: the doubles round-trip
                printf("{\"n_gpus\": 1, \"n_dof\": %d, \"n_reduced\": %lld, \"t_wall_s\": %.3f, \"modes\": {\"n_modes\": %d, \"block\": %d, "
                       "\"outer\": %d, \"converged\": %d, \"cg_iterations\": %lld, \"total_mass\": %.17g",
                       DB.nDOF, (long long)minfo.n_reduced, secs(t_wall), modes, rep.block, rep.outer, rep.converged,
                       (long long)rep.cg_iterations, msum.total_mass);
                if (consistent) printf(", \"mass\": \"consistent\"");
                if (modes_shift > 0) printf(", \"shift\": %.17g", modes_shift);   // rho: of the shifted problem
                for (int pass = 0; pass < 3; pass++) {
                    printf(", \"%s\": [", pass == 0 ? "lambda" : pass == 1 ? "frequency_hz" : "rho");
                    for (int j = 0; j < modes; j++)
                        printf("%s%.17g", j ? ", " : "", pass == 0 ? lambda[(size_t)j] : pass == 1 ? hz(lambda[(size_t)j]) : rho[(size_t)j]);
                    printf("]");
                }
                printf("}}\n");
            }
            return 0;
        }

        // thermal loads, in front of the distributed loads: their F - f_int(u0) then holds this load too
        ThermalLoads thermal_bc;
        stan_thermal_sums tsum{};
        std::vector<double> thermal_full;   // the thermal load over all DOFs: the supports exert f_int - this
        double t_thermal = 0;
        if (thermal) {
            const auto tt = clk::now();
            if (BuildThermalLoads(DB, K.flat, &thermal_bc, &err)) return fail("boundary conditions", err);
            Functions.Thermal_Load(K, nDOF_reduction, thermal_bc, &F, &thermal_full, &tsum);
            t_thermal = secs(tt);
            printf("   Thermal loads:\n");
            printf("     Total:              X %14.6e   Y %14.6e   Z %14.6e\n", tsum.load_sum[0], tsum.load_sum[1], tsum.load_sum[2]);
            printf("     On free DOFs:       X %14.6e   Y %14.6e   Z %14.6e\n", tsum.free_sum[0], tsum.free_sum[1], tsum.free_sum[2]);
            printf("     Heated volume: %.6e   mean dT: %.6e\n", tsum.volume, tsum.volume != 0 ? tsum.dT_integral / tsum.volume : 0.0);
        }

        // distributed loads: F becomes the whole external load, F_solve the right-hand side (F - f_int(u0) on the free DOFs)
        DistributedLoads dl;
        stan_load_sums lsum{};
        std::vector<double> F_rhs;
        double t_loads = 0;
        if (dist_loads) {
            const auto tl = clk::now();
            if (BuildDistributedLoads(DB, K.flat, nDOF_reduction, &dl, &err)) return fail("boundary conditions", err);
            if (dl.mat_body.empty() && dl.face_elem.empty() && dl.disp0.empty()) {   // such BCs, but nothing in them (a Pressure
                F_rhs = F;                                                           // set that forms no boundary face, an empty
                lsum.n_fixed = n_fixed;                                              // BodyForce): the block with zeros
            } else Functions.Load_Vector(K, nDOF_reduction, dl, &F, &F_rhs, &lsum);
            t_loads = secs(tl);
            printf("   Distributed loads:\n");
            printf("     Total:              X %14.6e   Y %14.6e   Z %14.6e\n", lsum.load_sum[0], lsum.load_sum[1], lsum.load_sum[2]);
            printf("     On free DOFs:       X %14.6e   Y %14.6e   Z %14.6e\n", lsum.free_sum[0], lsum.free_sum[1], lsum.free_sum[2]);
            printf("     Loaded volume: %.6e   loaded area: %.6e (%lld faces)   prescribed DOFs: %lld\n", lsum.volume, lsum.area,
                   (long long)lsum.n_faces, (long long)dl.n_prescribed);
        }
        const std::vector<double> &F_solve = dist_loads ? F_rhs : F;

        if (transient) {   // the time integration instead of the static solve: nothing of it reaches the STdb
            for (double x : dl.disp0)
                if (x != 0.0) {
                    fprintf(stderr, "stan_solver: --transient takes homogeneous supports only: the file prescribes a non-zero "
                                    "\"Displacement\"\n");
                    return 2;
                }
            // the probe: the free DOFs of one node, by its ID
            int probe_dir[3] = {0, 0, 0};
            if (have_probe) {
                int64_t node = -1;
                for (int64_t n = 0; n < n_nodes && node < 0; n++)
                    if (DB.NodeLib.Items()[(size_t)n].first == probe_node) node = n;
                if (node < 0) {
                    fprintf(stderr, "stan_solver: --probe-node %d: the file has no such node\n", probe_node);
                    return 2;
                }
                for (int c = 0; c < 3; c++) {
                    const int32_t d = K.flat.node_dof[(size_t)(3 * node + c)];
                    if (nDOF_reduction[(size_t)d] == -1) continue;
                    probe_dir[run.probe_dof.size()] = c;
                    run.probe_dof.push_back(d - nDOF_reduction[(size_t)d]);
                }
            }
            MassDensity md;
            if (BuildDensity(DB, K.flat, &md, &err)) return fail("boundary conditions", err);
            std::vector<double> probe_u, snaps, energy;
            stan_mass_sums msum{};
            stan_transient_report rep{};
            Functions.Transient(K, nDOF_reduction, md, F_solve, run, &probe_u, &snaps, &energy, &msum, &rep);
            const size_t np = run.probe_dof.size(), N = (size_t)minfo.n_reduced;
            const double bN = run.beta_N == 0 && run.gamma == 0 ? 0.25 : run.beta_N, gm = run.beta_N == 0 && run.gamma == 0 ? 0.5 : run.gamma;
            const double mean_its = rep.steps > 0 ? (double)rep.cg_iterations / rep.steps : 0.0;
            printf("   Total mass: %.6e   volume: %.6e\n", msum.total_mass, msum.volume);
            printf("   Transient: (%d steps of dt %.6e, Newmark beta %g gamma %g, Rayleigh alpha %g beta %g)\n", rep.steps, run.dt, bN, gm,
                   run.alpha_R, run.beta_R);
            printf("     sigma of K + sigma M: %.8e\n", rep.sigma);
            printf("     CG iterations per step: min %d  mean %.1f  max %d\n", rep.cg_min_iterations, mean_its, rep.cg_max_iterations);
            if (np) {
                printf("     Probe node %d:\n       step                 t", probe_node);
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
            if (vtu) {
                int last = 0;
                for (int s = 0; s <= run.n_steps; s += vtu_every) {
                    Functions.Export_Step_Vtu(K, nDOF_reduction, &snaps[(size_t)(s / vtu_every) * 3 * N], N, vtu_prefix, s);
                    last = s;
                }
                printf("   VTU export: %s_step_0000.vtu ... %s_step_%04d.vtu\n", vtu_prefix.c_str(), vtu_prefix.c_str(), last);
            }
            printf("\n%s\n  Total CPU time: %.2f s\n%s\n", separator, secs(t_total), separator);
            if (json) {   // %.17g: the doubles round-trip
                printf("{\"n_gpus\": 1, \"n_dof\": %d, \"n_reduced\": %lld, \"t_wall_s\": %.3f, \"transient\": {\"steps\": %d, \"dt\": %.17g, "
                       "\"beta_N\": %.17g, \"gamma\": %.17g, \"alpha_R\": %.17g, \"beta_R\": %.17g, \"sigma\": %.17g, \"cg_iterations\": %lld, "
                       "\"cg_min_iterations\": %d, \"cg_max_iterations\": %d, \"cg_worst_type\": %d, \"total_mass\": %.17g, "
                       "\"energy_final\": [%.17g, %.17g, %.17g]",
                       DB.nDOF, (long long)minfo.n_reduced, secs(t_wall), rep.steps, run.dt, bN, gm, run.alpha_R, run.beta_R, rep.sigma,
                       (long long)rep.cg_iterations, rep.cg_min_iterations, rep.cg_max_iterations, rep.cg_worst_type, msum.total_mass,
                       ef[0], ef[1], ef[2]);
                if (np) {
                    printf(", \"probe_node\": %d, \"probe_direction\": [", probe_node);
                    for (size_t q = 0; q < np; q++) printf("%s%d", q ? ", " : "", probe_dir[q]);
                    printf("], \"probe_u\": [");
                    for (int s = 0; s <= run.n_steps; s++) {
                        printf("%s[", s ? ", " : "");
                        for (size_t q = 0; q < np; q++) printf("%s%.17g", q ? ", " : "", probe_u[(size_t)s * np + q]);
                        printf("]");
                    }
                    printf("]");
                }
                printf("}}\n");
            }
            return 0;
        }

        if (buckling) {   // the static solve under the model's own loads, G from that U, then the load factors: nothing reaches the STdb
            const std::vector<double> Ub = Functions.LinearSolver_CG(K, F_solve, DB.AnalysisLib);
            printf("   CG iterations: %d, scaled relative residual %.3e\n", Functions.last_iterations, Functions.last_rel_residual);
            const std::vector<double> Ubf = Functions.Include_BC_DOF(Ub, nDOF_reduction);
            std::vector<double> dispb((size_t)n_nodes * 3);
            for (size_t k = 0; k < dispb.size(); k++) dispb[k] = Ubf[(size_t)K.flat.node_dof[k]];
            if (dist_loads && !dl.disp0.empty())   // the solved field is U on top of the prescribed u0
                for (size_t k = 0; k < dispb.size(); k++) dispb[k] += dl.disp0[k];
            std::vector<double> factor, phi, rho;
            stan_buckling_report rep{};
            Functions.Buckling(K, nDOF_reduction, dispb, buckling, buckling_tol, solve_eps, &factor, &phi, &rho, &rep);
            const int found = rep.n_positive < buckling ? rep.n_positive : buckling;
            printf("   Buckling load factors: (block %d, %d outer steps, %lld CG iterations, %s)\n", rep.block, rep.outer,
                   (long long)rep.cg_iterations, rep.converged ? "converged" : "NOT converged");
            printf("     mode            factor           rho\n");
            for (int j = 0; j < found; j++) printf("     %4d  %16.8e  %12.3e\n", j + 1, factor[(size_t)j], rho[(size_t)j]);
            if (found < buckling) printf("     only %d positive factors in the block of %d\n", rep.n_positive, rep.block);
            if (rep.lowest_negative_factor != 0)
                printf("     lowest negative factor (the load reversed): %.8e\n", rep.lowest_negative_factor);
            if (vtu) {
                const size_t N = (size_t)minfo.n_reduced;
                std::vector<double> shape((size_t)n_nodes * 3);
                for (int j = 0; j < found; j++) {
                    const std::vector<double> full = Functions.Include_BC_DOF(
                        std::vector<double>(phi.begin() + (ptrdiff_t)((size_t)j * N), phi.begin() + (ptrdiff_t)((size_t)(j + 1) * N)), nDOF_reduction);
                    for (size_t k = 0; k < shape.size(); k++) shape[k] = full[(size_t)K.flat.node_dof[k]];
                    Functions.Export_Buckle_Vtu(K, shape, vtu_prefix, j + 1);
                }
                if (found > 0) printf("   VTU export: %s_buckle_001.vtu ... %s_buckle_%03d.vtu\n", vtu_prefix.c_str(), vtu_prefix.c_str(), found);
            }
            printf("\n%s\n  Total CPU time: %.2f s\n%s\n", separator, secs(t_total), separator);
            if (json) {   // %.17g: the doubles round-trip
                printf("{\"n_gpus\": 1, \"n_dof\": %d, \"n_reduced\": %lld, \"t_wall_s\": %.3f, \"buckling\": {\"n_modes\": %d, \"block\": %d, "
                       "\"outer\": %d, \"converged\": %d, \"n_positive\": %d, \"cg_iterations\": %lld, \"static_cg_iterations\": %d, "
                       "\"lowest_negative_factor\": %.17g",
                       DB.nDOF, (long long)minfo.n_reduced, secs(t_wall), buckling, rep.block, rep.outer, rep.converged, rep.n_positive,
                       (long long)rep.cg_iterations, Functions.last_iterations, rep.lowest_negative_factor);
                for (int pass = 0; pass < 2; pass++) {
                    printf(", \"%s\": [", pass == 0 ? "factor" : "rho");
                    for (int j = 0; j < found; j++) printf("%s%.17g", j ? ", " : "", pass == 0 ? factor[(size_t)j] : rho[(size_t)j]);
                    printf("]");
                }
                printf("}}\n");
            }
            return 0;
        }

        std::vector<double> U((size_t)(DB.nDOF - n_fixed), 0.0);
        const std::string &ls = DB.AnalysisLib.LinSolver;
        if (ls == "CG") {  // Solver.cs:162
            U = Functions.LinearSolver_CG(K, F_solve, DB.AnalysisLib);
            printf("   CG iterations: %d, scaled relative residual %.3e\n", Functions.last_iterations,
                   Functions.last_rel_residual);
        } else if (ls == "Cholesky") {  // Solver.cs:163: CPU fallback, outside the GPU hot path (direct.cpp)
            if (devices.size() > 1) return fail("solver selection", "the direct solvers run on one device's export of K: drop --gpus/--devices");
            U = Functions.LinearSolver_Cholesky(K, F_solve);
        } else if (ls == "LU") {        // Solver.cs:164
            if (devices.size() > 1) return fail("solver selection", "the direct solvers run on one device's export of K: drop --gpus/--devices");
            U = Functions.LinearSolver_LU(K, F_solve);
        }  // any other string: the reference leaves U = 0 (Solver.cs:160-164)
        t_hot = secs(t0);   // flatten + context + upload + assembly + solve + download

        // U = Include_BC_DOF(U, nDOF_reduction); node.dU_buffer[d] = U[DOF[d]] (Solver.cs:168-178)
        t0 = clk::now();
        const std::vector<double> Ufull = Functions.Include_BC_DOF(U, nDOF_reduction);
        std::vector<double> disp((size_t)n_nodes * 3);
        parallel_ranges(disp.size(), [&](size_t a, size_t b) {
            for (size_t k = a; k < b; k++) disp[k] = Ufull[(size_t)K.flat.node_dof[k]];
        });
        if (!dl.disp0.empty())   // the supports' own displacement, before recovery, reactions, .vtu and the export
            for (size_t k = 0; k < disp.size(); k++)
                if (nDOF_reduction[(size_t)K.flat.node_dof[k]] == -1) disp[k] = dl.disp0[k];
        t_disp = secs(t0);

        printf("   Stress recovery: ");  // Solver.cs:183
        fflush(stdout);
        t0 = clk::now();
        std::vector<double> strain, stress;
        // the flat-array export takes the element results from the device chunk by chunk while it encodes (the
        // download overlaps the encoding and the file writes); --object-results needs them as whole host arrays
        if (object_results) Functions.Recovery_Stress(K, disp, &strain, &stress);
        else Functions.Recovery_Stress_Keep(K, disp);
        if (thermal) Functions.Thermal_Stress(K, thermal_bc, object_results ? &stress : nullptr);   // before .vtu, scalars and export
        t_recover = secs(t0);
        printf("            Done\n");
        stan_profile pr{};
        if (json) stan_hip_get_profile(K.ctx, &pr);
        // --reactions: f_int(U) element by element, never through K; the displacement vector carries 0 at the fixed DOFs
        stan_equilibrium eq{};
        std::vector<double> reaction;
        if (reactions) {
            t0 = clk::now();
            Functions.Equilibrium(K, disp, F, nDOF_reduction, nullptr, vtu || thermal ? &reaction : nullptr, &eq);
            if (thermal)   // the supports exert f_int - l at the fixed DOFs: the arrays, and the sums by direction in node order
                for (int64_t n = 0; n < n_nodes; n++)
                    for (int c = 0; c < 3; c++) {
                        const size_t d = (size_t)K.flat.node_dof[(size_t)(3 * n + c)];
                        if (nDOF_reduction[d] != -1) continue;
                        reaction[d] -= thermal_full[d];
                        eq.reaction_sum[c] -= thermal_full[d];
                    }
            t_react = secs(t0);
            int64_t node = -1;
            for (int64_t n = 0; n < n_nodes && eq.residual_max_dof >= 0; n++)
                if (K.flat.node_dof[(size_t)(3 * n)] == (int32_t)(eq.residual_max_dof - eq.residual_max_dof % 3)) { node = n; break; }
            printf("   Equilibrium check (internal forces of the solved displacements):\n");
            printf("     Support reactions:  X %14.6e   Y %14.6e   Z %14.6e\n", eq.reaction_sum[0], eq.reaction_sum[1], eq.reaction_sum[2]);
            printf("     Applied load:       X %14.6e   Y %14.6e   Z %14.6e\n", eq.load_sum[0], eq.load_sum[1], eq.load_sum[2]);
            printf("     Out of balance:     |F - f_int| = %.3e, %.3e of |F|\n", eq.residual_norm2,
                   eq.load_norm2 > 0 ? eq.residual_norm2 / eq.load_norm2 : 0.0);
            if (node >= 0)
                printf("     Largest:            %.3e at node %d, direction %c\n", eq.residual_max, DB.NodeLib.Items()[(size_t)node].first,
                       "XYZ"[eq.residual_max_dof % 3]);
        }
        // the .vtu takes its scalars from the results while they are still on the device (the STdb export frees them)
        if (vtu) {
            Functions.Export_Vtu(K, disp, object_results ? &strain : nullptr, object_results ? &stress : nullptr, vtu_prefix,
                                 vtu_sel, vtu_cells, &t_scalars, &t_vtu, reactions ? &reaction : nullptr);
            printf("   VTU export: %s_001.vtu\n", vtu_prefix.c_str());
        }
        // Solver.cs:81-90 (initialise step 0/1), :203-210 (update), Main :56
        t0 = clk::now();
        // Solver.cs:81-90, 203-210: every node / element object is initialised and updated with the results, then
        // ExportOutput serialises the objects.  By default the writer takes the results from the flat arrays
        // instead (Database::ResultView: the same bytes without 13 million small heap objects);
        // --object-results walks the reference's object path (tests/test_gpu_parity.py compares the files).
        if (!object_results) {
            DB.results.disp = disp.data();
            stan_results *res = K.results;
            DB.results.fetch = [res](size_t e0, size_t e1, const double **sn, const double **ss) {
                return stan_hip_results_map(res, (int64_t)e0, (int64_t)e1, sn, ss) == STAN_OK;
            };
        }
        auto &nodes = DB.NodeLib.Items();
        if (object_results) parallel_ranges(nodes.size(), [&](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) {
                Node &n = nodes[i].second;
                n.Initialize_StepZero();
                n.Initialize_NewDisp(1);
                for (int d = 0; d < 3; d++) n.dU_buffer[d] = disp[3 * i + (size_t)d];
                n.Update_Displacement(1);
            }
        });
        auto &elems = DB.ElemLib.Items();
        if (object_results) parallel_ranges(elems.size(), [&](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) {
                Element &e = elems[i].second;
                e.Initialize_StepZero();
                e.Initialize_Increment(1);
                memcpy(e.Strain[1].M.data(), &strain[48 * i], 48 * sizeof(double));
                memcpy(e.Stress[1].M.data(), &stress[48 * i], 48 * sizeof(double));
            }
        });
        t_store = secs(t0);
        printf("\n%s\n  Total CPU time: %.2f s\n%s\n", separator, secs(t_total), separator);
        DB.AnalysisLib.Result_StepNo = 1;
        // ExportOutput: overwrite the input path (Solver.cs:454-462)
        t0 = clk::now();
        if (!Functions.ProtoSerialize(DB, path, packed, &err)) return fail("ExportOutput", err);
        t_write = secs(t0);
        if (json) {  // one machine-readable line per run (metrics/logging), after the export
            const double spmv_ms = pr.spmv_launches ? pr.spmv_ms_total / (double)pr.spmv_launches : 0;
            const double wall = secs(t_wall), dev = (pr.assemble_ms + pr.cg_ms) * 1e-3;
            printf("{\"n_gpus\": %d, \"n_dof\": %d, \"n_reduced\": %lld, \"blocks_3x3\": %lld, \"cg_iterations\": %d, "
                   "\"termination_type\": %d, \"rel_residual\": %.3e, \"t_assembly_s\": %.4f, \"t_cg_s\": %.4f, "
                   "\"spmv_ms\": %.4f, \"spmv_GBs\": %.1f, \"hbm_frac\": %.3f, "
                   "\"host_threads\": %d, \"t_wall_s\": %.3f, \"t_device_assembly_plus_cg_s\": %.4f, "
                   "\"phases_s\": {\"read_parse\": %.3f, \"assign_dof\": %.3f, \"bc_tables\": %.3f, "
                   "\"flatten_upload_assemble_solve\": %.3f, \"displacements\": %.3f, \"stress_recovery\": %.3f, "
                   "\"store_results\": %.3f, \"serialize_write\": %.3f, \"result_scalars\": %.6f, \"write_vtu\": %.6f}",
                   devices.size() > 1 ? (int)devices.size() : 1, DB.nDOF, (long long)minfo.n_reduced, (long long)minfo.n_blocks, Functions.last_iterations,
                   Functions.last_termination_type, Functions.last_rel_residual, Functions.last_assembly_s,
                   Functions.last_cg_s, spmv_ms, spmv_ms > 0 ? pr.spmv_bytes / spmv_ms / 1e6 : 0.0,
                   spmv_ms > 0 ? pr.spmv_bytes / spmv_ms / 1e6 / 8000.0 : 0.0,
                   // (the two .vtu phases to the microsecond: on a small model they take less than the 0.5 ms that %.3f shows as 0)
                   HostThreads(), wall, dev, t_read, t_dof, t_bc, t_hot, t_disp, t_recover, t_store, t_write, t_scalars, t_vtu);
            if (reactions)   // %.17g: the doubles round-trip
                printf(", \"equilibrium\": {\"reaction_sum\": [%.17g, %.17g, %.17g], \"load_sum\": [%.17g, %.17g, %.17g], "
                       "\"fint_sum\": [%.17g, %.17g, %.17g], \"residual_norm2\": %.17g, \"load_norm2\": %.17g, \"residual_max\": %.17g, "
                       "\"residual_max_dof\": %lld, \"n_fixed\": %lld, \"t_s\": %.3f}",
                       eq.reaction_sum[0], eq.reaction_sum[1], eq.reaction_sum[2], eq.load_sum[0], eq.load_sum[1], eq.load_sum[2],
                       eq.fint_sum[0], eq.fint_sum[1], eq.fint_sum[2], eq.residual_norm2, eq.load_norm2, eq.residual_max,
                       (long long)eq.residual_max_dof, (long long)eq.n_fixed, t_react);
            if (dist_loads)
                printf(", \"loads\": {\"load_sum\": [%.17g, %.17g, %.17g], \"free_sum\": [%.17g, %.17g, %.17g], \"volume\": %.17g, "
                       "\"area\": %.17g, \"n_faces\": %lld, \"n_fixed\": %lld, \"n_prescribed\": %lld, \"t_s\": %.3f}",
                       lsum.load_sum[0], lsum.load_sum[1], lsum.load_sum[2], lsum.free_sum[0], lsum.free_sum[1], lsum.free_sum[2],
                       lsum.volume, lsum.area, (long long)lsum.n_faces, (long long)lsum.n_fixed, (long long)dl.n_prescribed, t_loads);
            if (thermal)
                printf(", \"thermal\": {\"load_sum\": [%.17g, %.17g, %.17g], \"free_sum\": [%.17g, %.17g, %.17g], \"volume\": %.17g, "
                       "\"dT_integral\": %.17g, \"mean_dT\": %.17g, \"n_fixed\": %lld, \"t_s\": %.3f}",
                       tsum.load_sum[0], tsum.load_sum[1], tsum.load_sum[2], tsum.free_sum[0], tsum.free_sum[1], tsum.free_sum[2],
                       tsum.volume, tsum.dT_integral, tsum.volume != 0 ? tsum.dT_integral / tsum.volume : 0.0, (long long)tsum.n_fixed,
                       t_thermal);
            printf("}\n");
        }
        return 0;
    } catch (const std::exception &e) {  // the C# lets these escape Main as unhandled exceptions
        return fail("SolverLinearStatics", e.what());
    } else if (DB.AnalysisLib.Type == "Nonlinear_Statics") {
        return fail("analysis type", "Nonlinear_Statics is unreachable from the GUI "
                                     "(MainWindow.xaml.cs:444) and outside the hot path");
    }

    // ExportOutput: overwrite the input path (Solver.cs:454-462) -- also when the analysis type is not one
    // this driver solves (Main writes the file back regardless)
    if (!Functions.ProtoSerialize(DB, path, packed, &err)) return fail("ExportOutput", err);
    return 0;
}
