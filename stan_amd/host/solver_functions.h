// solver_functions.h -- C++ mirror of STAN_Solver.SolverFunctions for the linear-static path
// (SolverFunctions.cs): same method names, argument meaning, console lines and error
// behaviour, with the two hot calls going through the C-ABI of libstan_hip.so.
//   ParallelAssembly_K   SolverFunctions.cs:117-180  -> stan_hip_assemble_hex8
//   LinearSolver_CG      SolverFunctions.cs:270-330  -> stan_hip_cg_solve
//   Include_BC_DOF       SolverFunctions.cs:520-538
//   Exclude_BC_DOF       SolverFunctions.cs:540-555
//   Vector_Norm          SolverFunctions.cs:559-569
//   ProtoSerialize / ProtoDeserialize  :48-63      -> stdb.cpp
// Failures that make the C# throw (det J == 0 in MatrixST.Inverse, KeyNotFound on MatID ...)
// throw std::runtime_error here; a CG that does not converge is reported, not thrown, and U is
// returned regardless (SolverFunctions.cs:323-329).
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/stan_hip.h"
#include "model.h"

namespace stan {

// alglib.sparsematrix in the reference: here an opaque device-resident K plus its context.
class SparseMatrixHandle {
  public:
    SparseMatrixHandle() {}
    ~SparseMatrixHandle();
    stan_results *results = nullptr;   // strain / stress kept on the device(s) until the export has encoded them
    SparseMatrixHandle(const SparseMatrixHandle &) = delete;
    SparseMatrixHandle &operator=(const SparseMatrixHandle &) = delete;
    stan_ctx *ctx = nullptr;
    stan_matrix *K = nullptr;
    FlatModel flat;  // kept for Recovery_Stress (the reference caches J/BL on the elements)
};

// a stan_matrix that this side made (K + sigma M, M_c, K_g) and frees on every way out
struct MatrixFree {
    void operator()(stan_matrix *m) const { stan_hip_matrix_free(m); }
};
using OwnedMatrix = std::unique_ptr<stan_matrix, MatrixFree>;

// fn(i0, i1) over [0, n) on the host threads of libstan_host (STAN_HOST_THREADS)
template <typename F>
void ParallelRanges(size_t n, F fn) {
    const size_t nt = (size_t)HostThreads();
    if (nt <= 1 || n < 4096) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back([=] { fn(n * t / nt, n * (t + 1) / nt); });
    for (std::thread &x : th) x.join();
}

struct SolverOptions {  // extras of the native driver, never stored in the STdb
    int device = 0;
    std::vector<int> devices;   // --gpus N / --devices a,b,...: one process drives them all (stan_hip_init_multi)
    int precision = STAN_PREC_FP64;
    bool merit_stop = true;
    bool profile = false;
    bool p2p = false;           // STAN_OPT_COMM_P2P on a multi-device handle (throws where the devices cannot reach each other)
    int placement_tries = 16;   // STAN_OPT_PLACEMENT_TRIES: K's value stream is placed by search (only blocks >= 256 MB)
};

class SolverFunctions {
  public:
    explicit SolverFunctions(const SolverOptions &opt = SolverOptions()) : opt_(opt) {}
    ~SolverFunctions();

    // Round 5: the device context (HIP runtime start-up, streams, the communicator of a multi-device handle) comes up
    // on a thread of its own while the input file is read; ParallelAssembly_K waits for it.  Not calling it is fine.
    void Prewarm();

    void Welcome_Messsage() const;
    bool ProtoDeserialize(const std::string &path, Database *db, std::string *err) const { return ReadStdb(path, db, err); }
    bool ProtoSerialize(const Database &db, const std::string &path, bool packed, std::string *err) const { return WriteStdb(db, path, packed, err); }

    // K = ParallelAssembly_K(DB, nDOF_reduction, inc, "Initial")
    void ParallelAssembly_K(const Database &DB, const std::vector<int32_t> &nDOF_reduction, int inc,
                            const std::string &type, SparseMatrixHandle *K) const;
    // U = LinearSolver_CG(K, F, AnalysisLib)
    std::vector<double> LinearSolver_CG(SparseMatrixHandle &K, const std::vector<double> &F,
                                        const Analysis &AnalysisLib) const;
    // U = LinearSolver_Cholesky(K, F) / LinearSolver_LU(K, F) (SolverFunctions.cs:332-516): the
    // direct solvers are outside the GPU hot path -- K is exported as the reduced upper CRS alglib
    // would hold and factorised on the CPU (libstan_host.so, direct.cpp)
    std::vector<double> LinearSolver_Cholesky(SparseMatrixHandle &K, const std::vector<double> &F) const;
    std::vector<double> LinearSolver_LU(SparseMatrixHandle &K, const std::vector<double> &F) const;
    // Element.Recovery_Stress + Update_StrainStress for every element (Solver.cs:183-210)
    void Recovery_Stress(SparseMatrixHandle &K, const std::vector<double> &nodal_dU,
                         std::vector<double> *strain, std::vector<double> *stress) const;
    // the same with the results left on the device(s) (K.results): the export maps them chunk by chunk
    // (stan_hip_results_map through Database::ResultView::fetch) instead of holding 1.5 KB per element on the host
    void Recovery_Stress_Keep(SparseMatrixHandle &K, const std::vector<double> &nodal_dU) const;

    // Part.Load_Scalar + Part.ExportGrid / ExportWindow.Export_Click (Part.cs:231-528, 858-939; ExportWindow.xaml.cs:43-108):
    // the point scalars `sel` (indices of stan_hip.h's STAN_SCALAR_*; with `cells` also their Max / Average / Min cell
    // arrays) of increment 1, from the results kept on the device (K.results) or, when strain / stress are given, from
    // those host arrays, written to <prefix>_001.vtu (inc.ToString("000")).  Seconds spent go to *t_scalars / *t_write.
    // `reaction` (full DOF numbering, from Equilibrium) adds the point arrays "Reaction Force X" / "Y" / "Z" behind them.
    void Export_Vtu(SparseMatrixHandle &K, const std::vector<double> &nodal_dU, const std::vector<double> *strain,
                    const std::vector<double> *stress, const std::string &prefix, const std::vector<int32_t> &sel, bool cells,
                    double *t_scalars, double *t_write, const std::vector<double> *reaction = nullptr) const;

    // Internal forces f_int(u) = sum_e int B^T D B u_e dV from coordinates and displacements alone, the support reactions
    // and the out-of-balance sums of F - f_int (stan_hip_internal_forces_hex8): no step of the reference -- a check of
    // assembly and solve that shares no code with them.  nodal_dU [n_nodes*3] in NodeLib order, F the reduced load vector;
    // f_int / reaction [nDOF] (either may be null), *eq always filled.
    void Equilibrium(SparseMatrixHandle &K, const std::vector<double> &nodal_dU, const std::vector<double> &F,
                     const std::vector<int32_t> &nDOF_reduction, std::vector<double> *f_int, std::vector<double> *reaction,
                     stan_equilibrium *eq) const;
    // Distributed loads and prescribed displacements (stan_hip_load_vector_hex8; no step of the reference): adds the
    // consistent nodal loads of `dl` to the reduced external load F (in place) and leaves in *F_solve the right-hand side
    // of the reduced system, F - f_int(u0)|free; *sums always filled.  One device only.
    void Load_Vector(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const DistributedLoads &dl,
                     std::vector<double> *F, std::vector<double> *F_solve, stan_load_sums *sums) const;
    // Thermal loads (stan_hip_thermal_load_hex8; no step of the reference): adds the load of `tl` to the reduced external
    // load F (in place) and leaves the load over all DOFs in *load_full (the supports exert f_int - load_full); *sums always
    // filled.  One device only.
    void Thermal_Load(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const ThermalLoads &tl,
                      std::vector<double> *F, std::vector<double> *load_full, stan_thermal_sums *sums) const;
    // ... and the recovered stress loses beta dT at every corner: the host array when given, else the results kept on the
    // device (K.results)
    void Thermal_Stress(SparseMatrixHandle &K, const ThermalLoads &tl, std::vector<double> *stress) const;
    // the row-sum lumped mass of `md` on the free DOFs, M [N] (stan_hip_lumped_mass_hex8); *sums always filled
    void LumpedMass(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const MassDensity &md, std::vector<double> *M,
                    stan_mass_sums *sums) const;
    // Modal analysis (stan_hip_lumped_mass_hex8 + stan_hip_modes; no step of the reference): the lumped mass of `md` and the
    // n_modes lowest eigenpairs of K phi = lambda M phi; lambda / rho [n_modes], phi [n_modes][N] on the free DOFs; *sums and
    // *rep always filled.  One device only.  shift > 0 (a free-free model): on K + shift M (stan_hip_matrix_shifted) and
    // lambda = mu - shift; rho and the report are the shifted problem's.
    // MASS_CONSISTENT: the same on M_c on K's layout (stan_hip_consistent_mass_hex8) and
    // stan_hip_modes_pencil; shift > 0: on stan_hip_matrix_axpy(K, shift, M_c).  phi is scaled to phi^T M_c phi = 1; *rep holds the
    // fields the two entries' reports share.
    enum MassKind { MASS_LUMPED, MASS_CONSISTENT };
    void Modes(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const MassDensity &md, MassKind mass, int n_modes,
               double tol, std::vector<double> *lambda, std::vector<double> *phi, std::vector<double> *rho, stan_mass_sums *sums,
               stan_modes_report *rep, double shift = 0.0) const;
    // Transient dynamics (stan_hip_lumped_mass_hex8 + stan_hip_transient; no step of the reference):
    // implicit Newmark steps of M a + C v + K u = g(t) F from rest, F the reduced external load.  probe_dof: reduced DOFs;
    // probe_u [(n_steps + 1)][n_probe]; snaps [n_snap][3][N] when snap_every > 0; energy [(n_steps + 1)][3]; *sums and *rep
    // always filled.  One device only.
    struct TransientRun {
        double dt = 0, beta_N = 0, gamma = 0, alpha_R = 0, beta_R = 0, solve_eps = 0;
        int n_steps = 0, snap_every = 0;
        std::vector<double> curve_t, curve_g;
        std::vector<int32_t> probe_dof;
    };
    void Transient(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const MassDensity &md, const std::vector<double> &F,
                   const TransientRun &run, std::vector<double> *probe_u, std::vector<double> *snaps, std::vector<double> *energy,
                   stan_mass_sums *sums, stan_transient_report *rep) const;
    // Explicit dynamics (stan_hip_lumped_mass_hex8 + stan_hip_stable_step + stan_hip_explicit; no step of the reference, DESIGN.md
    // section 3.14): central-difference steps of M a + alpha_R M v + K u = g(t) F from rest.  dt_auto: run->dt becomes dt_scale *
    // 2 / sqrt(lambda_upper) (the row bound, before the run).  n_power iterations give the report's lambda_power; a dt it proves
    // unstable is the library's refusal.  probe_u [(n_steps + 1)][n_probe]; snaps [n_snap][3][N] when snap_every > 0; energy [2][3]
    // (n_steps = 0: [1][3]): steps 0 and n_steps; *sums and *rep always filled.  One device only.
    struct ExplicitRun {
        bool dt_auto = false;
        double dt = 0, dt_scale = 0.9, alpha_R = 0;
        int n_steps = 0, snap_every = 0, n_power = 30;
        std::vector<double> curve_t, curve_g;
        std::vector<int32_t> probe_dof;
    };
    void Explicit(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const MassDensity &md, const std::vector<double> &F,
                  ExplicitRun *run, std::vector<double> *probe_u, std::vector<double> *snaps, std::vector<double> *energy,
                  stan_mass_sums *sums, stan_explicit_report *rep) const;
    // Frequency response (no step of the reference): the steady-state response of M a + C v + K u = F e^{i w t}
    // at run.omega (rad/s) from the n_modes lowest modes, with the static correction of K^-1 F.  The modes are asked for exactly as
    // Modes() asks (stan_hip_modes_dev, or stan_hip_modes_pencil_dev on the consistent mass: the host entries' bits), the static solve
    // is stan_hip_cg_solve_dev with LinearSolver_CG's console lines and report fields, and stan_hip_harmonic_dev runs on what stayed in
    // device memory: Phi, F and the static solution never come to the host.  zeta < 0: no modal damping.  lambda, p [n_modes]; probe
    // [n_freq][n_probe][2]; snaps [n_snap][2][N] at the frequency indices 0, snap_every, ... (snap_every > 0); peak / peak_idx [N];
    // *sums, *mrep and *rep always filled.  One device only.
    struct HarmonicRun {
        double alpha_R = 0, beta_R = 0, zeta = -1;
        int snap_every = 0;
        std::vector<double> omega;
        std::vector<int32_t> probe_dof;
    };
    void HarmonicResident(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const MassDensity &md, MassKind mass,
                          int n_modes, double tol, const std::vector<double> &F, const Analysis &AnalysisLib, const HarmonicRun &run,
                          std::vector<double> *lambda, std::vector<double> *p, std::vector<double> *probe, std::vector<double> *snaps,
                          std::vector<double> *peak, std::vector<int32_t> *peak_idx, stan_mass_sums *sums, stan_modes_report *mrep,
                          stan_harmonic_report *rep) const;
    // <prefix>_peak.vtu: peak / peak_idx [N] on the free DOFs as the point arrays "Peak Amplitude" (3 components) and "Peak Frequency"
    // (the frequency in Hz at which the node's largest component peaks); <prefix>_freq_NNNN.vtu: re, im [N] as "Displacement Re" and
    // "Displacement Im" (3 components each), through the writer of vtu.cpp
    void Export_Peak_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const double *peak, const int32_t *peak_idx,
                         const std::vector<double> &hz, const std::string &prefix) const;
    void Export_Freq_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const double *re_im, size_t N,
                         const std::string &prefix, int index) const;
    // <prefix>_step_NNNN.vtu for one snapshot: u, v, a [N] on the free DOFs as the point arrays "Displacement X" / "Y" / "Z",
    // "Velocity ..." and "Acceleration ...", through the writer of vtu.cpp
    void Export_Step_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const double *uva, size_t N,
                         const std::string &prefix, int step) const;
    // Linear buckling (stan_hip_geometric_stiffness_hex8 + stan_hip_buckling; no step of the reference):
    // G = K_g of the static solution nodal_dU [n_nodes*3] (NodeLib order), then the n_modes lowest positive load factors of
    // (K + lambda G) phi = 0; factor / rho [n_modes], phi [n_modes][N] on the free DOFs; *rep always filled.  One device only.
    void Buckling(SparseMatrixHandle &K, const std::vector<int32_t> &nDOF_reduction, const std::vector<double> &nodal_dU, int n_modes,
                  double tol, double solve_eps, std::vector<double> *factor, std::vector<double> *phi, std::vector<double> *rho,
                  stan_buckling_report *rep) const;
    // <prefix>_mode_NNN.vtu / <prefix>_buckle_NNN.vtu (NNN = 001 ...) for one mode or buckling shape: shape [n_nodes*3] in NodeLib
    // order as the point arrays "Mode Shape X" / "Y" / "Z" ("Buckling Shape ...") and "Magnitude", through the writer of vtu.cpp
    // (the shape also takes the place of the displacements)
    struct ShapeKind {
        const char *stem, *names[4];
    };
    static const ShapeKind MODE_SHAPE, BUCKLING_SHAPE;
    void Export_Shape_Vtu(SparseMatrixHandle &K, const std::vector<double> &shape, const std::string &prefix, const ShapeKind &kind,
                          int number) const;
    // "name,name,..." of --vtu-results -> indices (stan_host_scalar_name's strings; empty text = all 24); false + *err on an unknown name
    static bool ParseScalarNames(const std::string &text, std::vector<int32_t> *sel, std::string *err);

    // a reduced vector [N] in NodeLib order, [n_nodes*3]: U = Include_BC_DOF(U, nDOF_reduction) and node.dU_buffer[d] = U[DOF[d]]
    // (Solver.cs:168-178) in one pass over the nodes, without the vector over all DOFs in between; 0 at the fixed DOFs
    std::vector<double> Nodal_Vector(const SparseMatrixHandle &K, const double *reduced, const std::vector<int32_t> &nDOF_reduction) const;
    std::vector<double> Include_BC_DOF(const std::vector<double> &A, const std::vector<int32_t> &nDOF_reduction) const;
    std::vector<double> Exclude_BC_DOF(const std::vector<double> &A, const std::vector<int32_t> &nDOF_reduction) const;
    double Vector_Norm(const std::vector<double> &v) const;

    // report of the last LinearSolver_CG
    int last_termination_type = 0, last_iterations = 0;
    double last_rel_residual = 0, last_assembly_s = 0, last_cg_s = 0;

  private:
    SolverOptions opt_;
    struct Warm;            // the context being created ahead of its use
    Warm *warm_ = nullptr;
};

}  // namespace stan
