// solver_functions.cpp -- see solver_functions.h.
#include "solver_functions.h"

#include "../../include/stan_host.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <dlfcn.h>
#include <thread>

namespace stan {

using clk = std::chrono::steady_clock;
static double secs(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

namespace {

// the mesh arguments of a stan_hip_*_hex8 call: sizes and pointers of the flat model
struct MeshView {
    explicit MeshView(const FlatModel &f)
        : n_nodes((int64_t)(f.xyz.size() / 3)), n_elem((int64_t)f.elem_mat.size()), n_mat((int32_t)(f.mat_E_nu.size() / 2)),
          xyz(f.xyz.data()), mat_E_nu(f.mat_E_nu.data()), node_dof(f.node_dof.data()), conn(f.conn.data()),
          elem_mat(f.elem_mat.data()), elem_type(f.elem_type.data()) {}
    int64_t n_nodes, n_elem;
    int32_t n_mat;
    const double *xyz, *mat_E_nu;
    const int32_t *node_dof, *conn, *elem_mat;
    const uint8_t *elem_type;
};

// the free DOFs of a reduction map (-1 marks a fixed one)
size_t n_reduced(const std::vector<int32_t> &red) {
    size_t n_fixed = 0;
    for (int32_t r : red) n_fixed += r == -1;
    return red.size() - n_fixed;
}

// the fields that the reports of stan_hip_modes and stan_hip_modes_pencil share
stan_modes_report shared_fields(const stan_buckling_report &b) {
    return {b.block, b.outer, b.converged, b.cg_worst_type, b.cg_iterations, b.max_rho, b.solve_ms, b.product_ms, b.block_ms, b.gram_ms,
            b.rotate_ms};
}

}  // namespace

struct SolverFunctions::Warm {
    std::thread th;
    stan_ctx *ctx = nullptr;
    int rc = 0;
    std::string err;
};
SolverFunctions::~SolverFunctions() {
    if (!warm_) return;
    if (warm_->th.joinable()) warm_->th.join();
    if (warm_->ctx) stan_hip_destroy(warm_->ctx);   // never picked up (the run ended before the assembly)
    delete warm_;
}
void SolverFunctions::Prewarm() {
    if (warm_) return;
    warm_ = new Warm();
    Warm *w = warm_;
    const SolverOptions opt = opt_;
    w->th = std::thread([w, opt] {
        w->rc = opt.devices.size() > 1 ? stan_hip_init_multi((int)opt.devices.size(), opt.devices.data(), &w->ctx)
                                       : stan_hip_init(opt.devices.empty() ? opt.device : opt.devices[0], &w->ctx);
        if (w->rc) w->err = stan_hip_last_error(nullptr);   // (thread-local text: taken on this thread)
    });
}

SparseMatrixHandle::~SparseMatrixHandle() {
    if (results) stan_hip_results_free(results);
    if (K) stan_hip_matrix_free(K);
    if (ctx) stan_hip_destroy(ctx);
}

void SolverFunctions::Welcome_Messsage() const {  // SolverFunctions.cs:23-44 (no window sizing, :18-20)
    puts("");
    puts("  ========================================================== ");
    puts("  ********************************************************** ");
    puts("                  STAN - STructural ANalyser                 ");
    puts("  ********************************************************** ");
    puts("      Solver: Linear, Statics  (MI355X native hot path)      ");
    puts("  ========================================================== ");
    puts("                                                             ");
}

void SolverFunctions::ParallelAssembly_K(const Database &DB, const std::vector<int32_t> &red, int inc,
                                         const std::string &type, SparseMatrixHandle *K) const {
    if (type != "Initial" || inc != 1)  // "Tangent" belongs to the unfinished nonlinear driver
        throw std::runtime_error("ParallelAssembly_K: only type \"Initial\" at increment 1 (linear statics)");
    const auto t0 = clk::now();
    printf("   K Matrix assembly: ");  // SolverFunctions.cs:127
    fflush(stdout);
    std::string err;
    if (Flatten(DB, &K->flat, &err)) throw std::runtime_error(err);
    // several GPUs: still ONE process and the same calls -- the handle fans them out (stan_hip.h)
    if (warm_) {   // the context was started while the file was read (Prewarm)
        if (warm_->th.joinable()) warm_->th.join();
        if (warm_->rc) throw std::runtime_error(warm_->err);
        K->ctx = warm_->ctx;
        warm_->ctx = nullptr;
    } else {
        const int rc_init = opt_.devices.size() > 1
                                ? stan_hip_init_multi((int)opt_.devices.size(), opt_.devices.data(), &K->ctx)
                                : stan_hip_init(opt_.devices.empty() ? opt_.device : opt_.devices[0], &K->ctx);
        if (rc_init) throw std::runtime_error(stan_hip_last_error(nullptr));
    }
    stan_hip_set_option(K->ctx, STAN_OPT_CG_MERIT_STOP, opt_.merit_stop ? 1 : 0);
    stan_hip_set_option(K->ctx, STAN_OPT_POOL_MAX_BYTES, -1);   // this process owns its device(s)
    stan_hip_set_option(K->ctx, STAN_OPT_PLACEMENT_TRIES, opt_.placement_tries < 1 ? 1 : opt_.placement_tries);
    if (opt_.p2p && stan_hip_set_option(K->ctx, STAN_OPT_COMM_P2P, 1)) throw std::runtime_error(stan_hip_last_error(K->ctx));
    if (opt_.profile) stan_hip_set_profiling(K->ctx, 1);
    const MeshView v(K->flat);
    const int rc = stan_hip_assemble_hex8(K->ctx, v.n_nodes, v.xyz, v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat,
                                          v.mat_E_nu, DB.nDOF, red.data(), &K->K);
    if (rc) throw std::runtime_error(stan_hip_last_error(K->ctx));  // det J == 0: MatrixST.cs:315-318 throws
    const_cast<SolverFunctions *>(this)->last_assembly_s = secs(t0);
    printf("          Done in %.2fs\n", last_assembly_s);  // SolverFunctions.cs:177
}

std::vector<double> SolverFunctions::LinearSolver_CG(SparseMatrixHandle &K, const std::vector<double> &F,
                                                     const Analysis &A) const {
    const auto t0 = clk::now();
    printf("   Solving linear system...   ");  // SolverFunctions.cs:273
    fflush(stdout);
    std::vector<double> U(F.size(), 0.0);
    int32_t type = 0, its = 0;
    double rel = 0;
    if (stan_hip_cg_solve(K.ctx, K.K, F.data(), A.LinSolverTolerance, A.LinSolverIterMax, opt_.precision,
                          U.data(), &type, &its, &rel))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    SolverFunctions *self = const_cast<SolverFunctions *>(this);
    self->last_termination_type = type; self->last_iterations = its; self->last_rel_residual = rel;
    self->last_cg_s = secs(t0);
    printf(type == 1 || type == 7 ? "  NORMAL " : "  ERROR ");  // SolverFunctions.cs:323-324
    printf(" (type %d) in %.2fs\n", type, last_cg_s);          // :325-327
    return U;                                                    // :329, returned regardless
}

// alglib.sparsematrix as the reference holds it after ParallelAssembly_K: reduced upper CRS
static void ExportUpperCrs(SparseMatrixHandle &K, std::vector<int64_t> *rowptr, std::vector<int32_t> *col,
                           std::vector<double> *val) {
    int64_t nnz = 0;
    if (stan_hip_matrix_to_csr(K.ctx, K.K, 1, &nnz, nullptr, nullptr, nullptr))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    stan_matrix_info info;
    stan_hip_matrix_info(K.K, &info);
    rowptr->assign((size_t)info.n_reduced + 1, 0);
    col->assign((size_t)nnz, 0);
    val->assign((size_t)nnz, 0.0);
    if (stan_hip_matrix_to_csr(K.ctx, K.K, 1, &nnz, rowptr->data(), col->data(), val->data()))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

std::vector<double> SolverFunctions::LinearSolver_Cholesky(SparseMatrixHandle &K, const std::vector<double> &F) const {
    const auto t0 = clk::now();
    puts("   Linear system K*U=F:");                       // SolverFunctions.cs:385
    std::vector<int64_t> rp; std::vector<int32_t> ci; std::vector<double> cv;
    ExportUpperCrs(K, &rp, &ci, &cv);                      // sparseconverttosks works on the same triangle
    printf("    - Cholesky decomposition:");               // :388
    fflush(stdout);
    std::vector<double> U(F.size(), 0.0);
    int32_t type = 0;
    int64_t profile = 0;
    const int rc = stan_host_cholesky_skyline_solve((int64_t)F.size(), rp.data(), ci.data(), cv.data(), F.data(),
                                                    U.data(), &type, &profile);
    if (rc == STAN_HOST_E_MEMORY)
        throw std::runtime_error("LinearSolver_Cholesky: the skyline profile (" + std::to_string(profile) +
                                 " entries) does not fit in memory; use LinSolver = CG");
    if (rc) throw std::runtime_error("LinearSolver_Cholesky: bad matrix (code " + std::to_string(rc) + ")");
    puts(type > 0 ? "   Done" : "   ERROR");                 // :390-397
    printf("    - Solving:");                               // :426
    printf(type > 0 ? "                  NORMAL termination" : "                  ERROR termination");
    printf(" (type %d)\n", type);                           // :430-438
    SolverFunctions *self = const_cast<SolverFunctions *>(this);
    self->last_termination_type = type; self->last_iterations = 0; self->last_rel_residual = 0;
    self->last_cg_s = secs(t0);
    printf("    Total time to solve K*U=F:  %.2fs\n", last_cg_s);   // :441
    return U;
}

std::vector<double> SolverFunctions::LinearSolver_LU(SparseMatrixHandle &K, const std::vector<double> &F) const {
    const auto t0 = clk::now();
    printf("   Solving linear system...   ");               // SolverFunctions.cs:449
    fflush(stdout);
    std::vector<int64_t> rp; std::vector<int32_t> ci; std::vector<double> cv;
    ExportUpperCrs(K, &rp, &ci, &cv);
    std::vector<double> U(F.size(), 0.0);
    int32_t type = 0;
    if (int rc = stan_host_lu_upper_solve((int64_t)F.size(), rp.data(), ci.data(), cv.data(), F.data(), U.data(), &type))
        throw std::runtime_error("LinearSolver_LU: bad matrix (code " + std::to_string(rc) + ")");
    SolverFunctions *self = const_cast<SolverFunctions *>(this);
    self->last_termination_type = type; self->last_iterations = 0; self->last_rel_residual = 0;
    self->last_cg_s = secs(t0);
    printf(type > 0 ? "NORMAL TERMINATION" : "ERROR TERMINATION");   // :506-507
    printf(" (type %d) in %.2fs\n", type, last_cg_s);               // :508-510
    return U;
}

void SolverFunctions::Recovery_Stress(SparseMatrixHandle &K, const std::vector<double> &dU,
                                      std::vector<double> *strain, std::vector<double> *stress) const {
    const MeshView v(K.flat);
    strain->assign((size_t)v.n_elem * 48, 0.0);
    stress->assign((size_t)v.n_elem * 48, 0.0);
    if (stan_hip_recover_hex8(K.ctx, v.n_nodes, v.xyz, dU.data(), v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat, v.mat_E_nu,
                              strain->data(), stress->data()))
        throw std::runtime_error(stan_hip_last_error(K.ctx));  // HEX8_G1: the reference throws too (Element.cs:242)
}

void SolverFunctions::Equilibrium(SparseMatrixHandle &K, const std::vector<double> &dU, const std::vector<double> &F,
                                  const std::vector<int32_t> &red, std::vector<double> *f_int, std::vector<double> *reaction,
                                  stan_equilibrium *eq) const {
    const MeshView v(K.flat);
    if (f_int) f_int->assign(red.size(), 0.0);
    if (reaction) reaction->assign(red.size(), 0.0);
    if (stan_hip_internal_forces_hex8(K.ctx, v.n_nodes, v.xyz, dU.data(), v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat,
                                      v.mat_E_nu, (int64_t)red.size(), red.data(), F.empty() ? nullptr : F.data(),
                                      f_int ? f_int->data() : nullptr, reaction ? reaction->data() : nullptr, eq))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Load_Vector(SparseMatrixHandle &K, const std::vector<int32_t> &red, const DistributedLoads &dl,
                                  std::vector<double> *F, std::vector<double> *F_solve, stan_load_sums *sums) const {
    const MeshView v(K.flat);
    F_solve->assign(F->size(), 0.0);
    if (stan_hip_load_vector_hex8(K.ctx, v.n_nodes, v.xyz, v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat, v.mat_E_nu,
                                  (int64_t)red.size(), red.data(), dl.mat_body.empty() ? nullptr : dl.mat_body.data(), (int64_t)dl.face_elem.size(),
                                  dl.face_elem.data(), dl.face_id.data(), dl.face_p.data(),
                                  dl.disp0.empty() ? nullptr : dl.disp0.data(), F->data(), F_solve->data(), nullptr, sums))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Thermal_Load(SparseMatrixHandle &K, const std::vector<int32_t> &red, const ThermalLoads &tl,
                                   std::vector<double> *F, std::vector<double> *load_full, stan_thermal_sums *sums) const {
    const MeshView v(K.flat);
    load_full->assign(red.size(), 0.0);
    if (stan_hip_thermal_load_hex8(K.ctx, v.n_nodes, v.xyz, v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat, v.mat_E_nu,
                                   (int64_t)red.size(), red.data(), tl.mat_alpha.data(), tl.dT.data(), F->data(), load_full->data(), sums))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Thermal_Stress(SparseMatrixHandle &K, const ThermalLoads &tl, std::vector<double> *stress) const {
    const MeshView v(K.flat);
    const int rc = stress ? stan_hip_thermal_stress_hex8(K.ctx, v.n_nodes, tl.dT.data(), v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat,
                                                         v.mat_E_nu, tl.mat_alpha.data(), stress->data())
                          : stan_hip_results_thermal_stress(K.ctx, K.results, v.n_nodes, tl.dT.data(), v.conn, v.elem_mat, v.elem_type,
                                                            v.n_mat, v.mat_E_nu, tl.mat_alpha.data());
    if (rc) throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Modes(SparseMatrixHandle &K, const std::vector<int32_t> &red, const MassDensity &md, MassKind mass, int n_modes,
                            double tol, std::vector<double> *lambda, std::vector<double> *phi, std::vector<double> *rho,
                            stan_mass_sums *sums, stan_modes_report *rep, double shift) const {
    std::vector<double> M;
    LumpedMass(K, red, md, &M, sums);   // under the consistent mass too: the sums (total mass, volume) and the refusal of a free DOF without mass
    const size_t N = M.size();
    const size_t k = n_modes > 0 ? (size_t)n_modes : 1;
    lambda->assign(k, 0.0); rho->assign(k, 0.0); phi->assign(k * N, 0.0);
    OwnedMatrix Mc, shifted;   // the mass and the operator, by kind
    stan_matrix *made = nullptr;
    if (mass == MASS_CONSISTENT) {
        const MeshView v(K.flat);
        if (stan_hip_consistent_mass_hex8(K.ctx, K.K, v.n_nodes, v.xyz, md.mat_rho.data(), v.node_dof, v.n_elem, v.conn, v.elem_mat,
                                          v.elem_type, v.n_mat, v.mat_E_nu, (int64_t)red.size(), red.data(), &made))
            throw std::runtime_error(stan_hip_last_error(K.ctx));
        Mc.reset(made);
    }
    if (shift > 0) {
        if (Mc ? stan_hip_matrix_axpy(K.ctx, K.K, shift, Mc.get(), &made) : stan_hip_matrix_shifted(K.ctx, K.K, shift, M.data(), &made))
            throw std::runtime_error(stan_hip_last_error(K.ctx));
        shifted.reset(made);
    }
    stan_matrix *A = shifted ? shifted.get() : K.K;
    stan_buckling_report pencil{};
    if (Mc ? stan_hip_modes_pencil(K.ctx, A, Mc.get(), n_modes, tol, 0, 0.0, 0, lambda->data(), phi->data(), rho->data(), &pencil)
           : stan_hip_modes(K.ctx, A, M.data(), n_modes, tol, 0, 0.0, 0, lambda->data(), phi->data(), rho->data(), rep))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    if (Mc) *rep = shared_fields(pencil);
    if (shift > 0)
        for (double &l : *lambda) l -= shift;
}

void SolverFunctions::LumpedMass(SparseMatrixHandle &K, const std::vector<int32_t> &red, const MassDensity &md, std::vector<double> *M,
                                 stan_mass_sums *sums) const {
    const MeshView v(K.flat);
    const size_t N = n_reduced(red);
    M->assign(N > 0 ? N : 1, 0.0);
    if (stan_hip_lumped_mass_hex8(K.ctx, v.n_nodes, v.xyz, v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat, v.mat_E_nu,
                                  (int64_t)red.size(), red.data(), md.mat_rho.data(), M->data(), nullptr, sums))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Transient(SparseMatrixHandle &K, const std::vector<int32_t> &red, const MassDensity &md, const std::vector<double> &F,
                                const TransientRun &run, std::vector<double> *probe_u, std::vector<double> *snaps,
                                std::vector<double> *energy, stan_mass_sums *sums, stan_transient_report *rep) const {
    std::vector<double> M;
    LumpedMass(K, red, md, &M, sums);
    const size_t N = M.size(), rows = (size_t)run.n_steps + 1, np = run.probe_dof.size();
    const size_t n_snap = run.snap_every > 0 ? (size_t)(run.n_steps / run.snap_every) + 1 : 0;
    probe_u->assign(rows * np, 0.0);
    snaps->assign(n_snap * 3 * N, 0.0);
    energy->assign(rows * 3, 0.0);
    std::vector<double> u(N), v(N), a(N);
    if (stan_hip_transient(K.ctx, K.K, M.data(), F.data(), nullptr, nullptr, run.dt, run.n_steps, run.beta_N, run.gamma, run.alpha_R,
                           run.beta_R, (int32_t)run.curve_t.size(), run.curve_t.data(), run.curve_g.data(), run.solve_eps, 0, (int32_t)np,
                           np ? run.probe_dof.data() : nullptr, np ? probe_u->data() : nullptr, run.snap_every,
                           n_snap ? snaps->data() : nullptr, energy->data(), u.data(), v.data(), a.data(), rep))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

void SolverFunctions::Explicit(SparseMatrixHandle &K, const std::vector<int32_t> &red, const MassDensity &md, const std::vector<double> &F,
                               ExplicitRun *run, std::vector<double> *probe_u, std::vector<double> *snaps, std::vector<double> *energy,
                               stan_mass_sums *sums, stan_explicit_report *rep) const {
    std::vector<double> M;
    LumpedMass(K, red, md, &M, sums);
    if (run->dt_auto) {
        double upper = 0, power = 0, dt_stable = 0;
        if (stan_hip_stable_step(K.ctx, K.K, M.data(), 0, &upper, &power, &dt_stable)) throw std::runtime_error(stan_hip_last_error(K.ctx));
        run->dt = run->dt_scale * dt_stable;
    }
    const size_t N = M.size(), rows = (size_t)run->n_steps + 1, np = run->probe_dof.size();
    const size_t n_snap = run->snap_every > 0 ? (size_t)(run->n_steps / run->snap_every) + 1 : 0;
    const int energy_every = run->n_steps > 0 ? run->n_steps : 1;   // steps 0 and n_steps: a long run does not pay the sums each step
    probe_u->assign(rows * np, 0.0);
    snaps->assign(n_snap * 3 * N, 0.0);
    energy->assign((size_t)(run->n_steps / energy_every + 1) * 3, 0.0);
    std::vector<double> u(N), v(N), a(N);
    if (stan_hip_explicit(K.ctx, K.K, M.data(), F.data(), nullptr, nullptr, run->dt, run->n_steps, run->alpha_R, (int32_t)run->curve_t.size(),
                          run->curve_t.data(), run->curve_g.data(), (int32_t)np, np ? run->probe_dof.data() : nullptr,
                          np ? probe_u->data() : nullptr, run->snap_every, n_snap ? snaps->data() : nullptr, energy_every, energy->data(),
                          u.data(), v.data(), a.data(), run->n_power, rep))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

namespace {

// Device memory of this process for the run that keeps its arrays resident (HarmonicResident).  The HIP runtime is in the process
// already, as libstan_hip.so's own dependency: its four entries are looked up by name, so that this side needs neither HIP's
// headers nor a link line of its own.  Copies are the synchronous ones: an array is ready on every stream when upload() returns.
struct DeviceRuntime {
    int (*set_device)(int) = nullptr;
    int (*malloc_)(void **, size_t) = nullptr;
    int (*free_)(void *) = nullptr;
    int (*memcpy_)(void *, const void *, size_t, int) = nullptr;   // kind 1: host to device, 2: device to host
    DeviceRuntime() {
        set_device = (int (*)(int))dlsym(RTLD_DEFAULT, "hipSetDevice");
        malloc_ = (int (*)(void **, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
        free_ = (int (*)(void *))dlsym(RTLD_DEFAULT, "hipFree");
        memcpy_ = (int (*)(void *, const void *, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
        if (!set_device || !malloc_ || !free_ || !memcpy_) throw std::runtime_error("the HIP runtime's entries are not in this process");
    }
};

template <typename T>
struct DeviceArray {   // n entries on the device, given back on every way out
    const DeviceRuntime &rt;
    T *p = nullptr;
    size_t n;
    DeviceArray(const DeviceRuntime &r, size_t count) : rt(r), n(count) {
        if (rt.malloc_((void **)&p, (n ? n : 1) * sizeof(T))) throw std::runtime_error("hipMalloc of " + std::to_string(n * sizeof(T)) + " bytes failed");
    }
    DeviceArray(const DeviceRuntime &r, const std::vector<T> &host) : DeviceArray(r, host.size()) {
        if (n && rt.memcpy_(p, host.data(), n * sizeof(T), 1)) throw std::runtime_error("copy to the device failed");
    }
    DeviceArray(const DeviceArray &) = delete; DeviceArray &operator=(const DeviceArray &) = delete;
    ~DeviceArray() { rt.free_(p); }
    void fetch(std::vector<T> *host) const {
        host->resize(n);
        if (n && rt.memcpy_(host->data(), p, n * sizeof(T), 2)) throw std::runtime_error("copy from the device failed");
    }
};

}  // namespace

void SolverFunctions::HarmonicResident(SparseMatrixHandle &K, const std::vector<int32_t> &red, const MassDensity &md, MassKind mass,
                                       int n_modes, double tol, const std::vector<double> &F, const Analysis &A, const HarmonicRun &run,
                                       std::vector<double> *lambda, std::vector<double> *p, std::vector<double> *probe,
                                       std::vector<double> *snaps, std::vector<double> *peak, std::vector<int32_t> *peak_idx,
                                       stan_mass_sums *sums, stan_modes_report *mrep, stan_harmonic_report *rep) const {
    std::vector<double> M;
    LumpedMass(K, red, md, &M, sums);   // as Modes(): under the consistent mass too
    const size_t N = M.size(), k = n_modes > 0 ? (size_t)n_modes : 1, nf = run.omega.size(), np = run.probe_dof.size();
    const DeviceRuntime rt;
    if (rt.set_device(opt_.device)) throw std::runtime_error("hipSetDevice failed");
    // the modes, exactly as Modes() asks for them, into device memory
    DeviceArray<double> d_lambda(rt, k), d_phi(rt, k * N), d_rho(rt, k);
    if (mass == MASS_CONSISTENT) {
        const MeshView v(K.flat);
        stan_matrix *made = nullptr;
        if (stan_hip_consistent_mass_hex8(K.ctx, K.K, v.n_nodes, v.xyz, md.mat_rho.data(), v.node_dof, v.n_elem, v.conn, v.elem_mat,
                                          v.elem_type, v.n_mat, v.mat_E_nu, (int64_t)red.size(), red.data(), &made))
            throw std::runtime_error(stan_hip_last_error(K.ctx));
        const OwnedMatrix Mc(made);
        stan_buckling_report pencil{};
        if (stan_hip_modes_pencil_dev(K.ctx, K.K, Mc.get(), n_modes, tol, 0, 0.0, 0, d_lambda.p, d_phi.p, d_rho.p, &pencil))
            throw std::runtime_error(stan_hip_last_error(K.ctx));
        *mrep = shared_fields(pencil);
    } else {
        const DeviceArray<double> d_M(rt, M);
        if (stan_hip_modes_dev(K.ctx, K.K, d_M.p, n_modes, tol, 0, 0.0, 0, d_lambda.p, d_phi.p, d_rho.p, mrep))
            throw std::runtime_error(stan_hip_last_error(K.ctx));
    }
    d_lambda.fetch(lambda);
    // the static solution, with LinearSolver_CG's lines
    const auto t0 = clk::now();
    printf("   Solving linear system...   ");
    fflush(stdout);
    const DeviceArray<double> d_F(rt, F);
    DeviceArray<double> d_U(rt, N);
    int32_t type = 0, its = 0;
    double rel = 0;
    if (stan_hip_cg_solve_dev(K.ctx, K.K, d_F.p, A.LinSolverTolerance, A.LinSolverIterMax, opt_.precision, d_U.p, &type, &its, &rel))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    SolverFunctions *self = const_cast<SolverFunctions *>(this);
    self->last_termination_type = type; self->last_iterations = its; self->last_rel_residual = rel;
    self->last_cg_s = secs(t0);
    printf(type == 1 || type == 7 ? "  NORMAL " : "  ERROR ");
    printf(" (type %d) in %.2fs\n", type, last_cg_s);
    // the response on what stayed in device memory
    std::vector<int32_t> snap_freq;
    for (size_t f = 0; run.snap_every > 0 && f < nf; f += (size_t)run.snap_every) snap_freq.push_back((int32_t)f);
    const std::vector<double> zeta(k, run.zeta);
    const DeviceArray<int32_t> d_probe_dof(rt, run.probe_dof);
    DeviceArray<double> d_p(rt, k), d_probe(rt, nf * np * 2), d_snaps(rt, snap_freq.size() * 2 * N), d_peak(rt, N);
    DeviceArray<int32_t> d_peak_idx(rt, N);
    if (stan_hip_harmonic_dev(K.ctx, (int64_t)N, (int32_t)k, d_lambda.p, d_phi.p, d_F.p, d_U.p, run.alpha_R, run.beta_R,
                              run.zeta >= 0 ? zeta.data() : nullptr, (int32_t)nf, run.omega.data(), (int32_t)np,
                              np ? d_probe_dof.p : nullptr, np ? d_probe.p : nullptr, (int32_t)snap_freq.size(),
                              snap_freq.empty() ? nullptr : snap_freq.data(), snap_freq.empty() ? nullptr : d_snaps.p, d_p.p, d_peak.p,
                              d_peak_idx.p, rep))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    d_p.fetch(p); d_probe.fetch(probe); d_snaps.fetch(snaps); d_peak.fetch(peak); d_peak_idx.fetch(peak_idx);
}

// a reduced vector [N] as [n_nodes][3] in NodeLib order (0 at the fixed DOFs), appended to *point
static void AppendNodal(const SolverFunctions &fn, SparseMatrixHandle &K, const double *reduced, const std::vector<int32_t> &red,
                        std::vector<double> *point) {
    const std::vector<double> nodal = fn.Nodal_Vector(K, reduced, red);
    point->insert(point->end(), nodal.begin(), nodal.end());
}

void SolverFunctions::Export_Peak_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &red, const double *peak, const int32_t *peak_idx,
                                      const std::vector<double> &hz, const std::string &prefix) const {
    const MeshView v(K.flat);
    static const char *const names[2] = {"Peak Amplitude", "Peak Frequency"};
    static const int32_t comps[2] = {3, 1};
    std::vector<double> point;
    AppendNodal(*this, K, peak, red, &point);
    // the frequency at which the node's largest component peaks (a node without a free DOF: 0)
    const std::vector<int32_t> &node_dof = K.flat.node_dof;
    for (int64_t n = 0; n < v.n_nodes; n++) {
        double best = -1.0, at = 0.0;
        for (int c = 0; c < 3; c++) {
            const size_t d = (size_t)node_dof[(size_t)(3 * n + c)];
            if (red[d] == -1) continue;
            const size_t r = d - (size_t)red[d];
            if (peak[r] > best) { best = peak[r]; at = hz[(size_t)peak_idx[r]]; }
        }
        point.push_back(at);
    }
    const std::string path = prefix + "_peak.vtu";
    if (stan_host_write_vtu_components(path.c_str(), v.n_nodes, v.xyz, nullptr, v.n_elem, v.conn, 2, names, comps, point.data(), 0, nullptr,
                                       nullptr))
        throw std::runtime_error("cannot write " + path);
}

void SolverFunctions::Export_Freq_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &red, const double *re_im, size_t N,
                                      const std::string &prefix, int index) const {
    const MeshView v(K.flat);
    static const char *const names[2] = {"Displacement Re", "Displacement Im"};
    static const int32_t comps[2] = {3, 3};
    std::vector<double> point;
    AppendNodal(*this, K, re_im, red, &point);
    AppendNodal(*this, K, re_im + N, red, &point);
    char num[16];
    snprintf(num, sizeof num, "%04d", index);
    const std::string path = prefix + "_freq_" + num + ".vtu";
    if (stan_host_write_vtu_components(path.c_str(), v.n_nodes, v.xyz, nullptr, v.n_elem, v.conn, 2, names, comps, point.data(), 0, nullptr,
                                       nullptr))
        throw std::runtime_error("cannot write " + path);
}

void SolverFunctions::Export_Step_Vtu(SparseMatrixHandle &K, const std::vector<int32_t> &red, const double *uva, size_t N,
                                      const std::string &prefix, int step) const {
    const MeshView v(K.flat);
    static const char *const names[9] = {"Displacement X", "Displacement Y", "Displacement Z", "Velocity X", "Velocity Y", "Velocity Z",
                                         "Acceleration X", "Acceleration Y", "Acceleration Z"};
    std::vector<double> point(9 * (size_t)v.n_nodes), disp;
    for (int q = 0; q < 3; q++) {
        std::vector<double> nodal = Nodal_Vector(K, uva + (size_t)q * N, red);
        for (int64_t n = 0; n < v.n_nodes; n++)
            for (int c = 0; c < 3; c++) point[(size_t)(3 * q + c) * (size_t)v.n_nodes + (size_t)n] = nodal[(size_t)(3 * n + c)];
        if (q == 0) disp.swap(nodal);
    }
    char num[16];
    snprintf(num, sizeof num, "%04d", step);
    const std::string path = prefix + "_step_" + num + ".vtu";
    if (stan_host_write_vtu(path.c_str(), v.n_nodes, v.xyz, disp.data(), v.n_elem, v.conn, 9, names, point.data(), 0, nullptr, nullptr))
        throw std::runtime_error("cannot write " + path);
}

void SolverFunctions::Buckling(SparseMatrixHandle &K, const std::vector<int32_t> &red, const std::vector<double> &dU, int n_modes, double tol,
                               double solve_eps, std::vector<double> *factor, std::vector<double> *phi, std::vector<double> *rho,
                               stan_buckling_report *rep) const {
    const MeshView v(K.flat);
    const size_t N = n_reduced(red), k = n_modes > 0 ? (size_t)n_modes : 1;
    factor->assign(k, 0.0); rho->assign(k, 0.0); phi->assign(k * N, 0.0);
    stan_matrix *made = nullptr;
    if (stan_hip_geometric_stiffness_hex8(K.ctx, K.K, v.n_nodes, v.xyz, dU.data(), v.node_dof, v.n_elem, v.conn, v.elem_mat, v.elem_type,
                                          v.n_mat, v.mat_E_nu, (int64_t)red.size(), red.data(), &made))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
    const OwnedMatrix G(made);
    if (stan_hip_buckling(K.ctx, K.K, G.get(), n_modes, tol, 0, solve_eps, 0, factor->data(), phi->data(), rho->data(), rep))
        throw std::runtime_error(stan_hip_last_error(K.ctx));
}

const SolverFunctions::ShapeKind SolverFunctions::MODE_SHAPE = {"mode", {"Mode Shape X", "Mode Shape Y", "Mode Shape Z", "Magnitude"}};
const SolverFunctions::ShapeKind SolverFunctions::BUCKLING_SHAPE = {"buckle",
                                                                    {"Buckling Shape X", "Buckling Shape Y", "Buckling Shape Z", "Magnitude"}};

void SolverFunctions::Export_Shape_Vtu(SparseMatrixHandle &K, const std::vector<double> &shape, const std::string &prefix,
                                       const ShapeKind &kind, int number) const {
    const MeshView v(K.flat);
    std::vector<double> point(4 * (size_t)v.n_nodes);
    for (int64_t n = 0; n < v.n_nodes; n++) {
        double s2 = 0;
        for (int c = 0; c < 3; c++) {
            const double x = shape[(size_t)(3 * n + c)];
            point[(size_t)c * (size_t)v.n_nodes + (size_t)n] = x;
            s2 += x * x;
        }
        point[3 * (size_t)v.n_nodes + (size_t)n] = std::sqrt(s2);
    }
    char num[16];
    snprintf(num, sizeof num, "%03d", number);
    const std::string path = prefix + "_" + kind.stem + "_" + num + ".vtu";
    if (stan_host_write_vtu(path.c_str(), v.n_nodes, v.xyz, shape.data(), v.n_elem, v.conn, 4, kind.names, point.data(), 0, nullptr, nullptr))
        throw std::runtime_error("cannot write " + path);
}

void SolverFunctions::Recovery_Stress_Keep(SparseMatrixHandle &K, const std::vector<double> &dU) const {
    const MeshView v(K.flat);
    if (K.results) { stan_hip_results_free(K.results); K.results = nullptr; }
    if (stan_hip_recover_hex8_keep(K.ctx, v.n_nodes, v.xyz, dU.data(), v.n_elem, v.conn, v.elem_mat, v.elem_type, v.n_mat, v.mat_E_nu,
                                   &K.results))
        throw std::runtime_error(stan_hip_last_error(K.ctx));  // HEX8_G1: the reference throws too (Element.cs:242)
}

bool SolverFunctions::ParseScalarNames(const std::string &text, std::vector<int32_t> *sel, std::string *err) {
    sel->clear();
    if (text.empty()) {
        for (int32_t s = 0; s < STAN_SCALAR_COUNT; s++) sel->push_back(s);
        return true;
    }
    for (size_t a = 0; a <= text.size();) {
        size_t b = text.find(',', a);
        if (b == std::string::npos) b = text.size();
        size_t x = a, y = b;
        while (x < y && text[x] == ' ') x++;
        while (y > x && text[y - 1] == ' ') y--;
        const std::string name = text.substr(x, y - x);
        int32_t found = -1;
        for (int32_t s = 0; s < STAN_SCALAR_COUNT; s++)
            if (name == stan_host_scalar_name(s)) found = s;
        if (found < 0) { *err = "unknown result \"" + name + "\" (the names are those of the reference's result box, e.g. \"von Mises Stress\")"; return false; }
        for (int32_t s : *sel)
            if (s == found) { *err = "result \"" + name + "\" listed twice"; return false; }
        sel->push_back(found);
        a = b + 1;
    }
    return true;
}

void SolverFunctions::Export_Vtu(SparseMatrixHandle &K, const std::vector<double> &dU, const std::vector<double> *strain,
                                 const std::vector<double> *stress, const std::string &prefix, const std::vector<int32_t> &sel,
                                 bool cells, double *t_scalars, double *t_write, const std::vector<double> *reaction) const {
    const FlatModel &f = K.flat;
    const int64_t n_nodes = (int64_t)(f.xyz.size() / 3), n_elem = (int64_t)f.elem_mat.size();
    const int32_t n_sel = (int32_t)sel.size();
    auto t0 = clk::now();
    std::vector<double> point((size_t)n_sel * (size_t)n_nodes), cell(cells ? (size_t)n_sel * 3 * (size_t)n_elem : 0);
    const int rc = strain && stress
                       ? stan_hip_result_scalars_hex8(K.ctx, n_nodes, dU.data(), n_elem, f.conn.data(), strain->data(), stress->data(),
                                                      n_sel, sel.data(), point.data(), cells ? cell.data() : nullptr)
                       : stan_hip_results_scalars(K.ctx, K.results, n_nodes, dU.data(), f.conn.data(), n_sel, sel.data(),
                                                  point.data(), cells ? cell.data() : nullptr);
    if (rc) throw std::runtime_error(stan_hip_last_error(K.ctx));
    *t_scalars = secs(t0);
    t0 = clk::now();
    // a point array is named by its result string (Part.cs:931); the cell arrays keep Load_Scalar's prefixes (:266-297)
    std::vector<std::string> cell_names;
    std::vector<const char *> pn, cn;
    for (int32_t s : sel) {
        pn.push_back(stan_host_scalar_name(s));
        if (cells)
            for (const char *pre : {"Max ", "Average ", "Min "}) cell_names.push_back(std::string(pre) + stan_host_scalar_name(s));
    }
    for (const std::string &n : cell_names) cn.push_back(n.c_str());
    if (reaction) {   // by node and direction: reaction[Node.DOF[c]]
        static const char *const rn[3] = {"Reaction Force X", "Reaction Force Y", "Reaction Force Z"};
        point.resize((size_t)(n_sel + 3) * (size_t)n_nodes);
        for (int c = 0; c < 3; c++) {
            pn.push_back(rn[c]);
            for (int64_t n = 0; n < n_nodes; n++)
                point[(size_t)(n_sel + c) * (size_t)n_nodes + (size_t)n] = (*reaction)[(size_t)f.node_dof[(size_t)(3 * n + c)]];
        }
    }
    const std::string path = prefix + "_001.vtu";   // ExportWindow.xaml.cs:100
    if (stan_host_write_vtu(path.c_str(), n_nodes, f.xyz.data(), dU.data(), n_elem, f.conn.data(), (int32_t)pn.size(), pn.data(), point.data(),
                            (int32_t)cn.size(), cn.data(), cell.data()))
        throw std::runtime_error("cannot write " + path);
    *t_write = secs(t0);
}

std::vector<double> SolverFunctions::Nodal_Vector(const SparseMatrixHandle &K, const double *reduced, const std::vector<int32_t> &red) const {
    const std::vector<int32_t> &node_dof = K.flat.node_dof;
    std::vector<double> nodal(node_dof.size());
    ParallelRanges(nodal.size(), [&](size_t a, size_t b) {
        for (size_t k = a; k < b; k++) {
            const size_t d = (size_t)node_dof[k];
            nodal[k] = red[d] == -1 ? 0.0 : reduced[d - (size_t)red[d]];   // Include_BC_DOF's entry d
        }
    });
    return nodal;
}
std::vector<double> SolverFunctions::Include_BC_DOF(const std::vector<double> &A, const std::vector<int32_t> &red) const {
    std::vector<double> full(red.size(), 0.0);  // SolverFunctions.cs:520-538
    for (size_t i = 0; i < red.size(); i++) full[i] = red[i] == -1 ? 0.0 : A[i - (size_t)red[i]];
    return full;
}
std::vector<double> SolverFunctions::Exclude_BC_DOF(const std::vector<double> &A, const std::vector<int32_t> &red) const {
    std::vector<double> out(n_reduced(red), 0.0);  // SolverFunctions.cs:540-555
    for (size_t i = 0; i < red.size(); i++)
        if (red[i] != -1) out[i - (size_t)red[i]] = A[i];
    return out;
}
double SolverFunctions::Vector_Norm(const std::vector<double> &v) const {
    double n = 0;  // SolverFunctions.cs:559-569
    for (double x : v) n += std::pow(x, 2);
    return std::sqrt(n);
}

}  // namespace stan
