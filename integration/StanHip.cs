// StanHip.cs -- P/Invoke surface of libstan_hip.so (include/stan_hip.h), one declaration per exported function.
// New file for src/STAN_Solver/ of galuszkm/STAN; nothing in it depends on the rest of the solver.
//
// Kept in step with the header MECHANICALLY: tests/test_integration_shim.py parses every [DllImport] below and
// every prototype of include/stan_hip.h and fails on a missing function, a different arity, or an argument whose
// managed type is not the blittable image of the C type (int32_t -> int, int64_t -> long, double -> double,
// T* -> T[] / out T / IntPtr, handles -> IntPtr, T** -> out IntPtr); the two [StructLayout] records are checked
// field by field.  No .NET toolchain exists in the build image: this file is checked by that test, not by csc.
using System;
using System.Runtime.InteropServices;

namespace STAN_Solver
{
    /// stan_matrix_info (include/stan_hip.h)
    [StructLayout(LayoutKind.Sequential)]
    public struct StanMatrixInfo
    {
        public long n_dof;
        public long n_reduced;
        public long n_block_rows;
        public long row_begin;
        public long row_end;
        public long n_halo;
        public long n_blocks;
        public long n_slots;
        public long bytes_matrix;
        public int scaled;
        public int max_row_blocks;
        public long n_elements_on_device;
        public int sell_sigma;
        public int folded_slots_permille;
    }

    /// stan_profile (include/stan_hip.h)
    [StructLayout(LayoutKind.Sequential)]
    public struct StanProfile
    {
        public double assemble_ms;
        public double symbolic_ms;
        public double numeric_ms;
        public double cg_ms;
        public double spmv_ms_total;
        public long spmv_launches;
        public long spmv_bytes;
        public long cg_iteration_vector_bytes;
        public int iterations;
        public int termination_type;
        public int assembly_colours;
        public int value_stream;
        public double spmv2_ms_total;
        public long spmv2_launches;
        public long loop_kernel_launches;
        public long loop_collectives;
        public long loop_iterations_enqueued;
        public int placement_candidates;
        public float placement_ms_best;
        public float placement_ms_worst;
        public long col_slots_packed;
        public int placement_moved_vectors;
        public int repacked_streams;
        public long loop_stream_waits;
        public double comm_reduce_ms_total;
        public long comm_reduce_calls;
        public double comm_halo_ms_total;
        public long comm_halo_calls;
        public double rel_residual_recurrence;
        public double rel_residual_fp64;
        public int refine_passes;
        public int fp64_products;
        public double fp64_products_ms;
        public double scalars_cell_ms;
        public double scalars_list_ms;
        public double scalars_point_ms;
        public double forces_elem_ms;
        public double forces_list_ms;
        public double forces_gather_ms;
    }

    /// stan_equilibrium (include/stan_hip.h); filled through the IntPtr argument of stan_hip_internal_forces_hex8
    /// (Marshal.AllocHGlobal(Marshal.SizeOf<StanEquilibrium>()), then Marshal.PtrToStructure)
    [StructLayout(LayoutKind.Sequential)]
    public struct StanEquilibrium
    {
        public double reaction_sum_x, reaction_sum_y, reaction_sum_z;
        public double load_sum_x, load_sum_y, load_sum_z;
        public double fint_sum_x, fint_sum_y, fint_sum_z;
        public double residual_norm2;
        public double load_norm2;
        public double residual_max;
        public long residual_max_dof;
        public long n_fixed;
    }

    /// stan_load_sums (include/stan_hip.h); filled through the IntPtr argument of stan_hip_load_vector_hex8
    [StructLayout(LayoutKind.Sequential)]
    public struct StanLoadSums
    {
        public double load_sum_x, load_sum_y, load_sum_z;
        public double free_sum_x, free_sum_y, free_sum_z;
        public double volume;
        public double area;
        public long n_fixed;
        public long n_faces;
    }

    /// stan_thermal_sums (include/stan_hip.h); filled through the IntPtr argument of stan_hip_thermal_load_hex8
    [StructLayout(LayoutKind.Sequential)]
    public struct StanThermalSums
    {
        public double load_sum_x, load_sum_y, load_sum_z;
        public double free_sum_x, free_sum_y, free_sum_z;
        public double volume;
        public double dT_integral;
        public long n_fixed;
    }

    /// stan_mass_sums (include/stan_hip.h); filled through the IntPtr argument of stan_hip_lumped_mass_hex8
    [StructLayout(LayoutKind.Sequential)]
    public struct StanMassSums
    {
        public double total_mass;
        public double volume;
        public double free_sum_x, free_sum_y, free_sum_z;
        public double fixed_sum_x, fixed_sum_y, fixed_sum_z;
        public long n_fixed;
    }

    /// stan_modes_report (include/stan_hip.h); filled through the IntPtr argument of stan_hip_modes
    [StructLayout(LayoutKind.Sequential)]
    public struct StanModesReport
    {
        public int block;
        public int outer;
        public int converged;
        public int cg_worst_type;
        public long cg_iterations;
        public double max_rho;
        public double solve_ms;
        public double product_ms;
        public double block_ms;
        public double gram_ms;
        public double rotate_ms;
    }

    /// stan_transient_report (include/stan_hip.h); filled through the IntPtr argument of stan_hip_transient
    [StructLayout(LayoutKind.Sequential)]
    public struct StanTransientReport
    {
        public int steps;
        public int failed_step;
        public int cg_worst_type;
        public int cg_min_iterations;
        public int cg_max_iterations;
        public int reserved;
        public long cg_iterations;
        public double sigma;
        public double shift_ms;
        public double solve_ms;
        public double product_ms;
        public double step_ms;
        public double predict_ms;
        public double correct_ms;
    }

    /// stan_explicit_report (include/stan_hip.h); filled through the IntPtr argument of stan_hip_explicit
    [StructLayout(LayoutKind.Sequential)]
    public struct StanExplicitReport
    {
        public int steps;
        public int first_nonfinite_step;
        public double lambda_upper;
        public double lambda_power;
        public double dt_stable;
        public double product_ms;
        public double update_ms;
        public double bound_ms;
        public double power_ms;
    }

    /// stan_harmonic_report (include/stan_hip.h); filled through the IntPtr argument of stan_hip_harmonic
    [StructLayout(LayoutKind.Sequential)]
    public struct StanHarmonicReport
    {
        public int n_modes;
        public int n_freq;
        public long peak_dof;
        public double peak;
        public int peak_freq;
        public int static_correction;
        public double project_ms;
        public double sweep_ms;
        public double snap_ms;
        public double probe_ms;
    }

    internal static class StanHipNative
    {
        // "stan_hip" resolves to libstan_hip.so on Linux (.NET probes lib<name>.so; Mono: <dllmap> or the same probing)
        // and to stan_hip.dll on Windows.  The directory must be on LD_LIBRARY_PATH / next to the executable.
        const string Lib = "stan_hip";

        // error codes, element types, precision modes, options (the #defines of the header)
        internal const int STAN_OK = 0, STAN_E_HIP = -1, STAN_E_ARG = -2, STAN_E_ALLOC = -3, STAN_E_DETJ = -4,
                           STAN_E_DOF_LAYOUT = -5, STAN_E_VALENCE = -6, STAN_E_COMM = -7, STAN_E_UNSUPPORTED = -8;
        internal const byte STAN_HEX8_G1 = 1, STAN_HEX8_G2 = 2;
        internal const int STAN_PREC_FP64 = 0, STAN_PREC_MIXED = 1, STAN_PREC_FIXED48 = 2;
        internal const int STAN_OPT_CG_MERIT_STOP = 1, STAN_OPT_CG_RUPDATE = 2, STAN_OPT_SPMV_VARIANT = 3,
                           STAN_OPT_OVERLAP_HALO = 4, STAN_OPT_ASSEMBLY_MODE = 5, STAN_OPT_CG_FUSED_REFRESH = 6,
                           STAN_OPT_POOL = 7, STAN_OPT_PLACEMENT_TRIES = 8, STAN_OPT_POOL_MAX_BYTES = 9,
                           STAN_OPT_CG_SINGLE_REDUCE = 10, STAN_OPT_CG_FOLD_REDUCE = 11, STAN_OPT_VEC_STORE_NT = 12,
                           STAN_OPT_PACKED_COLUMNS = 13, STAN_OPT_CG_DEFER_X = 14, STAN_OPT_SPMV_SMALL = 15,
                           STAN_OPT_PLACEMENT_MAX_BYTES = 16, STAN_OPT_SELL_SIGMA = 17, STAN_OPT_COMM_P2P = 18,
                           STAN_OPT_ROW_FOLDING = 19, STAN_OPT_CG_REFINE = 20, STAN_OPT_CG_LAZY_SCALING = 21,
                           STAN_OPT_VALUE_STREAM_60 = 22, STAN_OPT_CG_X_RING = 23, STAN_OPT_CG_REFRESH_60 = 24;

        // ---- context
        [DllImport(Lib)] internal static extern int stan_hip_init(int device, out IntPtr ctx);
        [DllImport(Lib)] internal static extern int stan_hip_init_multi(int n_devices, int[] devices, out IntPtr ctx);
        [DllImport(Lib)] internal static extern void stan_hip_destroy(IntPtr ctx);
        [DllImport(Lib)] internal static extern IntPtr stan_hip_last_error(IntPtr ctx);
        [DllImport(Lib)] internal static extern long stan_hip_last_bad_element(IntPtr ctx);
        [DllImport(Lib)] internal static extern int stan_hip_set_stream(IntPtr ctx, IntPtr hip_stream);
        [DllImport(Lib)] internal static extern int stan_hip_set_option(IntPtr ctx, int option, long value);
        [DllImport(Lib)] internal static extern int stan_hip_pool_info(IntPtr ctx, out long bytes_parked, out long blocks_parked);
        [DllImport(Lib)] internal static extern int stan_hip_cg_loop_info(IntPtr ctx, out int x_ring_window, out long x_ring_flushes, out int refresh_stream);

        // ---- several processes, one per GPU (a .NET host normally uses stan_hip_init_multi instead)
        [DllImport(Lib)] internal static extern int stan_hip_comm_unique_id([Out] byte[] id);
        [DllImport(Lib)] internal static extern int stan_hip_comm_init(IntPtr ctx, int rank, int nranks, byte[] id);
        [DllImport(Lib)] internal static extern int stan_hip_comm_info(IntPtr ctx, out int rccl_version, out int comm_ranks, out int comm_rank, out int p2p);
        [DllImport(Lib)] internal static extern int stan_hip_comm_library(IntPtr ctx, [Out] byte[] path, long capacity, out int reused);

        // ---- assembly: ParallelAssembly_K (SolverFunctions.cs:117-180)
        [DllImport(Lib)] internal static extern int stan_hip_assemble_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, int[] node_dof, long n_elem, int[] conn, int[] elem_mat,
            byte[] elem_type, int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, out IntPtr outK);
        [DllImport(Lib)] internal static extern int stan_hip_assemble_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_node_dof, long n_elem, IntPtr d_conn, IntPtr d_elem_mat,
            IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, out IntPtr outK);
        [DllImport(Lib)] internal static extern void stan_hip_matrix_free(IntPtr K);

        // ---- solve: LinearSolver_CG (SolverFunctions.cs:270-330)
        [DllImport(Lib)] internal static extern int stan_hip_cg_solve(
            IntPtr ctx, IntPtr K, double[] F, double eps_f, int max_its, int precision_mode, [Out] double[] U,
            out int termination_type, out int iterations, out double rel_residual);
        [DllImport(Lib)] internal static extern int stan_hip_cg_solve_dev(
            IntPtr ctx, IntPtr K, IntPtr d_F, double eps_f, int max_its, int precision_mode, IntPtr d_U,
            out int termination_type, out int iterations, out double rel_residual);

        // ---- several load cases against one K: F, U [n_rhs * N]; termination_type, iterations, rel_residual [n_rhs]
        [DllImport(Lib)] internal static extern int stan_hip_cg_solve_multi(
            IntPtr ctx, IntPtr K, int n_rhs, double[] F, double eps_f, int max_its, int precision_mode, [Out] double[] U,
            [Out] int[] termination_type, [Out] int[] iterations, [Out] double[] rel_residual);
        [DllImport(Lib)] internal static extern int stan_hip_cg_solve_multi_dev(
            IntPtr ctx, IntPtr K, int n_rhs, IntPtr d_F, double eps_f, int max_its, int precision_mode, IntPtr d_U,
            [Out] int[] termination_type, [Out] int[] iterations, [Out] double[] rel_residual);

        // ---- Element.Recovery_Stress + Update_StrainStress (Element.cs:211-246, 257-267)
        [DllImport(Lib)] internal static extern int stan_hip_recover_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, double[] disp, long n_elem, int[] conn, int[] elem_mat,
            byte[] elem_type, int n_mat, double[] mat_E_nu, [Out] double[] strain, [Out] double[] stress);
        [DllImport(Lib)] internal static extern int stan_hip_recover_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_disp, long n_elem, IntPtr d_conn, IntPtr d_elem_mat,
            IntPtr d_elem_type, int n_mat, double[] mat_E_nu, IntPtr d_strain, IntPtr d_stress);

        // ---- Element.Compute_NodalForces + R[DOF] += NodalForces (Element.cs:248-255, Solver.cs:187-196)
        [DllImport(Lib)] internal static extern int stan_hip_nodal_forces_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, double[] disp, int[] node_dof, long n_elem, int[] conn,
            int[] elem_mat, byte[] elem_type, int n_mat, double[] mat_E_nu, long n_dof, [Out] double[] elem_forces,
            [Out] double[] R);

        // ---- internal forces f_int = sum_e int B^T D B u dV, support reactions, equilibrium sums: f_int, reaction [n_dof],
        //      F [N] or null, eq -> StanEquilibrium or IntPtr.Zero; at least one output
        [DllImport(Lib)] internal static extern int stan_hip_internal_forces_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, double[] disp, int[] node_dof, long n_elem, int[] conn, int[] elem_mat,
            byte[] elem_type, int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, double[] F,
            [Out] double[] f_int, [Out] double[] reaction, IntPtr eq);
        [DllImport(Lib)] internal static extern int stan_hip_internal_forces_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_disp, IntPtr d_node_dof, long n_elem, IntPtr d_conn,
            IntPtr d_elem_mat, IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction,
            IntPtr d_F, IntPtr d_f_int, IntPtr d_reaction, IntPtr eq);

        // ---- distributed loads and prescribed displacements: mat_body [n_mat * 3] or null; the face list sorted by
        //      face_elem * 6 + face_id; disp0 [n_nodes * 3] or null; F [N] in/out or null; F_solve [N] (required with disp0);
        //      load_full [n_dof] or null; sums -> StanLoadSums or IntPtr.Zero; at least one output (F is pinned: updated in place)
        [DllImport(Lib)] internal static extern int stan_hip_load_vector_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, int[] node_dof, long n_elem, int[] conn, int[] elem_mat, byte[] elem_type,
            int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, double[] mat_body, long n_faces, int[] face_elem,
            byte[] face_id, double[] face_pressure, double[] disp0, double[] F, [Out] double[] F_solve,
            [Out] double[] load_full, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_load_vector_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_node_dof, long n_elem, IntPtr d_conn, IntPtr d_elem_mat,
            IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, double[] mat_body,
            long n_faces, IntPtr d_face_elem, IntPtr d_face_id, IntPtr d_face_pressure, IntPtr d_disp0, IntPtr d_F,
            IntPtr d_F_solve, IntPtr d_load_full, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_load_vector_times(IntPtr ctx, [Out] double[] ms);

        // ---- thermal loads: mat_alpha [n_mat], dT [n_nodes]; F [N] in/out or null (pinned: updated in place); load_full
        //      [n_dof] or null; sums -> StanThermalSums or IntPtr.Zero; at least one output.  The stress [n_elem * 48] loses
        //      beta dT at its corner's node in xx, yy, zz (pinned: updated in place)
        [DllImport(Lib)] internal static extern int stan_hip_thermal_load_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, int[] node_dof, long n_elem, int[] conn, int[] elem_mat, byte[] elem_type,
            int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, double[] mat_alpha, double[] dT, double[] F,
            [Out] double[] load_full, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_thermal_load_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_node_dof, long n_elem, IntPtr d_conn, IntPtr d_elem_mat,
            IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, double[] mat_alpha,
            IntPtr d_dT, IntPtr d_F, IntPtr d_load_full, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_thermal_stress_hex8(
            IntPtr ctx, long n_nodes, double[] dT, long n_elem, int[] conn, int[] elem_mat, byte[] elem_type, int n_mat,
            double[] mat_E_nu, double[] mat_alpha, double[] stress);
        [DllImport(Lib)] internal static extern int stan_hip_thermal_stress_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_dT, long n_elem, IntPtr d_conn, IntPtr d_elem_mat, IntPtr d_elem_type, int n_mat,
            double[] mat_E_nu, double[] mat_alpha, IntPtr d_stress);
        [DllImport(Lib)] internal static extern int stan_hip_results_thermal_stress(
            IntPtr ctx, IntPtr results, long n_nodes, double[] dT, int[] conn, int[] elem_mat, byte[] elem_type, int n_mat,
            double[] mat_E_nu, double[] mat_alpha);
        [DllImport(Lib)] internal static extern int stan_hip_thermal_load_times(IntPtr ctx, [Out] double[] ms);

        // ---- modal analysis: mat_rho [n_mat]; M [N], mass_node [n_nodes] or null; sums -> StanMassSums or IntPtr.Zero.  modes:
        //      M [N], lambda / rho [n_modes], phi [n_modes * N]; rep -> StanModesReport or IntPtr.Zero.  The block helpers take
        //      [q * N] blocks, Q [q * q], mask [q] or null; rhs is pinned and updated in place
        [DllImport(Lib)] internal static extern int stan_hip_lumped_mass_hex8(
            IntPtr ctx, long n_nodes, double[] xyz, int[] node_dof, long n_elem, int[] conn, int[] elem_mat, byte[] elem_type,
            int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, double[] mat_rho, [Out] double[] M,
            [Out] double[] mass_node, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_lumped_mass_hex8_dev(
            IntPtr ctx, long n_nodes, IntPtr d_xyz, IntPtr d_node_dof, long n_elem, IntPtr d_conn, IntPtr d_elem_mat,
            IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, double[] mat_rho,
            IntPtr d_M, IntPtr d_mass_node, IntPtr sums);
        [DllImport(Lib)] internal static extern int stan_hip_modes(
            IntPtr ctx, IntPtr K, double[] M, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            [Out] double[] lambda, [Out] double[] phi, [Out] double[] rho, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_modes_dev(
            IntPtr ctx, IntPtr K, IntPtr d_M, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            IntPtr d_lambda, IntPtr d_phi, IntPtr d_rho, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_block_gram(
            IntPtr ctx, long N, int q, double[] Z, double[] W, double[] M, [Out] double[] A, [Out] double[] B);
        [DllImport(Lib)] internal static extern int stan_hip_block_rotate(
            IntPtr ctx, long N, int q, double[] Z, double[] W, double[] M, double[] Q, double[] lambda, byte[] mask, int in_place,
            [Out] double[] X, [Out] double[] KX, double[] rhs, [Out] double[] rho2);

        // ---- linear buckling: G = K_g(disp) on K's layout (freed with stan_hip_matrix_free), then the lowest positive load
        //      factors; factor / rho [n_modes], phi [n_modes * N]; rep -> a stan_buckling_report or IntPtr.Zero; s36 [n * 36]
        [DllImport(Lib)] internal static extern int stan_hip_kg_hex8_batch(
            IntPtr ctx, long n, double[] xyz8, double[] u8, double E, double nu, byte[] type, [Out] double[] s36);
        [DllImport(Lib)] internal static extern int stan_hip_geometric_stiffness_hex8(
            IntPtr ctx, IntPtr K, long n_nodes, double[] xyz, double[] disp, int[] node_dof, long n_elem, int[] conn, int[] elem_mat,
            byte[] elem_type, int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, out IntPtr G);
        [DllImport(Lib)] internal static extern int stan_hip_geometric_stiffness_hex8_dev(
            IntPtr ctx, IntPtr K, long n_nodes, IntPtr d_xyz, IntPtr d_disp, IntPtr d_node_dof, long n_elem, IntPtr d_conn,
            IntPtr d_elem_mat, IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, out IntPtr G);
        [DllImport(Lib)] internal static extern int stan_hip_geometric_stiffness_times(IntPtr ctx, [Out] double[] ms);
        [DllImport(Lib)] internal static extern int stan_hip_buckling(
            IntPtr ctx, IntPtr K, IntPtr G, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            [Out] double[] factor, [Out] double[] phi, [Out] double[] rho, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_buckling_dev(
            IntPtr ctx, IntPtr K, IntPtr G, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            IntPtr d_factor, IntPtr d_phi, IntPtr d_rho, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_buckling_rotate(
            IntPtr ctx, long N, int q, double[] Z, double[] W, double[] Y, double[] D, double[] Q, double[] mu,
            [Out] double[] X, [Out] double[] KX, [Out] double[] R, [Out] double[] r2, [Out] double[] kx2);

        // ---- consistent mass: m36 [n * 36]; Mc = the mass on K's layout and sum = A + sigma B (both freed with
        //      stan_hip_matrix_free); mat_rho [n_mat] host memory in both entries; ms [5]; lambda / rho [n_modes], phi
        //      [n_modes * N]; rep -> a stan_buckling_report or IntPtr.Zero
        [DllImport(Lib)] internal static extern int stan_hip_mass_hex8_batch(
            IntPtr ctx, long n, double[] xyz8, double rho, [Out] double[] m36);
        [DllImport(Lib)] internal static extern int stan_hip_consistent_mass_hex8(
            IntPtr ctx, IntPtr K, long n_nodes, double[] xyz, double[] mat_rho, int[] node_dof, long n_elem, int[] conn, int[] elem_mat,
            byte[] elem_type, int n_mat, double[] mat_E_nu, long n_dof, int[] ndof_reduction, out IntPtr Mc);
        [DllImport(Lib)] internal static extern int stan_hip_consistent_mass_hex8_dev(
            IntPtr ctx, IntPtr K, long n_nodes, IntPtr d_xyz, double[] mat_rho, IntPtr d_node_dof, long n_elem, IntPtr d_conn,
            IntPtr d_elem_mat, IntPtr d_elem_type, int n_mat, double[] mat_E_nu, long n_dof, IntPtr d_ndof_reduction, out IntPtr Mc);
        [DllImport(Lib)] internal static extern int stan_hip_consistent_mass_times(IntPtr ctx, [Out] double[] ms);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_axpy(
            IntPtr ctx, IntPtr A, double sigma, IntPtr B, out IntPtr sum);
        [DllImport(Lib)] internal static extern int stan_hip_modes_pencil(
            IntPtr ctx, IntPtr K, IntPtr Mmat, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            [Out] double[] lambda, [Out] double[] phi, [Out] double[] rho, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_modes_pencil_dev(
            IntPtr ctx, IntPtr K, IntPtr Mmat, int n_modes, double tol, int max_outer, double solve_eps, int solve_max_its,
            IntPtr d_lambda, IntPtr d_phi, IntPtr d_rho, IntPtr rep);

        // ---- transient dynamics: M, F, u0, v0 (or null) [N]; curve_t / curve_g [n_curve] or null; probe_dof [n_probe], probe_u
        //      [(n_steps + 1) * n_probe], snaps [n_snap * 3 * N], energy [(n_steps + 1) * 3] or null; rep -> StanTransientReport or
        //      IntPtr.Zero.  The step helpers take coef [8]; u, v, a of correct are pinned and updated in place
        [DllImport(Lib)] internal static extern int stan_hip_matrix_shifted(
            IntPtr ctx, IntPtr K, double sigma, double[] M, out IntPtr shifted);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_shifted_dev(
            IntPtr ctx, IntPtr K, double sigma, IntPtr d_M, out IntPtr shifted);
        [DllImport(Lib)] internal static extern int stan_hip_transient(
            IntPtr ctx, IntPtr K, double[] M, double[] F, double[] u0, double[] v0, double dt, int n_steps, double beta_N,
            double gamma, double alpha_R, double beta_R, int n_curve, double[] curve_t, double[] curve_g, double solve_eps,
            int solve_max_its, int n_probe, int[] probe_dof, [Out] double[] probe_u, int snap_every, [Out] double[] snaps,
            [Out] double[] energy, [Out] double[] u_end, [Out] double[] v_end, [Out] double[] a_end, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_transient_dev(
            IntPtr ctx, IntPtr K, IntPtr d_M, IntPtr d_F, IntPtr d_u0, IntPtr d_v0, double dt, int n_steps, double beta_N,
            double gamma, double alpha_R, double beta_R, int n_curve, double[] curve_t, double[] curve_g, double solve_eps,
            int solve_max_its, int n_probe, IntPtr d_probe_dof, IntPtr d_probe_u, int snap_every, IntPtr d_snaps,
            IntPtr d_energy, IntPtr d_u_end, IntPtr d_v_end, IntPtr d_a_end, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_newmark_predict(
            IntPtr ctx, long N, double[] u, double[] v, double[] a, double[] F, double[] M, double[] Kw, double[] coef, double gF,
            [Out] double[] w, [Out] double[] b);
        [DllImport(Lib)] internal static extern int stan_hip_newmark_correct(
            IntPtr ctx, long N, double[] u_new, double[] u, double[] v, double[] a, double[] coef, double dt, double gamma,
            double[] M, double[] F, double[] Ku, double gF, [Out] double[] energy);

        // ---- explicit dynamics: the arrays as for stan_hip_transient; energy [(n_steps / energy_every + 1) * 3] or null; rep ->
        //      StanExplicitReport or IntPtr.Zero.  The update helper: s and u_next_scaled together or both null, v and a likewise
        [DllImport(Lib)] internal static extern int stan_hip_stable_step(
            IntPtr ctx, IntPtr K, double[] M, int n_power, out double lambda_upper, out double lambda_power, out double dt_stable);
        [DllImport(Lib)] internal static extern int stan_hip_stable_step_dev(
            IntPtr ctx, IntPtr K, IntPtr d_M, int n_power, out double lambda_upper, out double lambda_power, out double dt_stable);
        [DllImport(Lib)] internal static extern int stan_hip_explicit(
            IntPtr ctx, IntPtr K, double[] M, double[] F, double[] u0, double[] v0, double dt, int n_steps, double alpha_R,
            int n_curve, double[] curve_t, double[] curve_g, int n_probe, int[] probe_dof, [Out] double[] probe_u, int snap_every,
            [Out] double[] snaps, int energy_every, [Out] double[] energy, [Out] double[] u_end, [Out] double[] v_end,
            [Out] double[] a_end, int n_power, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_explicit_dev(
            IntPtr ctx, IntPtr K, IntPtr d_M, IntPtr d_F, IntPtr d_u0, IntPtr d_v0, double dt, int n_steps, double alpha_R,
            int n_curve, double[] curve_t, double[] curve_g, int n_probe, IntPtr d_probe_dof, IntPtr d_probe_u, int snap_every,
            IntPtr d_snaps, int energy_every, IntPtr d_energy, IntPtr d_u_end, IntPtr d_v_end, IntPtr d_a_end, int n_power,
            IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_central_update(
            IntPtr ctx, long N, double[] y, double[] s, double[] u, double[] u_prev, double[] M, double[] F, double dt,
            double alpha_R, double gF, long step, [Out] double[] u_next, [Out] double[] u_next_scaled, [Out] double[] v,
            [Out] double[] a, [Out] double[] energy, out long first_nonfinite);

        // ---- frequency response: lambda [n_modes], phi [n_modes * N], omega [n_freq] in rad/s; u_static, zeta, probe, snaps, peak and
        //      peak_idx may be null (peak and peak_idx together); probe [n_freq * n_probe * 2], snaps [n_snap * 2 * N]; rep ->
        //      StanHarmonicReport or IntPtr.Zero
        [DllImport(Lib)] internal static extern int stan_hip_harmonic(
            IntPtr ctx, long N, int n_modes, double[] lambda, double[] phi, double[] F, double[] u_static, double alpha_R,
            double beta_R, double[] zeta, int n_freq, double[] omega, int n_probe, int[] probe_dof, [Out] double[] probe, int n_snap,
            int[] snap_freq, [Out] double[] snaps, [Out] double[] p, [Out] double[] peak, [Out] int[] peak_idx, IntPtr rep);
        [DllImport(Lib)] internal static extern int stan_hip_harmonic_dev(
            IntPtr ctx, long N, int n_modes, IntPtr d_lambda, IntPtr d_phi, IntPtr d_F, IntPtr d_u_static, double alpha_R,
            double beta_R, double[] zeta, int n_freq, double[] omega, int n_probe, IntPtr d_probe_dof, IntPtr d_probe, int n_snap,
            int[] snap_freq, IntPtr d_snaps, IntPtr d_p, IntPtr d_peak, IntPtr d_peak_idx, IntPtr rep);

        // ---- introspection / parity helpers
        [DllImport(Lib)] internal static extern int stan_hip_matrix_info(IntPtr K, out StanMatrixInfo info);
        [DllImport(Lib)] internal static extern int stan_hip_recover_hex8_keep(
            IntPtr ctx, long n_nodes, double[] xyz, double[] disp, long n_elem, int[] conn, int[] elem_mat, byte[] elem_type,
            int n_mat, double[] mat_E_nu, out IntPtr results);
        [DllImport(Lib)] internal static extern int stan_hip_results_map(IntPtr results, long e0, long e1, out IntPtr strain, out IntPtr stress);
        [DllImport(Lib)] internal static extern void stan_hip_results_free(IntPtr results);
        // ---- Part.Load_Scalar (Part.cs:231-528): point [n_sel * n_nodes], cell [n_sel * 3 * n_elem]; either may be null
        [DllImport(Lib)] internal static extern int stan_hip_result_scalars_hex8(
            IntPtr ctx, long n_nodes, double[] disp, long n_elem, int[] conn, double[] strain, double[] stress, int n_sel,
            int[] sel, [Out] double[] point, [Out] double[] cell);
        [DllImport(Lib)] internal static extern int stan_hip_results_scalars(
            IntPtr ctx, IntPtr results, long n_nodes, double[] disp, int[] conn, int n_sel, int[] sel, [Out] double[] point,
            [Out] double[] cell);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_diagonal(IntPtr ctx, IntPtr K, [Out] double[] diag);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_part_info(IntPtr K, int part, out StanMatrixInfo info);
        [DllImport(Lib)] internal static extern int stan_hip_ke_hex8(IntPtr ctx, double[] xyz8, double E, double nu, int type, [Out] double[] ke576);
        [DllImport(Lib)] internal static extern int stan_hip_ke_hex8_batch(IntPtr ctx, long n, double[] xyz8, double E, double nu, byte[] type, [Out] double[] ke);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_to_csr(IntPtr ctx, IntPtr K, int upper_only, ref long nnz, [Out] long[] rowptr, [Out] int[] col, [Out] double[] val);
        [DllImport(Lib)] internal static extern int stan_hip_matrix_plan(
            IntPtr ctx, IntPtr K, [Out] long[] row_starts, out long n_halo, [Out] int[] halo_glob, out int n_nbr,
            [Out] int[] nbr, [Out] long[] send_off, [Out] int[] send_rows, [Out] long[] recv_off);
        [DllImport(Lib)] internal static extern int stan_hip_spmv_local(IntPtr ctx, IntPtr K, double[] x_local, [Out] double[] y_owned);
        [DllImport(Lib)] internal static extern int stan_hip_spmv(IntPtr ctx, IntPtr K, double[] x, [Out] double[] y);
        [DllImport(Lib)] internal static extern int stan_hip_spmv_bench(IntPtr ctx, IntPtr K, int precision_mode, int reps, out double avg_ms);
        [DllImport(Lib)] internal static extern int stan_hip_stream_bench(IntPtr ctx, IntPtr K, int reps, out double avg_ms, out long bytes);
        [DllImport(Lib)] internal static extern int stan_hip_stream60_roundtrip(IntPtr ctx, long n, double[] input, double[] output, out long refused);
        [DllImport(Lib)] internal static extern int stan_hip_set_profiling(IntPtr ctx, int enabled);
        [DllImport(Lib)] internal static extern int stan_hip_get_profile(IntPtr ctx, out StanProfile profile);
        [DllImport(Lib)] internal static extern int stan_hip_get_profile_rank(IntPtr ctx, int rank, out StanProfile profile);
        [DllImport(Lib)] internal static extern int stan_hip_device_info(IntPtr ctx, int rank, out int hip_ordinal, [Out] byte[] bus_id);
    }

    /// Owner of the context and of K (library-owned objects, explicit free).  One per solve in the reference's
    /// single-shot process; a host that solves repeatedly keeps the context and frees only K.
    public sealed class StanHipMatrix : IDisposable
    {
        internal IntPtr Ctx = IntPtr.Zero, K = IntPtr.Zero;
        // the flat arrays the assembly was called with: the stress recovery takes the same ones
        internal double[] Xyz, MatEnu;
        internal int[] NodeDof, Conn, ElemMat;
        internal byte[] ElemType;

        public void Dispose()
        {
            if (K != IntPtr.Zero) { StanHipNative.stan_hip_matrix_free(K); K = IntPtr.Zero; }
            if (Ctx != IntPtr.Zero) { StanHipNative.stan_hip_destroy(Ctx); Ctx = IntPtr.Zero; }
        }
    }
}
