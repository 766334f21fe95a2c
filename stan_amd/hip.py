"""ctypes binding of libstan_hip.so (include/stan_hip.h).

This is plumbing for tests, bench.py and __graft_entry__: the product is the
shared library.  There is NO CPU fallback: loading fails loudly if the library
has not been built, and stan_hip_init fails if no GPU is present.

load() imports torch first (when installed) so that this library and torch share ONE HIP
runtime: torch bundles its own libamdhip64.so.7 and librccl.so.1.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STAN_HIP_LIB") or os.path.join(_HERE, "lib", "libstan_hip.so")

HEX8_G1, HEX8_G2 = 1, 2
N_SCALARS = 24   # STAN_SCALAR_COUNT; indices as include/stan_hip.h's STAN_SCALAR_*
PREC_FP64, PREC_MIXED, PREC_FIXED48 = 0, 1, 2
OPT_CG_MERIT_STOP, OPT_CG_RUPDATE, OPT_SPMV_VARIANT, OPT_OVERLAP_HALO, OPT_ASSEMBLY_MODE = 1, 2, 3, 4, 5
OPT_CG_FUSED_REFRESH = 6
OPT_POOL = 7
OPT_PLACEMENT_TRIES = 8
OPT_POOL_MAX_BYTES = 9
OPT_CG_SINGLE_REDUCE = 10
OPT_CG_FOLD_REDUCE = 11
OPT_VEC_STORE_NT = 12
OPT_PACKED_COLUMNS = 13
OPT_CG_DEFER_X = 14
OPT_SPMV_SMALL = 15
OPT_PLACEMENT_MAX_BYTES = 16
OPT_SELL_SIGMA = 17
OPT_COMM_P2P = 18
OPT_ROW_FOLDING = 19
OPT_CG_REFINE = 20
OPT_CG_LAZY_SCALING = 21
OPT_VALUE_STREAM_60 = 22
OPT_CG_X_RING = 23
OPT_CG_REFRESH_60 = 24
VALUE_STREAM_60 = 3   # Profile.value_stream of an fp64 solve whose plain products read the lossless 60-bit stream
E_HIP, E_ARG, E_ALLOC, E_DETJ, E_DOF_LAYOUT, E_VALENCE, E_COMM, E_UNSUPPORTED = (
    -1, -2, -3, -4, -5, -6, -7, -8)

EXPORTS = [
    "stan_hip_init", "stan_hip_init_multi", "stan_hip_destroy", "stan_hip_last_error", "stan_hip_last_bad_element",
    "stan_hip_set_stream", "stan_hip_comm_unique_id", "stan_hip_comm_init",
    "stan_hip_assemble_hex8", "stan_hip_assemble_hex8_dev", "stan_hip_matrix_free",
    "stan_hip_cg_solve", "stan_hip_cg_solve_dev", "stan_hip_cg_solve_multi", "stan_hip_cg_solve_multi_dev", "stan_hip_matrix_info", "stan_hip_ke_hex8",
    "stan_hip_ke_hex8_batch", "stan_hip_matrix_to_csr", "stan_hip_spmv", "stan_hip_spmv_bench", "stan_hip_stream_bench",
    "stan_hip_stream60_roundtrip",
    "stan_hip_set_profiling", "stan_hip_get_profile", "stan_hip_set_option", "stan_hip_recover_hex8", "stan_hip_recover_hex8_dev",
    "stan_hip_nodal_forces_hex8", "stan_hip_pool_info", "stan_hip_cg_loop_info",
    "stan_hip_matrix_plan", "stan_hip_spmv_local", "stan_hip_comm_info", "stan_hip_comm_library",
    "stan_hip_matrix_part_info", "stan_hip_get_profile_rank", "stan_hip_device_info", "stan_hip_matrix_diagonal",
    "stan_hip_recover_hex8_keep", "stan_hip_results_map", "stan_hip_results_free",
    "stan_hip_result_scalars_hex8", "stan_hip_results_scalars",
    "stan_hip_internal_forces_hex8", "stan_hip_internal_forces_hex8_dev",
    "stan_hip_load_vector_hex8", "stan_hip_load_vector_hex8_dev", "stan_hip_load_vector_times",
    "stan_hip_thermal_load_hex8", "stan_hip_thermal_load_hex8_dev", "stan_hip_thermal_load_times",
    "stan_hip_thermal_stress_hex8", "stan_hip_thermal_stress_hex8_dev", "stan_hip_results_thermal_stress",
    "stan_hip_lumped_mass_hex8", "stan_hip_lumped_mass_hex8_dev", "stan_hip_modes", "stan_hip_modes_dev",
    "stan_hip_block_gram", "stan_hip_block_rotate",
    "stan_hip_matrix_shifted", "stan_hip_matrix_shifted_dev", "stan_hip_transient", "stan_hip_transient_dev",
    "stan_hip_newmark_predict", "stan_hip_newmark_correct",
    "stan_hip_stable_step", "stan_hip_stable_step_dev", "stan_hip_explicit", "stan_hip_explicit_dev", "stan_hip_central_update",
    "stan_hip_harmonic", "stan_hip_harmonic_dev",
    "stan_hip_kg_hex8_batch", "stan_hip_geometric_stiffness_hex8", "stan_hip_geometric_stiffness_hex8_dev",
    "stan_hip_geometric_stiffness_times", "stan_hip_buckling", "stan_hip_buckling_dev", "stan_hip_buckling_rotate",
    "stan_hip_mass_hex8_batch", "stan_hip_consistent_mass_hex8", "stan_hip_consistent_mass_hex8_dev",
    "stan_hip_consistent_mass_times", "stan_hip_matrix_axpy", "stan_hip_modes_pencil", "stan_hip_modes_pencil_dev",
]
# only in the lab build (stan_amd/csrc/lab/stan_hip_lab.h, selected with STAN_HIP_LIB)
LAB_EXPORTS = ["stan_hip_csr_spmv_bench", "stan_hip_lab_placement_map", "stan_hip_lab_placement_variants", "stan_hip_lab_placement_alloc", "stan_hip_lab_placement_rounds", "stan_hip_lab_placement_cross", "stan_hip_lab_incg_penalty", "stan_hip_lab_placement_vecalloc", "stan_hip_lab_placement_vecshape", "stan_hip_lab_pairing_pmc"]


class MatrixInfo(C.Structure):
    _fields_ = [("n_dof", C.c_int64), ("n_reduced", C.c_int64), ("n_block_rows", C.c_int64),
                ("row_begin", C.c_int64), ("row_end", C.c_int64), ("n_halo", C.c_int64),
                ("n_blocks", C.c_int64), ("n_slots", C.c_int64), ("bytes_matrix", C.c_int64),
                ("scaled", C.c_int32), ("max_row_blocks", C.c_int32), ("n_elements_on_device", C.c_int64),
                ("sell_sigma", C.c_int32), ("folded_slots_permille", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("assemble_ms", C.c_double), ("symbolic_ms", C.c_double),
                ("numeric_ms", C.c_double), ("cg_ms", C.c_double), ("spmv_ms_total", C.c_double),
                ("spmv_launches", C.c_int64), ("spmv_bytes", C.c_int64),
                ("cg_iteration_vector_bytes", C.c_int64), ("iterations", C.c_int32),
                ("termination_type", C.c_int32), ("assembly_colours", C.c_int32),
                ("value_stream", C.c_int32), ("spmv2_ms_total", C.c_double), ("spmv2_launches", C.c_int64),
                ("loop_kernel_launches", C.c_int64), ("loop_collectives", C.c_int64),
                ("loop_iterations_enqueued", C.c_int64), ("placement_candidates", C.c_int32),
                ("placement_ms_best", C.c_float), ("placement_ms_worst", C.c_float),
                ("col_slots_packed", C.c_int64), ("placement_moved_vectors", C.c_int32), ("repacked_streams", C.c_int32),
                ("loop_stream_waits", C.c_int64), ("comm_reduce_ms_total", C.c_double),
                ("comm_reduce_calls", C.c_int64), ("comm_halo_ms_total", C.c_double), ("comm_halo_calls", C.c_int64),
                ("rel_residual_recurrence", C.c_double), ("rel_residual_fp64", C.c_double), ("refine_passes", C.c_int32),
                ("fp64_products", C.c_int32), ("fp64_products_ms", C.c_double),
                ("scalars_cell_ms", C.c_double), ("scalars_list_ms", C.c_double), ("scalars_point_ms", C.c_double),
                ("forces_elem_ms", C.c_double), ("forces_list_ms", C.c_double), ("forces_gather_ms", C.c_double)]


class _Sums(C.Structure):
    """the result structures of sums: as_dict() gives the 3-vectors (*_sum) as lists"""

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.endswith("_sum") else getattr(self, k)) for k, _ in self._fields_}


class Equilibrium(_Sums):
    """stan_equilibrium (include/stan_hip.h)"""
    _fields_ = [("reaction_sum", C.c_double * 3), ("load_sum", C.c_double * 3), ("fint_sum", C.c_double * 3),
                ("residual_norm2", C.c_double), ("load_norm2", C.c_double), ("residual_max", C.c_double),
                ("residual_max_dof", C.c_int64), ("n_fixed", C.c_int64)]


class LoadSums(_Sums):
    """stan_load_sums (include/stan_hip.h)"""
    _fields_ = [("load_sum", C.c_double * 3), ("free_sum", C.c_double * 3), ("volume", C.c_double), ("area", C.c_double),
                ("n_fixed", C.c_int64), ("n_faces", C.c_int64)]


class ThermalSums(_Sums):
    """stan_thermal_sums (include/stan_hip.h)"""
    _fields_ = [("load_sum", C.c_double * 3), ("free_sum", C.c_double * 3), ("volume", C.c_double), ("dT_integral", C.c_double),
                ("n_fixed", C.c_int64)]


class MassSums(_Sums):
    """stan_mass_sums (include/stan_hip.h)"""
    _fields_ = [("total_mass", C.c_double), ("volume", C.c_double), ("free_sum", C.c_double * 3), ("fixed_sum", C.c_double * 3),
                ("n_fixed", C.c_int64)]


class ModesReport(C.Structure):
    """stan_modes_report (include/stan_hip.h)"""
    _fields_ = [("block", C.c_int32), ("outer", C.c_int32), ("converged", C.c_int32), ("cg_worst_type", C.c_int32),
                ("cg_iterations", C.c_int64), ("max_rho", C.c_double), ("solve_ms", C.c_double), ("product_ms", C.c_double),
                ("block_ms", C.c_double), ("gram_ms", C.c_double), ("rotate_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BucklingReport(C.Structure):
    """stan_buckling_report (include/stan_hip.h)"""
    _fields_ = [("block", C.c_int32), ("outer", C.c_int32), ("converged", C.c_int32), ("n_positive", C.c_int32),
                ("cg_worst_type", C.c_int32), ("reserved", C.c_int32), ("cg_iterations", C.c_int64),
                ("lowest_negative_factor", C.c_double), ("max_rho", C.c_double), ("solve_ms", C.c_double),
                ("product_ms", C.c_double), ("block_ms", C.c_double), ("gram_ms", C.c_double), ("rotate_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TransientReport(C.Structure):
    """stan_transient_report (include/stan_hip.h)"""
    _fields_ = [("steps", C.c_int32), ("failed_step", C.c_int32), ("cg_worst_type", C.c_int32), ("cg_min_iterations", C.c_int32),
                ("cg_max_iterations", C.c_int32), ("reserved", C.c_int32), ("cg_iterations", C.c_int64), ("sigma", C.c_double),
                ("shift_ms", C.c_double), ("solve_ms", C.c_double), ("product_ms", C.c_double), ("step_ms", C.c_double),
                ("predict_ms", C.c_double), ("correct_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ExplicitReport(C.Structure):
    """stan_explicit_report (include/stan_hip.h)"""
    _fields_ = [("steps", C.c_int32), ("first_nonfinite_step", C.c_int32), ("lambda_upper", C.c_double), ("lambda_power", C.c_double),
                ("dt_stable", C.c_double), ("product_ms", C.c_double), ("update_ms", C.c_double), ("bound_ms", C.c_double),
                ("power_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class HarmonicReport(C.Structure):
    """stan_harmonic_report (include/stan_hip.h)"""
    _fields_ = [("n_modes", C.c_int32), ("n_freq", C.c_int32), ("peak_dof", C.c_int64), ("peak", C.c_double), ("peak_freq", C.c_int32),
                ("static_correction", C.c_int32), ("project_ms", C.c_double), ("sweep_ms", C.c_double), ("snap_ms", C.c_double),
                ("probe_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def newmark_coef(dt, beta_N=0.25, gamma=0.5, alpha_R=0.0, beta_R=0.0):
    """coef [8] of stan_hip_newmark_predict / _correct: a0 .. a5 in the expressions of include/stan_hip.h, alpha_R, beta_R."""
    return np.array([1.0 / (beta_N * dt * dt), gamma / (beta_N * dt), 1.0 / (beta_N * dt), 1.0 / (2.0 * beta_N) - 1.0,
                     gamma / beta_N - 1.0, dt * (gamma / (2.0 * beta_N) - 1.0), alpha_R, beta_R])


class StanHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libstan_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """dlopen the library (works without a GPU; compute calls do not)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % LIB_PATH)
        # torch bundles its own libamdhip64.so.7 / librccl.so.1.  If this library came first it
        # would pull in /opt/rocm's copies and a later `import torch` would add a SECOND HIP
        # runtime to the process (RCCL then fails with "no ROCm-capable device").  Loading
        # torch first makes both share one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.stan_hip_last_error.restype = C.c_char_p
        _lib.stan_hip_last_bad_element.restype = C.c_int64
        _lib.stan_hip_destroy.restype = None
        _lib.stan_hip_matrix_free.restype = None
    return _lib


def _ptr(a, t):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(t))


def _dev(p, t):
    """device pointer given as int (torch tensor.data_ptr())"""
    return C.cast(C.c_void_p(int(p)), C.POINTER(t))


def _opt(p, t=C.c_double):
    """an optional device pointer: None stays None (NULL)"""
    return None if p is None else _dev(p, t)


_MESH = dict(xyz=np.float64, disp=np.float64, node_dof=np.int32, conn=np.int32, elem_mat=np.int32, elem_type=np.uint8,
             mat_E_nu=np.float64, red=np.int32)


def _mesh(**arrays):
    """The mesh arrays an entry takes, by name and in the order given, as the ABI wants them: C-contiguous, its type, conn
    [n_elem, 8], mat_E_nu [n_mat, 2]."""
    out = {k: np.ascontiguousarray(a, dtype=_MESH[k]) for k, a in arrays.items()}
    return [a.reshape(-1, 8 if k == "conn" else 2) if k in ("conn", "mat_E_nu") else a for k, a in out.items()]


class Context:
    def __init__(self, device=0, devices=None):
        """device: one GPU.  devices=[...]: ONE handle driving several GPUs from this process
        (stan_hip_init_multi; ordinals may repeat only with the test transport tests/fake_rccl)."""
        self.lib = load()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            rc = self.lib.stan_hip_init_multi(C.c_int(len(devices)), arr, C.byref(h))
        else:
            rc = self.lib.stan_hip_init(C.c_int(device), C.byref(h))
        if rc != 0:
            self.lib.stan_hip_last_error.argtypes = [C.c_void_p]
            msg = self.lib.stan_hip_last_error(None)
            raise StanHipError(rc, msg.decode() if msg else "stan_hip_init failed")
        self.h = h
        self.lib.stan_hip_last_error.argtypes = [C.c_void_p]
        self.lib.stan_hip_last_bad_element.argtypes = [C.c_void_p]
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.stan_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise StanHipError(rc, self.lib.stan_hip_last_error(self.h).decode())

    def last_bad_element(self):
        return int(self.lib.stan_hip_last_bad_element(self.h))

    def set_stream(self, stream_ptr):
        self._chk(self.lib.stan_hip_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_option(self, option, value):
        self._chk(self.lib.stan_hip_set_option(self.h, C.c_int32(option), C.c_int64(value)))

    def set_profiling(self, on=True):
        self._chk(self.lib.stan_hip_set_profiling(self.h, C.c_int32(1 if on else 0)))

    def stream60_roundtrip(self, values):
        """(the doubles as the products would decode them from the 60-bit stream, entries the encoder refused)"""
        values = np.ascontiguousarray(values, dtype=np.float64)
        out, refused = np.zeros_like(values), C.c_int64(0)
        self._chk(self.lib.stan_hip_stream60_roundtrip(self.h, C.c_int64(values.size), _ptr(values, C.c_double),
                                                       _ptr(out, C.c_double), C.byref(refused)))
        return out, refused.value

    def profile(self):
        p = Profile()
        self._chk(self.lib.stan_hip_get_profile(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}

    def profile_rank(self, rank):
        """Profile of one rank of a multi-device handle (profile() reports rank 0's)."""
        p = Profile()
        self._chk(self.lib.stan_hip_get_profile_rank(self.h, C.c_int32(rank), C.byref(p)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}

    def device_info(self, rank=0):
        """(HIP ordinal, PCI bus id) of the device a rank drives."""
        o, b = C.c_int32(-1), C.create_string_buffer(32)
        self._chk(self.lib.stan_hip_device_info(self.h, C.c_int32(rank), C.byref(o), b))
        return o.value, b.value.decode()

    def pool_info(self):
        """(bytes, blocks) of device memory the context keeps parked for reuse (OPT_POOL)."""
        b, n = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.stan_hip_pool_info(self.h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def cg_loop_info(self):
        """(window W, flush launches, refresh stream) of the last solve: W of OPT_CG_X_RING, 0 when the loop formed x every
        iteration; the value stream its fused refresh passes read (OPT_CG_REFRESH_60), -1 when there were none."""
        w, n, s = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
        self._chk(self.lib.stan_hip_cg_loop_info(self.h, C.byref(w), C.byref(n), C.byref(s)))
        return w.value, n.value, s.value

    def cg_x_ring_info(self):
        """(window W, flush launches) of OPT_CG_X_RING in the last solve; W = 0: the loop formed x every iteration."""
        return self.cg_loop_info()[:2]

    # -- multi-GPU -----------------------------------------------------------------
    def unique_id(self):
        buf = C.create_string_buffer(128)
        rc = self.lib.stan_hip_comm_unique_id(buf)
        if rc != 0:
            raise StanHipError(rc, "ncclGetUniqueId failed")
        return bytes(buf.raw)

    def comm_init(self, rank, nranks, uid):
        """uid=None: detached rank (no collectives) for shard/plan checks."""
        if uid is None:
            self._chk(self.lib.stan_hip_comm_init(self.h, C.c_int(rank), C.c_int(nranks), None))
            return
        buf = C.create_string_buffer(bytes(uid), 128)
        self._chk(self.lib.stan_hip_comm_init(self.h, C.c_int(rank), C.c_int(nranks), buf))

    def comm_info(self):
        """What the sharded CG exchanges over: RCCL version code, the communicator's rank count / rank, p2p flag."""
        v, n, r, p = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.stan_hip_comm_info(self.h, C.byref(v), C.byref(n), C.byref(r), C.byref(p)))
        buf, reused = C.create_string_buffer(4096), C.c_int32(0)
        self._chk(self.lib.stan_hip_comm_library(self.h, buf, C.c_int64(4096), C.byref(reused)))
        return dict(rccl_version=v.value, comm_ranks=n.value, comm_rank=r.value, p2p=bool(p.value),
                    library=buf.value.decode(), library_reused=bool(reused.value))

    # -- K_e (debug / parity) ---------------------------------------------------------
    def ke_hex8(self, xyz8, E, nu, etype):
        xyz8 = np.ascontiguousarray(xyz8, dtype=np.float64).reshape(24)
        out = np.zeros(576)
        self._chk(self.lib.stan_hip_ke_hex8(self.h, _ptr(xyz8, C.c_double), C.c_double(E),
                                            C.c_double(nu), C.c_int32(etype),
                                            _ptr(out, C.c_double)))
        return out.reshape(24, 24)

    def ke_hex8_batch(self, xyz8, E, nu, etypes):
        xyz8 = np.ascontiguousarray(xyz8, dtype=np.float64).reshape(-1, 24)
        n = xyz8.shape[0]
        etypes = np.ascontiguousarray(etypes, dtype=np.uint8)
        out = np.zeros((n, 576))
        self._chk(self.lib.stan_hip_ke_hex8_batch(self.h, C.c_int64(n), _ptr(xyz8, C.c_double),
                                                  C.c_double(E), C.c_double(nu),
                                                  _ptr(etypes, C.c_uint8), _ptr(out, C.c_double)))
        return out.reshape(n, 24, 24)

    def kg_hex8_batch(self, xyz8, u8, E, nu, etypes):
        """stan_hip_kg_hex8_batch: s36 [n, 36], the upper triangle of the element scalars of the geometric stiffness."""
        xyz8 = np.ascontiguousarray(xyz8, dtype=np.float64).reshape(-1, 24)
        u8 = np.ascontiguousarray(u8, dtype=np.float64).reshape(-1, 24)
        n = xyz8.shape[0]
        etypes = np.ascontiguousarray(etypes, dtype=np.uint8).reshape(-1)
        if u8.shape[0] != n or etypes.shape[0] != n:
            raise ValueError("kg_hex8_batch: xyz8, u8 must be [n, 24] and etypes [n]")
        out = np.zeros((n, 36))
        self._chk(self.lib.stan_hip_kg_hex8_batch(self.h, C.c_int64(n), _ptr(xyz8, C.c_double), _ptr(u8, C.c_double),
                                                  C.c_double(E), C.c_double(nu), _ptr(etypes, C.c_uint8), _ptr(out, C.c_double)))
        return out

    def geometric_stiffness_times(self):
        """dict(kg_elem_ms, kg_layout_ms, kg_list_ms, kg_gather_ms) of the last geometric-stiffness call (profiling enabled)."""
        ms = (C.c_double * 4)()
        self._chk(self.lib.stan_hip_geometric_stiffness_times(self.h, ms))
        return dict(kg_elem_ms=ms[0], kg_layout_ms=ms[1], kg_list_ms=ms[2], kg_gather_ms=ms[3])

    def buckling(self, K, G, n_modes, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """stan_hip_buckling: the n_modes lowest positive load factors of (K + lambda G) phi = 0, G = K.geometric_stiffness(...).
        Returns (factor [n_modes], phi [n_modes, N], rho [n_modes], report dict of stan_buckling_report)."""
        N = K.info()["n_reduced"]
        k = max(int(n_modes), 1)
        fac, phi, rho, rep = np.zeros(k), np.zeros((k, N)), np.zeros(k), BucklingReport()
        self._chk(self.lib.stan_hip_buckling(
            self.h, K.k, G.k, C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer), C.c_double(solve_eps),
            C.c_int32(solve_max_its), _ptr(fac, C.c_double), _ptr(phi, C.c_double), _ptr(rho, C.c_double), C.byref(rep)))
        return fac, phi, rho, rep.as_dict()

    def buckling_dev(self, K, G, n_modes, d_factor, d_phi, d_rho, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """d_factor / d_rho [n_modes], d_phi [n_modes, N]: device pointers (ints).  Returns the report dict."""
        rep = BucklingReport()
        self._chk(self.lib.stan_hip_buckling_dev(
            self.h, K.k, G.k, C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer), C.c_double(solve_eps),
            C.c_int32(solve_max_its), _opt(d_factor), _opt(d_phi), _opt(d_rho), C.byref(rep)))
        return rep.as_dict()

    def mass_hex8_batch(self, xyz8, rho):
        """stan_hip_mass_hex8_batch: m36 [n, 36], the upper triangle of the element scalars of the consistent mass."""
        xyz8 = np.ascontiguousarray(xyz8, dtype=np.float64).reshape(-1, 24)
        n = xyz8.shape[0]
        out = np.zeros((n, 36))
        self._chk(self.lib.stan_hip_mass_hex8_batch(self.h, C.c_int64(n), _ptr(xyz8, C.c_double), C.c_double(rho), _ptr(out, C.c_double)))
        return out

    def consistent_mass_times(self):
        """dict(cm_elem_ms, cm_layout_ms, cm_list_ms, cm_gather_ms) of the last consistent-mass call and axpy_ms of the last
        Matrix.axpy (profiling enabled)."""
        ms = (C.c_double * 5)()
        self._chk(self.lib.stan_hip_consistent_mass_times(self.h, ms))
        return dict(cm_elem_ms=ms[0], cm_layout_ms=ms[1], cm_list_ms=ms[2], cm_gather_ms=ms[3], axpy_ms=ms[4])

    def modes_pencil(self, K, Mmat, n_modes, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """stan_hip_modes_pencil: the n_modes lowest eigenpairs of K phi = lambda Mmat phi, Mmat = K.consistent_mass(...).
        Returns (lambda [n_modes], phi [n_modes, N], rho [n_modes], report dict of stan_buckling_report)."""
        N = K.info()["n_reduced"]
        k = max(int(n_modes), 1)
        lam, phi, rho, rep = np.zeros(k), np.zeros((k, N)), np.zeros(k), BucklingReport()
        self._chk(self.lib.stan_hip_modes_pencil(
            self.h, K.k, Mmat.k, C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer), C.c_double(solve_eps),
            C.c_int32(solve_max_its), _ptr(lam, C.c_double), _ptr(phi, C.c_double), _ptr(rho, C.c_double), C.byref(rep)))
        return lam, phi, rho, rep.as_dict()

    def modes_pencil_dev(self, K, Mmat, n_modes, d_lambda, d_phi, d_rho, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """d_lambda / d_rho [n_modes], d_phi [n_modes, N]: device pointers (ints).  Returns the report dict."""
        rep = BucklingReport()
        self._chk(self.lib.stan_hip_modes_pencil_dev(
            self.h, K.k, Mmat.k, C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer), C.c_double(solve_eps),
            C.c_int32(solve_max_its), _opt(d_lambda), _opt(d_phi), _opt(d_rho), C.byref(rep)))
        return rep.as_dict()

    def buckling_rotate(self, Z, W, Y, D, Q, mu):
        """stan_hip_buckling_rotate: (X, KX, R, r2, kx2).  Z, W, Y [q, N], D [N], Q [q, q], mu [q]."""
        Z, W, Y, Q = (np.ascontiguousarray(x, dtype=np.float64) for x in (Z, W, Y, Q))
        D = np.ascontiguousarray(D, dtype=np.float64).reshape(-1)
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
        if Z.ndim != 2 or W.shape != Z.shape or Y.shape != Z.shape or D.shape[0] != Z.shape[1] or Q.shape != (Z.shape[0],) * 2 or mu.shape[0] != Z.shape[0]:
            raise ValueError("buckling_rotate: Z, W, Y must be [q, N], D [N], Q [q, q], mu [q]")
        q, N = Z.shape
        X, KX, R, r2, kx2 = np.zeros((q, N)), np.zeros((q, N)), np.zeros((q, N)), np.zeros(q), np.zeros(q)
        self._chk(self.lib.stan_hip_buckling_rotate(
            self.h, C.c_int64(N), C.c_int32(q), _ptr(Z, C.c_double), _ptr(W, C.c_double), _ptr(Y, C.c_double), _ptr(D, C.c_double),
            _ptr(Q, C.c_double), _ptr(mu, C.c_double), _ptr(X, C.c_double), _ptr(KX, C.c_double), _ptr(R, C.c_double),
            _ptr(r2, C.c_double), _ptr(kx2, C.c_double)))
        return X, KX, R, r2, kx2

    # -- stress recovery ---------------------------------------------------------------
    def recover_hex8(self, xyz, disp, conn, elem_mat, elem_type, mat_E_nu):
        xyz, disp, conn, elem_mat, elem_type, mat_E_nu = _mesh(
            xyz=xyz, disp=disp, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu)
        ne = conn.shape[0]
        strain = np.zeros((ne, 8, 6))
        stress = np.zeros((ne, 8, 6))
        self._chk(self.lib.stan_hip_recover_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(disp, C.c_double),
            C.c_int64(ne), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32),
            _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            _ptr(strain, C.c_double), _ptr(stress, C.c_double)))
        return strain, stress

    def recover_hex8_dev(self, n_nodes, d_xyz, d_disp, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, d_strain, d_stress):
        """All d_* are device pointers (ints, e.g. torch tensor.data_ptr()); d_strain, d_stress: [n_elem, 8, 6] doubles."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        self._chk(self.lib.stan_hip_recover_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_disp, C.c_double), C.c_int64(n_elem),
            _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), _dev(d_strain, C.c_double), _dev(d_stress, C.c_double)))

    def recover_hex8_keep(self, xyz, disp, conn, elem_mat, elem_type, mat_E_nu):
        """Stress recovery with the results kept on the device(s): returns a Results handle (map(e0, e1), free())."""
        xyz, disp, conn, elem_mat, elem_type, mat_E_nu = _mesh(
            xyz=xyz, disp=disp, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu)
        h = C.c_void_p()
        self._chk(self.lib.stan_hip_recover_hex8_keep(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(disp, C.c_double),
            C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32),
            _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.byref(h)))
        return Results(self, h, conn.shape[0])

    # -- result scalars (Part.Load_Scalar) ------------------------------------------------------
    def _scalars(self, call, disp, conn, sel, point, cell):
        disp = np.ascontiguousarray(disp, dtype=np.float64).reshape(-1, 3)
        conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
        sel = np.ascontiguousarray(range(N_SCALARS) if sel is None else sel, dtype=np.int32).reshape(-1)
        nn, ne, ns = disp.shape[0], conn.shape[0], sel.shape[0]
        pt = np.zeros((ns, nn)) if point else None
        ce = np.zeros((ns, 3, ne)) if cell else None
        self._chk(call(C.c_int64(nn), _ptr(disp, C.c_double), C.c_int64(ne), _ptr(conn, C.c_int32), C.c_int32(ns),
                       _ptr(sel, C.c_int32), _ptr(pt, C.c_double), _ptr(ce, C.c_double)))
        return pt, ce

    def result_scalars(self, disp, conn, strain, stress, sel=None, point=True, cell=True):
        """The scalars `sel` (indices 0..23, default all 24) of stan_hip_result_scalars_hex8 from host arrays
        strain / stress [n_elem, 8, 6]: (point [n_sel, n_nodes], cell [n_sel, 3, n_elem] = max, average, min); an
        output not asked for is None."""
        strain = np.ascontiguousarray(strain, dtype=np.float64)
        stress = np.ascontiguousarray(stress, dtype=np.float64)
        ne = np.asarray(conn).size // 8
        if strain.size != ne * 48 or stress.size != ne * 48:
            raise ValueError("result_scalars: strain / stress must be [n_elem, 8, 6]")
        return self._scalars(
            lambda nn, d, n_e, c, ns, s, pt, ce: self.lib.stan_hip_result_scalars_hex8(
                self.h, nn, d, n_e, c, _ptr(strain, C.c_double), _ptr(stress, C.c_double), ns, s, pt, ce),
            disp, conn, sel, point, cell)

    def nodal_forces_hex8(self, xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu):
        """Element.NodalForces [n_elem,24] and the assembled R [n_dof] (Solver.cs:184-196)."""
        xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu = _mesh(
            xyz=xyz, disp=disp, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu)
        ne, n_dof = conn.shape[0], xyz.shape[0] * 3
        f = np.zeros((ne, 24))
        R = np.zeros(n_dof)
        self._chk(self.lib.stan_hip_nodal_forces_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(disp, C.c_double),
            _ptr(node_dof, C.c_int32), C.c_int64(ne), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32),
            _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            C.c_int64(n_dof), _ptr(f, C.c_double), _ptr(R, C.c_double)))
        return f, R

    # -- internal forces, reactions, equilibrium ------------------------------------------------
    def internal_forces_hex8(self, xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu, red, F=None,
                             f_int=True, reaction=True, eq=True):
        """stan_hip_internal_forces_hex8: (f_int [n_dof], reaction [n_dof], eq Equilibrium) from host arrays; disp is any
        full nodal vector [n_nodes, 3], F the reduced load vector or None (= 0).  An output not asked for is None."""
        xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, disp=disp, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        F = None if F is None else np.ascontiguousarray(F, dtype=np.float64)
        n_dof = red.shape[0]
        if disp.size != xyz.size or (F is not None and F.shape[0] != n_dof - int((red == -1).sum())):
            raise ValueError("internal_forces_hex8: disp must be [n_nodes, 3] and F [n_dof - n_fixed]")
        fi = np.zeros(n_dof) if f_int else None
        re = np.zeros(n_dof) if reaction else None
        q = Equilibrium() if eq else None
        self._chk(self.lib.stan_hip_internal_forces_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(disp, C.c_double), _ptr(node_dof, C.c_int32),
            C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _ptr(red, C.c_int32),
            _ptr(F, C.c_double), _ptr(fi, C.c_double), _ptr(re, C.c_double), C.byref(q) if eq else None))
        return fi, re, q

    def internal_forces_hex8_dev(self, n_nodes, d_xyz, d_disp, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu,
                                 n_dof, d_red, d_F=None, d_f_int=None, d_reaction=None, eq=True):
        """All d_* are device pointers (ints, e.g. torch tensor.data_ptr()); d_F, d_f_int, d_reaction may be None.
        Returns the Equilibrium (None when not asked for)."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        q = Equilibrium() if eq else None
        self._chk(self.lib.stan_hip_internal_forces_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_disp, C.c_double), _dev(d_node_dof, C.c_int32),
            C.c_int64(n_elem), _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32),
            _opt(d_F), _opt(d_f_int), _opt(d_reaction), C.byref(q) if eq else None))
        return q

    # -- distributed loads and prescribed displacements -----------------------------------------
    def load_vector_hex8(self, xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red, mat_body=None, face_elem=None,
                         face_id=None, face_pressure=None, disp0=None, F=None, F_solve=None, load_full=True, sums=True):
        """stan_hip_load_vector_hex8 from host arrays: (F, F_solve, load_full, sums LoadSums).  mat_body [n_mat, 3] or None;
        the face list (face_elem, face_id, face_pressure) sorted by face_elem * 6 + face_id, or None; disp0 [n_nodes, 3] or
        None.  F: the reduced load vector to add to (a copy is returned) or None; F_solve: True / False, default = disp0
        given.  An output not asked for is None."""
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        n_dof = red.shape[0]
        N = n_dof - int((red == -1).sum())
        mb = None if mat_body is None else np.ascontiguousarray(mat_body, dtype=np.float64).reshape(-1, 3)
        if mb is not None and mb.shape[0] != mat_E_nu.shape[0]:
            raise ValueError("load_vector_hex8: mat_body must be [n_mat, 3]")
        fe = None if face_elem is None else np.ascontiguousarray(face_elem, dtype=np.int32).reshape(-1)
        fi = None if face_elem is None else np.ascontiguousarray(face_id, dtype=np.uint8).reshape(-1)
        fp = None if face_elem is None else np.ascontiguousarray(face_pressure, dtype=np.float64).reshape(-1)
        nf = 0 if fe is None else fe.shape[0]
        if fe is not None and not (fi.shape[0] == fp.shape[0] == nf):
            raise ValueError("load_vector_hex8: face_elem, face_id, face_pressure must have one length")
        u0 = None if disp0 is None else np.ascontiguousarray(disp0, dtype=np.float64)
        if u0 is not None and u0.size != xyz.size:
            raise ValueError("load_vector_hex8: disp0 must be [n_nodes, 3]")
        Fo = None if F is None else np.array(F, dtype=np.float64).reshape(-1)
        if Fo is not None and Fo.shape[0] != N:
            raise ValueError("load_vector_hex8: F must be [n_dof - n_fixed]")
        if F_solve is None:
            F_solve = u0 is not None
        Fs = np.zeros(N) if F_solve else None
        lf = np.zeros(n_dof) if load_full else None
        q = LoadSums() if sums else None
        self._chk(self.lib.stan_hip_load_vector_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(node_dof, C.c_int32), C.c_int64(conn.shape[0]),
            _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _ptr(red, C.c_int32), _ptr(mb, C.c_double), C.c_int64(nf),
            _ptr(fe, C.c_int32), _ptr(fi, C.c_uint8), _ptr(fp, C.c_double), _ptr(u0, C.c_double), _ptr(Fo, C.c_double),
            _ptr(Fs, C.c_double), _ptr(lf, C.c_double), C.byref(q) if sums else None))
        return Fo, Fs, lf, q

    def load_vector_hex8_dev(self, n_nodes, d_xyz, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, n_dof, d_red,
                             mat_body=None, n_faces=0, d_face_elem=None, d_face_id=None, d_face_pressure=None, d_disp0=None,
                             d_F=None, d_F_solve=None, d_load_full=None, sums=True):
        """All d_* are device pointers (ints, e.g. torch tensor.data_ptr()) or None; mat_body a host array or None.
        Returns the LoadSums (None when not asked for)."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        mb = None if mat_body is None else np.ascontiguousarray(mat_body, dtype=np.float64).reshape(-1, 3)
        q = LoadSums() if sums else None
        self._chk(self.lib.stan_hip_load_vector_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_node_dof, C.c_int32), C.c_int64(n_elem),
            _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32), _ptr(mb, C.c_double), C.c_int64(n_faces),
            _opt(d_face_elem, C.c_int32), _opt(d_face_id, C.c_uint8), _opt(d_face_pressure), _opt(d_disp0), _opt(d_F),
            _opt(d_F_solve), _opt(d_load_full), C.byref(q) if sums else None))
        return q

    def load_vector_times(self):
        """dict(loads_elem_ms, loads_list_ms, loads_gather_ms) of the last load-vector call (profiling enabled)."""
        ms = (C.c_double * 3)()
        self._chk(self.lib.stan_hip_load_vector_times(self.h, ms))
        return dict(loads_elem_ms=ms[0], loads_list_ms=ms[1], loads_gather_ms=ms[2])

    # -- thermal loads --------------------------------------------------------------------------
    def thermal_load_hex8(self, xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red, mat_alpha, dT, F=None, load_full=True,
                          sums=True):
        """stan_hip_thermal_load_hex8 from host arrays: (F, load_full, sums ThermalSums).  mat_alpha [n_mat], dT [n_nodes]
        (None is passed on as NULL); F: the reduced load vector to add to (a copy is returned) or None.  An output not asked
        for is None."""
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        n_dof = red.shape[0]
        N = n_dof - int((red == -1).sum())
        al = None if mat_alpha is None else np.ascontiguousarray(mat_alpha, dtype=np.float64).reshape(-1)
        if al is not None and al.shape[0] != mat_E_nu.shape[0]:
            raise ValueError("thermal_load_hex8: mat_alpha must be [n_mat]")
        t = None if dT is None else np.ascontiguousarray(dT, dtype=np.float64).reshape(-1)
        if t is not None and t.shape[0] != xyz.shape[0]:
            raise ValueError("thermal_load_hex8: dT must be [n_nodes]")
        Fo = None if F is None else np.array(F, dtype=np.float64).reshape(-1)
        if Fo is not None and Fo.shape[0] != N:
            raise ValueError("thermal_load_hex8: F must be [n_dof - n_fixed]")
        lf = np.zeros(n_dof) if load_full else None
        q = ThermalSums() if sums else None
        self._chk(self.lib.stan_hip_thermal_load_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(node_dof, C.c_int32), C.c_int64(conn.shape[0]),
            _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _ptr(red, C.c_int32), _ptr(al, C.c_double), _ptr(t, C.c_double),
            _ptr(Fo, C.c_double), _ptr(lf, C.c_double), C.byref(q) if sums else None))
        return Fo, lf, q

    def thermal_load_hex8_dev(self, n_nodes, d_xyz, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, n_dof, d_red,
                              mat_alpha, d_dT, d_F=None, d_load_full=None, sums=True):
        """All d_* are device pointers (ints, e.g. torch tensor.data_ptr()) or None; mat_alpha a host array.  Returns the
        ThermalSums (None when not asked for)."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        al = None if mat_alpha is None else np.ascontiguousarray(mat_alpha, dtype=np.float64).reshape(-1)
        q = ThermalSums() if sums else None
        self._chk(self.lib.stan_hip_thermal_load_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_node_dof, C.c_int32), C.c_int64(n_elem),
            _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32), _ptr(al, C.c_double), _opt(d_dT), _opt(d_F),
            _opt(d_load_full), C.byref(q) if sums else None))
        return q

    def thermal_load_times(self):
        """dict(thermal_elem_ms, thermal_list_ms, thermal_gather_ms) of the last thermal-load call (profiling enabled)."""
        ms = (C.c_double * 3)()
        self._chk(self.lib.stan_hip_thermal_load_times(self.h, ms))
        return dict(thermal_elem_ms=ms[0], thermal_list_ms=ms[1], thermal_gather_ms=ms[2])

    # -- modal analysis ---------------------------------------------------------------------------
    def lumped_mass_hex8(self, xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red, mat_rho, M=True, mass_node=True, sums=True):
        """stan_hip_lumped_mass_hex8 from host arrays: (M [N], mass_node [n_nodes], sums MassSums).  mat_rho [n_mat] (None is
        passed on as NULL).  An output not asked for is None."""
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        n_dof = red.shape[0]
        N = n_dof - int((red == -1).sum())
        rho = None if mat_rho is None else np.ascontiguousarray(mat_rho, dtype=np.float64).reshape(-1)
        if rho is not None and rho.shape[0] != mat_E_nu.shape[0]:
            raise ValueError("lumped_mass_hex8: mat_rho must be [n_mat]")
        Mo = np.zeros(N) if M else None
        mn = np.zeros(xyz.shape[0]) if mass_node else None
        q = MassSums() if sums else None
        self._chk(self.lib.stan_hip_lumped_mass_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(node_dof, C.c_int32), C.c_int64(conn.shape[0]),
            _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _ptr(red, C.c_int32), _ptr(rho, C.c_double), _ptr(Mo, C.c_double),
            _ptr(mn, C.c_double), C.byref(q) if sums else None))
        return Mo, mn, q

    def lumped_mass_hex8_dev(self, n_nodes, d_xyz, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, n_dof, d_red,
                             mat_rho, d_M=None, d_mass_node=None, sums=True):
        """All d_* are device pointers (ints, e.g. torch tensor.data_ptr()) or None; mat_rho a host array.  Returns the
        MassSums (None when not asked for)."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        rho = None if mat_rho is None else np.ascontiguousarray(mat_rho, dtype=np.float64).reshape(-1)
        q = MassSums() if sums else None
        self._chk(self.lib.stan_hip_lumped_mass_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_node_dof, C.c_int32), C.c_int64(n_elem),
            _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]),
            _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32), _ptr(rho, C.c_double), _opt(d_M),
            _opt(d_mass_node), C.byref(q) if sums else None))
        return q

    def block_gram(self, Z, W, M):
        """stan_hip_block_gram: (A, B) [q, q] = Z^T W, Z^T (M o Z) for block vectors Z, W [q, N] and the diagonal M [N]."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        if Z.ndim != 2 or W.shape != Z.shape or M.shape[0] != Z.shape[1]:
            raise ValueError("block_gram: Z, W must be [q, N] and M [N]")
        q, N = Z.shape
        A, B = np.zeros((q, q)), np.zeros((q, q))
        self._chk(self.lib.stan_hip_block_gram(self.h, C.c_int64(N), C.c_int32(q), _ptr(Z, C.c_double), _ptr(W, C.c_double),
                                               _ptr(M, C.c_double), _ptr(A, C.c_double), _ptr(B, C.c_double)))
        return A, B

    def block_rotate(self, Z, W, M, Q, lam, mask=None, in_place=False, rhs=None):
        """stan_hip_block_rotate: (X, KX, rhs, rho2).  Z, W [q, N], M [N], Q [q, q], lam [q]; mask [q] of 0 / 1 or None; rhs
        [q, N] the array whose unmasked columns are replaced (a copy is returned; None: zeros)."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
        if Z.ndim != 2 or W.shape != Z.shape or M.shape[0] != Z.shape[1] or Q.shape != (Z.shape[0],) * 2 or lam.shape[0] != Z.shape[0]:
            raise ValueError("block_rotate: Z, W must be [q, N], M [N], Q [q, q], lam [q]")
        q, N = Z.shape
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        X, KX, rho2 = np.zeros((q, N)), np.zeros((q, N)), np.zeros(q)
        R = np.zeros((q, N)) if rhs is None else np.array(rhs, dtype=np.float64).reshape(q, N)
        self._chk(self.lib.stan_hip_block_rotate(
            self.h, C.c_int64(N), C.c_int32(q), _ptr(Z, C.c_double), _ptr(W, C.c_double), _ptr(M, C.c_double), _ptr(Q, C.c_double),
            _ptr(lam, C.c_double), _ptr(mk, C.c_uint8), C.c_int32(int(bool(in_place))), _ptr(X, C.c_double), _ptr(KX, C.c_double),
            _ptr(R, C.c_double), _ptr(rho2, C.c_double)))
        return X, KX, R, rho2

    def harmonic(self, lam, phi, F, omega, u_static=None, alpha_R=0.0, beta_R=0.0, zeta=None, probe_dof=None, snap_freq=None,
                 peak=True, out=None):
        """stan_hip_harmonic: the steady-state response to F e^{i w t} at the circular frequencies omega [n_freq] from the
        M-orthonormal modes lam [k], phi [k, N], with the static correction when u_static = K^-1 F is given.  Returns a dict: p
        [k], probe [n_freq, n_probe, 2] or None, snaps [n_snap, 2, N] or None, peak [N] and peak_idx [N] (int32) or None, report
        (stan_harmonic_report; written on an error too: StanHipError.report).  out: a dict of preallocated arrays under the
        same names, used instead of fresh ones (a refused call must leave them untouched)."""
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        if phi.ndim != 2:
            raise ValueError("harmonic: phi must be [k, N]")
        k, N = phi.shape
        lam, F, omega = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (lam, F, omega))
        us, zt = (None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (u_static, zeta))
        if lam.shape[0] != k or F.shape[0] != N or (us is not None and us.shape[0] != N) or (zt is not None and zt.shape[0] != k):
            raise ValueError("harmonic: lam, zeta must be [k] and F, u_static [N]")
        pd = None if probe_dof is None else np.ascontiguousarray(probe_dof, dtype=np.int32).reshape(-1)
        sf = None if snap_freq is None else np.ascontiguousarray(snap_freq, dtype=np.int32).reshape(-1)
        npr, nsn, nf = (0 if pd is None else pd.shape[0]), (0 if sf is None else sf.shape[0]), omega.shape[0]
        o = dict(out or {})
        pr = o.get("probe", np.zeros((nf, npr, 2)) if npr else None)
        sn = o.get("snaps", np.zeros((nsn, 2, N)) if nsn else None)
        p = o.get("p", None)
        p = np.zeros(k) if p is None else p
        pk = o.get("peak", np.zeros(N) if peak else None)
        pi = o.get("peak_idx", np.zeros(N, dtype=np.int32) if peak else None)
        rep = HarmonicReport()
        rc = self.lib.stan_hip_harmonic(
            self.h, C.c_int64(N), C.c_int32(k), _ptr(lam, C.c_double), _ptr(phi, C.c_double), _ptr(F, C.c_double), _ptr(us, C.c_double),
            C.c_double(alpha_R), C.c_double(beta_R), _ptr(zt, C.c_double), C.c_int32(nf), _ptr(omega, C.c_double), C.c_int32(npr),
            _ptr(pd, C.c_int32), _ptr(pr, C.c_double), C.c_int32(nsn), _ptr(sf, C.c_int32), _ptr(sn, C.c_double), _ptr(p, C.c_double),
            _ptr(pk, C.c_double), _ptr(pi, C.c_int32), C.byref(rep))
        if rc != 0:
            e = StanHipError(rc, self.lib.stan_hip_last_error(self.h).decode())
            e.report = rep.as_dict()
            raise e
        return dict(p=p, probe=pr, snaps=sn, peak=pk, peak_idx=pi, report=rep.as_dict())

    def harmonic_dev(self, N, n_modes, d_lambda, d_phi, d_F, omega, d_p, d_u_static=None, alpha_R=0.0, beta_R=0.0, zeta=None, n_probe=0,
                     d_probe_dof=None, d_probe=None, snap_freq=None, d_snaps=None, d_peak=None, d_peak_idx=None):
        """Every d_* is a device pointer (int) or None; omega, zeta and snap_freq stay on the host.  Returns the report dict."""
        omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
        zt = None if zeta is None else np.ascontiguousarray(zeta, dtype=np.float64).reshape(-1)
        sf = None if snap_freq is None else np.ascontiguousarray(snap_freq, dtype=np.int32).reshape(-1)
        rep = HarmonicReport()
        self._chk(self.lib.stan_hip_harmonic_dev(
            self.h, C.c_int64(N), C.c_int32(int(n_modes)), _opt(d_lambda), _opt(d_phi), _opt(d_F), _opt(d_u_static), C.c_double(alpha_R),
            C.c_double(beta_R), _ptr(zt, C.c_double), C.c_int32(omega.shape[0]), _ptr(omega, C.c_double), C.c_int32(int(n_probe)),
            _opt(d_probe_dof, C.c_int32), _opt(d_probe), C.c_int32(0 if sf is None else sf.shape[0]), _ptr(sf, C.c_int32), _opt(d_snaps),
            _opt(d_p), _opt(d_peak), _opt(d_peak_idx, C.c_int32), C.byref(rep)))
        return rep.as_dict()

    def newmark_predict(self, u, v, a, F, M, coef, gF, Kw=None, want_w=True):
        """stan_hip_newmark_predict: (w or None, b) of one Newmark step from the state u, v, a [N]; coef as newmark_coef."""
        u, v, a, F, M = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (u, v, a, F, M))
        N = u.shape[0]
        Kw = None if Kw is None else np.ascontiguousarray(Kw, dtype=np.float64).reshape(-1)
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        if any(x.shape[0] != N for x in (v, a, F, M)) or (Kw is not None and Kw.shape[0] != N) or coef.shape[0] != 8:
            raise ValueError("newmark_predict: u, v, a, F, M, Kw must be [N] and coef [8]")
        w, b = (np.zeros(N) if want_w else None), np.zeros(N)
        self._chk(self.lib.stan_hip_newmark_predict(
            self.h, C.c_int64(N), _ptr(u, C.c_double), _ptr(v, C.c_double), _ptr(a, C.c_double), _ptr(F, C.c_double),
            _ptr(M, C.c_double), _ptr(Kw, C.c_double), _ptr(coef, C.c_double), C.c_double(gF), _ptr(w, C.c_double),
            _ptr(b, C.c_double)))
        return w, b

    def newmark_correct(self, u_new, u, v, a, coef, dt, gamma, M=None, F=None, Ku=None, gF=1.0, energy=False):
        """stan_hip_newmark_correct: (u', v', a', energy [3] or None); the inputs are left as they are."""
        u_new = np.ascontiguousarray(u_new, dtype=np.float64).reshape(-1)
        N = u_new.shape[0]
        u, v, a = (np.array(x, dtype=np.float64).reshape(-1) for x in (u, v, a))
        M, F, Ku = (None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (M, F, Ku))
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        if any(x.shape[0] != N for x in (u, v, a)) or any(x is not None and x.shape[0] != N for x in (M, F, Ku)) or coef.shape[0] != 8:
            raise ValueError("newmark_correct: the vectors must be [N] and coef [8]")
        e = np.zeros(3) if energy else None
        self._chk(self.lib.stan_hip_newmark_correct(
            self.h, C.c_int64(N), _ptr(u_new, C.c_double), _ptr(u, C.c_double), _ptr(v, C.c_double), _ptr(a, C.c_double),
            _ptr(coef, C.c_double), C.c_double(dt), C.c_double(gamma), _ptr(M, C.c_double), _ptr(F, C.c_double),
            _ptr(Ku, C.c_double), C.c_double(gF), _ptr(e, C.c_double)))
        return u, v, a, e

    def central_update(self, y, u, u_prev, M, F, dt, alpha_R=0.0, gF=1.0, step=1, s=None, state=True, energy=False):
        """stan_hip_central_update: dict(u_next, u_next_scaled or None, v, a (or None), energy [3] or None, first_nonfinite) of
        one central-difference update on host arrays [N]; y = K u, or A^ (u / s) with s given."""
        y, u, u_prev, M, F = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (y, u, u_prev, M, F))
        N = y.shape[0]
        s = None if s is None else np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
        if any(x.shape[0] != N for x in (u, u_prev, M, F)) or (s is not None and s.shape[0] != N):
            raise ValueError("central_update: the vectors must be [N]")
        un, uh = np.zeros(N), (None if s is None else np.zeros(N))
        v, a = (np.zeros(N), np.zeros(N)) if state else (None, None)
        e, bad = (np.zeros(3) if energy else None), C.c_int64(0)
        self._chk(self.lib.stan_hip_central_update(
            self.h, C.c_int64(N), _ptr(y, C.c_double), _ptr(s, C.c_double), _ptr(u, C.c_double), _ptr(u_prev, C.c_double),
            _ptr(M, C.c_double), _ptr(F, C.c_double), C.c_double(dt), C.c_double(alpha_R), C.c_double(gF), C.c_int64(step),
            _ptr(un, C.c_double), _ptr(uh, C.c_double), _ptr(v, C.c_double), _ptr(a, C.c_double), _ptr(e, C.c_double), C.byref(bad)))
        return dict(u_next=un, u_next_scaled=uh, v=v, a=a, energy=e, first_nonfinite=bad.value)

    def _thermal_stress_args(self, dT, conn, elem_mat, elem_type, mat_E_nu, mat_alpha):
        dT = np.ascontiguousarray(dT, dtype=np.float64).reshape(-1)
        conn, elem_mat, elem_type, mat_E_nu = _mesh(conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu)
        al = np.ascontiguousarray(mat_alpha, dtype=np.float64).reshape(-1)
        if al.shape[0] != mat_E_nu.shape[0] or elem_mat.shape[0] != conn.shape[0] or elem_type.shape[0] != conn.shape[0]:
            raise ValueError("thermal stress: mat_alpha must be [n_mat], elem_mat and elem_type [n_elem]")
        return dT, conn, elem_mat, elem_type, mat_E_nu, al

    def thermal_stress_hex8(self, dT, conn, elem_mat, elem_type, mat_E_nu, mat_alpha, stress):
        """stan_hip_thermal_stress_hex8: the corrected copy of stress [n_elem, 8, 6]."""
        dT, conn, elem_mat, elem_type, mat_E_nu, al = self._thermal_stress_args(dT, conn, elem_mat, elem_type, mat_E_nu, mat_alpha)
        out = np.array(stress, dtype=np.float64).reshape(-1, 8, 6)
        if out.shape[0] != conn.shape[0]:
            raise ValueError("thermal_stress_hex8: stress must be [n_elem, 8, 6]")
        self._chk(self.lib.stan_hip_thermal_stress_hex8(
            self.h, C.c_int64(dT.shape[0]), _ptr(dT, C.c_double), C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32),
            _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            _ptr(al, C.c_double), _ptr(out, C.c_double)))
        return out

    def thermal_stress_hex8_dev(self, n_nodes, d_dT, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, mat_alpha, d_stress):
        """All d_* are device pointers (ints); d_stress [n_elem, 8, 6] doubles is corrected in place."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        al = np.ascontiguousarray(mat_alpha, dtype=np.float64).reshape(-1)
        self._chk(self.lib.stan_hip_thermal_stress_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_dT, C.c_double), C.c_int64(n_elem), _dev(d_conn, C.c_int32),
            _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            _ptr(al, C.c_double), _dev(d_stress, C.c_double)))

    # -- assembly ------------------------------------------------------------------------
    def assemble_hex8(self, xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red):
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        k = C.c_void_p()
        self._chk(self.lib.stan_hip_assemble_hex8(
            self.h, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(node_dof, C.c_int32),
            C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32),
            _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            C.c_int64(red.shape[0]), _ptr(red, C.c_int32), C.byref(k)))
        return Matrix(self, k)

    def assemble_hex8_dev(self, n_nodes, d_xyz, d_node_dof, n_elem, d_conn, d_elem_mat,
                          d_elem_type, mat_E_nu, n_dof, d_red):
        """All d_* are device pointers (ints), e.g. torch tensor.data_ptr()."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        k = C.c_void_p()
        self._chk(self.lib.stan_hip_assemble_hex8_dev(
            self.h, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_node_dof, C.c_int32),
            C.c_int64(n_elem), _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32),
            _dev(d_elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double),
            C.c_int64(n_dof), _dev(d_red, C.c_int32), C.byref(k)))
        return Matrix(self, k)


class Results:
    """Strain / stress of a recovery kept on the device(s) (stan_results*)."""

    def __init__(self, ctx, handle, n_elem):
        self.ctx, self.h, self.n_elem = ctx, handle, n_elem
        ctx.lib.stan_hip_results_free.restype = None

    def map(self, e0, e1):
        """(strain, stress) of elements [e0, e1) as [e1 - e0, 8, 6] arrays (copies of the thread's staging memory)."""
        ps, pt = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        rc = self.ctx.lib.stan_hip_results_map(self.h, C.c_int64(e0), C.c_int64(e1), C.byref(ps), C.byref(pt))
        if rc != 0:
            raise StanHipError(rc, "stan_hip_results_map")
        n = (e1 - e0) * 48
        if n == 0:
            return np.zeros((0, 8, 6)), np.zeros((0, 8, 6))
        return (np.ctypeslib.as_array(ps, shape=(n,)).reshape(-1, 8, 6).copy(),
                np.ctypeslib.as_array(pt, shape=(n,)).reshape(-1, 8, 6).copy())

    def scalars(self, disp, conn, sel=None, point=True, cell=True):
        """Context.result_scalars on the kept results (stan_hip_results_scalars): nothing of the 2 x 48 x n_elem values
        is downloaded."""
        if np.asarray(conn).size != self.n_elem * 8:
            raise ValueError("Results.scalars: conn must be [n_elem, 8]")
        return self.ctx._scalars(
            lambda nn, d, n_e, c, ns, s, pt, ce: self.ctx.lib.stan_hip_results_scalars(self.ctx.h, self.h, nn, d, c, ns, s, pt, ce),
            disp, conn, sel, point, cell)

    def thermal_stress(self, dT, conn, elem_mat, elem_type, mat_E_nu, mat_alpha):
        """Context.thermal_stress_hex8 on the kept stress, in place (stan_hip_results_thermal_stress)."""
        dT, conn, elem_mat, elem_type, mat_E_nu, al = self.ctx._thermal_stress_args(dT, conn, elem_mat, elem_type, mat_E_nu, mat_alpha)
        if conn.shape[0] != self.n_elem:
            raise ValueError("Results.thermal_stress: conn must be [n_elem, 8]")
        self.ctx._chk(self.ctx.lib.stan_hip_results_thermal_stress(
            self.ctx.h, self.h, C.c_int64(dT.shape[0]), _ptr(dT, C.c_double), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32),
            _ptr(elem_type, C.c_uint8), C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), _ptr(al, C.c_double)))

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.stan_hip_results_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Matrix:
    """Opaque device-resident K (stan_matrix*)."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.k = handle

    def free(self):
        if getattr(self, "k", None):
            self.ctx.lib.stan_hip_matrix_free(self.k)
            self.k = None

    def __del__(self):
        # valid for a matrix whose context is already closed too: stan_hip_destroy detaches its
        # matrices, and a detached matrix gives its buffers straight back to the driver
        try:
            self.free()
        except Exception:
            pass

    def info(self):
        i = MatrixInfo()
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_info(self.k, C.byref(i)))
        return {k: getattr(i, k) for k, _ in MatrixInfo._fields_}

    def part_info(self, part):
        """info() of one shard of a matrix on a multi-device handle."""
        i = MatrixInfo()
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_part_info(self.k, C.c_int32(part), C.byref(i)))
        return {k: getattr(i, k) for k, _ in MatrixInfo._fields_}

    def cg_solve(self, F, eps_f, max_its=0, precision_mode=PREC_FP64):
        F = np.ascontiguousarray(F, dtype=np.float64)
        U = np.zeros_like(F)
        term, its, rel = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_cg_solve(
            self.ctx.h, self.k, _ptr(F, C.c_double), C.c_double(eps_f), C.c_int32(max_its),
            C.c_int32(precision_mode), _ptr(U, C.c_double), C.byref(term), C.byref(its),
            C.byref(rel)))
        return U, dict(terminationtype=term.value, iterations=its.value, rel_residual=rel.value)

    def cg_solve_dev(self, d_F, d_U, eps_f, max_its=0, precision_mode=PREC_FP64):
        term, its, rel = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_cg_solve_dev(
            self.ctx.h, self.k, _dev(d_F, C.c_double), C.c_double(eps_f), C.c_int32(max_its),
            C.c_int32(precision_mode), _dev(d_U, C.c_double), C.byref(term), C.byref(its),
            C.byref(rel)))
        return dict(terminationtype=term.value, iterations=its.value, rel_residual=rel.value)

    @staticmethod
    def _multi_reports(term, its, rel):
        return [dict(terminationtype=int(t), iterations=int(i), rel_residual=float(r)) for t, i, r in zip(term, its, rel)]

    def cg_solve_multi(self, F2d, eps_f, max_its=0, precision_mode=PREC_FP64):
        """F2d [n_rhs, N]: one load case per row, all solved in one loop over a single pass of K per iteration
        (stan_hip_cg_solve_multi).  Returns (U2d, [report dict per column, keys as cg_solve])."""
        F = np.ascontiguousarray(F2d, dtype=np.float64)
        if F.ndim != 2:
            raise ValueError("cg_solve_multi: F2d must be [n_rhs, N]")
        m = F.shape[0]
        U = np.zeros_like(F)
        term, its, rel = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1))
        self.ctx._chk(self.ctx.lib.stan_hip_cg_solve_multi(
            self.ctx.h, self.k, C.c_int32(m), _ptr(F, C.c_double), C.c_double(eps_f), C.c_int32(max_its),
            C.c_int32(precision_mode), _ptr(U, C.c_double), _ptr(term, C.c_int32), _ptr(its, C.c_int32),
            _ptr(rel, C.c_double)))
        return U, self._multi_reports(term[:m], its[:m], rel[:m])

    def cg_solve_multi_dev(self, d_F, d_U, n_rhs, eps_f, max_its=0, precision_mode=PREC_FP64):
        """d_F, d_U: device pointers (ints) of [n_rhs, N] arrays.  Returns the list of report dicts."""
        m = int(n_rhs)
        term, its, rel = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1))
        self.ctx._chk(self.ctx.lib.stan_hip_cg_solve_multi_dev(
            self.ctx.h, self.k, C.c_int32(m), _dev(d_F, C.c_double), C.c_double(eps_f), C.c_int32(max_its),
            C.c_int32(precision_mode), _dev(d_U, C.c_double), _ptr(term, C.c_int32), _ptr(its, C.c_int32),
            _ptr(rel, C.c_double)))
        return self._multi_reports(term[:m], its[:m], rel[:m])

    def modes(self, M, n_modes, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """stan_hip_modes: the n_modes lowest eigenpairs of K phi = lambda M phi, M [N] the diagonal mass.  Returns (lambda
        [n_modes], phi [n_modes, N], rho [n_modes], report dict of stan_modes_report)."""
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        N = self.info()["n_reduced"]
        if M.shape[0] != N:
            raise ValueError("modes: M must be [N]")
        k = max(int(n_modes), 1)
        lam, phi, rho, rep = np.zeros(k), np.zeros((k, N)), np.zeros(k), ModesReport()
        self.ctx._chk(self.ctx.lib.stan_hip_modes(
            self.ctx.h, self.k, _ptr(M, C.c_double), C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer),
            C.c_double(solve_eps), C.c_int32(solve_max_its), _ptr(lam, C.c_double), _ptr(phi, C.c_double), _ptr(rho, C.c_double),
            C.byref(rep)))
        return lam, phi, rho, rep.as_dict()

    def modes_dev(self, d_M, n_modes, d_lambda, d_phi, d_rho, tol=0.0, max_outer=0, solve_eps=0.0, solve_max_its=0):
        """d_M [N], d_lambda / d_rho [n_modes], d_phi [n_modes, N]: device pointers (ints).  Returns the report dict."""
        rep = ModesReport()
        self.ctx._chk(self.ctx.lib.stan_hip_modes_dev(
            self.ctx.h, self.k, _opt(d_M), C.c_int32(int(n_modes)), C.c_double(tol), C.c_int32(max_outer), C.c_double(solve_eps),
            C.c_int32(solve_max_its), _opt(d_lambda), _opt(d_phi), _opt(d_rho), C.byref(rep)))
        return rep.as_dict()

    def shifted(self, sigma, M):
        """stan_hip_matrix_shifted: a new Matrix holding K + sigma diag(M), M [N] the diagonal mass; K is left as it is."""
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        if M.shape[0] != self.info()["n_reduced"]:
            raise ValueError("shifted: M must be [N]")
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_shifted(self.ctx.h, self.k, C.c_double(sigma), _ptr(M, C.c_double), C.byref(k)))
        return Matrix(self.ctx, k)

    def shifted_dev(self, sigma, d_M):
        """d_M [N]: a device pointer (int)."""
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_shifted_dev(self.ctx.h, self.k, C.c_double(sigma), _opt(d_M), C.byref(k)))
        return Matrix(self.ctx, k)

    def geometric_stiffness(self, xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu, red):
        """stan_hip_geometric_stiffness_hex8: a new Matrix holding G = K_g(disp) in this matrix' layout; disp [n_nodes, 3] in
        NodeLib order, the mesh arrays those this matrix was assembled from.  This matrix is left as it is."""
        xyz, disp, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, disp=disp, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        if disp.size != xyz.size:
            raise ValueError("geometric_stiffness: disp must be [n_nodes, 3]")
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_geometric_stiffness_hex8(
            self.ctx.h, self.k, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(disp, C.c_double), _ptr(node_dof, C.c_int32),
            C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(red.shape[0]), _ptr(red, C.c_int32), C.byref(k)))
        return Matrix(self.ctx, k)

    def geometric_stiffness_dev(self, n_nodes, d_xyz, d_disp, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu,
                                n_dof, d_red):
        """All d_* are device pointers (ints), e.g. torch tensor.data_ptr()."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_geometric_stiffness_hex8_dev(
            self.ctx.h, self.k, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _dev(d_disp, C.c_double), _dev(d_node_dof, C.c_int32),
            C.c_int64(n_elem), _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32), C.byref(k)))
        return Matrix(self.ctx, k)

    def consistent_mass(self, xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red, mat_rho):
        """stan_hip_consistent_mass_hex8: a new Matrix holding the consistent mass M_c in this matrix' layout; mat_rho [n_mat],
        the mesh arrays those this matrix was assembled from.  This matrix is left as it is."""
        xyz, node_dof, conn, elem_mat, elem_type, mat_E_nu, red = _mesh(
            xyz=xyz, node_dof=node_dof, conn=conn, elem_mat=elem_mat, elem_type=elem_type, mat_E_nu=mat_E_nu, red=red)
        rho = None if mat_rho is None else np.ascontiguousarray(mat_rho, dtype=np.float64).reshape(-1)
        if rho is not None and rho.shape[0] != mat_E_nu.shape[0]:
            raise ValueError("consistent_mass: mat_rho must be [n_mat]")
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_consistent_mass_hex8(
            self.ctx.h, self.k, C.c_int64(xyz.shape[0]), _ptr(xyz, C.c_double), _ptr(rho, C.c_double), _ptr(node_dof, C.c_int32),
            C.c_int64(conn.shape[0]), _ptr(conn, C.c_int32), _ptr(elem_mat, C.c_int32), _ptr(elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(red.shape[0]), _ptr(red, C.c_int32), C.byref(k)))
        return Matrix(self.ctx, k)

    def consistent_mass_dev(self, n_nodes, d_xyz, mat_rho, d_node_dof, n_elem, d_conn, d_elem_mat, d_elem_type, mat_E_nu, n_dof,
                            d_red):
        """All d_* are device pointers (ints), e.g. torch tensor.data_ptr(); mat_rho and mat_E_nu host arrays."""
        mat_E_nu = np.ascontiguousarray(mat_E_nu, dtype=np.float64).reshape(-1, 2)
        rho = np.ascontiguousarray(mat_rho, dtype=np.float64).reshape(-1)
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_consistent_mass_hex8_dev(
            self.ctx.h, self.k, C.c_int64(n_nodes), _dev(d_xyz, C.c_double), _ptr(rho, C.c_double), _dev(d_node_dof, C.c_int32),
            C.c_int64(n_elem), _dev(d_conn, C.c_int32), _dev(d_elem_mat, C.c_int32), _dev(d_elem_type, C.c_uint8),
            C.c_int32(mat_E_nu.shape[0]), _ptr(mat_E_nu, C.c_double), C.c_int64(n_dof), _dev(d_red, C.c_int32), C.byref(k)))
        return Matrix(self.ctx, k)

    def axpy(self, sigma, B):
        """stan_hip_matrix_axpy: a new Matrix holding this matrix + sigma B, B a Matrix on this matrix' layout; both are left
        as they are."""
        k = C.c_void_p()
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_axpy(self.ctx.h, self.k, C.c_double(sigma), None if B is None else B.k, C.byref(k)))
        return Matrix(self.ctx, k)

    def modes_shifted(self, M, n_modes, sigma, **kw):
        """The n_modes lowest eigenpairs of a model that may be free-free, through the shift: stan_hip_modes on K + sigma M
        gives mu = lambda + sigma.  Returns (lambda = mu - sigma, phi, rho, report); rho and report["max_rho"] are the
        convergence measures of the SHIFTED problem (relative to mu), report["shift"] = sigma."""
        S = self.shifted(sigma, M)
        try:
            mu, phi, rho, rep = S.modes(M, n_modes, **kw)
        finally:
            S.free()
        rep["shift"] = float(sigma)
        return mu - sigma, phi, rho, rep

    def transient(self, M, F, dt, n_steps, u0=None, v0=None, beta_N=0.0, gamma=0.0, alpha_R=0.0, beta_R=0.0, curve=None,
                  solve_eps=0.0, solve_max_its=0, probe_dof=None, snap_every=0, energy=False):
        """stan_hip_transient: implicit Newmark steps of M a + C v + K u = g(t) F.  curve: [(t, g), ...] or None (g = 1).
        Returns a dict: u, v, a (the end state), probe_u [n_steps + 1, n_probe], snaps [n_snap, 3, N] or None, energy
        [n_steps + 1, 3] or None, report (stan_transient_report; written on an error too: StanHipError.report)."""
        N = self.info()["n_reduced"]
        M, F = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (M, F))
        u0, v0 = (None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (u0, v0))
        if any(x is not None and x.shape[0] != N for x in (M, F, u0, v0)):
            raise ValueError("transient: M, F, u0, v0 must be [N]")
        ct, cg, nc = None, None, 0
        if curve is not None:
            cv = np.ascontiguousarray(curve, dtype=np.float64).reshape(-1, 2)
            ct, cg, nc = np.ascontiguousarray(cv[:, 0]), np.ascontiguousarray(cv[:, 1]), cv.shape[0]
        pd = None if probe_dof is None else np.ascontiguousarray(probe_dof, dtype=np.int32).reshape(-1)
        npr = 0 if pd is None else pd.shape[0]
        rows = max(int(n_steps), 0) + 1
        pu = np.zeros((rows, npr)) if npr else None
        n_snap = (max(int(n_steps), 0) // snap_every + 1) if snap_every > 0 else 0
        sn = np.zeros((n_snap, 3, N)) if n_snap else None
        en = np.zeros((rows, 3)) if energy else None
        ue, ve, ae, rep = np.zeros(N), np.zeros(N), np.zeros(N), TransientReport()
        rc = self.ctx.lib.stan_hip_transient(
            self.ctx.h, self.k, _ptr(M, C.c_double), _ptr(F, C.c_double), _ptr(u0, C.c_double), _ptr(v0, C.c_double),
            C.c_double(dt), C.c_int32(int(n_steps)), C.c_double(beta_N), C.c_double(gamma), C.c_double(alpha_R), C.c_double(beta_R),
            C.c_int32(nc), _ptr(ct, C.c_double), _ptr(cg, C.c_double), C.c_double(solve_eps), C.c_int32(solve_max_its),
            C.c_int32(npr), _ptr(pd, C.c_int32), _ptr(pu, C.c_double), C.c_int32(int(snap_every)), _ptr(sn, C.c_double),
            _ptr(en, C.c_double), _ptr(ue, C.c_double), _ptr(ve, C.c_double), _ptr(ae, C.c_double), C.byref(rep))
        if rc != 0:
            e = StanHipError(rc, self.ctx.lib.stan_hip_last_error(self.ctx.h).decode())
            e.report = rep.as_dict()
            raise e
        return dict(u=ue, v=ve, a=ae, probe_u=pu, snaps=sn, energy=en, report=rep.as_dict())

    def transient_dev(self, d_M, d_F, dt, n_steps, d_u_end, d_v_end, d_a_end, d_u0=None, d_v0=None, beta_N=0.0, gamma=0.0,
                      alpha_R=0.0, beta_R=0.0, curve=None, solve_eps=0.0, solve_max_its=0, n_probe=0, d_probe_dof=None,
                      d_probe_u=None, snap_every=0, d_snaps=None, d_energy=None):
        """Every d_* is a device pointer (int) or None; the curve stays on the host.  Returns the report dict."""
        ct, cg, nc = None, None, 0
        if curve is not None:
            cv = np.ascontiguousarray(curve, dtype=np.float64).reshape(-1, 2)
            ct, cg, nc = np.ascontiguousarray(cv[:, 0]), np.ascontiguousarray(cv[:, 1]), cv.shape[0]
        rep = TransientReport()
        self.ctx._chk(self.ctx.lib.stan_hip_transient_dev(
            self.ctx.h, self.k, _opt(d_M), _opt(d_F), _opt(d_u0), _opt(d_v0), C.c_double(dt), C.c_int32(int(n_steps)),
            C.c_double(beta_N), C.c_double(gamma), C.c_double(alpha_R), C.c_double(beta_R), C.c_int32(nc), _ptr(ct, C.c_double),
            _ptr(cg, C.c_double), C.c_double(solve_eps), C.c_int32(solve_max_its), C.c_int32(int(n_probe)),
            _opt(d_probe_dof, C.c_int32), _opt(d_probe_u), C.c_int32(int(snap_every)), _opt(d_snaps), _opt(d_energy),
            _opt(d_u_end), _opt(d_v_end), _opt(d_a_end), C.byref(rep)))
        return rep.as_dict()

    def stable_step(self, M, n_power=0):
        """stan_hip_stable_step: (lambda_upper, lambda_power, dt_stable) of M^-1 K, M [N] the lumped mass."""
        M = np.ascontiguousarray(M, dtype=np.float64).reshape(-1)
        if M.shape[0] != self.info()["n_reduced"]:
            raise ValueError("stable_step: M must be [N]")
        lu, lp, dts = C.c_double(0), C.c_double(0), C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_stable_step(self.ctx.h, self.k, _ptr(M, C.c_double), C.c_int32(int(n_power)),
                                                        C.byref(lu), C.byref(lp), C.byref(dts)))
        return lu.value, lp.value, dts.value

    def stable_step_dev(self, d_M, n_power=0):
        """d_M: a device pointer (int)."""
        lu, lp, dts = C.c_double(0), C.c_double(0), C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_stable_step_dev(self.ctx.h, self.k, _opt(d_M), C.c_int32(int(n_power)),
                                                            C.byref(lu), C.byref(lp), C.byref(dts)))
        return lu.value, lp.value, dts.value

    @staticmethod
    def _curve(curve):
        if curve is None:
            return None, None, 0
        cv = np.ascontiguousarray(curve, dtype=np.float64).reshape(-1, 2)
        return np.ascontiguousarray(cv[:, 0]), np.ascontiguousarray(cv[:, 1]), cv.shape[0]

    def explicit(self, M, F, dt, n_steps, u0=None, v0=None, alpha_R=0.0, curve=None, probe_dof=None, snap_every=0, energy_every=0,
                 n_power=0, out=None):
        """stan_hip_explicit: central-difference steps of M a + alpha_R M v + K u = g(t) F.  curve: [(t, g), ...] or None (g = 1).
        Returns a dict: u, v, a (the state at step n_steps), probe_u [n_steps + 1, n_probe], snaps [n_snap, 3, N] or None, energy
        [n_en, 3] or None, report (stan_explicit_report; written on an error too: StanHipError.report).  out: a dict of
        preallocated arrays under the same names, used instead of fresh ones (a refused call must leave them untouched)."""
        N = self.info()["n_reduced"]
        M, F = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (M, F))
        u0, v0 = (None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in (u0, v0))
        if any(x is not None and x.shape[0] != N for x in (M, F, u0, v0)):
            raise ValueError("explicit: M, F, u0, v0 must be [N]")
        ct, cg, nc = self._curve(curve)
        pd = None if probe_dof is None else np.ascontiguousarray(probe_dof, dtype=np.int32).reshape(-1)
        npr = 0 if pd is None else pd.shape[0]
        steps = max(int(n_steps), 0)
        o = dict(out or {})
        pu = o.get("probe_u", np.zeros((steps + 1, npr)) if npr else None)
        sn = o.get("snaps", np.zeros((steps // snap_every + 1, 3, N)) if snap_every > 0 else None)
        en = o.get("energy", np.zeros((steps // energy_every + 1, 3)) if energy_every > 0 else None)
        ue, ve, ae = (o.get(k, None) for k in ("u", "v", "a"))
        ue, ve, ae = (np.zeros(N) if x is None else x for x in (ue, ve, ae))
        rep = ExplicitReport()
        rc = self.ctx.lib.stan_hip_explicit(
            self.ctx.h, self.k, _ptr(M, C.c_double), _ptr(F, C.c_double), _ptr(u0, C.c_double), _ptr(v0, C.c_double),
            C.c_double(dt), C.c_int32(int(n_steps)), C.c_double(alpha_R), C.c_int32(nc), _ptr(ct, C.c_double), _ptr(cg, C.c_double),
            C.c_int32(npr), _ptr(pd, C.c_int32), _ptr(pu, C.c_double), C.c_int32(int(snap_every)), _ptr(sn, C.c_double),
            C.c_int32(int(energy_every)), _ptr(en, C.c_double), _ptr(ue, C.c_double), _ptr(ve, C.c_double), _ptr(ae, C.c_double),
            C.c_int32(int(n_power)), C.byref(rep))
        if rc != 0:
            e = StanHipError(rc, self.ctx.lib.stan_hip_last_error(self.ctx.h).decode())
            e.report = rep.as_dict()
            raise e
        return dict(u=ue, v=ve, a=ae, probe_u=pu, snaps=sn, energy=en, report=rep.as_dict())

    def explicit_dev(self, d_M, d_F, dt, n_steps, d_u_end, d_v_end, d_a_end, d_u0=None, d_v0=None, alpha_R=0.0, curve=None, n_probe=0,
                     d_probe_dof=None, d_probe_u=None, snap_every=0, d_snaps=None, energy_every=0, d_energy=None, n_power=0):
        """Every d_* is a device pointer (int) or None; the curve stays on the host.  Returns the report dict."""
        ct, cg, nc = self._curve(curve)
        rep = ExplicitReport()
        self.ctx._chk(self.ctx.lib.stan_hip_explicit_dev(
            self.ctx.h, self.k, _opt(d_M), _opt(d_F), _opt(d_u0), _opt(d_v0), C.c_double(dt), C.c_int32(int(n_steps)),
            C.c_double(alpha_R), C.c_int32(nc), _ptr(ct, C.c_double), _ptr(cg, C.c_double), C.c_int32(int(n_probe)),
            _opt(d_probe_dof, C.c_int32), _opt(d_probe_u), C.c_int32(int(snap_every)), _opt(d_snaps), C.c_int32(int(energy_every)),
            _opt(d_energy), _opt(d_u_end), _opt(d_v_end), _opt(d_a_end), C.c_int32(int(n_power)), C.byref(rep)))
        return rep.as_dict()

    def to_csr(self, upper_only=True):
        nnz = C.c_int64(0)
        lib, h = self.ctx.lib, self.ctx.h
        self.ctx._chk(lib.stan_hip_matrix_to_csr(h, self.k, C.c_int32(int(upper_only)),
                                                 C.byref(nnz), None, None, None))
        N = self.info()["n_reduced"]
        rowptr = np.zeros(N + 1, dtype=np.int64)
        col = np.zeros(max(nnz.value, 1), dtype=np.int32)
        val = np.zeros(max(nnz.value, 1), dtype=np.float64)
        self.ctx._chk(lib.stan_hip_matrix_to_csr(h, self.k, C.c_int32(int(upper_only)),
                                                 C.byref(nnz), _ptr(rowptr, C.c_int64),
                                                 _ptr(col, C.c_int32), _ptr(val, C.c_double)))
        return rowptr, col[:nnz.value], val[:nnz.value]

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self.ctx._chk(self.ctx.lib.stan_hip_spmv(self.ctx.h, self.k, _ptr(x, C.c_double),
                                                 _ptr(y, C.c_double)))
        return y

    def diagonal(self):
        """K_ii of the reduced system (unscaled)."""
        d = np.zeros(self.info()["n_reduced"])
        self.ctx._chk(self.ctx.lib.stan_hip_matrix_diagonal(self.ctx.h, self.k, _ptr(d, C.c_double)))
        return d

    def scaled_residual(self, F, U):
        """||S (F - K U)|| / ||S F|| with s_i = 1/sqrt(K_ii): the quantity stan_hip_cg_solve reports, from an
        independent product (stan_hip_spmv) and the exported diagonal."""
        d = self.diagonal()
        s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
        r = s * (np.asarray(F, dtype=np.float64) - self.spmv(U))
        return float(np.linalg.norm(r) / np.linalg.norm(s * F))

    def plan(self):
        lib, h = self.ctx.lib, self.ctx.h
        i = self.info()
        nr = 64
        row_starts = np.zeros(nr + 1, np.int64)
        nh, nn = C.c_int64(0), C.c_int32(0)
        self.ctx._chk(lib.stan_hip_matrix_plan(h, self.k, None, C.byref(nh), None, C.byref(nn),
                                               None, None, None, None))
        halo = np.zeros(max(nh.value, 1), np.int32)
        nbr = np.zeros(max(nn.value, 1), np.int32)
        send_off = np.zeros(nn.value + 1, np.int64)
        recv_off = np.zeros(nn.value + 1, np.int64)
        self.ctx._chk(lib.stan_hip_matrix_plan(h, self.k, _ptr(row_starts, C.c_int64), C.byref(nh),
                                               _ptr(halo, C.c_int32), C.byref(nn), _ptr(nbr, C.c_int32),
                                               _ptr(send_off, C.c_int64), None, _ptr(recv_off, C.c_int64)))
        send_rows = np.zeros(max(int(send_off[-1]), 1), np.int32)
        self.ctx._chk(lib.stan_hip_matrix_plan(h, self.k, None, C.byref(nh), None, C.byref(nn), None,
                                               None, _ptr(send_rows, C.c_int32), None))
        return dict(halo_glob=halo[:nh.value], nbr=nbr[:nn.value], send_off=send_off,
                    recv_off=recv_off, send_rows=send_rows[:int(send_off[-1])],
                    row_begin=i["row_begin"], row_end=i["row_end"], row_starts=row_starts)

    def spmv_local(self, x_local):
        i = self.info()
        x_local = np.ascontiguousarray(x_local, dtype=np.float64)
        assert x_local.shape[0] == 3 * (i["row_end"] - i["row_begin"] + i["n_halo"])
        y = np.zeros(3 * (i["row_end"] - i["row_begin"]))
        self.ctx._chk(self.ctx.lib.stan_hip_spmv_local(self.ctx.h, self.k, _ptr(x_local, C.c_double),
                                                       _ptr(y, C.c_double)))
        return y

    def csr_spmv_bench(self, reps=20):
        """lab build only (make -C stan_amd/csrc lab; STAN_HIP_LIB=.../libstan_hip_lab.so)"""
        if not hasattr(self.ctx.lib, "stan_hip_csr_spmv_bench"):
            raise RuntimeError("stan_hip_csr_spmv_bench exists only in the lab build of the library")
        ms, nb, diff = C.c_double(0), C.c_int64(0), C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_csr_spmv_bench(self.ctx.h, self.k, C.c_int32(reps),
                                                           C.byref(ms), C.byref(nb), C.byref(diff)))
        return ms.value, nb.value, diff.value

    def stream_bench(self, reps=20):
        """(ms per read-only sweep of K's resident fp64 values in the product's access pattern, bytes per sweep)"""
        ms, nb = C.c_double(0), C.c_int64(0)
        self.ctx._chk(self.ctx.lib.stan_hip_stream_bench(self.ctx.h, self.k, C.c_int32(reps), C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def spmv_bench(self, reps=20, precision_mode=PREC_FP64):
        ms = C.c_double(0)
        self.ctx._chk(self.ctx.lib.stan_hip_spmv_bench(self.ctx.h, self.k,
                                                       C.c_int32(precision_mode), C.c_int32(reps),
                                                       C.byref(ms)))
        return ms.value
