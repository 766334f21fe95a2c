"""ctypes binding of libstan_host.so (include/stan_host.h): the host-side integer steps of
Solver.SolverLinearStatics around the GPU hot path.  No GPU needed."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libstan_host.so")

EXPORTS = ["stan_host_assign_dof", "stan_host_dof_reduction", "stan_host_load_vector",
           "stan_host_nodal_displacements", "stan_host_partition_rows", "stan_host_partition_plan",
           "stan_host_cholesky_skyline_solve", "stan_host_lu_upper_solve", "stan_host_partition_elements"]

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class StanHostError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("libstan_host error %d in %s" % (code, what))
        self.code = code


def assign_dof(n_nodes, conn):
    """Database.AssignDOF (Database.cs:140-234) -> (node_index[n], node_dof[n,3])."""
    conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
    idx = np.zeros(n_nodes, dtype=np.int32)
    dof = np.zeros((n_nodes, 3), dtype=np.int32)
    rc = load().stan_host_assign_dof(C.c_int64(n_nodes), C.c_int64(conn.shape[0]),
                                     _p(conn, C.c_int32), _p(idx, C.c_int32), _p(dof, C.c_int32))
    if rc:
        raise StanHostError(rc, "assign_dof")
    return idx, dof


def dof_reduction(n_dof, node_dof, spc_nodes, spc_vals):
    """Solver.cs:104-132 -> (red[n_dof], n_fixed)."""
    node_dof = np.ascontiguousarray(node_dof, dtype=np.int32)
    spc_nodes = np.ascontiguousarray(spc_nodes, dtype=np.int32)
    spc_vals = np.ascontiguousarray(spc_vals, dtype=np.float64).reshape(-1, 3)
    red = np.zeros(n_dof, dtype=np.int32)
    nfix = C.c_int64(0)
    rc = load().stan_host_dof_reduction(C.c_int64(n_dof), _p(node_dof, C.c_int32),
                                        C.c_int64(spc_nodes.shape[0]), _p(spc_nodes, C.c_int32),
                                        _p(spc_vals, C.c_double), _p(red, C.c_int32),
                                        C.byref(nfix))
    if rc:
        raise StanHostError(rc, "dof_reduction")
    return red, int(nfix.value)


def load_vector(n_dof, node_dof, red, n_fixed, load_nodes, load_vals):
    """Solver.cs:136-152 -> F[n_dof - n_fixed]."""
    node_dof = np.ascontiguousarray(node_dof, dtype=np.int32)
    red = np.ascontiguousarray(red, dtype=np.int32)
    load_nodes = np.ascontiguousarray(load_nodes, dtype=np.int32)
    load_vals = np.ascontiguousarray(load_vals, dtype=np.float64).reshape(-1, 3)
    F = np.zeros(n_dof - n_fixed, dtype=np.float64)
    rc = load().stan_host_load_vector(C.c_int64(n_dof), _p(node_dof, C.c_int32),
                                      _p(red, C.c_int32), C.c_int64(load_nodes.shape[0]),
                                      _p(load_nodes, C.c_int32), _p(load_vals, C.c_double),
                                      _p(F, C.c_double))
    if rc:
        raise StanHostError(rc, "load_vector")
    return F


def nodal_displacements(node_dof, red, U):
    """Include_BC_DOF (SolverFunctions.cs:520-538) + Solver.cs:171-178 -> disp[n_nodes,3]."""
    node_dof = np.ascontiguousarray(node_dof, dtype=np.int32)
    red = np.ascontiguousarray(red, dtype=np.int32)
    U = np.ascontiguousarray(U, dtype=np.float64)
    out = np.zeros(node_dof.shape, dtype=np.float64)
    rc = load().stan_host_nodal_displacements(C.c_int64(node_dof.shape[0]),
                                              _p(node_dof, C.c_int32), _p(red, C.c_int32),
                                              _p(U, C.c_double), _p(out, C.c_double))
    if rc:
        raise StanHostError(rc, "nodal_displacements")
    return out


def cholesky_skyline_solve(rowptr, col, val, b):
    """LinearSolver_Cholesky (SolverFunctions.cs:332-444) on the reduced upper CRS: returns
    (x, terminationtype, profile_entries); terminationtype -3 and x = 0 when K is not SPD."""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = rowptr.shape[0] - 1
    x = np.zeros(n)
    t, prof = C.c_int32(0), C.c_int64(0)
    rc = load().stan_host_cholesky_skyline_solve(C.c_int64(n), _p(rowptr, C.c_int64), _p(col, C.c_int32),
                                                 _p(val, C.c_double), _p(b, C.c_double), _p(x, C.c_double),
                                                 C.byref(t), C.byref(prof))
    if rc:
        raise StanHostError(rc, "cholesky_skyline_solve")
    return x, t.value, prof.value


def lu_upper_solve(rowptr, col, val, b):
    """LinearSolver_LU as the reference computes it (SolverFunctions.cs:446-516): triu(K) x = b."""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = rowptr.shape[0] - 1
    x = np.zeros(n)
    t = C.c_int32(0)
    rc = load().stan_host_lu_upper_solve(C.c_int64(n), _p(rowptr, C.c_int64), _p(col, C.c_int32),
                                         _p(val, C.c_double), _p(b, C.c_double), _p(x, C.c_double), C.byref(t))
    if rc:
        raise StanHostError(rc, "lu_upper_solve")
    return x, t.value


def partition_plan(node_index, conn, nranks, rank):
    """Row partition + halo plan of `rank` (stan_host_partition_plan) as a dict."""
    node_index = np.ascontiguousarray(node_index, dtype=np.int32)
    conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
    n = node_index.shape[0]
    row_starts = np.zeros(nranks + 1, np.int64)
    halo = np.zeros(n, np.int32)
    send_rows = np.zeros(n, np.int32)
    nbr = np.zeros(nranks, np.int32)
    send_off = np.zeros(nranks + 1, np.int64)
    recv_off = np.zeros(nranks + 1, np.int64)
    nh, nn = C.c_int64(0), C.c_int32(0)
    rc = load().stan_host_partition_plan(
        C.c_int64(n), _p(node_index, C.c_int32), C.c_int64(conn.shape[0]), _p(conn, C.c_int32),
        C.c_int32(nranks), C.c_int32(rank), _p(row_starts, C.c_int64), C.byref(nh),
        _p(halo, C.c_int32), C.byref(nn), _p(nbr, C.c_int32), _p(send_off, C.c_int64),
        _p(send_rows, C.c_int32), _p(recv_off, C.c_int64))
    if rc:
        raise StanHostError(rc, "partition_plan")
    k = nn.value
    return dict(row_starts=row_starts, halo_glob=halo[:nh.value].copy(), nbr=nbr[:k].copy(),
                send_off=send_off[:k + 1].copy(), recv_off=recv_off[:k + 1].copy(),
                send_rows=send_rows[:send_off[k]].copy())


def partition_elements(node_index, conn, nranks, rank):
    """Ascending indices of the elements `rank` must hold (stan_host_partition_elements)."""
    node_index = np.ascontiguousarray(node_index, dtype=np.int32)
    conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
    out = np.zeros(conn.shape[0], np.int32)
    n = C.c_int64(0)
    rc = load().stan_host_partition_elements(C.c_int64(node_index.shape[0]), _p(node_index, C.c_int32),
                                             C.c_int64(conn.shape[0]), _p(conn, C.c_int32), C.c_int32(nranks),
                                             C.c_int32(rank), _p(out, C.c_int32), C.byref(n))
    if rc:
        raise StanHostError(rc, "partition_elements")
    return out[:n.value].copy()


# ---- distributed loads: the pressure faces of a node set -------------------------------------------
EXPORTS += ["stan_host_pressure_faces"]


def pressure_faces(n_nodes, conn, set_nodes, set_p, capacity=None):
    """stan_host_pressure_faces -> (face_elem int32[], face_id uint8[], face_p float64[]) ascending by face_elem * 6 +
    face_id: the faces all of whose corners are in the node set, interior and collapsed (< 3 distinct nodes) faces left
    out.  capacity: the size of the arrays of the second call (default: what the first call reports)."""
    conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
    set_nodes = np.ascontiguousarray(set_nodes, dtype=np.int32).reshape(-1)
    set_p = np.ascontiguousarray(set_p, dtype=np.float64).reshape(-1)
    if set_nodes.shape[0] != set_p.shape[0]:
        raise ValueError("pressure_faces: set_nodes and set_p must have one length")
    n = C.c_int64(0)
    args = (C.c_int64(n_nodes), C.c_int64(conn.shape[0]), _p(conn, C.c_int32), C.c_int64(set_nodes.shape[0]),
            _p(set_nodes, C.c_int32), _p(set_p, C.c_double))
    rc = load().stan_host_pressure_faces(*args, C.c_int64(0), None, None, None, C.byref(n))
    if rc:
        raise StanHostError(rc, "pressure_faces")
    cap = n.value if capacity is None else int(capacity)
    fe, fi, fp = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1))
    rc = load().stan_host_pressure_faces(*args, C.c_int64(cap), _p(fe, C.c_int32), _p(fi, C.c_uint8), _p(fp, C.c_double), C.byref(n))
    if rc:
        raise StanHostError(rc, "pressure_faces")
    return fe[:n.value].copy(), fi[:n.value].copy(), fp[:n.value].copy()


# ---- result scalars: names + .vtu export (Part.Load_Scalar / Part.ExportGrid) -------------------
EXPORTS += ["stan_host_scalar_name", "stan_host_write_vtu"]
N_SCALARS = 24


def scalar_name(s):
    """Result string of scalar s as the reference's GUI lists it (Part.cs:403-428); None outside 0..23."""
    lib = load()
    lib.stan_host_scalar_name.restype = C.c_char_p
    r = lib.stan_host_scalar_name(C.c_int32(s))
    return r.decode() if r is not None else None


def write_vtu(path, xyz, disp, conn, point_arrays=(), cell_arrays=()):
    """One-piece UnstructuredGrid .vtu (appended raw data): points xyz + disp (disp may be None), hexahedra conn
    [n_elem, 8]; point_arrays / cell_arrays: sequences of (name, values[n_nodes] / values[n_elem]), stored as Float32."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    disp = None if disp is None else np.ascontiguousarray(disp, dtype=np.float64).reshape(-1, 3)
    conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1, 8)
    nn, ne = xyz.shape[0], conn.shape[0]

    def pack(arrays, n):
        names = (C.c_char_p * max(len(arrays), 1))(*[a[0].encode() for a in arrays])
        vals = np.ascontiguousarray([np.asarray(a[1], dtype=np.float64).reshape(n) for a in arrays], dtype=np.float64).reshape(len(arrays), n)
        return names, vals

    pn, pv = pack(list(point_arrays), nn)
    cn, cv = pack(list(cell_arrays), ne)
    rc = load().stan_host_write_vtu(os.fsencode(path), C.c_int64(nn), _p(xyz, C.c_double), _p(disp, C.c_double) if disp is not None else None,
                                    C.c_int64(ne), _p(conn, C.c_int32), C.c_int32(pv.shape[0]), pn, _p(pv, C.c_double),
                                    C.c_int32(cv.shape[0]), cn, _p(cv, C.c_double))
    if rc:
        raise StanHostError(rc, "write_vtu")


# ---- STAN_Database mirror + STdb codec (stan_db part of include/stan_host.h) -----------------
EXPORTS += [
    "stan_host_db_new", "stan_host_db_free", "stan_host_db_last_error", "stan_host_db_read_stdb",
    "stan_host_db_parse_stdb", "stan_host_db_write_stdb", "stan_host_db_serialize",
    "stan_host_db_read_bdf", "stan_host_db_set_mesh", "stan_host_db_add_material",
    "stan_host_db_assign_part", "stan_host_db_add_bc", "stan_host_db_set_analysis",
    "stan_host_db_sizes", "stan_host_db_get_analysis", "stan_host_db_assign_dof",
    "stan_host_db_get_flat", "stan_host_db_get_reduction", "stan_host_db_set_results",
    "stan_host_db_get_results", "stan_host_db_get_distributed_loads", "stan_host_db_get_thermal_loads", "stan_host_db_get_density",
]


class Db:
    """A Database (Database.cs:10-21) living in libstan_host.so."""

    def __init__(self):
        self.lib = load()
        self.lib.stan_host_db_last_error.restype = C.c_char_p
        self.lib.stan_host_db_free.restype = None
        self.h = C.c_void_p()
        rc = self.lib.stan_host_db_new(C.byref(self.h))
        if rc:
            raise StanHostError(rc, "db_new")

    def __del__(self):
        try:
            if self.h:
                self.lib.stan_host_db_free(self.h)
                self.h = None
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            msg = self.lib.stan_host_db_last_error(self.h)
            e = StanHostError(rc, what + ": " + (msg.decode() if msg else ""))
            raise e

    # -- STdb ---------------------------------------------------------------------------------
    @classmethod
    def read_stdb(cls, path):
        d = cls()
        d._chk(d.lib.stan_host_db_read_stdb(d.h, os.fsencode(path)), "read_stdb")
        return d

    @classmethod
    def parse_stdb(cls, data):
        d = cls()
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        d._chk(d.lib.stan_host_db_parse_stdb(d.h, buf, C.c_int64(len(data))), "parse_stdb")
        return d

    def write_stdb(self, path, packed=False):
        self._chk(self.lib.stan_host_db_write_stdb(self.h, os.fsencode(path), C.c_int32(int(packed))),
                  "write_stdb")

    def write_stdb_with_results(self, path, disp, strain, stress, packed=False):
        """ExportOutput straight from flat result arrays (same bytes as set_results + write_stdb)."""
        disp = np.ascontiguousarray(disp, dtype=np.float64)
        strain = np.ascontiguousarray(strain, dtype=np.float64)
        stress = np.ascontiguousarray(stress, dtype=np.float64)
        self._chk(self.lib.stan_host_db_write_stdb_with_results(
            self.h, os.fsencode(path), C.c_int32(int(packed)), _p(disp, C.c_double), _p(strain, C.c_double),
            _p(stress, C.c_double)), "write_stdb_with_results")

    def serialize(self, packed=False):
        n = C.c_int64(0)
        self._chk(self.lib.stan_host_db_serialize(self.h, C.c_int32(int(packed)), None, C.c_int64(0),
                                                  C.byref(n)), "serialize")
        buf = (C.c_uint8 * max(n.value, 1))()
        self._chk(self.lib.stan_host_db_serialize(self.h, C.c_int32(int(packed)), buf,
                                                  C.c_int64(n.value), C.byref(n)), "serialize")
        return bytes(buf[:n.value])

    # -- construction (what the GUI does before it launches the solver) -------------------------
    def read_bdf(self, path):
        nerr = C.c_int64(0)
        self._chk(self.lib.stan_host_db_read_bdf(self.h, os.fsencode(path), C.byref(nerr)), "read_bdf")
        return nerr.value

    def set_mesh(self, node_ids, xyz, elem_ids, elem_pids, nlist8, hex_type="HEX8_G2"):
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        elem_ids = np.ascontiguousarray(elem_ids, dtype=np.int32)
        elem_pids = np.ascontiguousarray(elem_pids, dtype=np.int32)
        nlist8 = np.ascontiguousarray(nlist8, dtype=np.int32)
        self._chk(self.lib.stan_host_db_set_mesh(
            self.h, C.c_int64(node_ids.shape[0]), _p(node_ids, C.c_int32), _p(xyz, C.c_double),
            C.c_int64(elem_ids.shape[0]), _p(elem_ids, C.c_int32), _p(elem_pids, C.c_int32),
            _p(nlist8, C.c_int32), hex_type.encode()), "set_mesh")

    def add_material(self, mid, name, E, nu):
        self._chk(self.lib.stan_host_db_add_material(self.h, C.c_int32(mid), name.encode(),
                                                     C.c_double(E), C.c_double(nu)), "add_material")

    def assign_part(self, pid, mat_id, hex_type="HEX8_G2"):
        self._chk(self.lib.stan_host_db_assign_part(self.h, C.c_int32(pid), C.c_int32(mat_id),
                                                    hex_type.encode()), "assign_part")

    def add_bc(self, bid, name, btype, node_ids, vals):
        node_ids = np.ascontiguousarray(node_ids, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, 3)
        self._chk(self.lib.stan_host_db_add_bc(self.h, C.c_int32(bid), name.encode(), btype.encode(),
                                               C.c_int64(node_ids.shape[0]), _p(node_ids, C.c_int32),
                                               _p(vals, C.c_double)), "add_bc")

    def set_analysis(self, atype="Linear_Statics", lin_solver="CG", tol=1e-6, max_iter=0, inc_numb=1):
        self._chk(self.lib.stan_host_db_set_analysis(self.h, atype.encode(), lin_solver.encode(),
                                                     C.c_double(tol), C.c_int32(max_iter),
                                                     C.c_int32(inc_numb)), "set_analysis")

    # -- queries ------------------------------------------------------------------------------
    def sizes(self):
        s = (C.c_int64 * 8)()
        self._chk(self.lib.stan_host_db_sizes(self.h, s), "sizes")
        return dict(nodes=s[0], elements=s[1], materials=s[2], bcs=s[3], nDOF=s[4],
                    result_step=s[5], import_errors=s[6])

    def analysis(self):
        t = C.create_string_buffer(64)
        ls = C.create_string_buffer(64)
        tol, mi, rs = C.c_double(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.stan_host_db_get_analysis(self.h, t, ls, C.c_int32(64), C.byref(tol),
                                                     C.byref(mi), C.byref(rs)), "get_analysis")
        return dict(type=t.value.decode(), lin_solver=ls.value.decode(), tol=tol.value,
                    max_iter=mi.value, result_step=rs.value)

    def assign_dof(self):
        self._chk(self.lib.stan_host_db_assign_dof(self.h), "assign_dof")

    def flat(self):
        s = self.sizes()
        n, e, nm = s["nodes"], s["elements"], max(s["materials"], 1)
        out = dict(xyz=np.zeros((n, 3)), node_ids=np.zeros(n, np.int32),
                   node_dof=np.zeros((n, 3), np.int32), conn=np.zeros((e, 8), np.int32),
                   elem_ids=np.zeros(e, np.int32), elem_mat=np.zeros(e, np.int32),
                   elem_type=np.zeros(e, np.uint8), mat_E_nu=np.zeros((nm, 2)))
        nmat = C.c_int32(0)
        self._chk(self.lib.stan_host_db_get_flat(
            self.h, _p(out["xyz"], C.c_double), _p(out["node_ids"], C.c_int32),
            _p(out["node_dof"], C.c_int32), _p(out["conn"], C.c_int32), _p(out["elem_ids"], C.c_int32),
            _p(out["elem_mat"], C.c_int32), _p(out["elem_type"], C.c_uint8),
            _p(out["mat_E_nu"], C.c_double), C.c_int32(nm), C.byref(nmat)), "get_flat")
        out["mat_E_nu"] = out["mat_E_nu"][:nmat.value]
        return out

    def reduction(self):
        ndof = self.sizes()["nDOF"]
        red = np.zeros(ndof, np.int32)
        F = np.zeros(max(ndof, 1))
        nfix = C.c_int64(0)
        self._chk(self.lib.stan_host_db_get_reduction(self.h, _p(red, C.c_int32), C.byref(nfix),
                                                      _p(F, C.c_double)), "get_reduction")
        return red, int(nfix.value), F[:ndof - nfix.value].copy()

    def distributed_loads(self):
        """BuildDistributedLoads: dict(any, mat_body [n_mat, 3] or None, face_elem, face_id, face_p (or None), disp0
        [n_nodes, 3] or None, n_prescribed) from the "Pressure" / "BodyForce" / "Displacement" BCs (needs assign_dof)."""
        cnt = (C.c_int64 * 4)()
        self._chk(self.lib.stan_host_db_get_distributed_loads(self.h, cnt, C.c_int32(0), None, C.c_int64(0), None, None, None,
                                                              None), "distributed_loads")
        nm, nf, nn = int(cnt[1]), int(cnt[2]), self.sizes()["nodes"]
        mb = np.zeros((max(nm, 1), 3))
        fe, fi, fp = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.uint8), np.zeros(max(nf, 1))
        u0 = np.zeros((nn, 3))
        self._chk(self.lib.stan_host_db_get_distributed_loads(
            self.h, cnt, C.c_int32(mb.shape[0]), _p(mb, C.c_double), C.c_int64(fe.shape[0]), _p(fe, C.c_int32),
            _p(fi, C.c_uint8), _p(fp, C.c_double), _p(u0, C.c_double)), "distributed_loads")
        return dict(any=bool(cnt[0]), mat_body=mb[:nm] if nm else None, face_elem=fe[:nf] if nf else None,
                    face_id=fi[:nf] if nf else None, face_p=fp[:nf] if nf else None,
                    disp0=u0 if np.any(u0) else None, n_prescribed=int(cnt[3]))

    def thermal_loads(self):
        """BuildThermalLoads: dict(any, mat_alpha [n_mat], dT [n_nodes]) from the "Temperature" / "ThermalExpansion" BCs."""
        cnt = (C.c_int64 * 2)()
        self._chk(self.lib.stan_host_db_get_thermal_loads(self.h, cnt, C.c_int32(0), None, None), "thermal_loads")
        nm, nn = int(cnt[1]), self.sizes()["nodes"]
        al, dT = np.zeros(max(nm, 1)), np.zeros(nn)
        self._chk(self.lib.stan_host_db_get_thermal_loads(self.h, cnt, C.c_int32(al.shape[0]), _p(al, C.c_double),
                                                          _p(dT, C.c_double)), "thermal_loads")
        return dict(any=bool(cnt[0]), mat_alpha=al[:nm], dT=dT)

    def density(self):
        """BuildDensity: dict(any, mat_rho [n_mat]) from the "Density" BCs (material IDs, component 0 = rho; they add up)."""
        cnt = (C.c_int64 * 2)()
        self._chk(self.lib.stan_host_db_get_density(self.h, cnt, C.c_int32(0), None), "density")
        nm = int(cnt[1])
        rho = np.zeros(max(nm, 1))
        self._chk(self.lib.stan_host_db_get_density(self.h, cnt, C.c_int32(rho.shape[0]), _p(rho, C.c_double)), "density")
        return dict(any=bool(cnt[0]), mat_rho=rho[:nm])

    def set_results(self, disp, strain=None, stress=None):
        disp = np.ascontiguousarray(disp, dtype=np.float64)
        if strain is not None:
            strain = np.ascontiguousarray(strain, dtype=np.float64)
            stress = np.ascontiguousarray(stress, dtype=np.float64)
        self._chk(self.lib.stan_host_db_set_results(
            self.h, _p(disp, C.c_double), None if strain is None else _p(strain, C.c_double),
            None if stress is None else _p(stress, C.c_double)), "set_results")

    def results(self, inc=1, with_stress=True):
        s = self.sizes()
        disp = np.zeros((s["nodes"], 3))
        strain = np.zeros((s["elements"], 8, 6))
        stress = np.zeros((s["elements"], 8, 6))
        self._chk(self.lib.stan_host_db_get_results(
            self.h, C.c_int32(inc), _p(disp, C.c_double),
            _p(strain, C.c_double) if with_stress else None,
            _p(stress, C.c_double) if with_stress else None), "get_results")
        return disp, strain, stress
