"""Guarded arrays for the entries that take the caller's own device memory (stan_hip_*_dev): what the host entries hide behind
the library's own rounded-up pool blocks -- a store one element past the end, a store at an unreduced DOF index, a ragged last
wave that does not stop at n_elem, an output entry that no kernel writes, a `const` argument that does not stay const.

One torch allocation per array: [front guard | payload | back guard]; the library gets the payload's address (Guarded.ptr).

  guard size   guard_len(n_dof) = max(8192, n_dof) elements on each side: a condition, not a measurement.  It exceeds the
               largest block footprint of a kernel that stores through a caller's pointer (k_recover: 32 elements x 48 doubles
               = 1536 per workgroup) and n_dof - N, so that a store at an unreduced DOF index lands in the guard and not
               outside the allocation.
  outputs      guards hold GUARD_BITS, the payload UNWRITTEN_BITS: two NaN patterns no kernel produces, compared through an
               int64 view -- a touched guard and an entry that was never written can be told from anything that was stored.
  inputs       guards hold values that are valid as data (NaN for coordinates, displacements and loads; 0 for indices; HEX8_G2
               for element types): an over-read can poison a result but never becomes an out-of-range index.  The WHOLE
               allocation is compared bit for bit with a clone taken before the call.
  offset=k     the payload starts k elements past a 256-byte boundary (offset=0: on one): natural alignment only, which is
               all the header promises a kernel.

The arrays live on any torch device: tests/test_device_buffers.py runs the checker on the CPU."""
import numpy as np
import torch

GUARD_BITS = 0x7FF8_4755_4152_4421       # quiet NaNs with a payload of their own ("GUARD!", "UNWRIT")
UNWRITTEN_BITS = 0x7FF8_554E_5752_4954
MIN_GUARD = 8192
ALIGN = 256
HEX8_G2 = 2

_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


def guard_len(n_dof=0):
    return max(MIN_GUARD, int(n_dof))


def _bits(t):
    """The tensor as integers of its own width (a NaN compares equal to itself this way)."""
    return t.view(torch.int64) if t.dtype == torch.float64 else t


class Guarded:
    """One guarded array.  alloc: the whole allocation; payload: the n elements the library is given; front / back: the
    guards (everything else in the allocation, at least `guard` elements each)."""

    def __init__(self, name, n, dtype, guard, device, offset, output):
        self.name, self.n, self.output = name, int(n), output
        item = torch.empty(0, dtype=dtype).element_size()
        slack = ALIGN // item + 1
        self.alloc = torch.empty(2 * guard + self.n + slack, dtype=dtype, device=device)
        # the first index >= guard whose address is `offset` elements past a 256-byte boundary
        want = (offset * item) % ALIGN
        start = guard
        while (self.alloc.data_ptr() + start * item) % ALIGN != want:
            start += 1
        assert start - guard < slack
        self.start = start
        self.front, self.payload, self.back = self.alloc[:start], self.alloc[start:start + self.n], self.alloc[start + self.n:]
        assert self.front.numel() >= guard and self.back.numel() >= guard
        self.before = None

    @property
    def ptr(self):
        return self.alloc.data_ptr() + self.start * self.alloc.element_size()

    def numpy(self):
        """The payload on the host."""
        return self.payload.cpu().numpy().copy()

    def refill(self):
        """An output back to its state before the call: guards and payload."""
        assert self.output
        _bits(self.alloc).fill_(GUARD_BITS)
        _bits(self.payload).fill_(UNWRITTEN_BITS)

    def snapshot(self):
        """An input as it is now: what problems() compares it with."""
        assert not self.output
        self.before = self.alloc.clone()

    def problems(self, written=True):
        """What is wrong with this array after a call, as a list of sentences (empty: nothing).  written=False: the payload
        of an output is not looked at (after an error code only the guards are promised)."""
        out = []
        if not self.output:
            same = _bits(self.alloc) == _bits(self.before)
            if not bool(same.all()):
                first = int(torch.nonzero(~same)[0]) - self.start
                out.append("%s: input modified, %d entries, the first at payload index %d" % (self.name, int((~same).sum()), first))
            return out
        for side, t, base in (("front", self.front, -self.start), ("back", self.back, self.n)):
            hit = _bits(t) != GUARD_BITS
            if bool(hit.any()):
                idx = torch.nonzero(hit).reshape(-1)
                out.append("%s: store into the %s guard, %d entries, payload indices %d .. %d" %
                           (self.name, side, idx.numel(), int(idx[0]) + base, int(idx[-1]) + base))
        if written and self.n:
            un = _bits(self.payload) == UNWRITTEN_BITS
            if bool(un.any()):
                out.append("%s: %d payload entries never written, the first at %d" % (self.name, int(un.sum()), int(torch.nonzero(un)[0])))
        return out


def output(name, n, guard, device, offset=0):
    """A float64 output of n entries: guards GUARD_BITS, payload UNWRITTEN_BITS."""
    g = Guarded(name, n, torch.float64, guard, device, offset, True)
    g.refill()
    return g


def input_(name, values, guard, device, offset=0, fill=None):
    """An input holding `values` (float64, int32 or uint8; flattened).  fill: what the guards hold (default NaN for float64,
    0 for the integers)."""
    v = np.ascontiguousarray(values).reshape(-1)
    g = Guarded(name, v.shape[0], _TORCH[v.dtype], guard, device, offset, False)
    if fill is None:
        fill = float("nan") if v.dtype == np.float64 else 0
    g.alloc.fill_(fill)
    if v.shape[0]:
        g.payload.copy_(torch.from_numpy(v))
    g.snapshot()
    return g


def problems(arrays, written=True):
    return [p for a in arrays for p in a.problems(written)]


def check(arrays, written=True):
    """Guards intact, every output entry written (unless written=False), inputs unchanged."""
    found = problems(arrays, written)
    assert not found, "; ".join(found)


class Mesh:
    """The mesh arrays of a job as guarded inputs, in the argument order of the device-pointer entries.  xyz, conn, elem_mat,
    elem_type, node_dof, disp: replacements for the job's (disp: none by default)."""

    def __init__(self, job, device, offset=0, disp=None, **replace):
        a = lambda k, dt: np.ascontiguousarray(replace.get(k, getattr(job, k, None)), dtype=dt)
        self.n_nodes, self.n_dof = int(job.xyz.shape[0]), int(job.red.shape[0])
        self.mat_E_nu = np.ascontiguousarray(job.mat_E_nu, dtype=np.float64)
        g = guard_len(self.n_dof)
        mk = lambda k, v, fill=None: input_(k, v, g, device, offset, fill)
        conn = a("conn", np.int32).reshape(-1, 8)
        self.n_elem = int(conn.shape[0])
        self.xyz, self.node_dof = mk("xyz", a("xyz", np.float64)), mk("node_dof", a("node_dof", np.int32))
        self.conn, self.elem_mat = mk("conn", conn), mk("elem_mat", a("elem_mat", np.int32))
        self.elem_type = mk("elem_type", a("elem_type", np.uint8), HEX8_G2)
        self.red = mk("red", a("red", np.int32))
        self.disp = None if disp is None else mk("disp", np.ascontiguousarray(disp, dtype=np.float64))
        self.inputs = [x for x in (self.xyz, self.node_dof, self.conn, self.elem_mat, self.elem_type, self.red, self.disp) if x is not None]

    def _e(self, g):
        return g.ptr if self.n_elem else 0    # no elements: null element pointers (the argument checks allow them)

    def assemble_args(self):
        return (self.n_nodes, self.xyz.ptr, self.node_dof.ptr, self.n_elem, self._e(self.conn), self._e(self.elem_mat),
                self._e(self.elem_type), self.mat_E_nu, self.n_dof, self.red.ptr)

    def recover_args(self):
        return (self.n_nodes, self.xyz.ptr, self.disp.ptr, self.n_elem, self._e(self.conn), self._e(self.elem_mat),
                self._e(self.elem_type), self.mat_E_nu)
