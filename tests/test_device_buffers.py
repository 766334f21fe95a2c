"""The checker of tests/device_buffers.py on CPU tensors: it must see each thing the device tests rely on it to see."""
import numpy as np
import pytest
import torch

from tests import device_buffers as B

CPU = torch.device("cpu")


def _out(n=10, offset=0):
    return B.output("U", n, B.guard_len(5), CPU, offset)


def _written(g):
    g.payload.copy_(torch.arange(g.n, dtype=torch.float64))
    return g


def test_a_fully_written_output_with_clean_guards_passes():
    g = _written(_out())
    assert g.problems() == []
    B.check([g])
    assert g.front.numel() >= B.MIN_GUARD and g.back.numel() >= B.MIN_GUARD
    assert np.array_equal(g.numpy(), np.arange(10.0))


def test_guard_len_covers_the_unreduced_index_and_the_largest_block():
    assert B.guard_len(0) == B.guard_len(8192) == 8192 and B.guard_len(100000) == 100000
    assert B.MIN_GUARD > 32 * 48                                   # k_recover's block: 32 elements x 48 doubles


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_store_into_the_front_guard_is_flagged(where):
    g = _written(_out())
    g.alloc[g.start - 1 if where == "last" else 0] = 1.5
    found = g.problems()
    assert len(found) == 1 and "front guard" in found[0]
    with pytest.raises(AssertionError):
        B.check([g])


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_store_into_the_back_guard_is_flagged(where):
    g = _written(_out())
    g.alloc[g.start + g.n if where == "first" else -1] = 0.0       # (a stored zero is a store)
    found = g.problems()
    assert len(found) == 1 and "back guard" in found[0] and (where == "last" or "indices 10 .. 10" in found[0])


def test_an_unwritten_payload_entry_is_flagged():
    g = _written(_out())
    B._bits(g.payload)[7] = B.UNWRITTEN_BITS
    found = g.problems()
    assert len(found) == 1 and "never written" in found[0] and "first at 7" in found[0]
    assert g.problems(written=False) == []                         # after an error code only the guards are looked at
    fresh = _out()
    assert "10 payload entries never written" in fresh.problems()[0]


def test_a_stored_nan_is_not_mistaken_for_either_pattern():
    g = _written(_out())
    g.payload[3] = float("nan")
    assert g.problems() == []
    g.front[5] = float("nan")                                      # ... and an ordinary NaN in a guard is a store
    assert "front guard" in g.problems()[0]


def test_refill_restores_an_output():
    g = _written(_out())
    g.alloc[0] = 2.0
    g.refill()
    assert [p for p in g.problems() if "guard" in p] == [] and "never written" in g.problems()[0]


@pytest.mark.parametrize("values,fill", [(np.arange(12.0), None), (np.arange(12, dtype=np.int32), None),
                                         (np.full(12, 1, np.uint8), B.HEX8_G2)])
def test_a_modified_input_is_flagged(values, fill):
    g = B.input_("x", values, B.guard_len(0), CPU, 0, fill)
    assert g.problems() == [] and np.array_equal(g.numpy(), values)
    for idx in (g.start + 4, 0, g.alloc.numel() - 1):              # payload, front guard, back guard
        keep = g.alloc[idx].clone()
        g.alloc[idx] = 7
        assert len(g.problems()) == 1 and "input modified" in g.problems()[0]
        g.alloc[idx] = keep
        assert g.problems() == []
    if values.dtype == np.float64:
        assert bool(torch.isnan(g.front).all()) and bool(torch.isnan(g.back).all())
    else:
        assert bool((g.front == (fill or 0)).all()) and bool((g.back == (fill or 0)).all())


@pytest.mark.parametrize("dtype,item", [(np.float64, 8), (np.int32, 4), (np.uint8, 1)])
@pytest.mark.parametrize("offset", [0, 1])
def test_offset_places_the_payload_one_element_past_a_256_byte_boundary(dtype, item, offset):
    g = B.input_("x", np.zeros(33, dtype), B.guard_len(0), CPU, offset)
    assert g.ptr % B.ALIGN == offset * item
    assert g.ptr == g.payload.data_ptr()
    o = B.output("U", 33, B.guard_len(0), CPU, offset)
    assert o.ptr % B.ALIGN == offset * 8


def test_mesh_holds_the_job_and_null_pointers_without_elements(built_libs):
    from stan_amd import problem
    job = problem.cube_job(1)
    m = B.Mesh(job, CPU, offset=1, disp=np.ones_like(job.xyz))
    assert m.assemble_args()[0] == 8 and m.assemble_args()[3] == 1 and m.assemble_args()[8] == 24
    assert np.array_equal(m.conn.numpy().reshape(-1, 8), job.conn) and np.array_equal(m.xyz.numpy().reshape(-1, 3), job.xyz)
    assert len(m.inputs) == 7 and B.problems(m.inputs) == []
    assert bool((m.elem_type.front == B.HEX8_G2).all())
    empty = B.Mesh(job, CPU, conn=np.zeros((0, 8), np.int32), elem_mat=np.zeros(0, np.int32), elem_type=np.zeros(0, np.uint8))
    assert empty.n_elem == 0 and empty.assemble_args()[4:7] == (0, 0, 0)
