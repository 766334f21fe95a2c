"""The block kernels and the two block drivers (modes, buckling) against tests/golden/block_record.json: the same bits of
every output and the same report as the commit the record was made at (tests/golden/make_block_record.py, which also
defines the cases: the gram and rotate kernels alone on every width they are built for, the drivers on the models of
their own tests, as tested, after one outer step and with a block of 20 columns).  A change of modal.hip, api_modal.hip or
api_buckling.hip that reorders one sum fails here in seconds.  The hashes are tied to the compiler and the device
generation; the generator's docstring says when to regenerate them."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_block_record", os.path.join(GOLDEN, "make_block_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def record():
    with open(GEN.RECORD) as f:
        return json.load(f)


def _differences(got, want):
    """{case: {field: (computed, recorded)}} where the two differ"""
    assert sorted(got) == sorted(want)
    flat = lambda r: {(c, f): v for c, d in r.items() for f, v in (d.items() if isinstance(d, dict) else [("", d)])}     # noqa: E731
    g, w = flat(got), flat(want)
    return {key: (g.get(key), w.get(key)) for key in sorted(set(g) | set(w), key=str) if g.get(key) != w.get(key)}


def test_the_record_holds_every_case(record):
    assert sorted(record) == sorted(GEN.keys())


@pytest.mark.parametrize("N", GEN.BLOCK_N)
def test_block_kernels_compute_what_the_record_says(gpu_ctx, record, N):
    for q in GEN.BLOCK_Q:
        wrong = _differences(GEN.block_case(gpu_ctx, N, q), record[GEN.block_key(N, q)])
        assert not wrong, "N %d q %d, (computed, recorded) per call and output: %r" % (N, q, wrong)


@pytest.mark.parametrize("name", GEN.MODES_MODELS)
def test_modes_compute_what_the_record_says(gpu_ctx, record, name):
    got = GEN.modes_cases(gpu_ctx, name)
    wrong = _differences(got, {run: record["modes/%s/%s" % (name, run)] for run in got})
    assert not wrong, "(computed, recorded) per run and field: %r" % wrong


@pytest.mark.parametrize("name", GEN.BUCKLING_MODELS)
def test_buckling_computes_what_the_record_says(gpu_ctx, record, name):
    got = GEN.buckling_cases(gpu_ctx, name)
    wrong = _differences(got, {run: record["buckling/%s/%s" % (name, run)] for run in got})
    assert not wrong, "(computed, recorded) per run and field: %r" % wrong
