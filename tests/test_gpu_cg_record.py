"""The CG loops against tests/golden/cg_loop_record.json: same bits of U, same report, and the same number of kernel
launches, enqueued iterations, collectives and stream waits as the commit the record was made at
(tests/golden/make_cg_loop_record.py, which also defines the cases: small and large-system product kernels, padded and
folded streams, every loop form one option at a time, the batched loop).  A host-side change of cg.hip that moves a bit
or an enqueue fails here in seconds.  The hashes are tied to the compiler and the device generation; the generator's
docstring says when to regenerate them."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_cg_loop_record", os.path.join(GOLDEN, "make_cg_loop_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def record():
    with open(GEN.RECORD) as f:
        return json.load(f)


def test_the_record_holds_every_case(record):
    assert sorted(record) == sorted(GEN.key(n, m) for n in GEN.SIZES for m, _, _ in GEN.MATRIX_FORMS)


@pytest.mark.parametrize("n", GEN.SIZES)
@pytest.mark.parametrize("matrix_form", [m for m, _, _ in GEN.MATRIX_FORMS])
def test_cg_loops_compute_and_enqueue_what_the_record_says(gpu_ctx, record, n, matrix_form):
    want = record[GEN.key(n, matrix_form)]
    got = GEN.cases(gpu_ctx, n, matrix_form)
    assert sorted(got) == sorted(want)
    wrong = {c: {f: (got[c].get(f), want[c].get(f)) for f in sorted(set(got[c]) | set(want[c])) if got[c].get(f) != want[c].get(f)}
             for c in sorted(want) if got[c] != want[c]}
    assert not wrong, "(computed, recorded) per case and field: %r" % wrong
