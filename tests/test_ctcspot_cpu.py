"""CPU: CTC phrase spotting — the host twin (pf_host_ctc_spot, csrc/hostutil.cpp) against the definition
(tests/ctcspot_ref.py) over the shared case table.  The table's inputs lie on a grid where float32 and float64 agree exactly
(asserted here, before anything reaches a GPU), so counts, frames and score bits must be identical.  One more case runs real
log-softmax rows against a float32 run of the same definition, bit for bit."""
import numpy as np
import pytest

import ctcspot_ref as R
from aliparaformerasr_amd.engine import host_ctc_spot


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(tag, got, k, ref):
    n, be, sc = ref
    assert int(got.n_hits[0, k]) == n, (tag, k, got.n_hits[0, k], n)
    np.testing.assert_array_equal(got.begin_end[0, k], be, err_msg="%s phrase %d" % (tag, k))
    np.testing.assert_array_equal(_bits(got.score[0, k]), _bits(sc), err_msg="%s phrase %d" % (tag, k))


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_host_twin_equals_reference_on_the_grid(case):
    tag, lp, phrases, thr, max_hits, expect = case
    assert R.on_grid(lp, thr), tag
    for k, y in enumerate(phrases):
        ref = R.spot(lp, y, thr, max_hits)
        if expect is not None:
            assert ref[0] == expect[k], (tag, ref)
        _same(tag, host_ctc_spot(lp, y, thr, max_hits), 0, ref)


def test_host_twin_equals_float32_reference_on_log_softmax_rows():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((50, 12)).astype(np.float32) * 3
    lp = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    hits = 0
    for y in ([5], [5, 5], [5, 6], [1, 2, 3, 4], list(range(1, 12))):
        ref = R.spot(lp, y, np.float32(-2.5), 6, dtype=np.float32)
        _same("log-softmax", host_ctc_spot(lp, y, -2.5, 6), 0, ref)
        hits += ref[0]
    assert hits >= 5

