"""GPU: the phrase-spotting kernel (csrc/k_ctcspot.hip) through pf_op_ctc_spot against the float64 definition
(tests/ctcspot_ref.py) on the shared grid cases, everything equal, and against the host twin bit for bit on log-softmax rows.

Every case runs as B = 3 utterances over the same rows with len = (T, 5, 0); rows at and beyond each length hold +huge and
NaN, the row stride is V + 5 with +inf in the pad, and the op itself checks that every output slot was written and that the
sentinel cells behind the result block kept their bits."""
import numpy as np
import pytest

import ctcspot_ref as R
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import host_ctc_spot

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


def _batch(lp):
    T, V = lp.shape
    lens = np.array([T, min(T, 5), 0], np.int32)
    x = np.empty((3, T, V + 5), np.float32)
    x[:, 0::2], x[:, 1::2] = 3e38, np.nan                                      # what lies at and beyond each length
    for b in range(3):
        x[b, : lens[b], :V] = lp[: lens[b]]
    x[:, :, V:] = np.inf
    return x, lens


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_kernel_equals_reference_on_the_grid(any_engine, case):
    tag, lp, phrases, thr, max_hits, _ = case
    x, lens = _batch(lp)
    got = any_engine.op_ctc_spot(x, phrases, lens, thr, max_hits, V=lp.shape[1])
    for b in range(3):
        for k, y in enumerate(phrases):
            n, be, sc = R.spot(lp[: lens[b]], y, thr, max_hits)
            assert int(got.n_hits[b, k]) == n, (tag, b, k)
            np.testing.assert_array_equal(got.begin_end[b, k], be, err_msg="%s b=%d k=%d" % (tag, b, k))
            np.testing.assert_array_equal(_bits(got.score[b, k]), _bits(sc), err_msg="%s b=%d k=%d" % (tag, b, k))


def test_kernel_equals_host_twin_on_log_softmax_rows(any_engine):
    rng = np.random.default_rng(4)
    z = rng.standard_normal((50, 12)).astype(np.float32) * 3
    lp = (z - np.log(np.exp(z.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    phrases = [[5], [5, 5], [5, 6], [1, 2, 3, 4], list(range(1, 12))]
    x, lens = _batch(lp)
    got = any_engine.op_ctc_spot(x, phrases, lens, -2.5, 6, V=12)
    for b in range(3):
        for k, y in enumerate(phrases):
            ref = host_ctc_spot(lp[: lens[b]], y, -2.5, 6)
            assert got.n_hits[b, k] == ref.n_hits[0, 0]
            np.testing.assert_array_equal(got.begin_end[b, k], ref.begin_end[0, 0])
            np.testing.assert_array_equal(_bits(got.score[b, k]), _bits(ref.score[0, 0]))
