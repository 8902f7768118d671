"""CPU: the CTC decoding feature without a device — the numpy reference of the collapse pinned by hand-derived cases, the
new C ABI symbols (exported, declared in _native.SIGNATURES, refusing a null handle), and the `-decode` option of the
examples harness."""
import ctypes as C

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import examples as ex
from ctc_ref import collapse_one, collapse_ref, timestamps_ms

A, B_, BL = 7, 9, 0
NEW = ("pf_engine_set_decode", "pf_fetch_scores", "pf_fetch_ctc", "pf_op_ctc_collapse", "pf_recognizer_set_decode",
       "pf_stream_scores")


def _f(*v):
    return np.asarray(v, np.float32)


def test_reference_a_a_blank_a_b_b():
    # frames: a a _ a b b ; the blank separates two tokens of the same id, the b run is one token
    s = _f(-0.5, -0.25, -0.1, -1.0, -0.75, -0.125)
    got = collapse_one([A, A, BL, A, B_, B_], s, 6)
    assert [(y, f, l) for y, f, l, _ in got] == [(A, 0, 1), (A, 3, 3), (B_, 4, 5)]
    assert [float(x[3]) for x in got] == [-0.25, -1.0, -0.125]          # the largest frame log-prob of each run


def test_reference_all_blank_and_len_zero():
    assert collapse_one([BL] * 5, _f(0, 0, 0, 0, 0), 5) == []
    assert collapse_one([A, A, B_], _f(-1, -2, -3), 0) == []
    n, ids, first, last, score = collapse_ref([[BL, BL], [A, B_]], [[-1, -1], [-1, -1]], [2, 0])
    assert n.tolist() == [0, 0] and ids.shape == (2, 0)


def test_reference_run_cut_by_len():
    # a a a b with len 2: the run ends at frame 1 with the maximum over frames 0..1 only; b is never seen
    got = collapse_one([A, A, A, B_], _f(-3.0, -2.0, -0.5, -0.1), 2)
    assert [(y, f, l, float(s)) for y, f, l, s in got] == [(A, 0, 1, -2.0)]


def test_reference_blank_at_frame_zero_and_single_frame():
    got = collapse_one([BL, A, A], _f(-0.1, -0.2, -0.3), 3)
    assert [(y, f, l, float(s)) for y, f, l, s in got] == [(A, 1, 2, np.float32(-0.2))]
    assert [(y, f, l, float(s)) for y, f, l, s in collapse_one([B_], _f(-0.7), 1)] == [(B_, 0, 0, np.float32(-0.7))]
    assert collapse_one([BL], _f(-0.7), 1) == []


def test_reference_padded_layout_and_timestamps():
    ids = [[A, A, BL, A, B_, B_], [BL, B_, B_, B_, A, A]]
    sc = [[-0.5, -0.25, -0.1, -1.0, -0.75, -0.125], [-0.1, -0.2, -0.3, -0.4, -0.6, -0.5]]
    n, o, first, last, score = collapse_ref(ids, sc, [6, 4], cap=4)
    assert n.tolist() == [3, 1]
    assert o.tolist() == [[A, A, B_, -1], [B_, -1, -1, -1]] and o.dtype == np.int64
    assert first.tolist() == [[0, 3, 4, -1], [1, -1, -1, -1]]
    assert last.tolist() == [[1, 3, 5, -1], [3, -1, -1, -1]]
    assert score.tolist() == [[-0.25, -1.0, -0.125, 0.0], [np.float32(-0.2), 0.0, 0.0, 0.0]]
    # lens beyond T are clamped; a run inside the four prompt rows gets {0, 0}
    assert collapse_ref(ids, sc, [99, -3])[0].tolist() == [3, 0]
    assert timestamps_ms([0, 3, 4, 10], [1, 3, 5, 12]) == [[0, 0], [0, 0], [0, 120], [360, 540]]


def test_new_symbols_are_exported_and_declared():
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert (N.PF_DECODE_SCORES, N.PF_DECODE_CTC) == (1, 2)
    assert lib.pf_version() == 6                      # additions only: the ABI number stays


def test_null_handles_are_refused():
    lib = N.load()
    n = C.c_int32()
    p = C.POINTER(C.c_float)()
    assert lib.pf_engine_set_decode(None, 1) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_scores(None, None, 0, n) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_ctc(None, None, None, None, None, 0, None, n) == N.PF_ERR_INVALID_ARG
    assert lib.pf_op_ctc_collapse(None, None, None, None, 1, 1, 0, None, None, None, None, 1, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_recognizer_set_decode(None, 2) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_scores(None, C.byref(p), n) == N.PF_ERR_INVALID_ARG


def test_examples_decode_option():
    cfg = ex.parse_args(["-type", "offline", "-decode", "ctc", "-files", "a.wav"])
    assert cfg["decode"] == "ctc" and cfg["files"] == ["a.wav"]
    assert ex.parse_args(["-type", "offline", "-decode", "frames"])["decode"] == "frames"
    assert "decode" not in ex.parse_args(["-type", "offline"])          # default: the reference's per-frame ids
    with pytest.raises(ValueError, match="decode"):
        ex.parse_args(["-type", "offline", "-decode", "bogus"])
    with pytest.raises(ValueError, match="decode"):
        ex.parse_args(["-type", "offline", "-decode"])
    with pytest.raises(ValueError, match="Unknown parameters"):
        ex.parse_args(["-type", "offline", "-decoding", "ctc"])
