"""CPU: voice-activity segmentation — the definition (tests/vad_ref.py) on the known answers of the design, the host forms
(pf_host_vad_levels / pf_host_vad_segments / pf_host_long_plan, csrc/hostutil.cpp) against the definition exactly (every value
is an integer: no tolerance exists), a fuzz over random telegraph signals and random valid configurations, the edges of the
window and of the percentile, every PF_ERR_INVALID_ARG constraint, the level's special values, and the batch plan."""
import ctypes as C

import numpy as np
import pytest

import vad_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import host_long_plan, host_vad_levels, host_vad_segments, vad_config

NEW = ("pf_vad_default", "pf_vad_segment", "pf_host_vad_levels", "pf_host_vad_segments", "pf_host_long_plan", "pf_op_vad_levels",
       "pf_op_vad_segments")
def _host(e, c, n_mels=80, lfr_n=6):
    return [tuple(p) for p in host_vad_segments(e, n_mels, c, lfr_n).tolist()]


def test_symbols_are_exported():
    lib = N.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES, name


def test_default_configuration_is_the_stated_one():
    c = vad_config()
    assert c.struct_size == C.sizeof(N.PfVadConfig) == 64
    assert {k: getattr(c, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert R.valid(R.DEFAULTS)
    assert N.load().pf_vad_default(None) == N.PF_ERR_INVALID_ARG


@pytest.mark.parametrize("case", R.known_answers(), ids=lambda c: c[0])
def test_known_answers_definition_and_host_form(case):
    _tag, e, over, want = case
    c = R.config(**over)
    assert R.segments(e, 80, c) == want
    # (min_speech = 10 is below 2 * lfr_n of the LFR front-end: those rows are a front-end without LFR, lfr_n = 1)
    assert _host(e, over, lfr_n=1 if over.get("min_speech", 50) < 12 else 6) == want


def test_fuzz_host_form_equals_the_definition():
    """500 random telegraph signals, T 1 .. 3000, random valid configurations (window = on = off = 1, pads 0, split_search 0
    among them): host == definition, and every list is ascending, disjoint and inside [min_speech, max_len]."""
    rng = np.random.default_rng(20240611)
    n_seg = n_split = 0
    for it in range(500):
        lfr_n = int(rng.choice([1, 6]))
        c = R.random_config(rng, lfr_n)
        if it % 25 == 0:
            c.update(window=1, on_count=1, off_count=1, pad_begin=0, pad_end=0, split_search=0, max_len=2 * c["min_speech"])
        assert R.valid(c, lfr_n), c
        T = int(rng.integers(1, 3001))
        e = R.telegraph(rng, T, mean_run=int(rng.choice([3, 15, 60, 400])), jitter=int(rng.choice([0, 0, 3, 4000])))
        n_mels = int(rng.choice([80, 1, 128]))
        want = R.segments(e, n_mels, c)
        assert _host(e, c, n_mels, lfr_n) == want, (it, c, T)
        prev = 0
        for b, en in want:
            assert prev <= b < en <= T and c["min_speech"] <= en - b <= c["max_len"], (it, c, want)
            prev = en
        n_seg += len(want)
        n_split += sum(1 for (b0, e0), (b1, e1) in zip(want, want[1:]) if e0 == b1)
    assert n_seg > 1000 and n_split > 100, (n_seg, n_split)       # the fuzz reaches the split


@pytest.mark.parametrize("floor_pct", [-1, 0, 100])
def test_window_edges_and_percentile_edges(floor_pct):
    rng = np.random.default_rng(5 + floor_pct)
    for window, on, off in ((20, 15, 15), (1, 1, 1), (7, 7, 1), (256, 1, 256)):
        for T in sorted({0, 1, max(window - 1, 0), window, window + 1, 3 * window + 5}):
            for trial in range(4):
                e = R.telegraph(rng, T, mean_run=5, jitter=2) if T else np.zeros(0, np.int32)
                c = R.config(floor_pct=floor_pct, abs_level=9000 if floor_pct == -1 else R.INT32_MIN, margin_q=0 if trial & 1 else 96,
                             window=window, on_count=on, off_count=off, min_speech=2, max_len=8, split_search=3, pad_begin=trial, pad_end=1)
                want = R.segments(e, 80, c)
                assert _host(e, c, 80, 1) == want, (window, T, trial)
                if T == 0:
                    assert want == []


def test_every_constraint_is_invalid_arg():
    lib = N.load()
    e = R.lv((R.Q, 100), (R.S, 200), (R.Q, 100))
    bad = [dict(floor_pct=-2), dict(floor_pct=101), dict(window=0), dict(window=257, on_count=200, off_count=200), dict(on_count=0),
           dict(on_count=21), dict(off_count=0), dict(off_count=21), dict(on_count=10, off_count=10), dict(pad_begin=-1),
           dict(pad_begin=1025), dict(pad_end=-1), dict(pad_end=1025), dict(min_speech=11), dict(split_search=-1),
           dict(split_search=1025, max_len=5000), dict(max_len=599), dict(min_speech=1500)]
    seg, n = np.zeros((64, 2), np.int32), C.c_int32()
    i32 = C.POINTER(C.c_int32)
    for over in bad:
        assert not R.valid(R.config(**over)), over
        rc = lib.pf_host_vad_segments(e.ctypes.data_as(i32), e.size, 80, 6, C.byref(vad_config(**over)), seg.ctypes.data_as(i32), 64, n)
        assert rc == N.PF_ERR_INVALID_ARG, (over, rc)
    # the boundary values themselves pass
    for over in (dict(floor_pct=-1), dict(floor_pct=100), dict(window=256, on_count=256, off_count=1), dict(pad_begin=1024, pad_end=1024),
                 dict(min_speech=12), dict(split_search=1024, max_len=1124), dict(max_len=600), dict(split_search=0, max_len=100)):
        assert R.valid(R.config(**over)), over
        assert _host(e, over) == R.segments(e, 80, R.config(**over)), over
    # min_speech is measured against the front-end's lfr_n
    assert _host(e, dict(min_speech=2, max_len=504), lfr_n=1) == R.segments(e, 80, R.config(min_speech=2, max_len=504))
    c = vad_config()
    c.struct_size = 60
    assert lib.pf_host_vad_segments(e.ctypes.data_as(i32), e.size, 80, 6, C.byref(c), seg.ctypes.data_as(i32), 64, n) == N.PF_ERR_INVALID_ARG
    # capacity: the count is reported
    rc = lib.pf_host_vad_segments(e.ctypes.data_as(i32), e.size, 80, 6, None, None, 0, n)
    assert rc == N.PF_ERR_CAPACITY and n.value == 1


def test_host_levels_special_values():
    one = lambda v: int(host_vad_levels(np.array([[v]], np.float32))[0])
    assert [one(v) for v in (np.nan, -np.inf, np.inf, 64, -64, 64.01, -64.01, 1e30)] == [-4096, -4096, 4096, 4096, -4096, 4096, -4096, 4096]
    assert [one(k / 128.0) for k in (1, 3, 5, -1, -3, 255, 257)] == [0, 2, 2, 0, -2, 128, 128]          # half to even
    for T, m in ((1, 80), (65, 80), (7, 3), (33, 128)):
        x = R.special_rows(T, m, seed=T)
        np.testing.assert_array_equal(host_vad_levels(x), R.levels(x))
    assert host_vad_levels(np.zeros((0, 80), np.float32)).size == 0
    e = host_vad_levels(np.full((2, 80), np.inf, np.float32))
    assert e.tolist() == [4096 * 80] * 2


def test_long_plan_equals_the_restatement():
    assert host_long_plan([3000, 100, 2900, 50, 3000], batch_max=2) == ([(0, 0), (1, 1), (1, 0), (2, 0), (0, 1)], 3)
    assert R.long_plan([3000, 100, 2900, 50, 3000], batch_max=2) == ([(0, 0), (1, 1), (1, 0), (2, 0), (0, 1)], 3)
    assert host_long_plan([]) == ([], 0)
    # a segment longer than the budget still gets a batch of its own; batch_max = 1: one batch each, longest first
    assert host_long_plan([500, 120000, 400], frame_budget=96000) == R.long_plan([500, 120000, 400])
    assert host_long_plan([500, 120000, 400], frame_budget=96000)[0][1] == (0, 0)
    assert host_long_plan([5, 9, 9, 1], batch_max=1) == ([(2, 0), (0, 0), (1, 0), (3, 0)], 4)
    rng = np.random.default_rng(3)
    for _ in range(200):
        lens = rng.integers(12, 3001, int(rng.integers(0, 80))).tolist()
        bm, fb = int(rng.integers(1, 40)), int(rng.choice([96000, 3000, 10000, 1]))
        got = host_long_plan(lens, bm, fb)
        assert got == R.long_plan(lens, bm, fb)
        place, nb = got
        for k in range(nb):                                        # rows of a batch: 0 .. r-1, longest first, inside the budget
            rows = sorted((r, lens[i]) for i, (b, r) in enumerate(place) if b == k)
            assert [r for r, _ in rows] == list(range(len(rows))) and len(rows) <= bm
            assert len(rows) == 1 or len(rows) * rows[0][1] <= fb
            assert all(a[1] >= b[1] for a, b in zip(rows, rows[1:]))
    assert host_long_plan([100] * 40) == R.long_plan([100] * 40)   # the defaults: 32 rows, 96000 frames
    assert host_long_plan([100] * 40)[1] == 2


def test_cli_vad_option():
    from aliparaformerasr_amd.examples import parse_args
    base = ["-type", "offline"]
    assert "vad" not in parse_args(base + ["-files", "a.wav"])
    assert parse_args(base + ["-vad", "-files", "a.wav"])["vad"] == dict(cfg={}, batch_max=0, frame_budget=0, sep="")
    got = parse_args(base + ["-vad", "max_len=300,min_speech=50,batch_max=4,sep= | ", "-files", "a.wav"])
    assert got["vad"] == dict(cfg=dict(max_len=300, min_speech=50), batch_max=4, frame_budget=0, sep=" | ") and got["files"] == ["a.wav"]
    for bad in (["-vad", "speed=3"], ["-vad", "window=x"], ["-vad", "-nbest", "2"], ["-vad", "-align", "t.txt"]):
        with pytest.raises(ValueError):
            parse_args(base + bad)
    with pytest.raises(ValueError):
        parse_args(["-type", "online", "-vad"])
