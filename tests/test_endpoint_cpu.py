"""CPU: the streaming endpoint detector — the definition (tests/endpoint_ref.py) on known answers derived by hand below, the
host form (pf_host_endpoint_update, csrc/hostutil.cpp) against the definition exactly (every value is an integer: no tolerance
exists; the state block is compared word for word), chunk invariance over random signals and configurations, the tie to the
offline detector (tests/vad_ref.py), the tracked floor at the int32 extremes, and every contract of the entry point."""
import ctypes as C

import numpy as np
import pytest

import endpoint_ref as R
import vad_ref as V
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import endpoint_config, endpoint_state, host_endpoint_update

NEW = ("pf_endpoint_default", "pf_host_endpoint_update", "pf_op_endpoint_update")
SIL, FORCED, FLUSH = R.SILENCE, R.FORCED, R.FLUSH
S, Q, lv = V.S, V.Q, V.lv


def _host(state, e, flush, c, n_mels=80, lfr_n=6):
    ev, ins, ob = host_endpoint_update(state, e, flush, n_mels, c, lfr_n)
    return [tuple(r) for r in ev.tolist()], ins, ob


def _host_run(e, c, n_mels=80, lfr_n=6, flush=True):
    s = endpoint_state()
    ev, _, _ = _host(s, e, flush, c, n_mels, lfr_n)
    return ev, s


def test_symbols_are_exported():
    lib = N.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES, name


def test_default_configuration_is_the_stated_one():
    c = endpoint_config()
    assert c.struct_size == C.sizeof(N.PfEndpointConfig) == 64
    assert {k: getattr(c, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert R.valid(R.DEFAULTS)
    # the stated relation of the default rise: a sentence that starts at the floor keeps its speech until the forced cut
    assert R.DEFAULTS["rise"] * R.DEFAULTS["max_len"] < R.DEFAULTS["margin_q"] * 80
    assert N.load().pf_endpoint_default(None) == N.PF_ERR_INVALID_ARG
    assert N.PF_ENDPOINT_STATE_INTS == R.STATE_INTS and (N.PF_ENDPOINT_SILENCE, N.PF_ENDPOINT_FORCED, N.PF_ENDPOINT_FLUSH) == (SIL, FORCED, FLUSH)


# Derived by hand with window 20, on 15, off 15: a burst of raw frames [r0, r1) of at least 15 frames gives the state run
# [r0 + 14, r1 + 14) (the 15th raw frame switches on, the 15th silent one off).  Levels S = 20000 and Q = 0; with the default
# floor a burst that follows silence has F <= 2 * its length, so thr <= 7680 + 2 * 400 < S, and F falls back to 0 at once.
ABS = dict(rise=-1, abs_level=7680)
KNOWN = [
    # s0 = 114: b = 84; s1 = 314: e = 319, closed at t = 313 + 80 = 393 < 400
    ("one burst", lv((Q, 100), (S, 200), (Q, 100)), {}, False, [(84, 319, SIL)], (0, -1)),
    # runs [14, 74) and [174, ..): (0, 79) closed at 153; b = max(79, 144); the state is 1 at T = 220
    ("speech at both ends", lv((S, 60), (Q, 100), (S, 60)), ABS, True, [(0, 79, SIL), (144, 220, FLUSH)], (0, -1)),
    # the tracked floor starts at F[0] = e[0]: speech at frame 0 IS the floor until the level drops
    ("speech at both ends, tracked floor", lv((S, 60), (Q, 100), (S, 60)), {}, True, [(144, 220, FLUSH)], (0, -1)),
    ("speech at both ends, not finished", lv((S, 60), (Q, 100), (S, 60)), ABS, False, [(0, 79, SIL)], (1, 144)),
    # runs [114, 214) and [214 + gap, ..): a state-1 frame AT t = 213 + 80 keeps the sentence open
    ("gap of end_silence - 1", lv((Q, 100), (S, 100), (Q, 79), (S, 100), (Q, 100)), {}, False, [(84, 398, SIL)], (0, -1)),
    ("gap of end_silence", lv((Q, 100), (S, 100), (Q, 80), (S, 100), (Q, 100)), {}, False, [(84, 219, SIL), (264, 399, SIL)], (0, -1)),
    # run [114, 129): (84, 134) is 50 long and dropped at t = 148; prev_end stays 0, so the next one begins at 154 - 30, not at 134
    ("dropped by min_speech", lv((Q, 100), (S, 15), (Q, 25), (S, 100), (Q, 100)), dict(min_speech=51, end_silence=20), False,
     [(124, 259, SIL)], (0, -1)),
    ("kept at min_speech", lv((Q, 100), (S, 15), (Q, 25), (S, 100), (Q, 100)), dict(min_speech=50, end_silence=20), False,
     [(84, 134, SIL), (134, 259, SIL)], (0, -1)),
    # run [114, 514): cuts at t = 283 and t = 483 (t + 1 - b = 200); the rest (484, 519) is 35 long and dropped
    ("forced cut, short remainder", lv((Q, 100), (S, 400), (Q, 100)), dict(max_len=200), False, [(84, 284, FORCED), (284, 484, FORCED)], (0, -1)),
    # run [114, 364): one cut; the rest (284, 369) closes at t = 363 + 80 = 443
    ("forced cut, remainder kept", lv((Q, 100), (S, 250), (Q, 100)), dict(max_len=200), False, [(84, 284, FORCED), (284, 369, SIL)], (0, -1)),
    # run [114, 464): the rest would close at t = 543, but t + 1 - 284 = 200 comes first, at t = 483 inside the trailing silence:
    # the cut takes the frames seen so far and, the state being 0, closes the sentence
    ("forced cut inside the trailing silence", lv((Q, 100), (S, 350), (Q, 100)), dict(max_len=200), False,
     [(84, 284, FORCED), (284, 484, FORCED)], (0, -1)),
    ("flush inside speech", lv((Q, 100), (S, 200)), {}, True, [(84, 300, FLUSH)], (0, -1)),
    ("flush inside trailing silence", lv((Q, 100), (S, 200), (Q, 40)), {}, True, [(84, 319, FLUSH)], (0, -1)),
    ("flush inside the end padding", lv((Q, 100), (S, 200), (Q, 16)), {}, True, [(84, 316, FLUSH)], (0, -1)),
    ("no flush inside trailing silence", lv((Q, 100), (S, 200), (Q, 40)), {}, False, [], (1, 84)),
]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c[0])
def test_known_answers_definition_and_host_form(case):
    _tag, e, over, flush, want, status = case
    c = R.config(**over)
    assert R.valid(c)
    s_ref = R.new_state()
    ev, ins, ob = R.update(s_ref, e, flush, 80, c)
    assert (ev, (ins, ob)) == (want, status)
    s = endpoint_state()
    assert _host(s, e, flush, over) == (want, *status)
    np.testing.assert_array_equal(s, s_ref)


def _chunks(rng, T):
    kind = rng.choice(["1", "59", "60", "64", "65", "257", "random"])
    out, t = [], 0
    while t < T:
        n = int(rng.integers(0, 400)) if kind == "random" else int(kind)
        if kind == "1" and t > 300:                 # (frame by frame for the first 300 frames, then larger steps)
            n = int(rng.integers(1, 130))
        out.append((t, min(T, t + n)))
        t = min(T, t + n)
    return out


def test_chunk_invariance_and_host_form_equals_the_definition():
    """300 random telegraph signals under random valid configurations: the host form in a random chunking == the host form in one
    call == the definition in one call — events, status after every call's last frame, and the final state block."""
    rng = np.random.default_rng(20241021)
    kinds = {SIL: 0, FORCED: 0, FLUSH: 0}
    for it in range(300):
        lfr_n = int(rng.choice([1, 6]))
        c = R.random_config(rng, lfr_n)
        assert R.valid(c, lfr_n), c
        T = int(rng.integers(1, 2001))
        e = V.telegraph(rng, T, mean_run=int(rng.choice([3, 15, 60, 400])), jitter=int(rng.choice([0, 3, 4000])))
        n_mels = int(rng.choice([80, 1, 128]))
        flush = bool(rng.integers(0, 2))
        s_ref = R.new_state()
        want, ins_w, ob_w = R.update(s_ref, e, flush, n_mels, c)
        one, s_one = _host_run(e, c, n_mels, lfr_n, flush)
        assert one == want, (it, c, T)
        np.testing.assert_array_equal(s_one, s_ref, err_msg=str((it, c)))
        s, got = endpoint_state(), []
        pieces = _chunks(rng, T)
        for i, (a, b) in enumerate(pieces):
            ev, ins, ob = _host(s, e[a:b], flush and i == len(pieces) - 1, c, n_mels, lfr_n)
            got += ev
        assert got == want and (ins, ob) == (ins_w, ob_w), (it, c, T, pieces[:4])
        np.testing.assert_array_equal(s, s_ref, err_msg=str((it, c)))
        prev = 0
        for b, en, k in want:
            assert prev <= b < en <= T and c["min_speech"] <= en - b <= c["max_len"], (it, c, want)
            prev = en
            kinds[k] += 1
    assert kinds[SIL] > 100 and kinds[FORCED] > 100 and kinds[FLUSH] > 15, kinds     # the fuzz reaches every kind of event


def _tie(e, over, abs_level):
    pb, pe = over.get("pad_begin", 30), over.get("pad_end", 5)
    keys = {k: over[k] for k in ("window", "on_count", "off_count", "pad_begin", "pad_end", "min_speech") if k in over}
    vc = V.config(floor_pct=-1, abs_level=abs_level, max_len=2 * V.MAX_FRAMES, split_search=0, **keys)
    ec = R.config(rise=-1, abs_level=abs_level, end_silence=pb + pe + 1, max_len=V.MAX_FRAMES, **keys)
    assert R.valid(ec, 1)
    want = V.segments(e, 80, vc)
    ev, _ = _host_run(e, ec, 80, 1, True)
    assert [(b, en) for b, en, _ in ev] == want, (over, want, ev)
    assert [(b, en) for b, en, _ in R.run(e, 80, ec)[0]] == want
    return want


def test_tie_to_the_offline_detector():
    """rise = -1, end_silence = pad_begin + pad_end + 1, no forced cut, flushed at T: the (b, e) list is the offline detector's
    with floor_pct = -1 (both merge two runs iff the gap is at most pad_begin + pad_end)."""
    n = 0
    for tag, e, over, _want in V.known_answers():
        if tag in ("split at the dip", "constant level"):
            continue
        _tie(e, over, 96 * 80)
        n += 1
    assert n == 6
    rng = np.random.default_rng(7)
    total = 0
    for it in range(200):
        vc = V.random_config(rng, 1)
        over = {k: vc[k] for k in ("window", "on_count", "off_count", "pad_begin", "pad_end", "min_speech")}
        e = V.telegraph(rng, int(rng.integers(1, 2001)), mean_run=int(rng.choice([3, 15, 60, 400])), jitter=int(rng.choice([0, 3, 4000])))
        total += len(_tie(e, over, int(rng.choice([5000, 10000, 25000]))))
    assert total > 150, total                                       # the signals do have segments


def test_floor():
    # rise 0: a pure running minimum; the int32 extremes (the arithmetic is int64)
    rng = np.random.default_rng(11)
    e = rng.integers(-(1 << 31), 1 << 31, 700).astype(np.int64)
    assert R.floor(e, 0) == np.minimum.accumulate(e).tolist()
    for rise in (0, 1, 1 << 20):
        for margin_q in (0, 96, -300, (1 << 31) - 1, -(1 << 31)):
            c = R.config(rise=rise, margin_q=margin_q, window=1, on_count=1, off_count=1, pad_begin=0, pad_end=0, end_silence=1,
                         min_speech=2, max_len=64)
            x = e.astype(np.int32)
            x[:3] = [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1]
            want, s_ref = R.run(x, 128, c)
            got, s = _host_run(x, c, 128, 1)
            assert got == want, (rise, margin_q)
            np.testing.assert_array_equal(s, s_ref)
            F = R.floor(x, rise)[-1]
            assert (int(s[R.FLOOR_LO]) & 0xFFFFFFFF) | (int(s[R.FLOOR_HI]) << 32) == F
    # a step up of the noise level is followed at `rise` per frame: with margin m the frames of the step are raw until
    # F + m reaches the new level, ceil((step - m) / rise) - 1 frames in all — window 1 turns raw into the state itself
    for rise, step, m in ((2, 1000, 200), (7, 1000, 300), (7, 1000, 301), (1, 50, 0)):
        c = R.config(rise=rise, margin_q=m, window=1, on_count=1, off_count=1, pad_begin=0, pad_end=0, end_silence=1, min_speech=2,
                     max_len=4000)
        x = lv((100, 50), (100 + step, 1200))
        k = -(-(step - m) // rise) - 1                               # the j = v - 49 >= 1 with rise * j < step - m (e > thr is strict)
        assert R.floor(x, rise)[50 + 10] == 100 + rise * 11
        want = [(50, 50 + k, SIL)]
        assert R.run(x, 1, c, flush=False)[0] == want
        assert _host_run(x, c, 1, 1, False)[0] == want


def test_every_constraint_is_invalid_arg():
    lib = N.load()
    e = lv((Q, 100), (S, 200), (Q, 100))
    i32 = C.POINTER(C.c_int32)
    ev, n = np.zeros((64, 3), np.int32), C.c_int32()

    def call(cfg, state=None, levels=e, n_new=None, flush=0, cap=64, lfr_n=6):
        st = endpoint_state() if state is None else state
        return lib.pf_host_endpoint_update(st.ctypes.data_as(i32), levels.ctypes.data_as(i32), levels.size if n_new is None else n_new, flush,
                                           80, lfr_n, None if cfg is None else C.byref(cfg), ev.ctypes.data_as(i32), cap, n, None, None)

    bad = [dict(rise=-2), dict(rise=(1 << 20) + 1), dict(window=0), dict(window=257, on_count=200, off_count=200), dict(on_count=0),
           dict(on_count=21), dict(off_count=0), dict(off_count=21), dict(on_count=10, off_count=10), dict(pad_begin=-1),
           dict(pad_begin=1025), dict(pad_end=-1), dict(pad_end=81), dict(end_silence=0, pad_end=0), dict(end_silence=(1 << 16) + 1),
           dict(min_speech=11), dict(min_speech=3001), dict(max_len=49), dict(max_len=(1 << 22) + 1),
           dict(pad_begin=60, max_len=60, min_speech=50)]
    for over in bad:
        assert not R.valid(R.config(**over)), over
        s = endpoint_state()
        assert call(endpoint_config(**over), s) == N.PF_ERR_INVALID_ARG, over
        assert not s.any()                                           # nothing was touched
    for over in (dict(rise=-1), dict(rise=1 << 20), dict(window=256, on_count=256, off_count=1), dict(pad_begin=1024), dict(pad_end=80),
                 dict(pad_end=0, end_silence=1), dict(end_silence=1 << 16), dict(min_speech=12), dict(min_speech=3000), dict(max_len=50),
                 dict(max_len=1 << 22), dict(pad_begin=59, max_len=60, min_speech=50)):
        assert R.valid(R.config(**over)), over
        assert _host_run(e, over)[0] == R.run(e, 80, R.config(**over))[0], over
    # min_speech is measured against the front-end's lfr_n
    assert call(endpoint_config(min_speech=2)) == N.PF_ERR_INVALID_ARG and call(endpoint_config(min_speech=2), lfr_n=1) == N.PF_OK
    c = endpoint_config()
    c.struct_size = 60
    assert call(c) == N.PF_ERR_INVALID_ARG
    assert call(None, n_new=-1) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_endpoint_update(None, e.ctypes.data_as(i32), e.size, 0, 80, 6, None, ev.ctypes.data_as(i32), 64, n, None, None) == N.PF_ERR_INVALID_ARG


def test_capacity_flush_and_empty_calls():
    lib = N.load()
    i32 = C.POINTER(C.c_int32)
    e = lv((Q, 100), (S, 100), (Q, 80), (S, 100), (Q, 100))         # two sentences
    want, s_ref = R.run(e, 80, None, flush=False)
    assert len(want) == 2
    # capacity: the count is filled in, the first cap events are written, the state has advanced
    for cap in (0, 1):
        s, n = endpoint_state(), C.c_int32()
        ev = np.full((2, 3), -7, np.int32)
        rc = lib.pf_host_endpoint_update(s.ctypes.data_as(i32), e.ctypes.data_as(i32), e.size, 0, 80, 6, None,
                                         ev.ctypes.data_as(i32) if cap else None, cap, n, None, None)
        assert rc == N.PF_ERR_CAPACITY and n.value == 2
        assert [tuple(r) for r in ev[:cap].tolist()] == want[:cap] and (ev[cap:] == -7).all()
        np.testing.assert_array_equal(s, s_ref)
    with pytest.raises(N.PfError) as ei:
        host_endpoint_update(endpoint_state(), e, cap=1)
    assert ei.value.code == N.PF_ERR_CAPACITY and ei.value.n == 2
    # n_new = 0 is a no-op that reports the status
    s = endpoint_state()
    assert _host(s, e[:0], False, None) == ([], 0, -1) and not s.any()
    _host(s, e[:150], False, None)
    before = s.copy()
    assert _host(s, e[:0], False, None) == ([], 1, 84)
    np.testing.assert_array_equal(s, before)
    # the flush: once; a second bare flush is a no-op; frames, or frames with a flush, are refused and change nothing
    assert _host(s, e[:0], True, None) == ([(84, 150, FLUSH)], 0, -1)
    flushed = s.copy()
    assert flushed[R.FLUSHED] == 1
    assert _host(s, e[:0], True, None) == ([], 0, -1)
    for flush in (False, True):
        with pytest.raises(N.PfError) as ei:
            host_endpoint_update(s, e[:5], flush)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    np.testing.assert_array_equal(s, flushed)
    # a block the detector cannot have left is refused, untouched
    for word, value in ((R.STATE, 2), (R.LAST_ONE, 7), (R.RUN_FIRST, -1), (R.PREV_END, 1), (R.COUNT, -1), (R.FLOOR_HI, 1), (R.FLUSHED, 5)):
        s = endpoint_state()
        s[word] = value
        bad = s.copy()
        with pytest.raises(N.PfError) as ei:
            host_endpoint_update(s, e[:5])
        assert ei.value.code == N.PF_ERR_INVALID_ARG, word
        np.testing.assert_array_equal(s, bad)
    # a state block that has counted PF_ENDPOINT_MAX_STREAM_FRAMES takes no more
    s = endpoint_state()
    s[R.COUNT] = N.PF_ENDPOINT_MAX_STREAM_FRAMES - 4
    with pytest.raises(N.PfError) as ei:
        host_endpoint_update(s, e[:5])
    assert ei.value.code == N.PF_ERR_CAPACITY
    assert _host(s, e[:4], False, None)[0] == []


def test_cli_endpoint_option():
    from aliparaformerasr_amd.examples import parse_args
    base = ["-type", "online"]
    assert "endpoint" not in parse_args(base + ["-files", "a.wav"])
    assert parse_args(base + ["-endpoint", "-files", "a.wav"])["endpoint"] == {}
    got = parse_args(base + ["-endpoint", "end_silence=40,max_len=1500", "-secondpass", "offline-model", "-files", "a.wav"])
    assert got["endpoint"] == dict(end_silence=40, max_len=1500) and got["secondpass"] == "offline-model" and got["files"] == ["a.wav"]
    for bad in (["-endpoint", "speed=3"], ["-endpoint", "window=x"], ["-secondpass", "m"], ["-endpoint", "-secondpass"]):
        with pytest.raises(ValueError):
            parse_args(base + bad)
    with pytest.raises(ValueError):
        parse_args(["-type", "offline", "-endpoint"])
