"""The definition of the streaming endpoint detector in numpy (include/paraformer_hip.h "Voice-activity endpointing,
streaming").  Normative: the host form (pf_host_endpoint_update, csrc/hostutil.cpp) and the device form
(csrc/k_endpoint.hip) must equal it exactly, the state block included — every value past the clamp of step 1 is an integer, so
there is no tolerance anywhere.

It is the detector of tests/vad_ref.py made causal: the percentile floor becomes a tracked floor (step 2'), the padding step
becomes events (steps 4' - 6).  Frames v = 0, 1, ... are the 10 ms fbank rows of the caller's audio; the levels are step 1 of
vad_ref (vad_ref.levels).  A configuration is a dict with the keys of DEFAULTS.

The walk here is deliberately the plainest one: one frame at a time, Python integers, the state block decoded into a dict and
encoded again.  update() may be called with any chunking; the block after it is the detector's whole memory."""
import numpy as np

INT32_MIN = -(1 << 31)
MAX_FRAMES = 1 << 22                 # PF_VAD_MAX_FRAMES: the largest max_len
MAX_STREAM_FRAMES = 1 << 30          # PF_ENDPOINT_MAX_STREAM_FRAMES: frames one state block may count
STATE_INTS = 16
SILENCE, FORCED, FLUSH = 1, 2, 3     # PF_ENDPOINT_SILENCE / _FORCED / _FLUSH
DEFAULTS = dict(rise=2, margin_q=96, abs_level=INT32_MIN, window=20, on_count=15, off_count=15, pad_begin=30, pad_end=5,
                end_silence=80, min_speech=50, max_len=3000)

# the state block, int32 words (all zero = a fresh stream)
H0 = 0            # 0 .. 7   the raw bits of the previous 256 frames: bit 255 - k of the 256-bit little-endian number is frame count-1-k
STATE = 8         # state of the last frame
LAST_ONE = 9      # the last state-1 frame + 1 (0: none)
RUN_FIRST = 10    # the first state-1 frame of the open sentence + 1 (0: no sentence is open)
PREV_END = 11     # the end of the last emitted sentence
COUNT = 12        # frames seen
FLOOR_LO, FLOOR_HI = 13, 14   # F[count - 1] as an int64 (meaningful once count > 0 and rise >= 0)
FLUSHED = 15


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        assert k in DEFAULTS, k
    c.update(kw)
    return c


def valid(c, lfr_n=6):
    """the constraints outside which every entry point answers PF_ERR_INVALID_ARG"""
    return (-1 <= c["rise"] <= 1 << 20 and 1 <= c["window"] <= 256 and 1 <= c["on_count"] <= c["window"]
            and 1 <= c["off_count"] <= c["window"] and c["on_count"] + c["off_count"] > c["window"]
            and 0 <= c["pad_begin"] <= 1024 and 0 <= c["pad_end"] <= c["end_silence"] <= 1 << 16 and c["end_silence"] >= 1
            and c["min_speech"] >= 2 * lfr_n and c["min_speech"] <= c["max_len"] <= MAX_FRAMES and c["pad_begin"] < c["max_len"])


def new_state():
    return np.zeros(STATE_INTS, np.int32)


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def update(state, levels, flush=False, n_mels=80, c=None):
    """Feeds `levels` (int32, any count) and then, with flush, ends the input.  `state` [STATE_INTS] int32 is updated in place.
    Returns (events, in_speech, open_begin): events = [(b, e, kind)] in order, open_begin = -1 when no sentence is open."""
    c = config() if c is None else c
    s = state
    assert s.dtype == np.int32 and s.shape == (STATE_INTS,)
    lev = [int(x) for x in np.asarray(levels, np.int64).reshape(-1)]
    assert not (s[FLUSHED] and lev), "frames after a flush"
    hist = 0
    for j in range(8):
        hist |= (int(s[H0 + j]) & 0xFFFFFFFF) << (32 * j)
    st, last_one, run_first, prev_end, count = int(s[STATE]), int(s[LAST_ONE]) - 1, int(s[RUN_FIRST]) - 1, int(s[PREV_END]), int(s[COUNT])
    F = _i32(int(s[FLOOR_LO])) & 0xFFFFFFFF | (int(s[FLOOR_HI]) << 32)
    assert count + len(lev) <= MAX_STREAM_FRAMES
    events = []
    begin = lambda: max(prev_end, run_first - c["pad_begin"])

    for e in lev:
        t = count
        # 2' the tracked floor
        if c["rise"] >= 0:
            F = e if t == 0 else min(e, F + c["rise"])
            thr = max(F + c["margin_q"] * n_mels, c["abs_level"])
        else:
            thr = c["abs_level"]
        raw = 1 if e > thr else 0
        hist = (hist >> 1) | (raw << 255)
        # 3 hysteresis (vad_ref.states, one frame)
        w = min(c["window"], t + 1)
        cnt = bin(hist >> (256 - w)).count("1")
        if cnt >= c["on_count"]:
            st = 1
        elif w - cnt >= c["off_count"]:
            st = 0
        # 4' events
        if st:
            if run_first < 0:
                run_first = t
            last_one = t
        elif run_first >= 0 and t == last_one + c["end_silence"]:
            b, en = begin(), last_one + 1 + c["pad_end"]
            if en - b >= c["min_speech"]:
                events.append((b, en, SILENCE))
                prev_end = en
            run_first = -1
        # 5' the forced cut
        if run_first >= 0 and t + 1 - begin() == c["max_len"]:
            events.append((begin(), t + 1, FORCED))
            prev_end = t + 1
            if not st:
                run_first = -1
        count += 1

    if flush and not s[FLUSHED]:
        # 6 flush
        if run_first >= 0:
            b, en = begin(), min(count, last_one + 1 + c["pad_end"])
            if en - b >= c["min_speech"]:
                events.append((b, en, FLUSH))
                prev_end = en
            run_first = -1
        s[FLUSHED] = 1

    for j in range(8):
        s[H0 + j] = _i32(hist >> (32 * j))
    s[STATE], s[LAST_ONE], s[RUN_FIRST], s[PREV_END], s[COUNT] = st, last_one + 1, run_first + 1, prev_end, count
    if c["rise"] >= 0 and count > 0:
        s[FLOOR_LO], s[FLOOR_HI] = _i32(F), _i32(F >> 32)
    return events, int(run_first >= 0), (begin() if run_first >= 0 else -1)


def run(levels, n_mels=80, c=None, flush=True):
    """one-shot: a fresh state, all levels, the flush -> (events, state)"""
    s = new_state()
    ev, _, _ = update(s, levels, flush, n_mels, c)
    return ev, s


def floor(levels, rise):
    """F[v] of step 2' for a whole signal (Python ints)"""
    out, F = [], None
    for e in [int(x) for x in np.asarray(levels, np.int64)]:
        F = e if F is None else min(e, F + rise)
        out.append(F)
    return out


def random_config(rng, lfr_n=6):
    window = int(rng.choice([1, 2, 20, 256, int(rng.integers(1, 65))]))
    on = int(rng.integers(1, window + 1))
    off = int(rng.integers(max(1, window - on + 1), window + 1))
    pad_begin = int(rng.choice([0, 0, 5, 30, 1024, int(rng.integers(0, 80))]))
    end_silence = int(rng.choice([1, 2, 36, 80, int(rng.integers(1, 120))]))
    pad_end = int(rng.choice([0, end_silence, int(rng.integers(0, end_silence + 1))]))
    min_speech = int(rng.integers(2 * lfr_n, 2 * lfr_n + 70))
    max_len = max(min_speech, pad_begin + 1) + int(rng.choice([0, 1, 63, int(rng.integers(0, 400)), 3000]))
    return config(rise=int(rng.choice([-1, 0, 1, 2, 50, 1 << 20])), margin_q=int(rng.choice([96, 0, -20, 300])),
                  abs_level=int(rng.choice([INT32_MIN, 5000, 25000])), window=window, on_count=on, off_count=off,
                  pad_begin=pad_begin, pad_end=pad_end, end_silence=end_silence, min_speech=min_speech, max_len=max_len)
