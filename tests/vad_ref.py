"""The definition of the voice-activity segmentation in numpy (include/paraformer_hip.h "Voice-activity segmentation",
DESIGN.md §4.6h).  Normative: the host forms (pf_host_vad_levels / pf_host_vad_segments / pf_host_long_plan, csrc/hostutil.cpp)
and the device form (csrc/k_vad.hip) must equal it exactly — every value past the clamp of step 1 is an integer, so there is
no tolerance anywhere.

Frames are the 10 ms fbank frames t = 0 .. T-1 of a whole stream.  A configuration is a dict with the keys of DEFAULTS."""
import numpy as np

INT32_MIN = -(1 << 31)
MAX_SEGMENTS = 65536
MAX_FRAMES = 1 << 22
DEFAULTS = dict(floor_pct=10, margin_q=96, abs_level=INT32_MIN, window=20, on_count=15, off_count=15, pad_begin=30, pad_end=5,
                min_speech=50, max_len=3000, split_search=500)


def config(**kw):
    c = dict(DEFAULTS)
    for k in kw:
        assert k in DEFAULTS, k
    c.update(kw)
    return c


def valid(c, lfr_n=6):
    """the constraints outside which every entry point answers PF_ERR_INVALID_ARG"""
    return (-1 <= c["floor_pct"] <= 100 and 1 <= c["window"] <= 256 and 1 <= c["on_count"] <= c["window"]
            and 1 <= c["off_count"] <= c["window"] and c["on_count"] + c["off_count"] > c["window"]
            and 0 <= c["pad_begin"] <= 1024 and 0 <= c["pad_end"] <= 1024 and c["min_speech"] >= 2 * lfr_n
            and 0 <= c["split_search"] <= 1024 and 2 * c["min_speech"] + c["split_search"] <= c["max_len"])


def levels(rows):
    """step 1: rows [T, n_mels] float32 -> e [T] int32"""
    x = np.asarray(rows, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(x > np.float32(-64), x, np.float32(-64))         # NaN and -inf: the comparison is false
        v = np.where(v > np.float32(64), np.float32(64), v)
    q = np.rint(v * np.float32(64)).astype(np.int64)                   # the product is exact; half to even
    return q.sum(axis=1).astype(np.int32) if x.ndim == 2 and x.shape[0] else np.zeros(0, np.int32)


def threshold(e, n_mels, c):
    """step 2 (a Python int)"""
    T = len(e)
    if c["floor_pct"] < 0:
        return int(c["abs_level"])
    k = min(T - 1, T * c["floor_pct"] // 100)
    F = int(np.sort(np.asarray(e, np.int64))[k])
    return max(F + c["margin_q"] * n_mels, int(c["abs_level"]))


def states(e, n_mels, c):
    """steps 2 and 3: state [T] bool"""
    e = np.asarray(e, np.int64)
    T = len(e)
    raw = e > threshold(e, n_mels, c)
    cs = np.concatenate([[0], np.cumsum(raw)])
    t = np.arange(T)
    w = np.minimum(c["window"], t + 1)
    cnt = cs[t + 1] - cs[t + 1 - w]
    on = cnt >= c["on_count"]
    off = ~on & (w - cnt >= c["off_count"])
    last = np.maximum.accumulate(np.where(on | off, t, -1))           # the last event at or before t wins
    return np.where(last >= 0, on[np.maximum(last, 0)], False)


def segments(e, n_mels=80, c=None):
    """steps 2-6: the list of (begin, end) frame pairs, ascending"""
    c = config() if c is None else c
    e = np.asarray(e, np.int64)
    T = len(e)
    assert T <= MAX_FRAMES
    if T == 0:
        return []
    st = states(e, n_mels, c)
    # step 4: d[t] = some state-1 frame in [t - pad_end, t + pad_begin]
    diff = np.zeros(T + 1, np.int64)
    u = np.flatnonzero(st)
    np.add.at(diff, np.maximum(u - c["pad_begin"], 0), 1)
    np.add.at(diff, np.minimum(u + c["pad_end"] + 1, T), -1)
    d = np.cumsum(diff)[:T] > 0
    edge = np.diff(np.concatenate([[0], d.astype(np.int8), [0]]))
    out = []
    for b, en in zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()):
        if en - b < c["min_speech"]:
            continue
        # step 5
        while en - b > c["max_len"]:
            hi = min(b + c["max_len"], en - c["min_speech"])
            lo = hi - c["split_search"]
            win = e[lo:hi + 1]
            cut = lo + (len(win) - 1 - int(np.argmin(win[::-1])))      # the smallest level, ties to the largest t
            out.append((b, cut))
            b = cut
        out.append((b, en))
    assert len(out) <= MAX_SEGMENTS
    return out


def sample_range(seg, n_samples):
    b, en = seg
    return 160 * b, min(n_samples, 160 * en)


def long_plan(lens, batch_max=32, frame_budget=96000):
    """the batch plan: (batch, row) per segment, and the number of batches"""
    order = sorted(range(len(lens)), key=lambda i: (-lens[i], i))
    place = [None] * len(lens)
    nb, i = 0, 0
    while i < len(order):
        L = lens[order[i]]
        rows = 0
        while True:
            place[order[i]] = (nb, rows)
            rows += 1
            i += 1
            if not (i < len(order) and rows < batch_max and (rows + 1) * L <= frame_budget):
                break
        nb += 1
    return place, nb


def telegraph(rng, T, lo=0, hi=20000, mean_run=40, jitter=0):
    """a random two-level signal with geometric run lengths (the fuzz input)"""
    e = np.empty(T, np.int32)
    t, lvl = 0, int(rng.integers(0, 2))
    while t < T:
        n = int(rng.geometric(1.0 / mean_run))
        e[t:t + n] = hi if lvl else lo
        t += n
        lvl ^= 1
    if jitter:
        e = e + rng.integers(-jitter, jitter + 1, T).astype(np.int32)
    return e


# ---- inputs shared by the CPU and the GPU tests ------------------------------------------------------------------
S, Q = 20000, 0          # speech / silence levels of the known answers


def lv(*runs):
    return np.concatenate([np.full(n, v, np.int32) for v, n in runs])


def known_answers():
    """(tag, levels, config overrides, expected segments): the table of the design, from its numpy sketch"""
    split = lv((Q, 50), (S, 400), (Q, 50))
    split[200:210] = 9000
    return [
        ("one burst", lv((Q, 100), (S, 200), (Q, 100)), {}, [(84, 319)]),
        ("speech at both ends", lv((S, 60), (Q, 100), (S, 60)), {}, [(0, 79), (144, 220)]),
        ("14-frame burst", lv((Q, 100), (S, 14), (Q, 100)), dict(min_speech=10), []),
        ("15-frame burst", lv((Q, 100), (S, 15), (Q, 100)), dict(min_speech=10), [(84, 134)]),
        ("35-frame gap", lv((Q, 100), (S, 100), (Q, 35), (S, 100), (Q, 100)), {}, [(84, 354)]),
        ("36-frame gap", lv((Q, 100), (S, 100), (Q, 36), (S, 100), (Q, 100)), {}, [(84, 219), (220, 355)]),
        ("split at the dip", split, dict(max_len=200, split_search=100, min_speech=50), [(34, 209), (209, 409), (409, 469)]),
        ("constant level", lv((S, 500)), {}, []),
    ]


def random_config(rng, lfr_n):
    window = int(rng.choice([1, 2, 20, 256, int(rng.integers(1, 65))]))
    on = int(rng.integers(1, window + 1))
    off = int(rng.integers(max(1, window - on + 1), window + 1))
    pad = lambda: int(rng.choice([0, 0, 5, 30, 1024, int(rng.integers(0, 80))]))
    min_speech = int(rng.integers(2 * lfr_n, 2 * lfr_n + 70))
    split_search = int(rng.choice([0, 0, 1, int(rng.integers(0, 120)), 1024]))
    max_len = 2 * min_speech + split_search + int(rng.choice([0, 1, int(rng.integers(0, 300))]))
    return config(floor_pct=int(rng.integers(-1, 101)), margin_q=int(rng.choice([96, 0, -20, 300])),
                    abs_level=int(rng.choice([INT32_MIN, 5000, 25000])), window=window, on_count=on, off_count=off,
                    pad_begin=pad(), pad_end=pad(), min_speech=min_speech, max_len=max_len, split_search=split_search)


def special_rows(T, n_mels=80, seed=0):
    """fbank-like rows with the special values of step 1 scattered in: NaN, +-inf, +-64, +-64.01, half-way values k / 128"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, n_mels)) * 6 - 4).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 64, -64, 64.01, -64.01, 63.9921875, -63.9921875, 1e30, -1e30, 0.0, -0.0], np.float32)
    halves = (np.arange(-8191, 8192, 2, dtype=np.float32) / np.float32(128.0)).astype(np.float32)      # exactly between two levels
    mask = rng.random((T, n_mels)) < 0.2
    x[mask] = rng.choice(np.concatenate([special, halves]), int(mask.sum()))
    if T:
        x[0, : min(n_mels, special.size)] = special[: min(n_mels, special.size)]
    return x


def burst_audio(seconds, bursts, seed):
    rng = np.random.default_rng(seed)
    x = (0.001 * rng.standard_normal(16000 * seconds)).astype(np.float32)
    for f0, f1 in bursts:
        x[160 * f0: 160 * f1] = np.clip(0.3 * rng.standard_normal(160 * (f1 - f0)), -0.999, 0.999).astype(np.float32)
    return x
