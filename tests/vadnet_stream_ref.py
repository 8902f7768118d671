"""The release schedule of the streaming FSMN-VAD model score in Python (include/paraformer_hip.h "Voice-activity endpointing,
streaming, model score").  It builds on tests/vadnet_ref.py, which defines the values: the streaming levels
and logits ARE vadnet_ref's over the complete stream; this file only says which of them leave at which call.

    left = (lfr_m - 1) // 2, right = lfr_m - 1 - left
    a stream that has received n frames has released max(0, n - right) levels; all n once flushed
    level t leaves in the call that brings frame t + right, or in the call that flushes

A Stream restates that schedule call by call.  It keeps every row it received and recomputes the definition over them: before
the flush a level t < n - right never looks at a frame beyond n - 1 (its LFR window ends at t + right and the FSMN taps look
back only), so the levels it hands out are final; at the flush the upper clamp binds at the last frame received."""
import numpy as np

import vadnet_ref as R

MAX_STREAM_FRAMES = 1 << 30          # PF_ENDPOINT_MAX_STREAM_FRAMES
CHUNKS = [0, 1, 2, 3, 59, 60, 63, 64, 65, 131]


def right(cfg):
    return cfg["lfr_m"] - 1 - (cfg["lfr_m"] - 1) // 2


def released(cfg, n, flushed):
    """how many levels a stream of n received frames has released"""
    return n if flushed else max(0, n - right(cfg))


def counts(cfg, chunks, flush_at=None):
    """the released count of every call: chunks[k] new frames in call k, the flush in call flush_at (None: never)"""
    out, n, rel = [], 0, 0
    for k, c in enumerate(chunks):
        n += c
        now = released(cfg, n, flush_at is not None and k >= flush_at)
        out.append(now - rel)
        rel = now
    return out


def chunkings(T, seed, sizes=CHUNKS):
    """a list of chunk sizes drawn from `sizes` that add up to T (the last one cut to fit); zeros included"""
    rng = np.random.default_rng(seed)
    out, left = [], T
    while left > 0:
        c = int(rng.choice(sizes))
        out.append(min(c, left))
        left -= out[-1]
    return out or [0]


class Stream:
    """One stream under the schedule: feed(rows, flush) -> (levels, logits) of the levels that leave in this call, float64
    logits, from the definition over everything received so far."""

    def __init__(self, cfg, w):
        self.cfg, self.w = cfg, w
        self.rows = np.zeros((0, cfg["n_mels"]), np.float32)
        self.flushed = False
        self.rel = 0

    def feed(self, rows, flush=False):
        rows = np.asarray(rows, np.float32).reshape(-1, self.cfg["n_mels"])
        if self.flushed and rows.shape[0]:
            raise ValueError("frames after a flush")
        if self.rows.shape[0] + rows.shape[0] > MAX_STREAM_FRAMES:
            raise OverflowError("more than MAX_STREAM_FRAMES frames in one stream")
        self.rows = np.concatenate([self.rows, rows])
        self.flushed = self.flushed or bool(flush)
        now = released(self.cfg, self.rows.shape[0], self.flushed)
        z = R.logits(self.cfg, self.w, self.rows)[self.rel: now]
        self.rel, first = now, self.rel
        return R.levels_from_logits(self.cfg, z), z, first


def poisoned_levels(cfg, T, bad_frames):
    """the levels of a stream of T frames that a non-finite value in the fbank rows `bad_frames` reaches under the definition:
    the LFR window carries frame f to the levels f - right .. f + left (clamped), every layer `reach` levels further on"""
    left = (cfg["lfr_m"] - 1) // 2
    reach = (cfg["lorder"] - 1) * cfg["lstride"] * cfg["n_layers"]
    bad = np.zeros(T, bool)
    for f in bad_frames:
        bad[max(0, f - right(cfg)): min(T, f + left + reach + 1)] = True
    return bad
