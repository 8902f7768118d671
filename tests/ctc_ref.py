"""numpy statement of the CTC collapse the device kernel implements (csrc/k_ctc.hip; DESIGN.md "CTC decoding"), shared by
tests/test_ctc_cpu.py (which pins it with hand-derived cases) and tests/test_gpu_ctc.py.

Rule: over frames t in [0, lens[b]) a token starts where ids[t] != blank and (t == 0 or ids[t] != ids[t-1]) and extends
while ids stays equal; per token: id, first frame, last frame, score = fmax over the run of scores[t] (the peak-frame
log-prob: independent of the order of evaluation, so results can be compared bit for bit)."""
import numpy as np


def collapse_one(ids, scores, n, blank=0):
    """[(id, first, last, score)] of one utterance; only frames [0, n) are looked at."""
    out = []
    t = 0
    while t < n:
        y = int(ids[t])
        u = t
        while u + 1 < n and int(ids[u + 1]) == y:
            u += 1
        if y != blank:
            out.append((y, t, u, np.fmax.reduce(np.asarray(scores[t:u + 1], np.float32))))
        t = u + 1
    return out


def collapse_ref(ids, scores, lens, blank=0, cap=None):
    """ids / scores [B, T], lens [B] (clamped to [0, T]) -> (n [B] int32, ids [B, cap] int64, first, last [B, cap] int32,
    score [B, cap] float32) in the layout of pf_fetch_ctc / pf_op_ctc_collapse: slots past n[b] hold -1 / -1 / -1 / 0.
    cap defaults to max(n)."""
    ids = np.asarray(ids)
    scores = np.asarray(scores, np.float32)
    B, T = ids.shape
    toks = [collapse_one(ids[b], scores[b], min(max(int(lens[b]), 0), T), blank) for b in range(B)]
    n = np.asarray([len(t) for t in toks], np.int32)
    cap = int(n.max()) if cap is None and B else (cap or 0)
    o_ids = np.full((B, cap), -1, np.int64)
    first, last = np.full((B, cap), -1, np.int32), np.full((B, cap), -1, np.int32)
    score = np.zeros((B, cap), np.float32)
    for b, tk in enumerate(toks):
        for k, (y, f, l, s) in enumerate(tk):
            o_ids[b, k], first[b, k], last[b, k], score[b, k] = y, f, l, s
    return n, o_ids, first, last, score


def timestamps_ms(first, last, lfr_n=6, prompt_rows=4):
    """[begin, end] in milliseconds of tokens with the given first / last frames (a frame = lfr_n x 10 ms; the prompt rows
    carry no audio): begin = ms * max(first - P, 0), end = ms * max(last + 1 - P, 0)."""
    ms = lfr_n * 10
    return [[ms * max(int(f) - prompt_rows, 0), ms * max(int(l) + 1 - prompt_rows, 0)] for f, l in zip(first, last)]
