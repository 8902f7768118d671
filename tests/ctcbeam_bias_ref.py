"""Hot-word boosting (shallow fusion) inside the CTC prefix beam search: the definition the host twin (pf_host_ctc_beam_hot),
the automaton (pf_host_hotword_graph) and the biased form of the device kernel (k_ctcbeam.hip) are compared with.  Float64
Python on top of tests/ctcbeam_ref.py.

Inputs: everything ctcbeam_ref.beam_search takes, a hot-word set (sequences of ids in [1, V); blank is 0) and a boost s >= 0
(float32, widened to float64).

Matched tokens of a label sequence y (plain text, no automaton): walk y left to right keeping the SEGMENT read since the last
completion (empty at the start, m = 0).  After each token, if one or more hot words are a suffix of the segment, the longest
completes: m += its length and the segment is emptied.  At the end d(y) is the length of the longest suffix of the segment
that is a PROPER prefix of some hot word (0 when there is none).  Matches do not overlap; of `ab` and `abc` only `ab` can ever
complete, so hot-word sets should be prefix-free.

    bias(y)  = double(s) * (m(y) + d(y))          bonus(y) = double(s) * m(y)

each ONE float64 product of the widened boost by an integer.

The search is ctcbeam_ref.beam_search with two changes:
  select   a candidate's key is total + bias(its prefix); a candidate whose total is -inf is still discarded; the W best by
           key stay, ties to the smaller candidate index; the stored pb / pnb remain unbiased.
  finish   after the last frame every entry gets score = lse(pb, pnb) + bonus(prefix) (the pending part is revoked), the
           entries are re-ordered by descending score, ties to the smaller beam rank, and the first N are the hypotheses:
           ids, score, matched = m(prefix), loglik_sum = lse(pb, pnb).
s = 0 or an empty set gives ctcbeam_ref.beam_search's lists and scores bit for bit."""
import math

import numpy as np

import ctcbeam_ref as R

NEG = R.NEG


def clean_set(hot):
    """The set as tuples of ints, empty entries dropped."""
    return [tuple(int(c) for c in w) for w in hot if len(w) > 0]


def walk(y, hot):
    """(m(y), d(y)) by the plain-text rule."""
    hot = clean_set(hot)
    seg = []
    m = 0
    for c in y:
        seg.append(int(c))
        best = 0
        for w in hot:
            if len(w) <= len(seg) and len(w) > best and tuple(seg[len(seg) - len(w):]) == w:
                best = len(w)
        if best:
            m += best
            seg = []
    d = 0
    for w in hot:
        for L in range(min(len(w) - 1, len(seg)), d, -1):
            if tuple(seg[len(seg) - L:]) == w[:L]:
                d = L
                break
    return m, d


def walk_positions(y, hot):
    """[(m, d)] after every token of y."""
    return [walk(y[:p + 1], hot) for p in range(len(y))]


def tol(T, s):
    """The comparison bound of a biased score: ctcbeam_ref.tol's 16 roundings per frame plus the product and the two
    additions the bias adds."""
    return (16.0 * max(T, 1) + 4.0) * 2.0 ** -53 * max(1.0, abs(s))


class BiasResult:
    def __init__(self, hyps, gap, gap_pos, beam):
        self.hyps = hyps          # [(ids tuple, score, matched, loglik_sum)], at most N, in the output order
        self.gap = gap            # the smallest decision gap over biased keys (select) and final scores (inf: no decision)
        self.gap_pos = gap_pos    # the same over the gaps that are not exactly 0
        self.beam = beam          # all final entries in the output order

    @property
    def n_hyp(self):
        return len(self.hyps)


def beam_search(lb, ids, val, n, W, hot, boost, N=None, blank=0):
    """lb [T], ids [T, K], val [T, K], n [T] of ONE utterance, a hot-word set and a boost -> BiasResult."""
    s = float(np.float32(boost))
    assert s >= 0 and math.isfinite(s)
    hot = clean_set(hot)
    lb = np.asarray(lb, dtype=np.float64).reshape(-1)
    T = lb.shape[0]
    ids = np.asarray(ids)
    K = ids.shape[-1]
    ids = ids.reshape(T, K)
    val = np.asarray(val, dtype=np.float64).reshape(T, K)
    n = np.asarray(n).reshape(T)
    N = W if N is None else N
    assert 1 <= N <= W
    if any(int(n[t]) == 0 or math.isnan(lb[t]) for t in range(T)):
        return BiasResult([], math.inf, math.inf, [])
    memo = {}

    def md(prefix):
        if prefix not in memo:
            memo[prefix] = walk(prefix, hot)
        return memo[prefix]

    def bias(prefix):
        m, d = md(prefix)
        return s * (m + d)

    beam = [[(), 0.0, NEG]]
    gap = gap_pos = math.inf
    for t in range(T):
        cand = [(r, int(ids[t, r]), float(val[t, r])) for r in range(int(n[t])) if int(ids[t, r]) != blank]
        lp = {c: v for _, c, v in cand}
        stay = []
        for prefix, pb, pnb in beam:
            tot = R.lse(pb, pnb)
            e = prefix[-1] if prefix else None
            stay.append([tot + lb[t], pnb + lp[e] if prefix and e in lp else NEG])
        where = {b[0]: j for j, b in enumerate(beam)}
        assert len(where) == len(beam)
        ext = []
        for i, (prefix, pb, pnb) in enumerate(beam):
            tot = R.lse(pb, pnb)
            e = prefix[-1] if prefix else None
            for r, c, v in cand:
                base = pb if c == e else tot
                if base == NEG:
                    continue
                value = base + v
                new = prefix + (c,)
                if new in where:
                    q = where[new]
                    stay[q][1] = R.lse(stay[q][1], value)
                else:
                    ext.append((i * (K + 1) + 1 + r, new, value))
        allc = []                                  # (key, index, prefix, pb', pnb', total)
        for i, (prefix, pb, pnb) in enumerate(beam):
            tot = R.lse(stay[i][0], stay[i][1])
            allc.append((tot + bias(prefix), i * (K + 1), prefix, stay[i][0], stay[i][1], tot))
        for idx, new, value in ext:
            allc.append((value + bias(new), idx, new, NEG, value, value))
        allc = [c for c in allc if c[5] != NEG]
        allc.sort(key=lambda c: (-c[0], c[1]))
        if len(allc) > W:
            g = allc[W - 1][0] - allc[W][0]
            gap = min(gap, g)
            if g != 0:
                gap_pos = min(gap_pos, g)
        beam = [[c[2], c[3], c[4]] for c in allc[:W]]
    final = []
    for rank, (prefix, pb, pnb) in enumerate(beam):
        ll = R.lse(pb, pnb)
        m = md(prefix)[0]
        final.append((prefix, ll + s * m, m, ll, rank))
    final.sort(key=lambda f: (-f[1], f[4]))
    final = [f[:4] for f in final]
    for a, b in zip(final, final[1:]):
        gap = min(gap, a[1] - b[1])
        if a[1] != b[1]:
            gap_pos = min(gap_pos, a[1] - b[1])
    return BiasResult(final[:N], gap, gap_pos, final)


# ---- the hot-word recipe of the case tables (ctcbeam_ref.CPU_CASES / GPU_CASES) ------------------------------------------
RECIPE_BOOST = 2.0


def case_hotwords(case):
    """Deterministic: from the unbiased definition's hypothesis number min(n_hyp - 1, 3) its ids [0:3] and [4:6] where they
    exist, plus two random words of 2 and 4 ids from default_rng(seed + 7).integers(1, V)."""
    _name, seed, _T, V, _K, _W, _kind = case
    ref = R.case_reference(case)
    hot = []
    if ref.n_hyp > 0:
        y = ref.hyps[min(ref.n_hyp - 1, 3)][0]
        if len(y[0:3]) > 0:
            hot.append(tuple(int(c) for c in y[0:3]))
        if len(y[4:6]) > 0:
            hot.append(tuple(int(c) for c in y[4:6]))
    rng = np.random.default_rng(seed + 7)
    hot.append(tuple(int(c) for c in rng.integers(1, V, 2)))
    hot.append(tuple(int(c) for c in rng.integers(1, V, 4)))
    return hot


def flat(hot):
    """(ids int32 [sum of lengths], lens int32 [H]) as the C entry points take a set (empty entries kept: they are dropped
    there)."""
    ids = np.asarray([c for w in hot for c in w], dtype=np.int32)
    lens = np.asarray([len(w) for w in hot], dtype=np.int32)
    return ids, lens


_cache = {}


def case_reference(case, boost=RECIPE_BOOST, hot=None, T=None):
    """The biased definition's result for a table entry (its first T frames), computed once per process."""
    key = (case, float(np.float32(boost)), None if hot is None else tuple(map(tuple, hot)), T)
    if key not in _cache:
        lb, ids, val, n = R.case_arrays(case)
        TT = lb.shape[0] if T is None else T
        h = case_hotwords(case) if hot is None else hot
        _cache[key] = beam_search(lb[:TT], ids[:TT], val[:TT], n[:TT], case[5], h, boost)
    return _cache[key]
