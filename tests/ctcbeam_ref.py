"""CTC prefix beam search over per-frame top-k lists: the definition the host twin (pf_host_ctc_beam) and the device kernel
(k_ctcbeam.hip) are compared with.  Float64 throughout; fp32 inputs are widened first.

Per utterance: T frames, the blank log-prob lb[t], the frame's top-k list ids[t, 0..K) / val[t, ..] / n[t] as launch_topk
leaves it.  lse(a, b) = max + log1p(exp(-|a - b|)), an argument of -inf gives the other one.

The beam is an ordered list of at most W entries (prefix, pb, pnb), starting as [((), 0, -inf)].  At frame t the candidates
C_t are the listed entries r < n[t] whose id is not blank.  For beam entry i (last token e, tot = lse(pb, pnb)):
  stay      (candidate index i*(K+1)):       pb' = tot + lb[t];  pnb' = pnb + lp_t(e) when the prefix is non-empty and e in C_t
  extend c  (candidate index i*(K+1)+1+r):   pnb' = (c == e ? pb : tot) + lp_t(c), pb' = -inf; dropped when the base is -inf
  merge     prefix + c is the prefix of beam entry q: the value is folded into q's stay candidate, pnb'_q = lse(pnb'_q, value)
  select    candidates whose total is -inf are discarded; the W best by total stay, ties to the smaller candidate index.
After the last frame the first N <= W entries are the hypotheses.  No hypothesis when a frame has n[t] == 0 or a NaN blank.

identity="parent" is the FAULTY variant in which a prefix is a node (parent node, token) and an extension meets q only when
q's node hangs off p's node: a prefix that left the beam and was re-created under a new node no longer meets its descendants.
Tests use it to pick inputs on which node identity and sequence identity differ."""
import itertools
import math

import numpy as np

NEG = -math.inf


def lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def tol(T, s):
    """The comparison bound of a score: at most 16 roundings of relative size 2^-53 per frame on magnitudes <= |s|."""
    return 16.0 * max(T, 1) * 2.0 ** -53 * max(1.0, abs(s))


class BeamResult:
    def __init__(self, hyps, gap, beam, gap_pos=math.inf):
        self.hyps = hyps          # [(ids tuple, score)], at most N
        self.gap = gap            # the smallest decision gap met (inf when no decision was made): the W-th kept total minus
        #                           the best dropped one at every frame, and neighbouring totals of the final beam
        self.gap_pos = gap_pos    # the same over the gaps that are not exactly 0 (inputs with mirrored columns tie exactly)
        self.beam = beam          # the whole final beam [(ids tuple, score)], at most W

    @property
    def n_hyp(self):
        return len(self.hyps)


def beam_search(lb, ids, val, n, W, N=None, blank=0, identity="exact"):
    """lb [T], ids [T, K], val [T, K], n [T] of ONE utterance -> BeamResult."""
    assert identity in ("exact", "parent")
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
        return BeamResult([], math.inf, [])
    # entry: [prefix, pb, pnb, node, parent node]
    beam = [[(), 0.0, NEG, 0, -1]]
    next_node = 1
    gap = gap_pos = math.inf
    for t in range(T):
        cand = [(r, int(ids[t, r]), float(val[t, r])) for r in range(int(n[t])) if int(ids[t, r]) != blank]
        lp = {c: v for _, c, v in cand}
        stay = []
        for prefix, pb, pnb, node, par in beam:
            tot = lse(pb, pnb)
            e = prefix[-1] if prefix else None
            stay.append([tot + lb[t], pnb + lp[e] if prefix and e in lp else NEG])
        ext = []                                   # (candidate index, prefix, pnb', parent node)
        where = {b[0]: j for j, b in enumerate(beam)} if identity == "exact" else None
        assert where is None or len(where) == len(beam)          # prefixes are unique
        for i, (prefix, pb, pnb, node, par) in enumerate(beam):
            tot = lse(pb, pnb)
            e = prefix[-1] if prefix else None
            for r, c, v in cand:
                base = pb if c == e else tot
                if base == NEG:
                    continue
                value = base + v
                new = prefix + (c,)
                if identity == "exact":
                    q = [where[new]] if new in where else []
                else:
                    q = [j for j, b in enumerate(beam) if b[4] == node and b[0] and b[0][-1] == c]
                if q:
                    stay[q[0]][1] = lse(stay[q[0]][1], value)
                else:
                    ext.append((i * (K + 1) + 1 + r, new, value, node))
        allc = []                                  # (total, index, prefix, pb', pnb', node or None, parent node)
        for i, (prefix, pb, pnb, node, par) in enumerate(beam):
            allc.append((lse(stay[i][0], stay[i][1]), i * (K + 1), prefix, stay[i][0], stay[i][1], node, par))
        for idx, new, value, pnode in ext:
            allc.append((value, idx, new, NEG, value, None, pnode))
        allc = [c for c in allc if c[0] != NEG]
        allc.sort(key=lambda c: (-c[0], c[1]))
        if len(allc) > W:
            g = allc[W - 1][0] - allc[W][0]
            gap = min(gap, g)
            if g != 0:
                gap_pos = min(gap_pos, g)
        beam = []
        for total, idx, prefix, pb, pnb, node, par in allc[:W]:
            if node is None:
                node = next_node
                next_node += 1
            beam.append([prefix, pb, pnb, node, par])
    final = [(b[0], lse(b[1], b[2])) for b in beam]
    for a, b in zip(final, final[1:]):
        gap = min(gap, a[1] - b[1])
        if a[1] != b[1]:
            gap_pos = min(gap_pos, a[1] - b[1])
    return BeamResult(final[:N], gap, final, gap_pos)


def collapse(path, blank=0):
    out = []
    prev = None
    for y in path:
        if y != blank and y != prev:
            out.append(y)
        prev = y
    return tuple(out)


def brute_force(logp, blank=0):
    """{labeling: log-probability} by enumeration of all V^T alignments of logp [T, V] (float64)."""
    logp = np.asarray(logp, dtype=np.float64)
    T, V = logp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        for t, y in enumerate(path):
            s += logp[t, y]
        acc.setdefault(collapse(path, blank), []).append(s)
    return {k: math.log(math.fsum(math.exp(x) for x in v)) for k, v in acc.items()}


def ctc_loglik(logp, labels, blank=0):
    """The CTC forward log-likelihood of `labels` under logp [T, V] (float64): the sum over all of its alignments."""
    logp = np.asarray(logp, dtype=np.float64)
    T = logp.shape[0]
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    S = len(ext)
    if T == 0:
        return 0.0 if not labels else NEG
    a = [NEG] * S
    a[0] = logp[0, ext[0]]
    if S > 1:
        a[1] = logp[0, ext[1]]
    for t in range(1, T):
        b = [NEG] * S
        for s in range(S):
            v = a[s]
            if s >= 1:
                v = lse(v, a[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = lse(v, a[s - 2])
            b[s] = v + logp[t, ext[s]] if v != NEG else NEG
        a = b
    return lse(a[S - 1], a[S - 2]) if S > 1 else a[0]


def topk_lists(logp32, K):
    """Top-k lists of fp32 rows [T, V] in launch_topk's order (larger value, then larger index; NaN never ranked)."""
    x = np.asarray(logp32, dtype=np.float32)
    T, V = x.shape
    ids = np.full((T, K), -1, np.int64)
    val = np.full((T, K), -np.inf, np.float32)
    n = np.zeros(T, np.int32)
    for t in range(T):
        order = sorted((v for v in range(V) if not np.isnan(x[t, v])), key=lambda v: (-float(x[t, v]), -v))[:K]
        n[t] = len(order)
        for r, v in enumerate(order):
            ids[t, r] = v
            val[t, r] = x[t, v]
    return ids, val, n


def random_rows(seed, T, V, scale=1.5):
    """Rows scale * normal, log-softmax in float64, narrowed to fp32."""
    rng = np.random.default_rng(seed)
    z = scale * rng.standard_normal((T, V))
    z = z - z.max(axis=1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    return lp.astype(np.float32)


def mirrored_rows(seed, T, V, a, b, scale=1.5):
    """random_rows with column b made a bit-identical copy of column a (rows no longer normalised: the search does not care)."""
    x = random_rows(seed, T, V, scale)
    x[:, b] = x[:, a]
    return x


def case_inputs(logp32, K, blank=0):
    """(lb [T] fp32, ids, val, n) of one utterance from its fp32 rows."""
    ids, val, n = topk_lists(logp32, K)
    return np.ascontiguousarray(logp32[:, blank]), ids, val, n


# ---- the committed inputs of tests/test_ctcbeam_cpu.py and tests/test_gpu_ctcbeam.py ----------------------------------------
# (name, seed, T, V, K, W, kind).  kind: "random"; "lowblank" / "highblank": the blank column shifted by -8 / +3 (blank outside
# / at the head of the lists); "ragged": n[t] drawn from 1 .. K; "mirror": columns 2 and 4 bit-identical copies of 1 and 3.
# PARENT_SEEDS: T = 12, V = 4, K = 3, W = 3 inputs on which identity="parent" gives another list than the definition.
PARENT_SEEDS = (6, 107, 198)
CPU_CASES = [("parent%d" % s, s, 12, 4, 3, 3, "random") for s in PARENT_SEEDS]
CPU_CASES += [("w%d_k%d" % (W, K), 10 * W + K, 30, 12, K, W, "random") for W in (1, 2, 3, 16, 64) for K in (1, 4, 8)]
CPU_CASES += [("lowblank", 21, 24, 10, 4, 8, "lowblank"), ("highblank", 22, 24, 10, 4, 8, "highblank"),
              ("ragged", 23, 40, 16, 8, 16, "ragged"), ("ragged_k4", 24, 33, 9, 4, 3, "ragged"),
              ("mirror", 25, 20, 8, 4, 8, "mirror"), ("mirror_w3", 26, 16, 6, 5, 3, "mirror"), ("mirror_w64", 27, 12, 6, 8, 64, "mirror")]
GPU_CASES = [("t%d" % T, 300 + T, T, 14, 4, 16, "random") for T in (1, 12, 63, 64, 65, 130)]
GPU_CASES += [("full_lds", 41, 65, 40, 8, 64, "random"), ("ragged", 23, 40, 16, 8, 16, "ragged"), ("lowblank", 21, 24, 10, 4, 8, "lowblank"),
              ("mirror", 25, 20, 8, 4, 8, "mirror"), ("mirror_w64", 27, 12, 6, 8, 64, "mirror"), ("w1", 44, 20, 9, 8, 1, "random")]
GPU_CASES += [c for c in CPU_CASES if c[0].startswith("parent")]


def case_arrays(case):
    """(lb [T] fp32, ids [T, K] int64, val [T, K] fp32, n [T] int32) of one table entry."""
    _name, seed, T, V, K, _W, kind = case
    x = random_rows(seed, T, V)
    if kind == "lowblank":
        x[:, 0] -= np.float32(8)
    elif kind == "highblank":
        x[:, 0] += np.float32(3)
    elif kind == "mirror":
        x[:, 2] = x[:, 1]
        x[:, 4] = x[:, 3]
    lb, ids, val, n = case_inputs(x, K)
    if kind == "ragged":
        n = np.minimum(n, np.random.default_rng(seed + 1000).integers(1, K + 1, T)).astype(np.int32)
        for t in range(T):
            ids[t, n[t]:] = -1
            val[t, n[t]:] = -np.inf
    return lb, ids, val, n


_ref_cache = {}


def case_reference(case, T=None):
    """The definition's result for a table entry (its first T frames), computed once per process."""
    key = (case, T)
    if key not in _ref_cache:
        lb, ids, val, n = case_arrays(case)
        T = lb.shape[0] if T is None else T
        _ref_cache[key] = beam_search(lb[:T], ids[:T], val[:T], n[:T], case[5])
    return _ref_cache[key]
