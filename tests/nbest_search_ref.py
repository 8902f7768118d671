"""Position-synchronous beam search over paraformer's per-position top-k lists, with optional hot-word and n-gram LM shallow
fusion: the definition the host twin (pf_host_nbest_search) and the kernel (k_nbestsearch.hip, pf_op_nbest_search,
pf_fetch_nbest_search) are compared with.  Float64 Python; the LM is tests/ctcbeam_lm_ref.py's Model (a dict of n-grams), the
hot-word terms m and d are tests/ctcbeam_bias_ref.py's walk (plain text, no automaton), both read over an id sequence.

INPUTS per utterance: the top-k block as pf_fetch_topk returns it — ids [L, K], val [L, K] float32, n [L] — and
n_free = min(L, max(token_num, 0)); 1 <= N <= W <= PF_NBEST_MAX, K <= PF_TOPK_MAX; optionally a hot-word set with a boost s
(float32) and a model with alpha >= 0, beta (float32) and flags.  float32 inputs are widened, all scores are float64;
alpha * x and s * integer are exact products, every + is ONE rounded addition in the order written, nothing transcendental is
evaluated.  So definition, twin and kernel agree BIT FOR BIT on every input, ties included: no decision-gap condition.

BEAM: an ordered list of at most W entries (rank prefix, a, LM context, g, hot-word segment, m); it starts as
[((), +0.0, start, +0.0, (), 0)].  The hot-word segment is what ctcbeam_bias_ref.walk carries between tokens (hot_step below).

POSITION l < n_free: beam entry i (in rank order) and list rank r < n[l] make candidate index i * K + r with c = ids[l, r]:
    a' = a + val[l, r];  one LM step on c gives g';  one hot-word step on c gives m', d'
    key = (a' + s * (m' + d')) + g'        the hot-word term only with a set that biases, the g term only with a model
No candidate is discarded (-inf orders like any other value).  The W best by key stay, ties to the smaller candidate index;
that order is the new beam's.  There is no merging: the ids of a list are distinct, so distinct candidates spell distinct
sequences.

POSITIONS n_free <= l < L: every entry takes rank 0, a = a + val[l, 0], in order; the LM and the hot words do not see these
ids (as pf_host_nbest keeps them at rank 0).

FINISH: with PF_LM_EOS and an eos id one eos step without beta; score = (a + s * m) + g_final (the pending part d is revoked);
re-ordered by descending score, ties to the smaller beam rank; the first N are the hypotheses, each with ranks [L], score,
loglik_sum = a, lm_sum = g_final, matched = m.  score == (loglik_sum + s * matched) + lm_sum bit for bit.

NO HYPOTHESES: n_hyp = 0 when L = 0, when some n[l] == 0 for l < L, or when a listed value is NaN or +inf.

CONSEQUENCES: with no set and alpha = beta = 0 every score is pf_host_nbest's score of that rank vector bit for bit, and with
W >= N the list is pf_host_nbest's whenever no two hypotheses tie (only the tie rules differ); with W >= K ** n_free nothing is
pruned and the list is the brute-force enumeration sorted by score (brute_force below)."""
import itertools
import math

import numpy as np

import ctcbeam_bias_ref as BR
import ctcbeam_lm_ref as LR

PF_LM_EOS = LR.PF_LM_EOS
PF_NBEST_MAX = 64
PF_TOPK_MAX = 8
f32 = LR.f32


class Hyp:
    def __init__(self, ranks, score, loglik_sum, lm_sum, matched):
        self.ranks, self.score, self.loglik_sum, self.lm_sum, self.matched = tuple(ranks), score, loglik_sum, lm_sum, matched

    def key(self):
        """Everything, floats by their bits: what bit-for-bit equality compares."""
        return (self.ranks, bits(self.score), bits(self.loglik_sum), bits(self.lm_sum), self.matched)

    def __repr__(self):
        return "Hyp(%r, %r, %r, %r, %r)" % (self.ranks, self.score, self.loglik_sum, self.lm_sum, self.matched)


def bits(x):
    return int(np.float64(x).view(np.int64))


def _prepare(ids, val, n, token_num):
    ids = np.asarray(ids)
    K = ids.shape[-1]
    ids = ids.reshape(-1, K)
    L = ids.shape[0]
    val = np.asarray(val, np.float32).reshape(L, K).astype(np.float64)
    n = np.asarray(n).reshape(L)
    assert all(0 <= int(k) <= K for k in n)
    n_free = min(L, max(int(token_num), 0))
    ok = L > 0
    for l in range(L):
        if int(n[l]) == 0:
            ok = False
        for r in range(int(n[l])):
            if math.isnan(val[l, r]) or val[l, r] == math.inf:
                ok = False
    return ids, val, n, L, K, n_free, ok


def _weights(model, alpha, beta, hot, boost):
    a, b, s = f32(alpha), f32(beta), f32(boost)
    assert s >= 0 and math.isfinite(s)
    if model is not None:
        assert a >= 0 and math.isfinite(a) and math.isfinite(b)
    hot = BR.clean_set(hot)
    return a, b, s, hot, (s > 0 and len(hot) > 0)


def hot_step(seg, m, c, hot):
    """One token of ctcbeam_bias_ref.walk, carried: (segment, m, d) after c.  The segment read since the last completion grows
    by c; the longest hot word that is a suffix of it completes (m += its length, the segment empties); d is the longest
    suffix of the segment that is a proper prefix of a hot word.  walk(y) itself scores the brute-force enumeration."""
    seg = seg + (int(c),)
    best = 0
    for w in hot:
        if best < len(w) <= len(seg) and seg[len(seg) - len(w):] == w:
            best = len(w)
    if best:
        return (), m + best, 0
    d = 0
    for w in hot:
        for k in range(min(len(w) - 1, len(seg)), d, -1):
            if seg[len(seg) - k:] == w[:k]:
                d = k
                break
    return seg[len(seg) - d:] if d else (), m, d


def search(ids, val, n, token_num, W, N=None, model=None, alpha=0.0, beta=0.0, flags=0, hot=(), boost=0.0):
    """The definition: [Hyp] (at most N, in the output order) of ONE utterance."""
    N = W if N is None else N
    assert 1 <= N <= W <= PF_NBEST_MAX
    ids, val, n, L, K, n_free, ok = _prepare(ids, val, n, token_num)
    assert 1 <= K <= PF_TOPK_MAX
    a_, b_, s, hot, biased = _weights(model, alpha, beta, hot, boost)
    if not ok:
        return []
    # (ranks, a, h, g, y, m): y the segment the hot words have read since the last completion, h the LM context
    beam = [((), 0.0, model.start() if model is not None else (), 0.0, (), 0)]
    for l in range(n_free):
        cand = []
        for i, (ranks, a, h, g, y, m) in enumerate(beam):
            for r in range(int(n[l])):
                c = int(ids[l, r])
                a1 = a + float(val[l, r])
                g1, h1 = (model.step(g, h, c, a_, b_) if model is not None else (g, h))
                key = a1
                y1, m1 = y, m
                if biased:
                    y1, m1, d1 = hot_step(y, m, c, hot)
                    key = key + s * (m1 + d1)
                if model is not None:
                    key = key + g1
                cand.append((key, i * K + r, (ranks + (r,), a1, h1, g1, y1, m1)))
        cand.sort(key=lambda x: (-x[0], x[1]))
        beam = [x[2] for x in cand[:W]]
    final = []
    for rank, (ranks, a, h, g, y, m) in enumerate(beam):
        for l in range(n_free, L):
            a = a + float(val[l, 0])
        if model is not None and (flags & PF_LM_EOS) and model.eos >= 0:
            g, h = model.step(g, h, model.eos, a_, b_, bonus=False)
        sc = a
        if biased:
            sc = sc + s * m
        if model is not None:
            sc = sc + g
        final.append((sc, rank, Hyp(ranks + (0,) * (L - n_free), sc, a, g, m)))
    final.sort(key=lambda x: (-x[0], x[1]))
    return [x[2] for x in final[:N]]


def brute_force(ids, val, n, token_num, N, model=None, alpha=0.0, beta=0.0, flags=0, hot=(), boost=0.0):
    """Every rank vector scored from scratch (the LM by Model.score over the whole sequence, m by one walk), [Hyp] sorted by
    descending score (N = None: all).  The unpruned search orders equal scores by the beam rank the vector reached, a function
    of the keys along the way: compare through grouped(), which does not depend on the order inside a tie."""
    ids, val, n, L, K, n_free, ok = _prepare(ids, val, n, token_num)
    a_, b_, s, hot, biased = _weights(model, alpha, beta, hot, boost)
    if not ok:
        return []
    out = []
    for ranks in itertools.product(*[range(int(n[l])) if l < n_free else range(1) for l in range(L)]):
        a = 0.0
        for l in range(L):
            a = a + float(val[l, ranks[l]])
        y = tuple(int(ids[l, ranks[l]]) for l in range(n_free))
        g = 0.0
        if model is not None:
            g = model.score(y, a_, b_, flags)[0]
        m = BR.walk(y, hot)[0] if biased else 0
        sc = a
        if biased:
            sc = sc + s * m
        if model is not None:
            sc = sc + g
        out.append(Hyp(ranks, sc, a, g, m))
    out.sort(key=lambda h: -h.score)
    return out[:N] if N is not None else out


def grouped(hyps):
    """[(score bits, frozenset of Hyp.key())] in list order: equal lists up to the order inside a tie compare equal."""
    out = []
    for h in hyps:
        if out and out[-1][0] == bits(h.score):
            out[-1][1].add(h.key())
        else:
            out.append((bits(h.score), {h.key()}))
    return [(b, frozenset(k)) for b, k in out]


# ---- the case table (tests/test_nbest_search_cpu.py, tests/test_gpu_nbest_search.py, tests/native/nbest_search_sanitize.cpp) ----
def log_softmax_lists(rng, L, K, V):
    """Seeded random log-softmax rows -> (ids [L, K] int64, val [L, K] float32, n [L]) by tests/topk_ref.py's selection."""
    import topk_ref as TR
    x = rng.standard_normal((L, V)).astype(np.float32) * np.float32(2.0)
    y = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    return TR.topk_ref(y, K)


def small_model(V, order=3, bos=-1, eos=-1, unk=-1, transparent=(), missing=(), seed=5):
    """A model of the given order over [1, V): every id but `missing` a unigram, V random n-grams per higher order."""
    rng = np.random.default_rng(seed)
    grams = {}
    for c in range(1, V):
        if c not in missing:
            grams[(c,)] = (np.float32(rng.uniform(-4.0, -0.5)), np.float32(rng.uniform(-1.0, 0.0)))
    for k in range(2, order + 1):
        for x in range(3 * V):
            w = tuple(int(c) for c in rng.integers(1, V, k))
            if all((c,) in grams for c in w) and w not in grams:
                grams[w] = (np.float32(rng.uniform(-3.0, -0.2)), None if x % 4 == 0 or k == order else np.float32(rng.uniform(-0.7, 0.0)))
    return LR.Model(order, grams, V, bos=bos, eos=eos, unk=unk, oov=-7.5, transparent=transparent)


def model_arrays(model):
    """A Model as pf_host_lm_build's arrays: (order, counts, ids, logp, backoff)."""
    counts, ids, logp, bo = [], [], [], []
    for k in range(1, model.order + 1):
        ws = sorted(w for w in model.ngrams if len(w) == k)
        counts.append(len(ws))
        for w in ws:
            ids += list(w)
            logp.append(model.ngrams[w][0])
            bo.append(np.nan if model.ngrams[w][1] is None else model.ngrams[w][1])
    return (model.order, np.asarray(counts, np.int64), np.asarray(ids, np.int32), np.asarray(logp, np.float32),
            np.asarray(bo, np.float32))


TABLE_SHAPES = ((5, 2), (3, 4), (3, 3), (4, 2))          # (L, K): K ** L <= 64
TABLE_VARIANTS = ("plain", "ragged", "tied", "neginf")


def table_lists(L, K, variant, seed=0):
    """The small inputs of the brute-force table: per position K distinct ids of [1, K + 3) with descending float32 values.
    ragged: n[l] varies in 1 .. K (id -1 / value -inf past it); tied: equal values within and across positions; neginf: one
    listed value is -inf."""
    rng = np.random.default_rng(1000 * L + 10 * K + seed)
    V = K + 3
    ids = np.full((L, K), -1, np.int64)
    val = np.full((L, K), -np.inf, np.float32)
    n = np.full(L, K, np.int32)
    for l in range(L):
        if variant == "ragged":
            n[l] = int(rng.integers(1, K + 1))
        ids[l, :n[l]] = rng.permutation(np.arange(1, V))[:n[l]]
        v = np.sort(rng.uniform(-6.0, -0.05, int(n[l])).astype(np.float32))[::-1]
        if variant == "tied":
            v = np.round(v * 2) / 2                  # halves: many equal values and equal sums
        val[l, :n[l]] = v
    if variant == "neginf":
        val[L // 2, int(n[L // 2]) - 1] = -np.inf
    return ids, val, n, V


def fusion_forms(ids, n, n_free, V):
    """[(name, model, alpha, beta, flags, hot, boost)]: the plain search, LMs of order 1 - 3 with and without bos / eos / unk, a
    transparent id, a missing unigram, PF_LM_EOS on and off; hot words — one completed at the last free position, one left as
    a pending partial match there; both together."""
    L = len(n)
    last = max(n_free - 1, 0)
    r1 = lambda l: int(ids[l, min(1, int(n[l]) - 1)])                                   # noqa: E731
    hot = []
    if L > 0 and n_free >= 2:
        hot.append((r1(last - 1), int(ids[last, 0])))              # completes at the last free position
        hot.append((r1(last), 1 + (r1(last) % (V - 1)), 2))       # its first id at the last free position: a pending match
        hot.append((int(ids[0, 0]), r1(1)))
    elif L > 0:
        hot.append((int(ids[0, 0]),))
        hot.append((r1(0), 2))
    forms = [("plain", None, 0.0, 0.0, 0, (), 0.0),
             ("lm1", small_model(V, 1), 0.7, 0.0, 0, (), 0.0),
             ("lm2-bos-eos", small_model(V, 2, bos=1, eos=2), 0.4, 0.5, PF_LM_EOS, (), 0.0),
             ("lm3-bos-eos-off", small_model(V, 3, bos=2, eos=1), 1.0, -0.25, 0, (), 0.0),
             ("lm2-missing-oov", small_model(V, 2, missing=(V - 1,)), 0.5, 0.25, 0, (), 0.0),
             ("lm2-missing-unk", small_model(V, 2, unk=1, eos=2, missing=(V - 1,)), 0.5, 0.0, PF_LM_EOS, (), 0.0),
             ("lm3-transparent", small_model(V, 3, eos=2, transparent=(3,)), 0.6, 0.1, PF_LM_EOS, (), 0.0),
             ("hot", None, 0.0, 0.0, 0, hot, 1.5),
             ("hot+lm3", small_model(V, 3, bos=1, eos=2), 0.5, 0.5, 0, hot, 2.0),
             ("hot+lm2-eos", small_model(V, 2, bos=1, eos=2, missing=(V - 1,)), 0.3, 1.0, PF_LM_EOS, hot, 0.75)]
    return forms


def as_hyps(res, b=0):
    """An engine.NbestSearchResult's utterance b as [Hyp]."""
    return [Hyp(res.ranks[b, i].tolist(), float(res.score[b, i]), float(res.loglik_sum[b, i]), float(res.lm_sum[b, i]),
                int(res.matched[b, i])) for i in range(int(res.n_hyp[b]))]
