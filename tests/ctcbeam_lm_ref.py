"""N-gram LM shallow fusion inside the CTC prefix beam search: the definition the builder and scorer (pf_host_lm_build,
pf_host_lm_score, pf_host_lm_from_arpa), the host twin (pf_host_ctc_beam_lm), the walk kernel (pf_op_lm_score) and the kLm forms
of the search kernel (k_ctcbeam.hip) are compared with.  Float64 Python on top of tests/ctcbeam_ref.py and
tests/ctcbeam_bias_ref.py; no automaton, no image: n-grams are looked up in a dict by their token tuple.

THE MODEL: a back-off n-gram LM of order O (1 <= O <= 8) over token ids in [1, V): {n-gram: (logp, back-off or None)} with
float32 natural-log weights (a back-off at order O is ignored), optional bos / eos / unk ids (-1: none; an unk must be a
listed unigram), a float32 oov log-probability used when there is no unk, a set of TRANSPARENT ids.

ONE STEP (Model.step): g and the context h are functions of the label sequence alone.  Start: g = +0.0, h = (bos) with a bos,
else ().  For a token c:
  * c transparent: nothing changes — no weight, no bonus, same h.
  * c is no listed unigram: with an unk, c is replaced by unk for scoring and for the context; else g = (g + alpha * oov) + beta
    and h = ().
  * otherwise h' = the last min(|h|, O - 1) tokens of h; repeat: if h' . c is listed, g = g + alpha * logp(h' . c) and stop;
    else, if h' is listed with a back-off, g = g + alpha * bo(h'); drop the first token of h'.  Then g = g + beta.  The new h is
    the longest suffix of h . c that is a listed n-gram of order < O.
alpha >= 0 and beta are float32 widened to float64, as every weight; alpha * x is the product of two widened float32 values,
hence exact in float64; every + is ONE rounded float64 addition in exactly this order (a fused multiply-add of an exact
product rounds the same).  g of the definition, of the host scorer and of the kernels are bit-equal.
END OF SENTENCE: with PF_LM_EOS and an eos id a hypothesis takes one more step for eos at finish, without beta.

THE SEARCH is ctcbeam_bias_ref.beam_search (ctcbeam_ref.beam_search when no hot-word set biases) with one more term:
  select   key = (total + boost * (m + d)) + g(prefix), the hot-word term only with a set that biases; a candidate whose total
           is -inf is still discarded; the W best by key stay, ties to the smaller candidate index; pb / pnb stay unfused
           (equal prefixes have equal g, so folding a merged extension into the stay candidate stays valid).
  finish   score = (lse(pb, pnb) + boost * m) + g_final; re-ordered by descending score, ties to the smaller beam rank;
           per hypothesis ids, score, matched = m, loglik_sum = lse(pb, pnb), lm_sum = g_final.
alpha = beta = 0: every g is +0.0 and the lists and scores are the unfused ones bit for bit.

COMPARISON: token lists identical and in the same order; lm_sum and matched bit-equal; score and loglik_sum within
ctcbeam_bias_ref.tol.  Roundings behind a score: at most 16 per frame in lse(pb, pnb) (ctcbeam_ref.tol), one for
+ boost * m (the product is exact: float32 by a small integer) and one for + g_final; g_final itself carries NO error
against the definition (bit-equal), so 16 T + 2 <= the 16 T + 4 that ctcbeam_bias_ref.tol allows, on the largest magnitude
among score, loglik_sum and lm_sum."""
import math

import numpy as np

import ctcbeam_bias_ref as BR
import ctcbeam_ref as R

NEG = R.NEG
LN10 = 2.302585092994046
PF_LM_EOS = 1
PF_LM_ORDER_MAX = 8


def f32(x):
    return float(np.float32(x))


class Model:
    def __init__(self, order, ngrams, V, bos=-1, eos=-1, unk=-1, oov=-10.0, transparent=()):
        assert 1 <= order <= PF_LM_ORDER_MAX
        self.order, self.V, self.bos, self.eos, self.unk = int(order), int(V), int(bos), int(eos), int(unk)
        self.ngrams = {tuple(int(c) for c in w): v for w, v in ngrams.items()}         # as given: what the builders are fed
        self.logp = {w: f32(v[0]) for w, v in self.ngrams.items()}
        self.bo = {w: f32(v[1]) for w, v in self.ngrams.items() if v[1] is not None and len(w) < order}
        self.oov = f32(oov)
        self.transparent = frozenset(int(c) for c in transparent)
        assert all(1 <= len(w) <= order and all(1 <= c < V for c in w) for w in self.logp)
        assert unk < 0 or (unk,) in self.logp

    def start(self):
        return (self.bos,) if self.bos >= 0 else ()

    def step(self, g, h, c, alpha, beta, bonus=True):
        """(g, h) after token c."""
        c = int(c)
        if c in self.transparent:
            return g, h
        if (c,) not in self.logp:
            if self.unk >= 0:
                c = self.unk
            else:
                g = g + alpha * self.oov
                if bonus:
                    g = g + beta
                return g, ()
        hp = h[len(h) - min(len(h), self.order - 1):]
        while True:
            if hp + (c,) in self.logp:
                g = g + alpha * self.logp[hp + (c,)]
                break
            if hp in self.bo:
                g = g + alpha * self.bo[hp]
            hp = hp[1:]                            # (the empty context finds the unigram: c is listed)
        if bonus:
            g = g + beta
        full = h + (c,)
        new = ()
        for k in range(min(len(full), self.order - 1), 0, -1):
            if full[len(full) - k:] in self.logp:
                new = full[len(full) - k:]
                break
        return g, new

    def score(self, y, alpha, beta, flags=0):
        """(g, [g after every token]) of the sequence y; PF_LM_EOS adds the end-of-sentence step to g."""
        a, b = f32(alpha), f32(beta)
        g, h = 0.0, self.start()
        pos = []
        for c in y:
            g, h = self.step(g, h, c, a, b)
            pos.append(g)
        if (flags & PF_LM_EOS) and self.eos >= 0:
            g, h = self.step(g, h, self.eos, a, b, bonus=False)
        return g, pos


def tol(T, *magnitudes):
    """The comparison bound of a fused score or loglik_sum (see COMPARISON above)."""
    return BR.tol(T, max(abs(x) for x in magnitudes))


class LmResult:
    def __init__(self, hyps, gap, gap_pos, beam):
        self.hyps = hyps          # [(ids tuple, score, matched, loglik_sum, lm_sum)], at most N, in the output order
        self.gap = gap            # the smallest decision gap over fused keys (select) and final scores (inf: no decision)
        self.gap_pos = gap_pos    # the same over the gaps that are not exactly 0
        self.beam = beam          # all final entries in the output order

    @property
    def n_hyp(self):
        return len(self.hyps)


def beam_search(lb, ids, val, n, W, model, alpha, beta, flags=0, hot=(), boost=0.0, N=None, blank=0):
    """lb [T], ids [T, K], val [T, K], n [T] of ONE utterance, a Model with its weights, optionally a hot-word set -> LmResult."""
    a, b, s = f32(alpha), f32(beta), f32(boost)
    assert a >= 0 and math.isfinite(a) and math.isfinite(b) and s >= 0 and math.isfinite(s)
    hot = BR.clean_set(hot)
    biased = s > 0 and len(hot) > 0
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
        return LmResult([], math.inf, math.inf, [])
    md_memo, lm_memo = {}, {(): (0.0, model.start())}

    def md(prefix):
        if prefix not in md_memo:
            md_memo[prefix] = BR.walk(prefix, hot)
        return md_memo[prefix]

    def lm(prefix):                                # g is the same chain of additions however the prefix was reached
        if prefix not in lm_memo:
            g, h = lm(prefix[:-1])
            lm_memo[prefix] = model.step(g, h, prefix[-1], a, b)
        return lm_memo[prefix]

    def key(tot, prefix):
        k = tot + s * (md(prefix)[0] + md(prefix)[1]) if biased else tot
        return k + lm(prefix)[0]

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
        where = {x[0]: j for j, x in enumerate(beam)}
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
            if tot != NEG:
                allc.append((key(tot, prefix), i * (K + 1), prefix, stay[i][0], stay[i][1], tot))
        for idx, new, value in ext:
            if value != NEG:
                allc.append((key(value, new), idx, new, NEG, value, value))
        allc.sort(key=lambda c: (-c[0], c[1]))
        if len(allc) > W:
            d = allc[W - 1][0] - allc[W][0]
            gap = min(gap, d)
            if d != 0:
                gap_pos = min(gap_pos, d)
        beam = [[c[2], c[3], c[4]] for c in allc[:W]]
    final = []
    for rank, (prefix, pb, pnb) in enumerate(beam):
        ll = R.lse(pb, pnb)
        m = md(prefix)[0] if biased else 0
        g, h = lm(prefix)
        if (flags & PF_LM_EOS) and model.eos >= 0:
            g, h = model.step(g, h, model.eos, a, b, bonus=False)
        sc = ll + s * m if biased else ll
        final.append((prefix, sc + g, m, ll, g, rank))
    final.sort(key=lambda f: (-f[1], f[5]))
    final = [f[:5] for f in final]
    for x, y in zip(final, final[1:]):
        gap = min(gap, x[1] - y[1])
        if x[1] != y[1]:
            gap_pos = min(gap_pos, x[1] - y[1])
    return LmResult(final[:N], gap, gap_pos, final)


# ---- ARPA text ----------------------------------------------------------------------------------------------------------------
def read_arpa(path, tokens):
    """(order, {n-gram: (logp, back-off or None)}, dropped, bos, eos, unk, transparent) of an ARPA file against a token table:
    each value float32(float(text) * ln 10); words to ids by exact equality (first spelling wins); an n-gram with a word that
    is not in the table, or is id 0, is dropped and counted; <s> </s> <unk> by spelling (an unk the file does not list as a
    unigram is none); every token spelled <|...|> is transparent.  ValueError for a malformed file."""
    id_of = {}
    for i, t in enumerate(tokens):
        id_of.setdefault(t, i)
    transparent = [i for i, t in enumerate(tokens) if len(t) >= 4 and t.startswith("<|") and t.endswith("|>")]
    declared, ngrams, dropped = [], {}, 0
    k, seen, ended = 0, 0, False
    with open(path, encoding="utf-8") as f:
        for line in f:
            w = line.replace("\r", " ").replace("\t", " ").split(" ")
            w = [x for x in (y.strip("\n") for y in w) if x]
            if not w:
                continue
            if ended:
                raise ValueError("text after \\end\\")
            if k == 0:
                if w == ["\\data\\"]:
                    k = -1
                continue
            if w[0].startswith("\\"):
                if k >= 1 and seen != declared[k - 1]:
                    raise ValueError("section count")
                if w == ["\\end\\"]:
                    if (0 if k == -1 else k) != len(declared):
                        raise ValueError("\\end\\ early")
                    ended = True
                    continue
                want = 1 if k == -1 else k + 1
                if w != ["\\%d-grams:" % want] or want > len(declared):
                    raise ValueError("section header")
                k, seen = want, 0
                continue
            if k == -1:
                if len(w) != 2 or w[0] != "ngram" or not w[1].startswith("%d=" % (len(declared) + 1)):
                    raise ValueError("ngram count line")
                declared.append(int(w[1].split("=", 1)[1]))
                continue
            if len(w) not in (k + 1, k + 2):
                raise ValueError("fields")
            lp = np.float32(float(w[0]) * LN10)
            bo = np.float32(float(w[k + 1]) * LN10) if len(w) == k + 2 else None
            seen += 1
            ws = [id_of.get(x, -1) for x in w[1:k + 1]]
            if any(i < 1 for i in ws):
                dropped += 1
                continue
            ngrams[tuple(ws)] = (lp, bo)
    if not ended or not declared:
        raise ValueError("truncated")

    def special(sp):
        return id_of[sp] if id_of.get(sp, -1) >= 1 else -1
    unk = special("<unk>")
    if unk >= 0 and (unk,) not in ngrams:
        unk = -1
    return len(declared), ngrams, dropped, special("<s>"), special("</s>"), unk, transparent


# ---- the LM recipe of the case tables (ctcbeam_ref.CPU_CASES / GPU_CASES) ---------------------------------------------------
WEIGHTS = ((0.5, 0.0), (0.3, 1.0), (1.0, -0.5))


def case_lm(case, order=3):
    """Deterministic per case, from default_rng(seed + 11): every id in [1, V) but one (V - 1 when V > 4: it stays out of the
    unigrams) is a unigram with logp in [-4, -0.5] and a back-off in [-1, 0]; the 2- and 3-grams of the unfused definition's
    first four hypotheses are listed, and 3 V random 2-grams and 3-grams more (some without their prefix context, as pruned
    models have them; every fourth bigram without a back-off).  bos = 1, eos = 2 when V > 5.  For the "mirror" inputs (columns
    2 / 4 copies of 1 / 3) every n-gram is listed in all of its mirrored spellings with the same weights, so the LM scores the
    mirrored ids alike."""
    _name, seed, _T, V, _K, _W, kind = case
    rng = np.random.default_rng(seed + 11)
    mirror = {1: 2, 2: 1, 3: 4, 4: 3} if kind == "mirror" else {}
    canon = (lambda c: min(c, mirror.get(c, c)))
    skip = V - 1 if V > 4 else -1
    grams = {}

    def add(w, lp, bo):
        w = tuple(canon(int(c)) for c in w)
        if skip in w or w in grams:
            return
        grams[w] = (np.float32(lp), None if bo is None else np.float32(bo))

    for c in range(1, V):
        add((c,), rng.uniform(-4.0, -0.5), rng.uniform(-1.0, 0.0))
    ref = R.case_reference(case)
    for y, _s in ref.hyps[:4]:
        for k in (2, 3)[:order - 1]:
            for p in range(len(y) - k + 1):
                add(y[p:p + k], rng.uniform(-2.0, -0.1), rng.uniform(-0.7, 0.0))
    for x in range(3 * V):
        k = 2 + (x % 2) if order >= 3 else min(2, order)
        if k > order or k < 2:
            break
        add(rng.integers(1, V, k), rng.uniform(-3.0, -0.2), None if x % 4 == 0 else rng.uniform(-0.7, 0.0))
    out = {}
    for w, v in grams.items():                      # all mirrored spellings
        spell = [()]
        for c in w:
            spell = [sp + (d,) for sp in spell for d in sorted({c, mirror.get(c, c)})]
        for sp in spell:
            out[sp] = v
    big = V > 5
    return Model(order, out, V, bos=1 if big else -1, eos=2 if big else -1, oov=-7.5)


_cache = {}


def case_reference(case, alpha, beta, flags=0, with_hot=False, T=None):
    """The fused definition's result for a table entry (its first T frames), computed once per process; with_hot: together with
    ctcbeam_bias_ref's hot-word recipe at its boost."""
    key = (case, f32(alpha), f32(beta), flags, with_hot, T)
    if key not in _cache:
        lb, ids, val, n = R.case_arrays(case)
        TT = lb.shape[0] if T is None else T
        hot = BR.case_hotwords(case) if with_hot else ()
        _cache[key] = beam_search(lb[:TT], ids[:TT], val[:TT], n[:TT], case[5], case_lm(case), alpha, beta, flags, hot,
                                  BR.RECIPE_BOOST if with_hot else 0.0)
    return _cache[key]


# ---- the arc-list edge table (tests/test_ctcbeam_lm_cpu.py, tests/test_gpu_lm.py) --------------------------------------------
EDGE_V = 25055
EDGE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 4097)
_edge = []


def edge_model():
    """(Model, probes): an order-3 model over V = 25 055 in which every id is a unigram, the context (100 + k) has an arc list of
    EDGE_SIZES[k] bigrams and the context (100 + k, its first arc) one of as many trigrams, over tokens 1000 + 3 j + (0 | 1) —
    so between any two arcs lies an id that is none.  probes: sequences that end at every arc of every list, and per list at an
    id between two arcs, below the first and above the last (those back off)."""
    if _edge:
        return _edge[0]
    rng = np.random.default_rng(2024)
    grams = {}
    lp = rng.uniform(-9.0, -1.0, EDGE_V).astype(np.float32)
    bo = rng.uniform(-1.0, 0.0, EDGE_V).astype(np.float32)
    for c in range(1, EDGE_V):
        grams[(c,)] = (lp[c], bo[c])
    probes = []
    for k, size in enumerate(EDGE_SIZES):
        a = 100 + k
        toks = [1000 + 3 * j + int(x) for j, x in enumerate(rng.integers(0, 2, size))]
        for ctx in ((a,), (a, toks[0])):
            for t in toks:
                w = ctx + (t,)
                if w not in grams:
                    grams[w] = (np.float32(rng.uniform(-5.0, -0.1)), np.float32(rng.uniform(-0.5, 0.0)) if len(w) < 3 else None)
            miss = [toks[0] - 1, toks[-1] + 1] + ([toks[0] + 1 if toks[0] + 1 != toks[1] else toks[0] + 2] if size > 1 else [])
            assert all(ctx + (m,) not in grams and 1 <= m < EDGE_V for m in miss)
            probes += [ctx + (t,) for t in toks] + [ctx + (m,) for m in miss]
    _edge.append((Model(3, grams, EDGE_V, oov=-20.0), probes))
    return _edge[0]


# ---- a model too large for the caches, by formula (tests/test_gpu_ctcbeam_lm.py; its gap condition: the CPU suite) -----------------
BIG_V = 25055
BIG_LOW = 14          # contexts are made of the ids below it: the ids of the GPU_CASES inputs at V = 14


def _big_weight(w, salt):
    h = sum(int(c) * m for c, m in zip(w, (7919, 104729, 1299709))) + salt
    return np.float32(-0.25 - (h % 4096) / 1024.0)


class _BigGrams:
    """{n-gram: value} without storing one: every id is a unigram; (a, b) is listed when a < BIG_LOW and b % 3 != 0; (a, b, c) when
    a, b < BIG_LOW and c % 4 != 0.  Unigrams and bigrams carry a back-off."""

    def __init__(self, salt, longest):
        self.salt, self.longest = salt, longest

    def __contains__(self, w):
        if len(w) > self.longest or not all(1 <= c < BIG_V for c in w):
            return False
        if len(w) == 1:
            return True
        if len(w) == 2:
            return w[0] < BIG_LOW and w[1] % 3 != 0
        return len(w) == 3 and w[0] < BIG_LOW and w[1] < BIG_LOW and w[2] % 4 != 0

    def __getitem__(self, w):
        return float(_big_weight(w, self.salt))


def big_model():
    """An order-3 Model over V = 25 055 with some 3.4 million n-grams (an image above 32 MB), bos = 1, eos = 2."""
    m = Model(1, {}, BIG_V, bos=1, eos=2, oov=-9.0)
    m.order = 3
    m.logp, m.bo = _BigGrams(0, 3), _BigGrams(17, 2)
    return m


def big_model_arrays():
    """big_model() as the builder's arrays: (counts [3], ids, logp, backoff)."""
    def weights(cols, salt):
        h = sum(c.astype(np.int64) * k for c, k in zip(cols, (7919, 104729, 1299709))) + salt
        return (-0.25 - (h % 4096) / 1024.0).astype(np.float32)
    a1 = np.arange(1, BIG_V, dtype=np.int32)
    low = np.arange(1, BIG_LOW, dtype=np.int32)
    b2 = a1[a1 % 3 != 0]
    c3 = a1[a1 % 4 != 0]
    g2 = np.stack(np.meshgrid(low, b2, indexing="ij"), -1).reshape(-1, 2)
    g3 = np.stack(np.meshgrid(low, low, c3, indexing="ij"), -1).reshape(-1, 3)
    ids = np.concatenate([a1, g2.ravel(), g3.ravel()]).astype(np.int32)
    logp = np.concatenate([weights([a1], 0), weights(list(g2.T), 0), weights(list(g3.T), 0)])
    bo = np.concatenate([weights([a1], 17), weights(list(g2.T), 17), np.full(len(g3), np.nan, np.float32)])
    return [len(a1), len(g2), len(g3)], ids, logp, bo


def write_arpa(path, order, ngrams, tokens):
    """{n-gram: (natural-log logp, back-off or None)} as ARPA text (log10 values, 9 significant digits, tab after the value) with
    the words of `tokens`.  Read it back with read_arpa for the model the text holds: its float32 weights are those of the text."""
    lines = ["\\data\\"] + ["ngram %d=%d" % (k, sum(len(w) == k for w in ngrams)) for k in range(1, order + 1)] + [""]
    for k in range(1, order + 1):
        lines.append("\\%d-grams:" % k)
        for w in sorted(x for x in ngrams if len(x) == k):
            lp, bo = ngrams[w]
            lines.append("%.9g\t%s%s" % (float(lp) / LN10, " ".join(tokens[c] for c in w), "" if bo is None or k == order else "\t%.9g" % (float(bo) / LN10)))
        lines.append("")
    lines.append("\\end\\")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
