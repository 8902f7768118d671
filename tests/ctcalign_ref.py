"""The definition of CTC forced alignment (PF_DECODE_ALIGN) in numpy: the contract the device kernel
(csrc/k_ctcalign.hip) and the host twin (host_ctc_align, csrc/hostutil.cpp) are compared with.

Inputs of one job: log-prob rows lp [T, V] float32 (the rows t < n_b of an utterance), a target y [U] of non-blank ids in
[1, V); the blank is id 0.  States s in [0, S), S = 2U + 1; lab(s) = blank for even s, y[s // 2] for odd s.

Best path (float32, one add per cell, in frame order):
    a[0][0] = lp[0][0], a[0][1] = lp[0][y[0]], every other state -inf
    a[t][s] = fl32(best + lp[t][lab(s)]),  best among a[t-1][s], a[t-1][s-1] and, for odd s with lab(s) != lab(s-2),
              a[t-1][s-2]: tried in that order with a strict >, so of equal values the LARGER state wins
    end state S-1 unless a[T-1][S-2] > a[T-1][S-1]
Float addition is monotone, so the score equals the best sequentially-summed score over all valid alignments
(`brute`), bit for bit.

Per token u: first[u] / last[u] = first / last frame of the path in state 2u+1, tok_score[u] = the float32 maximum of
lp[t][y[u]] over that run.

Log-likelihood (float64): the same recursion with lse(a, b) = max + log1p(exp(-|a - b|)) (-inf operands passed through) in
place of max, in the order ((stay (+) s-1) (+) s-2) + lp; the end is lse(a[S-1], a[S-2]).  Comparison rule for another
implementation: |x - ref| <= 16 * T * 2^-53 * max(1, |ref|) — a cell does two lse and one add per frame; an lse is one
subtraction, exp and log1p (each within 2 ulp) and one add, so 2 * (1 + 2 + 2 + 1) = 12 roundings, plus the add: 13,
bounded by 16 per frame.

Not ok = not (path_score > -inf): U > T, too few frames for the repeats, T = 0 with U > 0, a NaN on every path.  Then
ok = 0, first / last hold -1, tok_score 0, path_score / loglik whatever the recursion gives.  U = 0 is the all-blank path;
T = 0 with U = 0 is ok with score 0."""
import itertools
import math

import numpy as np

F32 = np.float32
NEG = F32(-np.inf)
MAX_TOKENS = 1023
ROUNDINGS_PER_FRAME = 16


def lse(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = a if a > b else b
    return m + math.log1p(math.exp(-abs(a - b)))


def _lse_v(a, b):
    m = np.where(a > b, a, b)
    return np.where(a == -np.inf, b, np.where(b == -np.inf, a, m + np.log1p(np.exp(-np.abs(a - b)))))


def loglik_tol(T, s):
    return ROUNDINGS_PER_FRAME * max(T, 1) * 2.0 ** -53 * max(1.0, abs(s))


def min_frames(y):
    """the fewest frames a target can be aligned to: one per token and one blank between equal neighbours"""
    return len(y) + sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


class Alignment:
    def __init__(self, path_score, loglik, ok, first, last, tok_score, path):
        self.path_score, self.loglik, self.ok = path_score, loglik, ok
        self.first, self.last, self.tok_score, self.path = first, last, tok_score, path


def align(lp, y, blank=0):
    """lp [T, V] float32, y: U ids -> Alignment (first / last int32 [U], tok_score float32 [U], path: states per frame)"""
    lp = np.asarray(lp, dtype=F32)
    T = lp.shape[0]
    y = [int(v) for v in y]
    U = len(y)
    S = 2 * U + 1
    lab = [blank if s % 2 == 0 else y[s // 2] for s in range(S)]
    first = np.full(U, -1, np.int32)
    last = np.full(U, -1, np.int32)
    tok = np.zeros(U, F32)
    if T == 0:
        if U == 0:
            return Alignment(F32(0), 0.0, 1, first, last, tok, [])
        return Alignment(NEG, -math.inf, 0, first, last, tok, None)
    a = np.full(S, NEG, F32)
    d = np.full(S, -np.inf, np.float64)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, lab[1]]
    d[:2] = a[:2]
    labs = np.asarray(lab, np.int64)
    skip = np.zeros(S, bool)
    skip[3::2] = labs[3::2] != labs[1:-2:2]
    bp = np.zeros((T, S), np.int8)
    with np.errstate(all="ignore"):
        for t in range(1, T):                      # every state of a frame at once; per state exactly the steps above
            v = lp[t, labs]
            p1 = np.concatenate(([NEG], a[:-1]))[:S]
            p2 = np.concatenate(([NEG, NEG], a[:-2]))[:S]
            best, m = a.copy(), np.zeros(S, np.int8)
            w = p1 > best
            best[w], m[w] = p1[w], 1
            w = skip & (p2 > best)
            best[w], m[w] = p2[w], 2
            a = (best + v).astype(F32)
            bp[t] = m
            q1 = np.concatenate(([-np.inf], d[:-1]))[:S]
            q2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], d[:-2]))[:S], -np.inf)
            d = _lse_v(_lse_v(d, q1), q2) + v.astype(np.float64)
    d = [float(x) for x in d]
    s = S - 1
    if S > 1 and a[S - 2] > a[S - 1]:
        s = S - 2
    score = a[s]
    ll = lse(d[S - 1], d[S - 2]) if S > 1 else d[0]
    if not score > NEG:
        return Alignment(score, ll, 0, first, last, tok, None)
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(bp[t, s])
    for t, s in enumerate(path):
        if s % 2:
            u = s // 2
            v = lp[t, y[u]]
            if first[u] < 0:
                first[u] = t
                tok[u] = v
            else:
                tok[u] = v if v > tok[u] else tok[u]          # fmaxf; no NaN on an ok path
            last[u] = t
    return Alignment(score, ll, 1, first, last, tok, path)


def brute(lp, y, blank=0):
    """(best sequentially-summed float32 score, every path that reaches it, float64 log of the summed alignments)"""
    lp = np.asarray(lp, dtype=F32)
    T = lp.shape[0]
    y = [int(v) for v in y]
    S = 2 * len(y) + 1
    lab = [blank if s % 2 == 0 else y[s // 2] for s in range(S)]
    best, paths, total = NEG, [], []
    for p in itertools.product(range(S), repeat=T):
        if p[0] > 1 or p[-1] < S - 2:
            continue
        ok = True
        for t in range(1, T):
            dd = p[t] - p[t - 1]
            if dd < 0 or dd > 2 or (dd == 2 and (p[t] % 2 == 0 or lab[p[t]] == lab[p[t] - 2])):
                ok = False
                break
        if not ok:
            continue
        sc = F32(lp[0, lab[p[0]]])
        for t in range(1, T):
            sc = F32(sc + lp[t, lab[p[t]]])
        total.append(sum(float(lp[t, lab[p[t]]]) for t in range(T)))
        if sc > best:
            best, paths = sc, [p]
        elif sc == best and sc > NEG:
            paths.append(p)
    ll = -math.inf
    if total:
        m = max(total)
        ll = m if m == -math.inf else m + math.log(sum(math.exp(x - m) for x in total))
    return best, paths, ll


def random_case(rng, T, V, U):
    x = rng.standard_normal((T, V)).astype(F32)
    lp = (x - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True))).astype(F32)
    return lp, [int(v) for v in rng.integers(1, V, U)]


def tie_case(rng, T, V, U):
    """integer-valued log-probs: every sum is exact, so equal scores are exact ties (no mirrored columns needed)"""
    return -rng.integers(1, 3, (T, V)).astype(F32), [int(v) for v in rng.integers(1, V, U)]


def check_against_brute(n_random=400, n_ties=400, seed=0):
    """The three assertions of the definition; returns (cases with one optimum, tie cases with several optima)."""
    rng = np.random.default_rng(seed)
    unique = multi = 0
    for _ in range(n_random):
        T, V, U = int(rng.integers(1, 7)), int(rng.integers(2, 5)), int(rng.integers(0, 4))
        lp, y = random_case(rng, T, V, U)
        r = align(lp, y)
        b, ps, ll = brute(lp, y)
        assert F32(r.path_score).tobytes() == F32(b).tobytes(), (lp, y)             # 1. score bits, always
        if r.ok:
            if len(ps) == 1:                                                        # 2. the path where it is unique
                unique += 1
                assert tuple(r.path) == ps[0], (lp, y)
            assert abs(r.loglik - ll) <= 1e-9 * max(1.0, abs(ll))
        else:
            assert not ps and ll == -math.inf and r.loglik == -math.inf
    for _ in range(n_ties):
        T, V, U = int(rng.integers(1, 7)), int(rng.integers(2, 4)), int(rng.integers(0, 4))
        lp, y = tie_case(rng, T, V, U)
        r = align(lp, y)
        b, ps, _ = brute(lp, y)
        assert F32(r.path_score).tobytes() == F32(b).tobytes(), (lp, y)
        if r.ok:
            multi += len(ps) > 1
            want = max(ps, key=lambda p: tuple(reversed(p)))                        # 3. largest from the last frame backwards
            assert tuple(r.path) == want, (lp, y)
        else:
            assert not ps
    return unique, multi
