"""The CIF conformance suite's inputs and its float64 tier (tests/test_cif_ref_cpu.py, tests/test_gpu_cif_conformance.py).

Pure numpy; imports neither the engine nor oracle.model.  Four parts:

  cases()            the case table: named alpha matrices [B, T+1] float32 by family (random, dyadic, near-tie, inexact, threshold),
                     each with a one-hot hidden state when T <= 129
  cumsum_walk()      a numpy restatement of cif_scan_cumsum_kernel's chunked TwoSum walk: does any of its float64 additions round,
                     and which fire table would the walk arrive at on its own?
  check_weights() / fire_frames() / float64_crossings()
                     the float64 tier: what integrate-and-fire means, stated from the definition on the weight matrix W[l, t] = "how
                     much of frame t went into token l", with bounds derived from the arithmetic (below)
  alpha_ref()        the predictor's alpha stage (conv over time + ReLU, output projection, sigmoid, smooth / noise clip) in a chosen
                     precision, operands rounded as the engine rounds them

One-hot hidden states.  With H[b, t, c] = (c == t) and D = round_up(T, 4) every product in both gather kernels is alpha * 1 or
alpha * 0 and every sum has at most one non-zero addend per channel, so E[b, l, t] IS the weight of frame t in token l — the whole fire
table read through op_cif as it is.  The tail frame T has a zero hidden state: its weight is not visible, which is why the row rule below
speaks of tokens "whose fire frame is not the tail frame".

Bounds of the float64 tier (u = 2^-24, the unit round-off of float32 below 2; ulp32(x) = the float32 spacing at x):

  rows, sequential.  Token l takes rem (left over from the previous fire frame), then whole alphas, then completion = fl(1 - I) at
      its fire frame, I being the running float32 integrate.  I differs from the exact sum rem + sum(alpha) by at most one rounding
      per addition, each below u because I < 2: n additions for n frames.  Two more roundings: completion itself, and
      rem = fl(alpha - completion) against the integrate the kernel carries on, fl(I + alpha) - 1.  |sum(row) - 1| <= (n + 2) u.
  rows, cumsum.  The row is remain[f'] + alphas + (alpha[f] - remain[f]) with remain = fl(fl(1 + frac) - 1), frac = p32 - floor(p32),
      p32 = fl32(float64 prefix).  p32 is off by at most ulp32(p)/2 at each end of the token; fl(1 + frac) rounds by at most u at each
      end; fl(alpha - remain) by at most u.  |sum(row) - 1| <= ulp32(max(p[f], 1)) + 3 u  (p grows, so the fire frame's ulp covers both).
  columns.  A fire frame's weight is split as w + fl(alpha - w): one rounding of a value no larger than alpha, so
      |sum(column) - alpha| <= u * alpha; every other frame's weight is alpha itself.
  fire decisions.  The sequential chain's integrate is off the exact prefix by at most (T+1) u; an utterance is compared with the
      float64 crossings when every prefix is further than 2 (T+1) u from every integer.  The prefix-sum rule decides on
      fl32(float64 prefix): off by at most ulp32(total)/2, compared when every prefix is further than ulp32(total) from every integer.
"""
import collections
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
TAIL = F32(0.45)

Case = collections.namedtuple("Case", "name family alphas H what threshold")

RANDOM_T1 = (2, 3, 9, 63, 64, 65, 127, 128, 129, 301, 1025)
NEAR_TIE_WEIGHTS = (0.1, 0.2, 0.3, 0.7, 0.9, 0.01, 0.126)
NEAR_TIE_T1 = (10, 50, 100, 200, 500)
# (weight, T+1) -> (sequential fires, token_num, cumsum fires), computed from the oracle alone
NEAR_TIE_ANCHORS = {(0.1, 50): (5, 4, 5), (0.3, 100): (30, 29, 30), (0.7, 50): (34, 35, 35), (0.9, 200): (179, 179, 180),
                    (0.01, 200): (1, 1, 2)}
INEXACT_T1 = (65, 129, 501)
INEXACT_SCALES = (1e-9, 1e-30)
SEED = 20


def round_up(n, m):
    return (n + m - 1) // m * m


def _frozen(a):
    a.flags.writeable = False
    return a


def one_hot_hidden(B, T):
    """H[b, t, c] = (c == t), D = round_up(T, 4)"""
    H = np.zeros((B, T, round_up(T, 4)), F32)
    H[:, np.arange(T), np.arange(T)] = 1.0
    return _frozen(H)


def _random_alphas(rng, B, T1):
    a = rng.uniform(0.0, 0.7, (B, T1)).astype(F32)
    a[:, -1] = TAIL
    return a


def _case(name, family, alphas, what, threshold=1.0):
    a = _frozen(np.ascontiguousarray(alphas, dtype=F32))
    B, T1 = a.shape
    H = one_hot_hidden(B, T1 - 1) if 1 <= T1 - 1 <= 129 else None
    return Case(name, family, a, H, what, threshold)


DYADIC_HAND = np.asarray([[.5, .5, .25, .25, .25, .25, 1, 0, .75, .25, .45]], F32)
DYADIC_HAND_FIRES = (1, 5, 6, 9)
DYADIC_HAND_ROWS = ({0: .5, 1: .5}, {2: .25, 3: .25, 4: .25, 5: .25}, {6: 1.0}, {8: .75, 9: .25})


# 1 + (1 - 2^-23) + (2^-24 - 2^-28) + (2^-28 - 2^-52) = 2 - 2^-24 - 2^-52 exactly in float64: one float64 ulp below 2 - 2^-24, the
# midpoint between the float32 neighbours 2 - 2^-23 and 2.0.  Every weight is a float32.  Sequentially each following 2^-54 is a
# quarter ulp and is rounded away: float32(prefix) stays 2 - 2^-23 and the second fire comes on the tail.  Summed in any other
# order the four make 2^-52, the prefix reaches the midpoint and rounds (to even) to 2.0 on one of those frames.  On the random
# inexact cases a re-associated sum differs from the sequential one too, by 1e-16 — which float32(prefix) never shows; here it does.
INEXACT_MIDPOINT = np.asarray([[1.0, 1 - 2.0 ** -23, 2.0 ** -24 - 2.0 ** -28, 2.0 ** -28 - 2.0 ** -52,
                                2.0 ** -54, 2.0 ** -54, 2.0 ** -54, 2.0 ** -54, TAIL]], F32)


@functools.lru_cache(maxsize=None)
def cases():
    """the whole table, built once; every array is read-only"""
    out = []
    rng = np.random.default_rng(SEED)
    for T1 in RANDOM_T1:
        out.append(_case("random_T1_%d" % T1, "random", _random_alphas(rng, 4 if T1 == 1025 else 3, T1),
                         "uniform(0, 0.7) weights with the 0.45 tail; T+1 around the 64-lane chunking of the cumsum scan"))
    a = _random_alphas(rng, 4, 200)
    a[0, :150] = 0.0                                   # long silence
    a[1, :] = 0.0                                      # nothing at all: fire_count 0
    a[2, :-1] = rng.uniform(0.55, 0.7, 199).astype(F32)   # dense
    out.append(_case("random_ragged", "random", a, "ragged batch: a long silence, an all-zero row, a dense row, a plain row"))

    out.append(_case("dyadic_hand", "dyadic", DYADIC_HAND, "fires at frames 1, 5, 6, 9 with known weight rows; every sum exact"))
    out.append(_case("dyadic_ones", "dyadic", np.ones((1, 33), F32), "a fire on every frame, the tail included; integrate == threshold every time"))
    out.append(_case("dyadic_zeros", "dyadic", np.zeros((2, 17), F32), "no fire, L = 0"))
    out.append(_case("dyadic_single_frame", "dyadic", np.asarray([[.75, .25]], F32), "T = 1: the only fire is on the tail frame and lands on 1.0"))
    out.append(_case("dyadic_tail_only", "dyadic", np.asarray([[.125, .125, .25, 0, .125, .5]], F32),
                     "0.625 before the tail, 0.5 on it: one fire, on the tail frame"))

    for T1 in NEAR_TIE_T1:
        a = np.stack([np.full(T1, w, F32) for w in NEAR_TIE_WEIGHTS])
        out.append(_case("near_tie_T1_%d" % T1, "near_tie", a,
                         "constant weights %s: float32 chains within an ulp of an integer" % (NEAR_TIE_WEIGHTS,)))

    rng = np.random.default_rng(SEED + 1)
    for T1 in INEXACT_T1:
        base = _random_alphas(rng, 3, T1)
        for s in INEXACT_SCALES:
            a = base.copy()
            a[:, ::7] = (a[:, ::7] * F32(s)).astype(F32)
            a[:, -1] = TAIL
            out.append(_case("inexact_T1_%d_x%g" % (T1, s), "inexact", a,
                             "every 7th weight x %g: a float64 addition rounds, the cumsum scan redoes the utterance sequentially" % s))

    out.append(_case("inexact_midpoint", "inexact", INEXACT_MIDPOINT,
                     "the float64 prefix one ulp under the float32 midpoint below 2.0, then four weights of a quarter ulp: the "
                     "sequential sum absorbs each, a re-associated sum gathers them, reaches the midpoint and rounds to 2.0 early"))

    rng = np.random.default_rng(SEED + 2)
    out.append(_case("threshold_0.9", "threshold", _random_alphas(rng, 2, 70), "sequential rule at threshold 0.9", threshold=0.9))
    return tuple(out)


def family(name):
    return [c for c in cases() if c.family == name]


def random_hidden(case, D, seed=0):
    B, T1 = case.alphas.shape
    rng = np.random.default_rng([seed, B, T1, D])
    return rng.standard_normal((B, T1 - 1, D), dtype=np.float32)


# ------------------------------------------------------------------ the cumsum scan's chunked walk
def _two_sum(a, b):
    """Knuth's TwoSum on Python floats (IEEE double): the rounded sum and whether it rounded"""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return s, err != 0.0


def cumsum_walk(alphas_row):
    """cif_scan_cumsum_kernel's additions for one utterance, in its order: lane i of 64 owns the chunk [i c, (i+1) c) of
    c = ceil((T+1) / 64) weights and sums it in double; the 64 totals go through a Hillis-Steele inclusive scan; every lane walks
    its chunk again from its exclusive offset, deciding fires on floor(float32(running sum)) against the floor before it (the
    floor of its offset at the chunk's start).  Returns (whether any of these additions was inexact — the kernel then redoes the
    utterance sequentially on lane 0 —, the fire frames this walk itself arrives at)."""
    a = [float(x) for x in np.asarray(alphas_row, F32)]
    T1 = len(a)
    c = (T1 + 63) // 64
    lo = [min(i * c, T1) for i in range(64)]
    hi = [min(l + c, T1) for l in lo]
    inexact = False
    inc = []
    for i in range(64):
        tot = 0.0
        for t in range(lo[i], hi[i]):
            tot, r = _two_sum(tot, a[t])
            inexact |= r
        inc.append(tot)
    o = 1
    while o < 64:
        nxt = list(inc)
        for i in range(o, 64):
            nxt[i], r = _two_sum(inc[i - o], inc[i])
            inexact |= r
        inc = nxt
        o <<= 1
    fires = []
    for i in range(64):
        run = inc[i - 1] if i else 0.0
        prev = 0.0 if lo[i] == 0 else float(np.floor(F32(run)))
        for t in range(lo[i], hi[i]):
            run, r = _two_sum(run, a[t])
            inexact |= r
            fl = float(np.floor(F32(run)))
            if fl - prev > 0:
                fires.append(t)
            prev = fl
    return inexact, fires


def cumsum_walk_inexact(alphas_row):
    return cumsum_walk(alphas_row)[0]


def sequential_prefix_fires(alphas_row):
    """the prefix-sum rule on the sequential float64 running sum (ONNX CumSum), the definition the kernel's redo restates"""
    p = np.cumsum(np.asarray(alphas_row, F32).astype(np.float64)).astype(F32)
    fl = np.floor(p)
    return [int(t) for t in np.flatnonzero(fl - np.concatenate([[F32(0)], fl[:-1]]) > 0)]


# ------------------------------------------------------------------ the float64 tier
def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def weight_matrix(E_b, count, T):
    """W[l, t] of one utterance from its one-hot embeds E_b [L, D]: the first `count` rows, the T frame columns.  Everything else
    (rows >= count, the D - T padding channels) must be exactly zero."""
    E_b = np.asarray(E_b)
    assert not E_b[count:].any(), "rows l >= fire_count are not zero"
    assert not E_b[:, T:].any(), "a padding channel received weight"
    return E_b[:count, :T].astype(np.float64)


def row_bound(variant, n_frames, prefix_at_fire):
    if variant == "cumsum":
        return ulp32(max(prefix_at_fire, 1.0)) + 3 * U
    return (n_frames + 2) * U


def fire_frames(W, alphas_row, variant):
    """Fire frame of every token from W alone (the tail frame T for a token completed on the invisible tail frame).  Rows 0 .. n-2
    end on their last non-zero column: a fire frame always keeps a strictly positive share (the distance to the integer).  The last
    row ends there too when its weights already sum to 1 within the row bound; otherwise, or when it has no visible weight, the
    tail completed it."""
    n, T = W.shape
    p = np.cumsum(np.asarray(alphas_row, np.float64))
    ff = []
    for l in range(n):
        nz = np.flatnonzero(W[l])
        if l < n - 1:
            assert nz.size, "token %d of %d has no weight" % (l, n)
            ff.append(int(nz[-1]))
            continue
        if not nz.size:
            ff.append(T)
            continue
        c = int(nz[-1])
        first = ff[-1] if ff else 0
        ff.append(c if abs(W[l].sum() - 1.0) <= row_bound(variant, c - first + 1, p[c]) else T)
    return ff


def check_weights(W, alphas_row, variant, threshold=1.0):
    """rows, columns and monotonicity of one utterance's weight matrix; returns (fire frames, largest row error, largest column
    error relative to u * alpha).  threshold 1 only for the row rule's "sums to 1" (the table's threshold case has no one-hot run)."""
    assert threshold == 1.0
    a = np.asarray(alphas_row, np.float64)
    n, T = W.shape
    p = np.cumsum(a)
    ff = fire_frames(W, alphas_row, variant)
    assert all(x < y for x, y in zip(ff, ff[1:])), ("fire frames not strictly increasing", ff)
    assert (W >= 0).all()
    row_err = 0.0
    for l in range(n):
        if ff[l] >= T:
            continue                                            # completed on the tail frame: its share is not visible
        first = ff[l - 1] if l else 0
        err = abs(W[l].sum() - 1.0)
        bound = row_bound(variant, ff[l] - first + 1, p[ff[l]])
        assert err <= bound, ("row", l, err, bound)
        row_err = max(row_err, err)
        assert not W[l, ff[l] + 1:].any() and not W[l, :first].any(), ("weight outside the token's frames", l)
    # columns: complete up to the last fire (what follows it never reached a token and is dropped)
    last = ff[-1] if n else -1
    col_err = 0.0
    for t in range(T):
        nz = np.flatnonzero(W[:, t])
        assert nz.size <= 2 and (nz.size < 2 or nz[1] == nz[0] + 1), ("column", t, nz)
        if t > last:
            assert not nz.size, ("weight behind the last fire", t)
        elif t < last:
            err = abs(W[:, t].sum() - a[t])
            assert err <= U * a[t], ("column", t, err, U * a[t])
            if a[t] > 0:
                col_err = max(col_err, err / (U * a[t]))
    return ff, row_err, col_err


def float64_crossings(alphas_row, variant):
    """(fire frames by the definition in float64: floor(prefix[t]) > floor(prefix[t-1]), whether the utterance is decidable: every
    prefix further from every integer than the float32 error of the rule, see the module docstring).  Weights below 1 only."""
    a = np.asarray(alphas_row, np.float64)
    T1 = a.size
    p = np.cumsum(a)
    fl = np.floor(p)
    prev = np.concatenate([[0.0], fl[:-1]])
    fires = [int(t) for t in np.flatnonzero(fl > prev)]
    eps = ulp32(max(p[-1], 1.0)) if variant == "cumsum" else 2.0 * T1 * U
    dist = np.abs(p - np.rint(p))
    live = p > 0.5                                              # a fire is a crossing of 1, 2, ...: the integer 0 decides nothing
    return fires, bool((dist[live] > eps).all())


# ------------------------------------------------------------------ the predictor's alpha stage
def _h16(x):
    return np.asarray(x, F32).astype(np.float16).astype(F32)


def alpha_ref(H, w, cfg, dtype, operands):
    """alphas [B, T+1] in `dtype` arithmetic (float32: every product and sum rounded, each sum accumulated in ascending index
    order — the plain definition of the sum).  operands "f16": H and the conv weight rounded to f16 first, as math_mode 0 holds them
    (the conv bias, the output projection and everything behind the GEMM stay fp32); "exact": as given (the fp32 graph).
      y[b, t, o] = relu(bias[o] + sum_j sum_c Wc[o, c, j] * Hpad[b, t + j - l, c]),  Hpad zero outside [0, T)
      alpha = relu(sigmoid(y . w_out + b_out) * smooth - noise);  alphas[b, T] = tail (float32, as stored)
    Also returns z = y . w_out + b_out."""
    H = np.asarray(H, F32)
    B, T, D = H.shape
    l, r = cfg["cif_l_order"], cfg["cif_r_order"]
    Wc, bc = w["predictor.conv.weight"], w["predictor.conv.bias"]
    if operands == "f16":
        H, Wc = _h16(H), _h16(Wc)
    taps = l + r + 1
    Hp = np.zeros((B, T + l + r, D), dtype)
    Hp[:, l:l + T] = H
    acc = np.zeros((B, T, D), dtype)
    for j in range(taps):
        Wj = Wc[:, :, j].astype(dtype)                          # [o, c]
        for c in range(D):
            acc = acc + Hp[:, j:j + T, c, None] * Wj[None, None, :, c]
    y = np.maximum(acc + bc.astype(dtype), dtype(0))
    wo = w["predictor.out.weight"].reshape(-1).astype(dtype)
    z = np.zeros((B, T), dtype)
    for c in range(D):
        z = z + y[:, :, c] * wo[c]
    z = z + dtype(w["predictor.out.bias"].reshape(-1)[0])
    with np.errstate(over="ignore"):
        s = dtype(1) / (dtype(1) + np.exp(-z))
    a = np.maximum(s * dtype(cfg["cif_smooth"]) - dtype(cfg["cif_noise"]), dtype(0))
    out = np.concatenate([a, np.full((B, 1), F32(cfg["cif_tail"]), dtype)], axis=1)
    return out, z


def alpha_inputs(name, w, cfg):
    """H [B, T, 512] of the alpha-stage cases"""
    D = cfg["d_model"]
    shapes = {"b1_t1": (1, 1), "b1_t2": (1, 2), "b1_t3": (1, 3), "b3_t9": (3, 9), "b2_t83": (2, 83)}
    if name in shapes:
        B, T = shapes[name]
        return np.random.default_rng([7, B, T]).standard_normal((B, T, D), dtype=np.float32)
    if name == "contrast":
        # neighbours that differ by orders of magnitude and in sign: a frame read across the batch boundary moves alpha visibly
        rng = np.random.default_rng(8)
        H = rng.standard_normal((3, 5, D), dtype=np.float32)
        H[0] *= F32(0.01)
        H[1] = F32(8.0) * np.abs(H[1])
        H[2] = -F32(8.0) * np.abs(H[2])
        return H
    if name == "saturated":
        # H scaled by 50: one random utterance, and two that are constant in time along the directions that drive the logit down
        # and up (the conv rows of the output projection's negative / positive channels), unit RMS before the scaling
        Ws = w["predictor.conv.weight"].astype(np.float64).sum(axis=2)                  # [o, c]
        wo = w["predictor.out.weight"].reshape(-1)
        rng = np.random.default_rng(9)
        H = rng.standard_normal((3, 12, D), dtype=np.float32)
        for b, sel in ((1, wo < 0), (2, wo > 0)):
            v = Ws[sel].sum(axis=0)
            H[b] = (v / np.sqrt((v ** 2).mean())).astype(F32)[None]
        return (F32(50.0) * H).astype(F32)
    raise KeyError(name)


ALPHA_CASES = ("b1_t1", "b1_t2", "b1_t3", "b3_t9", "b2_t83", "contrast", "saturated")
# float64 logits beyond which float32 sigmoid(z) * 1 - 0 has one possible value: 1 / (1 + e^-z) rounds to 1.0 once e^-z < 2^-25
# (z > 17.4), and is below the smallest float32 subnormal once z < -104
Z_SATURATED_HIGH = 20.0
Z_SATURATED_LOW = -110.0
