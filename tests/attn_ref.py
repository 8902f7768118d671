"""numpy statement of softmax(q k^T) v per head (head dim 128, q pre-scaled) as the attention kernels implement it
(csrc/k_attn.hip, csrc/k_fp32.hip), input designs whose answer is known exactly, the error bounds and the assertion
helper — shared by tests/test_attn_ref_cpu.py (which proves on the CPU that the designs and the helper reject wrong
attentions) and tests/test_gpu_attn_conformance.py.

Kinds (pf_op_attention_ex): 0 = f16 operands and output, 1 = fp32, 2 = fp32 with the output as the (hi | lo') f16 pair.

Bounds, per output element, derived and not tuned (u16 = 2^-11, u32 = 2^-24; O the float64 result on the operands
as the kernel sees them, A = softmax(S) @ |V|):
  kind 0:   |err| <= u16 |O| + 3 u16 A + Lk u32 max_j |V_j|
            u16 |O|: the output rounding; 3 u16 A: P rounded to f16 in the numerator against the unrounded fp32 sum
            in the denominator (1 u16), plus slack for the fp32 rounding of the scores under exp; the last term: P
            below the f16 normal range (absolute error 2^-25 each) and the fp32 accumulation.
  kind 1/2: |err| <= (2 g + (Lk + 16) u32) A + 2^-22 |O|,   g = 128 u32 max_j sum_d |q_d k_jd|
            g: the worst-case rounding of a 128-term fp32 dot product, carried through exp into numerator and
            denominator; 2^-22 |O|: the 22-bit mantissa of the pair."""
import collections
import functools

import numpy as np

U16 = 2.0 ** -11
U32 = 2.0 ** -24
CANARY = 0x4D2B                     # PF_ATTN_CANARY: the 16-bit pattern of every output element nothing was stored to
DESIGNS = ("select", "uniform", "stress", "random")

# the shapes of the GPU suite: (Lq, Lk) of the cross forms, T of the self-attention forms (Lq == Lk), hotword counts
CROSS_SHAPES = ((1, 1), (31, 2), (32, 63), (33, 64), (97, 65), (128, 127), (129, 128), (160, 129), (255, 192), (256, 193),
                (257, 65), (300, 129))
SELF_T = (1, 2, 33, 64, 65, 128, 129, 193, 257)
BLOCKED_T = (77, 129)
SHARED_LK = (1, 2, 5)
GRID_SHAPES = tuple(sorted(set(CROSS_SHAPES) | {(t, t) for t in SELF_T + BLOCKED_T} | {(33, n) for n in SHARED_LK}))

AttnRef = collections.namedtuple("AttnRef", "O A smax qk_abs vmax")
Case = collections.namedtuple("Case", "design q k v heads pick exact")


def round_operands(x, kind):
    """fp32 host values -> what the kernel of this kind multiplies, as float64"""
    x = np.asarray(x, np.float32)
    return (x.astype(np.float16) if kind == 0 else x).astype(np.float64)


def attn_ref(q, k, v, heads):
    """float64 attention on operands ALREADY rounded to the kernel's operand type.  q [B, Lq, H*128], k / v [B or 1, Lk,
    H*128].  Returns AttnRef of [B, Lq, H*128] arrays: O; A = softmax(S) @ |V|; smax = max_j |S| and
    qk_abs = max_j sum_d |q_d k_jd| of the element's (batch, query, head); vmax = max_j |V_jd| of its column."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    B, Lq, Dm = q.shape
    Lk = k.shape[1]
    qh = q.reshape(B, Lq, heads, 128).transpose(0, 2, 1, 3)
    kh = np.broadcast_to(k, (B, Lk, Dm)).reshape(B, Lk, heads, 128).transpose(0, 2, 1, 3)
    vh = np.broadcast_to(v, (B, Lk, Dm)).reshape(B, Lk, heads, 128).transpose(0, 2, 1, 3)
    S = qh @ kh.transpose(0, 1, 3, 2)                                   # [B, H, Lq, Lk]
    P = np.exp(S - S.max(axis=-1, keepdims=True))
    P /= P.sum(axis=-1, keepdims=True)
    back = lambda x: x.transpose(0, 2, 1, 3).reshape(B, Lq, Dm)
    per_q = lambda x: np.repeat(x.transpose(0, 2, 1), 128, axis=2)      # [B, H, Lq] -> [B, Lq, Dm]
    qk_abs = (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)).max(axis=-1)
    vmax = np.broadcast_to(np.abs(vh).max(axis=2, keepdims=True), (B, heads, Lq, 128))
    return AttnRef(back(P @ vh), back(P @ np.abs(vh)), per_q(np.abs(S).max(axis=-1)), per_q(qk_abs), back(vmax))


def bound(ref, kind, Lk):
    if kind == 0:
        return U16 * np.abs(ref.O) + 3 * U16 * ref.A + Lk * U32 * ref.vmax
    g = 128 * U32 * ref.qk_abs
    return (2 * g + (Lk + 16) * U32) * ref.A + 2.0 ** -22 * np.abs(ref.O)


# ------------------------------------------------------------------------------------------------ designs
def code(j):
    """+-1 code of label j: its 12 bits repeated ten times, padded with +1 to 128 dims.  Two different labels below 4096
    differ in at least one bit, i.e. in at least ten dims: score 128 against itself, at most 108 against another."""
    j = np.asarray(j)
    bits = (j[..., None] >> np.arange(12)) & 1
    c = np.ones(j.shape + (128,), np.float32)
    c[..., :120] = np.tile(1.0 - 2.0 * bits, 10)
    return c


def _values(rng, shape, sign=0):
    """random f16 values with 0.25 <= |x| < 4 on the grid 2^-8 (exact in f16).  Away from zero on purpose: the exact
    answer of `select` is V[pick] + O(1e-7) and has to round to V[pick] in f16, which a value near 0 would not promise."""
    mag = rng.integers(64, 1024, shape).astype(np.float32) / 256.0
    sgn = np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0).astype(np.float32) if sign == 0 else np.float32(sign)
    return mag * sgn


def _stress_scores(rng, pattern, Lk):
    j = np.arange(Lk)
    step = 5.0 * np.log(2.0)                          # 5 log2 units per 64-key tile: the lazy max (threshold 8) skips one tile, takes the next
    if pattern == 0:
        return step * (j // 64) + rng.uniform(-0.5, 0.0, Lk)
    if pattern == 1:
        return -2.4 * step * (j // 64) + rng.uniform(-0.5, 0.0, Lk)     # 12 log2 units per tile: late P underflows in f16
    if pattern in (2, 3):
        s = rng.uniform(-1.0, 1.0, Lk)
        s[Lk - 1 if pattern == 2 else 0] = 30.0
        return s
    if pattern == 4:
        return np.full(Lk, -50.0)
    return rng.uniform(-60.0, 60.0, Lk)


@functools.lru_cache(maxsize=None)
def make_case(design, B, H, Lq, Lk, shared=False, sign=0, seed=0):
    """Seeded fp32 host inputs of one design.  pick [B, H, Lq] (select: the key each query selects) and exact
    [B, Lq, H*128] (the exact answer, float64) where the design has them, else None."""
    rng = np.random.default_rng([DESIGNS.index(design), B, H, Lq, Lk, int(shared), sign + 1, seed])
    Bk, Dm = (1 if shared else B), H * 128
    pick = exact = None
    if design == "select":
        pick = rng.integers(0, Lk, (B, H, Lq))
        pick[:, :, 0] = Lk - 1                                           # the last key, the first, the tile seam
        for i, key in ((1, 0), (2, 63), (3, 64)):
            if i < Lq and key < Lk:
                pick[:, :, i] = key
        # key j of (batch, head) carries the code of label[b, h][j], distinct labels below 4096 drawn per (batch, head): the
        # gap is that of the codes, and keys read from another batch or head no longer hold the query's winner
        label = np.stack([[rng.choice(4096, Lk, replace=False) for _ in range(H)] for _ in range(Bk)])      # [Bk, H, Lk]
        k = code(label).transpose(0, 2, 1, 3).reshape(Bk, Lk, Dm)
        q = code(np.take_along_axis(np.broadcast_to(label, (B, H, Lk)), pick, axis=2)).transpose(0, 2, 1, 3).reshape(B, Lq, Dm)
        v = _values(rng, (Bk, Lk, Dm), sign)
        vb = np.broadcast_to(v, (B, Lk, Dm)).reshape(B, Lk, H, 128)
        exact = np.stack([np.stack([vb[b, pick[b, h], h] for h in range(H)], axis=1) for b in range(B)]).reshape(B, Lq, Dm).astype(np.float64)
    elif design == "uniform":
        q = np.zeros((B, Lq, Dm), np.float32)
        k = rng.standard_normal((Bk, Lk, Dm)).astype(np.float32)
        v = rng.integers(-1, 2, (Bk, Lk, H, 128)).astype(np.float32)
        v[:, :, :, 0:4] = 0
        v[:, :, :, 0] = 1                                                # the denominator counted exactly Lk keys
        v[:, Lk - 1, :, 1] = Lk                                          # the last key: dropped -> 0, doubled -> 2 Lk / (Lk + 1)
        v[:, 0, :, 2] = Lk
        for key in (63, 64):                                             # the tile seam: 1 when one of them exists, 2 when both
            if key < Lk:
                v[:, key, :, 3] = Lk
        v = v.reshape(Bk, Lk, Dm)
        exact = np.broadcast_to(v.astype(np.float64).sum(axis=1, keepdims=True) / Lk, (B, Lq, Dm)).copy()
    elif design == "stress":
        u = np.where(rng.integers(0, 2, 128) == 1, 1.0, -1.0)
        a = np.asarray([1 / 16, 1 / 32, -1 / 16])[np.arange(Lq) % 3]     # S_ij = 128 a_i c_j
        q = np.broadcast_to((a[:, None] * u)[None, :, None, :], (B, Lq, H, 128)).reshape(B, Lq, Dm).astype(np.float32)
        c = np.stack([[_stress_scores(rng, (b * H + h + seed) % 6, Lk) / 8.0 for h in range(H)] for b in range(Bk)])   # [Bk, H, Lk]
        k = (c.transpose(0, 2, 1)[..., None] * u).reshape(Bk, Lk, Dm).astype(np.float32)
        v = rng.standard_normal((Bk, Lk, Dm)).astype(np.float32)
    else:
        q = (rng.standard_normal((B, Lq, Dm)) / np.sqrt(128) ** 0.5).astype(np.float32)
        k = (rng.standard_normal((Bk, Lk, Dm)) / np.sqrt(128) ** 0.5).astype(np.float32)
        v = rng.standard_normal((Bk, Lk, Dm)).astype(np.float32)
    for x in (q, k, v):
        x.setflags(write=False)
    return Case(design, q, k, v, H, pick, exact)


@functools.lru_cache(maxsize=None)
def case_ref(design, B, H, Lq, Lk, shared=False, sign=0, seed=0, kind=0):
    c = make_case(design, B, H, Lq, Lk, shared, sign, seed)
    return attn_ref(round_operands(c.q, kind), round_operands(c.k, kind), round_operands(c.v, kind), H)


# ------------------------------------------------------------------------------------------------ raw buffers
def f16_bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def pack_raw(out, kind, o_ld=0, store_rows=None):
    """the whole output buffer pf_op_attention_ex returns, built from an attention result `out` [B, Lq, Dm]: canary
    everywhere, then the first store_rows (default all) rows of every utterance stored"""
    B, Lq, Dm = out.shape
    ld = o_ld or Dm
    rows = B * Lq + 256
    o = np.asarray(out, np.float64).reshape(B * Lq, Dm)
    keep = (np.arange(B * Lq) % Lq) < (Lq if store_rows is None else store_rows)
    if kind == 1:
        raw = np.full((rows, ld), CANARY * 0x10001, np.uint32)
        raw[:B * Lq, :Dm][keep] = o.astype(np.float32).view(np.uint32)[keep]
        return raw
    raw = np.full((rows, 2 * ld if kind == 2 else ld), CANARY, np.uint16)
    hi = o.astype(np.float32).astype(np.float16) if kind == 2 else o.astype(np.float16)
    raw[:B * Lq, :Dm][keep] = hi.view(np.uint16)[keep]
    if kind == 2:
        lo = ((o.astype(np.float32) - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
        raw[:B * Lq, ld:ld + Dm][keep] = lo.view(np.uint16)[keep]
    return raw


def unpack_raw(raw, kind, B, Lq, Dm):
    """-> (value [B, Lq, Dm] float64 as the buffer holds it, number of words outside the valid region that are not the canary)"""
    n = B * Lq
    ld = raw.shape[1] // 2 if kind == 2 else raw.shape[1]
    assert raw.shape[0] == n + 256 and ld >= Dm
    valid = np.zeros(raw.shape, bool)
    valid[:n, :Dm] = True
    if kind == 1:
        val = raw[:n, :Dm].view(np.float32).astype(np.float64)
        touched = int((raw[~valid] != CANARY * 0x10001).sum())
    else:
        val = raw[:n, :Dm].view(np.float16).astype(np.float64)
        if kind == 2:
            valid[:n, ld:ld + Dm] = True
            val = (val.astype(np.float32) + raw[:n, ld:ld + Dm].view(np.float16).astype(np.float32) * np.float32(2.0 ** -11)).astype(np.float64)
        touched = int((raw[~valid] != CANARY).sum())
    return val.reshape(B, Lq, Dm), touched


# ------------------------------------------------------------------------------------------------ the assertion
def assert_conforms(case, ref, kind, raw, what=""):
    """The one check both suites apply to a returned buffer: nothing stored outside [B, Lq, Dm]; no NaN inside; every
    element within the bound of its kind; kind 0 additionally bit-exact on `select` and within one f16 ulp of the exact
    quotient on `uniform`.  Returns max(|err| / bound)."""
    B, Lq, Dm = case.q.shape
    Lk = case.k.shape[1]
    val, touched = unpack_raw(raw, kind, B, Lq, Dm)
    assert touched == 0, "%s: %d words outside the valid region changed" % (what, touched)
    bad = np.argwhere(~np.isfinite(val))
    assert bad.size == 0, "%s: %d non-finite outputs, first at (b, q, col) = %s" % (what, len(bad), tuple(bad[0]))
    err, bnd = np.abs(val - ref.O), bound(ref, kind, Lk)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    where = "(b, q, col) = %s (head %d): got %r, want %r" % (at, at[2] // 128, val[at], ref.O[at])
    if kind == 0 and case.design == "select":
        ne = np.argwhere(f16_bits(val) != f16_bits(case.exact))
        if ne.size:
            b, i, c = ne[0]
            raise AssertionError("%s: select: %d elements differ; first at batch %d, head %d, query %d (its key %d), column %d: got %r, want %r"
                                 % (what, len(ne), b, c // 128, i, case.pick[b, c // 128, i], c % 128, val[b, i, c], case.exact[b, i, c]))
    if kind == 0 and case.design == "uniform":
        ulp = np.spacing(np.abs(case.exact).astype(np.float16)).astype(np.float64)
        off = np.argwhere(np.abs(val - case.exact) > ulp)
        assert off.size == 0, "%s: uniform: %d elements off by more than one f16 ulp; first at %s: got %r, want %r" % (
            what, len(off), tuple(off[0]), val[tuple(off[0])], case.exact[tuple(off[0])])
    assert ratio[at] <= 1.0, "%s: |err| / bound = %.3g at %s" % (what, ratio[at], where)
    return float(ratio[at])
