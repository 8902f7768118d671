"""numpy statement of the Linear of the fp32 graph (csrc/engine_fp32.cpp Engine::gemm32): math_mode 1 on the fp32 matrix
path (k_fp32.hip gemm_f32_kernel), math_mode 3 as the "x3" product of (hi, lo') f16 operand pairs on gemm_f16_pp3<2, *> or
the short-input kernel, with the epilogue in the order csrc/kernels.h states,

    bias -> * scale (columns < scale_cols) -> + add2 (gemm32's resid2) -> + resid -> ReLU,

the operand split, input designs whose answer is known exactly, the bounds of the real-valued designs and the assertion
helpers — shared by tests/test_x3_ref_cpu.py (which proves the designs and shows that the helpers reject wrong
implementations) and tests/test_gpu_fp32_conformance.py.  f16, ln_ref, ln_bound, assert_exact and assert_bounded are
gemm_ref's.

Split.  For a finite fp32 v, |v| < 65520:  hi = f16(v) (round to nearest even), r = v - hi, lo' = f16(2048 r).  r has at most
13 significant bits and lies on v's grid, so r and 2048 r are exact in fp32: the split is a bit-exact specification.
|2048 r| <= 2^10 ulp16(hi) stays in f16's normal range while |v| >= 2^-14, where lo' then rounds r to 11 bits:
|v - (hi + lo'/2048)| <= 2^-11 |r| <= 2^-22 |hi| <= 2^-22 |v| (1 + 2^-11) — and <= 2^-22 |v| proper whenever v is not within
2^-11 of the top of a binade; the statement used below carries the factor.  Below 2^-14, hi is an f16 subnormal (a
multiple of 2^-24), |r| <= 2^-25, 2048 |r| <= 2^-14 is itself subnormal in f16 and rounds to a multiple of 2^-24: the error is
at most 2^-25 / 2048 = 2^-36.  v = 0 splits into (0, 0).

x3 product.  x W^T ~ hi_x hi_W^T + 2^-11 (hi_x lo'_W^T + lo'_x hi_W^T): every f16 x f16 product is exact in fp32, the sums are
fp32.  With v^ = hi + lo'/2048 the formula is x^ W^^T - 2^-22 lo'_x lo'_W^T.  |lo'/2048| <= 2^-11 |hi| (half an f16 ulp), so
the dropped term is at most 2^-22 |hi_x||hi_W| <= 2^-22 (1 + 2^-10) |x||W|, and with the two representation errors

    |formula - x W^T| <= 3 2^-22 (1 + 2^-10) sum |x||W|  [ + 2^-36 sum_{x != 0} |W| where hi_x may be subnormal ].

Designs (make_case asserts each design's cap, so that every partial sum fits 24 bits):

  exact22  A: 4 non-zeros per row, multiples of g = 2^-20 in (-1, 1) (2^-17 when a scale 2^-3 follows); W in {+-1, +-2}, so
           lo'_W = 0.  hi_x is a multiple of g; r is a multiple of g with |r| <= 2^-12, so lo'_x = 2048 r (a multiple of 2^-9
           below 1/2: 9 bits) is exact and hi + lo'/2048 = x.  Cross phase: multiples of 2^-9 below 4; after 2^-11: multiples of
           g; with the main phase, bias, resid and add2 (multiples of g in [-2, 2]): multiples of g below 16 = 2^24 g.  The x3
           result equals the float64 product bit for bit in any summation order and either phase order.
  both     A (8 non-zeros per row) and W (dense): +-p 2^-5 + q 2^-14, 17 <= p <= 32, |q| <= 3.  f16's ulp is >= 2^-11 from 1/2
           on and 3 2^-14 < 2^-12, so hi = +-p 2^-5 and lo' = q 2^-3 exactly (p = 16 would put v - q 2^-14 into the binade
           below, where 3 2^-14 exceeds half an ulp).  hi hi: multiples of 2^-10; hi lo' = p q 2^-8; after 2^-11: multiples of
           2^-19; sums below 32 = 2^24 2^-19.  The kernel must return the truncated formula bit for bit: lo lo is dropped
           (q q' 2^-28 per term) and nothing else.  No scale.
  place    A one-hot at k = (37 m) mod K with a = 1 + 2^-12 (hi 1, lo' 1/2); W[n, k] = h + l 2^-11 with
           h = 1024 + (131 n + 17 k) mod 1021 (hi) and l = 1 + (29 n + 7 k) mod 61 (lo').  C = h + l 2^-11 + h 2^-12, a multiple of
           2^-12 below 2^12: a wrong cell decodes into the (h, l) it was made from.  bias / resid / add2 small integers.
  sparse   A: 4 non-zeros per row, N(0, 1) 10^U(-3, 3) (reaches f16-subnormal hi); W dense, N(0, 1) 10^U(-2, 1), values below
           2^-13 lifted to it.  Against float64 under

               (3 2^-22 (1 + 2^-10) + (3 nz + 2) 2^-24) sum |a||w| + 2^-36 sum_{a != 0} |w|  + epilogue,

           (3 nz + 2) 2^-24: one fp32 rounding per non-zero term of the three phases, the scaling and the junction; epilogue:
           5 2^-24 (max(|s|, 1) (sum |a||w| + |bias|) + |add2| + |resid|) for bias, scale (two where the cross launch is scaled
           apart), add2 and resid.
  normal   dense standard normal: 3 2^-22 (1 + 2^-10) sum |a||w| + 2^-36 (sum |a| + sum |w|) + (3 K + 8) 2^-23 (...) — one fp32
           ulp per accumulated term, the safety net, not the sharp test.
  place24  (fp32 matrix path) A one-hot with a 24-bit value, W with 24-bit significands: the cell must be fl32(a w), the float64
           product rounded once — the path truncates no operand.
  dyadic   gemm_ref's, for gemm_f32_kernel.

LayerNorm pair: hi + lo'/2048 within ln_bound (fp32 form) + 2^-22 (1 + 2^-11) |n| + 2^-36 of the float64 LayerNorm; the pair
is self-consistent: |lo'/2048| <= half an f16 ulp of hi, and hi == f16(hi + lo'/2048) wherever that is not an exact tie (a
remainder just inside half an ulp may round, as lo', onto the half ulp).

FFN chain (make_ffn_case): x row m = a selector 32 at s = (37 m) mod D plus 4 fractions (multiples of 2^-14 in (-1, 1));
W1[f, k] = 2 for the four f in T(k) = (5 k + j F / 4) mod F, otherwise -2 or +-1; b1 = -40.  Hidden columns in T(s): 64 - 40 +
fractions in (16, 32), a multiple of 2^-14 (19 bits: wider than f16); every other column is at most 32 - 40 + 8 and dies in
the ReLU.  Pair of the hidden: ulp16 = 2^-6, |r| <= 2^-7, lo' = 2048 r a multiple of 2^-3 up to 16: exact.  W2 in {+-1, +-2},
b2 multiples of 2^-14 in [-2, 2], resid = x: y is a multiple of 2^-14 below 512 = 2^23 2^-14.  With a scale s on the hidden
(hidden_scale) the fp32 hidden is v = fl32(e s) with e exact: its pair must be split(v) bit for bit."""
import zlib

import numpy as np

import gemm_ref as G
from gemm_ref import f16, ln_ref, ln_bound, assert_exact, assert_bounded      # noqa: F401  (re-exported)

X3_EXACT = ("exact22", "both", "place")
BOUNDED = ("sparse", "normal")
DESIGNS = X3_EXACT + BOUNDED + ("place24", "dyadic")
Case = G.Case
QSCALE = G.QSCALE
PLACE_A = 1.0 + 2.0 ** -12


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def round_up(x, m):
    return -(-x // m) * m


# ------------------------------------------------------------------------------------------------ the split
def split(v):
    """(hi, lo') of fp32 v as float16 arrays"""
    v = np.asarray(v, np.float32)
    assert np.all(np.abs(v) < 65520.0)
    hi = v.astype(np.float16)
    r = v - hi.astype(np.float32)
    assert np.array_equal(r.astype(np.float64), v.astype(np.float64) - hi.astype(np.float64))
    return hi, (r * np.float32(2048.0)).astype(np.float16)


def split64(v):
    hi, lo = split(v)
    return hi.astype(np.float64), lo.astype(np.float64)


def join(hi, lo):
    return np.asarray(hi, np.float64) + np.asarray(lo, np.float64) / 2048.0


def split_image(x, K, Kp, ldo, swap, fill):
    """what split_x3_kernel leaves in a [rows, ldo] uint16 buffer pre-filled with `fill`"""
    x = np.asarray(x, np.float32)
    out = np.full((x.shape[0], ldo), fill, np.uint16)
    hi, lo = split(x[:, :K])
    out[:, :2 * Kp] = 0
    out[:, (Kp if swap else 0):(Kp if swap else 0) + K] = hi.view(np.uint16)
    out[:, (0 if swap else Kp):(0 if swap else Kp) + K] = lo.view(np.uint16)
    return out


def split_err_bound(v):
    v = np.abs(np.asarray(v, np.float64))
    return np.where(v >= 2.0 ** -14, 2.0 ** -22 * (1 + 2.0 ** -11) * v, np.where(v > 0, 2.0 ** -36, 0.0))


def assert_pair_consistent(hi, lo, what=""):
    hi16, lo16 = np.asarray(hi, np.float16), np.asarray(lo, np.float16)
    v = join(hi16, lo16)
    ulp = np.maximum(np.spacing(np.abs(hi16)).astype(np.float64), 2.0 ** -24)
    off = np.abs(lo16.astype(np.float64)) / 2048.0
    assert np.all(off <= ulp / 2), what + ": lo'/2048 exceeds half an f16 ulp of hi"
    # (a remainder just inside half an ulp may round, as lo', onto the half ulp itself: the sum is then a tie, which
    # round-to-nearest-even need not send back to hi — everywhere else it must)
    inside = off < ulp / 2
    assert np.array_equal(f16(v)[inside], hi16.astype(np.float64)[inside]), what + ": hi is not f16(hi + lo'/2048)"


def assert_pair_is_split(v32, hi, lo, what=""):
    """the pair a kernel wrote for the fp32 value v32 against split(v32), bit for bit"""
    eh, el = split(v32)
    for name, got, want in (("hi", hi, eh), ("lo'", lo, el)):
        got = np.asarray(got, np.float16)
        bad = got.view(np.uint16) != want.view(np.uint16)
        bad &= ~((got == 0) & (want == 0))                              # (+0 and -0 are the same operand)
        if bad.any():
            i = tuple(int(t) for t in np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs in %d of %d cells; first at %r: value %r, got %r, want %r" % (
                what, name, int(bad.sum()), bad.size, i, float(np.asarray(v32)[i]), float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------------ products
def x3_product(A, W):
    ah, al = split64(A)
    wh, wl = split64(W)
    return ah @ wh.T + 2.0 ** -11 * (ah @ wl.T + al @ wh.T)


def epilogue(v, c):
    v = np.array(v, np.float64)
    if c.bias is not None:
        v = v + c.bias.astype(np.float64)[None, :]
    if c.scale_cols > 0:
        n = min(c.scale_cols, c.N)
        assert G.pow2(c.scale) or c.design in BOUNDED
        v[:, :n] = v[:, :n] * np.float64(np.float32(c.scale))
    if c.add2 is not None:
        v = v + c.add2.astype(np.float64)
    if c.resid is not None:
        v = v + c.resid.astype(np.float64)
    return np.maximum(v, 0.0) if c.relu else v


def product(c):
    A, W = c.A.astype(np.float64), c.W.astype(np.float64)
    if c.design in X3_EXACT:
        return x3_product(c.A, c.W)
    if c.design == "place24":
        return (A @ W.T).astype(np.float32).astype(np.float64)
    return A @ W.T


def reference(c):
    return G.reference(c) if c.design == "dyadic" else epilogue(product(c), c)


def _mags(c):
    aw = np.abs(c.A.astype(np.float64)) @ np.abs(c.W.astype(np.float64)).T
    s = max(abs(c.scale), 1.0) if c.scale_cols > 0 else 1.0
    epi = aw + (np.abs(c.bias.astype(np.float64))[None, :] if c.bias is not None else 0.0)
    epi = s * epi
    for t in (c.add2, c.resid):
        if t is not None:
            epi = epi + np.abs(t.astype(np.float64))
    return aw, epi


def bound(c, fp32_path=False):
    """per-cell bound of the real-valued designs (module docstring).  fp32_path: gemm_f32_kernel — no representation
    term, one fp32 ulp per term of the K-long sum"""
    assert c.design in BOUNDED
    aw, epi = _mags(c)
    if fp32_path:
        return (c.K + 5) * 2.0 ** -23 * epi
    absA, absW = np.abs(c.A.astype(np.float64)), np.abs(c.W.astype(np.float64))
    rep = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) * aw + 2.0 ** -36 * ((absA != 0).astype(np.float64) @ absW.T)
    if c.design == "sparse":
        nz = int((absA != 0).sum(axis=1).max())
        return rep + (3 * nz + 2) * 2.0 ** -24 * aw + 5 * 2.0 ** -24 * epi
    rep = rep + 2.0 ** -36 * (absA @ (absW != 0).astype(np.float64).T)
    return rep + (3 * c.K + 8) * 2.0 ** -23 * epi


def _nonzero_cols(r, M, K, nz):
    nz = min(nz, K)
    return np.argsort(r.random((M, K)), axis=1)[:, :nz]


def make_case(design, M, N, K, bias=False, resid=False, add2=False, relu=False, scale_cols=0, scale=1.0, seed=0):
    assert design in DESIGNS, design
    if design == "dyadic":
        return G.make_case("dyadic", M, N, K, bias=bias, resid=resid, add2=add2, relu=relu, scale_cols=scale_cols, scale=scale, seed=seed)
    r = _rng(design, M, N, K, bias, resid, add2, relu, scale_cols, seed)
    rows = np.arange(M)[:, None]
    grid, cap = None, None
    ints = lambda shape, lim: r.integers(-lim, lim + 1, shape).astype(np.float64)
    if design == "exact22":
        assert scale_cols == 0 or scale == 0.125
        grid = 2.0 ** -17 if scale_cols else 2.0 ** -20
        cap = 2.0 ** 24 * grid * (0.125 if scale_cols else 1.0)
        lim = int(1 / grid) - 1
        v = r.integers(1, lim + 1, (M, min(4, K))) * r.choice((-1.0, 1.0), (M, min(4, K)))
        A = np.zeros((M, K))
        A[rows, _nonzero_cols(r, M, K, 4)] = v * grid
        W = r.choice((-2.0, -1.0, 1.0, 2.0), (N, K))
        add = lambda shape: ints(shape, int(2 / grid)) * grid
    elif design == "both":
        assert scale_cols == 0
        grid, cap = 2.0 ** -19, 32.0
        val = lambda shape: r.choice((-1.0, 1.0), shape) * r.integers(17, 33, shape) * 2.0 ** -5 + r.integers(-3, 4, shape) * 2.0 ** -14
        A = np.zeros((M, K))
        A[rows, _nonzero_cols(r, M, K, 8)] = val((M, min(8, K)))
        W = val((N, K))
        add = lambda shape: ints(shape, int(2 / grid)) * grid
    elif design == "place":
        assert scale_cols == 0
        grid, cap = 2.0 ** -12, 4096.0
        A = np.zeros((M, K))
        A[np.arange(M), (G.PLACE_P * np.arange(M)) % K] = PLACE_A
        n, k = np.arange(N)[:, None], np.arange(K)[None, :]
        W = 1024.0 + (131 * n + 17 * k) % 1021 + (1.0 + (29 * n + 7 * k) % 61) * 2.0 ** -11
        add = lambda shape: ints(shape, 3)
    elif design == "place24":
        assert not (bias or resid or add2 or scale_cols)
        A = np.zeros((M, K))
        A[np.arange(M), (G.PLACE_P * np.arange(M)) % K] = (1.0 + (2 * r.integers(0, 2 ** 22, M) + 1) * 2.0 ** -23)
        W = r.choice((-1.0, 1.0), (N, K)) * (1.0 + (2 * r.integers(0, 2 ** 22, (N, K)) + 1) * 2.0 ** -23) * 2.0 ** r.integers(-8, 9, (N, K))
        add = None
    elif design == "sparse":
        A = np.zeros((M, K))
        A[rows, _nonzero_cols(r, M, K, 4)] = r.standard_normal((M, min(4, K))) * 10.0 ** r.uniform(-3, 3, (M, min(4, K)))
        W = r.standard_normal((N, K)) * 10.0 ** r.uniform(-2, 1, (N, K))
        W = np.where(np.abs(W) < 2.0 ** -13, np.copysign(2.0 ** -13, W) + W, W)
        add = lambda shape: r.standard_normal(shape)
    else:                                                            # normal
        A, W = r.standard_normal((M, K)), r.standard_normal((N, K))
        add = lambda shape: r.standard_normal(shape)
    f = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    b = add((N,)) if bias else None
    rs = add((M, N)) if resid else None
    a2 = add((M, N)) if add2 else None
    c = Case(design, M, N, K, f(A), f(W), f(b), f(rs), f(a2), bool(relu), int(scale_cols), float(scale), 0, None, None, 0, 0.0)
    if design not in BOUNDED:
        for got, want in ((c.A, A), (c.W, W), (c.bias, b), (c.resid, rs), (c.add2, a2)):
            assert want is None or np.array_equal(got.astype(np.float64), want), design     # the design's values are fp32 numbers
    mag = float(G.magnitude(c).max())
    if cap is not None:
        assert mag < cap, (design, M, N, K, mag, cap)
    if design == "exact22":
        hi, lo = split64(c.A)
        assert np.array_equal(join(hi, lo), c.A.astype(np.float64)) and not split64(c.W)[1].any()
    if design == "both":
        for t in (c.A, c.W):
            hi, lo = split64(t)
            nzm = t != 0
            assert np.array_equal(np.abs(hi[nzm]) * 32, np.round(np.abs(hi[nzm]) * 32)) and np.all(np.abs(lo) <= 0.375)
            assert np.array_equal(join(hi, lo), t.astype(np.float64))
    return c._replace(cap=mag)


def _place_decode(v):
    h = np.floor(v)
    return int(h), float((v - h - h * 2.0 ** -12) * 2048.0)


def check(c, got, what="", fp32_path=False):
    """exact designs: bit equality, returns 0; sparse / normal: the bound, returns the worst |err| / bound"""
    ref = reference(c)
    if c.design in BOUNDED:
        return assert_bounded(ref, bound(c, fp32_path), got, what)
    try:
        assert_exact(c._replace(design="x3:" + c.design), ref, got, what)
    except AssertionError as e:
        if c.design != "place" or c.bias is not None or c.resid is not None or c.add2 is not None:
            raise
        got = np.asarray(got, np.float64)
        m, n = (int(i) for i in np.argwhere(~(got == ref))[0])
        raise AssertionError("%s — the value decodes to (hi %d, lo' %g), wanted (hi %d, lo' %g) of W[n %d, k %d]" % (
            (e,) + _place_decode(got[m, n]) + _place_decode(ref[m, n]) + (n, (G.PLACE_P * m) % c.K)))
    return 0.0


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_pair_bound(x, g, b):
    return ln_bound(x, g, b) + 2.0 ** -22 * (1 + 2.0 ** -11) * np.abs(ln_ref(x, g, b)) + 2.0 ** -36


# ------------------------------------------------------------------------------------------------ the FFN chain
class FfnCase:
    def __init__(self, M, D, F, seed=0):
        assert D % 4 == 0 and F % 4 == 0 and D >= 8
        r = _rng("ffn32", M, D, F, seed)
        self.M, self.D, self.F = M, D, F
        sel = (G.PLACE_P * np.arange(M)) % D
        x = np.zeros((M, D))
        cols = _nonzero_cols(r, M, D, 5)
        for m in range(M):                                           # four fraction columns that are not the selector
            cs = [k for k in cols[m] if k != sel[m]][:4]
            x[m, cs] = r.integers(1, 2 ** 14, 4) * r.choice((-1.0, 1.0), 4) * 2.0 ** -14
        x[np.arange(M), sel] = 32.0
        w1 = r.choice((-2.0, -1.0, 1.0), (F, D))
        for j in range(4):
            w1[(5 * np.arange(D) + j * (F // 4)) % F, np.arange(D)] = 2.0
        w2 = r.choice((-2.0, -1.0, 1.0, 2.0), (D, F))
        b2 = r.integers(-2 ** 15, 2 ** 15 + 1, D) * 2.0 ** -14
        f = lambda t: np.ascontiguousarray(t, np.float32)
        self.x, self.w1, self.b1, self.w2, self.b2 = f(x), f(w1), f(np.full(F, -40.0)), f(w2), f(b2)
        self.sel = sel
        e = self.pre_scale()
        live = e > 0
        assert live.sum(axis=1).max() <= 4 and np.all((e[live] > 16) & (e[live] < 32))
        hi, lo = split64(e.astype(np.float32))
        assert np.array_equal(join(hi, lo), e) and (lo != 0).mean() > 0.0
        cap = float((e @ np.abs(w2).T + np.abs(b2) + np.abs(x)).max())
        assert cap < 512.0, cap
        self.cap = cap

    def pre_scale(self):
        """relu(x W1^T + b1), exact"""
        return np.maximum(self.x.astype(np.float64) @ self.w1.astype(np.float64).T + self.b1.astype(np.float64), 0.0)

    def hidden32(self, scale=1.0):
        """the fp32 hidden: relu(fl32(e s)); s = 1: exact"""
        e = self.x.astype(np.float64) @ self.w1.astype(np.float64).T + self.b1.astype(np.float64)
        v = e.astype(np.float32)
        assert np.array_equal(v.astype(np.float64), e)
        return np.maximum(v * np.float32(scale), np.float32(0))

    def reference(self):
        return self.pre_scale() @ self.w2.astype(np.float64).T + self.b2.astype(np.float64) + self.x.astype(np.float64)

    def scaled_case(self, scale):
        """the second product behind a scaled hidden as a `sparse` case (A = the fp32 hidden, at most 4 non-zeros per row)"""
        h = self.hidden32(scale)
        return Case("sparse", self.M, self.D, self.F, h, self.w2, self.b2, self.x, None, False, 0, 1.0, 0, None, None, 0, 0.0)
