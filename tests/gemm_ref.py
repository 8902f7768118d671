"""numpy statement of the GEMM family (csrc/k_gemm.hip, k_gemm_small.hip, k_gemm_rc.hip, k_gemm_big.hip, k_gemm_qkv.hip,
k_ffn.hip): C = A W^T with the epilogue in the order csrc/kernels.h states,

    bias -> * scale (columns < scale_cols) -> + add2 -> + FSMN(V) -> + resid -> ReLU -> f16 (round to nearest even),

input designs whose answer is known exactly, the error bounds of the one real-valued design and the assertion helpers —
shared by tests/test_gemm_ref_cpu.py (which proves on the CPU that the designs and the helpers reject wrong GEMMs) and
tests/test_gpu_gemm_conformance.py.

Why an exact answer exists: an f16 x f16 product is exact in fp32, and when every partial sum is representable too, the
result does not depend on accumulation order, tile shape, split or kernel.  The reference is float64 BLAS, which is exact
for these designs (every partial sum needs at most 24 bits).

  dyadic  A, W multiples of 2^-5 in [-2, 2] (exact in f16); bias, resid, add2 multiples of 2^-10 in [-4, 4]; FSMN taps and
          V multiples of 2^-5 (|w| <= 1, |V| <= 2), so every tap product is a multiple of 2^-10 as well.  Every partial sum is
          a multiple of 2^-10 and, while cap = sum |a||w| + |bias| + |resid| + |add2| + sum |w_j||V| + |V| < 2^14, fits 24
          bits.  make_case asserts the cap per case.  Results carry up to 23 significant bits: their f16 rounding is not
          trivial.
  int     the FFN block (its hidden is stored as f16): x in {-1, 0, 1} with 8 non-zeros per row, W1 integers in [-8, 8], b1
          integers with relu(hidden) <= 2048 (exact in f16), W2 integers in [-4, 4], b2 and resid integers; every sum below
          2^24.
  ties    every result is exactly halfway between two f16 values: row m of A holds two ones, at k = 2 j and 2 j + 1
          (j = m mod K / 2); W[n, 2 j] = s 2048, W[n, 2 j + 1] = s odd, odd <= 2047, s = +-1: the result s (2048 + odd) lies
          in [2048, 4096), where f16 values are 2 apart.  Round-to-nearest-even sends 2049 to 2048 and 2051 to 2052.
  place   A one-hot at k = (37 m) mod K, W[n, k] = ((131 n + 17 k) mod 4093) - 2046: C[m, n] = W[n, k(m)], and a wrong
          value names the (n, k) it really came from.
  normal  A, W standard normal rounded to f16, bias / resid / add2 standard normal: against float64 under

              |got - ref| <= (K + 4 + taps) 2^-23 (sum |a||w| + |bias| + |resid| + |add2| + FSMN terms)
                             [ + 2^-11 |ref| + 2^-25 for an f16 result ]

          one fp32 ulp (not half) per accumulated term, so that a matrix core that truncates when it aligns addends is
          covered as well; 2^-11 |ref| is the f16 rounding, 2^-25 the f16 subnormal spacing.

Scale.  A power of two (2^-3) is exact and may be combined with everything.  128^-0.5 is used only where the pipeline
uses it (f16 results, no residual or addend); the reference is f16(fl32(fl32(v) fl32(s))) with v = acc + bias exact.

LayerNorm behind an exact x (gemm_rc, the short-input reduction, the fused FFN block): ln_ref / ln_bound.  With
c = (512 + 8) 2^-24 (gamma of a 512-term fp32 sum in any order, plus the handful of scalar operations), A = max |x| of the
row, s = sqrt(var + eps), z = (x - mean) / s:
    the mean is off by at most c A, so x - mean by e_d <= 2 c A; var = mean(d^2) by 2 s e_d + c var, hence s by the relative
    amount 2 c A / s + c / 2; z therefore by (2 c A / s)(1 + |z|) + |z| (c / 2 + 3 u), and
    |n_got - n| <= |g| dz + 2^-23 (|z g| + |b|)   [ + 2^-11 |n| + 2^-25 for the f16 copy ]."""
import collections
import zlib

import numpy as np

DESIGNS = ("dyadic", "ties", "place", "normal")
CAP = 2.0 ** 14
PLACE_P = 37
FSMN_K = 11
LN_EPS = 1e-12
QSCALE = float(np.float32(1.0) / np.sqrt(np.float32(128.0)))       # "128^-0.5" as the engine forms it: fl32(1 / fl32(sqrt(128)))

Case = collections.namedtuple("Case", "design M N K A W bias resid add2 relu scale_cols scale out_kind V taps T cap")
FfnCase = collections.namedtuple("FfnCase", "M x w1 b1 w2 b2 resid cap")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f16(x):
    """round to nearest even, as float64"""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def is_f16(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(f16(x), x))


def fsmn_terms(V, taps, T):
    """the FSMN memory sum_j w_j V[t + j - 5] + V[t] with zero padding at the edges of each run of T rows (taps [512, 11]),
    and the sum of the absolute values of its terms.  float64."""
    V = np.asarray(V, np.float64)
    w = np.asarray(taps, np.float64)
    M, D = V.shape
    k = w.shape[1]
    out, mag = V.copy(), np.abs(V)
    t = np.arange(M) % T
    for j in range(k):
        d = j - (k - 1) // 2
        src = np.arange(M) + d
        ok = (t + d >= 0) & (t + d < T) & (src >= 0) & (src < M)
        term = np.where(ok[:, None], V[np.clip(src, 0, M - 1)], 0.0) * w[:, j][None, :]
        out += term
        mag += np.abs(term)
    return out, mag


def magnitude(c):
    """sum |a||w| + |bias| + |resid| + |add2| + |FSMN terms| per output element (float64)"""
    mag = np.abs(c.A.astype(np.float64)) @ np.abs(c.W.astype(np.float64)).T
    for t in (c.bias, c.resid, c.add2):
        if t is not None:
            mag = mag + np.abs(np.asarray(t, np.float64))
    if c.V is not None:
        mag = mag + fsmn_terms(c.V, c.taps, c.T)[1]
    return mag


def make_case(design, M, N, K, bias=False, resid=False, add2=False, relu=False, scale_cols=0, scale=1.0, out_kind=0,
              fsmn=None, seed=0):
    """Seeded case of a design.  out_kind 0 = fp32 result, 1 = f16, 2 = f16 in the blocked layout.  fsmn = (B, T) with
    B T == M adds V [M, N] and taps [N, 11] (N = 512).  Every array is float32 and, where the kernel reads it as f16, exact in
    f16."""
    assert design in DESIGNS, design
    r = _rng(design, M, N, K, bias, resid, add2, relu, scale_cols, out_kind, fsmn, seed)
    V = taps = None
    T = 0
    grid = lambda shape, steps, unit: r.integers(-steps, steps + 1, shape).astype(np.float64) * unit
    b = rs = a2 = None
    if design == "dyadic":
        A, W = grid((M, K), 64, 2.0 ** -5), grid((N, K), 64, 2.0 ** -5)
        b = grid((N,), 4096, 2.0 ** -10) if bias else None
        rs = grid((M, N), 4096, 2.0 ** -10) if resid else None
        a2 = grid((M, N), 4096, 2.0 ** -10) if add2 else None
        if fsmn:
            V, taps = grid((M, N), 64, 2.0 ** -5), grid((N, FSMN_K), 32, 2.0 ** -5)
    elif design == "normal":
        A, W = f16(r.standard_normal((M, K))), f16(r.standard_normal((N, K)))
        b = r.standard_normal(N).astype(np.float32).astype(np.float64) if bias else None
        rs = r.standard_normal((M, N)).astype(np.float32).astype(np.float64) if resid else None
        a2 = r.standard_normal((M, N)).astype(np.float32).astype(np.float64) if add2 else None
        if fsmn:
            V, taps = f16(r.standard_normal((M, N))), (0.3 * r.standard_normal((N, FSMN_K))).astype(np.float32).astype(np.float64)
    elif design == "ties":
        assert not (bias or resid or add2 or fsmn or scale_cols) and K % 2 == 0
        J = K // 2
        A = np.zeros((M, K))
        j = np.arange(M) % J
        A[np.arange(M), 2 * j] = 1.0
        A[np.arange(M), 2 * j + 1] = 1.0
        s = np.where(r.integers(0, 2, (N, J)) == 1, 1.0, -1.0)
        odd = 2.0 * r.integers(0, 1024, (N, J)) + 1.0
        W = np.zeros((N, K))
        W[:, 0::2] = s * 2048.0
        W[:, 1::2] = s * odd
    else:                                                            # place
        assert not fsmn
        A = np.zeros((M, K))
        A[np.arange(M), (PLACE_P * np.arange(M)) % K] = 1.0
        W = ((131 * np.arange(N)[:, None] + 17 * np.arange(K)[None, :]) % 4093 - 2046).astype(np.float64)
        b = r.integers(-3, 4, N).astype(np.float64) if bias else None
        rs = r.integers(-3, 4, (M, N)).astype(np.float64) if resid else None
        a2 = r.integers(-3, 4, (M, N)).astype(np.float64) if add2 else None
    if fsmn:
        B, T = fsmn
        assert B * T == M and N == 512
    assert is_f16(A) and is_f16(W) and (V is None or is_f16(V))
    f = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    c = Case(design, M, N, K, f(A), f(W), f(b), f(rs), f(a2), bool(relu), int(scale_cols), float(scale), out_kind, f(V), f(taps), T, 0.0)
    for got, want in ((c.A, A), (c.W, W), (c.bias, b), (c.resid, rs), (c.add2, a2), (c.V, V), (c.taps, taps)):
        assert want is None or np.array_equal(got.astype(np.float64), want)
    cap = float(magnitude(c).max())
    if design != "normal":
        assert cap < (CAP if design == "dyadic" else 2.0 ** 24), (design, M, N, K, cap)
    return c._replace(cap=cap)


def pow2(s):
    m, _ = np.frexp(s)
    return m == 0.5


def reference(c):
    """float64 value of every output element as the kernel stores it (f16 results: the f16 value).  Exact for the exact
    designs; for `normal` the f16 rounding is applied to the float64 value."""
    v = c.A.astype(np.float64) @ c.W.astype(np.float64).T
    if c.bias is not None:
        v = v + c.bias.astype(np.float64)[None, :]
    if c.scale_cols > 0:
        n = min(c.scale_cols, c.N)
        if pow2(c.scale) or c.design == "normal":
            v[:, :n] = v[:, :n] * np.float64(np.float32(c.scale))
        else:
            assert c.design != "normal" and c.out_kind != 0 and c.resid is None and c.add2 is None and c.V is None
            v32 = v[:, :n].astype(np.float32)
            assert np.array_equal(v32.astype(np.float64), v[:, :n])
            v[:, :n] = (v32 * np.float32(c.scale)).astype(np.float64)       # fl32(fl32(v) fl32(s))
    if c.add2 is not None:
        v = v + c.add2.astype(np.float64)
    if c.V is not None:
        v = v + fsmn_terms(c.V, c.taps, c.T)[0]
    if c.resid is not None:
        v = v + c.resid.astype(np.float64)
    if c.relu:
        v = np.maximum(v, 0.0)
    if c.out_kind != 0:
        v = f16(v)
        assert np.isfinite(v).all(), "an f16 result of the design is not finite"
    return v


def bound(c):
    """the bound of the `normal` design per output element (module docstring)"""
    mag = magnitude(c)
    s = abs(c.scale) if c.scale_cols > 0 else 1.0
    if c.scale_cols > 0:
        mag = mag.copy()
        mag[:, :c.scale_cols] *= max(s, 1.0)
    b = (c.K + 4 + (FSMN_K + 1 if c.V is not None else 0)) * 2.0 ** -23 * mag
    if c.out_kind != 0:
        b = b + 2.0 ** -11 * np.abs(reference(c)) + 2.0 ** -25
    return b


# ------------------------------------------------------------------------------------------------ the FFN block
def make_ffn_case(M, resid=True, seed=0):
    """the `int` design for x_out = resid + relu(x W1^T + b1) W2^T + b2 (d_model 512, hidden 2048)"""
    r = _rng("int", M, resid, seed)
    D, F = 512, 2048
    x = np.zeros((M, D))
    for m in range(M):
        x[m, r.choice(D, 8, replace=False)] = r.choice((-1.0, 1.0), 8)
    w1 = r.integers(-8, 9, (F, D)).astype(np.float64)
    b1 = np.where(np.arange(F) % 2 == 0, r.integers(-40, 9, F), r.integers(0, 1001, F)).astype(np.float64)
    w2 = r.integers(-4, 5, (D, F)).astype(np.float64)
    b2 = r.integers(-1000, 1001, D).astype(np.float64)
    rs = r.integers(-1000, 1001, (M, D)).astype(np.float64) if resid else None
    h = np.maximum(x @ w1.T + b1, 0.0)
    assert h.max() <= 2048 and is_f16(h) and is_f16(x) and is_f16(w1) and is_f16(w2)
    cap = float((h @ np.abs(w2).T + np.abs(b2) + (np.abs(rs) if resid else 0.0)).max())
    assert cap < 2.0 ** 24, cap
    f = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    return FfnCase(M, f(x), f(w1), f(b1), f(w2), f(b2), f(rs), cap)


def ffn_reference(c):
    x, w1, b1, w2, b2 = (t.astype(np.float64) for t in (c.x, c.w1, c.b1, c.w2, c.b2))
    h = f16(np.maximum(x @ w1.T + b1, 0.0))
    y = h @ w2.T + b2
    return y + c.resid.astype(np.float64) if c.resid is not None else y


# ------------------------------------------------------------------------------------------------ LayerNorm behind x
def ln_ref(x, g, b, eps=LN_EPS):
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def ln_bound(x, g, b, half=False, eps=LN_EPS):
    x, g, b = (np.asarray(t, np.float64) for t in (x, g, b))
    D = x.shape[1]
    c, u = (D + 8) * 2.0 ** -24, 2.0 ** -24
    mu = x.mean(axis=1, keepdims=True)
    s = np.sqrt(((x - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    z = np.abs(x - mu) / s
    A = np.abs(x).max(axis=1, keepdims=True)
    dz = (2 * c * A / s) * (1 + z) + z * (c / 2 + 3 * u)
    out = np.abs(g) * dz + 2.0 ** -23 * (np.abs(z * g) + np.abs(b))
    if half:
        out = out + 2.0 ** -11 * np.abs(ln_ref(x, g, b, eps)) + 2.0 ** -25
    return out


# ------------------------------------------------------------------------------------------------ assertions
def _place_source(c, value):
    hit = np.argwhere(c.W.astype(np.float64) == value)
    return "W[n %d, k %d]" % tuple(hit[0]) if len(hit) else "no element of W"


def assert_exact(c, ref, got, what=""):
    """got == ref bit for bit (both as float64 of the stored values); reports the first offending (m, n)"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    if not bad.any():
        return
    m, n = (int(i) for i in np.argwhere(bad)[0])
    msg = "%s: %d of %d elements differ; first at (m %d, n %d): got %r, want %r" % (what, int(bad.sum()), bad.size, m, n,
                                                                                  float(got[m, n]), float(ref[m, n]))
    if isinstance(c, Case) and c.design == "place":
        msg += " — the value is %s, wanted k %d" % (_place_source(c, got[m, n]), (PLACE_P * m) % c.K)
    raise AssertionError(msg)


def assert_bounded(ref, bnd, got, what=""):
    """|got - ref| <= bnd everywhere; returns the worst |err| / bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bnd)
    if bad.any():
        m, n = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements out of bound; first at (m %d, n %d): got %r, want %r, |err| %.3e > %.3e"
                             % (what, int(bad.sum()), bad.size, m, n, float(got[m, n]), float(ref[m, n]), float(err[m, n]),
                                float(bnd[m, n])))
    return float((err / bnd).max())


def check(c, got, what=""):
    """exact designs: bit equality, returns 0; normal: the bound, returns the worst ratio"""
    ref = reference(c)
    if c.design == "normal":
        return assert_bounded(ref, bound(c), got, what)
    assert_exact(c, ref, got, what)
    return 0.0
