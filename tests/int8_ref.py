"""Input designs with known answers, and the assertion helpers, for the int8 path (math_mode 2): the quantisers of
csrc/k_quant.hip (minmax_kernel + quantize_rows_kernel, ln_minmax_kernel + ln_quantize_kernel, quantize_weight_kernel,
import_weight_kernel, pack_dz_kernel) and the integer GEMM of csrc/k_gemm.hip (gemm_i8_pp3, gemm_i8f_pp3).  The definition
of the arithmetic stays oracle/int8.py; this file adds the epilogue in the order csrc/kernels.h states for GemmI8Args,

    dequantise -> + bias -> x scale (columns < scale_cols) -> + add2 -> + resid -> ReLU -> f16 (round to nearest even),

every step one float32 operation.  Shared by tests/test_int8_ref_cpu.py (which proves on the CPU that the designs and the
helpers reject wrong implementations: MUTANTS_Q, MUTANTS_G) and tests/test_gpu_int8_conformance.py.

Quantiser designs (make_quant_case):
  grid    max' - min' = 255 2^-j, so the scale is exactly 2^-j; x holds every multiple of scale / 2 of the range, so every code
          boundary is met as a tie.  min' = -(z + 0.5) scale: z = 100 gives the zero point 100 (a tie, to even); z = 101 gives
          102, the top value reaches 256 and must saturate.  A tensor smaller than the 511 values holds min', max' and a seeded
          subset.  Every value has at most 10 significant bits: exact in f16 too.
  nonneg / nonpos / zeros / single / negzero
          only positive values (zero point 0: the range is widened to 0), only negative ones (255), all zeros (scale 1, zero
          point 0), one non-zero element (the last), and -0.0 among zeros.
  recip   a scale that is no power of two, found by a seeded search so that at least 32 elements x have
          rne(fl(x / scale)) != rne(fl(x fl(1 / scale))).
  zptie   (min', max') found by a seeded search so that fl(min' / scale) is exactly k + 0.5 while the float64 quotient lies on
          the side that rounds the other way: the zero point at a tie that only float32 arithmetic sees.
  place   small values with the tensor's minimum and maximum at chosen cells (places()): the first and the last element, the
          last quad of a row, a row that is not a multiple of 4 from the end and, at the one shape whose quad count passes
          3 x 256 x 1024, each of the four unrolled slots of minmax_kernel and its remainder loop.
LayerNorm designs (make_ln_case):
  ln_exact   row r holds (+-1 + off_r) c_r with exactly D / 2 of each sign, c_r a power of two in 2^-7 .. 2^9, off_r an integer
             up to 1000: every partial sum is exact in any order, the variance is c_r^2, 1e-12 is absorbed, the normalised
             value is exactly +-1 (checked in float32 here).  gamma and beta are multiples of scale / 2 that make
             LayerNorm(x) the `grid` design; columns 0 and 1 pin max' and min' in every row.
  ln_normal  random rows against the float64 LayerNorm under gemm_ref.ln_bound (check_ln_normal).
GEMM designs (make_gemm_case):
  extreme  a and w codes 0 or 255 (by row / column parity) against zero points 0, 128, 255: all sixteen corners of
           (code, zero point) x (code, zero point); scales 2^-8.  Above K = 257 the integer sums pass 2^24; rows 2 and 3 of every
           four flip their first one / three codes, so that their sums are no multiples of 4 and the cast to float rounds.
  place    a_q - a_zp one-hot at k = (37 m) mod K, w_q[n, k] = (131 n + 17 k) mod 256, scales 1: a wrong value names its origin.
  ties     scales 1, sixteen ones per row of a_q - a_zp, W chosen so that the sum is +-(2048 + odd): halfway between two f16
           values.
  random   uniform codes, per-column zero points and float32 scales that are no powers of two."""
import collections
import functools

import numpy as np

import gemm_ref as G
from oracle import int8 as O

F32 = np.float32
QSCALE = G.QSCALE
Q_DESIGNS = ("grid", "nonneg", "nonpos", "zeros", "single", "negzero", "recip", "zptie", "place")
G_DESIGNS = ("extreme", "place", "ties", "random")
MUTANTS_Q = ("recip", "half_away", "trunc", "zp_f64", "no_zero", "scale0", "wrap", "pad_row", "last_quad")
MUTANTS_G = ("kpad", "cast_trunc", "scale_order", "bias_after_scale", "relu_before_resid", "zp_per_row", "range_pad_row",
             "range_unrounded")
UNROLL_SHAPE = (6200, 512)                                     # rows * cols / 4 just above 3 * 256 * 1024
MINMAX_STRIDE = 256 * 1024                                     # QMM_G * QMM_T quads per trip of minmax_kernel

QCase = collections.namedtuple("QCase", "design rows cols x codes scale zp")
LnCase = collections.namedtuple("LnCase", "design rows D x gamma beta y codes scale zp")
GCase = collections.namedtuple("GCase", "design M N K a_codes a_scale a_zp w_codes w_zp w_scale bias resid add2 relu scale_cols scale out_kind")


# ------------------------------------------------------------------------------------------------ the quantiser's model
def quantize_model(x, mutant=""):
    """(codes int32, scale float32, zero point int) of DynamicQuantizeLinear over the whole tensor.  mutant "": oracle/int8.py
    itself; otherwise one of MUTANTS_Q, a wrong implementation that the designs must tell apart."""
    x = np.asarray(x, F32)
    if mutant == "":
        return O.quantize_activation(x)
    assert mutant in MUTANTS_Q, mutant
    seen = x
    if mutant == "pad_row":                                    # a hostile pad row reaches the range
        seen = np.concatenate([x.reshape(-1), F32([2.0 ** 100, -2.0 ** 100])])
    if mutant == "last_quad":                                  # the min / max pass stops a quad early
        seen = x.reshape(-1)[:-4]
    mn, mx = F32(seen.min()), F32(seen.max())
    if mutant != "no_zero":
        mn, mx = min(mn, F32(0)), max(mx, F32(0))
    with np.errstate(all="ignore"):
        scale = F32(F32(mx - mn) / F32(255))
        if mx == mn and mutant != "scale0":
            scale = F32(1)
        if mutant == "zp_f64":
            z = 0.0 - float(mn) / float(scale)
        else:
            z = F32(F32(0) - F32(mn / scale))
        zp = F32(np.nan_to_num(np.rint(np.clip(z, 0, 255)), nan=0.0))
        q = (x * F32(F32(1) / scale)).astype(F32) if mutant == "recip" else (x / scale).astype(F32)
        if mutant == "half_away":
            r = (np.sign(q) * np.floor(np.abs(q) + F32(0.5))).astype(F32)
        elif mutant == "trunc":
            r = np.trunc(q)
        else:
            r = np.rint(q)
        v = np.nan_to_num((r + zp).astype(F32), nan=0.0, posinf=255.0, neginf=0.0)
        codes = np.mod(v, 256) if mutant == "wrap" else np.clip(v, 0, 255)
    return codes.astype(np.int32), scale, int(zp)


def weight_model(W):
    """per output channel: (codes int32 [N, K], scale float32 [N], zero point int32 [N]) — oracle/int8.py"""
    return O.quantize_weight(np.asarray(W, F32))


def pack_dz(colsum, wzp, K):
    """the packed column word of the f16-result kernel: (colsum - K wzp') * 256 + (wzp' & 255), primes minus 128"""
    colsum, wzp = np.asarray(colsum, np.int64), np.asarray(wzp, np.int64)
    v = (colsum - K * wzp) * 256 + (wzp & 255)
    assert np.abs(v).max(initial=0) < 2 ** 31
    return v.astype(np.int32)


def _fill(values, pinned, rows, cols, r):
    """rows x cols float32 holding the pinned values and then `values`, repeated to size, in a seeded order"""
    seq = np.concatenate([np.asarray(pinned, np.float64), r.permutation(np.asarray(values, np.float64))])
    x = np.resize(seq, rows * cols)
    out = r.permutation(x).reshape(rows, cols).astype(F32)
    assert np.array_equal(np.sort(out.reshape(-1).astype(np.float64)), np.sort(x)), "a value of the design is not exact in float32"
    return out


def _range_pairs(r, f16, n):
    """n seeded (min', max') pairs, min' in (-2, -1], max' in [2, 4), exact in f16 when asked"""
    b = 10 if f16 else 12                                      # bits behind the leading one: 10 is exact in f16
    lo = -(r.integers(1 << b, 2 << b, n).astype(F32) / F32(1 << b))
    hi = r.integers(1 << b, 2 << b, n).astype(F32) / F32(1 << (b - 1))
    return lo, hi, ((hi - lo).astype(F32) / F32(255)).astype(F32)


@functools.lru_cache(maxsize=None)
def _recip_search(f16):
    """(min', max', x values) of the `recip` design: at least 32 inputs whose code differs between fl(x / scale) and
    fl(x fl(1 / scale)).  Seeded, float32 arithmetic throughout."""
    lo, hi, scale = _range_pairs(G._rng("recip", f16), f16, 1 << 14)
    for i in range(len(lo)):
        s = scale[i]
        if np.frexp(s)[0] == 0.5:
            continue
        if f16:
            cand = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(F32)
            cand = cand[np.isfinite(cand)]
        else:                                                  # the float32 neighbours of every code boundary
            zp = np.rint(F32(0) - F32(lo[i] / s))
            up = dn = ((np.arange(255, dtype=np.float64) - float(zp) + 0.5) * float(s)).astype(F32)
            steps = [up]
            for _ in range(6):
                up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
                steps += [up, dn]
            cand = np.concatenate(steps)
        cand = cand[(cand >= lo[i]) & (cand <= hi[i])]
        pick = cand[np.rint((cand / s).astype(F32)) != np.rint((cand * F32(F32(1) / s)).astype(F32))]
        if len(pick) >= 32:
            return float(lo[i]), float(hi[i]), tuple(float(v) for v in pick[:96])
    raise AssertionError("recip: the search found no (min', max') with 32 reciprocal-sensitive inputs")


@functools.lru_cache(maxsize=None)
def _zptie_search(f16):
    """(min', max') of the `zptie` design: fl(min' / scale) is exactly k + 0.5 while the float64 quotient lies on the side
    that rounds the other way"""
    r = G._rng("zptie", f16)
    for _ in range(64):
        lo, hi, scale = _range_pairs(r, f16, 1 << 18)
        z32 = (F32(0) - (lo / scale).astype(F32)).astype(F32)
        z64 = -lo.astype(np.float64) / scale.astype(np.float64)
        tie = np.flatnonzero((z32 - np.floor(z32) == F32(0.5)) & (np.rint(z32) != np.rint(z64)))
        if len(tie):
            return float(lo[tie[0]]), float(hi[tie[0]])
    raise AssertionError("zptie: the search found no (min', max') whose zero point is a tie in float32 only")


def places(rows, cols):
    """name -> flat index (row-major, into [rows, cols]) of the cells the `place` design visits"""
    p = {"first": 0, "last": rows * cols - 1, "last quad of a row": (rows // 2) * cols + cols - 2,
         "row not a multiple of 4 from the end": max(rows - 2, 0) * cols + min(1, cols - 1)}
    if (rows, cols) == UNROLL_SHAPE:
        total, st = rows * cols // 4, MINMAX_STRIDE
        assert 3 * st < total < 3 * st + st // 8
        lead = total - 3 * st                                  # threads below it run the unrolled trip once
        for k in range(4):
            p["unrolled slot %d" % k] = 4 * ((lead - 2 if k % 2 else 5) + k * st) + k
        p["remainder loop, first trip"] = 4 * lead + 1
        p["remainder loop, last trip"] = 4 * (st - 1 + 2 * st) + 2
    return p


def make_quant_case(design, rows, cols, j=7, z=100, f16=False, where=("first", "last"), seed=0):
    """Seeded case of a quantiser design; asserts the design's own conditions (module docstring).  f16: every value is exact
    in f16 (the op hands the tensor to the kernel as f16).  where: (place of the minimum, place of the maximum) for `place`."""
    assert design in Q_DESIGNS, design
    r = G._rng("q", design, rows, cols, j, z, f16, where, seed)
    n = rows * cols
    s = 2.0 ** -j
    if design == "grid":
        lo = -(z + 0.5) * s
        vals = lo + np.arange(511) * (s / 2)
        x = _fill(vals[1:-1], [vals[0], vals[-1]], rows, cols, r)
    elif design == "nonneg":
        x = _fill(np.arange(1, 510) * (s / 2), [255 * s], rows, cols, r)
    elif design == "nonpos":
        x = _fill(-np.arange(1, 510) * (s / 2), [-255 * s], rows, cols, r)
    elif design == "zeros":
        x = np.zeros((rows, cols), F32)
    elif design == "single":
        x = np.zeros((rows, cols), F32)
        x[-1, -1] = 3.0
    elif design == "negzero":
        x = np.where(r.integers(0, 2, (rows, cols)) == 1, F32(-0.0), F32(0.0)).astype(F32)
        x[0, 0] = F32(-0.0)
    elif design == "recip":
        lo, hi, pick = _recip_search(bool(f16))
        x = _fill(pick, [lo, hi], rows, cols, r)
    elif design == "zptie":
        lo, hi = _zptie_search(bool(f16))
        x = _fill(r.integers(-1024, 2049, 64) * 2.0 ** -10, [lo, hi], rows, cols, r)
    else:
        x = (r.integers(-64, 65, (rows, cols)) * 2.0 ** -6).astype(F32)
        p = places(rows, cols)
        assert p[where[0]] != p[where[1]], where
        x.reshape(-1)[p[where[0]]] = -7.0
        x.reshape(-1)[p[where[1]]] = 9.0
    if f16:
        assert G.is_f16(x), design
    codes, scale, zp = quantize_model(x)
    # the design's own conditions
    if design == "grid":
        assert scale == F32(s) and zp == {100: 100, 101: 102}[z], (scale, zp)
        if n >= 511 + 2:
            assert len(np.unique(x)) == 511
            v = np.rint(x.astype(np.float64) / s) + zp
            assert (v > 255).sum() >= 1 if z == 101 else v.max() == 254
        assert codes.min() == 0 and codes.max() == (255 if z == 101 else 254)
    elif design in ("nonneg", "nonpos"):
        assert scale == F32(s) and zp == (0 if design == "nonneg" else 255) and (x.min() > 0 if design == "nonneg" else x.max() < 0)
    elif design in ("zeros", "negzero"):
        assert scale == F32(1) and zp == 0 and not codes.any()
        assert design == "zeros" or np.signbit(x).any()
    elif design == "single":
        assert zp == 0 and codes[-1, -1] == 255 and codes.sum() == 255
    elif design == "recip":
        assert np.frexp(scale)[0] != 0.5
        if n >= len(pick) + 2:
            other = quantize_model(x, "recip")[0]
            assert (other != codes).sum() >= 32, int((other != codes).sum())
    elif design == "zptie":
        assert quantize_model(x, "zp_f64")[2] != zp
    else:
        assert scale == F32(16.0) / F32(255) and x.min() == -7 and x.max() == 9
    return QCase(design, rows, cols, x, codes, F32(scale), int(zp))


def rowsum_of(codes):
    return (np.asarray(codes, np.int64) - 128).sum(axis=1).astype(np.int32)


def check_quant(c, aq, rowsum, params, what=""):
    """the op's (a' [rows, ld], rowsum, (scale, zp)) against the case: the same bits everywhere, pad columns 0"""
    scale, zp = params
    assert F32(scale) == c.scale and float(zp) == c.zp, "%s: scale %r zp %r, want %r %r" % (what, float(scale), float(zp), float(c.scale), c.zp)
    aq = np.asarray(aq)
    cols = c.codes.shape[1]
    assert aq.shape[0] == c.codes.shape[0] and aq.shape[1] >= cols, (what, aq.shape)
    got = aq[:, :cols].astype(np.int32) + 128
    bad = got != c.codes
    if bad.any():
        m, n = (int(i) for i in np.argwhere(bad)[0])
        x = getattr(c, "y", None)
        x = c.x if x is None else x
        raise AssertionError("%s: %d of %d codes differ; first at (%d, %d): got %d, want %d (value %r, value / scale %r)"
                             % (what, int(bad.sum()), bad.size, m, n, got[m, n], c.codes[m, n], float(x[m, n]), float(x[m, n]) / float(c.scale)))
    assert not aq[:, cols:].any(), what + ": a pad column does not hold 0"
    want = rowsum_of(c.codes)
    assert np.array_equal(np.asarray(rowsum), want), "%s: row sums differ, first at row %d" % (what, int(np.flatnonzero(np.asarray(rowsum) != want)[0]))


# ------------------------------------------------------------------------------------------------ LayerNorm in front
LN_C_EXP = (-7, 9)
LN_OFF_MAX = 1000
LN_NORMAL_CASES = ((5, 128, 0), (37, 512, 1), (37, 560, 2), (19, 2048, 3), (257, 512, 4))     # (rows, D, seed) of the GPU suite
LN_LEFT_OUT_MAX = 0.20


def make_ln_case(design, rows, D, j=7, z=100, seed=0):
    assert design in ("ln_exact", "ln_normal") and D % 4 == 0
    r = G._rng("ln", design, rows, D, j, z, seed)
    if design == "ln_normal":
        x = (r.standard_normal((rows, D)) * np.exp(r.uniform(-2, 2, (rows, 1))) + r.uniform(-3, 3, (rows, 1))).astype(F32)
        gamma = (1 + 0.2 * r.standard_normal(D)).astype(F32)
        beta = (0.3 * r.standard_normal(D)).astype(F32)
        y = G.ln_ref(x, gamma, beta)
        codes, scale, zp = quantize_model(y.astype(F32))
        assert codes.min() == 0 and codes.max() == 255
        return LnCase(design, rows, D, x, gamma, beta, y, codes, F32(scale), int(zp))
    s = 2.0 ** -j
    lo = -(z + 0.5) * s
    sign = np.empty((rows, D))
    for m in range(rows):
        sign[m, :2] = (1.0, -1.0)
        sign[m, 2:] = r.permutation(np.repeat((1.0, -1.0), (D - 2) // 2))
    assert (sign.sum(axis=1) == 0).all()
    c = 2.0 ** r.integers(LN_C_EXP[0], LN_C_EXP[1] + 1, (rows, 1))
    off = r.integers(-LN_OFF_MAX, LN_OFF_MAX + 1, (rows, 1)).astype(np.float64)
    x = ((sign + off) * c).astype(F32)
    assert np.array_equal(x.astype(np.float64), (sign + off) * c)
    # half-step indices of the values column i takes at sign +1 / -1: the same parity, so that gamma is a multiple of scale / 2
    hp = r.integers(0, 511, D)
    hm = hp + 2 * r.integers(-255, 256, D)
    hm = np.where(hm < 0, hp % 2, np.where(hm > 510, 510 - hp % 2, hm))
    hp[:2], hm[:2] = 510, 0                                    # column 0 (sign +1) is max', column 1 (sign -1) is min', in every row
    gamma64, beta64 = (hp - hm) / 2 * (s / 2), lo + (hp + hm) / 2 * (s / 2)
    gamma, beta = gamma64.astype(F32), beta64.astype(F32)
    assert np.array_equal(gamma.astype(np.float64), gamma64) and np.array_equal(beta.astype(np.float64), beta64)
    assert (np.round(gamma64 / (s / 2)) == gamma64 / (s / 2)).all() and (np.round(beta64 / (s / 2)) == beta64 / (s / 2)).all()
    y64 = sign * gamma64 + beta64
    y = y64.astype(F32)
    assert np.array_equal(y.astype(np.float64), y64) and y64.min() == lo and y64.max() == lo + 255 * s
    # the claim of the design, in float32 in the kernel's shifted two-pass form (any summation order gives the same)
    d = (x - x[:, :1]).astype(F32)
    mean = (d.sum(axis=1, keepdims=True, dtype=F32) / F32(D)).astype(F32)
    e = (d - mean).astype(F32)
    var = ((e * e).astype(F32).sum(axis=1, keepdims=True, dtype=F32) / F32(D)).astype(F32)
    assert np.array_equal(var.astype(np.float64), c * c) and np.array_equal((var + F32(1e-12)).astype(F32), var)
    rstd = (F32(1) / np.sqrt((var + F32(1e-12)).astype(F32))).astype(F32)
    assert np.array_equal((e * rstd).astype(F32).astype(np.float64), sign)
    codes, scale, zp = quantize_model(y)
    assert scale == F32(s) and zp == {100: 100, 101: 102}[z]
    return LnCase(design, rows, D, x, gamma, beta, y, codes, F32(scale), int(zp))


def ln_left_out(c):
    """share of the cells of an ln_normal case that lie within ln_bound of a code boundary, from the reference alone"""
    bnd = G.ln_bound(c.x, c.gamma, c.beta)
    v = c.y / float(c.scale) + c.zp
    dist = np.abs(v - np.floor(v) - 0.5) * float(c.scale)
    return float((dist <= bnd + 2.0 ** -22 * np.abs(c.y)).mean())


def check_ln_normal(c, aq, rowsum, params, what=""):
    """ln_normal: the parameters lie within what ln_bound allows for min' and max'; with the op's own parameters a code equals
    the float64 value's code wherever that value lies further than ln_bound (+ the float32 rounding of value / scale) from a
    code boundary, elsewhere it may differ by one; both ends of the code range occur; the row sums are the codes' sums."""
    scale, zp = float(params[0]), float(params[1])
    bnd = G.ln_bound(c.x, c.gamma, c.beta)
    e_lo = e_hi = bnd.max()                                    # the extremum may sit in another cell than the reference's
    lo, hi = min(c.y.min(), 0.0), max(c.y.max(), 0.0)
    u = 2.0 ** -23
    s_lo, s_hi = (hi - lo - e_lo - e_hi) / 255 * (1 - 2 * u), (hi - lo + e_lo + e_hi) / 255 * (1 + 2 * u)
    assert s_lo <= scale <= s_hi, "%s: scale %r outside [%r, %r]" % (what, scale, s_lo, s_hi)
    z_lo, z_hi = -(lo + e_lo) / s_hi * (1 - 2 * u), -(lo - e_lo) / s_lo * (1 + 2 * u)
    assert np.floor(z_lo) <= zp <= np.ceil(z_hi) and zp == np.rint(zp), "%s: zero point %r outside [%r, %r]" % (what, zp, z_lo, z_hi)
    aq = np.asarray(aq)
    got = aq[:, :c.D].astype(np.int64) + 128
    assert not aq[:, c.D:].any(), what + ": a pad column does not hold 0"
    v = c.y / scale + zp
    want = np.clip(np.rint(v), 0, 255)
    near = np.abs(v - np.floor(v) - 0.5) * scale <= bnd + 2.0 ** -22 * np.abs(c.y)
    bad = np.where(near, np.abs(got - want) > 1, got != want)
    if bad.any():
        m, n = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d codes off; first at (%d, %d): got %d, value / scale + zp = %r, bound / scale %r"
                             % (what, int(bad.sum()), m, n, got[m, n], float(v[m, n]), float(bnd[m, n] / scale)))
    assert got.min() == 0 and got.max() == 255, what + ": the code 0 or the code 255 does not occur"
    assert np.array_equal(np.asarray(rowsum, np.int64), (got - 128).sum(axis=1)), what + ": row sums are not the sums of the codes"
    return float(near.mean())


# ------------------------------------------------------------------------------------------------ weights
def make_weight_case(N, K, seed=0):
    """W [N, K]: per row, in turn, the `grid` design (z = 100, 101, j = 3, 7, 10), an all-zero row and a constant row; with the
    stored form (codes uint8, zero points uint8, scales) that import_weight takes"""
    r = G._rng("w", N, K, seed)
    W = np.zeros((N, K), F32)
    for n in range(N):
        kind = n % 8
        if kind == 6:
            continue
        if kind == 7:
            W[n] = F32((-1) ** (n // 8) * 0.75)
            continue
        s, z = 2.0 ** -(3, 7, 10)[kind % 3], (100, 101)[kind // 3]
        lo = -(z + 0.5) * s
        vals = lo + np.arange(511) * (s / 2)
        W[n] = _fill(vals[1:-1], [vals[0], vals[-1]], 1, K, r)[0]
    codes, scale, zp = weight_model(W)
    for n in range(N):
        if n % 8 < 6:
            assert scale[n] == F32(2.0 ** -(3, 7, 10)[n % 8 % 3]) and zp[n] == (100, 102)[n % 8 // 3]
        if n % 8 == 6:
            assert scale[n] == 1 and zp[n] == 0
    return W, codes, scale, zp


def check_weight(codes, scale, zp, K, got, what=""):
    """the weight op's (w' [N, ld], colsum, wzp, wscale, dz) against codes / scale / zp"""
    w, cs, wz, ws, dz = got
    assert np.array_equal(np.asarray(w)[:, :K].astype(np.int32) + 128, codes), what + ": codes differ"
    assert not np.asarray(w)[:, K:].any(), what + ": a pad column does not hold 0"
    want_cs = (np.asarray(codes, np.int64) - 128).sum(axis=1)
    assert np.array_equal(cs, want_cs), what + ": column sums differ"
    assert np.array_equal(np.asarray(wz) + 128, zp), what + ": zero points differ"
    assert np.array_equal(np.asarray(ws, F32).view(np.uint32), np.asarray(scale, F32).view(np.uint32)), what + ": scales differ"
    assert np.array_equal(dz, pack_dz(want_cs, np.asarray(zp, np.int64) - 128, K)), what + ": dz differs"


# ------------------------------------------------------------------------------------------------ the integer GEMM
def make_gemm_case(design, M, N, K, bias=False, resid=False, add2=False, relu=False, scale_cols=0, scale=1.0, out_kind=0, variant=0):
    """Seeded case of a GEMM design.  out_kind as pf_qgemm_desc: 0 fp32, 1 f16 (gemm_i8f_pp3), 2 f16 unpadded, 3 both.
    variant: the activation zero point of `extreme` (0, 1, 2 -> 0, 128, 255)."""
    assert design in G_DESIGNS, design
    r = G._rng("g", design, M, N, K, bias, resid, add2, relu, scale_cols, out_kind, variant)
    ints = lambda shape: r.integers(-3, 4, shape).astype(F32)
    b = rs = a2 = None
    if design == "extreme":
        a_zp, a_scale = (0, 128, 255)[variant], 2.0 ** -8
        a = np.repeat(255 * ((np.arange(M) + variant) & 1)[:, None], K, axis=1)
        a[2::4, :1] = 255 - a[2::4, :1]                        # K is a multiple of 4 and so is every constant row's sum: these rows'
        a[3::4, :3] = 255 - a[3::4, :3]                        # sums are not, and above 2^24 they are no float32 values
        w = np.repeat(255 * (np.arange(N) & 1)[:, None], K, axis=1)
        w_zp = np.asarray((0, 128, 255))[(np.arange(N) >> 1) % 3]
        w_scale = np.full(N, 2.0 ** -8, F32)
    elif design == "place":
        a_zp, a_scale = 3, 1.0
        a = np.full((M, K), 3)
        a[np.arange(M), (G.PLACE_P * np.arange(M)) % K] = 4
        w = (131 * np.arange(N)[:, None] + 17 * np.arange(K)[None, :]) % 256
        w_zp = (7 * np.arange(N) + 1) % 256
        w_scale = np.ones(N, F32)
    elif design == "ties":
        assert not (bias or resid or add2 or relu or scale_cols) and K >= 16
        J = K // 16
        a_zp, a_scale = 7, 1.0
        a = np.full((M, K), 7)
        j = np.arange(M) % J
        for t in range(16):
            a[np.arange(M), 16 * j + t] = 8
        neg = r.integers(0, 2, N) == 1
        odd = 2 * r.integers(0, 64, (N, J)) + 1
        w = np.full((N, K), 128)
        w[:, 15:16 * J:16] = 128 + odd
        w[neg] = 255 - w[neg]
        w_zp = np.where(neg, 255, 0)
        w_scale = np.ones(N, F32)
    else:
        a_zp, a_scale = int(r.integers(0, 256)), F32(r.uniform(0.01, 0.03))
        a, w = r.integers(0, 256, (M, K)), r.integers(0, 256, (N, K))
        w_zp = r.integers(0, 256, N)
        w_scale = r.uniform(0.002, 0.006, N).astype(F32)
        assert (np.frexp(w_scale)[0] != 0.5).all() and np.frexp(a_scale)[0] != 0.5
    if design != "ties":
        gen = (lambda shape: r.standard_normal(shape).astype(F32)) if design == "random" else ints
        b = gen(N) if bias else None
        rs = gen((M, N)) if resid else None
        a2 = gen((M, N)) if add2 else None
    if scale_cols and not G.pow2(scale):
        assert out_kind in (1, 2) and not resid and not add2, "a scale that is no power of two: f16 results without residual or addend only"
    c = GCase(design, M, N, K, a.astype(np.uint8), F32(a_scale), int(a_zp), w.astype(np.uint8), w_zp.astype(np.int32), w_scale, b, rs, a2,
              bool(relu), int(scale_cols), float(scale), out_kind)
    assert np.array_equal(c.a_codes, a) and np.array_equal(c.w_codes, w)
    if design == "extreme" and M >= 2 and N >= 6 and variant != 1:
        assert {(int(x), int(y)) for x, y in zip(c.w_codes[:, 0], c.w_zp)} >= {(0, 0), (0, 255), (255, 0), (255, 255)}
        assert set(c.a_codes[:, 0]) == {0, 255}
    y32, y16, _ = gemm_reference(c)
    if design == "extreme" and M >= 4 and N >= 2 and K >= 560:
        iv = integer_sums(c)
        assert (iv.astype(F32).astype(np.float64) != iv).any(), "no sum of the design is rounded by the cast"
    if design == "ties":
        assert (np.abs(y32) >= 2048).all() and (np.abs(y32) % 2 == 1).all()
    assert out_kind == 0 or np.isfinite(y16).all()
    return c


def integer_sums(c, mutant=""):
    """sum_k (a_q - a_zp)(w_q - w_zp[n]), exact (float64 holds every partial sum), the way the device forms it: the product of
    the signed bytes corrected by the row and column sums"""
    a = c.a_codes.astype(np.float64) - 128
    w = c.w_codes.astype(np.float64) - 128
    az = float(c.a_zp) - 128
    wz = c.w_zp.astype(np.float64) - 128
    if mutant == "zp_per_row":
        wz = np.resize(wz, c.M)[:, None] * np.ones((1, c.N))
    else:
        wz = wz[None, :] * np.ones((c.M, 1))
    Kx = -(-c.K // 128) * 128 if mutant == "kpad" else c.K
    iv = a @ w.T - wz * a.sum(axis=1)[:, None] - az * w.sum(axis=1)[None, :] + Kx * az * wz
    assert np.abs(iv).max() < 2.0 ** 31
    if mutant == "" and c.M * c.N * c.K <= 1 << 26:
        direct = (c.a_codes.astype(np.float64) - c.a_zp) @ (c.w_codes.astype(np.float64) - c.w_zp[:, None]).T
        assert np.array_equal(iv, direct)
    return iv


def gemm_reference(c, mutant=""):
    """(y32, y16 as float32, (min, max) of the f16 results including 0): every step one float32 operation in kernels.h's
    order.  mutant: one of MUTANTS_G, a wrong implementation for tests/test_int8_ref_cpu.py."""
    assert mutant == "" or mutant in MUTANTS_G, mutant
    iv = integer_sums(c, mutant)
    if mutant == "cast_trunc":
        v = iv.astype(F32)
        over = np.abs(v.astype(np.float64)) > np.abs(iv)
        v = np.where(over, np.nextafter(v, F32(0)), v).astype(F32)
    else:
        v = iv.astype(np.int64).astype(np.int32).astype(F32)
    if mutant == "scale_order":
        y = ((v * c.a_scale).astype(F32) * c.w_scale[None, :]).astype(F32)
    else:
        y = (v * (c.a_scale * c.w_scale).astype(F32)[None, :]).astype(F32)
    sc = np.ones(c.N, F32)
    sc[:min(c.scale_cols, c.N)] = F32(c.scale)
    if mutant == "bias_after_scale":
        y = (y * sc[None, :]).astype(F32)
        if c.bias is not None:
            y = (y + c.bias[None, :]).astype(F32)
    else:
        if c.bias is not None:
            y = (y + c.bias[None, :]).astype(F32)
        y = (y * sc[None, :]).astype(F32)
    if mutant == "relu_before_resid" and c.relu:
        y = np.maximum(y, F32(0))
    if c.add2 is not None:
        y = (y + c.add2).astype(F32)
    if c.resid is not None:
        y = (y + c.resid).astype(F32)
    if c.relu:
        y = np.maximum(y, F32(0))
    with np.errstate(over="ignore"):
        y16 = y.astype(np.float16).astype(F32)
    src = y if mutant == "range_unrounded" else y16
    rng = (min(float(src.min()), 0.0), max(float(src.max()), 0.0))
    if mutant == "range_pad_row":
        rng = (min(rng[0], -65504.0), rng[1])
    return y, y16, rng


def _origin(c, m, n, value):
    if c.design != "place":
        return ""
    hit = np.flatnonzero(c.w_codes[n].astype(np.int64) - int(c.w_zp[n]) == value)
    src = np.argwhere(c.w_codes.astype(np.int64) - c.w_zp[:, None] == value)
    return " — wanted k %d; row n of W holds the value at k %s; first (n, k) anywhere: %s" % (
        (G.PLACE_P * m) % c.K, list(hit[:4]), tuple(src[0]) if len(src) else None)


def check_gemm(c, got, what="", ref=None):
    """the op's (y32, y16, range) against the reference: the same values everywhere (a None on either side is skipped)"""
    ref = ref or gemm_reference(c)
    for name, g, w in (("fp32", got[0], ref[0]), ("f16", got[1], ref[1])):
        if g is None or w is None:
            continue
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = ~(g == w)
        if bad.any():
            m, n = (int(i) for i in np.argwhere(bad)[0])
            raise AssertionError("%s: %d of %d %s results differ; first at (m %d, n %d): got %r, want %r%s"
                                 % (what, int(bad.sum()), bad.size, name, m, n, float(g[m, n]), float(w[m, n]), _origin(c, m, n, g[m, n])))
    if got[2] is not None:
        assert tuple(got[2]) == tuple(ref[2]), "%s: range %r, want %r" % (what, tuple(got[2]), tuple(ref[2]))
