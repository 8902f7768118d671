"""numpy statement of the kernels that ARE a layer (csrc/k_ffn.hip in its decoder split forms and its finishing pass,
its encoder form with the out-projection in front and the next Q | K | V behind, csrc/k_decmid.hip, csrc/k_norm.hip
fsmn_dec_ln_kernel), float64, in the style of tests/gemm_ref.py whose f16 / is_f16 /
fsmn_terms / ln_ref / ln_bound / assert_exact / assert_bounded it reuses: one reference per op, two input designs, the error
bounds of the real-valued one and numpy models of the ops with a `mutate=` switch — shared by tests/test_layer_ref_cpu.py
(which proves the designs' claims and shows that the assertions reject the mutants) and tests/test_gpu_layer_conformance.py.

The ops (D = 512, F = 2048, M = B L rows):

  decoder split block   [x = resid + ctx Wo^T + bo,  a = f16(LN1(x))]   (the out-projection form; otherwise a is given)
                        h = f16(relu(a W1^T + b1))
                        t = ((h - mean) rstd) . G^T + d,   G = f16(gamma_F (.) W2),  d = beta_F W2^T,   mean / rstd of the 2048 h
                        [n = LN(t)]
                        The device computes rstd (sum_s part_s - mean c) + d with c = the row sums of G, the sums split over
                        1 | 2 | 3 | 4 | 8 shares, mean and E[h^2] from fp32 sums, the variance E[h^2] - mean^2 in double.
  decoder middle        tn = LN2(t), a zero row at l >= token_num[b];   x += sum_j w_j tn[l + j - 5] + tn[l] for l < token_num[b];
                        xn = f16(LN3(x)) on every row;   q = f16((xn Wq^T + bq) qscale)
  fsmn_dec_ln           the middle two lines on a given tn, 11 or 21 taps.
  encoder tail          stated, with its designs, in front of make_enc_case at the end of the module.

Design `steer` — every value up to and including t / x is known exactly, whatever the order of the sums.  The difficulty is
the LayerNorm between two products; it is removed by construction:

  * 15 row types j = 1 .. 15, row m has type 1 + 7 m mod 15 (rows 32 apart differ).  H16, H512 = Sylvester Hadamard matrices.
  * the operand of type j is a_j = s_j (.) g1 + b1n, s_j = row 7 + 31 j of H512 (balanced +-1), g1 in {+-1, +-2}, b1n in {-1, 0, 1}:
    the exact value of LN1 on x = 2^q s_j (mean 0, mean square 4^q, fl32(1 / sqrtf(4^q + 1e-12)) = 2^-q), q = m mod 4 + 1.  In the
    out-projection form ctx, Wo, bo are small integers and resid = 2^q s_j - ctx Wo^T - bo.
  * W1[f, :] = (1 / 512) sum_j (P[f, j] - r[f]) s_j / g1 and b1[f] = r[f] - W1[f, :] . b1n, so that a_j W1[f]^T + b1[f] = P[f, j]:
    2^(p_j + 1) where H16[j, f // 128] = +1 and a negative number elsewhere (p_j = j mod 5).  W1 is a multiple of 2^-10 below 2
    (11 bits: exact in f16), every partial sum of the product a multiple of 2^-10 below 2^13.  The hidden row is 1024 zeros and
    1024 values 2^(p + 1): mean 2^p, E[h^2] - mean^2 = 4^p, fp32 sums and sums of squares exact in any order.
  * G[n, f] = g[n, f // 128] + noise[n, f];  noise comes in pairs (v, -v) inside a group of 128, so a group's noise cancels only if
    every hidden column entered with its own weight;  g[n, .] = sum_j (2^(r_j - 11) u[j, n] - e[n]) H16[j, .] + g0[n] with
    u[j, .] a balanced +-1 pattern, r_j = 11 + j mod 3, e in {-1, 0, 1}, g0 in [-2, 2]:  sum_f (+-1)_j G[n, f] = 2^r_j u[j, n] - 2048 e[n],
    c[n] = 2048 g0[n] (non-zero: the mean term must cancel it), and d[n] = 2048 e[n] through beta_F = +-2048 at one hidden column
    whose G is e[n].  gamma_F = +-1, W2 = gamma_F G + gamma_F 2^-14 where |G| >= 1: f16(gamma_F W2) = G, but a colsum of the
    UNrounded product is off by up to 1 / 8.
        t[m, n] = 2^-p (2^(p + 1) sum_on G - 2^p c) + d = 2^r_j u[j, n]       exactly (every intermediate a multiple of 2^p below 2^(p + 24))
  * LN2 of a balanced +-2^r row: mean 0, rstd 2^-r, tn = u g2 + b2 with small-integer g2, b2: exact.  Taps are distinct
    multiples of 2^-8, x integers: x + FSMN(tn) is a multiple of 2^-8 below 2^11, exact.
  Behind the last LayerNorm (n, xn, q) the derived bound applies.

Design `normal` — real-valued operands at the magnitudes weights.synth_weights produces; bounds derived here, not tuned:

  * a value v that the device stores as f16 and feeds to the next product (the LN1 / LN3 result, the hidden, q) is f16(v) in the
    reference.  If the device's v' is within dv of v — dv = ln_bound of the fp32 LayerNorm arithmetic, or the accumulation term
    (K + 4) 2^-23 sum |a||w| of a product, plus what the inputs carry — then f16(v') = f16(v) bit for bit wherever
    f16(v - dv) = f16(v + dv), and is at most dv + one f16 spacing away elsewhere (f16_flip_bound): the slack the old tests
    gave every element is given only to the elements that sit on a rounding boundary.  An xn16 that is itself an output is
    compared with the unrounded LayerNorm under ln_bound(half=True), as in the GEMM suite.
  * through a product a bound becomes sum_k |W[n, k]| bound[m, k]; a perturbed input of a LayerNorm moves its result by
    ln_input_bound (mean, deviation and norm are 1-Lipschitz).
  * t: with c1 = (2048 + 8) 2^-24 the fp32 sums give mean within c1 mean and E[h^2] within c1 E[h^2], hence the one-pass variance
    within dv = c1 (E[h^2] + 2 mean^2) = c1 var (1 + 3 mean^2 / var): the conditioning of E[h^2] - mean^2.  rstd' lies in
    [1 / sqrt(var + dv + eps), 1 / sqrt(max(var - dv, 0) + eps)] (the clamp of a negative variance is the lower end), and
        |t' - t| <= rs_hi ((F + 4) 2^-23 sum |h||G| + c1 mean |c| + 2^-22 (|x| + |mean c|)) + max(rs_hi - rs, rs - rs_lo) |x - mean c|
                    + 2^-23 (|t| + |d|)  +  sum_f |G[n, f]| dz[m, f]                      (dz: ln_input_bound of bh)
    For a constant hidden row x - mean c = 0 exactly and rs_hi = 1e6: the bound is wide, and finite.
  * how wide: the accumulation term is a worst case over every summation order and over a matrix core that truncates, and at
    K = 512 it is about one f16 spacing of the result.  So by this bound nearly every stored f16 operand MAY sit on a rounding
    boundary, and the chained bound of t is a third of |t| (several |t| behind the out-projection) where the measured error
    is 1e-5 of that.  It still rejects a dropped share without the out-projection (tests/test_layer_ref_cpu.py); the
    discriminating power of the suite is in `steer`, `normal` adds the real-valued magnitudes, the conditioning of the
    one-pass variance and the degenerate rows.
"""
import collections
import zlib

import numpy as np

import gemm_ref as R
from gemm_ref import LN_EPS, QSCALE, assert_bounded, assert_exact, f16, fsmn_terms, is_f16, ln_bound, ln_ref  # noqa: F401

D, F, NT = 512, 2048, 15
TOKEN_SET = (0, 1, 4, 5, 6, 32, 33)                            # and L - 1, L

DecCase = collections.namedtuple("DecCase", "design M a w1 b1 gf bf w2 ln out_proj types")
MidCase = collections.namedtuple("MidCase", "dec B L token_num n2 taps x n3 wq bq")
FdlCase = collections.namedtuple("FdlCase", "B L k token_num tn taps x ln")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(*ts):
    out = []
    for t in ts:
        t32 = np.ascontiguousarray(t, np.float32)
        assert np.array_equal(t32.astype(np.float64), np.asarray(t, np.float64)), "a design value is not exact in fp32"
        out.append(t32)
    return out[0] if len(out) == 1 else out


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def row_type(m):
    return 1 + (7 * np.asarray(m)) % NT


def _ln_params(r, scale=0.1):
    return (1 + scale * r.standard_normal(D)).astype(np.float32), (scale * r.standard_normal(D)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the decoder split block
def steer_parts(seed=0):
    """everything of the `steer` design that does not depend on M (float64): the type tables and the weights"""
    r = _rng("steer", seed)
    H16, H512 = hadamard(16), hadamard(D)
    j = np.arange(NT + 1)
    s = H512[(7 + 31 * j) % D]                                   # s[j]: balanced for j >= 1 (row 0 of the table is unused)
    assert (s[1:].sum(1) == 0).all() and len(set((7 + 31 * j[1:]) % D)) == NT
    p = j % 5
    g1 = r.choice((1.0, 2.0, -1.0, -2.0), D)
    b1n = r.integers(-1, 2, D).astype(np.float64)
    on = H16[j][:, np.arange(F) // 128] > 0                      # [16, F]
    P = np.where(on, 2.0 ** (p + 1)[:, None], -(2.0 ** (p + 1))[:, None] * (1 + np.arange(F) % 3)[None, :]).T      # [F, 16]
    rr = r.integers(-2, 3, F).astype(np.float64)
    w1 = ((P[:, 1:] - rr[:, None]) @ s[1:]) / D / g1[None, :]
    b1 = rr - w1 @ b1n
    # second product
    u = np.zeros((NT + 1, D))
    for jj in range(1, NT + 1):
        u[jj] = r.permutation(np.repeat((1.0, -1.0), D // 2))
    rj = 11 + j % 3
    e = r.integers(-1, 2, D).astype(np.float64)
    g0 = r.integers(-2, 3, D).astype(np.float64)
    g0[g0 == 0] = 1.0
    grp = ((2.0 ** (rj - 11))[1:, None] * u[1:] - e[None, :]).T @ H16[1:] + g0[:, None]            # [D, 16]
    v = r.integers(-3, 4, (D, F // 2)).astype(np.float64)
    noise = np.empty((D, F))
    noise[:, 0::2], noise[:, 1::2] = v, -v
    f0 = 3 * 128 + 10
    noise[:, f0] = e - grp[:, 3]
    noise[:, f0 + 1] = -noise[:, f0]
    G = grp[:, np.arange(F) // 128] + noise
    gf = r.choice((1.0, -1.0), F)
    bf = np.zeros(F)
    bf[f0] = 2048.0 * gf[f0]
    w2 = gf[None, :] * G + np.where(np.abs(G) >= 1, gf[None, :] * 2.0 ** -14, 0.0)
    w2[:, f0] = gf[f0] * G[:, f0]
    return dict(s=s, p=p, g1=g1, b1n=b1n, on=on, P=P, w1=w1, b1=b1, u=u, rj=rj, e=e, g0=g0, G=G, gf=gf, bf=bf, w2=w2,
                c=2048.0 * g0, d=2048.0 * e)


_PARTS = {}


def _parts(seed=0):
    if seed not in _PARTS:
        _PARTS[seed] = steer_parts(seed)
    return _PARTS[seed]


def make_dec_case(design, M, out_proj=False, seed=0, special=None):
    """`steer`, or `normal` (special = None | "offset": b1 = 16, mean / std of the hidden = 16, row 0 a zero operand, i.e. a
    constant non-zero hidden row | "zero": b1 <= 0, row 0 a zero operand, i.e. an all-zero hidden row)"""
    r = _rng(design, M, out_proj, seed, special)
    ln = _ln_params(r)
    if design == "steer":
        assert special is None
        P_ = _parts(seed)
        jt = row_type(np.arange(M))
        a = P_["s"][jt] * P_["g1"][None, :] + P_["b1n"][None, :]
        op = None
        if out_proj:
            q = np.arange(M) % 4 + 1
            xo = (2.0 ** q)[:, None] * P_["s"][jt]
            ctx = np.zeros((M, D))
            for m in range(M):
                ctx[m, r.choice(D, 8, replace=False)] = r.choice((-1.0, 1.0), 8)
            wo = r.integers(-8, 9, (D, D)).astype(np.float64)
            bo = r.integers(-3, 4, D).astype(np.float64)
            resid = xo - ctx @ wo.T - bo
            op = tuple(_f32(ctx, wo, bo, resid)) + ((_f32(P_["g1"]), _f32(P_["b1n"])),)
        a, w1, b1, gf, bf, w2 = _f32(a, P_["w1"], P_["b1"], P_["gf"], P_["bf"], P_["w2"])
        assert is_f16(a) and is_f16(w1)
        return DecCase(design, M, a, w1, b1, gf, bf, w2, ln, op, jt)
    assert design == "normal"
    w1 = (r.standard_normal((F, D)) / np.sqrt(D)).astype(np.float32)
    b1 = (0.1 * r.standard_normal(F)).astype(np.float32)
    if special == "offset":
        b1 = np.full(F, 16.0, np.float32)
    elif special == "zero":
        b1 = -np.abs(b1)
    gf = (1 + 0.2 * r.standard_normal(F)).astype(np.float32)
    bf = (0.1 * r.standard_normal(F)).astype(np.float32)
    w2 = (r.standard_normal((D, F)) / np.sqrt(F)).astype(np.float32)
    a = f16(r.standard_normal((M, D))).astype(np.float32)
    if special:
        a[0] = 0.0
    op = None
    if out_proj:
        ctx = f16(r.standard_normal((M, D))).astype(np.float32)
        wo = f16(r.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
        bo = (0.1 * r.standard_normal(D)).astype(np.float32)
        resid = (2 * r.standard_normal((M, D))).astype(np.float32)
        op = (ctx, wo, bo, resid, _ln_params(r))
    return DecCase(design, M, a, f16(w1).astype(np.float32), b1, gf, bf, w2, ln, op, None)


def ln_steer(x, g, b, eps=LN_EPS):
    """LayerNorm with rstd rounded to fp32, everything else exact: what the device returns where the design makes
    fl32(1 / sqrt(var + eps)) a power of two"""
    x = np.asarray(x, np.float64)
    d = x - x.mean(1, keepdims=True)
    rs = fl32(1 / np.sqrt((d ** 2).mean(1, keepdims=True) + eps))
    return d * rs * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def _ln(design):
    return ln_steer if design == "steer" else ln_ref


def f16_flip_bound(v, dv):
    """|f16(v') - f16(v)| for any |v' - v| <= dv: 0 where the whole interval rounds alike, else dv + the f16 spacing"""
    v, dv = np.asarray(v, np.float64), np.asarray(dv, np.float64)
    same = f16(v - dv) == f16(v + dv)
    return np.where(same, 0.0, dv + _f16_spacing(np.abs(v) + dv))


def _x_out(c):
    ctx, wo, bo, resid, _ = (None if t is None else t for t in c.out_proj)
    return ctx.astype(np.float64) @ wo.astype(np.float64).T + bo.astype(np.float64) + resid.astype(np.float64)


def dec_reference(c):
    """dict(x_out, a, a_raw, pre, h, G, d, t, n): float64; a = the operand as stored (f16), a_raw the LayerNorm value in front of
    that rounding"""
    out = dict(x_out=None)
    a = c.a.astype(np.float64)
    if c.out_proj is not None:
        out["x_out"] = _x_out(c)
        g1, b1n = c.out_proj[4]
        out["a_raw"] = _ln(c.design)(out["x_out"], g1, b1n)
        a = f16(out["a_raw"])
        if c.design == "steer":
            assert np.array_equal(out["a_raw"], c.a.astype(np.float64)), "steer: LN1 of the designed x is not the designed operand"
    pre = a @ c.w1.astype(np.float64).T + c.b1.astype(np.float64)
    h = f16(np.maximum(pre, 0.0))
    Gm = f16(c.gf.astype(np.float64)[None, :] * c.w2.astype(np.float64))
    d = c.bf.astype(np.float64) @ c.w2.astype(np.float64).T
    mean = h.mean(1, keepdims=True)
    var = ((h - mean) ** 2).mean(1, keepdims=True)
    rs = 1 / np.sqrt(var + LN_EPS)
    t = ((h - mean) * (fl32(rs) if c.design == "steer" else rs)) @ Gm.T + d
    out.update(a=a, pre=pre, h=h, G=Gm, d=d, t=t, n=ln_ref(t, *c.ln))
    return out


def ln_input_bound(x, bx, g, eps=LN_EPS):
    """how far (x - mean) / sqrt(var + eps) * g moves when every x[m, k] moves by at most bx[m, k]"""
    x, bx, g = (np.asarray(t, np.float64) for t in (x, bx, g))
    mu = x.mean(1, keepdims=True)
    dd = bx + bx.mean(1, keepdims=True)
    s = np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps)
    ds = np.minimum(np.sqrt((dd ** 2).mean(1, keepdims=True)), 0.5 * s)      # (beyond s / 2 the bound is void anyway)
    z = np.abs(x - mu) / s
    return np.abs(g) * (dd + z * ds) / (s - ds)


def _f16_spacing(x):
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def dec_bounds(c, ref=None):
    """`normal`: dict(x_out, t, n, rho) — the bounds of the module docstring, rho = mean^2 / var per row"""
    ref = ref or dec_reference(c)
    w1 = np.abs(c.w1.astype(np.float64))
    out = dict(x_out=None)
    ba = np.zeros((c.M, D))
    if c.out_proj is not None:
        ctx, wo, bo, resid, (g1, b1n) = c.out_proj
        mag = np.abs(ctx.astype(np.float64)) @ np.abs(wo.astype(np.float64)).T + np.abs(bo) + np.abs(resid)
        out["x_out"] = (D + 4) * 2.0 ** -23 * mag
        ba = f16_flip_bound(ref["a_raw"], ln_input_bound(ref["x_out"], out["x_out"], g1) + ln_bound(ref["x_out"], g1, b1n))
    a = np.abs(ref["a"])
    ea = (D + 4) * 2.0 ** -23 * (a @ w1.T) + 2.0 ** -23 * np.abs(c.b1) + ba @ w1.T       # (a zero operand row: pre = b1, exactly)
    pre = ref["pre"]                                                # (the ReLU first: a negative value stays 0 whatever it carries)
    bh = np.where(f16(np.maximum(pre - ea, 0.0)) == f16(np.maximum(pre + ea, 0.0)), 0.0, ea + _f16_spacing(np.abs(pre) + ea))
    h, G, d = ref["h"], np.abs(ref["G"]), ref["d"]
    c1 = (F + 8) * 2.0 ** -24
    mean = h.mean(1, keepdims=True)
    e2 = (h ** 2).mean(1, keepdims=True)
    var = ((h - mean) ** 2).mean(1, keepdims=True)
    dv = c1 * (e2 + 2 * mean ** 2)
    rs = 1 / np.sqrt(var + LN_EPS)
    rs_hi, rs_lo = 1 / np.sqrt(np.maximum(var - dv, 0.0) + LN_EPS), 1 / np.sqrt(var + dv + LN_EPS)
    cs = ref["G"].sum(1)[None, :]
    x = h @ ref["G"].T
    bt = rs_hi * ((F + 4) * 2.0 ** -23 * (h @ G.T) + c1 * mean * np.abs(cs) + 2.0 ** -22 * (np.abs(x) + np.abs(mean * cs))) \
        + np.maximum(rs_hi - rs, rs - rs_lo) * np.abs(x - mean * cs) + 2.0 ** -23 * (np.abs(ref["t"]) + np.abs(d)) \
        + ln_input_bound(h, bh, 1.0) @ G.T
    out.update(t=bt, n=ln_input_bound(ref["t"], bt, c.ln[0]) + ln_bound(ref["t"], *c.ln), rho=(mean ** 2 / np.maximum(var, 1e-300))[:, 0])
    return out


SHARE_CHUNKS = {1: 8, 2: 4, 3: 3, 4: 2, 8: 1}                    # chunks of 256 hidden columns per share; 3 x 3 = 9: the ninth is zeros


def fl32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def dec_model(c, splits, mutate=None, shuffle=None):
    """The split block as the device computes it, in numpy: shares of SHARE_CHUNKS[splits] chunks, partial rows and statistics
    per share, the finishing pass rstd (sum_s part_s - mean c) + d.  Every fp32 operation is emulated by rounding a float64
    result to fp32 (exact for `steer`); shuffle = a Generator: the hidden columns of a share are summed in a shuffled order,
    one fp32 addition at a time.  Returns dict(x_out, t, parts, stats)."""
    assert mutate in (None, "share_rows_dropped", "share_stats_dropped", "ninth_chunk_bias", "unrounded_colsum", "operand_rows_32_swapped",
                      "stale_x_out")
    ref = dec_reference(c)
    a = f16(ref["a"])
    if mutate == "operand_rows_32_swapped" and c.M > 32:
        a = a.copy()
        a[[0, 32]] = a[[32, 0]]
    h = f16(np.maximum(a @ c.w1.astype(np.float64).T + c.b1.astype(np.float64), 0.0))
    G = ref["G"]
    nch = SHARE_CHUNKS[splits]
    part, ssum, ssq = np.zeros((c.M, D)), np.zeros(c.M), np.zeros(c.M)
    for sh in range(splits):
        cols = np.arange(sh * nch * 256, min((sh + 1) * nch * 256, F))
        hs, Gs = h[:, cols], G[:, cols]
        if mutate == "ninth_chunk_bias" and splits == 3 and sh == 2:        # the zero chunk computes relu(0 + b1[0:256]) against zero weights ...
            hs = np.concatenate([hs, f16(np.maximum(c.b1[:256].astype(np.float64), 0.0))[None, :].repeat(c.M, 0)], 1)
            Gs = np.concatenate([Gs, np.zeros((D, 256))], 1)                # ... and its hidden enters the statistics
        if shuffle is not None:
            o = shuffle.permutation(hs.shape[1])
            p_, s1, s2 = np.zeros((c.M, D)), np.zeros(c.M), np.zeros(c.M)
            for f in o:
                p_ = fl32(p_ + hs[:, f:f + 1] * Gs[None, :, f])
                s1, s2 = fl32(s1 + hs[:, f]), fl32(s2 + fl32(hs[:, f] * hs[:, f]))
        else:
            p_, s1, s2 = fl32(hs @ Gs.T), fl32(hs.sum(1)), fl32((hs ** 2).sum(1))
        if mutate == "share_rows_dropped" and sh == splits - 1:
            p_ = np.zeros_like(p_)
        if mutate == "share_stats_dropped" and sh == splits - 1:
            s1, s2 = np.zeros_like(s1), np.zeros_like(s2)
        part, ssum, ssq = fl32(part + p_), fl32(ssum + s1), fl32(ssq + s2)
    mu = ssum / F
    var = np.maximum(ssq / F - mu * mu, 0.0)
    mu32, rs = fl32(mu)[:, None], fl32(1 / np.sqrt(var + LN_EPS))[:, None]
    cs = fl32((c.gf.astype(np.float64)[None, :] * c.w2.astype(np.float64)).sum(1) if mutate == "unrounded_colsum" else G.sum(1))
    t = fl32(fl32(rs * fl32(part - fl32(mu32 * cs[None, :]))) + fl32(ref["d"])[None, :])
    xo = ref["x_out"]
    if mutate == "stale_x_out" and xo is not None:                           # every share writes x; a late one from a residual that is not this launch's
        xo = xo.copy()
        xo[c.M // 2:] -= c.out_proj[3].astype(np.float64)[c.M // 2:]
    return dict(x_out=xo, t=t, part=part, stats=(ssum, ssq))


# ------------------------------------------------------------------------------------------------ the decoder middle
# (L, token_num) of the decoder-middle cases, B = 3: every value of {0, 1, 4, 5, 6, 32, 33, L - 1, L} stands in the first, the
# middle and the last utterance somewhere in the set (test_layer_ref_cpu.py checks that); B L is never a multiple of 64
MID_CASES = ((1, (0, 0, 0)), (5, (1, 4, 5)), (31, (4, 1, 6)), (32, (5, 32, 1)), (33, (33, 5, 4)), (37, (6, 33, 32)), (70, (32, 6, 33)),
             (1, (1, 0, 1)), (5, (5, 0, 4)), (31, (31, 30, 0)), (32, (31, 32, 0)), (33, (32, 33, 1)), (37, (37, 0, 36)), (70, (69, 70, 33)))
FDL_L = (1, 2, 3, 11, 21, 40)


def token_nums(L, i):
    """three values of TOKEN_SET + {L - 1, L} within [0, L], rotated by i (the fsmn_dec_ln cases)"""
    vals = sorted({v for v in TOKEN_SET + (L - 1, L) if 0 <= v <= L})
    return np.array([vals[(i + 2 * k) % len(vals)] for k in range(3)], np.int32)


def steer_taps(k):
    j, col = np.arange(k)[:, None], np.arange(D)[None, :]
    return ((j + 1) + 32 * (col % 3)) * 2.0 ** -8 * np.where((j + col) % 2 == 0, 1.0, -1.0)          # [k, 512], all different per column


def make_mid_case(design, B, L, token_num, seed=0):
    r = _rng("mid", design, B, L, tuple(int(t) for t in token_num), seed)
    dec = make_dec_case(design, B * L, seed=seed)
    if design == "steer":
        n2 = _f32(r.choice((1.0, 2.0, 3.0, -1.0, -2.0), D), r.integers(-2, 3, D).astype(np.float64))
        taps = _f32(steer_taps(11))
        x = _f32(r.integers(-1000, 1001, (B, L, D)).astype(np.float64))
    else:
        n2 = _ln_params(r)
        taps = (0.1 * r.standard_normal((11, D))).astype(np.float32)
        x = (2 * r.standard_normal((B, L, D))).astype(np.float32)
    wq = f16(r.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    bq = (0.1 * r.standard_normal(D)).astype(np.float32)
    return MidCase(dec, B, L, np.asarray(token_num, np.int32), n2, taps, x, _ln_params(r), wq, bq)


def fsmn_dec(tn, taps, token_num, x, mutate=None):
    """x + masked FSMN memory of tn [B, L, D] (taps [k, D]); returns (x_new, |terms| summed, tn masked).  float64."""
    tn, x, w = np.asarray(tn, np.float64), np.asarray(x, np.float64), np.asarray(taps, np.float64)
    B, L, _ = tn.shape
    k = w.shape[0]
    left = (k - 1) // 2 + (1 if mutate == "window_off_by_one" else 0)
    valid = np.arange(L)[None, :] < np.asarray(token_num)[:, None]
    tm = tn if mutate == "input_mask_missing" else np.where(valid[..., None], tn, 0.0)
    flat = tm.reshape(B * L, -1)
    mem, mag = tm.copy(), np.abs(tm)
    for j in range(k):
        for l in range(L):
            src = l + j - left
            if mutate == "tap_across_edge":
                rows = np.arange(B) * L + src
                ok = (rows >= 0) & (rows < B * L)
                term = np.where(ok[:, None], flat[np.clip(rows, 0, B * L - 1)], 0.0) * w[j]
            elif 0 <= src < L:
                term = tm[:, src] * w[j]
            else:
                continue
            mem[:, l] += term
            mag[:, l] += np.abs(term)
    keep = np.ones_like(valid) if mutate == "output_mask_missing" else valid
    return np.where(keep[..., None], x + mem, x), np.where(keep[..., None], np.abs(x) + mag, 0.0), tm


def mid_reference(c, t=None):
    """dict(t, tn, x, xmag, xn_raw, xn, q_raw, q): float64; xn = f16(LN3(x)), q = f16((xn Wq^T + bq) qscale)"""
    t = dec_reference(c.dec)["t"] if t is None else t
    tn = _ln(c.dec.design)(t, *c.n2).reshape(c.B, c.L, D)
    x, mag, tm = fsmn_dec(tn, c.taps, c.token_num, c.x)
    xn_raw = ln_ref(x.reshape(-1, D), *c.n3)
    xn = f16(xn_raw)
    q_raw = (xn @ c.wq.astype(np.float64).T + c.bq.astype(np.float64)) * QSCALE
    return dict(t=t, tn=tm.reshape(-1, D), x=x.reshape(-1, D), xmag=mag.reshape(-1, D), xn_raw=xn_raw, xn=xn, q_raw=q_raw, q=f16(q_raw))


def q_bound(c, ref, bxn):
    wq = np.abs(c.wq.astype(np.float64))
    mag = np.abs(ref["xn"]) @ wq.T + np.abs(c.bq)
    return f16_flip_bound(ref["q_raw"], QSCALE * (bxn @ wq.T + (D + 4) * 2.0 ** -23 * mag) + 2.0 ** -23 * np.abs(ref["q_raw"]))


def mid_bounds(c, ref, bt=None):
    """dict(tn, x, xn16, q).  bt = None: t (and so tn and x) is exact — the `steer` design, where only xn and q carry a bound.
    xn16 bounds the xn16 OUTPUT of the three-launch forms against xn_raw"""
    if bt is None:
        bx = np.zeros_like(ref["x"])
        btn = bx
    else:
        valid = (np.arange(c.L)[None, :] < c.token_num[:, None]).reshape(-1, 1)
        btn = np.where(valid, ln_input_bound(ref["t"], bt, c.n2[0]) + ln_bound(ref["t"], *c.n2), 0.0)
        _, spread, _ = fsmn_dec(btn.reshape(c.B, c.L, D), np.abs(c.taps), c.token_num, np.zeros_like(c.x))
        bx = spread.reshape(-1, D) + (11 + 3) * 2.0 ** -23 * ref["xmag"]
    moved = ln_input_bound(ref["x"], bx, c.n3[0])
    bxn = f16_flip_bound(ref["xn_raw"], moved + ln_bound(ref["x"], *c.n3))
    return dict(tn=btn, x=bx, xn16=moved + ln_bound(ref["x"], *c.n3, half=True), q=q_bound(c, ref, bxn))


def mid_model(c, mutate=None):
    """The middle as the device computes it, in numpy on the exact t of the case (the block's mutants live in dec_model):
    dict(x, q, xn).  x is exact arithmetic (float64), xn the f16 of the float64 LayerNorm."""
    assert mutate in (None, "tap_across_edge", "window_off_by_one", "input_mask_missing", "output_mask_missing", "norm3_skipped_on_masked",
                      "q_groups_swapped", "q_unscaled", "bias_after_scale")
    t = dec_reference(c.dec)["t"]
    tn = _ln(c.dec.design)(t, *c.n2).reshape(c.B, c.L, D)
    fm = mutate if mutate in ("tap_across_edge", "window_off_by_one", "input_mask_missing", "output_mask_missing") else None
    x, _, _ = fsmn_dec(tn, c.taps, c.token_num, c.x, mutate=fm)
    x = x.reshape(-1, D)
    xn = f16(ln_ref(x, *c.n3))
    if mutate == "norm3_skipped_on_masked":
        valid = (np.arange(c.L)[None, :] < c.token_num[:, None]).reshape(-1, 1)
        xn = np.where(valid, xn, 0.0)
    acc = xn @ c.wq.astype(np.float64).T
    bq = c.bq.astype(np.float64)
    q = f16(acc + bq if mutate == "q_unscaled" else acc * QSCALE + bq if mutate == "bias_after_scale" else (acc + bq) * QSCALE)
    if mutate == "q_groups_swapped":
        q = q.copy()
        q[:, 8:16], q[:, 16:24] = q[:, 16:24].copy(), q[:, 8:16].copy()
    return dict(x=x, q=q, xn=xn)


def check_mid(c, ref, bnd, x, q, what, exact_x):
    """the assertions of the GPU file on x and q; returns the worst ratios (x, q)"""
    if exact_x:
        assert_exact(None, ref["x"], x, what + " x")
        rx = 0.0
    else:
        rx = ratio(ref["x"], bnd["x"], x, what + " x")
    return rx, ratio(ref["q"], bnd["q"], q, what + " q")


# ------------------------------------------------------------------------------------------------ fsmn_dec_ln alone
def make_fdl_case(B, L, k, token_num, seed=0):
    """integer tn, dyadic taps, integer x: x exact"""
    r = _rng("fdl", B, L, k, tuple(int(t) for t in token_num), seed)
    tn = _f32(r.integers(-5, 6, (B, L, D)).astype(np.float64))
    x = _f32(r.integers(-1000, 1001, (B, L, D)).astype(np.float64))
    return FdlCase(B, L, k, np.asarray(token_num, np.int32), tn, _f32(steer_taps(k)), x, _ln_params(r))


def fdl_reference(c, mutate=None):
    x, _, _ = fsmn_dec(c.tn, c.taps, c.token_num, c.x, mutate=mutate)
    x = x.reshape(-1, D)
    return dict(x=x, xn=ln_ref(x, *c.ln), bxn=ln_bound(x, *c.ln, half=True))


# ------------------------------------------------------------------------------------------------ the encoder tail (OP = 1)
#   x_mid = resid + f16(ctx) Wo^T + bo + FSMN(f16 V)   (11 taps [512, 11], utterances = runs of T rows)
#   a = f16(LN2(x_mid));  x = x_mid + f16(relu(a W1^T + b1)) W2^T + b2;  n = LN(x);  Q | K | V = f16((f16(n) Wqkv^T + bqkv) [x QSCALE for Q])
# `steer`: x_mid = 2^q s_j exactly, so a, the hidden (the decoder design's W1 / b1: 0 | 2^(p + 1)) and x are exact.  With a
# residual it is the free addend: resid = 2^q s_j - (ctx Wo^T + bo + FSMN(V)) on small-integer ctx, Wo, bo, V and the dyadic taps.
# Without one (the first layer) ctx itself steers: V[m, :] = beta(m) v, beta in {1, 2, 3}; column j of Wo holds 2^q_j s_j and ctx
# selects it; columns 16 .. 26 hold -taps[:, jj] v and ctx[m, 16 + jj] = beta(m + jj - 5) where that row is inside the utterance,
# so the product cancels every tap the FSMN is allowed to take — a tap across an utterance edge, or a missing one, stays visible;
# column 27 = -v cancels the identity term, column 28 = -bo the bias.
EncCase = collections.namedtuple("EncCase", "design B T ctx wo bo v taps resid ln2 w1 b1 w2 b2 ln wqkv bqkv")


def make_enc_case(design, B, T, resid=True, seed=0):
    r = _rng("enc", design, B, T, resid, seed)
    M = B * T
    wqkv = f16(r.standard_normal((3 * D, D)) / np.sqrt(D)).astype(np.float32)
    bqkv = (0.1 * r.standard_normal(3 * D)).astype(np.float32)
    ln = _ln_params(r)
    if design == "normal":
        ctx, v = f16(r.standard_normal((M, D))).astype(np.float32), f16(r.standard_normal((M, D))).astype(np.float32)
        wo = f16(r.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
        taps = (0.1 * r.standard_normal((D, 11))).astype(np.float32)
        w1 = f16(r.standard_normal((F, D)) / np.sqrt(D)).astype(np.float32)
        w2 = f16(r.standard_normal((D, F)) / np.sqrt(F)).astype(np.float32)
        b = [(0.1 * r.standard_normal(n)).astype(np.float32) for n in (D, F, D)]
        rs = (2 * r.standard_normal((M, D))).astype(np.float32) if resid else None
        return EncCase(design, B, T, ctx, wo, b[0], v, taps, rs, _ln_params(r), w1, b[1], w2, b[2], ln, wqkv, bqkv)
    P_ = _parts(seed)
    taps = steer_taps(11).T                                          # [512, 11]
    m = np.arange(M)
    jt = row_type(m)
    if resid:
        q = m % 4 + 1
        ctx = np.zeros((M, D))
        for i in range(M):
            ctx[i, r.choice(D, 8, replace=False)] = r.choice((-1.0, 1.0), 8)
        wo = r.integers(-8, 9, (D, D)).astype(np.float64)
        bo = r.integers(-3, 4, D).astype(np.float64)
        v = r.integers(-4, 5, (M, D)).astype(np.float64)
        rs = (2.0 ** q)[:, None] * P_["s"][jt] - (ctx @ wo.T + bo + fsmn_terms(v, taps, T)[0])
    else:
        vcol = r.choice((-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0), D)
        beta = 1.0 + (5 * m + m // T) % 3
        v = beta[:, None] * vcol[None, :]
        bo = r.integers(-3, 4, D).astype(np.float64)
        wo = r.integers(-8, 9, (D, D)).astype(np.float64)
        jj = np.arange(1, NT + 1)
        wo[:, jj] = ((2.0 ** (1 + jj % 4))[:, None] * P_["s"][jj]).T
        wo[:, 16:27] = -taps * vcol[:, None]
        wo[:, 27], wo[:, 28] = -vcol, -bo
        ctx = np.zeros((M, D))
        ctx[m, jt] = 1.0
        t = m % T
        for k in range(11):
            ok = (t + k - 5 >= 0) & (t + k - 5 < T)
            ctx[ok, 16 + k] = beta[np.clip(m + k - 5, 0, M - 1)][ok]
        ctx[:, 27], ctx[:, 28] = beta, 1.0
        rs = None
    w2 = r.integers(-4, 5, (D, F)).astype(np.float64)
    b2 = r.integers(-1000, 1001, D).astype(np.float64)
    assert is_f16(ctx) and is_f16(wo) and is_f16(v)
    vals = _f32(ctx, wo, bo, v, taps, P_["w1"], P_["b1"], w2, b2)
    ctx, wo, bo, v, taps, w1, b1, w2, b2 = vals
    return EncCase(design, B, T, ctx, wo, bo, v, taps, None if rs is None else _f32(rs), (_f32(P_["g1"]), _f32(P_["b1n"])), w1, b1, w2, b2,
                   ln, wqkv, bqkv)


def enc_reference(c, mutate=None):
    """dict(x_mid, xmag, a_raw, a, pre, h, x, n_raw, n, qkv_raw, qkv): float64.  mutate = "tap_across_edge": the FSMN ignores the
    utterance edges"""
    f = lambda t: np.asarray(t, np.float64)
    M = c.B * c.T
    mem, mag = fsmn_terms(c.v, c.taps, M if mutate == "tap_across_edge" else c.T)
    xm = f(c.ctx) @ f(c.wo).T + f(c.bo) + mem + (f(c.resid) if c.resid is not None else 0.0)
    xmag = np.abs(f(c.ctx)) @ np.abs(f(c.wo)).T + np.abs(f(c.bo)) + mag + (np.abs(f(c.resid)) if c.resid is not None else 0.0)
    a_raw = _ln(c.design)(xm, *c.ln2)
    a = f16(a_raw)
    pre = a @ f(c.w1).T + f(c.b1)
    h = f16(np.maximum(pre, 0.0))
    x = xm + h @ f(c.w2).T + f(c.b2)
    n_raw = ln_ref(x, *c.ln)
    n = f16(n_raw)
    qkv_raw = n @ f(c.wqkv).T + f(c.bqkv)
    qkv_raw[:, :D] *= QSCALE
    return dict(x_mid=xm, xmag=xmag, a_raw=a_raw, a=a, pre=pre, h=h, x=x, n_raw=n_raw, n=n, qkv_raw=qkv_raw, qkv=f16(qkv_raw))


def enc_bounds(c, ref):
    """dict(x, n16, qkv); `steer`: x is exact (bound 0)"""
    f = lambda t: np.abs(np.asarray(t, np.float64))
    if c.design == "steer":
        bx = np.zeros_like(ref["x"])
    else:
        bxm = (D + 4 + 12) * 2.0 ** -23 * ref["xmag"]
        ba = f16_flip_bound(ref["a_raw"], ln_input_bound(ref["x_mid"], bxm, c.ln2[0]) + ln_bound(ref["x_mid"], *c.ln2))
        ea = (D + 4) * 2.0 ** -23 * (f(ref["a"]) @ f(c.w1).T) + 2.0 ** -23 * f(c.b1) + ba @ f(c.w1).T
        pre = ref["pre"]
        bh = np.where(f16(np.maximum(pre - ea, 0.0)) == f16(np.maximum(pre + ea, 0.0)), 0.0, ea + _f16_spacing(np.abs(pre) + ea))
        bx = bxm + bh @ f(c.w2).T + (F + 4) * 2.0 ** -23 * (ref["h"] @ f(c.w2).T + f(c.b2) + f(ref["x_mid"]))
    moved = ln_input_bound(ref["x"], bx, c.ln[0])
    bn = f16_flip_bound(ref["n_raw"], moved + ln_bound(ref["x"], *c.ln))
    scale = np.where(np.arange(3 * D) < D, QSCALE, 1.0)[None, :]
    mag = f(ref["n"]) @ f(c.wqkv).T + f(c.bqkv)
    bqkv = f16_flip_bound(ref["qkv_raw"], scale * (bn @ f(c.wqkv).T + (D + 4) * 2.0 ** -23 * mag) + 2.0 ** -23 * np.abs(ref["qkv_raw"]))
    return dict(x=bx, n16=moved + ln_bound(ref["x"], *c.ln, half=True), qkv=bqkv)


def ratio(ref, bnd, got, what=""):
    """assert_bounded, the worst |err| / bound taken over the cells whose bound is not zero (a zero bound demands equality)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        assert_bounded(ref, bnd, got, what)
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
