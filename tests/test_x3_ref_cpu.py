"""CPU: tests/x3_ref.py proves itself.  An fp32 emulation of the x3 product (f16 x f16 products exact in fp32, fp32
accumulation term by term) shows every exact design bit-equal to its reference under permuted summation orders and both
phase orders (cross terms first, scaled, then the main term: the K-loop wrap; main term first into an intermediate, then the
scaled cross terms on top: the two-launch form), the real-valued designs inside their bounds — and the same assertions
reject fifteen wrong implementations, each on the design meant to see it."""
import numpy as np
import pytest

import gemm_ref as G
import x3_ref as R

F32 = np.float32


def _pad(t, Kp, fill=0.0):
    out = np.full((t.shape[0], Kp), fill, np.float32)
    out[:, :t.shape[1]] = t.astype(np.float32)
    return out


def _acc(acc, a, w, order):
    """acc += sum_k a[:, k] w[:, k], one fp32 rounding per term, in the given order of k"""
    for k in order:
        if a[:, k].any():
            acc = (acc + np.outer(a[:, k], w[:, k]).astype(F32)).astype(F32)
    return acc


def emulate(c, order=None, form="wrap", bug=None):
    """the x3 Linear in fp32 arithmetic; bug = one of the wrong implementations of the module docstring's list"""
    Kp = R.round_up(c.K, 64)
    ah, al = R.split(c.A)
    wh, wl = R.split(c.W)
    if bug == "lo_unscaled":
        al = (c.A - ah.astype(F32)).astype(np.float16)
    if bug == "f16_operands":
        al, wl = np.zeros_like(al), np.zeros_like(wl)
    pad = 52000.0 if bug == "pad_not_zeroed" else 0.0
    ah, al, wh, wl = (_pad(t, Kp, pad) for t in (ah, al, wh, wl))
    if bug == "halves_swapped":
        ah, al = al, ah
    order = np.arange(Kp) if order is None else order
    zero = np.zeros((c.M, c.N), F32)
    wscale = F32(2.0 ** -10 if bug == "wrap_scale" else 2.0 ** -11)
    bias = c.bias[None, :] if c.bias is not None else F32(0)
    cross = zero
    if bug != "no_hi_lo":
        cross = _acc(cross, ah, wl, order)
    if bug != "no_lo_hi":
        cross = _acc(cross, al, wh, order)
    main_w = wl if bug == "cursor_wrong_half" else wh
    if form == "wrap":
        if bug == "bias_before_wrap":
            cross = (cross + bias).astype(F32)
        v = _acc((cross * wscale).astype(F32), ah, main_w, order)
        if bug != "bias_before_wrap":
            v = (v + bias).astype(F32)
    else:
        v = (_acc(zero, ah, main_w, order) + bias).astype(F32)
    sc = c.scale_cols + (64 if bug == "scale_edge" else 0)
    s = np.where(np.arange(c.N) < sc, F32(c.scale), F32(1))[None, :].astype(F32)
    add2 = c.add2 if c.add2 is not None else F32(0)
    resid = c.resid if c.resid is not None else F32(0)
    if form == "wrap":
        if bug == "scale_on_resid":
            v = (((v + add2).astype(F32) + resid).astype(F32) * s).astype(F32)
        else:
            v = (v * s).astype(F32)
            v = (v + add2).astype(F32)
    else:                                                            # t = (main + bias) s + add2; out = cross 2^-11 s + t + resid
        t = ((v * s).astype(F32) + add2).astype(F32)
        v = ((cross * (s * wscale).astype(F32)).astype(F32) + t).astype(F32)
    if bug == "relu_before_resid" and c.relu:
        return (np.maximum(v, F32(0)) + resid).astype(F32)
    if bug != "scale_on_resid" or form != "wrap":
        v = (v + resid).astype(F32)
    return np.maximum(v, F32(0)) if c.relu else v


def emulate_fp32(c, order=None, trunc_bits=0):
    """gemm_f32_kernel: one fused multiply-add per term (float64 product, one rounding)"""
    A, W = c.A.astype(np.float64), c.W.astype(np.float64)
    if trunc_bits:
        m, e = np.frexp(A)
        A = np.ldexp(np.trunc(m * 2.0 ** trunc_bits) / 2.0 ** trunc_bits, e)
    acc = np.zeros((c.M, c.N), F32)
    for k in (np.arange(c.K) if order is None else order):
        if A[:, k].any():
            acc = (acc.astype(np.float64) + np.outer(A[:, k], W[:, k])).astype(F32)
    return acc


def _orders(Kp, n=3):
    r = np.random.default_rng(Kp)
    return [np.arange(Kp), np.arange(Kp)[::-1]] + [r.permutation(Kp) for _ in range(n - 1)]


EPI = (dict(), dict(bias=True, resid=True, add2=True, relu=True))


# ---- the split
def test_split_is_exact_and_within_its_bound():
    r = np.random.default_rng(1)
    v = (r.standard_normal(1_400_000) * 10.0 ** r.uniform(-8, 4, 1_400_000)).astype(np.float32)
    v = v[np.abs(v) < 65000.0]
    hi, lo = R.split64(v)                                            # (split itself asserts that r is exact)
    err = np.abs(v.astype(np.float64) - R.join(hi, lo))
    big = np.abs(v) >= 2.0 ** -14
    assert (err[big] / np.abs(v[big].astype(np.float64))).max() <= 2.0 ** -22 * (1 + 2.0 ** -11)
    assert err[~big].max() <= 2.0 ** -36
    assert np.all(err <= R.split_err_bound(v))
    R.assert_pair_consistent(*R.split(v))
    for x in (0.0, -0.0, 2.0 ** -24, 2.0 ** -14, 65504.0, 65519.996, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-40):
        h, l = R.split(np.float32([x]))
        assert np.isfinite(h).all() and np.isfinite(l).all()
    assert R.split(np.float32([1 + 2.0 ** -11]))[0][0] == 1.0 and R.split(np.float32([1 + 3 * 2.0 ** -11]))[0][0] == np.float16(1 + 2.0 ** -9)
    # the image helper: pads zero, the rest keeps its fill
    img = R.split_image(np.float32([[1 + 2.0 ** -12, 3.0, 9.0]]), 2, 4, 10, 1, 0x7E5A)
    assert img[0, 4:6].view(np.float16).tolist() == [1.0, 3.0] and img[0, 0:2].view(np.float16).tolist() == [0.5, 0.0]
    assert not img[0, 2:4].any() and not img[0, 6:8].any() and (img[0, 8:] == 0x7E5A).all()


# ---- the exact designs
@pytest.mark.parametrize("epi", range(len(EPI)))
@pytest.mark.parametrize("design", R.X3_EXACT)
def test_exact_designs_in_any_order_and_either_phase_order(design, epi):
    for M, N, K in ((9, 70, 64), (5, 9, 100), (3, 4, 192)):
        c = R.make_case(design, M, N, K, **EPI[epi])
        ref = R.reference(c)
        for order in _orders(R.round_up(K, 64)):
            for form in ("wrap", "two"):
                R.check(c, emulate(c, order, form), "%s %s" % (design, form))
        if design == "exact22":                                      # the formula IS the product
            assert np.array_equal(R.product(c), c.A.astype(np.float64) @ c.W.astype(np.float64).T)
            if not epi:
                assert (np.abs(emulate(c, bug="f16_operands") - ref) > 0).mean() > 0.9
        if design == "both":                                         # the formula is NOT the product: lo lo is missing
            d = np.abs(R.product(c) - c.A.astype(np.float64) @ c.W.astype(np.float64).T)
            assert (d > 0).mean() > 0.8 and d.max() <= 8 * 9 * 2.0 ** -28


def test_exact22_with_a_scale():
    c = R.make_case("exact22", 7, 192, 64, bias=True, resid=True, scale_cols=64, scale=0.125)
    for form in ("wrap", "two"):
        for order in _orders(64):
            R.check(c, emulate(c, order, form))
    c = R.make_case("exact22", 7, 70, 100, bias=True, add2=True, relu=True, scale_cols=70, scale=0.125)
    R.check(c, emulate(c, form="two"))


def test_fp32_path_designs():
    c = R.make_case("place24", 9, 11, 37)
    for order in _orders(37):
        R.check(c, emulate_fp32(c, order))
    c = R.make_case("dyadic", 9, 70, 33, bias=False)
    R.check(c, emulate_fp32(c))
    c = R.make_case("normal", 9, 11, 100)
    assert R.check(c, emulate_fp32(c), fp32_path=True) < 0.5


# ---- the real-valued designs
@pytest.mark.parametrize("design", R.BOUNDED)
def test_bounded_designs_hold_with_room(design):
    worst = 0.0
    for epi in (dict(), dict(bias=True, resid=True, add2=True), dict(bias=True, scale_cols=64, scale=R.QSCALE)):
        c = R.make_case(design, 12, 70, 192, **epi)
        for order in _orders(192, 2):
            for form in ("wrap", "two"):
                worst = max(worst, R.check(c, emulate(c, order, form)))
    assert 0.0 < worst < 0.6, worst


# ---- wrong implementations
def _case_for(bug):
    if bug in ("bias_before_wrap",):
        return R.make_case("exact22", 9, 70, 64, bias=True), "wrap"
    if bug == "scale_on_resid":
        return R.make_case("exact22", 9, 70, 64, bias=True, resid=True, scale_cols=70, scale=0.125), "wrap"
    if bug == "scale_edge":
        return R.make_case("exact22", 9, 192, 64, bias=True, scale_cols=64, scale=0.125), "wrap"
    if bug == "relu_before_resid":
        return R.make_case("exact22", 9, 70, 64, resid=True, relu=True), "wrap"
    if bug == "pad_not_zeroed":
        return R.make_case("exact22", 9, 70, 100), "wrap"
    return None, "wrap"


BUGS = ("no_hi_lo", "no_lo_hi", "wrap_scale", "cursor_wrong_half", "halves_swapped", "lo_unscaled", "pad_not_zeroed",
        "bias_before_wrap", "scale_on_resid", "relu_before_resid", "scale_edge", "f16_operands")


@pytest.mark.parametrize("bug", BUGS)
def test_wrong_x3_products_are_rejected(bug):
    c, form = _case_for(bug)
    seen = []
    cases = [c] if c is not None else [R.make_case(d, 9, 70, 64) for d in ("exact22", "both", "place", "sparse")]
    for c in cases:
        assert R.check(c, emulate(c, form=form)) < 1.0               # the right implementation passes this very case
        try:
            R.check(c, emulate(c, form=form, bug=bug))
        except AssertionError:
            seen.append(c.design)
    # W's low half is empty in exact22 by design: a missing hi_x lo'_W^T shows in `both`, `place` and `sparse`
    want = {"no_hi_lo": {"both", "place", "sparse"}, "cursor_wrong_half": {"exact22", "both", "place", "sparse"}}.get(bug)
    if c is not None and len(cases) == 1:
        assert seen == [cases[0].design], (bug, seen)
    elif want:
        assert want <= set(seen), (bug, seen)
    else:
        assert {"exact22", "sparse"} <= set(seen) or {"both", "sparse"} <= set(seen), (bug, seen)


def test_sparse_bound_is_sharp():
    """a dropped cross term, a wrap scale of 2^-10 and f16 operands exceed the bound by two orders of magnitude"""
    c = R.make_case("sparse", 32, 70, 512)
    ref, bnd = R.reference(c), R.bound(c)
    assert (np.abs(emulate(c) - ref) / bnd).max() < 0.6
    for bug in ("no_hi_lo", "no_lo_hi", "wrap_scale", "f16_operands"):
        ratio = np.abs(emulate(c, bug=bug) - ref) / bnd
        assert (ratio > 1).mean() > 0.95 and np.median(ratio) > 50, (bug, float(np.median(ratio)))


def test_lo_from_the_unrounded_product_is_rejected():
    """the contraction the attention suite found: v = fl32(p q), but lo' taken from fma(p, q, -hi)"""
    r = np.random.default_rng(3)
    p, q = r.standard_normal(4096).astype(np.float32), np.float32(R.QSCALE)
    v = p * q
    hi, lo = R.split(v)
    R.assert_pair_is_split(v, hi, lo)
    lo_fused = ((p.astype(np.float64) * np.float64(q) - hi.astype(np.float64)) * 2048.0).astype(np.float16)
    with pytest.raises(AssertionError, match="lo'"):
        R.assert_pair_is_split(v, hi, lo_fused)
    with pytest.raises(AssertionError):
        R.assert_pair_consistent(hi, (lo.astype(np.float32) * 4).astype(np.float16))


def test_a_truncated_lo_is_rejected():
    """lo' cut where it should be rounded: at most one more unit of 2^-22, inside every product bound and invisible to the
    exact designs (their lo' is exact) — the split comparison is what sees it"""
    r = np.random.default_rng(4)
    v = (r.standard_normal((8, 64)) * 10.0 ** r.uniform(-3, 3, (8, 64))).astype(np.float32)
    hi, lo = R.split(v)
    rr = ((v - hi.astype(F32)) * F32(2048)).astype(np.float64)
    cut = np.where(np.abs(lo.astype(np.float64)) > np.abs(rr), np.nextafter(lo, np.float16(0)), lo).astype(np.float16)
    assert (cut != lo).mean() > 0.1
    with pytest.raises(AssertionError, match="lo'"):
        R.assert_pair_is_split(v, hi, cut)


def test_a_truncated_operand_on_the_fp32_path_is_rejected():
    c = R.make_case("place24", 9, 11, 37)
    with pytest.raises(AssertionError):
        R.check(c, emulate_fp32(c, trunc_bits=19))


def test_place_names_the_source():
    c = R.make_case("place", 9, 70, 64)
    got = R.reference(c).copy()
    got[3, 5] = got[3, 6]
    with pytest.raises(AssertionError, match="decodes to"):
        R.check(c, got)


# ---- LayerNorm pair and the FFN chain
def test_layernorm_pair_bound_and_consistency():
    r = np.random.default_rng(5)
    x = (r.standard_normal((7, 512)) * 3 + 1).astype(np.float32)
    g, b = (1 + 0.1 * r.standard_normal(512)).astype(np.float32), (0.1 * r.standard_normal(512)).astype(np.float32)
    n32 = G.ln_ref(x, g, b).astype(np.float32)
    hi, lo = R.split(n32)
    R.assert_pair_consistent(hi, lo)
    assert R.assert_bounded(G.ln_ref(x, g, b), R.ln_pair_bound(x, g, b), R.join(hi, lo)) < 1.0
    with pytest.raises(AssertionError):                              # hi alone is not the pair
        R.assert_bounded(G.ln_ref(x, g, b), R.ln_pair_bound(x, g, b), hi.astype(np.float64))


@pytest.mark.parametrize("D,F", ((64, 128), (512, 2048)))
def test_ffn_chain_design(D, F):
    c = R.FfnCase(33, D, F)
    h = c.hidden32()
    assert np.array_equal(h.astype(np.float64), c.pre_scale())
    hi, lo = R.split(h)
    assert (lo[h > 0] != 0).mean() > 0.9                             # wider than f16
    # second product on the pair, fp32 arithmetic, two orders: the reference bit for bit
    c2 = R.Case("exact22", c.M, D, F, h, c.w2, c.b2, c.x, None, False, 0, 1.0, 0, None, None, 0, 0.0)
    for order in _orders(R.round_up(F, 64), 1):
        assert np.array_equal(emulate(c2, order).astype(np.float64), c.reference())
    # a hidden that travels as f16 only is seen
    c3 = c2._replace(A=hi.astype(np.float32))
    assert (emulate(c3).astype(np.float64) != c.reference()).mean() > 0.5
    # the scaled hidden is a rounded fp32 number whose pair is its split; the product behind it holds the sparse bound
    cs = c.scaled_case(R.QSCALE)
    assert R.check(cs, emulate(cs)) < 0.6
