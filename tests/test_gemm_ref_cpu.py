"""CPU: the designs of tests/gemm_ref.py keep what they promise (caps, f16-representable operands, every `ties` result a tie,
finite f16 results), the float64 reference equals fp32 arithmetic in three summation orders bit for bit, and the assertions
the GPU suite uses reject fourteen wrong GEMMs written in numpy, each at the smallest shape of its design."""
import numpy as np
import pytest

import gemm_ref as R

SHAPES = ((64, 128, 64), (129, 515, 576), (300, 256, 2048))


def _f32_sum(A, W, order):
    """A W^T accumulated in fp32: products are formed exactly (float64 of f16 values), every partial sum is rounded to fp32"""
    K = A.shape[1]
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    if order == "forward":
        ks = [np.arange(k, k + 1) for k in range(K)]
    elif order == "reverse":
        ks = [np.arange(k, k + 1) for k in range(K - 1, -1, -1)]
    else:                                                     # 16-wide blocks (an MFMA's depth), each summed pairwise, then chained
        ks = [np.arange(k, min(k + 16, K)) for k in range(0, K, 16)]
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for idx in ks:
        part = [(A64[:, k:k + 1] * W64[:, k][None, :]).astype(np.float32) for k in idx]
        while len(part) > 1:
            part = [(part[i] + part[i + 1]) if i + 1 < len(part) else part[i] for i in range(0, len(part), 2)]
        acc = acc + part[0]
    return acc


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dyadic_reference_equals_fp32_in_three_orders(M, N, K):
    if K == 2048:
        M, N = 40, 48                                         # the chained fp32 sums are slow in numpy; the cap is what matters
    c = R.make_case("dyadic", M, N, K)
    assert c.cap < R.CAP
    ref = c.A.astype(np.float64) @ c.W.astype(np.float64).T
    for order in ("forward", "reverse", "blocked"):
        assert np.array_equal(_f32_sum(c.A, c.W, order).astype(np.float64), ref), order


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dyadic_caps_and_nontrivial_rounding(M, N, K):
    c = R.make_case("dyadic", M, N, K, bias=True, resid=True, add2=True)
    assert c.cap < R.CAP and R.is_f16(c.A) and R.is_f16(c.W)
    for t in (c.bias, c.resid, c.add2):
        assert np.array_equal(np.round(t.astype(np.float64) * 1024), t.astype(np.float64) * 1024)
    exact = R.reference(c)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)          # fits fp32
    half = R.reference(c._replace(out_kind=1))
    assert np.isfinite(half).all() and (half != exact).mean() > 0.5                   # the f16 rounding has work to do


def test_dyadic_fsmn_stays_on_the_grid():
    c = R.make_case("dyadic", 249, 512, 512, bias=True, resid=True, fsmn=(3, 83))
    assert c.cap < R.CAP and R.is_f16(c.V)
    ref = R.reference(c)
    assert np.array_equal(np.round(ref * 1024), ref * 1024) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)


@pytest.mark.parametrize("M,N,K", ((33, 64, 64), (300, 515, 576)))
def test_every_ties_result_is_a_tie(M, N, K):
    c = R.make_case("ties", M, N, K, out_kind=1)
    assert R.is_f16(c.A) and R.is_f16(c.W)
    v = c.A.astype(np.float64) @ c.W.astype(np.float64).T
    a = np.abs(v)
    assert ((a >= 2049) & (a <= 4095) & (a % 2 == 1)).all()
    lo, hi = np.sign(v) * (a - 1), np.sign(v) * (a + 1)
    assert R.is_f16(lo) and R.is_f16(hi)                      # the two neighbours, one apart on either side
    even = np.where((a - 1) % 4 == 0, lo, hi)                 # f16 values are 2 apart here: the even mantissa is the multiple of 4
    assert np.array_equal(R.reference(c), even)
    assert (v > 0).any() and (v < 0).any() and ((a - 1) % 4 == 0).any() and ((a + 1) % 4 == 0).any()


def test_place_names_the_source():
    c = R.make_case("place", 70, 96, 128)
    ref = R.reference(c)
    assert np.array_equal(ref, c.W.astype(np.float64)[:, (R.PLACE_P * np.arange(70)) % 128].T) and R.is_f16(c.W)
    with pytest.raises(AssertionError, match=r"W\[n 5, k 74\]"):      # row 3 delivered as row 2: k = 74 instead of 111
        got = ref.copy()
        got[3] = ref[2]
        got[3, :5] = ref[3, :5]
        R.assert_exact(c, ref, got, "swap")


@pytest.mark.parametrize("M", (1, 65))
def test_int_design_keeps_its_caps(M):
    for resid in (False, True):
        c = R.make_ffn_case(M, resid)
        assert c.cap < 2.0 ** 24
        y = R.ffn_reference(c)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.array_equal(np.round(y), y)
        h = np.maximum(c.x.astype(np.float64) @ c.w1.astype(np.float64).T + c.b1, 0)
        assert (h == 0).mean() > 0.1 and h.max() > 512       # ReLU both ways, hidden values that need their 11 bits


def test_non_power_of_two_scale_formula():
    s = R.QSCALE
    c = R.make_case("dyadic", 33, 128, 64, bias=True, scale_cols=64, scale=s, out_kind=1)
    v = (c.A.astype(np.float64) @ c.W.astype(np.float64).T + c.bias)[:, :64]
    want = (v.astype(np.float32) * np.float32(s)).astype(np.float16).astype(np.float64)
    assert np.array_equal(R.reference(c)[:, :64], want)


# ------------------------------------------------------------------------------------------------ mutants
def _blocked(x, transpose_block=False):
    """store [M, N] into the blocked layout and read it back; transpose_block: each 32 x 8 block written column-major"""
    M, N = x.shape
    Mp = -(-M // 32) * 32
    full = np.zeros((Mp, N))
    full[:M] = x
    blocks = full.reshape(Mp // 32, 32, N // 8, 8).transpose(0, 2, 1, 3)             # [mb, nb, 32, 8]
    if transpose_block:
        blocks = blocks.transpose(0, 1, 3, 2).reshape(blocks.shape)
    return blocks.transpose(0, 2, 1, 3).reshape(Mp, N)[:M]


def _trunc16(v):
    h = R.f16(v)
    over = np.abs(h) > np.abs(v)
    return np.where(over, np.nextafter(h.astype(np.float16), np.float16(0)).astype(np.float64), h)


def wrong_gemm(c, bug=None):
    """the GEMM + epilogue in numpy, with one bug"""
    A, W = c.A.astype(np.float64), c.W.astype(np.float64)
    if bug == "w_transposed":
        v = A @ W
    elif bug == "k_column_dropped":
        keep = np.arange(c.K) != c.K // 3
        v = A[:, keep] @ W[:, keep].T
    elif bug == "last_k_step_dropped":
        v = A[:, :c.K - 64] @ W[:, :c.K - 64].T
    elif bug == "f16_accumulation":
        v = np.zeros((c.M, c.N), np.float16)
        for k in range(c.K):
            v = (v.astype(np.float64) + A[:, k:k + 1] * W[:, k][None, :]).astype(np.float16)
        v = v.astype(np.float64)
    else:
        v = A @ W.T
    bias = None if c.bias is None else c.bias.astype(np.float64)
    if bug == "bias_f16" and bias is not None:
        bias = R.f16(bias)
    ncols = c.scale_cols + (64 if bug == "scale_one_group_too_far" else 0)
    s = np.float64(np.float32(c.scale))
    if bug == "scale_before_bias" and c.scale_cols:
        v[:, :ncols] *= s
    if bias is not None:
        v = v + bias * (2 if bug == "bias_twice" else 1)
    if bug != "scale_before_bias" and c.scale_cols:
        v[:, :ncols] *= s
    if c.add2 is not None:
        v = v + c.add2
    if c.V is not None:
        taps = c.taps[:, ::-1] if bug == "fsmn_taps_reversed" else c.taps
        v = v + R.fsmn_terms(c.V, taps, c.M if bug == "fsmn_across_utterances" else c.T)[0]
    if bug == "relu_before_resid" and c.relu:
        v = np.maximum(v, 0)
    if c.resid is not None:
        v = v + c.resid
    if bug != "relu_before_resid" and c.relu:
        v = np.maximum(v, 0)
    if c.out_kind:
        v = _trunc16(v) if bug == "f16_truncation" else R.f16(v)
    if bug == "rows_swapped":
        idx = np.arange(c.M) ^ 1
        idx[idx >= c.M] = c.M - 1
        v = v[idx]
    if bug == "block_transposed":
        v = _blocked(v, True)
    elif c.out_kind == 2:
        v = _blocked(v)
    return v


# bug -> the cases (design, M, N, K, epilogue) that must reject it: the smallest shape of the design that exercises it
MUTANTS = {
    "w_transposed": [("place", 64, 64, 64, {}), ("dyadic", 64, 64, 64, {})],
    "k_column_dropped": [("dyadic", 1, 64, 64, {}), ("place", 64, 64, 64, {})],
    "last_k_step_dropped": [("dyadic", 1, 64, 128, {}), ("place", 4, 64, 128, {}), ("ties", 64, 64, 128, dict(out_kind=1))],
    "bias_twice": [("dyadic", 1, 64, 64, dict(bias=True)), ("place", 1, 64, 64, dict(bias=True))],
    "bias_f16": [("dyadic", 1, 64, 64, dict(bias=True))],
    "relu_before_resid": [("dyadic", 1, 64, 64, dict(resid=True, relu=True))],
    "scale_before_bias": [("dyadic", 1, 128, 64, dict(bias=True, scale_cols=64, scale=0.125))],
    "scale_one_group_too_far": [("dyadic", 1, 128, 64, dict(bias=True, scale_cols=64, scale=0.125))],
    "f16_truncation": [("dyadic", 1, 64, 64, dict(out_kind=1)), ("ties", 2, 64, 64, dict(out_kind=1))],
    "f16_accumulation": [("dyadic", 1, 64, 64, {})],
    "rows_swapped": [("place", 2, 64, 64, {}), ("dyadic", 2, 64, 64, {})],
    "block_transposed": [("place", 32, 64, 64, dict(out_kind=2)), ("dyadic", 32, 64, 64, dict(out_kind=2))],
    "fsmn_across_utterances": [("dyadic", 14, 512, 64, dict(fsmn=(2, 7)))],
    "fsmn_taps_reversed": [("dyadic", 14, 512, 64, dict(fsmn=(2, 7)))],
}


@pytest.mark.parametrize("bug", sorted(MUTANTS))
def test_the_assertion_rejects_the_mutant(bug):
    for design, M, N, K, epi in MUTANTS[bug]:
        c = R.make_case(design, M, N, K, **epi)
        R.check(c, wrong_gemm(c), "the numpy GEMM itself")                          # the harness is right without the bug
        with pytest.raises(AssertionError, match="first at"):
            R.check(c, wrong_gemm(c, bug), bug)


@pytest.mark.parametrize("bug", ("k_column_dropped", "bias_twice", "f16_accumulation", "rows_swapped", "scale_before_bias"))
def test_the_bound_of_the_normal_design_rejects_the_mutant(bug):
    c = R.make_case("normal", 33, 128, 64, bias=True, resid=True, scale_cols=64, scale=0.125)
    assert R.check(c, wrong_gemm(c), "numpy") < 0.01                                # float64 arithmetic sits far inside the bound
    with pytest.raises(AssertionError, match="out of bound"):
        R.check(c, wrong_gemm(c, bug), bug)


def test_ln_bound_admits_fp32_and_rejects_a_biased_variance():
    r = np.random.default_rng(3)
    x = R.reference(R.make_case("dyadic", 65, 512, 512, bias=True, resid=True))
    g, b = 1 + 0.1 * r.standard_normal(512), 0.1 * r.standard_normal(512)
    ref, bnd = R.ln_ref(x, g, b), R.ln_bound(x, g, b)
    x32 = x.astype(np.float32)
    mu = x32.mean(axis=1, keepdims=True, dtype=np.float32)
    d = x32 - mu
    got = d / np.sqrt((d * d).mean(axis=1, keepdims=True, dtype=np.float32) + np.float32(1e-12)) * g.astype(np.float32) + b.astype(np.float32)
    assert R.assert_bounded(ref, bnd, got, "fp32 LayerNorm") < 1.0
    assert R.assert_bounded(ref, R.ln_bound(x, g, b, half=True), R.f16(got), "f16 copy") < 1.0
    d64 = x - x.mean(axis=1, keepdims=True)
    wrong = d64 / np.sqrt((d64 ** 2).sum(axis=1, keepdims=True) / 511 + 1e-12) * g + b           # unbiased variance
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_bounded(ref, bnd, wrong, "n - 1")
