"""GPU: the Linear of the fp32 graph (csrc/engine_fp32.cpp Engine::gemm32) — math_mode 1 on k_fp32.hip gemm_f32_kernel,
math_mode 3 as the x3 product of (hi, lo') f16 operand pairs: the two-launch form on the short-input kernel (64 <= M <= 512),
the K-loop wrap of k_gemm.hip gemm_f16_pp3<2, *> (M > 512), the pair epilogue, split_x3_kernel, the LayerNorm that leaves as a
pair and the arena hand-over between them — against the exact-answer designs and the float64 reference of tests/x3_ref.py,
through stand-alone ops that call Engine::gemm32 / layernorm32 the way the layers do (engine_ops.cpp: op_linear32_ex,
op_split_x3, op_layernorm32, op_ffn32_ex, op_qkv32).  The ops are hostile hosts: every cell outside a matrix (rows behind the
last, the gap between width and row stride) holds +-2^100, the three x3 arenas are filled with 52 032 before the call, every
result sits in a sentinel-filled buffer that is checked for unwritten cells of [M, N] and for stores outside it (an fp32
result: no row at or beyond M, no column in [N, ldc); a pair: nothing outside [0, 2 Kp)).  Every case predicts its kernels
from a restatement of gemm32_impl's rule and launch_gemm's choice (below, _predict) and asserts what Engine.profile_kernel
names; every case is called twice and must return the same bits.  tests/test_x3_ref_cpu.py shows that the same assertions
reject fifteen wrong implementations.

Measured on an MI355X (run with -s: one line per bounded case, the worst per kernel and output at the end): all 49 tests pass,
every exact case bit-equal (exact22, both, place, dyadic, place24, the FFN chain, every split image, every pair against the
split of its fp32 value), no guard violation, every kernel as predicted; the file takes 6.5 s of wall time, the largest single
test (the 513 x 11 520 wrap case with more tiles than compute units, K = 192) 0.5 s.  Worst |err| / bound, bounds derived in
tests/x3_ref.py and not tuned:
    sparse (the sharp design; an fp32 emulation in four summation orders reaches 0.31, a dropped cross term 300):
        gemm_f16_pp3<2, 1|2> with the K-loop wrap 0.338    three products on one operand 0.329    operand pair in (FFN chain) 0.093
        two launches: gemm_small_kernel<8> + <16> 0.349, <16> + <32> 0.304, <24> + <48> 0.336, <64> + gemm_f16_pp3<2, 1> 0.263,
        <72> + gemm_f16_pp3<2, 1> 0.455
    normal (one fp32 ulp per term: the safety net): every x3 form <= 0.006    gemm_f32_kernel 0.052 (sparse 0.010)
    launch_layernorm, fp32 rows at D = 512, 560, 2048: 0.002    launch_layernorm_pair, hi + lo'/2048: 0.002
The sparse design holds f16-subnormal hi and lo' operands (0.5 % of its non-zeros lie below 2^-14, down to 1e-5): at a third
of the bound, the matrix core does not flush them.

Found in the kernels and the engine: nothing.  The seams M = 63 | 64 and 512 | 513, the shortest wrap (Kp = 64: k_wrap = 2 of 3
k-steps), a wrap with 450 tiles on 256 compute units, resid == out in both forms, ldr != ldc, the partial q-scale, the second
addend, pad columns at K = 100 and 560 over poisoned arenas, the pair epilogue in both of its code paths (interior and edge
tiles) with and without a scale in front of it, and the hand-over of a pair from layernorm32 or a producing product all return
the designs' bits.  No kernel on the benchmark's path changed (launch_gemm_f32 notes its name; the two-launch form of gemm32_impl
opens a nested profile class around its first launch, a no-op unless profiling is on).

Claims corrected: (1) "22 bits of mantissa" (k_fp32.hip, kernels.h launch_split_x3) holds for 2^-14 <= |x| < 65520 only — below,
hi and the scaled low part are both f16 subnormals and the error is up to 2^-36 absolute; the domain and the rows and columns
read and written by launch_gemm_f32, launch_split_x3 and launch_layernorm_pair are now stated in kernels.h.  (2) "hi ==
f16(hi + lo'/2048)" is not a property of a correct pair: a remainder just inside half an f16 ulp may round, as lo', onto the half
ulp itself, and the sum is then a tie that round-to-nearest-even may send to hi's neighbour (206 of 1.4 M random values over 12 decades);
x3_ref.assert_pair_consistent demands |lo'/2048| <= half an ulp of hi everywhere and hi == f16(hi + lo'/2048) wherever the sum
is not such a tie.  "Exact fp32 products" on v_mfma_f32_32x32x2_f32 stands: a one-term product of two 24-bit operands comes back
as the float64 product rounded once (place24, 16 shapes)."""
import math
import os
import re

import numpy as np
import pytest

import gemm_ref as G
import x3_ref as R
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

WORST = {}
F32K = "gemm_f32_kernel"
SMALL_MAX = 512                                                    # gemm_small_max_rows() with PF_SMALL_M unset


def _engine(mode):
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=5)), cmvn=W.synth_cmvn(), device=0, math_mode=mode)
    e.profile(True)
    return e


@pytest.fixture(scope="module")
def e1():
    e = _engine(1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def e3():
    e = _engine(3)
    yield e
    e.close()
    print("worst |err| / bound per kernel and output:")
    for k, v in sorted(WORST.items()):
        print("    %-70s %.3f" % (k, v))


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def test_the_dispatch_knobs_are_unset():
    """the predictions below restate the rules at their defaults"""
    for k in ("PF_SMALL_M", "PF_GEMM_MI_X", "PF_CU_CAP"):
        assert k not in os.environ, k


# ---- the rules, restated (not read from the run)
def _pp3(M, N, cus):
    """launch_gemm's tile height for an fp32-kind result: 128-row tiles where 256-row tiles would fill less than 0.6 of the
    compute units or need no fewer rounds"""
    t2, t1 = -(-M // 256) * -(-N // 128), -(-M // 128) * -(-N // 128)
    few = np.float32(t2) < np.float32(0.6) * np.float32(cus)
    rounds1 = 0.58 * -(-t1 // cus) < float(-(-t2 // cus))
    return 1 if (few or rounds1) else 2


def _short(M, N, Kd, cus, scaled):
    """a launch of depth Kd at M <= 512: the short-input kernel where it applies (one launch up to Kd = 576; the split path needs
    N = 512, no scale and S round_up(M, 128) <= 4096 workspace rows), otherwise gemm_f16_pp3"""
    if Kd <= 576:
        return "gemm_small_kernel<%d>, %d-row bricks" % (Kd // 8, 96 if Kd > 512 else 128)
    nkb = Kd // 64
    S = next((s for s in range(2, nkb + 1) if nkb % s == 0 and (nkb // s) * 64 <= 256), 0)
    if S and N == 512 and not scaled and S * -(-M // 128) * 128 <= 4096:
        return "gemm_small_kernel<%d>, split %d + small_reduce_kernel" % (Kd // S // 8, S)
    return "gemm_f16_pp3<2, %d>" % _pp3(M, N, cus)


def _predict(mode, M, N, K, ldw, ldc, ldr, resid, scale_cols, cus):
    """gemm32_impl: the kernels of one Linear, in launch order"""
    part = 0 < scale_cols < N
    x3 = (mode == 3 and M >= 64 and ldw == K and (not part or (scale_cols % 64 == 0 and M > SMALL_MAX)) and ldc % 4 == 0
          and (not resid or ldr % 4 == 0))
    if not x3:
        return (F32K,)
    Kp = R.round_up(K, 64)
    if M > SMALL_MAX:
        return ("gemm_f16_pp3<2, %d>" % _pp3(M, N, cus),)
    return (_short(M, N, Kp, cus, scale_cols > 0), _short(M, N, 2 * Kp, cus, True))


def _lin(eng, mode, cus, c, alias=False, lda=0, ldw=0, ldc=0, ldr=0, expect=None):
    """one Linear through pf_op_linear32_ex: the predicted kernels, the design's assertion, the same bits from a second call"""
    eldc = ldc or R.round_up(c.N, 4)
    names = _predict(mode, c.M, c.N, c.K, ldw or c.K, eldc, eldc if alias else (ldr or eldc), c.resid is not None, c.scale_cols, cus)
    if expect is not None:
        assert names[-1].startswith(expect), (names, expect)      # the case is on the path it was written for
    what = "mode %d %s M %d N %d K %d bias %d resid %d alias %d resid2 %d relu %d scale %d x %g ld %d %d %d %d" % (
        mode, c.design, c.M, c.N, c.K, c.bias is not None, c.resid is not None, alias, c.add2 is not None, c.relu, c.scale_cols, c.scale,
        lda, ldw, ldc, ldr)
    kw = dict(bias=c.bias, resid=c.resid, resid2=c.add2, relu=c.relu, scale_cols=c.scale_cols, scale=c.scale, lda=lda, ldw=ldw, ldc=ldc, ldr=ldr,
              resid_aliases_out=alias)
    eng.profile_reset()
    got = eng.op_linear32_ex(c.A, c.W, **kw)
    ran = (eng.profile_kernel("gemm32_x3_main"), eng.profile_kernel("gemm32_op"))
    assert ran == (names if len(names) == 2 else ("",) + names), "%s: ran %r, expected %r" % (what, ran, names)
    ratio = R.check(c, got, what + " [" + " + ".join(names) + "]", fp32_path=names == (F32K,))
    if c.design in R.BOUNDED:
        print("%s [%s]: |err| / bound = %.3f" % (what, " + ".join(names), ratio))
        _note("%s, %s" % (" + ".join(re.sub(r", (\d+-row bricks|split .*)$", "", n) for n in names), c.design), ratio)
    assert np.array_equal(eng.op_linear32_ex(c.A, c.W, **kw), got), what + ": a second call returned other bits"
    return got


# =============================================================================== gemm_f32_kernel
F32_SHAPES = ((1, 1, 1), (1, 64, 2), (63, 65, 31), (63, 64, 32), (64, 1, 33), (64, 515, 100), (65, 65, 560), (129, 64, 32), (129, 515, 33),
              (65, 1, 560), (1, 515, 100), (63, 1, 2), (129, 65, 31), (64, 64, 1), (65, 515, 2), (129, 1, 100))
F32_EPI = (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, resid=True), dict(resid=True, relu=True),
           dict(bias=True, resid=True, scale_cols=10 ** 6, scale=0.125))


@pytest.mark.parametrize("i", range(len(F32_SHAPES)))
def test_gemm_f32_kernel_shapes_strides_and_epilogues(e1, cus, i):
    M, N, K = F32_SHAPES[i]
    epi = dict(F32_EPI[i % len(F32_EPI)])
    if "scale_cols" in epi:
        epi["scale_cols"] = N                                       # full scale
    wide = dict(lda=K + 3, ldw=K + 5, ldc=N + 7, ldr=N + 2)
    _lin(e1, 1, cus, R.make_case("dyadic", M, N, K, **epi), expect=F32K, **wide)
    _lin(e1, 1, cus, R.make_case("dyadic", M, N, K, **epi), expect=F32K)
    _lin(e1, 1, cus, R.make_case("place24", M, N, K), expect=F32K, **wide)
    if epi.get("resid"):
        _lin(e1, 1, cus, R.make_case("dyadic", M, N, K, **epi), alias=True, expect=F32K, lda=K + 1, ldc=N + 7)
    _lin(e1, 1, cus, R.make_case("exact22", M, N, K, bias=True, resid=True), alias=True, expect=F32K)


@pytest.mark.parametrize("scale_cols", (1, 64, 192))
def test_gemm_f32_kernel_scales(e1, cus, scale_cols):
    for M, K in ((63, 100), (129, 33)):
        _lin(e1, 1, cus, R.make_case("dyadic", M, 192, K, bias=True, resid=True, scale_cols=scale_cols, scale=0.125), expect=F32K, ldc=196, ldr=200)
        _lin(e1, 1, cus, R.make_case("exact22", M, 192, K, bias=True, relu=True, scale_cols=scale_cols, scale=0.125), expect=F32K)
        _lin(e1, 1, cus, R.make_case("normal", M, 192, K, bias=True, resid=True, scale_cols=scale_cols, scale=R.QSCALE), expect=F32K)
    _lin(e1, 1, cus, R.make_case("normal", 129, 515, 560, bias=True, resid=True, relu=True), expect=F32K)
    _lin(e1, 1, cus, R.make_case("sparse", 129, 515, 560, bias=True), expect=F32K)


def test_gemm_f32_kernel_second_addend(e1, cus):
    """resid2 is added by launch_add_f32 over contiguous rows; any other layout is refused"""
    from aliparaformerasr_amd import _native as N
    for M, Nn, K in ((65, 65, 33), (129, 64, 100)):
        c = R.make_case("dyadic", M, Nn, K, bias=True, resid=True, add2=True)
        _lin(e1, 1, cus, c, expect=F32K, ldc=Nn, ldr=Nn)
        with pytest.raises(N.PfError, match="contiguous rows"):
            e1.op_linear32_ex(c.A, c.W, bias=c.bias, resid=c.resid, resid2=c.add2, ldc=Nn + 4, ldr=Nn + 4)
    _lin(e1, 1, cus, R.make_case("dyadic", 65, 65, 33, bias=True), expect=F32K)      # the engine is usable after the refusal


# =============================================================================== split_x3_kernel
def _special_values():
    f = np.float32
    v = [0.0, -0.0, 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, float(np.nextafter(f(65520.0), f(0))), 2.0 ** -25, 3 * 2.0 ** -25,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -10 + 2.0 ** -11, 2048 + 1.0, 2048 + 3.0,          # hi ties (to even, both ways)
         1 + 2.0 ** -12 + 2.0 ** -23, 1 + 2.0 ** -22, 1 + 3 * 2.0 ** -22, 1 + 5 * 2.0 ** -23,              # lo' ties and just off them
         1 + 2.0 ** -23, 2 - 2.0 ** -23, 1.0 / 3, 0.1, 1e-3, 6.1e-5, 6.0e-5, 1e-7, 1e-10, 1e-20,
         float(np.finfo(f).tiny), float(np.finfo(f).tiny) / 2, 1e-45, 7e-42]                               # fp32 subnormals
    v = np.array(v, np.float64)
    return np.concatenate([v, -v]).astype(np.float32)


def _canon(img):
    """-0 and +0 are the same operand"""
    return np.where(img == 0x8000, 0, img)


@pytest.mark.parametrize("K", (1, 3, 64, 100, 560))
def test_split_x3_kernel(e3, K):
    r = np.random.default_rng(K)
    sp = _special_values()
    rows = max(-(-sp.size // K) + 1, 100_000 // K // (8 if K < 64 else 1) + 1)
    x = (r.standard_normal(rows * K) * 10.0 ** r.uniform(-8, 4, rows * K)).astype(np.float32)
    x = np.where(np.abs(x) < 65000.0, x, np.float32(1.5))
    x[:sp.size] = sp
    x = x.reshape(rows, K)
    for swap in (0, 1):
        for Kp, ldx, ldo in ((R.round_up(K, 64), 0, 0), (R.round_up(K, 64), K + 3, 2 * R.round_up(K, 64) + 8), (R.round_up(K, 4), K + 1, 0)):
            got = e3.op_split_x3(x, Kp, ldx=ldx, ldo=ldo, swap=swap)
            want = R.split_image(x, K, Kp, ldo or 2 * Kp, swap, 0x7E5A)
            bad = _canon(got) != _canon(want)
            if bad.any():
                i = tuple(int(t) for t in np.argwhere(bad)[0])
                raise AssertionError("K %d Kp %d swap %d ldx %d ldo %d: %d cells differ, first at %r: got %#x, want %#x" % (
                    K, Kp, swap, ldx, ldo, int(bad.sum()), i, int(got[i]), int(want[i])))
            assert np.array_equal(e3.op_split_x3(x, Kp, ldx=ldx, ldo=ldo, swap=swap), got)


# =============================================================================== LayerNorm
def _ln_params(D, seed):
    r = np.random.default_rng(seed)
    return (1 + 0.1 * r.standard_normal(D)).astype(np.float32), (0.1 * r.standard_normal(D)).astype(np.float32)


def _ln_rows(M, D, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal((M, D)) * 10.0 ** r.uniform(-1, 1, (M, 1)) + r.standard_normal((M, 1))).astype(np.float32)


@pytest.mark.parametrize("D", (512, 560, 2048))
def test_layernorm_fp32_rows(e1, D):
    for M in (7, 515):
        x = _ln_rows(M, D, D + M)
        g, b = _ln_params(D, D)
        out, pair, _ = e1.op_layernorm32(x, g, b)
        assert pair is None
        ratio = R.assert_bounded(G.ln_ref(x, g, b), G.ln_bound(x, g, b), out, "layernorm fp32 D %d M %d" % (D, M))
        print("launch_layernorm fp32 D %d M %d: |err| / bound = %.3f" % (D, M, ratio))
        _note("launch_layernorm, fp32 rows", ratio)
        assert np.array_equal(e1.op_layernorm32(x, g, b)[0], out)


@pytest.mark.parametrize("M", (1, 7, 513, 515))
def test_layernorm_pair(e3, M):
    x = _ln_rows(M, 512, M)
    g, b = _ln_params(512, M)
    _, (hi, lo), _ = e3.op_layernorm32(x, g, b, direct_pair=True)
    R.assert_pair_consistent(hi, lo, "layernorm pair M %d" % M)
    ratio = R.assert_bounded(G.ln_ref(x, g, b), R.ln_pair_bound(x, g, b), R.join(hi, lo), "layernorm pair M %d" % M)
    print("launch_layernorm_pair M %d: |err| / bound = %.3f" % (M, ratio))
    _note("launch_layernorm_pair, hi + lo'/2048", ratio)
    hi2, lo2 = e3.op_layernorm32(x, g, b, direct_pair=True)[1]
    assert np.array_equal(hi2.view(np.uint16), hi.view(np.uint16)) and np.array_equal(lo2.view(np.uint16), lo.view(np.uint16))
    # Engine::layernorm32 writes the pair above the short-input threshold and fp32 rows at or below it
    out, pair, _ = e3.op_layernorm32(x, g, b)
    if M > SMALL_MAX:
        assert out is None and np.array_equal(pair[0].view(np.uint16), hi.view(np.uint16)) and np.array_equal(pair[1].view(np.uint16), lo.view(np.uint16))
    else:
        assert pair is None
        R.assert_bounded(G.ln_ref(x, g, b), G.ln_bound(x, g, b), out, "layernorm32 fp32 rows M %d" % M)


def test_layernorm_pair_feeds_the_product(e3, cus):
    """layernorm32 -> gemm32 as enc_layer_fp32 runs them: the pair in the arena is the operand.  The product of the returned pair
    (an exact 22-bit number per cell) with W in {+-1, +-2} under the dense bound"""
    M, D, Nn = 513, 512, 192
    x = _ln_rows(M, D, 77)
    g, b = _ln_params(D, 77)
    w = R.make_case("exact22", 4, Nn, D, bias=True)
    e3.profile_reset()
    out, (hi, lo), y = e3.op_layernorm32(x, g, b, W=w.W, bias=w.bias)
    assert out is None and e3.profile_kernel("gemm32_op") == _predict(3, M, Nn, D, D, Nn, Nn, False, 0, cus)[0]
    a = R.join(hi, lo).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), R.join(hi, lo))
    c = R.Case("normal", M, Nn, D, a, w.W, w.bias, None, None, False, 0, 1.0, 0, None, None, 0, 0.0)
    ratio = R.check(c, y, "layernorm32 -> gemm32")
    print("layernorm32 -> gemm32 M %d: |err| / bound = %.3f" % (M, ratio))
    _note("layernorm32 -> gemm_f16_pp3<2, *> (K-loop wrap), normal", ratio)
    # at or below the threshold the fp32 rows are the operand of the two-launch form
    x = x[:65]
    out, pair, y = e3.op_layernorm32(x, g, b, W=w.W, bias=w.bias)
    assert pair is None
    c = R.Case("normal", 65, Nn, D, out, w.W, w.bias, None, None, False, 0, 1.0, 0, None, None, 0, 0.0)
    R.check(c, y, "layernorm32 -> gemm32 (two-launch)")


# =============================================================================== x3 products
X3_K = (64, 100, 192, 512, 560)
X3_N = ((64, 0), (192, 0), (515, 516), (1536, 0))
X3_EPI = (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, resid=True), dict(bias=True, resid=True, alias=True),
          dict(bias=True, resid=True, add2=True), dict(resid=True, relu=True), dict(bias=True, add2=True, relu=True))


def _x3_cases(M, ki):
    """two designs per (M, K), N, design and epilogue rotated so that every M meets every N, design and epilogue"""
    K = X3_K[ki]
    mi = (64, 65, 512, 513, 769).index(M)
    for j in range(2):
        t = 2 * (ki + mi) + j
        yield K, X3_N[(ki + mi + j) % 4], ("exact22", "both", "place", "sparse", "normal")[t % 5], dict(X3_EPI[(t + mi) % len(X3_EPI)])


@pytest.mark.parametrize("M", (64, 65, 512, 513, 769))
def test_x3_products(e3, cus, M):
    form = "gemm_f16_pp3<2" if M > SMALL_MAX else ""
    for ki in range(len(X3_K)):
        for K, (Nn, ldc), design, epi in _x3_cases(M, ki):
            alias = epi.pop("alias", False)
            _lin(e3, 3, cus, R.make_case(design, M, Nn, K, **epi), alias=alias, ldc=ldc, lda=K + 4 if ki % 2 else 0, expect=form)
    # full scale: 2^-3 exact, 128^-0.5 bounded
    for K, Nn in ((100, 192), (512, 64)):
        _lin(e3, 3, cus, R.make_case("exact22", M, Nn, K, bias=True, resid=True, scale_cols=Nn, scale=0.125), expect=form)
        _lin(e3, 3, cus, R.make_case("sparse", M, Nn, K, bias=True, scale_cols=Nn, scale=R.QSCALE), expect=form)
    # the q-scale of the fused Q | K | V product: x3 above the threshold, the fp32 matrix path at or below it
    part = form if M > SMALL_MAX else F32K
    _lin(e3, 3, cus, R.make_case("exact22", M, 1536, 64, bias=True, scale_cols=512, scale=0.125), expect=part)
    _lin(e3, 3, cus, R.make_case("sparse", M, 1536, 192, bias=True, scale_cols=512, scale=R.QSCALE), expect=part)


def test_x3_deep_k(e3, cus):
    for design, epi in (("exact22", dict(bias=True, resid=True)), ("place", dict()), ("sparse", dict(bias=True, relu=True))):
        _lin(e3, 3, cus, R.make_case(design, 513, 192, 2048, **epi), expect="gemm_f16_pp3<2")
    _lin(e3, 3, cus, R.make_case("exact22", 512, 512, 2048, bias=True), expect="gemm_f16_pp3<2")     # two launches; 2 Kp = 4096 has no short-input form
    _lin(e3, 3, cus, R.make_case("exact22", 512, 512, 1024, bias=True), expect="gemm_f16_pp3<2")
    _lin(e3, 3, cus, R.make_case("exact22", 128, 512, 1024, bias=True, add2=True, resid=True), expect="gemm_f16_pp3<2")


@pytest.mark.parametrize("K", (64, 192))
def test_x3_wrap_with_several_tiles_per_workgroup(e3, cus, K):
    """more tiles than compute units: the issue-side cursor crosses from one tile's main phase into the next tile's cross phase
    while the consume side is still S - 1 or S steps behind.  K = 64: k_wrap = 2 of nk = 3, the shortest wrap there is"""
    M = 513
    Nn = 128 * math.ceil(1.05 * cus / -(-M // 256))
    rows = 128 * _pp3(M, Nn, cus)
    assert -(-M // rows) * (Nn // 128) > cus
    _lin(e3, 3, cus, R.make_case("exact22", M, Nn, K, bias=True, resid=True, relu=True), expect="gemm_f16_pp3<2, %d>" % (rows // 128))
    _lin(e3, 3, cus, R.make_case("place", M, Nn, K), expect="gemm_f16_pp3<2, %d>" % (rows // 128))


def test_x3_fallbacks_by_name(e3, cus):
    """every documented condition under which math_mode 3 runs a Linear on the fp32 matrix path"""
    mk = lambda M, Nn=192, K=100, **kw: R.make_case("exact22", M, Nn, K, bias=True, **kw)
    _lin(e3, 3, cus, mk(63), expect=F32K)                                                    # M < 64
    _lin(e3, 3, cus, mk(64), expect="gemm_small_kernel")                                     # (the seam's other side)
    _lin(e3, 3, cus, mk(65), ldw=104, expect=F32K)                                           # ldw != K
    _lin(e3, 3, cus, mk(513), ldw=104, expect=F32K)
    _lin(e3, 3, cus, mk(65), ldc=193, expect=F32K)                                           # ldc % 4
    _lin(e3, 3, cus, mk(513, resid=True), ldc=196, ldr=194, expect=F32K)                     # ldr % 4
    _lin(e3, 3, cus, mk(513, resid=True), ldc=196, ldr=200, expect="gemm_f16_pp3<2")         # (ldr != ldc alone is no reason)
    _lin(e3, 3, cus, mk(512, scale_cols=64, scale=0.125), expect=F32K)                       # partial scale with M <= 512
    _lin(e3, 3, cus, mk(513, scale_cols=64, scale=0.125), expect="gemm_f16_pp3<2")
    _lin(e3, 3, cus, mk(513, scale_cols=1, scale=0.125), expect=F32K)                        # partial scale, scale_cols % 64
    _lin(e3, 3, cus, R.make_case("dyadic", 63, 65, 33, bias=True, resid=True, add2=True), ldc=65, ldr=65, expect=F32K)   # resid2 on the fallback
    _lin(e3, 3, cus, R.make_case("normal", 63, 192, 100, bias=True, resid=True), expect=F32K)


def test_x3_other_weights_at_the_same_address(e3, cus):
    """the ops drop the cached pair image of their weights (x3_forget): a second product at the same address uses its own"""
    for M in (65, 513):
        for seed in (0, 1, 2):
            _lin(e3, 3, cus, R.make_case("both", M, 192, 100, bias=True, seed=seed))


# ---- the FFN chain: pair epilogue -> operand pair
def _ffn_names(M, D, F, cus):
    return _predict(3, M, F, D, D, F, F, False, 0, cus)[-1], _predict(3, M, D, F, F, D, D, True, 0, cus)[-1]


@pytest.mark.parametrize("D,F", ((64, 128), (512, 2048)))
def test_ffn_chain(e3, e1, cus, D, F):
    M = 513
    c = R.FfnCase(M, D, F)
    e3.profile_reset()
    y, pair = e3.op_ffn32_ex(c.x, c.w1, c.b1, c.w2, c.b2)
    assert (e3.profile_kernel("gemm32_ffn1"), e3.profile_kernel("gemm32_ffn2")) == _ffn_names(M, D, F, cus)
    assert pair is not None, "the hidden did not travel as an operand pair"
    R.assert_pair_is_split(c.hidden32(), pair[0], pair[1], "FFN hidden pair D %d F %d" % (D, F))
    R.assert_exact(None, c.reference(), y, "FFN chain D %d F %d" % (D, F))
    y2, pair2 = e3.op_ffn32_ex(c.x, c.w1, c.b1, c.w2, c.b2)
    assert np.array_equal(y2, y) and np.array_equal(pair2[1].view(np.uint16), pair[1].view(np.uint16))
    assert np.array_equal(e3.op_ffn32(c.x, c.w1, c.b1, c.w2, c.b2), y)
    # a scaled hidden is a rounded fp32 number: its pair must be the split of THAT number (no contraction into the subtraction)
    y, pair = e3.op_ffn32_ex(c.x, c.w1, c.b1, c.w2, c.b2, hidden_scale=R.QSCALE)
    R.assert_pair_is_split(c.hidden32(R.QSCALE), pair[0], pair[1], "scaled FFN hidden pair D %d F %d" % (D, F))
    ratio = R.check(c.scaled_case(R.QSCALE), y, "FFN chain behind a scaled hidden")
    print("FFN chain D %d F %d, hidden x 128^-0.5: |err| / bound = %.3f" % (D, F, ratio))
    _note("gemm_f16_pp3<2, *> (operand pair in), sparse", ratio)
    # at the threshold's other side and in math_mode 1 the hidden is an fp32 matrix
    for eng, m in ((e3, 64), (e3, 512), (e1, 65)):
        cs = R.FfnCase(m, D, F)
        y, pair = eng.op_ffn32_ex(cs.x, cs.w1, cs.b1, cs.w2, cs.b2)
        assert pair is None
        R.assert_exact(None, cs.reference(), y, "FFN chain M %d D %d F %d" % (m, D, F))


# ---- Q, K, V on one operand
@pytest.mark.parametrize("M,D,K", ((513, 128, 100), (513, 512, 512), (65, 128, 192)))
def test_qkv_triple_against_the_fused_product(e3, cus, M, D, K):
    for design, s in (("exact22", 0.125), ("sparse", R.QSCALE)):
        c = R.make_case(design, M, 3 * D, K, bias=True, scale_cols=D, scale=s)
        e3.profile_reset()
        got = e3.op_qkv32(c.A, c.W, c.bias, s)
        one = _predict(3, M, D, K, K, D, D, False, D, cus)[-1]
        assert [e3.profile_kernel("gemm32_op_" + t) for t in "qkv"] == [one] * 3
        what = "qkv triple %s M %d D %d K %d" % (design, M, D, K)
        ratio = R.check(c, got, what)
        assert np.array_equal(e3.op_qkv32(c.A, c.W, c.bias, s), got), what + ": a second call returned other bits"
        fused = _lin(e3, 3, cus, c)
        if M > SMALL_MAX:                                            # the same x3 accumulation per cell, bit for bit
            assert np.array_equal(fused, got), what + ": the three products differ from the fused one"
        if design == "sparse":
            _note("three products on one operand, sparse", ratio)
