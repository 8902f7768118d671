"""GPU: the GEMM family (csrc/k_gemm.hip gemm_f16_pp3<1|2|3, 1|2>, k_gemm_small.hip gemm_small_kernel<CPR> and its split
reduction, k_gemm_rc.hip gemm_rc_kernel<0|11, 0>, k_gemm_big.hip gemm_bigp_kernel, k_gemm_qkv.hip gemm_qkvp_kernel, k_ffn.hip
ffn_fused_kernel) against the exact-answer designs and the float64 reference of tests/gemm_ref.py, launched through the
stand-alone ops the way the pipeline launches them.  The exact designs (dyadic, ties, place, int) demand the same bits;
`normal` the derived bound.  Every case asserts the kernel that ran (Engine.profile_kernel) and is called twice and must
return the same bits.  The ops themselves are hostile hosts (engine_ops.cpp): pad rows of A, W and V hold a large finite
pattern, every output buffer is sentinel-filled and checked for unwritten cells of [M, N] and for stores into columns
[N, ld) or rows at or beyond round_up(M, 256).  tests/test_gemm_ref_cpu.py shows that the same assertions reject fourteen
wrong GEMMs.

Measured on an MI355X (run with -s: one line per `normal` and LayerNorm case, the worst per kernel at the end): all 100
tests pass, every exact case bit-equal, no guard violation; the file takes 12 s of wall time (the largest single test, the
46 080-column bias-line case of gemm_bigp_kernel, 1.3 s).  Worst |err| / bound of the `normal` design, bounds derived in
tests/gemm_ref.py and not tuned:
    gemm_f16_pp3<2, 1|2> (fp32 result) 0.002    gemm_f16_pp3<1, 1|2> (f16) 0.746    gemm_f16_pp3<3, 1|2> (blocked f16) 0.626
    gemm_small_kernel<72> 0.001 (fp32) / 0.726 (f16), <32> with its split reduction 0.178    gemm_bigp_kernel 0.717
    gemm_qkvp_kernel 0.723
    gemm_rc_kernel<0, 0> 0.001    gemm_rc_kernel<11, 0> 0.002
(an f16 result sits at up to 0.75 because the f16 rounding term, half an f16 ulp, is most of its bound; the fp32 figures say
the matrix core's accumulation stays three orders of magnitude inside one fp32 ulp per term.)  LayerNorm behind an exact x
against ln_bound: fp32 copy 0.001 everywhere; f16 copy 0.644 (short-input reduction), 0.642 / 0.651 (gemm_rc_kernel<0 | 11, 0>),
0.645 (ffn_fused_kernel).

Finding, fixed in k_gemm.hip: a missing wait in the f16-result kinds of gemm_f16_pp3 (and its int8 twin) with one or two
k-steps per tile.  The bias line of tile t + 2 is requested by LDS-DMA at the end of tile t and read, by a plain LDS read, at
the end of tile t + 1.  The counted waits of the k-steps in between retire that request only from the third step on: group B
waits in front of the step's own pieces, so in the first step the request may still be in flight, and in the second step the
store term of the wait still counts stores older than the request.  At K = 64 and 128, from a workgroup's third tile on,
nothing but latency ordered the DMA's arrival against the read; had it lost, the accumulators would have started from the
previous tile's bias.  No case here produced a wrong bit before the fix (the hazard was found by reading the kernel for
these cases), and the pipeline never launches the shape (M <= 512 goes to the short-input kernel, every other K is >= 192),
but launch_gemm accepts it and a bit-exact suite must not rest on timing.  Fix: tile_end drains the vector-memory counter
before it reads the line when a tile has fewer than three k-steps — uniform per launch, never taken at the pipeline's depths.
bench.py step time, this tree against its parent, alternating in one session, three runs each of 40 steps: 8.526 / 8.551 /
8.530 ms against 8.551 / 8.509 / 8.593 ms, same ids digest.  test_pp3_several_tiles_per_workgroup and test_pp3_few_k_steps
are the cases that cover it.

Otherwise: 128^-0.5 meets f16(fl32(fl32(v) fl32(s))) in every kernel that scales, so kernels.h stands as written (the scale
the engine passes, fl32(1 / fl32(sqrt(128))) = gemm_ref.QSCALE, equals fl32(128^-0.5)).  gemm_rc_kernel<11, 0> documents
T >= 8 and its launcher refuses T = 5 (asserted below); the short-input kernel takes T = 5 and T = 7.  The short-input
launcher notes its instance and its form ("gemm_small_kernel<72>, 96-row bricks", "gemm_small_kernel<32>, split 8 +
small_reduce_kernel"), so the 96-row bricks and the split path are asserted by name; its workspace rule sends M = 512 at
K = 704 and K = 2304 to gemm_f16_pp3 (asserted by name)."""
import math

import numpy as np
import pytest

import gemm_ref as R
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

WORST = {}
PP3 = {(0, 128): "gemm_f16_pp3<2, 1>", (0, 256): "gemm_f16_pp3<2, 2>", (1, 128): "gemm_f16_pp3<1, 1>", (1, 256): "gemm_f16_pp3<1, 2>",
       (2, 128): "gemm_f16_pp3<3, 1>", (2, 256): "gemm_f16_pp3<3, 2>"}
SMALL, BIGP, QKVP = "gemm_small_kernel", "gemm_bigp_kernel", "gemm_qkvp_kernel"
SPLITS = {640: 5, 704: 11, 1024: 4, 1536: 6, 2048: 8, 2304: 9}          # K -> partial products of the short-input split path
RC0, RC11 = "gemm_rc_kernel<0, 0>", "gemm_rc_kernel<11, 0>"
FFN = "ffn_fused_kernel<8, 0, 2, 0, 0, 0>"


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    w = W.synth_weights(cfg, seed=5)
    e = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    e.profile(True)
    yield e
    e.close()
    print("worst |err| / bound per kernel:", {k: "%.3f" % v for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _note(kernel, ratio):
    if SMALL in kernel:
        kernel = kernel.split(",")[0]                          # the instance, without the form
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def _expected(kernel, K):
    """the name the launcher notes; the short-input kernel's names its instance and its form: one launch of 128-row bricks
    (96-row at K = 576) or the split partials with their reduction"""
    if kernel != SMALL:
        return kernel
    if K in SPLITS:
        return "gemm_small_kernel<%d>, split %d + small_reduce_kernel" % (K // SPLITS[K] // 8, SPLITS[K])
    return "gemm_small_kernel<%d>, %d-row bricks" % (K // 8, 96 if K == 576 else 128)


def _gemm(eng, c, tile_rows, kernel, a_blocked=False):
    """one case through pf_op_gemm_ex: the kernel's name, the design's assertion, the same bits from a second call"""
    what = "%s M %d N %d K %d kind %d tile %d relu %d bias %d resid %d add2 %d scale %d x %g blocked A %d" % (
        c.design, c.M, c.N, c.K, c.out_kind, tile_rows, c.relu, c.bias is not None, c.resid is not None, c.add2 is not None,
        c.scale_cols, c.scale, a_blocked)
    kw = dict(bias=c.bias, resid=c.resid, add2=c.add2, relu=c.relu, out_kind=c.out_kind, a_blocked=a_blocked, tile_rows=tile_rows,
              scale_cols=c.scale_cols, scale=c.scale)
    eng.profile_reset()
    got = eng.op_gemm_ex(c.A, c.W, **kw)
    ran = eng.profile_kernel("gemm_op")
    kernel = _expected(kernel, c.K)
    assert ran.startswith(kernel) if kernel.endswith("pp3") else ran == kernel, "%s: ran %r, expected %r" % (what, ran, kernel)
    ratio = R.check(c, got, what)
    if c.design == "normal":
        print("%s [%s]: |err| / bound = %.3f" % (what, ran, ratio))
        _note(ran, ratio)
    assert np.array_equal(eng.op_gemm_ex(c.A, c.W, **kw), got), what + ": a second call returned other bits"
    return got


# the epilogues of a kind, rotated over the six shapes: the 128-row run of a K starts at its index, the 256-row run two further,
# so that the two runs of every K together meet all eight (kind 0) or six of them
def _epilogues(kind):
    if kind == 0:
        return (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, resid=True), dict(bias=True, add2=True),
                dict(bias=True, resid=True, add2=True, relu=True), dict(bias=True, resid=True, scale_cols=64, scale=0.125),
                dict(resid=True, relu=True))
    return (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, scale_cols=64, scale=0.125),
            dict(bias=True, scale_cols=64, scale=R.QSCALE), dict(relu=True))


def _fit(epi, N):
    """scale_cols needs N > scale_cols"""
    if epi.get("scale_cols", 0) >= N:
        epi = {k: v for k, v in epi.items() if k not in ("scale_cols", "scale")}
    return epi


PP3_SHAPES = ((1, 64), (31, 128), (129, 192), (257, 320), (200, 515), (77, 100))
PP3_K = (64, 128, 192, 448, 512, 576)


# ---- gemm_f16_pp3: nk = 1, 2, 3, 7, 8, 9 k-steps against a ring of 3 stages and 8 deferred store passes
@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("K", PP3_K)
def test_pp3_few_k_steps(eng, K, tile_rows):
    ki = PP3_K.index(K)
    for kind in (0, 1, 2):
        epis = _epilogues(kind)
        for i, (M, N) in enumerate(PP3_SHAPES):
            if kind == 2:
                N = -(-N // 64) * 64
            epi = _fit(epis[(i + ki + 2 * (tile_rows == 256)) % len(epis)], N)
            _gemm(eng, R.make_case("dyadic", M, N, K, out_kind=kind, **epi), tile_rows, PP3[kind, tile_rows])
        # scale_cols = 512 with N beyond it (and 64 next to it)
        N = 576 if kind == 2 else 515
        for sc, s in ((512, 0.125), (64, 0.125)) + (((512, R.QSCALE),) if kind else ()):
            epi = dict(bias=True, scale_cols=sc, scale=s, **(dict(resid=True) if kind == 0 else {}))
            _gemm(eng, R.make_case("dyadic", 200, N, K, out_kind=kind, **epi), tile_rows, PP3[kind, tile_rows])


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("K", (64, 192))
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_pp3_several_tiles_per_workgroup(eng, cus, kind, K, tile_rows):
    """fewer k-steps than ring stages / deferred passes while every workgroup walks more than two tiles: the deferred stores of
    one tile and the bias line fetched two tiles ahead meet the next tiles' k-steps.  M = 300: a ragged last tile row."""
    M = 300
    N = 128 * math.ceil(2.1 * cus / -(-M // tile_rows))
    assert -(-M // tile_rows) * (N // 128) > 2 * cus
    epi = (dict(bias=True, resid=True, relu=True), dict(bias=True, relu=True), dict(bias=True, scale_cols=512, scale=R.QSCALE))[kind]
    _gemm(eng, R.make_case("dyadic", M, N, K, out_kind=kind, **epi), tile_rows, PP3[kind, tile_rows])


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_pp3_deep_k(eng, kind, tile_rows):
    epi = (dict(bias=True, resid=True, add2=True), dict(bias=True, scale_cols=64, scale=R.QSCALE), dict(bias=True, relu=True))[kind]
    _gemm(eng, R.make_case("dyadic", 300, 512, 2048, out_kind=kind, **epi), tile_rows, PP3[kind, tile_rows])


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("K", (64, 192, 2048))
def test_pp3_blocked_a_operand(eng, K, tile_rows):
    for M in (33, 300):
        _gemm(eng, R.make_case("dyadic", M, 192, K, bias=True, resid=True), tile_rows, PP3[0, tile_rows], a_blocked=True)
        _gemm(eng, R.make_case("place", M, 192, K, out_kind=1), tile_rows, PP3[1, tile_rows], a_blocked=True)


# ---- gemm_small_kernel<CPR>, CPR = K / 8 for K = 64 .. 576: every instance
SMALL_M = (1, 32, 33, 127, 128, 129, 512)
SMALL_N = (32, 515, 544)


@pytest.mark.parametrize("j", range(1, 10))
def test_small_every_instance(eng, j):
    K = 64 * j
    for i, M in enumerate(SMALL_M):
        N = SMALL_N[(i + j) % 3]
        kind = (i + j) % 2
        epis = _epilogues(kind)
        epi = _fit(epis[(i + 2 * j) % len(epis)], N)
        _gemm(eng, R.make_case("dyadic", M, N, K, out_kind=kind, **epi), 32, SMALL)
    if K == 576:                                               # 96-row bricks
        for M in (96, 97, 200):
            for N in SMALL_N:
                _gemm(eng, R.make_case("dyadic", M, N, K, bias=True, resid=True, relu=True), 32, SMALL)
                epi = dict(bias=True, scale_cols=64, scale=0.125) if N > 64 else dict(bias=True)
                _gemm(eng, R.make_case("dyadic", M, N, K, out_kind=1, **epi), 32, SMALL)


# split path (N = 512): K -> splits 5, 11, 4, 6, 8, 9; the workspace holds S * round_up(M, 128) <= 4096 rows
SPLIT_EXPECT = {(640, 512): SMALL, (704, 512): "gemm_f16_pp3", (704, 129): SMALL, (1024, 512): SMALL, (1536, 512): SMALL,
                (2048, 512): SMALL, (2304, 512): "gemm_f16_pp3", (2304, 384): SMALL, (2304, 1): SMALL, (640, 1): SMALL, (2048, 129): SMALL}


@pytest.mark.parametrize("K,M", sorted(SPLIT_EXPECT))
def test_small_split_path_and_its_fallback(eng, K, M):
    """tile_rows = 0: the dispatch itself decides; where the partials would not fit the workspace (M = 512 at K = 704 and
    2304) it must fall back to gemm_f16_pp3, not overflow"""
    for kind, epi in ((0, dict(bias=True, resid=True, relu=True)), (0, dict(add2=True)), (1, dict(bias=True, relu=True))):
        _gemm(eng, R.make_case("dyadic", M, 512, K, out_kind=kind, **epi), 0, SPLIT_EXPECT[K, M])


@pytest.mark.parametrize("M,kernel", ((512, SMALL), (513, "gemm_f16_pp3")))
def test_short_input_threshold(eng, M, kernel):
    _gemm(eng, R.make_case("dyadic", M, 512, 512, bias=True, resid=True), 0, kernel)
    _gemm(eng, R.make_case("dyadic", M, 515, 64, bias=True, out_kind=1), 0, kernel)


def _ln_params(seed):
    r = np.random.default_rng(seed)
    return (1 + 0.1 * r.standard_normal(512)).astype(np.float32), (0.1 * r.standard_normal(512)).astype(np.float32)


def _rc(eng, c, kernel, short_input=False, a_blocked=False, ln=True):
    """one case through pf_op_gemm_rc: x exact (or bounded for `normal`), n32 / n16 against the float64 LayerNorm of the
    reference x under ln_bound"""
    what = "%s rc M %d K %d T %d short %d blocked A %d bias %d resid %d fsmn %d" % (
        c.design, c.M, c.K, c.T, short_input, a_blocked, c.bias is not None, c.resid is not None, c.V is not None)
    g, b = _ln_params(c.M + c.K)
    kw = dict(bias=c.bias, resid=c.resid, fsmn_v=c.V, fsmn_w=c.taps, T=c.T, ln=(g, b) if ln else None, a_blocked=a_blocked,
              short_input=short_input)
    eng.profile_reset()
    x, n16, n32 = eng.op_gemm_rc(c.A, c.W, **kw)
    ran = eng.profile_kernel("gemm_op")
    assert ran == _expected(kernel, c.K), "%s: ran %r, expected %r" % (what, ran, _expected(kernel, c.K))
    ratio = R.check(c, x, what)
    if c.design == "normal":
        print("%s [%s]: |err| / bound = %.3f" % (what, ran, ratio))
        _note(ran, ratio)
    elif ln:
        ref = R.reference(c)
        r32 = R.assert_bounded(R.ln_ref(ref, g, b), R.ln_bound(ref, g, b), n32, what + " n32")
        r16 = R.assert_bounded(R.ln_ref(ref, g, b), R.ln_bound(ref, g, b, half=True), n16, what + " n16")
        print("%s [%s]: LayerNorm |err| / bound = %.3f (fp32), %.3f (f16)" % (what, ran, r32, r16))
        _note("LayerNorm behind " + ran, max(r32, r16))
        assert np.array_equal(n16, n32.astype(np.float16).astype(np.float32)), what + ": n16 is not the f16 rounding of n32"
    x2, n16b, n32b = eng.op_gemm_rc(c.A, c.W, **kw)
    assert np.array_equal(x2, x) and (not ln or (np.array_equal(n16b, n16) and np.array_equal(n32b, n32))), what + ": a second call returned other bits"
    if ln:                                                     # the LayerNorm-only form (x not kept) computes the same
        _, m16, m32 = eng.op_gemm_rc(c.A, c.W, want_x=False, **kw)
        assert np.array_equal(m16, n16) and np.array_equal(m32, n32), what + ": without out_x the LayerNorm differs"


@pytest.mark.parametrize("K", (640, 1024, 2048))
def test_small_split_reduction_with_layernorm(eng, K):
    for M in (1, 129, 512):
        _rc(eng, R.make_case("dyadic", M, 512, K, bias=True, resid=True), SMALL, short_input=True)
        _rc(eng, R.make_case("dyadic", M, 512, K, bias=True), SMALL, short_input=True, ln=False)


@pytest.mark.parametrize("B,T", ((3, 83), (4, 64), (9, 7)))
def test_small_fsmn_epilogue(eng, B, T):
    for K in (64, 512, 576):
        _rc(eng, R.make_case("dyadic", B * T, 512, K, bias=True, resid=True, fsmn=(B, T)), SMALL, short_input=True)
    _rc(eng, R.make_case("dyadic", B * T, 512, 512, bias=True, fsmn=(B, T)), SMALL, short_input=True, ln=False)


# ---- gemm_rc_kernel
@pytest.mark.parametrize("a_blocked", (False, True))
@pytest.mark.parametrize("K", (64, 128, 512, 2048))
def test_rc(eng, K, a_blocked):
    for i, M in enumerate((1, 63, 64, 65, 200)):
        epi = (dict(bias=True, resid=True), dict(bias=True), dict(resid=True), dict())[(i + K // 64) % 4]
        _rc(eng, R.make_case("dyadic", M, 512, K, **epi), RC0, a_blocked=a_blocked)
    _rc(eng, R.make_case("place", 65, 512, K, bias=True, resid=True), RC0, a_blocked=a_blocked, ln=False)


@pytest.mark.parametrize("B,T", ((3, 83), (5, 64), (25, 8), (2, 11)))
def test_rc_fsmn(eng, B, T):
    """utterance edges inside and on the 64-row tiles; T = 8 is the shortest utterance the fused FSMN takes"""
    for K, a_blocked in ((512, False), (64, True), (2048, False)):
        _rc(eng, R.make_case("dyadic", B * T, 512, K, bias=True, resid=True, fsmn=(B, T)), RC11, a_blocked=a_blocked)
    _rc(eng, R.make_case("dyadic", B * T, 512, 512, fsmn=(B, T)), RC11, ln=False)


def test_rc_fsmn_refuses_utterances_shorter_than_its_window(eng):
    from aliparaformerasr_amd import _native as N
    c = R.make_case("dyadic", 200, 512, 512, bias=True, fsmn=(40, 5))
    with pytest.raises(N.PfError, match="T >= 8"):
        eng.op_gemm_rc(c.A, c.W, bias=c.bias, fsmn_v=c.V, fsmn_w=c.taps, T=5)
    # the short-input kernel takes them
    _rc(eng, c, SMALL, short_input=True, ln=False)


# ---- gemm_bigp_kernel
@pytest.mark.parametrize("K", (128, 192, 512))
def test_bigp(eng, K):
    epis = (dict(bias=True, relu=True), dict(bias=True, scale_cols=64, scale=0.125), dict(bias=True, relu=True, scale_cols=256, scale=R.QSCALE),
            dict(relu=True), dict(bias=True, scale_cols=256, scale=0.125), dict(bias=True, scale_cols=64, scale=R.QSCALE), dict(), dict(bias=True))
    i = K // 64
    for M in (1, 255, 256, 257):
        for N in (256, 512):
            _gemm(eng, R.make_case("dyadic", M, N, K, out_kind=2, **_fit(epis[i % len(epis)], N)), 1024, BIGP)
            i += 1


def test_bigp_bias_line_reuse(eng, cus):
    """K = 128 (two k-steps of 64, the kernel's minimum) with at least three tiles per workgroup: the bias line fetched with a
    tile's first stage is reused two tiles later"""
    M, N = 700, 256 * math.ceil(2.1 * cus / 3)
    assert N <= 65536 and 3 * (N // 256) >= 2.1 * cus
    _gemm(eng, R.make_case("dyadic", M, N, 128, bias=True, relu=True, scale_cols=256, scale=R.QSCALE, out_kind=2), 1024, BIGP)


# ---- gemm_qkvp_kernel (q, k, v only: ctx belongs to the attention suite)
def _qkv(eng, design, B, T, K, bias, first_col=0):
    """first_col = 512: k | v only, against a case without the scale (`ties`: q is scaled by 128^-0.5, no tie survives it)"""
    M = B * T
    c = R.make_case(design, M, 1536, K, bias=bias, out_kind=1, **(dict() if first_col else dict(scale_cols=512, scale=R.QSCALE)))
    what = "%s qkv B %d T %d K %d bias %d" % (design, B, T, K, bias)
    eng.profile_reset()
    q, k, v, _ = eng.op_qkv_attention(c.A, c.W, c.bias, B, T)
    ran = eng.profile_kernel("gemm_op")
    assert ran == QKVP, (what, ran)
    got = np.concatenate([q, k, v], axis=1)[:, first_col:]
    if first_col:
        R.assert_exact(c, R.reference(c)[:, first_col:], got, what)
    ratio = 0.0 if first_col else R.check(c, got, what)
    if design == "normal":
        print("%s [%s]: |err| / bound = %.3f" % (what, ran, ratio))
        _note(ran, ratio)
    q2, k2, v2, _ = eng.op_qkv_attention(c.A, c.W, c.bias, B, T)
    assert np.array_equal(np.concatenate([q2, k2, v2], axis=1)[:, first_col:], got), what + ": a second call returned other bits"


@pytest.mark.parametrize("K", (128, 192, 512, 576))
def test_qkvp(eng, K):
    for i, (B, T) in enumerate(((1, 1), (1, 255), (3, 83), (2, 257))):
        _qkv(eng, "dyadic", B, T, K, bias=bool((i + K // 64) % 2))
    _qkv(eng, "dyadic", 3, 83, K, bias=not bool((2 + K // 64) % 2))


def test_qkvp_several_tiles_per_workgroup(eng, cus):
    B, T = -(-cus // 4) + 1, 257
    assert -(-B * T // 256) * 8 > 2 * cus
    _qkv(eng, "dyadic", B, T, 128, bias=True)


# ---- the encoder FFN block, `int` design
@pytest.mark.parametrize("resid", (False, True))
@pytest.mark.parametrize("M", (1, 63, 64, 65, 300))
def test_ffn_block(eng, M, resid):
    c = R.make_ffn_case(M, resid)
    ref = R.ffn_reference(c)
    what = "int M %d resid %d" % (M, resid)
    # two launches, blocked hand-off of the hidden
    rs = c.resid if resid else np.zeros((M, 512), np.float32)
    eng.profile_reset()
    y = eng.op_ffn(c.x, c.w1, c.b1, c.w2, c.b2, rs)
    up, down = eng.profile_kernel("gemm_ffn1"), eng.profile_kernel("gemm_ffn2")
    assert up.startswith("gemm_f16_pp3<3,") and down.startswith("gemm_f16_pp3<2,"), (what, up, down)
    R.assert_exact(c, ref, y, what + " op_ffn")
    assert np.array_equal(eng.op_ffn(c.x, c.w1, c.b1, c.w2, c.b2, rs), y)
    # one launch
    g, b = _ln_params(M)
    eng.profile_reset()
    x, n16 = eng.op_ffn_fused(c.x, c.w1, c.b1, c.w2, c.b2, resid=c.resid, ln=(g, b))
    assert eng.profile_kernel("gemm_op") == FFN, (what, eng.profile_kernel("gemm_op"))
    R.assert_exact(c, ref, x, what + " op_ffn_fused")
    ratio = R.assert_bounded(R.ln_ref(ref, g, b), R.ln_bound(ref, g, b, half=True), n16, what + " fused LayerNorm")
    print("%s [%s]: LayerNorm |err| / bound = %.3f" % (what, FFN, ratio))
    _note("LayerNorm behind " + FFN, ratio)
    x2, n2 = eng.op_ffn_fused(c.x, c.w1, c.b1, c.w2, c.b2, resid=c.resid, ln=(g, b))
    assert np.array_equal(x2, x) and np.array_equal(n2, n16), what + ": a second call returned other bits"
    x3, _ = eng.op_ffn_fused(c.x, c.w1, c.b1, c.w2, c.b2, resid=c.resid)
    assert np.array_equal(x3, x), what + ": without the LayerNorm x differs"


# ---- ties and place once per kernel, at its smallest multi-tile shape
@pytest.mark.parametrize("design", ("ties", "place"))
def test_ties_and_place_per_kernel(eng, design):
    for tile_rows in (128, 256):
        for kind in (0, 1, 2):
            _gemm(eng, R.make_case(design, tile_rows + 1, 192, 128, out_kind=kind), tile_rows, PP3[kind, tile_rows])
    for kind in (0, 1):
        _gemm(eng, R.make_case(design, 129, 96, 128, out_kind=kind), 32, SMALL)
        _gemm(eng, R.make_case(design, 129, 512, 1024, out_kind=kind), 32, SMALL)
    _gemm(eng, R.make_case(design, 257, 512, 128, out_kind=2), 1024, BIGP)
    _rc(eng, R.make_case(design, 65, 512, 128), RC0, ln=False)
    _rc(eng, R.make_case(design, 65, 512, 128), RC0, a_blocked=True, ln=False)
    _qkv(eng, design, 1, 257, 128, bias=False, first_col=512 if design == "ties" else 0)


# ---- the real-valued design under the derived bound
@pytest.mark.parametrize("M,N,K", ((300, 515, 576), (300, 512, 2048)))
def test_normal_design_per_kernel(eng, M, N, K):
    for tile_rows in (128, 256):
        _gemm(eng, R.make_case("normal", M, N, K, bias=True, resid=True, add2=True), tile_rows, PP3[0, tile_rows])
        _gemm(eng, R.make_case("normal", M, N, K, bias=True, relu=True, out_kind=1), tile_rows, PP3[1, tile_rows])
        _gemm(eng, R.make_case("normal", M, 512, K, bias=True, relu=True, scale_cols=64, scale=R.QSCALE, out_kind=2), tile_rows, PP3[2, tile_rows])
    _gemm(eng, R.make_case("normal", M, N, K, bias=True, resid=True), 32, SMALL)
    _gemm(eng, R.make_case("normal", M, N, K, bias=True, out_kind=1), 32, SMALL)
    _gemm(eng, R.make_case("normal", M, 512, K, bias=True, relu=True, out_kind=2), 1024, BIGP)
    _rc(eng, R.make_case("normal", M, 512, K, bias=True, resid=True), RC0)
    _rc(eng, R.make_case("normal", 4 * 75, 512, K, bias=True, resid=True, fsmn=(4, 75)), RC11)
    _qkv(eng, "normal", 1, M, K, bias=True)
