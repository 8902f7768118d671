"""GPU: the int8 path's kernels one at a time (csrc/k_quant.hip minmax_kernel, quantize_rows_kernel, ln_minmax_kernel<2|3|8>,
ln_quantize_kernel<2|3|8>, quantize_weight_kernel, import_weight_kernel, pack_dz_kernel; csrc/k_gemm.hip gemm_i8_pp3<1|2>,
gemm_i8f_pp3<1|2>) against the exact-answer designs of tests/int8_ref.py, which builds on oracle/int8.py.  Every design demands
the same bits (ln_normal: the derived bound); every GEMM case asserts the kernel that ran (Engine.profile_kernel); every case
is called twice and must return the same bits.  The ops are hostile hosts (engine_int8.cpp): pad rows, pad columns and the
cells behind a tensor hold a large finite pattern, float vectors behind N NaN, rowsum behind M large magnitudes, the operand
pad rows the codes +127 / -128; every output is sentinel-filled and checked for unwritten result cells and for stores outside
what kernels.h allows.  tests/test_int8_ref_cpu.py shows that the same assertions reject seventeen wrong implementations.

Measured on an MI355X: all 94 tests pass, every exact case bit-equal, no guard violation, every second call the same bits; the
file takes 21 to 29 s of wall time (two runs), 3 s of it the engine's set-up (the largest single test, a several-tiles case
with N = 34 432, 1.3 s; most of every test is the host side of the ops and the float64 reference).  ln_normal, share of the cells that lie
within ln_bound of a code boundary and may therefore differ by one code, computed from the reference alone (the condition is
under 0.20): 0.0016 (5 x 128), 0.0395 (37 x 512), 0.0311 (37 x 560), 0.1032 (19 x 2048), 0.0310 (257 x 512); the kernels'
codes met the reference's on all the other cells and never differed by more than one on these.

Findings.
  * No kernel returned a wrong bit and none read or stored outside its contract.  In particular the int8 twin of the f16
    kernels' bias-line wait (tile_end's drain with fewer than three k-steps, fixed by reading the code when the f16 suite found
    it) holds with one, two and three k-steps per tile and more than two tiles per workgroup, for every result kind and both
    tile heights (test_gemm_several_tiles_per_workgroup), and the range a launch reports ignores what the pad rows of the
    operands and of rowsum hold (test_gemm_range).
  * range_out beside an fp32 result: no caller passes both (Engine::qgemm sets kRangeOut on the encoder's FFN-up alone, an f16
    result), and the pair is rounded to f16, which is not what a consumer of the fp32 result reads.  launch_gemm_i8 now refuses
    the combination (PF_ERR_UNSUPPORTED); test_gemm_range asserts the refusal.
  * The design as first written — constant rows of codes 0 / 255 — never makes the int32 -> float cast round, although the
    sums pass 2^24 above K = 257: a sum is K times 255 x 255, 255 x 127 or 255 x 128, and at the K used here (560 = 35 x 16,
    1024, 2048, 16384) its odd part fits 24 bits, so it is a float32 value.  int8_ref's `extreme` therefore flips the first
    one / three codes of two rows in four (make_gemm_case asserts that a sum of the case is no float32 value).
  * pack_dz's limit K <= 16384 is conservative: the packed word holds |colsum - K wzp| <= 255 K in 24 bits up to K = 32 895.
    The launcher's refusal is kept as it is and asserted (test_pack_dz_at_the_extreme_column_sums).
  * Dead code removed from k_quant.hip (fkey / fkey_inv); kernels.h now states what GemmI8Args' kernels read and write per
    result kind, and the ops enforce exactly that; launch_quantize_rows' comment names quant_scratch_bytes().
No change touches gemm_pp3_impl or a quantiser's device code, so no step-time comparison against the parent was needed."""
import math

import numpy as np
import pytest

import int8_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

F32 = np.float32
KERNEL = {(0, 128): "gemm_i8_pp3<1>", (0, 256): "gemm_i8_pp3<2>", (1, 128): "gemm_i8f_pp3<1>", (1, 256): "gemm_i8f_pp3<2>",
          (2, 128): "gemm_i8_pp3<1>", (2, 256): "gemm_i8_pp3<2>", (3, 128): "gemm_i8_pp3<1>", (3, 256): "gemm_i8_pp3<2>"}
ROWS = (1, 3, 4, 5, 257)
COLS = (4, 252, 256, 260, 560, 2048)
LEFT_OUT = {}


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    w = W.synth_weights(cfg, seed=5)
    e = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    e.profile(True)
    yield e
    e.close()
    print("ln_normal, share of cells within the bound of a code boundary:", {k: "%.4f" % v for k, v in sorted(LEFT_OUT.items())})


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up(x, m):
    return -(-x // m) * m


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ the activation quantiser
def _quant(eng, c, f16, ldx, ld):
    what = "%s rows %d cols %d f16 %d ldx %d ld %d" % (c.design, c.rows, c.cols, f16, ldx, ld)
    aq, rs, par = eng.op_quantize(c.x, x_is_f16=f16, ldx=ldx, ld=ld)
    R.check_quant(c, aq, rs, par, what)
    again = eng.op_quantize(c.x, x_is_f16=f16, ldx=ldx, ld=ld)
    assert np.array_equal(again[0], aq) and np.array_equal(again[1], rs) and again[2] == par, what + ": a second call returned other bits"


def _strides(i, k, cols):
    """ldx >= cols and ld >= cols, rotated: dense, a few quads wider, the GEMM's operand stride"""
    return cols + 4 * ((i + k) % 3), (cols, cols + 8, _up(cols, 128))[(i + 2 * k) % 3]


@pytest.mark.parametrize("f16", (False, True))
@pytest.mark.parametrize("design", [d for d in R.Q_DESIGNS if d != "place"])
def test_quantiser_designs(eng, design, f16):
    for i, rows in enumerate(ROWS):
        for k, cols in enumerate(COLS):
            ldx, ld = _strides(i, k, cols)
            c = R.make_quant_case(design, rows, cols, j=(3, 7, 10)[(i + k) % 3], z=(100, 101)[(i + k // 3) % 2], f16=f16)
            _quant(eng, c, f16, ldx, ld)


@pytest.mark.parametrize("f16", (False, True))
def test_quantiser_extrema_at_every_place(eng, f16):
    """the minimum and the maximum each in turn at the first and the last element, in the last quad of a row and in a row that
    is not a multiple of 4 from the end"""
    for i, rows in enumerate(ROWS):
        for k, cols in enumerate(COLS):
            names = list(R.places(rows, cols))
            for t, name in enumerate(names):
                other = names[(t + 1) % len(names)]
                if R.places(rows, cols)[name] == R.places(rows, cols)[other]:
                    continue
                ldx, ld = _strides(i + t, k, cols)
                _quant(eng, R.make_quant_case("place", rows, cols, f16=f16, where=(name, other)), f16, ldx, ld)


@pytest.mark.parametrize("f16", (False, True))
def test_minmax_unrolled_loop_and_its_remainder(eng, f16):
    """rows * cols / 4 just above 3 * 256 * 1024: the four-way unrolled loop of minmax_kernel runs one trip for the first threads,
    the remainder loop three for the others; the extrema visit each of the four unrolled loads and both ends of the remainder"""
    rows, cols = R.UNROLL_SHAPE
    names = [n for n in R.places(rows, cols) if n.startswith(("unrolled", "remainder"))]
    for t, name in enumerate(names):
        c = R.make_quant_case("place", rows, cols, f16=f16, where=(name, names[(t + 1) % len(names)]))
        what = "place %s f16 %d" % (name, f16)
        aq, rs, par = eng.op_quantize(c.x, x_is_f16=f16, ldx=cols + 4 * (t % 2), ld=cols)
        R.check_quant(c, aq, rs, par, what)
    again = eng.op_quantize(c.x, x_is_f16=f16, ldx=cols + 4 * (t % 2), ld=cols)
    assert np.array_equal(again[0], aq) and np.array_equal(again[1], rs) and again[2] == par, what + ": a second call returned other bits"


# ------------------------------------------------------------------------------------------------ LayerNorm in front
def _ln(eng, c, ld):
    what = "%s rows %d D %d ld %d" % (c.design, c.rows, c.D, ld)
    got = eng.op_quantize(c.x, ld=ld, ln=(c.gamma, c.beta))
    if c.design == "ln_exact":
        R.check_quant(c, *got, what=what)
    else:
        LEFT_OUT[(c.rows, c.D)] = R.check_ln_normal(c, *got, what=what)
    again = eng.op_quantize(c.x, ld=ld, ln=(c.gamma, c.beta))
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2] == got[2], what + ": a second call returned other bits"


@pytest.mark.parametrize("D,ld", ((4, 4), (4, 128), (128, 128), (512, 512), (560, 640), (2048, 2048)))
def test_ln_exact(eng, D, ld):
    """ln_minmax_kernel / ln_quantize_kernel <2> (ld <= 512), <3> (560 with ld 640) and <8> (2048)"""
    for i, rows in enumerate((1, 3, 4, 5)):
        _ln(eng, R.make_ln_case("ln_exact", rows, D, j=(3, 7, 10)[i % 3], z=(100, 101)[i % 2]), ld)


def test_ln_exact_second_trip_of_the_row_loop(eng):
    """256 workgroups of 16 waves take 4096 rows per trip of ln_minmax_kernel's row loop: row 4096 is a second trip"""
    _ln(eng, R.make_ln_case("ln_exact", 4097, 128, z=101), 128)
    _ln(eng, R.make_ln_case("ln_exact", 4097, 560, z=100), 640)


@pytest.mark.parametrize("rows,D,seed", R.LN_NORMAL_CASES)
def test_ln_normal(eng, rows, D, seed):
    c = R.make_ln_case("ln_normal", rows, D, seed=seed)
    assert R.ln_left_out(c) < R.LN_LEFT_OUT_MAX
    _ln(eng, c, _up(D, 128))
    print("ln_normal rows %d D %d: %.4f of the cells within the bound of a code boundary" % (rows, D, LEFT_OUT[(rows, D)]))


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("K", (4, 60, 64, 68, 560))
def test_weight_quantiser_and_import(eng, K):
    for i, Nn in enumerate((1, 3, 4, 5, 130)):
        Wm, codes, scale, zp = R.make_weight_case(Nn, K)
        ld = (K, _up(K, 128))[i % 2] if K % 4 == 0 else _up(K, 128)
        what = "N %d K %d ld %d" % (Nn, K, ld)
        got = eng.op_quantize_weight(Wm, ld=ld)
        R.check_weight(codes, scale, zp, K, got, "quantize_weight " + what)
        assert _same(eng.op_quantize_weight(Wm, ld=ld), got), what + ": a second call returned other bits"
        # the stored form of an export: any bytes, any zero point, any scale
        r = np.random.default_rng(Nn * 1000 + K)
        q, z, s = r.integers(0, 256, (Nn, K)), r.integers(0, 256, Nn), r.uniform(1e-4, 1e-1, Nn).astype(F32)
        q[0], z[0] = 255 * (K % 8 == 4), 255 * (i % 2)
        got = eng.op_import_weight(q, z, s, ld=ld)
        R.check_weight(q, s, z, K, got, "import_weight " + what)
        assert _same(eng.op_import_weight(q, z, s, ld=ld), got), what + ": a second call returned other bits"


def test_pack_dz_at_the_extreme_column_sums(eng):
    K = 16384
    q = np.repeat(np.asarray((0, 0, 255, 255), np.uint8)[:, None], K, axis=1)
    z = np.asarray((0, 255, 0, 255), np.uint8)
    got = eng.op_import_weight(q, z, np.ones(4, F32), ld=K)
    R.check_weight(q, np.ones(4, F32), z, K, got, "pack_dz K 16384")
    assert sorted(np.asarray(got[4], np.int64) >> 8) == [-255 * K, 0, 0, 255 * K]
    with pytest.raises(N.PfError, match="pack_dz"):
        eng.op_import_weight(np.zeros((4, K + 4), np.uint8), z, np.ones(4, F32), ld=K + 4)


# ------------------------------------------------------------------------------------------------ the integer GEMM
def _qgemm(eng, c, tile_rows, want_range=None):
    """one case through pf_op_qgemm_ex: the kernel's name, the design's assertion, the same bits from a second call.  An f16-only
    result reports its range unless told otherwise."""
    want_range = c.out_kind in (1, 2) if want_range is None else want_range
    what = "%s M %d N %d K %d kind %d tile %d relu %d bias %d resid %d add2 %d scale %d x %g a_zp %d" % (
        c.design, c.M, c.N, c.K, c.out_kind, tile_rows, c.relu, c.bias is not None, c.resid is not None, c.add2 is not None,
        c.scale_cols, c.scale, c.a_zp)
    kw = dict(bias=c.bias, resid=c.resid, add2=c.add2, relu=c.relu, scale_cols=c.scale_cols, scale=c.scale, out_kind=c.out_kind,
              tile_rows=tile_rows, want_range=want_range, K_true=c.K)
    args = (c.a_codes, c.a_scale, c.a_zp, c.w_codes, c.w_zp, c.w_scale)
    eng.profile_reset()
    got = eng.op_qgemm_ex(*args, **kw)
    ran = eng.profile_kernel("gemm_op")
    assert ran == KERNEL[c.out_kind, tile_rows], "%s: ran %r, expected %r" % (what, ran, KERNEL[c.out_kind, tile_rows])
    ref = R.gemm_reference(c)
    R.check_gemm(c, got, what, ref=(ref[0] if c.out_kind in (0, 3) else None, ref[1] if c.out_kind else None, ref[2]))
    assert _same(eng.op_qgemm_ex(*args, **kw), got), what + ": a second call returned other bits"
    return got


# the epilogues of a result kind, rotated as the f16 suite rotates them; kind 1 (gemm_i8f_pp3) takes no residual or addend; a
# scale that is no power of two only where the pipeline uses it (f16 results without residual or addend)
def _epilogues(kind):
    full = (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, resid=True), dict(bias=True, add2=True),
            dict(bias=True, resid=True, add2=True, relu=True), dict(bias=True, resid=True, scale_cols=64, scale=0.125),
            dict(resid=True, relu=True))
    if kind in (0, 3):
        return full
    f16 = (dict(), dict(bias=True), dict(bias=True, relu=True), dict(bias=True, scale_cols=64, scale=0.125),
           dict(bias=True, scale_cols=64, scale=R.QSCALE), dict(relu=True))
    return f16 if kind == 1 else f16 + full[3:]


def _fit(epi, Nn, design, K):
    if epi.get("scale_cols", 0) >= Nn:
        epi = {k: v for k, v in epi.items() if k not in ("scale_cols", "scale")}
    return {} if design == "ties" else epi


GEMM_M = (1, 127, 128, 129, 255, 257, 300)
GEMM_N = (64, 100, 128, 148, 515)
GEMM_K = (4, 128, 132, 256, 384, 560, 1024, 2048)


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("K", GEMM_K)
def test_gemm_per_kernel(eng, K, tile_rows):
    """every result kind at every M, the N rotated against them (the eight K together pair every M with every N), designs,
    epilogues and the activation zero point of `extreme` rotated along"""
    ki = GEMM_K.index(K)
    for kind in (0, 1, 2, 3):
        epis = _epilogues(kind)
        for i, M in enumerate(GEMM_M):
            Nn = GEMM_N[(i + ki) % len(GEMM_N)]
            design = R.G_DESIGNS[(i + ki + kind) % 4]
            if design == "ties" and K < 16:
                design = "place"
            epi = _fit(epis[(i + ki + 2 * (tile_rows == 256)) % len(epis)], Nn, design, K)
            _qgemm(eng, R.make_gemm_case(design, M, Nn, K, out_kind=kind, variant=(i + ki) % 3, **epi), tile_rows)


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("design", R.G_DESIGNS)
def test_gemm_every_design_per_kernel(eng, design, tile_rows):
    """each design once per kernel and result kind at its smallest multi-tile shape, ragged in M, N and K"""
    for kind in (0, 1, 2, 3):
        for variant in ((0, 1, 2) if design == "extreme" else (0,)):
            _qgemm(eng, R.make_gemm_case(design, tile_rows + 1, 148, 560, out_kind=kind, variant=variant), tile_rows)
    _qgemm(eng, R.make_gemm_case(design, 300, 515, 132, out_kind=1, **({} if design == "ties" else dict(bias=True, relu=True))), tile_rows)


@pytest.mark.parametrize("tile_rows", (128, 256))
def test_gemm_deepest_k(eng, tile_rows):
    """K = 16384, the deepest the packed column word takes: sums of 2^30, the largest correction terms"""
    for kind in (0, 1, 2, 3):
        _qgemm(eng, R.make_gemm_case("extreme", 4, 64, 16384, out_kind=kind, variant=(0, 2, 1, 2)[kind], bias=kind != 2), tile_rows)


@pytest.mark.parametrize("tile_rows", (128, 256))
@pytest.mark.parametrize("K", (128, 256, 384))
@pytest.mark.parametrize("kind", (0, 1, 2, 3))
def test_gemm_several_tiles_per_workgroup(eng, cus, kind, K, tile_rows):
    """one, two and three k-steps per tile (Kpad = 128, 256, 384) while every workgroup walks more than two tiles: the deferred
    stores of one tile and the column lines fetched a tile ahead meet the next tiles' k-steps.  The int8 twins of the f16
    suite's test_pp3_several_tiles_per_workgroup and test_pp3_few_k_steps.  M = 300: a ragged last tile row."""
    M = 300
    Nn = 128 * math.ceil(2.1 * cus / -(-M // tile_rows))
    assert -(-M // tile_rows) * (Nn // 128) > 2 * cus
    epi = (dict(bias=True, resid=True, relu=True), dict(bias=True, relu=True), dict(bias=True, scale_cols=512, scale=R.QSCALE),
           dict(bias=True, add2=True))[kind]
    _qgemm(eng, R.make_gemm_case("place", M, Nn, K - 28 * (kind % 2), out_kind=kind, **epi), tile_rows)


@pytest.mark.parametrize("tile_rows", (128, 256))
def test_gemm_range(eng, tile_rows):
    """the reported pair is the minimum and the maximum (with 0) of the f16 results over rows < M and columns < N, whatever the
    pad rows of the operands and of rowsum hold; with an fp32 result the launcher refuses to report one: no caller passes both
    (kRangeOut is set on the encoder's FFN-up alone), and the pair is rounded to f16, which is not what an fp32 consumer reads"""
    for M, Nn, K in ((1, 64, 128), (129, 100, 132), (257, 148, 560), (300, 515, 384)):
        for kind in (1, 2):
            for epi in (dict(), dict(bias=True, relu=True)):
                got = _qgemm(eng, R.make_gemm_case("random", M, Nn, K, out_kind=kind, **epi), tile_rows, want_range=True)
                y16 = got[1]
                assert got[2] == (min(float(y16.min()), 0.0), max(float(y16.max()), 0.0))
            got = _qgemm(eng, R.make_gemm_case("random", M, Nn, K, out_kind=kind, relu=True), tile_rows, want_range=False)
            assert got[2] is None
    c = R.make_gemm_case("random", 129, 100, 132, bias=True)
    for kind in (0, 3):
        with pytest.raises(N.PfError, match="range output is the range of an f16 result"):
            eng.op_qgemm_ex(c.a_codes, c.a_scale, c.a_zp, c.w_codes, c.w_zp, c.w_scale, bias=c.bias, out_kind=kind, tile_rows=tile_rows,
                            want_range=True)


def test_gemm_dispatch_by_shape_is_unchanged(eng, cus):
    """tile_rows = 0: the launcher's own rule — few 256-row tiles (under 0.9 of the CUs) or a shorter last round choose 128 rows"""
    for M, Nn in ((300, 128), (2 * 256, 128 * cus)):
        t2, t1 = -(-M // 256) * (Nn // 128), -(-M // 128) * (Nn // 128)
        mi = 1 if (t2 < 0.9 * cus or 0.58 * -(-t1 // cus) < -(-t2 // cus)) else 2
        c = R.make_gemm_case("place", M, Nn, 128, out_kind=1)
        eng.profile_reset()
        got = eng.op_qgemm_ex(c.a_codes, c.a_scale, c.a_zp, c.w_codes, c.w_zp, c.w_scale, out_kind=1)
        assert eng.profile_kernel("gemm_op") == "gemm_i8f_pp3<%d>" % mi
        R.check_gemm(c, got, "dispatch by shape", ref=(None,) + R.gemm_reference(c)[1:2] + (None,))


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("M,Nn,K,f16_result", ((5, 100, 132, False), (129, 148, 560, True), (300, 515, 256, False)))
def test_chain_equals_op_qlinear(eng, M, Nn, K, f16_result):
    """op_quantize, op_quantize_weight and op_qgemm_ex one after the other return op_qlinear's bits"""
    r = np.random.default_rng(M + Nn + K)
    x, Wm, bias = r.standard_normal((M, K)).astype(F32), (0.1 * r.standard_normal((Nn, K))).astype(F32), r.standard_normal(Nn).astype(F32)
    y, xq, (xs, xz), wq, ws, wz = eng.op_qlinear(x, Wm, bias, relu=f16_result, f16_result=f16_result, details=True)
    aq, rs, (scale, zp) = eng.op_quantize(x, ld=_up(K, 128))
    w, cs, wzp, wsc, dz = eng.op_quantize_weight(Wm, ld=_up(K, 128))
    assert np.array_equal(aq[:, :K].astype(np.int32) + 128, xq) and (float(scale), int(zp)) == (xs, xz)
    assert np.array_equal(w[:, :K].astype(np.int32) + 128, wq) and np.array_equal(wsc, ws) and np.array_equal(wzp + 128, wz)
    y32, y16, _ = eng.op_qgemm_ex(xq, scale, int(zp), wq, wz, ws, bias=bias, relu=f16_result, out_kind=1 if f16_result else 0)
    assert np.array_equal(y16 if f16_result else y32, y)
