"""CPU: the designs and assertion helpers of tests/int8_ref.py reject wrong implementations of the int8 path.  Every mutant
of int8_ref.MUTANTS_Q / MUTANTS_G is a plausible kernel bug; for each one a named design must raise in the very helper the GPU
suite (tests/test_gpu_int8_conformance.py) calls, and the unmutated model must pass every design."""
import numpy as np
import pytest

import gemm_ref as G
import int8_ref as R

F32 = np.float32
SHAPES = ((1, 4), (3, 252), (4, 256), (5, 260), (257, 560))


def _as_op(codes, scale, zp, ld=None):
    """the quantiser op's outputs (a' [rows, ld], rowsum, (scale, zp)) for a model's codes"""
    rows, cols = codes.shape
    aq = np.zeros((rows, ld or cols), np.int8)
    aq[:, :cols] = (codes - 128).astype(np.int8)
    return aq, R.rowsum_of(codes), (F32(scale), F32(zp))


def _quant_cases(design, f16=False):
    if design == "grid":
        return [R.make_quant_case("grid", r, c, j=j, z=z, f16=f16) for (r, c) in SHAPES for j in (3, 7, 10) for z in (100, 101)]
    if design == "place":
        return [R.make_quant_case("place", r, c, f16=f16, where=w) for (r, c) in SHAPES[1:]
                for w in (("first", "last"), ("last", "first"), ("last quad of a row", "row not a multiple of 4 from the end"),
                          ("row not a multiple of 4 from the end", "last quad of a row"))]
    return [R.make_quant_case(design, r, c, f16=f16) for (r, c) in SHAPES]


@pytest.mark.parametrize("f16", (False, True))
@pytest.mark.parametrize("design", R.Q_DESIGNS)
def test_the_oracle_passes_every_quantiser_design(design, f16):
    for c in _quant_cases(design, f16):
        R.check_quant(c, *_as_op(c.codes, c.scale, c.zp, ld=c.cols + 12), what=design)
        assert np.array_equal(R.quantize_model(c.x)[0], c.codes)


def test_grid_conditions_checked_with_the_oracle():
    """the issue's figures: for j = 3, 7, 10 the scale is exact, the zero point 100 / 102, and the second form saturates"""
    for j in (3, 7, 10):
        for z, zp in ((100, 100), (101, 102)):
            c = R.make_quant_case("grid", 4, 256, j=j, z=z)
            assert c.scale == F32(2.0 ** -j) and c.zp == zp
            v = np.rint(c.x.astype(np.float64) * 2.0 ** j) + zp
            assert ((v > 255).sum() >= 1) == (z == 101)
            ties = np.abs(c.x.astype(np.float64) * 2.0 ** j % 1.0) == 0.5
            assert ties.sum() >= 255                                    # every code boundary is met as a tie
    assert R.make_quant_case("recip", 4, 256).scale != 0


Q_KILLERS = {"recip": "recip", "half_away": "grid", "trunc": "grid", "zp_f64": "zptie", "no_zero": "nonneg", "scale0": "zeros",
             "wrap": "grid", "pad_row": "single", "last_quad": "place"}


@pytest.mark.parametrize("mutant", R.MUTANTS_Q)
def test_quantiser_mutants_are_rejected(mutant):
    assert set(Q_KILLERS) == set(R.MUTANTS_Q)
    killed = 0
    for f16 in (False, True):
        for c in _quant_cases(Q_KILLERS[mutant], f16):
            if c.rows * c.cols < 16 and mutant in ("recip", "half_away", "trunc", "wrap"):
                continue                                                # the four-element tensor holds min', max' and two more values
            if mutant == "wrap" and c.codes.max() < 255:
                continue                                                # z = 100 does not saturate
            if mutant == "last_quad" and c.x.reshape(-1)[-4:].max() < 9 and c.x.reshape(-1)[-4:].min() > -7:
                continue                                                # neither extremum in the last quad
            with pytest.raises(AssertionError):
                R.check_quant(c, *_as_op(*R.quantize_model(c.x, mutant)), what=mutant)
            killed += 1
    assert killed >= 4, killed
    if mutant == "no_zero":
        c = R.make_quant_case("nonpos", 5, 260)
        with pytest.raises(AssertionError):
            R.check_quant(c, *_as_op(*R.quantize_model(c.x, mutant)))


def test_check_quant_rejects_pad_columns_and_row_sums():
    c = R.make_quant_case("grid", 5, 260)
    aq, rs, par = _as_op(c.codes, c.scale, c.zp, ld=384)
    R.check_quant(c, aq, rs, par)
    bad = aq.copy()
    bad[3, 300] = 1
    with pytest.raises(AssertionError, match="pad column"):
        R.check_quant(c, bad, rs, par)
    bad = rs.copy()
    bad[4] += 1
    with pytest.raises(AssertionError, match="row sums"):
        R.check_quant(c, aq, bad, par)
    with pytest.raises(AssertionError, match="scale"):
        R.check_quant(c, aq, rs, (np.nextafter(par[0], F32(1)), par[1]))


def test_places_reach_every_loop_of_the_min_max_pass():
    rows, cols = R.UNROLL_SHAPE
    p = R.places(rows, cols)
    total, st = rows * cols // 4, R.MINMAX_STRIDE
    assert total > 3 * st
    for k in range(4):
        q = p["unrolled slot %d" % k] // 4
        i = q % st                                                      # the thread's first quad
        assert i + 3 * st < total and q == i + k * st                   # the unrolled trip runs for it, and q is its k-th load
    for name in ("remainder loop, first trip", "remainder loop, last trip"):
        q = p[name] // 4
        assert not (q % st + 3 * st < total)                            # only the remainder loop visits this thread's quads
    assert len(set(p.values())) == len(p)
    names = list(p)
    for i, name in enumerate(names[:3]):                                # the model that misses the last quad is caught there
        c = R.make_quant_case("place", rows, cols, where=(name, names[(i + 1) % len(names)]))
        assert c.x.reshape(-1)[p[name]] == -7


# ------------------------------------------------------------------------------------------------ weights
def test_weight_design_and_pack_dz():
    for N, K in ((1, 4), (5, 60), (130, 68)):
        W, codes, scale, zp = R.make_weight_case(N, K)
        ld = -(-K // 128) * 128
        w = np.zeros((N, ld), np.int8)
        w[:, :K] = codes - 128
        cs = (codes - 128).sum(axis=1).astype(np.int32)
        got = (w, cs, (zp - 128).astype(np.int32), scale, R.pack_dz(cs, zp - 128, K))
        R.check_weight(codes, scale, zp, K, got)
        with pytest.raises(AssertionError, match="dz"):
            R.check_weight(codes, scale, zp, K, got[:4] + (R.pack_dz(cs, zp - 128, ld),))
    # the extreme column sums of the packed word at its largest K, and one past it
    for code, z in ((0, 0), (0, 255), (255, 0), (255, 255)):
        dz = R.pack_dz([(code - 128) * 16384], [z - 128], 16384)
        assert dz[0] >> 8 == (code - z) * 16384 and np.int8(dz[0] & 255) == z - 128
    with pytest.raises(AssertionError):
        R.pack_dz([127 * 40000], [-128], 40000)                         # the word's 24 bits do not hold 255 K


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln32(c):
    """LayerNorm in float32 (numpy's pairwise sums, not the kernel's order): what a correct kernel may return"""
    x = c.x.astype(F32)
    d = x - x.mean(axis=1, keepdims=True, dtype=F32)
    var = (d * d).mean(axis=1, keepdims=True, dtype=F32)
    return (d / np.sqrt(var + F32(1e-12)) * c.gamma + c.beta).astype(F32)


@pytest.mark.parametrize("D", (4, 128, 512, 560, 2048))
def test_ln_exact_is_the_grid_design(D):
    for rows in (1, 3, 4, 5):
        for z in (100, 101):
            c = R.make_ln_case("ln_exact", rows, D, z=z)
            assert np.array_equal(_ln32(c), c.y)                        # exact in another summation order too
            R.check_quant(c, *_as_op(c.codes, c.scale, c.zp, ld=-(-D // 128) * 128), what="ln_exact")
            for mutant in ("half_away", "trunc"):
                if D >= 128:
                    with pytest.raises(AssertionError):
                        R.check_quant(c, *_as_op(*R.quantize_model(c.y, mutant)))


@pytest.mark.parametrize("rows,D,seed", R.LN_NORMAL_CASES)
def test_ln_normal_share_left_out_and_rejections(rows, D, seed):
    c = R.make_ln_case("ln_normal", rows, D, seed=seed)
    share = R.ln_left_out(c)
    print("ln_normal rows %d D %d seed %d: share of cells left out %.4f" % (rows, D, seed, share))
    assert share < R.LN_LEFT_OUT_MAX
    codes, scale, zp = R.quantize_model(_ln32(c))
    near = R.check_ln_normal(c, *_as_op(codes, scale, zp))
    assert near < R.LN_LEFT_OUT_MAX
    with pytest.raises(AssertionError):                                 # truncation moves every code boundary by half a code
        R.check_ln_normal(c, *_as_op(*R.quantize_model(_ln32(c), "trunc")))
    # an epsilon of 1e-2, a scale off by one per cent, one code off by two: outside what the bound allows
    y_bad = G.ln_ref(c.x, c.gamma, c.beta, eps=1e-2)
    with pytest.raises(AssertionError):
        R.check_ln_normal(c, *_as_op(*R.quantize_model(y_bad.astype(F32))))
    with pytest.raises(AssertionError):
        R.check_ln_normal(c, *_as_op(codes, scale * F32(1.01), zp))
    bad = codes.copy()
    bad[0, 0] += 2 if bad[0, 0] < 200 else -2
    with pytest.raises(AssertionError):
        R.check_ln_normal(c, *_as_op(bad, scale, zp))


# ------------------------------------------------------------------------------------------------ the integer GEMM
G_KILLERS = {
    "kpad": dict(design="extreme", M=5, N=100, K=132, variant=0),
    "cast_trunc": dict(design="extreme", M=5, N=100, K=560, variant=2),
    "scale_order": dict(design="random", M=33, N=100, K=132),
    "bias_after_scale": dict(design="place", M=33, N=100, K=132, bias=True, scale_cols=64, scale=0.125),
    "relu_before_resid": dict(design="random", M=33, N=100, K=132, resid=True, relu=True),
    "zp_per_row": dict(design="place", M=33, N=100, K=132),
    "range_pad_row": dict(design="random", M=33, N=100, K=132, out_kind=1),
    "range_unrounded": dict(design="random", M=33, N=100, K=132, out_kind=1),
}


@pytest.mark.parametrize("mutant", R.MUTANTS_G)
def test_gemm_mutants_are_rejected(mutant):
    assert set(G_KILLERS) == set(R.MUTANTS_G)
    c = R.make_gemm_case(**G_KILLERS[mutant])
    R.check_gemm(c, R.gemm_reference(c), what=mutant)
    with pytest.raises(AssertionError):
        R.check_gemm(c, R.gemm_reference(c, mutant), what=mutant)


@pytest.mark.parametrize("design", R.G_DESIGNS)
def test_gemm_designs_hold_their_conditions(design):
    for M, N, K in ((1, 64, 16), (129, 100, 132), (300, 515, 560), (4, 64, 16384)):
        for kind in (0, 1, 2, 3):
            for variant in ((0, 1, 2) if design == "extreme" else (0,)):
                c = R.make_gemm_case(design, M, N, K, out_kind=kind, variant=variant)
                y32, y16, rng = R.gemm_reference(c)
                assert np.isfinite(y16).all() and rng[0] <= 0 <= rng[1]
                if design == "extreme" and K > 257:
                    assert np.abs(R.integer_sums(c)).max() > 2 ** 24   # the cast to float rounds
                if design == "ties":
                    assert (y16 != y32).all() and (np.abs(y16) % 4 == 0).all()      # every f16 result was a tie, sent to even
                if design == "place":
                    k = (G.PLACE_P * np.arange(M)) % K
                    assert np.array_equal(y32, (c.w_codes[:, k].T.astype(np.int64) - c.w_zp[None, :]).astype(F32))


def test_place_names_the_origin_of_a_wrong_value():
    c = R.make_gemm_case("place", 33, 100, 132)
    y32, y16, rng = R.gemm_reference(c)
    bad = y32.copy()
    bad[7, 9] = float(int(c.w_codes[9, 5]) - int(c.w_zp[9]))
    with pytest.raises(AssertionError, match=r"wanted k %d" % ((G.PLACE_P * 7) % 132)):
        R.check_gemm(c, (bad, None, None))
    with pytest.raises(AssertionError, match="range"):
        R.check_gemm(c, (y32, None, (rng[0], rng[1] + 1)))


def test_non_power_of_two_scale_only_where_the_pipeline_uses_it():
    R.make_gemm_case("random", 5, 128, 132, bias=True, scale_cols=64, scale=R.QSCALE, out_kind=1)
    with pytest.raises(AssertionError):
        R.make_gemm_case("random", 5, 128, 132, bias=True, resid=True, scale_cols=64, scale=R.QSCALE, out_kind=0)
