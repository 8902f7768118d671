"""CPU: the designs, bounds and assertions of tests/layer_ref.py, which tests/test_gpu_layer_conformance.py applies to the
layer kernels (k_ffn.hip's decoder split forms, k_decmid.hip, fsmn_dec_ln_kernel) — proven here without a GPU:

  * every intermediate of the `steer` design is an integer below 2^24 or exactly representable (f16 where the device stores
    f16, fp32 with room to spare elsewhere), and the stated rstd values are exact in fp32;
  * an fp32 emulation of the split block that sums the hidden columns of each share in a shuffled order, one fp32 addition at
    a time, returns the bits of the float64 reference for every split count;
  * the `normal` bounds hold for that emulation (it is a legitimate implementation) with room, and the special rows (all-zero
    hidden, constant hidden, mean / std = 16) behave as stated;
  * numpy models of the ops with one defect each are rejected by the very assertions the GPU file uses."""
import numpy as np
import pytest

import layer_ref as LR

SPLITS = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def dec():
    c = LR.make_dec_case("steer", 129, out_proj=True)
    return c, LR.dec_reference(c)


@pytest.fixture(scope="module")
def mid():
    c = LR.make_mid_case("steer", 3, 37, (5, 37, 33))
    ref = LR.mid_reference(c)
    return c, ref, LR.mid_bounds(c, ref)


def _is_int(x, below=2.0 ** 24):
    x = np.asarray(x, np.float64)
    return bool((x == np.round(x)).all() and (np.abs(x) < below).all())


def _bits(x, unit):
    """significant bits x needs as a multiple of `unit`"""
    k = np.asarray(x, np.float64) / unit
    assert (k == np.round(k)).all()
    return float(np.log2(np.abs(k).max() + 1))


def test_steer_intermediates_are_exact(dec, mid):
    c, ref = dec
    P = LR._parts()
    ctx, wo, bo, resid, (g1, b1n) = c.out_proj
    assert all(_is_int(t) for t in (ctx, wo, bo, resid, g1, b1n, ref["x_out"]))
    assert _is_int(np.abs(ctx.astype(np.float64)) @ np.abs(wo.astype(np.float64)).T + np.abs(bo) + np.abs(resid))   # every partial sum
    # x_out = 2^q s: mean 0, mean square 4^q; the operand is the designed small-integer pattern, an f16
    x = ref["x_out"]
    assert (x.sum(1) == 0).all() and np.array_equal((x ** 2).mean(1), 4.0 ** (np.arange(c.M) % 4 + 1))
    assert _is_int(ref["a"], 4) and LR.is_f16(ref["a"]) and np.array_equal(ref["a"], c.a)
    # first product: W1 and b1 multiples of 2^-10, every partial sum |a||w1| + |b1| within 24 bits; the hidden 0 | 2^(p + 1)
    assert LR.is_f16(c.w1) and _bits(c.w1, 2.0 ** -10) <= 11
    assert _bits(np.abs(ref["a"]) @ np.abs(c.w1.astype(np.float64)).T + np.abs(c.b1), 2.0 ** -10) < 24
    p = P["p"][c.types]
    on = P["on"][c.types]
    assert np.array_equal(ref["h"], np.where(on, 2.0 ** (p + 1)[:, None], 0.0)) and (on.sum(1) == 1024).all()
    assert np.array_equal(ref["h"].mean(1), 2.0 ** p) and np.array_equal((ref["h"] ** 2).mean(1) - ref["h"].mean(1) ** 2, 4.0 ** p)
    assert _bits(ref["h"].sum(1), 1) <= 24 and _bits((ref["h"] ** 2).sum(1) / 4.0 ** (p + 1), 1) <= 11       # k 4^(p + 1), k <= 1024
    # second product: G integers, f16; sums of |h||G| a multiple of 2^(p + 1) within 24 bits; c and d as designed
    G = ref["G"]
    assert _is_int(G, 2048) and LR.is_f16(G) and not np.array_equal(c.gf[None, :] * c.w2.astype(np.float64), G)
    assert (((ref["h"] @ np.abs(G).T) / 2.0 ** (p + 1)[:, None]) < 2.0 ** 24).all()
    assert np.array_equal(G.sum(1), P["c"]) and (P["c"] != 0).all() and np.array_equal(ref["d"], P["d"]) and (P["d"] != 0).any()
    assert np.array_equal(ref["t"], (2.0 ** P["rj"][c.types])[:, None] * P["u"][c.types])
    # the middle: tn small integers, x + FSMN(tn) a multiple of 2^-8 within 24 bits
    m, mref, _ = mid
    valid = (np.arange(m.L)[None, :] < m.token_num[:, None]).reshape(-1)
    assert _is_int(mref["tn"], 8) and (mref["tn"][~valid] == 0).all() and (np.abs(mref["tn"][valid]).max(1) > 0).all()
    assert _bits(mref["xmag"], 2.0 ** -8) < 24
    assert len(np.unique(np.abs(m.taps[:, 0]))) == 11 and _bits(m.taps, 2.0 ** -8) <= 7


def test_stated_rstd_values_are_exact_in_fp32():
    for p in range(0, 14):
        for eps in (np.float32(1e-12),):
            v = np.float32(4.0 ** p) + eps                      # 1e-12 is below half an ulp of 1
            assert np.float32(1.0) / np.sqrt(v, dtype=np.float32) == np.float32(2.0 ** -p)
        assert np.float32(1.0 / np.sqrt(4.0 ** p + 1e-12)) == np.float32(2.0 ** -p)       # the finishing pass: double, then fp32
        assert LR.fl32(1 / np.sqrt(4.0 ** p + 1e-12)) == 2.0 ** -p


@pytest.mark.parametrize("splits", SPLITS)
def test_shuffled_fp32_emulation_returns_the_reference_bits(dec, splits):
    c, ref = dec
    m = LR.dec_model(c, splits, shuffle=np.random.default_rng(splits))
    LR.assert_exact(None, ref["t"], m["t"], "shuffled fp32 model, splits %d" % splits)
    LR.assert_exact(None, ref["t"], LR.dec_model(c, splits)["t"], "fp32 model, splits %d" % splits)


def test_normal_bounds_hold_for_the_fp32_emulation_and_the_special_rows():
    for special, op in ((None, True), ("offset", False), ("zero", False)):
        c = LR.make_dec_case("normal", 9, out_proj=op, special=special)
        ref = LR.dec_reference(c)
        bnd = LR.dec_bounds(c, ref)
        assert np.isfinite(bnd["t"]).all() and np.isfinite(ref["t"]).all()
        ratio = LR.assert_bounded(ref["t"], bnd["t"], LR.dec_model(c, 3, shuffle=np.random.default_rng(1))["t"], "normal %s" % special)
        assert ratio < 1
        if special == "offset":
            assert (ref["h"][0] == 16).all() and np.array_equal(ref["t"][0], ref["d"])           # the constant row: t = d
            assert 200 < np.median(bnd["rho"][1:]) < 320                                         # (mean / std)^2 = 256
        if special == "zero":
            assert (ref["h"][0] == 0).all() and np.array_equal(ref["t"][0], ref["d"]) and (bnd["t"][0] < 1e-6).all()
        if not op:                                             # wide as it is (layer_ref's docstring), the bound rejects a dropped share
            with pytest.raises(AssertionError):
                LR.assert_bounded(ref["t"], bnd["t"], LR.dec_model(c, 3, mutate="share_rows_dropped")["t"])


DEC_MUTANTS = ("share_rows_dropped", "share_stats_dropped", "ninth_chunk_bias", "unrounded_colsum", "operand_rows_32_swapped", "stale_x_out")


@pytest.mark.parametrize("mutate", DEC_MUTANTS)
def test_block_mutants_are_rejected(dec, mutate):
    c, ref = dec
    m = LR.dec_model(c, 3, mutate=mutate)
    with pytest.raises(AssertionError):
        LR.assert_exact(None, ref["t"], m["t"], mutate)
        LR.assert_exact(None, ref["x_out"], m["x_out"], mutate)


MID_MUTANTS = ("tap_across_edge", "window_off_by_one", "input_mask_missing", "output_mask_missing", "norm3_skipped_on_masked",
               "q_groups_swapped", "q_unscaled", "bias_after_scale")


def test_the_unmutated_middle_passes(mid):
    c, ref, bnd = mid
    m = LR.mid_model(c)
    rx, rq = LR.check_mid(c, ref, bnd, m["x"], m["q"], "model", exact_x=True)
    assert rx == 0 and rq <= 1


@pytest.mark.parametrize("mutate", MID_MUTANTS)
def test_middle_mutants_are_rejected(mid, mutate):
    c, ref, bnd = mid
    m = LR.mid_model(c, mutate=mutate)
    with pytest.raises(AssertionError):
        LR.check_mid(c, ref, bnd, m["x"], m["q"], mutate, exact_x=True)


@pytest.mark.parametrize("k", (11, 21))
def test_fsmn_dec_ln_design_and_its_mutants(k):
    c = LR.make_fdl_case(3, 40, k, (5, 40, 33))
    ref = LR.fdl_reference(c)
    assert _bits(ref["x"], 2.0 ** -8) < 24 and len(np.unique(np.abs(c.taps[:, 0]))) == k
    for mutate in ("tap_across_edge", "window_off_by_one", "input_mask_missing", "output_mask_missing"):
        with pytest.raises(AssertionError):
            LR.assert_exact(None, ref["x"], LR.fdl_reference(c, mutate=mutate)["x"], mutate)


@pytest.mark.parametrize("resid", (True, False))
def test_encoder_tail_steer_design_and_an_ignored_utterance_edge(resid):
    for B, T in ((7, 9), (1, 65)):
        c = LR.make_enc_case("steer", B, T, resid)
        ref = LR.enc_reference(c)
        xm = ref["x_mid"]
        assert (xm.sum(1) == 0).all() and (np.abs(xm) == np.abs(xm[:, :1])).all() and _bits(np.abs(xm[:, 0]), 1) <= 5     # +-2^q, balanced
        assert all(LR.is_f16(t) for t in (c.ctx, c.wo, c.v, c.w1, c.w2)) and _bits(ref["xmag"], 2.0 ** -8) < 24
        assert np.array_equal(ref["a_raw"], ref["a"]) and _is_int(ref["a"], 4)
        assert set(np.unique(ref["h"])) <= {0.0, 2.0, 4.0, 8.0, 16.0, 32.0}
        assert _is_int(ref["h"] @ np.abs(c.w2.astype(np.float64)).T + np.abs(c.b2) + np.abs(xm)) and _is_int(ref["x"])
        bnd = LR.enc_bounds(c, ref)
        assert (bnd["x"] == 0).all() and np.isfinite(bnd["qkv"]).all()
        if B > 1:
            with pytest.raises(AssertionError):
                LR.assert_exact(None, ref["x"], LR.enc_reference(c, mutate="tap_across_edge")["x"], "edge ignored")


def test_token_num_sets_cover_every_value_at_every_position():
    seen = set()
    for L, t in LR.MID_CASES:
        assert len(t) == 3 and all(0 <= v <= L for v in t) and (3 * L) % 64 != 0
        for pos, v in enumerate(t):
            seen |= {(s, pos) for s in ((v,) if v in LR.TOKEN_SET else ()) + (("L-1",) if v == L - 1 else ()) + (("L",) if v == L else ())}
    for v in LR.TOKEN_SET + ("L-1", "L"):
        assert {(v, 0), (v, 1), (v, 2)} <= seen, v
    assert {L for L, _ in LR.MID_CASES} == {1, 5, 31, 32, 33, 37, 70}
