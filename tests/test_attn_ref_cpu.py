"""CPU: the attention conformance designs of tests/attn_ref.py have teeth.  (a) The properties each design claims hold for
the float64 reference alone, at every shape of the GPU suite.  (b) A tile-wise numpy attention (64-key tiles, online
softmax, f16 P, the way k_attn.hip works) passes the assertion helper the GPU suite calls, and each of nine deliberately
wrong variants of it is rejected by that helper on at least one design at those shapes."""
import numpy as np
import pytest

import attn_ref as R


# ------------------------------------------------------------------------------------------------ (a) the designs
def test_select_code_gap_is_20_up_to_4096_keys():
    c = R.code(np.arange(4096))
    assert set(np.unique(c)) == {-1.0, 1.0} and (c[:, 120:] == 1).all()
    S = c @ c.T
    assert (np.diag(S) == 128).all()
    np.fill_diagonal(S, -np.inf)
    assert S.max() == 108                                    # the winner leads by at least 20 nats


@pytest.mark.parametrize("Lq,Lk", R.GRID_SHAPES)
def test_design_properties_hold_for_the_reference(Lq, Lk):
    B, H = 2, 2
    # select: every query's winning key leads by >= 20; the reference rounds to exactly V[pick]
    c = R.make_case("select", B, H, Lq, Lk)
    for x in (c.q, c.k, c.v):
        assert np.array_equal(x, x.astype(np.float16).astype(np.float32))            # exact in f16
    assert c.pick[:, :, 0].tolist() == [[Lk - 1] * H] * B
    ref = R.case_ref("select", B, H, Lq, Lk)
    S = np.einsum("bihd,bjhd->bhij", c.q.reshape(B, Lq, H, 128).astype(np.float64), c.k.reshape(B, Lk, H, 128).astype(np.float64))
    win = np.take_along_axis(S, c.pick[..., None], axis=-1)[..., 0]
    assert (win == 128).all()
    np.put_along_axis(S, c.pick[..., None], -np.inf, axis=-1)
    assert Lk == 1 or S.max() <= 108
    assert np.abs(ref.O - c.exact).max() <= 1.3e-7 * 4
    assert np.array_equal(R.f16_bits(ref.O), R.f16_bits(c.exact))
    assert (np.abs(c.exact) >= 0.25).all()
    # uniform: the answers are exact, and they are the ones the design promises
    c = R.make_case("uniform", B, H, Lq, Lk)
    assert np.array_equal(c.v, c.v.astype(np.float16).astype(np.float32)) and not c.q.any()
    ref = R.case_ref("uniform", B, H, Lq, Lk)
    assert np.abs(ref.O - c.exact).max() <= 1e-12
    e = c.exact.reshape(B, Lq, H, 128)
    assert (e[..., 0] == 1).all() and (e[..., 1] == 1).all() and (e[..., 2] == 1).all()
    assert (e[..., 3] == (0 if Lk <= 63 else 1 if Lk == 64 else 2)).all()
    # stress: |S| stays within 60 and reaches past the lazy-max threshold whenever there is a second tile
    ref = R.case_ref("stress", B, H, Lq, Lk)
    assert ref.smax.max() <= 60.5 and np.isfinite(ref.O).all()


def test_stress_patterns_are_the_ones_described():
    rng = np.random.default_rng(0)
    up, down = R._stress_scores(rng, 0, 193) / np.log(2), R._stress_scores(rng, 1, 193) / np.log(2)
    t = [up[64 * i:64 * i + 64].max() for i in range(4)]
    assert t[1] - t[0] < 8 < t[2] - t[0]                     # the running max is kept on tile 1 and raised on tile 2
    assert down[192] - down[:64].max() < -25                 # P of the last tile underflows f16 (2^-25 rounds to 0)
    assert np.argmax(R._stress_scores(rng, 2, 65)) == 64 and np.argmax(R._stress_scores(rng, 3, 65)) == 0
    assert (R._stress_scores(rng, 4, 65) == -50).all() and np.abs(R._stress_scores(rng, 5, 4000)).max() > 59


# ------------------------------------------------------------------------------------------------ (b) mutants
MUTANTS = ("last_key_dropped", "tail_row_twice", "mask_off_by_one", "k_halves_swapped", "v_heads_swapped", "next_batch_keys",
           "max_raised_without_rescale", "f16_sum_with_tail_at_one", "last_row_not_stored")


def tiled_attention(q, k, v, heads, mutant=None):
    """float64 model of the f16 kernel on rounded operands: per (batch, head) 64-key tiles, online softmax, P rounded to
    f16 for the numerator, unrounded in the denominator.  Behind the last key lies a NaN row, as in the suite's buffers."""
    B, Lq, Dm = q.shape
    Bk, Lk = k.shape[0], k.shape[1]
    out = np.zeros((B, Lq, Dm))
    for b in range(B):
        for h in range(heads):
            sl = slice(128 * h, 128 * h + 128)
            vsl = slice(128 * (3 - h), 128 * (3 - h) + 128) if mutant == "v_heads_swapped" and h in (1, 2) and heads == 4 else sl
            bk = ((b + 1) % B if mutant == "next_batch_keys" else b) % Bk
            kk, vv, n = k[bk][:, sl], v[b % Bk][:, vsl], Lk
            if mutant == "last_key_dropped" and Lk > 1:
                kk, vv, n = kk[:-1], vv[:-1], Lk - 1
            if mutant == "tail_row_twice":
                kk, vv, n = np.vstack([kk, kk[-1:]]), np.vstack([vv, vv[-1:]]), Lk + 1
            if mutant == "mask_off_by_one":
                kk, vv, n = np.vstack([kk, np.full((1, 128), np.nan)]), np.vstack([vv, np.full((1, 128), np.nan)]), Lk + 1
            if mutant == "k_halves_swapped":
                j = np.arange(n)
                kk = kk[np.where((j ^ 32) < n, j ^ 32, j)]
            m, l, o = np.full(Lq, -np.inf), np.zeros(Lq), np.zeros((Lq, 128))
            for j0 in range(0, n, 64):
                S = q[b][:, sl] @ kk[j0:j0 + 64].T
                m_new = np.maximum(m, S.max(axis=1))
                alpha = np.exp(m - m_new)
                P = np.exp(S - m_new[:, None])
                P16 = P.astype(np.float16).astype(np.float64)
                if mutant == "f16_sum_with_tail_at_one":
                    l = l * alpha + P16.sum(axis=1) + (64 - S.shape[1])
                else:
                    l = l * alpha + P.sum(axis=1)
                o = (o if mutant == "max_raised_without_rescale" else o * alpha[:, None]) + P16 @ vv[j0:j0 + 64]
                m = m_new
            out[b][:, sl] = o / l[:, None]
    return out


MUTANT_SHAPES = ((3, 4, 33, 65), (1, 2, 129, 193), (2, 4, 97, 129))


def _run(design, B, H, Lq, Lk, mutant):
    c = R.make_case(design, B, H, Lq, Lk)
    ref = R.case_ref(design, B, H, Lq, Lk)
    out = tiled_attention(R.round_operands(c.q, 0), R.round_operands(c.k, 0), R.round_operands(c.v, 0), H, mutant)
    raw = R.pack_raw(out, 0, store_rows=Lq - 1 if mutant == "last_row_not_stored" else None)
    return R.assert_conforms(c, ref, 0, raw, "%s %s" % (design, mutant))


@pytest.mark.parametrize("design", R.DESIGNS)
def test_the_correct_attention_passes(design):
    for (B, H, Lq, Lk) in MUTANT_SHAPES + ((2, 2, 1, 1), (1, 4, 31, 2), (2, 2, 33, 64)):
        assert _run(design, B, H, Lq, Lk, None) <= 1.0


def test_the_correct_attention_passes_in_every_kind_and_stride():
    c, H = R.make_case("random", 2, 2, 33, 65), 2
    for kind in (0, 1, 2):
        ref = R.case_ref("random", 2, 2, 33, 65, kind=kind)
        for o_ld in (0, 260):
            assert R.assert_conforms(c, ref, kind, R.pack_raw(ref.O, kind, o_ld), "kind %d" % kind) <= 1.0
    raw = R.pack_raw(ref.O, 2)
    raw[5, 256 + 7] ^= 0x4000                                # a wrong lo' half is a wrong value
    with pytest.raises(AssertionError):
        R.assert_conforms(c, ref, 2, raw)
    raw = R.pack_raw(ref.O, 1, 260)
    raw[3, 257] = 0                                          # a store into a pad column
    with pytest.raises(AssertionError, match="outside the valid region"):
        R.assert_conforms(c, R.case_ref("random", 2, 2, 33, 65, kind=1), 1, raw)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_is_rejected(mutant):
    caught = []
    for design in R.DESIGNS:
        for shape in MUTANT_SHAPES:
            try:
                _run(design, *shape, mutant)
            except AssertionError:
                caught.append((design, shape))
    print(mutant, "rejected by", sorted({d for d, _ in caught}))
    assert caught, "no design rejects " + mutant
    # the exact-answer designs are the ones meant to catch index and mask faults
    if mutant not in ("max_raised_without_rescale",):
        assert {d for d, _ in caught} & {"select", "uniform"}, caught
