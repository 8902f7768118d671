"""CPU: tests/fsmn_ref.py against independent formulations, the exactness of its dyadic design, and the discriminating power of
the cases tests/test_gpu_fsmn_conformance.py runs.

  * fsmn() against oracle.model.fsmn (torch conv1d, float64) without a mask, under a binary, a fractional and a length mask;
    against rows_ref.fsmn_stream_ref with a zero cache and one call (that form looks back only: with k - 1 - left zero rows
    appended, its sum at row l + k - 1 - left is ours at row l); against layer_ref.fsmn_dec;
  * the dyadic design evaluated in fp32 in forward, reversed and pairwise order equals the float64 value bit for bit, and
    check() accepts it; the normal design evaluated in fp32 in forward order stays inside the derived bound;
  * KILLS: each of the eleven wrong kernels of fsmn_ref.MUTANTS (an off-by-one `left` in both directions) is rejected by
    check() on the named case, a case of the GPU table at D = 8; test_every_mutant_is_rejected asserts exactly that pairing and
    counts, per mutant, how many cases of the D = 8 table reject it."""
import numpy as np
import pytest
import torch

import fsmn_ref as F
import layer_ref as LR
import rows_ref as R
from oracle import model as om

# mutant -> the case of the GPU table that rejects it (every one at D = 8, B T D <= 3 * 33 * 8)
KILLS = {
    "left_plus": "enc-dyadic-k3-B1-T2-D8",
    "left_minus": "enc-dyadic-k3-B1-T2-D8",
    "taps_reversed": "enc-dyadic-k5-B1-T4-D8",
    "no_identity": "enc-dyadic-k3-B1-T1-D8",
    "double_identity": "enc-dyadic-k3-B1-T1-D8",
    "seam": "enc-dyadic-k11-B3-T9-D8-ld24+16",
    "mask_input_only": "dec-dyadic-k9-B3-T17-D8-n20.5.17-inf",
    "mask_output_only": "dec-dyadic-k9-B3-T17-D8-n20.5.17-inf",
    "token_le": "dec-dyadic-k11-B3-T17-D8-n20.8.17-inf",
    "skip_last_frame": "enc-dyadic-k7-B1-T9-D8",
    "masked_x_plus_zero": "dec-dyadic-k9-B3-T17-D8-n20.16.17-nan",
    "clamped_edge": "f32-dyadic-k11-B1-T5-D8",
}


def _table(D=8):
    specs = []
    for k in F.KS_ENC:
        specs += F.enc_specs(k, D)
    specs += F.win_specs(D) + F.generic_specs(D)
    for k in (11, 21, 9):
        specs += F.dec_specs(k, D)
    return specs


def _rejects(spec, got):
    try:
        with np.errstate(all="ignore"):
            F.check(spec, got)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("k", (3, 5, 9, 11, 21))
def test_definition_is_the_oracles_conv1d(k):
    r = np.random.default_rng(k)
    for (B, T, D) in ((1, 1, 4), (3, 7, 8), (2, 33, 12)):
        v, w = r.standard_normal((B, T, D)), 0.1 * r.standard_normal((k, D))
        lens = r.integers(0, T + 1, B)
        binary = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)
        frac = r.choice([0.0, 0.25, 0.5, 1.0], (B, T))
        for mask in (None, binary, frac):
            want = om.fsmn(torch.from_numpy(v), torch.from_numpy(w.T.copy()), k, None if mask is None else torch.from_numpy(mask)[..., None]).numpy()
            got, mag = F.fsmn(v, w, k, mask=mask)
            assert np.abs(got - want).max() < 1e-13 and (mag >= np.abs(got) - 1e-13).all()
        want = om.fsmn(torch.from_numpy(v), torch.from_numpy(w.T.copy()), k, torch.from_numpy(binary)[..., None]).numpy()
        assert np.abs(F.fsmn(v, w, k, valid=lens)[0] - want).max() < 1e-13


@pytest.mark.parametrize("k", (3, 11, 21))
def test_definition_is_the_streaming_reference_with_a_zero_cache(k):
    """fsmn_stream_ref computes x + sum_j w_j xc[p + j] + tn[p] over xc = [k - 1 zeros | tn]: a window that looks back k - 1
    rows from p.  Ours reaches `left` rows back and right = k - 1 - left rows ahead of l: with `right` zero rows appended, its
    sum at l is the streaming sum at p = l + right; the identity term is taken out on both sides"""
    r = np.random.default_rng(k)
    B, L, D = 3, 19, 8
    left = (k - 1) // 2
    right = k - 1 - left
    tn, w = r.standard_normal((B, L, D)), 0.1 * r.standard_normal((k, D))
    lens = np.array([L, 7, 0])
    tn = np.where((np.arange(L)[None, :] < lens[:, None])[..., None], tn, 0.0)
    padded = np.concatenate([tn, np.zeros((B, right, D))], axis=1)
    xs, _, _ = R.fsmn_stream_ref(padded, w, np.full(B, L + right), np.zeros((B, D, k - 1)), np.zeros_like(padded))
    conv_stream = (xs - padded)[:, right:]                                                # sum_j w_j tn[l + j - left]
    ours, _ = F.fsmn(tn, w, k, valid=np.full(B, L))
    assert np.abs((ours - tn) - conv_stream).max() < 1e-13


@pytest.mark.parametrize("k", (9, 11, 21))
def test_definition_is_layer_refs_decoder_form(k):
    r = np.random.default_rng(k)
    B, L, D = 3, 17, 8
    tn, x, w = r.standard_normal((B, L, D)), r.standard_normal((B, L, D)), 0.1 * r.standard_normal((k, D))
    for num in ((L, 5, 0), (L + 3, L, 1)):
        want, wmag, _ = LR.fsmn_dec(tn, w, np.asarray(num), x)
        y, mag = F.fsmn(tn, w, k, valid=num)
        ok = (np.arange(L)[None, :] < np.asarray(num)[:, None])[..., None]
        assert np.abs(np.where(ok, x + y, x) - want).max() < 1e-13
        assert np.abs(np.where(ok, np.abs(x) + mag, 0.0) - wmag).max() < 1e-13


# ------------------------------------------------------------------------------------------------ the designs
def test_dyadic_is_exact_in_fp32_in_any_order():
    n = 0
    for spec in _table():
        if spec.design != "dyadic":
            continue
        ref, bnd = F.expect(spec)
        assert not bnd.any()
        with np.errstate(all="ignore"):
            outs = [F.evaluate(spec, order=o) for o in ("forward", "reversed", "pairwise")]
        for o in outs:
            assert F.check(spec, o) == 0.0
            assert np.array_equal(R.bits(o), R.bits(outs[0])), spec.name
        n += 1
    assert n > 300


def test_normal_in_fp32_stays_inside_the_derived_bound():
    """an fp32 evaluation with separately rounded products (more roundings than the kernels' FMAs) uses a part of the bound"""
    worst = 0.0
    for spec in _table():
        if spec.design == "normal":
            with np.errstate(all="ignore"):
                worst = max(worst, F.check(spec, F.evaluate(spec)))
    assert 0.0 < worst < 1.0, worst


def test_seam_rows_are_loud():
    """make_case asserts it for every dyadic case with B > 1; here once by hand: the last row of utterance 0 under a tap that
    reaches row 0 of utterance 1"""
    spec = [s for s in F.enc_specs(11, 8) if s.name == KILLS["seam"]][0]
    c = F.make_case(spec)
    y, _ = F.fsmn(c.v, c.taps, 11)
    ys, _ = F.fsmn(c.v, c.taps, 11, mutate="seam")
    d = np.abs(ys - y)[0, spec.T - 1]
    assert (d >= 1.0).all() and np.abs(y).max() < 2.0 ** 9


# ------------------------------------------------------------------------------------------------ the mutants
def test_every_mutant_is_rejected():
    table = {s.name: s for s in _table()}
    assert set(KILLS) == set(F.MUTANTS)
    for mutant, name in KILLS.items():
        assert name in table, name
        with np.errstate(all="ignore"):
            got = F.evaluate(table[name], mutate=mutant)
        assert _rejects(table[name], got), "%s survives %s" % (mutant, name)
        assert not _rejects(table[name], F.evaluate(table[name])), name
    counts = {}
    for mutant in F.MUTANTS:
        kinds = ("dec",) if mutant in ("mask_input_only", "mask_output_only", "token_le", "masked_x_plus_zero") else ("enc", "f32", "dec")
        with np.errstate(all="ignore"):
            counts[mutant] = sum(_rejects(s, F.evaluate(s, mutate=mutant)) for s in table.values() if s.kind in kinds and s.design == "dyadic")
    print("cases of the D = 8 table that reject each mutant:", counts)
    assert min(counts.values()) >= 10, counts
