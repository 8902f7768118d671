"""CPU: the CIF conformance suite's case table (tests/cif_ref.py) on the reference alone.

What the GPU suite (tests/test_gpu_cif_conformance.py) relies on is proved here without a device: the inexact family makes the
cumsum scan's chunked walk round and the random family never does; the near-tie family holds an utterance of each disagreement
(fires > token_num, fires < token_num, sequential fires != cumsum fires); the float64 tier's bounds hold on both oracle functions; the
hand answers are what the oracle gives; at most 5 % of the random family's utterances are too close to an integer for the
fire-decision check.  The streaming CIF of the host library goes over the dyadic and near-tie sequences in one piece and in chunks."""
import ctypes as C
import functools

import numpy as np
import pytest

import cif_ref as CR
from oracle import model as om
from oracle import online as oo

VARIANTS = {"loop": om.Oracle.cif_fire, "cumsum": om.Oracle.cif_fire_cumsum}


@functools.lru_cache(maxsize=None)
def _oracle(name, variant):
    """(E, fire_count, token_num) of a table case on its one-hot hidden state (8 random channels where it has none)"""
    case = next(c for c in CR.cases() if c.name == name)
    H = case.H if case.H is not None else CR.random_hidden(case, 8)
    thr = case.threshold if variant == "loop" else 1.0
    return VARIANTS[variant](H, case.alphas, thr)


def test_table_has_what_the_issue_lists():
    by = {c.name: c for c in CR.cases()}
    assert len(by) == len(CR.cases())
    assert [c.alphas.shape[1] for c in CR.family("random")[:-1]] == list(CR.RANDOM_T1)
    assert max(c.alphas.shape[0] * (c.alphas.shape[1] - 1) for c in CR.cases()) == 4 * 1024
    rag = by["random_ragged"].alphas
    assert rag.shape[0] == 4 and not rag[1].any() and not rag[0, :150].any() and rag[2, :-1].min() > 0.5
    for c in CR.cases():
        assert c.alphas.dtype == np.float32 and not c.alphas.flags.writeable and c.what
        T = c.alphas.shape[1] - 1
        assert (c.H is not None) == (T <= 129)
        if c.H is not None:
            assert c.H.shape == (c.alphas.shape[0], T, CR.round_up(T, 4))
            assert (c.H.sum(axis=2) == 1).all() and (c.H[0].argmax(axis=1) == np.arange(T)).all()
        if c.family in ("random", "inexact", "threshold"):
            assert (c.alphas[:, -1] == CR.TAIL).all() or c.name == "random_ragged"
    assert len(CR.family("near_tie")) == len(CR.NEAR_TIE_T1) and len(CR.family("inexact")) == 7


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hand_answers(variant):
    E, fc, tn = _oracle("dyadic_hand", variant)
    W = CR.weight_matrix(E[0], int(fc[0]), 10)
    want = np.zeros((4, 10))
    for l, row in enumerate(CR.DYADIC_HAND_ROWS):
        for t, v in row.items():
            want[l, t] = v
    np.testing.assert_array_equal(W, want)
    assert CR.fire_frames(W, CR.DYADIC_HAND[0], variant) == list(CR.DYADIC_HAND_FIRES)
    assert int(fc[0]) == 4 and int(tn[0]) == 4                    # 4.45 in all
    E, fc, tn = _oracle("dyadic_ones", variant)
    assert int(fc[0]) == 33 and int(tn[0]) == 33
    np.testing.assert_array_equal(E[0, :32, :32], np.eye(32, dtype=np.float32))      # token l = frame l, the 33rd is the tail's
    assert not E[0, 32].any()
    E, fc, tn = _oracle("dyadic_zeros", variant)
    assert E.shape[1] == 0 and not fc.any() and not tn.any()
    E, fc, tn = _oracle("dyadic_single_frame", variant)
    assert int(fc[0]) == 1 and int(tn[0]) == 1 and E[0, 0, 0] == 0.75
    E, fc, tn = _oracle("dyadic_tail_only", variant)
    assert int(fc[0]) == 1 and int(tn[0]) == 1
    np.testing.assert_array_equal(E[0, 0, :5], [.125, .125, .25, 0, .125])
    tail_only = next(c for c in CR.cases() if c.name == "dyadic_tail_only")
    assert CR.fire_frames(CR.weight_matrix(E[0], 1, 5), tail_only.alphas[0], variant) == [5]


def test_near_tie_family_holds_every_disagreement():
    seen = {}
    more = less = differ = 0
    for c in CR.family("near_tie"):
        _, fs, tn = _oracle(c.name, "loop")
        _, fcs, tn2 = _oracle(c.name, "cumsum")
        np.testing.assert_array_equal(tn, tn2)
        for b, w in enumerate(CR.NEAR_TIE_WEIGHTS):
            seen[(w, c.alphas.shape[1])] = (int(fs[b]), int(tn[b]), int(fcs[b]))
            more += int(fs[b] > tn[b]) + int(fcs[b] > tn[b])
            less += int(fs[b] < tn[b]) + int(fcs[b] < tn[b])
            differ += int(fs[b] != fcs[b])
    for key, want in CR.NEAR_TIE_ANCHORS.items():
        assert seen[key] == want, (key, seen[key], want)
    assert more and less and differ, (more, less, differ)
    # a batch in which token_num exceeds the decoder length L = max fire_count does exist
    assert seen[(0.7, 50)][1] > seen[(0.7, 50)][0]


def test_inexact_family_rounds_and_random_family_does_not():
    """what proves that the device suite reaches cif_scan_cumsum_kernel's sequential redo — and leaves it on the other cases"""
    for c in CR.family("inexact"):
        for b in range(c.alphas.shape[0]):
            assert CR.cumsum_walk_inexact(c.alphas[b]), (c.name, b)
    for c in CR.family("random"):
        for b in range(c.alphas.shape[0]):
            assert not CR.cumsum_walk_inexact(c.alphas[b]), (c.name, b)
    # one case where the redo is visible in the result: the chunked walk on its own arrives at another fire table than the
    # sequential sum (on the random inexact cases the two differ by 1e-16, which float32(prefix) never shows)
    assert (CR.INEXACT_MIDPOINT.astype(np.float64)[0, :4].sum() == 2 - 2.0 ** -24 - 2.0 ** -52)
    inexact, fires = CR.cumsum_walk(CR.INEXACT_MIDPOINT[0])
    assert inexact and CR.sequential_prefix_fires(CR.INEXACT_MIDPOINT[0]) == [0, 8] and fires != [0, 8], fires
    _, fcm, _ = _oracle("inexact_midpoint", "cumsum")
    assert int(fcm[0]) == 2
    # the emulation itself: a sum that needs more than 53 bits rounds, dyadic sums do not
    assert CR.cumsum_walk_inexact(np.asarray([1.0, 2.0 ** -60], np.float32))
    assert not CR.cumsum_walk_inexact(CR.DYADIC_HAND[0])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_float64_tier_holds_on_the_oracle(variant):
    """rows, columns, monotonicity on every one-hot case; fire decisions on the random and inexact families"""
    worst_row = worst_col = 0.0
    checked = 0
    for c in CR.cases():
        if c.H is None or c.threshold != 1.0:
            continue
        E, fc, _ = _oracle(c.name, variant)
        T = c.alphas.shape[1] - 1
        for b in range(c.alphas.shape[0]):
            W = CR.weight_matrix(E[b], int(fc[b]), T)
            ff, re_, ce = CR.check_weights(W, c.alphas[b], variant)
            worst_row, worst_col = max(worst_row, re_), max(worst_col, ce)
            if c.family in ("random", "inexact"):
                want, decidable = CR.float64_crossings(c.alphas[b], variant)
                if decidable:
                    assert ff == want, (c.name, b)
                    checked += 1
    print("%s: largest |row sum - 1| %.3g, largest column error %.3g u alpha, %d utterances' fire frames compared" %
          (variant, worst_row, worst_col, checked))
    assert checked >= 20


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fire_counts_match_float64_crossings_and_skip_cap(variant):
    """every utterance of the random family, the long ones included (fire_count against the number of float64 crossings);
    at most 5 % of them may be too close to an integer to compare"""
    total = skipped = 0
    for c in CR.family("random"):
        _, fc, _ = _oracle(c.name, variant)
        for b in range(c.alphas.shape[0]):
            want, decidable = CR.float64_crossings(c.alphas[b], variant)
            total += 1
            if not decidable:
                skipped += 1
                continue
            assert int(fc[b]) == len(want), (c.name, b)
    print("%s: %d of %d random-family utterances skipped by the fire-decision check" % (variant, skipped, total))
    assert skipped <= 0.05 * total, (skipped, total)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _host_cif(lib, N, h, a):
    n, D = h.shape
    fired = np.zeros((n + 1, D), np.float32)
    nf, ca, ch = C.c_int32(), C.c_float(), np.zeros(D, np.float32)
    N.check(lib.pf_host_online_cif(_fp(h), _fp(a), n, D, 1.0, _fp(fired), n + 1, nf, ca, _fp(ch)))
    return fired[: nf.value].copy(), np.float32(ca.value), ch


@pytest.mark.parametrize("chunk", [0, 1, 2, 7])
def test_host_streaming_cif_on_the_dyadic_and_near_tie_sequences(chunk):
    """pf_host_online_cif against oracle.online.cif, bit for bit: each sequence in one piece (chunk 0) and in chunks of 1, 2 and 7
    frames, the carried weight and hidden state in front of every chunk as the streaming recognizer puts them"""
    from aliparaformerasr_amd import _native as N
    lib = N.load()
    D = 8
    for c in CR.family("dyadic") + CR.family("near_tie"):
        for b in range(c.alphas.shape[0]):
            a_all = c.alphas[b]
            h_all = np.random.default_rng([3, b, a_all.size]).standard_normal((a_all.size, D), dtype=np.float32)
            step = chunk or a_all.size
            carry_a, carry_h, n_fired = np.float32(0.0), np.zeros(D, np.float32), 0
            for s in range(0, a_all.size, step):
                h = np.ascontiguousarray(np.concatenate([carry_h[None], h_all[s:s + step]]), np.float32)
                a = np.ascontiguousarray(np.concatenate([[carry_a], a_all[s:s + step]]), np.float32)
                fired, ca, ch = _host_cif(lib, N, h, a)
                rf, ra, rh = oo.cif(h, a, 1.0)
                assert fired.shape == rf.shape, (c.name, b, s)
                np.testing.assert_array_equal(fired, rf)
                assert ca.tobytes() == np.float32(ra).tobytes(), (c.name, b, s, ca, ra)
                np.testing.assert_array_equal(ch, rh)
                carry_a, carry_h, n_fired = ca, ch, n_fired + fired.shape[0]
            if c.name == "dyadic_hand":
                assert n_fired == 4


def test_alpha_reference_saturates_both_ways():
    """the saturated alpha case holds logits beyond both ends in the float64 reference, in f16-operand and exact form"""
    from aliparaformerasr_amd import weights as Wt
    cfg = Wt.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    w = Wt.synth_weights(cfg, seed=5)
    H = CR.alpha_inputs("saturated", w, cfg)
    for operands in ("f16", "exact"):
        a, z = CR.alpha_ref(H, w, cfg, np.float64, operands)
        assert (z > CR.Z_SATURATED_HIGH).any() and (z < CR.Z_SATURATED_LOW).any(), (z.min(), z.max())
        assert (a[:, -1] == np.float32(cfg["cif_tail"])).all()
        a32, _ = CR.alpha_ref(H, w, cfg, np.float32, operands)
        assert (a32[:, :-1][z > CR.Z_SATURATED_HIGH] == np.float32(cfg["cif_smooth"] - cfg["cif_noise"])).all()
        assert (a32[:, :-1][z < CR.Z_SATURATED_LOW] == 0.0).all()
