"""GPU: the language model's walk on the device (lm_walk_kernel, csrc/k_lm.hip, through pf_op_lm_score) against the host scorer
(pf_host_lm_score) bit for bit — g and the state after every token — over the arc-list edge table (lists of 1 .. 9 and 4097
arcs probed at the first arc, the last, between two, below the first and above the last, V = 25 055), B = 3 sequences of
lengths (40, 1, 0) and one sequence of 300 tokens.  Outputs are canary-filled: a position past a length is not written."""
import numpy as np
import pytest

import ctcbeam_lm_ref as LR
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import LanguageModel

pytestmark = pytest.mark.gpu
G_CANARY, S_CANARY = 12345.0, -77


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


def native(model):
    return LanguageModel(model.order, model.ngrams, model.V, model.bos, model.eos, model.unk, model.oov, sorted(model.transparent))


def check(eng, lm, seqs, L, alpha, beta):
    """the device's g / state of every sequence against the host's, canaries past the lengths"""
    B = len(seqs)
    ids = np.full((B, L), 1 << 30, np.int32)                                         # poison past a length
    for b, y in enumerate(seqs):
        ids[b, :len(y)] = y
    lens = np.asarray([len(y) for y in seqs], np.int32)
    g, st = eng.op_lm_score(lm, ids, lens, alpha, beta, out=(np.full((B, L), G_CANARY), np.full((B, L), S_CANARY, np.int32)))
    for b, y in enumerate(seqs):
        _g, _s, gp, sp = lm.score(y, alpha, beta)
        assert g[b, :len(y)].view(np.uint64).tolist() == gp.view(np.uint64).tolist(), (b, y[:8])
        assert st[b, :len(y)].tolist() == sp.tolist(), (b, y[:8])
        assert (g[b, len(y):] == G_CANARY).all() and (st[b, len(y):] == S_CANARY).all()


def test_walk_over_the_arc_list_edges(any_engine):
    model, probes = LR.edge_model()
    lm = native(model)
    check(any_engine, lm, probes, 3, 0.9, 0.1)
    # the definition once more at the list ends of the longest list, so that host and device cannot be wrong alike
    for y in probes[-6:]:
        g, st = any_engine.op_lm_score(lm, np.asarray([y], np.int32), [len(y)], 0.9, 0.1)
        assert g[0].view(np.uint64).tolist() == np.asarray(model.score(y, 0.9, 0.1)[1]).view(np.uint64).tolist()
    lm.close()


@pytest.mark.parametrize("order", [1, 3, 8])
def test_walk_over_ragged_and_long_sequences(any_engine, order):
    rng = np.random.default_rng(order)
    V = 9
    grams = {(c,): (np.float32(rng.uniform(-4, -0.3)), np.float32(rng.uniform(-1, 0)) if c % 3 else None) for c in range(1, V) if c != 5}
    for k in range(2, order + 1):
        for x in range(40):
            w = tuple(int(c) for c in rng.integers(1, V, k))
            if 5 not in w:
                grams[w] = (np.float32(rng.uniform(-3, -0.1)), np.float32(rng.uniform(-0.8, 0)) if x % 3 else None)
    model = LR.Model(order, grams, V, bos=1, eos=2, transparent=(7,), oov=-3.5)
    lm = native(model)
    seqs = [[int(c) for c in rng.integers(0, V + 2, 40)], [3], []]
    check(any_engine, lm, seqs, 40, 0.37, 0.8)
    long = [int(c) for c in rng.integers(1, 4, 300)]                                  # a small alphabet: long matches
    check(any_engine, lm, [long], 300, 1.0, -0.5)
    g, _st = any_engine.op_lm_score(lm, np.asarray([long], np.int32), [300], 1.0, -0.5)
    assert g[0].view(np.uint64).tolist() == np.asarray(model.score(long, 1.0, -0.5)[1]).view(np.uint64).tolist()
    lm.close()


def test_refusals(any_engine):
    lm = LanguageModel(1, {(1,): (-1.0, None)}, 3)
    for a, b in ((-1.0, 0.0), (float("nan"), 0.0), (1.0, float("inf"))):
        with pytest.raises(N.PfError) as e:
            any_engine.op_lm_score(lm, np.ones((1, 2), np.int32), [2], a, b)
        assert e.value.code == N.PF_ERR_INVALID_ARG
    lm.close()
