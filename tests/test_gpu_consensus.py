"""GPU: the consensus kernels (csrc/k_consensus.hip) against the definition in plain Python (tests/consensus_ref.py), exactly:
winner and D as integers, risk and conf bit for bit.  Every list goes through pf_op_consensus, whose sentinels refuse a result
that was not written and a guard cell that was, and through the plain pf_engine_consensus; then all lists in one call, forward
and reversed; then the recogniser's step on its own Alternatives."""
import ctypes as C

import pytest

import consensus_cases as K
import consensus_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu
NAMES = sorted(K.CASES)
bits, same = K.bits, K.same


@pytest.fixture(scope="module")
def eng():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


@pytest.mark.parametrize("op", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_one_list_equals_the_definition(eng, name, op):
    hyps, p = K.CASES[name]
    (got,) = eng.consensus([hyps], [p], op=op)
    assert same(got, K.want(name)), name


def test_a_list_does_not_depend_on_its_batch(eng):
    lists, weights = [K.CASES[n][0] for n in NAMES], [K.CASES[n][1] for n in NAMES]
    fwd = eng.consensus(lists, weights, op=True)
    rev = eng.consensus(lists[::-1], weights[::-1], op=True)[::-1]
    for name, a, b in zip(NAMES, fwd, rev):
        assert same(a, K.want(name)) and same(b, K.want(name)), name
    three = ("one", "tie", "five")                                             # L = 3, N = 1, 3, 5, D not asked for
    got = eng.consensus([K.CASES[n][0] for n in three], [K.CASES[n][1] for n in three], want_D=False)
    for name, r in zip(three, got):
        w, risk, conf, _ = K.want(name)
        assert (r.winner, bits(r.risk), bits(r.conf), r.D) == (w, bits(risk), bits(conf), None), name


def test_refusals_launch_nothing(eng):
    eng.profile(True)
    eng.profile_reset()
    for lists, weights, code in (([[[1]] * 65], [[1.0] * 65], N.PF_ERR_INVALID_ARG), ([[[1] * 256]], [[1.0]], N.PF_ERR_INVALID_ARG),
                                 ([[[1], [2]]], [[1.0, -1.0]], N.PF_ERR_INVALID_ARG), ([[[1], [2]]], [[1.0, float("nan")]], N.PF_ERR_INVALID_ARG),
                                 ([[]], [[]], N.PF_ERR_INVALID_ARG), ([[[1]]] * 1025, [[1.0]] * 1025, N.PF_ERR_CAPACITY)):
        for op in (False, True):
            with pytest.raises(N.PfError) as ei:
                eng.consensus(lists, weights, op=op)
            assert ei.value.code == code
    assert eng.profile_get("consensus")[1] == 0
    eng.consensus([[[1, 2], [1]]], [[0.5, 0.5]])
    assert eng.profile_get("consensus")[1] == 2
    eng.profile(False)


def _census(rec, audio, classes):
    """one GetResults on the recogniser's engine with the profile on: (streams, results, launches per class)"""
    from test_gpu_nnlm import _get
    lib, h = rec._lib, C.c_void_p(rec._lib.pf_recognizer_engine(rec._h))
    N.check(lib.pf_profile_enable(h, 1))
    N.check(lib.pf_profile_reset(h))
    streams, res = _get(rec, audio)
    counts = []
    for c in classes:
        ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
        N.check(lib.pf_profile_get(h, c.encode(), ms, n, fpl))
        counts.append(n.value)
    N.check(lib.pf_profile_enable(h, 0))
    return streams, res, counts


@pytest.mark.parametrize("kind,setup", [("paraformer", "nbest"), ("sensevoice", "beam")])
def test_recognizer_reports_the_consensus_of_its_alternatives(tmp_path, sv_embed, kind, setup):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    from test_gpu_nnlm import CLASSES, _model_dir
    classes = ("consensus",) + CLASSES
    paths, _, _ = _model_dir(tmp_path, kind, sv_embed)
    audio = [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]
    rec = OfflineRecognizer(*paths)
    if setup == "beam":
        rec.SetCtcBeam(4, 8, 4)
    else:
        rec.SetNBest(6, 4)
    s0, res0, census0 = _census(rec, audio, classes)
    assert census0[0] == 0 and sum(len(s.Alternatives) for s in s0) >= 4
    assert all(s.ConsensusIndex == -1 and s.ConsensusConfidence == [] for s in s0)
    assert all(a.Posterior is None and a.Risk is None for s in s0 for a in s.Alternatives)
    scale = 0.7
    rec.SetConsensus(True, scale)
    s1, res1, census1 = _census(rec, audio, classes)                           # one call over the lists of all streams
    assert census1 == [2] + census0[1:]
    for a, b, ra, rb in zip(s0, s1, res0, res1):
        assert (a.Tokens, a.Timestamps, a.Scores) == (b.Tokens, b.Timestamps, b.Scores)
        assert (ra.Text, ra.Tokens, ra.Timestamps) == (rb.Text, rb.Tokens, rb.Timestamps)
        old, new = a.Alternatives, b.Alternatives
        assert [(x.Ids, x.Score, x.Text, x.Tokens) for x in new] == [(x.Ids, x.Score, x.Text, x.Tokens) for x in old]
        if not old:
            assert b.ConsensusIndex == -1 and b.ConsensusConfidence == []
            continue
        post = R.posterior([x.Score for x in old], scale)
        w, risk, conf, _ = R.consensus([x.Ids for x in old], post)
        assert b.ConsensusIndex == w and bits(b.ConsensusConfidence) == bits(conf)
        assert bits([x.Posterior for x in new]) == bits(post) and bits([x.Risk for x in new]) == bits(risk)
    rec.SetConsensus(False)                                                    # off: the parent's launches, nothing reported
    s2, _, census2 = _census(rec, audio, classes)
    assert census2 == census0
    assert [s.Alternatives for s in s2] == [s.Alternatives for s in s0] and all(s.ConsensusIndex == -1 for s in s2)
    rec.Dispose()
