"""CPU: pf_host_consensus (the host twin of csrc/k_consensus.hip) against the definition in plain Python (tests/consensus_ref.py),
exactly: winner and D as integers, risk and conf bit for bit; the refusals; the exported names; SetConsensus's argument checks."""
import pytest

import consensus_cases as K
import consensus_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E


bits, same = K.bits, K.same


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_host_twin_equals_the_definition(name):
    hyps, p = K.CASES[name]
    got = E.host_consensus(hyps, p=p)
    assert same(got, K.want(name)) and bits(got.post) == bits(p)
    if name in K.HAND_MASKS:                                                   # the preference itself, not only the agreement
        assert got.winner == 0 and got.conf.tolist() == [0.75 + 0.25 * m for m in K.HAND_MASKS[name]]
    if name in K.WINNER_LEN:                                                   # the long hypothesis is the one on the rows
        assert len(got.conf) == K.WINNER_LEN[name] and len(set(got.conf.tolist())) > 8    # and the others' masks show in conf
    if name == "tie":
        assert got.winner == 0 and got.risk[0] == got.risk[1] < got.risk[2]


@pytest.mark.parametrize("scale", [1.0, 0.3, 7.0])
def test_posterior_from_scores(scale):
    hyps = K.CASES["five"][0]
    scores = [-3.25, -3.5, -40.0, -3.25, -900.0]
    got = E.host_consensus(hyps, scores=scores, scale=scale)
    post = R.posterior(scores, scale)
    assert bits(got.post) == bits(post) and same(got, R.consensus(hyps, post))


@pytest.mark.parametrize("hyps,kw", [
    ([], dict(p=[])),                                                          # N = 0
    ([[1]] * 65, dict(p=[1.0] * 65)),                                          # N = 65
    ([[1] * 256], dict(p=[1.0])),                                              # 256 ids
    ([[1], [2]], dict(p=[1.0, -0.5])),
    ([[1], [2]], dict(p=[1.0, float("inf")])),
    ([[1], [2]], dict(p=[float("nan"), 1.0])),
    ([[1], [2]], dict(scores=[0.0, float("nan")])),
    ([[1], [2]], dict(scores=[0.0, -1.0], scale=0.0)),
    ([[1], [2]], dict(scores=[0.0, -1.0], scale=float("inf"))),
    ([[1], [2]], dict()),                                                      # neither weights nor scores
])
def test_refusals(hyps, kw):
    with pytest.raises(N.PfError) as ei:
        E.host_consensus(hyps, **kw)
    assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_names_and_argument_checks():
    lib = N.load()
    for name in ("pf_host_consensus", "pf_engine_consensus", "pf_op_consensus", "pf_recognizer_set_consensus", "pf_stream_consensus",
                 "pf_stream_alternative_consensus"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    rec = OfflineRecognizer.__new__(OfflineRecognizer)                         # the checks come before the handle is touched
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rec.SetConsensus(True, scale)
    with pytest.raises(TypeError):
        rec.SetConsensus("yes")
