"""GPU: cif_stream_kernel (csrc/k_cif_stream.hip) through pf_op_online_cif_step against pf_host_online_cif_step, which
tests/test_cif_stream_cpu.py holds to the numpy restatement.  No tolerance anywhere: fired rows, fire entries, counts and every
byte of the state blocks are equal.

  * the CPU case table (cif_stream_ref.step_cases: exact-threshold sums, no fire, integrate == 0, a firing carry, a reset, a
    second tile of rows, a chunk shorter than the mask window, a channel group that is not full) with every case alone (B = 1) and
    three cases of one shape as the streams of one launch (B = 3), chained over their six calls
  * three streams with different reset patterns
  * a stream's outputs and state do not change when its neighbours' inputs and states are replaced
"""
import numpy as np
import pytest

import cif_stream_ref as CR
import online_lockstep_ref as LR
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = CR.step_cases()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=5)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host():
    """the host statement's answer to every case, computed once"""
    return {c.name: CR.run_case(c, CR.host_step) for c in CASES}


def _run_batch(engine, cases, host):
    B, D = len(cases), cases[0].D
    states = np.stack([CR.new_state(D) if c.state0 is None else c.state0.copy() for c in cases])
    fires = 0
    for k in range(CR.CHAIN):
        h = np.stack([c.calls[k][0] for c in cases])
        a = np.stack([c.calls[k][1] for c in cases])
        rs = [int(c.calls[k][2]) for c in cases]
        thr = cases[0].threshold
        fired, entry, n = CR.op_step(engine, states, h, a, thr, rs)
        for b, c in enumerate(cases):
            wf, we, wn, ws = host[c.name][k]
            assert n[b] == wn, (c.name, k)
            assert (entry[b] == we).all(), (c.name, k)
            assert (_bits(fired[b]) == _bits(wf)).all(), (c.name, k)
            assert (_bits(states[b]) == _bits(ws)).all(), (c.name, k)
            fires += wn
    return fires


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_stream(engine, host, case):
    _run_batch(engine, [case], host)


def _triples():
    by = {}
    for c in CASES:
        by.setdefault((c.D, c.Tc, c.threshold), []).append(c)
    out = []
    for group in by.values():
        for i in range(0, len(group) - 2, 3):
            out.append(group[i: i + 3])
        if len(group) >= 3 and len(group) % 3:
            out.append(group[-3:])
    return out


TRIPLES = _triples()


@pytest.mark.parametrize("cases", TRIPLES, ids=["+".join(c.name for c in t) for t in TRIPLES])
def test_three_streams_in_one_launch(engine, host, cases):
    assert _run_batch(engine, cases, host) > 0


def test_the_triples_cover_the_table():
    named = {c.name for t in TRIPLES for c in t}
    assert named >= {c.name for c in CASES if c.threshold == 1.0}


def test_reset_patterns_per_stream(engine):
    D, Tc = 512, 20
    r = np.random.default_rng(77)
    patterns = ((0, 0, 0, 1, 0, 0), (1, 0, 1, 0, 0, 1), (0, 0, 0, 0, 0, 0))
    dev = np.stack([CR.new_state(D) for _ in patterns])
    dev[1, :D] = 3.0                                                  # a used slot: its first step resets it
    dev[1, D: D + 2] = 0.5
    hst = dev.copy()
    resets = 0
    for k in range(6):
        h = r.standard_normal((3, Tc, D)).astype(F32)
        a = r.random((3, Tc)).astype(F32)
        rs = [p[k] for p in patterns]
        fired, entry, n = CR.op_step(engine, dev, h, a, 1.0, rs)
        for b in range(3):
            wf, we, wn = CR.host_step(hst[b], h[b], a[b], 1.0, reset=bool(rs[b]))
            assert n[b] == wn and (entry[b] == we).all() and (_bits(fired[b]) == _bits(wf)).all(), (k, b)
            resets += rs[b]
        assert (_bits(dev) == _bits(hst)).all(), k
    assert resets == 4


def test_a_stream_does_not_see_its_neighbours(engine):
    D, Tc = 512, 20
    r = np.random.default_rng(78)
    st = r.standard_normal((3, CR.state_words(D))).astype(F32)
    st[:, D:] = 0
    st[:, D: D + 2] = np.asarray([0.25, 0.5, 0.75], F32)[:, None]
    h = r.standard_normal((3, Tc, D)).astype(F32)
    a = r.random((3, Tc)).astype(F32)
    s1 = st.copy()
    f1, e1, n1 = CR.op_step(engine, s1, h, a, 1.0, [0, 0, 0])
    st2, h2, a2 = st.copy(), h.copy(), a.copy()
    for j in (0, 2):
        st2[j, :D] = r.standard_normal(D).astype(F32) * 40
        st2[j, D: D + 2] = 0.99
        h2[j] = r.standard_normal((Tc, D)).astype(F32) * 40
        a2[j] = 1.0
    f2, e2, n2 = CR.op_step(engine, st2, h2, a2, 1.0, [1, 0, 0])
    assert n2[1] == n1[1] and (e2[1] == e1[1]).all() and (_bits(f2[1]) == _bits(f1[1])).all() and (_bits(st2[1]) == _bits(s1[1])).all()
    assert n1[1] >= 3 and (n2[2] != n1[2] or (_bits(f2[2]) != _bits(f1[2])).any())


def test_argument_errors(engine):
    from aliparaformerasr_amd import _native as N
    D, Tc = 8, 20
    st = np.zeros((1, CR.state_words(D)), F32)
    h, a = np.zeros((1, Tc, D), F32), np.zeros((1, Tc), F32)
    with pytest.raises(N.PfError) as ei:
        CR.op_step(engine, st, h, a, 1.0, [0], cap=Tc)
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    f, e, n = CR.op_step(engine, st, h, a, 1.0, [0], cap=Tc + 1)
    assert n[0] == 0 and (e == -1).all() and not f.any()
