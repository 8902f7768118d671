"""GPU: streaming punctuation on the device (csrc/k_punc_stream.hip) through pf_op_punc_stream_step: ONE launch
per call over all streams.  A word's logits, its mark and the state bytes do not depend on how the stream was cut into calls
and tiles or on who shares the launch (asserted on bits); the logits lie within the allowance of the float64 definition
(tests/punc_stream_ref.py; the allowance is 4 x the f16 emulation's deviation, test_punc_stream_cpu.py holds the cap on the share of
positions whose margin does not clear it); the loop's marks, flags and flush marks are the rule over the device's own logits and,
on models whose marks are decided by wide margins, the host twin's."""
import os

import numpy as np
import pytest

import punc_ref as R
import punc_stream_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd import engine as E

pytestmark = pytest.mark.gpu
LAYERS = [1, 2, 4]
NR = S.NO_RESTARTS
NONE, PERIOD = 1, 3
MARKER, STAND_IN = 7, 8
CLASSES = ("punc_stream", "punc", "layernorm", "gemm_op", "fsmn", "cif_misc", "argmax", "attn_self", "vad", "vadnet", "vadnet_stream", "fbank",
           "attn_op", "topk", "lfr_cmvn_pad", "gemm_qkv", "gemm_outffn", "gemm_out", "gemm_ffn2", "gemm_dec_ffn", "dec_mid", "attn_cross",
           "gemm_op_mid", "quantize", "lstm", "ts_misc", "pcm_to_samples", "endpoint", "cif_stream", "spk")


@pytest.fixture(scope="module")
def eng():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.set_punc_model(None)
    e.close()


def _causal(n_layers, kernel=11, seed=42):
    cfg = W.ct_transformer_config(vocab=64, n_layers=n_layers, kernel=kernel)
    return S.causal_config(cfg), W.synth_punc_weights(cfg, seed=seed)


@pytest.fixture(scope="module")
def models():
    """per layer count: config, weights, the loaded model, the emulation's deviation and the float64 logits of the 256-word context"""
    out = {}
    for nl in LAYERS:
        cfg, w = _causal(nl)
        dev, _ = S.deviation_and_margin(w, cfg)
        ids = R.window_ids(256, 64, 256)
        out[nl] = (cfg, w, E.load_punc_model(W.pack_pfw(cfg, w)), dev, ids, S.logits64(w, cfg, ids))
    yield out
    for v in out.values():
        v[2].close()


def _marker_model(n_layers):
    """every word is marked "_" by a decoder bias of 5, except word MARKER, whose embedding 4 * (+1, -1, ...) dominates the
    residual stream and meets a "。" row of the decoder along that direction: its logit is 10 (float64: 9.99 .. 10.0 against at
    most 1.6 for any other word, csrc-independent: measured with the host twin at 1, 2 and 4 layers)."""
    cfg, w = _causal(n_layers)
    w = dict(w)
    u = np.where(np.arange(256) % 2 == 0, 1.0, -1.0).astype(np.float32)
    emb = w["embed.weight"].copy()
    emb[MARKER] = 4.0 * u
    w["embed.weight"] = emb
    w["after_norm.weight"], w["after_norm.bias"] = np.ones(256, np.float32), np.zeros(256, np.float32)
    dw = np.zeros((6, 256), np.float32)
    dw[PERIOD] = u * np.float32(10.0 / 256)
    db = np.zeros(6, np.float32)
    db[NONE] = 5.0
    w["decoder.weight"], w["decoder.bias"] = dw, db
    return cfg, w


def _plain_ids(n, seed):
    ids = R.window_ids(n, 64, seed)
    ids[ids == MARKER] = STAND_IN
    return ids


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(eng, m, ids, calls, flush=False, max_context=S.DEFAULT_CONTEXT, flags=0, state=None):
    """one stream through the device in calls of the given sizes (the flush with the last): marks, flags, logits, flush_mark, state"""
    st = E.punc_stream_state(m, B=1) if state is None else state
    mk, mf, zs, at, fm = [], [], [], 0, -1
    for k, n in enumerate(calls):
        res, z, f = eng.op_punc_stream_step(st, [ids[at: at + n]], flush=[flush and k == len(calls) - 1], max_context=max_context, flags=flags)
        mk.append(res[0][0]); mf.append(res[0][1]); zs.append(z[0]); fm = int(f[0])
        at += n
    assert at == len(ids)
    return np.concatenate(mk), np.concatenate(mf), np.concatenate(zs), fm, st


def _cycle(total, sizes):
    out, at, k = [], 0, 0
    while at < total:
        n = min(sizes[k % len(sizes)], total - at)
        out.append(n); at += n; k += 1
    return out


# ---- no restarts: the pure network --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", LAYERS)
def test_every_cut_of_a_256_word_context_gives_the_same_bits(eng, models, nl):
    cfg, w, m, dev, ids, z64 = models[nl]
    eng.set_punc_model(m)
    mk, mf, z, fm, st = _run(eng, m, ids, [256], flags=NR)
    assert not mf.any() and fm == -1 and st[0, -16:].view(np.int32).tolist() == [256, int(mk[-1]), 0, 0]
    for calls in ([1] * 256, _cycle(256, [1, 2, 31, 32, 33, 63, 64, 65]), _cycle(256, [65, 64, 63, 33])):
        g = _run(eng, m, ids, calls, flags=NR)
        assert _same(g[2], z) and g[0].tolist() == mk.tolist() and not g[1].any(), calls[:8]
        assert np.array_equal(g[4], st), calls[:8]
    # against the float64 definition: the allowance is 4 x the emulation's deviation; marks where the margin clears twice that
    allow = 4 * dev
    err = float(np.abs(z.astype(np.float64) - z64).max())
    print("layers %d: device deviation %.3g, allowance %.3g" % (nl, err, allow))
    assert err <= allow
    s = np.sort(z64, axis=1)
    clear = (s[:, -1] - s[:, -2]) > 2 * allow
    assert clear.mean() >= 0.95 and mk[clear].tolist() == R.argmax_ties_larger(z64)[clear].tolist()


@pytest.mark.parametrize("kernel,lens", [(11, [9, 10, 11, 12]), (3, [1, 2, 3, 4, 70])])
def test_fsmn_edges(eng, kernel, lens):
    cfg, w = _causal(1, kernel=kernel)
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    eng.set_punc_model(m)
    dev, _ = S.deviation_and_margin(w, cfg, lengths=[12, 64])
    for T in lens:
        ids = R.window_ids(T, 64, T)
        z = _run(eng, m, ids, [T], flags=NR)[2]
        assert np.abs(z.astype(np.float64) - S.logits64(w, cfg, ids)).max() <= 4 * dev, T
        assert _same(_run(eng, m, ids, [1] * T, flags=NR)[2], z), T
    eng.set_punc_model(None)
    m.close()


# ---- the loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", LAYERS)
def test_loop_is_the_rule_over_the_devices_own_logits(eng, models, nl):
    cfg, w, m, dev, ids, _ = models[nl]
    eng.set_punc_model(m)
    for mc, calls in ((200, [131, 70, 55]), (9, [131, 70, 55]), (2, [70]), (200, _cycle(256, [1, 5, 64, 65]))):
        n = sum(calls)
        mk, mf, z, fm, st = _run(eng, m, ids[:n], calls, flush=True, max_context=mc)
        p, f, count = S.loop_from_logits(z, cfg["punc_list"], cfg["sentence_end_id"], mc)
        assert mk.tolist() == p.tolist() and mf.tolist() == f.tolist()
        want_fm = -1 if count == 0 else (cfg["sentence_end_id"] if p[-1] in (1, 2, 5) else int(p[-1]))
        assert fm == want_fm and not st[0, -16:].any()
        assert (mf == 1).sum() >= 5                                  # (with random weights a quarter of the words end a sentence)
        # a word's logits are those of its context alone: every sentence again as a stream of its own, without restarts
        starts = [0] + [i + 1 for i in np.nonzero(mf)[0].tolist()]
        for a, b in list(zip(starts, starts[1:] + [n]))[:6]:
            if b > a:
                assert _same(_run(eng, m, ids[a:b], [b - a], flags=NR)[2], z[a:b]), (a, b)
        # and every other cut into calls gives the same stream
        g = _run(eng, m, ids[:n], _cycle(n, [33, 1, 64]), flush=True, max_context=mc)
        assert g[0].tolist() == mk.tolist() and g[1].tolist() == mf.tolist() and g[3] == fm and _same(g[2], z)


@pytest.mark.parametrize("nl", LAYERS)
def test_restarts_at_every_tile_position_equal_the_host_twin(eng, nl):
    cfg, w = _marker_model(nl)
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    eng.set_punc_model(m)
    cases = [  # (marker positions, calls, max_context)
        ([0], [131], 200),                       # a sentence end at row 0 of the first tile
        ([63], [131], 200), ([64], [131], 200),  # at the last row of a tile, at row 0 of the second
        ([130], [131], 200),                     # at the last row of the call
        ([0, 1, 2, 5, 40, 41, 63, 64, 65, 130], [131], 200),         # several in one tile, two in a row
        ([3, 70], [5, 0, 70, 1, 55], 200),
        ([], [131], 64), ([], [131], 65), ([], [131], 63), ([], [70], 2), ([], [256], 256), ([], [255], 256),   # forced restarts
        ([10, 80], [131], 64),                   # both rules in one call
    ]
    for marks_at, calls, mc in cases:
        n = sum(calls)
        ids = _plain_ids(n, 17 + n)
        ids[marks_at] = MARKER
        hs = E.punc_stream_state(m, host=True)                        # the host twin: the words, then the flush in a call of its own
        hk, hf, hz, _ = E.host_punc_stream_step(m, hs, ids, max_context=mc)
        words = hs[-16:].view(np.int32).tolist()
        hfm = E.host_punc_stream_step(m, hs, [], flush=True, max_context=mc)[3]
        mk, mf, z, fm, st = _run(eng, m, ids, calls, flush=True, max_context=mc)
        assert mk.tolist() == hk.tolist() and mf.tolist() == hf.tolist() and fm == hfm, (marks_at, calls, mc)
        assert [i for i in range(n) if mf[i] == 1] == marks_at and not st[0, -16:].any()
        # (a plain sanity bound, not the project's allowance: this model's marks are decided by a margin of 5, and the allowance
        #  of 4 x the emulation's deviation is asserted on the random models above)
        assert np.abs(z.astype(np.float64) - hz).max() <= 0.05
        # without the flush the count and the newest mark stay in the state; the flush may come in a call of its own
        g = _run(eng, m, ids, calls, max_context=mc)
        assert g[4][0, -16:].view(np.int32).tolist() == words and g[3] == -1 and _same(g[2], z)
        assert _run(eng, m, ids[:0], [0], flush=True, max_context=mc, state=g[4])[3] == hfm
        assert not g[4][0, -16:].any()
    eng.set_punc_model(None)
    m.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", LAYERS)
@pytest.mark.parametrize("flags,mc", [(NR, 200), (0, 200), (0, 7)])
def test_a_stream_does_not_depend_on_its_launch_mates(eng, models, nl, flags, mc):
    cfg, w, m, dev, ids, _ = models[nl]
    eng.set_punc_model(m)
    n_new = [5, 0, 70, 1, 131]
    before = [3, 0, 10, 200, 60]                                      # what each stream's context holds already (no restarts: 60 + 131 <= 256)
    words = [R.window_ids(before[b] + n_new[b], 64, 50 + b) for b in range(5)]
    flush = [False, True, True, False, True]

    def seeded(b):
        st = E.punc_stream_state(m, B=1)
        eng.op_punc_stream_step(st, [words[b][: before[b]]], max_context=mc, flags=flags)
        return st
    alone = []
    for b in range(5):
        st = seeded(b)
        res, z, fm = eng.op_punc_stream_step(st, [words[b][before[b]:]], flush=[flush[b]], max_context=mc, flags=flags)
        alone.append((res[0][0], res[0][1], z[0], int(fm[0]), st[0]))
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 4, 0, 3, 1]):
        states = np.concatenate([seeded(b) for b in order])
        raw = {}
        res, z, fm = eng.op_punc_stream_step(states, [words[b][before[b]:] for b in order], flush=[flush[b] for b in order],
                                             max_context=mc, flags=flags, ld=140, out=raw)
        for k, b in enumerate(order):
            a = alone[b]
            assert res[k][0].tolist() == a[0].tolist() and res[k][1].tolist() == a[1].tolist() and int(fm[k]) == a[3], (order, b)
            assert _same(z[k], a[2]) and np.array_equal(states[k], a[4]), (order, b)
            # the guard words round every output: nothing at or beyond a stream's n_new is written
            assert (raw["marks"][k, n_new[b]:] == -77777).all() and (raw["mark_flags"][k, n_new[b]:] == -77777).all()
            assert (raw["logits"][k, n_new[b]:] == np.float32(-7e7)).all()


# ---- errors and the census ------------------------------------------------------------------------------------------------------
def _census(eng):
    return [eng.profile_get(c)[1] for c in CLASSES]


def test_argument_errors_launch_nothing_and_each_entry_refuses_the_wrong_model(eng, models):
    cfg, w, m, dev, ids, _ = models[1]
    cfg0 = W.ct_transformer_config(vocab=64, n_layers=1)
    m0 = E.load_punc_model(W.pack_pfw(cfg0, w))
    st = E.punc_stream_state(m, B=2)
    eng.set_punc_model(m)
    eng.op_punc_stream_step(st, [ids[:9], ids[:4]], flags=NR)
    before = st.copy()
    eng.profile(True)
    eng.profile_reset()
    bad_count = st.copy()
    bad_count[1, -16:].view(np.int32)[0] = 257
    for kw, lists, code, states in (
            (dict(max_context=1), [[1], [1]], N.PF_ERR_INVALID_ARG, st), (dict(max_context=257), [[1], [1]], N.PF_ERR_INVALID_ARG, st),
            (dict(flags=2), [[1], [1]], N.PF_ERR_INVALID_ARG, st), (dict(), [[1], [64]], N.PF_ERR_INVALID_ARG, st),
            (dict(), [[1, 2, -1], []], N.PF_ERR_INVALID_ARG, st), (dict(flags=NR), [[1], np.zeros(253, np.int32)], N.PF_ERR_INVALID_ARG, st),
            (dict(max_context=4), [[1], [1]], N.PF_ERR_INVALID_ARG, st), (dict(flags=NR), [[1], [1]], N.PF_ERR_INVALID_ARG, bad_count)):
        keep = states.copy()
        with pytest.raises(N.PfError) as ei:
            eng.op_punc_stream_step(states, lists, **kw)
        assert ei.value.code == code, kw
        assert np.array_equal(states, keep)
    # a causal model at the offline entries, a model that is not causal at the streaming entry, no model at all
    for fn in (lambda: eng.op_punc_logits([ids[:5]]), lambda: eng.op_punc_window([ids[:5]], [True]), lambda: eng.punctuate([ids[:5]])):
        with pytest.raises(N.PfError) as ei:
            fn()
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_punc_model(m0)
    with pytest.raises(N.PfError) as ei:
        eng.op_punc_stream_step(st, [[1], [1]])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_punc_model(None)
    with pytest.raises(N.PfError) as ei:
        eng.op_punc_stream_step(st, [[1], [1]])
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    assert not any(_census(eng)) and np.array_equal(st, before)
    eng.profile(False)
    m0.close()


def test_one_launch_per_call(eng, models):
    cfg, w, m, dev, ids, _ = models[2]
    eng.set_punc_model(m)
    st = E.punc_stream_state(m, B=3)
    eng.profile(True)
    eng.profile_reset()
    eng.op_punc_stream_step(st, [ids[:131], ids[:1], ids[:70]], flush=[True, False, True], max_context=9)
    c1 = _census(eng)
    eng.op_punc_stream_step(st, [[], ids[:200], []], flags=NR)
    c2 = _census(eng)
    eng.op_punc_stream_step(st[:0], [])
    c3 = _census(eng)
    eng.profile(False)
    assert c1[0] == 1 and not any(c1[1:]) and c2[0] == 2 and not any(c2[1:]) and c3 == c2


def test_a_real_model():
    """Opt-in: PF_REAL_PUNC_STREAM_MODEL names a `.pfw` converted from FunASR's realtime CT-Transformer (convert --kind cttransformer
    --causal).  The one route by which what is remembered of that model (its dimensions, a causal last layer) can be checked: the
    container must load as causal and the device must agree with the host twin on a stream of its own vocabulary."""
    path = os.environ.get("PF_REAL_PUNC_STREAM_MODEL")
    if not path:
        pytest.skip("PF_REAL_PUNC_STREAM_MODEL is not set")
    m = E.load_punc_model(path)
    assert m.causal
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    e.set_punc_model(m)
    ids = R.window_ids(64, m.dims["vocab"], 1)
    st = E.punc_stream_state(m, B=1)
    res, z, fm = e.op_punc_stream_step(st, [ids], flags=NR)
    hz = E.host_punc_stream_step(m, E.punc_stream_state(m, host=True), ids, flags=NR)[2]
    assert np.abs(z[0].astype(np.float64) - hz).max() <= 0.05
    e.set_punc_model(None)
    e.close()
    m.close()
