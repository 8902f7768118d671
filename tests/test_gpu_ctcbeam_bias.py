"""GPU: hot-word boosting inside the CTC prefix beam search on the device (the kBias form of csrc/k_ctcbeam.hip,
Engine.set_ctc_hotwords, OfflineRecognizer.SetHotwordBoost) — the kernel against the definition (tests/ctcbeam_bias_ref.py)
over the committed inputs with canaries and poisoned unread rows, a set at the state limit, no bias = no change, the engine
in all four math modes against the definition fed the engine's own lists, and the recognizer surface: hot words from the file
and from stream.Hotwords, the union over a batch, two caller threads, SetAlign beside it, the CLI, refusals.

Comparison rule: token lists, their order and matched identical; scores within (16 T + 4) * 2^-53 * max(1, |s|)."""
import io
import threading
import wave

import numpy as np
import pytest

import ctcbeam_bias_ref as BR
import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import glue

pytestmark = pytest.mark.gpu
SCORES, CTC, TOPK, BEAM, ALIGN = N.PF_DECODE_SCORES, N.PF_DECODE_CTC, N.PF_DECODE_TOPK, N.PF_DECODE_CTC_BEAM, N.PF_DECODE_ALIGN
SV_VOCAB = 403
BOOST = BR.RECIPE_BOOST


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hyps(res, b):
    return [(tuple(res.ids[b, i, : int(res.len[b, i])].tolist()), float(res.score[b, i]), int(res.matched[b, i]),
             float(res.loglik_sum[b, i])) for i in range(int(res.n_hyp[b]))]


def _same(got, want, T):
    assert [h[0] for h in got] == [h[0] for h in want]
    assert [h[2] for h in got] == [h[2] for h in want]
    for g, w in zip(got, want):
        print("    score %.17g  definition %.17g  |diff| %.3g  tol %.3g  matched %d" % (g[1], w[1], abs(g[1] - w[1]), BR.tol(T, w[1]), g[2]))
        assert abs(g[1] - w[1]) <= BR.tol(T, w[1]), (g, w, abs(g[1] - w[1]), BR.tol(T, w[1]))
        assert abs(g[3] - w[3]) <= BR.tol(T, w[3]), (g, w)


def _canaries(B, n_best, cap):
    return (np.full((B, n_best, cap), 0x5A5A5A5A5A5A5A5A, np.int64), np.full((B, n_best), -77, np.int32),
            np.full((B, n_best), 12345.0, np.float64), np.full(B, -77, np.int32), np.full((B, n_best), -77, np.int32),
            np.full((B, n_best), 12345.0, np.float64))


def _check_fill(r, b, n_best, T):
    for i in range(n_best):                                                       # fill values, no canary left
        k = int(r.len[b, i])
        assert 0 <= k <= T and (r.ids[b, i, k:] == -1).all() and (r.ids[b, i, :k] >= 1).all()
        if i >= r.n_hyp[b]:
            assert k == 0 and r.score[b, i] == -np.inf and r.matched[b, i] == 0 and r.loglik_sum[b, i] == -np.inf


def _batch_of_three(lb, ids, val, n, T):
    """B = 3 with lengths (T, 1, 0) over one input; whatever lies at or beyond an utterance's length is poison"""
    rep = lambda a: np.ascontiguousarray(np.stack([a, a, a]))  # noqa: E731
    lb3, ids3, val3, n3 = rep(lb), rep(ids), rep(val), rep(n)
    for b, ln in ((1, 1), (2, 0)):
        lb3[b, ln:] = np.nan
        ids3[b, ln:] = 1
        val3[b, ln:] = np.inf
        n3[b, ln:] = 0
    return lb3, ids3, val3, n3, np.array([T, 1, 0], np.int32)


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


# ---- 1: the kernel against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_kernel_equals_definition(any_engine, case):
    """The recipe's hot words at s = 2; N = W and N = 1; every output slot is overwritten (canary)."""
    lb, ids, val, n = R.case_arrays(case)
    T, Wd = case[2], case[5]
    hot = BR.case_hotwords(case)
    args = _batch_of_three(lb, ids, val, n, T)
    refs = [BR.case_reference(case).beam, BR.case_reference(case, T=1).beam, [((), 0.0, 0, 0.0)]]
    for n_best in sorted({Wd, 1}):
        r = any_engine.op_ctc_beam_hot(*args, Wd, hot, BOOST, n_best, out=_canaries(3, n_best, T))
        for b in range(3):
            want = refs[b][:n_best]
            print("  %s N=%d utterance %d: %d hypotheses" % (case[0], n_best, b, len(want)))
            assert r.n_hyp[b] == len(want)
            _same(_hyps(r, b), want, max(int(args[4][b]), 1))
            _check_fill(r, b, n_best, T)
            for h in _hyps(r, b):
                assert h[1] == h[3] + BOOST * h[2]                                # one product, one addition


def _set_at_the_state_limit(V):
    """64-id hot words over the ids 1 .. V-1 whose trie has exactly PF_HOTWORD_STATES_MAX nodes"""
    rng = np.random.default_rng(5)
    many, seen = [], set()
    while True:
        w = tuple(int(c) for c in rng.integers(1, V, 64))
        pre = {w[:k] for k in range(1, 65)}
        if 1 + len(seen | pre) > N.PF_HOTWORD_STATES_MAX:
            break
        many.append(w)
        seen |= pre
    p = 64 - (N.PF_HOTWORD_STATES_MAX - 1 - len(seen))                            # the last word leaves an earlier one after p ids
    free = [c for c in range(1, V) if many[0][:p] + (c,) not in seen]
    many.append(many[0][:p] + (free[0],) * (64 - p))
    return many


@pytest.mark.parametrize("name", ["t12", "lowblank"])
def test_kernel_with_a_set_at_the_state_limit(any_engine, name):
    from aliparaformerasr_amd.engine import HotwordGraph
    case = [c for c in R.GPU_CASES if c[0] == name][0]
    lb, ids, val, n = R.case_arrays(case)
    T, V, Wd = case[2], case[3], case[5]
    hot = _set_at_the_state_limit(V)
    g = HotwordGraph(hot, V)
    assert g.S == N.PF_HOTWORD_STATES_MAX and all(len(w) == 64 for w in hot)
    ref = BR.case_reference(case, BOOST, hot)
    assert [h[0] for h in ref.beam] != [h[0] for h in R.case_reference(case).beam]     # pending matches steer the search
    args = _batch_of_three(lb, ids, val, n, T)
    r = any_engine.op_ctc_beam_hot(*args, Wd, hot, BOOST, out=_canaries(3, Wd, T))
    _same(_hyps(r, 0), ref.beam, T)
    _same(_hyps(r, 1), BR.case_reference(case, BOOST, hot, 1).beam, 1)
    for b in range(3):
        _check_fill(r, b, Wd, T)


# ---- 2: no bias means no change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t65", "full_lds", "ragged", "mirror_w64", "w1"])
def test_no_bias_is_the_unbiased_kernel_bit_for_bit(any_engine, name):
    case = [c for c in R.GPU_CASES if c[0] == name][0]
    lb, ids, val, n = R.case_arrays(case)
    T, Wd = case[2], case[5]
    args = _batch_of_three(lb, ids, val, n, T)
    plain = any_engine.op_ctc_beam(*args, Wd)
    for hot, boost in ((BR.case_hotwords(case), 0.0), ([], BOOST), ([(), ()], BOOST)):
        r = any_engine.op_ctc_beam_hot(*args, Wd, hot, boost, out=_canaries(3, Wd, T))
        assert (r.n_hyp == plain.n_hyp).all() and (r.ids == plain.ids).all() and (r.len == plain.len).all()
        assert (r.score.view(np.uint64) == plain.score.view(np.uint64)).all()
        assert (r.matched == 0).all() and (r.loglik_sum.view(np.uint64) == plain.score.view(np.uint64)).all()


def test_kernel_refusals(any_engine):
    lb, ids, val, n = R.case_arrays(R.GPU_CASES[-1])
    args = (lb[None], ids[None], val[None], n[None], np.array([12], np.int32))
    for hot, boost, code in (([(1, 2)], -1.0, N.PF_ERR_INVALID_ARG), ([(1, 2)], float("nan"), N.PF_ERR_INVALID_ARG),
                             ([(1, 2)], float("inf"), N.PF_ERR_INVALID_ARG), ([(0, 2)], 1.0, N.PF_ERR_INVALID_ARG),
                             ([tuple([1] * 65)], 1.0, N.PF_ERR_CAPACITY)):
        with pytest.raises(N.PfError) as ei:
            any_engine.op_ctc_beam_hot(*args, 3, hot, boost)
        assert ei.value.code == code, (hot, boost)


# ---- 3: the engine, the tiny SenseVoice model of tests/test_gpu_ctcbeam.py, every math mode ---------------------------------
def _sv_model(sv_embed):
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=SV_VOCAB)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)
    b[8:] -= 30
    b[0] += 1.0
    w["ctc.bias"] = b
    return cfg, w


def _audio():
    return [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]


def _hot_from(hyps):
    """hot words out of a list of hypotheses [(ids, ...)]: of number min(n - 1, 3) the ids [0:3] and [4:6], of the last [1:3]"""
    y = hyps[min(len(hyps) - 1, 3)][0]
    hot = [tuple(y[0:3]), tuple(y[4:6]), tuple(hyps[-1][0][1:3])]
    return [w for w in hot if w]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_biased_beam_is_the_definition_of_its_own_lists(sv_embed, mode):
    import ctypes as C
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    Wd, NB = 8, 5
    for e in (e0, e1):
        e.set_decode(BEAM | CTC)
        e.set_ctc_beam(Wd, NB)
    r0 = e0.recognize(audio, want_logits=True)
    hot = _hot_from(r0.beam.hyps(0)) + _hot_from(r0.beam.hyps(2))
    e1.set_ctc_hotwords(hot, BOOST)
    r1 = e1.recognize(audio, want_logits=True)
    assert r0.beam.matched is None and r1.beam.matched is not None and r1.beam.N == NB
    # token ids, scores, the collapse, the lists and the logits are bit-identical with and without the set
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r1.scores), _bits(r0.scores))
    np.testing.assert_array_equal(_bits(r1.logits), _bits(r0.logits))
    np.testing.assert_array_equal(r1.topk.ids, r0.topk.ids)
    np.testing.assert_array_equal(_bits(r1.topk.val), _bits(r0.topk.val))
    np.testing.assert_array_equal(r1.topk.n, r0.topk.n)
    np.testing.assert_array_equal(r1.ctc.n, r0.ctc.n)
    np.testing.assert_array_equal(r1.ctc.ids, r0.ctc.ids)
    np.testing.assert_array_equal(_bits(r1.ctc.score), _bits(r0.ctc.score))
    rows = [4 + e1.frontend(a).shape[0] for a in audio]                          # n_b: the prompt rows and the utterance's frames
    changed = 0
    for b, nb in enumerate(rows):
        ref = BR.beam_search(r1.logits[b, :nb, 0], r1.topk.ids[b, :nb], r1.topk.val[b, :nb], r1.topk.n[b, :nb], Wd, hot, BOOST, NB)
        print("  mode %d utterance %d: n_b=%d, %d hypotheses, decision gap %.3g" % (mode, b, nb, ref.n_hyp, ref.gap))
        assert r1.beam.n_hyp[b] == ref.n_hyp >= 2
        got = _hyps(r1.beam, b)
        _same(got, ref.hyps, nb)
        changed += [h[0] for h in got] != [h[0] for h in r0.beam.hyps(b)]
        lp = r1.logits[b, :nb].astype(np.float64)
        for labels, score, m, ll in got:
            assert score - BOOST * m == ll                                        # bit for bit
            full = R.ctc_loglik(lp, labels)                                       # the search sums a subset of the alignments
            assert ll <= full + BR.tol(nb, full), (labels, ll, full)
    assert changed >= 1 and r1.beam.matched.max() >= 2                            # the set mattered
    # the same set again keeps the table (by content); another boost re-scores
    e1.set_ctc_hotwords(hot, BOOST)
    r2 = e1.recognize(audio)
    assert [_hyps(r2.beam, b) for b in range(3)] == [_hyps(r1.beam, b) for b in range(3)]
    # after clearing the set the unbiased results return, and the extras are refused
    e1.set_ctc_hotwords([], 0.0)
    r3 = e1.recognize(audio)
    assert r3.beam.matched is None
    assert [r3.beam.hyps(b) for b in range(3)] == [r0.beam.hyps(b) for b in range(3)]
    e1.recognize(audio[:1])
    m = np.zeros((1, NB), np.int32)
    assert e1._lib.pf_fetch_ctc_beam_hot(e1._h, m.ctypes.data_as(C.POINTER(C.c_int32)), None) == N.PF_ERR_INVALID_ARG
    e1.set_ctc_hotwords(hot, 0.0)                                                 # boost 0 is "off" too
    assert [e1.recognize(audio).beam.hyps(b) for b in range(3)] == [r0.beam.hyps(b) for b in range(3)]
    e0.close(); e1.close()


def test_engine_align_jobs_are_the_biased_hypotheses(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    audio = _audio()
    eng.set_decode(BEAM | ALIGN)
    eng.set_ctc_beam(8, 4)
    r0 = eng.recognize(audio, want_logits=True)
    eng.set_ctc_hotwords(_hot_from(r0.beam.hyps(0)), BOOST)
    r1 = eng.recognize(audio, want_logits=True)
    assert r1.align.len.shape == (3, 4)
    rows = [4 + eng.frontend(a).shape[0] for a in audio]
    for b in range(3):
        for i, (labels, _score, _m, ll) in enumerate(_hyps(r1.beam, b)):
            assert r1.align.len[b, i] == len(labels)                              # job i is biased hypothesis i
            full = R.ctc_loglik(r1.logits[b, : rows[b]].astype(np.float64), labels)
            assert abs(r1.align.loglik[b, i] - full) <= 1e-9 * max(1.0, abs(full)) and ll <= r1.align.loglik[b, i] + 1e-9
    eng.close()


def test_engine_refusals(sv_embed):
    from aliparaformerasr_amd.engine import Engine, EngineGroup
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pf = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        pf.set_ctc_hotwords([(1, 2)], 1.0)                                        # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    sc = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        sc.set_ctc_hotwords([(1, 2)], 1.0)                                        # SeACo biases through its own decoder
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    sc.close()
    cfg, w = _sv_model(sv_embed)
    blob = W.pack_pfw(cfg, w)
    eng = Engine(weights=blob, cmvn=W.synth_cmvn(), device=0)
    for hot, boost, code in (([(1, 2)], -1.0, N.PF_ERR_INVALID_ARG), ([(1, 2)], float("nan"), N.PF_ERR_INVALID_ARG),
                             ([(1, SV_VOCAB)], 1.0, N.PF_ERR_INVALID_ARG), ([(0,)], 1.0, N.PF_ERR_INVALID_ARG),
                             ([tuple([5] * 65)], 1.0, N.PF_ERR_CAPACITY)):
        with pytest.raises(N.PfError) as ei:
            eng.set_ctc_hotwords(hot, boost)
        assert ei.value.code == code, (hot, boost)
    for bit in (4, 64):                                                           # there is no decode bit for it
        assert eng._lib.pf_engine_set_decode(eng._h, BEAM | bit) == N.PF_ERR_INVALID_ARG
    eng.close()
    # a group forward refuses the beam search as it always did, set or no set
    g = EngineGroup([0, 0], weights=blob, cmvn=W.synth_cmvn())
    h0 = g._lib.pf_group_engine(g._h, 0)
    assert g._lib.pf_engine_set_decode(h0, BEAM) == N.PF_OK
    ids, lens = np.asarray([1, 2], np.int32), np.asarray([2], np.int32)
    import ctypes as C
    i32 = C.POINTER(C.c_int32)
    assert g._lib.pf_engine_set_ctc_hotwords(h0, ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), 1, 1.0) == N.PF_OK
    with pytest.raises(N.PfError) as ei:
        g.recognize(_audio()[:2])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    g.close()


# ---- 4: the recognizer and the API surface -------------------------------------------------------------------------------------
def _sv_dir(tmp_path, sv_embed, hot_lines=None):
    """a SenseVoice model directory whose ids 1 .. are single characters, so that a hot-word file can spell them"""
    cfg, w = _sv_model(sv_embed)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = ["<blank>"] + [chr(0x4E00 + i) for i in range(SV_VOCAB - 1)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    paths = [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]
    if hot_lines is not None:
        (tmp_path / "hotword.txt").write_text("\n".join(hot_lines) + "\n", encoding="utf-8")
        paths += ["", str(tmp_path / "hotword.txt")]
    return paths, toks


def _get(rec, audio, hotwords=None):
    streams = []
    for u, a in enumerate(audio):
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        if hotwords is not None:
            s.Hotwords = hotwords[u]
        streams.append(s)
    return streams, rec.GetResults(streams)


def _alts(streams):
    return [[(tuple(a.Ids), a.Score, a.HotwordTokens, a.LogLikSum, a.Text) for a in s.Alternatives] for s in streams]


def test_recognizer_hotword_boost(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer, RecognizerException
    NB, Wd, K = 4, 8, 4
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    paths, toks = _sv_dir(tmp_path / "a", sv_embed)
    plain = OfflineRecognizer(*paths)
    plain.SetCtcBeam(NB, Wd, K)
    s0, res0 = _get(plain, audio)
    base = _alts(s0)
    assert all(a[2] == 0 and a[3] is None for u in base for a in u)               # unbiased: no extras
    # hot words out of the unbiased lists of both utterances; "x" is no token and is dropped by the file's rule
    w0 = tuple(base[0][min(len(base[0]) - 1, 3)][0][0:3])
    w1 = tuple(base[1][-1][0][1:3]) or tuple(base[1][-1][0][0:1])
    assert w0 and w1
    lines = ["".join(toks[c] for c in w0), "x" + "".join(toks[c] for c in w1)]
    paths_f, _ = _sv_dir(tmp_path / "b", sv_embed, lines)
    boost = 2.0
    from_file, from_streams = OfflineRecognizer(*paths_f), OfflineRecognizer(*paths)
    for r in (from_file, from_streams):
        r.SetHotwordBoost(boost)
    sf, resf = _get(from_file, audio)
    assert _alts(sf) == [[]] * 2 and resf[0].Text == res0[0].Text                 # inert until SetCtcBeam is set
    for r in (from_file, from_streams):
        r.SetCtcBeam(NB, Wd, K)
    sf, resf = _get(from_file, audio)
    # the union over the batch: one word on each stream, the [1] terminator entry wherever it appears
    ss, ress = _get(from_streams, audio, [[list(w0), [1]], [[1], list(w1)]])
    assert _alts(sf) == _alts(ss)
    hot = [w0, w1]
    changed = 0
    for b in range(2):
        # the 1-best fields are what they are without the boost
        assert sf[b].Tokens == s0[b].Tokens and sf[b].Timestamps == s0[b].Timestamps
        assert (resf[b].Text, resf[b].Tokens, resf[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        alts = _alts(sf)[b]
        assert 2 <= len(alts) <= NB
        sc = [a[1] for a in alts]
        assert sc == sorted(sc, reverse=True)
        for ids, score, m, ll, text in alts:
            assert m == BR.walk(ids, hot)[0] and score == ll + boost * m
            assert text == glue.decode_multi_one(toks, list(ids), [[0, 0]] * len(ids))[0]
        changed += [a[0] for a in alts] != [a[0] for a in base[b]]
    assert changed >= 1 and max(a[2] for u in _alts(sf) for a in u) >= 2
    # the file's words when no stream carries any; a null list fails as it does for SeACo
    ss2, _ = _get(from_file, audio, [[], []])
    assert _alts(ss2) == _alts(sf)
    with pytest.raises(RecognizerException):
        _get(from_streams, audio, [None, []])
    # SetAlign beside it: the biased alternatives get their own times and the full log-likelihood
    from_file.SetAlign(True)
    sa, _ = _get(from_file, audio)
    assert [(a[0], a[1], a[2], a[3]) for a in _alts(sa)[0]] == [(a[0], a[1], a[2], a[3]) for a in _alts(sf)[0]]
    for a in sa[0].Alternatives:
        assert a.LogLik is not None and a.LogLikSum <= a.LogLik + 1e-9 and len(a.Timestamps) in (0, len(a.Ids))
    # off again: the unbiased list; refusals
    from_file.SetAlign(False)
    from_file.SetHotwordBoost(0)
    so, _ = _get(from_file, audio)
    assert _alts(so) == base
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(N.PfError) as ei:
            from_file.SetHotwordBoost(bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    for r in (plain, from_file, from_streams):
        r.Dispose()


def test_recognizer_refuses_paraformer_and_seaco(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    for k, (cfg, seed, V) in enumerate(((W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64), 3, 64),
                                        (W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111), 21, 120))):
        d = tmp_path / str(k)
        d.mkdir()
        W.save_pfw(str(d / "model.pfw"), cfg, W.synth_weights(cfg, seed))
        (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
        (d / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
        (d / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(V - 3)]) + "\n", encoding="utf-8")
        rec = OfflineRecognizer(*[str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
        with pytest.raises(N.PfError) as ei:
            rec.SetHotwordBoost(1.0)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
        rec.SetHotwordBoost(0)                                                    # "off" is always fine
        rec.Dispose()


def test_two_threads_on_one_recognizer(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, _ = _sv_dir(tmp_path, sv_embed)
    rec = OfflineRecognizer(*paths)
    rec.SetCtcBeam(5, 8, 4)
    batches = [[W.synth_audio(32000, 5), W.synth_audio(20000, 6)], [W.synth_audio(26000, 91)]]
    plain = [_alts(_get(rec, b)[0]) for b in batches]
    hots = [[[list(plain[0][0][-1][0][0:2])], []], [[list(plain[1][0][-1][0][0:3])]]]     # each caller its own words
    rec.SetHotwordBoost(3.0)

    def snapshot(i):
        streams, res = _get(rec, batches[i], hots[i])
        return [r.Text for r in res], _alts(streams)
    want = [snapshot(i) for i in range(2)]
    assert want[0][1] != plain[0] and want[1][1] != plain[1] and want[0][1][0] != want[1][1][0]
    assert max(a[2] for a in want[0][1][0]) >= 2 and max(a[2] for a in want[1][1][0]) >= 2
    errors = []

    def worker(i):
        try:
            for _ in range(4):
                assert snapshot(i) == want[i]
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    rec.Dispose()


def test_cli_hotboost(tmp_path, sv_embed):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "m"
    d.mkdir()
    _, toks = _sv_dir(d, sv_embed)
    pcm = (np.clip(W.synth_audio(32000, 40), -1, 1) * 32767).astype("<i2")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())

    def run(**kw):
        out = io.StringIO()
        res = ex.offline_recognizer(method="one", model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=3, topk=4, beam=8, **kw)
        return res, [ln for ln in out.getvalue().splitlines() if ln.startswith("nbest[")]
    res0, nb0 = run()
    assert len(nb0) == 3 and all(" hot:" not in ln for ln in nb0)                 # without -hotboost the lines of today
    last = nb0[-1].split("text:")[1]
    assert len(last) >= 2
    (d / "hotword.txt").write_text(last[:2] + "\n", encoding="utf-8")             # the model directory's hot-word file
    res1, nb1 = run(hotboost=4.0)
    assert res1[0].Text == res0[0].Text and len(nb1) == 3
    fields = [(float(ln.split("score:")[1].split(" ")[0]), int(ln.split(" hot:")[1].split(" ")[0]), float(ln.split("loglik_sum:")[1]))
              for ln in nb1]
    assert [f[0] for f in fields] == sorted((f[0] for f in fields), reverse=True)
    assert max(f[1] for f in fields) >= 2
    for score, m, ll in fields:
        assert abs(score - (ll + 4.0 * m)) < 1e-5
