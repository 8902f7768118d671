"""GPU: n-gram LM shallow fusion inside the CTC prefix beam search on the device (the kLm forms of csrc/k_ctcbeam.hip through
pf_op_ctc_beam_lm) — the kernel against the definition (tests/ctcbeam_lm_ref.py) over the committed inputs with the model alone
and together with hot words, canaries and poisoned unread rows, a model whose image exceeds 32 MB, alpha = beta = 0 = no change,
and the unfused and hot-word forms untouched by a model in use on the same engine.

Comparison rule: token lists and their order identical; lm_sum and matched bit-equal; score and loglik_sum within
ctcbeam_lm_ref.tol; the identity score == (loglik_sum + boost * matched) + lm_sum bit for bit."""
import numpy as np
import pytest

import ctcbeam_bias_ref as BR
import ctcbeam_lm_ref as LR
import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import LanguageModel

pytestmark = pytest.mark.gpu
EOS = LR.PF_LM_EOS
BOOST = BR.RECIPE_BOOST


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _hyps(res, b):
    return [(tuple(res.ids[b, i, : int(res.len[b, i])].tolist()), float(res.score[b, i]), int(res.matched[b, i]),
             float(res.loglik_sum[b, i]), float(res.lm_sum[b, i])) for i in range(int(res.n_hyp[b]))]


def _same(got, want, T, boost):
    assert [h[0] for h in got] == [h[0] for h in want]
    for g, w in zip(got, want):
        tol = LR.tol(T, w[1], w[3], w[4])
        print("    score %.17g  definition %.17g  |diff| %.3g  tol %.3g  matched %d  lm %.17g" % (g[1], w[1], abs(g[1] - w[1]), tol, g[2], g[4]))
        assert g[2] == w[2] and _u64([g[4]])[0] == _u64([w[4]])[0], (g, w)
        assert abs(g[1] - w[1]) <= tol and abs(g[3] - w[3]) <= tol, (g, w, tol)
        assert g[1] == (g[3] + float(np.float32(boost)) * g[2]) + g[4]


def _canaries(B, n_best, cap):
    return (np.full((B, n_best, cap), 0x5A5A5A5A5A5A5A5A, np.int64), np.full((B, n_best), -77, np.int32),
            np.full((B, n_best), 12345.0, np.float64), np.full(B, -77, np.int32), np.full((B, n_best), -77, np.int32),
            np.full((B, n_best), 12345.0, np.float64), np.full((B, n_best), 12345.0, np.float64))


def _check_fill(r, b, n_best, T):
    for i in range(n_best):                                                       # fill values, no canary left
        k = int(r.len[b, i])
        assert 0 <= k <= T and (r.ids[b, i, k:] == -1).all() and (r.ids[b, i, :k] >= 1).all()
        if i >= r.n_hyp[b]:
            assert k == 0 and r.score[b, i] == -np.inf and r.matched[b, i] == 0 and r.loglik_sum[b, i] == -np.inf and r.lm_sum[b, i] == 0


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


_models = {}


def case_native(case):
    if case not in _models:
        m = LR.case_lm(case)
        _models[case] = LanguageModel(m.order, m.ngrams, m.V, m.bos, m.eos, m.unk, m.oov, sorted(m.transparent))
    return _models[case]


# ---- 1: the kernel against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_hot", [False, True], ids=["lm", "lm+hot"])
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_kernel_equals_definition(any_engine, case, with_hot):
    """The recipe's model (and hot words at s = 2); N = W and N = 1; every output slot is overwritten (canary).  full_lds takes
    the 1024-thread forms, the others the 256-thread ones."""
    lb, ids, val, n = R.case_arrays(case)
    T, Wd = case[2], case[5]
    alpha, beta, flags = ((0.3, 1.0, EOS) if with_hot else (0.5, 0.0, 0))
    hot, boost = (BR.case_hotwords(case), BOOST) if with_hot else ((), 0.0)
    args = _batch_of_three(lb, ids, val, n, T)
    refs = [LR.case_reference(case, alpha, beta, flags, with_hot, T=t).beam for t in (None, 1, 0)]
    lm = case_native(case)
    for n_best in sorted({Wd, 1}):
        r = any_engine.op_ctc_beam_lm(*args, Wd, lm, alpha, beta, flags, hot, boost, n_best, out=_canaries(3, n_best, T))
        for b in range(3):
            want = refs[b][:n_best]
            print("  %s N=%d utterance %d: %d hypotheses" % (case[0], n_best, b, len(want)))
            assert r.n_hyp[b] == len(want)
            _same(_hyps(r, b), want, max(int(args[4][b]), 1), boost)
            _check_fill(r, b, n_best, T)


def test_kernel_with_an_image_above_32_mb(any_engine):
    """An order-3 model over V = 25 055 with 3.4 million n-grams: the arc lists the search walks hold up to 18 790 entries."""
    case = [c for c in R.GPU_CASES if c[0] == "t65"][0]
    lb, ids, val, n = R.case_arrays(case)
    T, Wd = case[2], case[5]
    counts, gi, lp, bo = LR.big_model_arrays()
    lm = LanguageModel.from_arrays(3, counts, gi, lp, bo, LR.BIG_V, bos=1, eos=2, oov=-9.0)
    assert lm.image_bytes > 32 * 1024 * 1024 and lm.arcs == counts[1] + counts[2]
    model = LR.big_model()
    args = _batch_of_three(lb, ids, val, n, T)
    for alpha, beta, flags in ((0.5, 0.0, 0), (0.3, 1.0, EOS)):
        r = any_engine.op_ctc_beam_lm(*args, Wd, lm, alpha, beta, flags, out=_canaries(3, Wd, T))
        for b, t in enumerate((T, 1, 0)):
            ref = LR.beam_search(lb[:t], ids[:t], val[:t], n[:t], Wd, model, alpha, beta, flags)
            _same(_hyps(r, b), ref.beam, max(t, 1), 0.0)
            _check_fill(r, b, Wd, T)
    lm.close()


# ---- 2: no weight means no change; the other forms are what they were ------------------------------------------------------
@pytest.mark.parametrize("name", ["t65", "full_lds", "ragged", "mirror_w64", "w1"])
def test_zero_weights_are_the_unfused_kernel_bit_for_bit(any_engine, name):
    case = [c for c in R.GPU_CASES if c[0] == name][0]
    lb, ids, val, n = R.case_arrays(case)
    T, Wd = case[2], case[5]
    args = _batch_of_three(lb, ids, val, n, T)
    hot = BR.case_hotwords(case)
    plain = any_engine.op_ctc_beam(*args, Wd)
    biased = any_engine.op_ctc_beam_hot(*args, Wd, hot, BOOST)
    lm = case_native(case)
    r = any_engine.op_ctc_beam_lm(*args, Wd, lm, 0.0, 0.0, EOS, out=_canaries(3, Wd, T))
    assert (r.n_hyp == plain.n_hyp).all() and (r.ids == plain.ids).all() and (r.len == plain.len).all()
    assert (_u64(r.score) == _u64(plain.score)).all() and (_u64(r.loglik_sum) == _u64(plain.score)).all()
    assert (r.matched == 0).all() and (r.lm_sum == 0).all()
    r = any_engine.op_ctc_beam_lm(*args, Wd, lm, 0.0, 0.0, 0, hot, BOOST, out=_canaries(3, Wd, T))
    assert (r.n_hyp == biased.n_hyp).all() and (r.ids == biased.ids).all() and (r.len == biased.len).all()
    assert (_u64(r.score) == _u64(biased.score)).all() and (_u64(r.loglik_sum) == _u64(biased.loglik_sum)).all()
    assert (r.matched == biased.matched).all() and (r.lm_sum == 0).all()
    # and with a model in use on this engine the unfused and the hot-word forms answer what they answered before
    any_engine.op_ctc_beam_lm(*args, Wd, lm, 0.5, 0.25, EOS, hot, BOOST)
    again, again_hot = any_engine.op_ctc_beam(*args, Wd), any_engine.op_ctc_beam_hot(*args, Wd, hot, BOOST)
    for a, b in ((again, plain), (again_hot, biased)):
        assert (a.n_hyp == b.n_hyp).all() and (a.ids == b.ids).all() and (a.len == b.len).all() and (_u64(a.score) == _u64(b.score)).all()
    assert (again_hot.matched == biased.matched).all() and (_u64(again_hot.loglik_sum) == _u64(biased.loglik_sum)).all()


def test_kernel_refusals(any_engine):
    case = R.GPU_CASES[-1]
    lb, ids, val, n = R.case_arrays(case)
    args = (lb[None], ids[None], val[None], n[None], np.array([12], np.int32))
    lm = case_native(case)
    for a, b, f, hot, boost in ((-1.0, 0.0, 0, (), 0.0), (float("nan"), 0.0, 0, (), 0.0), (1.0, float("inf"), 0, (), 0.0),
                                (1.0, 0.0, 2, (), 0.0), (1.0, 0.0, 0, [(1, 2)], -1.0), (1.0, 0.0, 0, [(0, 2)], 1.0)):
        with pytest.raises(N.PfError) as ei:
            any_engine.op_ctc_beam_lm(*args, 3, lm, a, b, f, hot, boost)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (a, b, f, hot, boost)


# ---- 3: the engine, the tiny SenseVoice model of tests/test_gpu_ctcbeam.py, every math mode ---------------------------------
import io          # noqa: E402
import threading   # noqa: E402
import wave        # noqa: E402

from oracle import frontend as fe   # noqa: E402
from oracle import glue             # noqa: E402

SCORES, CTC, TOPK, BEAM, ALIGN = N.PF_DECODE_SCORES, N.PF_DECODE_CTC, N.PF_DECODE_TOPK, N.PF_DECODE_CTC_BEAM, N.PF_DECODE_ALIGN
SV_VOCAB = 403


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def _sv_lm_grams(hyp_lists, seed=5):
    """An order-3 model over the tiny SenseVoice vocabulary: the ids 1 .. 19 but 6 are unigrams (6 and everything above 19 are
    not), the 2- and 3-grams of the LAST hypotheses of the given lists are listed with good weights (so the model pulls them
    up), and 60 random ones over the ids the model emits (below 8) more."""
    rng = np.random.default_rng(seed)
    grams = {(c,): (np.float32(rng.uniform(-4.0, -1.0)), np.float32(rng.uniform(-1.0, 0.0))) for c in range(1, 20) if c != 6}
    for hyps in hyp_lists:
        y = hyps[-1][0]
        for k in (2, 3):
            for p in range(len(y) - k + 1):
                w = tuple(int(c) for c in y[p:p + k])
                if 6 not in w and w not in grams:
                    grams[w] = (np.float32(rng.uniform(-0.3, -0.05)), np.float32(rng.uniform(-0.3, 0.0)) if k == 2 else None)
    for x in range(60):
        w = tuple(int(c) for c in rng.integers(1, 8, 2 + x % 2))
        if 6 not in w and w not in grams:
            grams[w] = (np.float32(rng.uniform(-3.0, -0.5)), None if x % 4 == 0 or len(w) == 3 else np.float32(rng.uniform(-0.5, 0.0)))
    return grams


def _hot_from(hyps):
    y = hyps[min(len(hyps) - 1, 3)][0]
    return [w for w in (tuple(y[0:3]), tuple(y[4:6])) if w]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_fused_beam_is_the_definition_of_its_own_lists(sv_embed, mode):
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
    model = LR.Model(3, _sv_lm_grams([r0.beam.hyps(b) for b in range(3)]), SV_VOCAB, bos=1, eos=2, oov=-6.0)
    lm = LanguageModel(model.order, model.ngrams, model.V, model.bos, model.eos, model.unk, model.oov)
    alpha, beta = 0.8, 0.4
    e1.set_ctc_lm(lm, alpha, beta, EOS)
    r1 = e1.recognize(audio, want_logits=True)
    assert r0.beam.lm_sum is None and r1.beam.lm_sum is not None and r1.beam.N == NB and not r1.beam.matched.any()
    # token ids, scores, the collapse, the lists and the logits are bit-identical with and without the model
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits32(r1.scores), _bits32(r0.scores))
    np.testing.assert_array_equal(_bits32(r1.logits), _bits32(r0.logits))
    np.testing.assert_array_equal(r1.topk.ids, r0.topk.ids)
    np.testing.assert_array_equal(_bits32(r1.topk.val), _bits32(r0.topk.val))
    np.testing.assert_array_equal(r1.topk.n, r0.topk.n)
    np.testing.assert_array_equal(r1.ctc.n, r0.ctc.n)
    np.testing.assert_array_equal(r1.ctc.ids, r0.ctc.ids)
    np.testing.assert_array_equal(_bits32(r1.ctc.score), _bits32(r0.ctc.score))
    rows = [4 + e1.frontend(a).shape[0] for a in audio]                          # n_b: the prompt rows and the utterance's frames
    changed = 0
    for b, nb in enumerate(rows):
        ref = LR.beam_search(r1.logits[b, :nb, 0], r1.topk.ids[b, :nb], r1.topk.val[b, :nb], r1.topk.n[b, :nb], Wd, model, alpha, beta,
                             EOS, N=NB)
        print("  mode %d utterance %d: n_b=%d, %d hypotheses, decision gap %.3g" % (mode, b, nb, ref.n_hyp, ref.gap))
        assert r1.beam.n_hyp[b] == ref.n_hyp >= 2
        got = _hyps(r1.beam, b)
        _same(got, ref.hyps, nb, 0.0)                                             # (with the identity, bit for bit)
        changed += [h[0] for h in got] != [h[0] for h in r0.beam.hyps(b)]
        lp = r1.logits[b, :nb].astype(np.float64)
        for labels, _score, _m, ll, _g in got:
            full = R.ctc_loglik(lp, labels)                                       # the search sums a subset of the alignments
            assert ll <= full + BR.tol(nb, full), (labels, ll, full)
    assert changed >= 1                                                           # the model mattered
    # the same model again only takes the weights; the unfused and hot-word kernels on this engine answer as on the other
    e1.set_ctc_lm(lm, alpha, beta, EOS)
    r2 = e1.recognize(audio)
    assert [_hyps(r2.beam, b) for b in range(3)] == [_hyps(r1.beam, b) for b in range(3)]
    case = R.GPU_CASES[2]
    cl = R.case_arrays(case)
    args = tuple(a[None] for a in cl) + (np.array([case[2]], np.int32),)
    hot = BR.case_hotwords(case)
    for a, b in ((e1.op_ctc_beam(*args, case[5]), e0.op_ctc_beam(*args, case[5])),
                 (e1.op_ctc_beam_hot(*args, case[5], hot, BOOST), e0.op_ctc_beam_hot(*args, case[5], hot, BOOST))):
        assert (a.ids == b.ids).all() and (a.len == b.len).all() and (_u64(a.score) == _u64(b.score)).all()
    if mode == 0:                                                                 # together with hot words, one search
        hw = _hot_from(r0.beam.hyps(0)) + _hot_from(r0.beam.hyps(2))
        e1.set_ctc_hotwords(hw, BOOST)
        r4 = e1.recognize(audio, want_logits=True)
        for b, nb in enumerate(rows):
            ref = LR.beam_search(r4.logits[b, :nb, 0], r4.topk.ids[b, :nb], r4.topk.val[b, :nb], r4.topk.n[b, :nb], Wd, model, alpha,
                                 beta, EOS, hw, BOOST, NB)
            _same(_hyps(r4.beam, b), ref.hyps, nb, BOOST)
        assert r4.beam.matched.max() >= 2
        e1.set_ctc_hotwords([], 0.0)
    # after clearing the model the unfused results return, and the extras are refused
    e1.set_ctc_lm(None)
    r3 = e1.recognize(audio)
    assert r3.beam.lm_sum is None and r3.beam.matched is None
    assert [r3.beam.hyps(b) for b in range(3)] == [r0.beam.hyps(b) for b in range(3)]
    e1.recognize(audio[:1])
    g = np.zeros((1, NB), np.float64)
    assert e1._lib.pf_fetch_ctc_beam_lm(e1._h, g.ctypes.data_as(C.POINTER(C.c_double)), None) == N.PF_ERR_INVALID_ARG
    e1.set_ctc_lm(lm, 0.0, 0.0, 0)                                                # zero weights: the unfused list with lm_sum 0
    r5 = e1.recognize(audio)
    assert [r5.beam.hyps(b) for b in range(3)] == [r0.beam.hyps(b) for b in range(3)] and not r5.beam.lm_sum.any()
    lm.close()                                                                    # the engine keeps its own reference
    assert [_hyps(e1.recognize(audio).beam, b) for b in range(3)] == [_hyps(r5.beam, b) for b in range(3)]
    e0.close(); e1.close()


def test_engine_align_jobs_are_the_fused_hypotheses(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    audio = _audio()
    eng.set_decode(BEAM | ALIGN)
    eng.set_ctc_beam(8, 4)
    r0 = eng.recognize(audio, want_logits=True)
    lm = LanguageModel(3, _sv_lm_grams([r0.beam.hyps(b) for b in range(3)]), SV_VOCAB, 1, 2, oov=-6.0)
    eng.set_ctc_lm(lm, 0.8, 0.4, EOS)
    r1 = eng.recognize(audio, want_logits=True)
    assert r1.align.len.shape == (3, 4)
    rows = [4 + eng.frontend(a).shape[0] for a in audio]
    for b in range(3):
        for i, (labels, _score, _m, ll, _g) in enumerate(_hyps(r1.beam, b)):
            assert r1.align.len[b, i] == len(labels)                              # job i is fused hypothesis i
            full = R.ctc_loglik(r1.logits[b, : rows[b]].astype(np.float64), labels)
            assert abs(r1.align.loglik[b, i] - full) <= 1e-9 * max(1.0, abs(full)) and ll <= r1.align.loglik[b, i] + 1e-9
    lm.close()
    eng.close()


def test_engine_refusals(sv_embed):
    from aliparaformerasr_amd.engine import Engine, EngineGroup
    lm = LanguageModel(1, {(1,): (-1.0, None)}, 3)
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pf = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        pf.set_ctc_lm(lm, 0.5)                                                    # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    sc = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        sc.set_ctc_lm(lm, 0.5)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    sc.close()
    cfg, w = _sv_model(sv_embed)
    blob = W.pack_pfw(cfg, w)
    eng = Engine(weights=blob, cmvn=W.synth_cmvn(), device=0)
    for a, b, f in ((-1.0, 0.0, 0), (float("nan"), 0.0, 0), (float("inf"), 0.0, 0), (1.0, float("inf"), 0), (1.0, 0.0, 4)):
        with pytest.raises(N.PfError) as ei:
            eng.set_ctc_lm(lm, a, b, f)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (a, b, f)
    for bit in (4, 64):                                                           # there is no decode bit for it
        assert eng._lib.pf_engine_set_decode(eng._h, BEAM | bit) == N.PF_ERR_INVALID_ARG
    eng.close()
    # a group forward refuses the beam search as it always did, model or no model
    g = EngineGroup([0, 0], weights=blob, cmvn=W.synth_cmvn())
    h0 = g._lib.pf_group_engine(g._h, 0)
    assert g._lib.pf_engine_set_decode(h0, BEAM) == N.PF_OK
    assert g._lib.pf_engine_set_ctc_lm(h0, lm._h, 0.5, 0.0, 0) == N.PF_OK
    with pytest.raises(N.PfError) as ei:
        g.recognize(_audio()[:2])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    g.close()
    lm.close()


# ---- 4: the recognizer and the API surface -------------------------------------------------------------------------------------
def _sv_dir(tmp_path, sv_embed):
    """a SenseVoice model directory whose ids 1 .. are single characters (1 and 2 spelled <s> and </s>), so that an ARPA file
    can spell them"""
    cfg, w = _sv_model(sv_embed)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(SV_VOCAB - 3)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], toks


def _get(rec, audio):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        streams.append(s)
    return streams, rec.GetResults(streams)


def _alts(streams):
    return [[(tuple(a.Ids), a.Score, a.HotwordTokens, a.LogLikSum, a.LmSum, a.Text) for a in s.Alternatives] for s in streams]


def _arpa_for(tmp_path, toks, base):
    """an ARPA file made from the unfused alternatives `base`, and the model its text holds"""
    grams = _sv_lm_grams([[(a[0],) for a in u] for u in base])
    LR.write_arpa(tmp_path / "lm.arpa", 3, grams, toks)
    order, g, dropped, bos, eos, unk, tr = LR.read_arpa(tmp_path / "lm.arpa", toks)
    assert dropped == 0 and (bos, eos, unk) == (1, 2, -1)
    return str(tmp_path / "lm.arpa"), LR.Model(order, g, len(toks), bos, eos, unk, -10.0, tr)


def test_recognizer_lm(tmp_path, sv_embed, monkeypatch):
    """An ARPA file, a pool of two engines and two caller threads, SetAlign beside it, clearing."""
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    monkeypatch.setenv("PF_RECOGNIZER_ENGINES", "2")
    NB, Wd, K = 4, 8, 4
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    paths, toks = _sv_dir(tmp_path, sv_embed)
    rec = OfflineRecognizer(*paths)
    rec.SetCtcBeam(NB, Wd, K)
    s0, res0 = _get(rec, audio)
    base = _alts(s0)
    assert all(a[3] is None and a[4] is None for u in base for a in u)            # unfused: no extras
    arpa, model = _arpa_for(tmp_path, toks, base)
    alpha, beta = 0.8, 0.4
    rec.SetCtcBeam(0, 0, 0)
    rec.SetLm(arpa, alpha, beta, EOS)
    s1, res1 = _get(rec, audio)
    assert _alts(s1) == [[]] * 2 and res1[0].Text == res0[0].Text                 # inert until SetCtcBeam is set
    rec.SetCtcBeam(NB, Wd, K)
    sf, resf = _get(rec, audio)
    changed = 0
    for b in range(2):
        assert sf[b].Tokens == s0[b].Tokens and (resf[b].Text, resf[b].Tokens, resf[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        alts = _alts(sf)[b]
        assert 2 <= len(alts) <= NB
        sc = [a[1] for a in alts]
        assert sc == sorted(sc, reverse=True)
        for ids, score, m, ll, g, text in alts:
            assert m == 0 and _u64([g])[0] == _u64([model.score(ids, alpha, beta, EOS)[0]])[0] and score == ll + g
            assert text == glue.decode_multi_one(toks, list(ids), [[0, 0]] * len(ids))[0]
        changed += [a[0] for a in alts] != [a[0] for a in base[b]]
    assert changed >= 1
    want = _alts(sf)
    errors = []

    def worker(i):
        try:
            for _ in range(3):
                assert _alts(_get(rec, audio)[0]) == want
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert rec._lib.pf_recognizer_num_engines(rec._h) == 2                       # both engines uploaded the image
    # SetAlign beside it: the fused alternatives get their own times and the full log-likelihood
    rec.SetAlign(True)
    sa, _ = _get(rec, audio)
    assert [a[:5] for a in _alts(sa)[0]] == [a[:5] for a in want[0]]
    for a in sa[0].Alternatives:
        assert a.LogLik is not None and a.LogLikSum <= a.LogLik + 1e-9 and len(a.Timestamps) in (0, len(a.Ids))
    rec.SetAlign(False)
    # other weights re-score without a reload of anything but the file; off again: the unfused list; refusals
    rec.SetLm(arpa, 0.0, 0.0, 0)
    assert [[a[:2] for a in u] for u in _alts(_get(rec, audio)[0])] == [[a[:2] for a in u] for u in base]
    rec.SetLm(None)
    assert _alts(_get(rec, audio)[0]) == base
    for a, b, f in ((-1.0, 0.0, 0), (float("nan"), 0.0, 0), (1.0, float("inf"), 0), (1.0, 0.0, 8)):
        with pytest.raises(N.PfError) as ei:
            rec.SetLm(arpa, a, b, f)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        rec.SetLm(str(tmp_path / "missing.arpa"))
    assert ei.value.code == N.PF_ERR_IO
    rec.Dispose()


def test_recognizer_refuses_paraformer_and_seaco(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    for k, (cfg, seed, V) in enumerate(((W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64), 3, 64),
                                        (W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111), 21, 120))):
        d = tmp_path / str(k)
        d.mkdir()
        W.save_pfw(str(d / "model.pfw"), cfg, W.synth_weights(cfg, seed))
        (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
        (d / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
        toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(V - 3)]
        (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
        LR.write_arpa(d / "lm.arpa", 1, {(3,): (-1.0, None)}, toks)
        rec = OfflineRecognizer(*[str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
        with pytest.raises(N.PfError) as ei:
            rec.SetLm(str(d / "lm.arpa"))
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
        rec.SetLm(None)                                                           # "off" is always fine
        rec.Dispose()


def test_cli_lm(tmp_path, sv_embed):
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
    assert len(nb0) == 3 and all(" lm:" not in ln for ln in nb0)                  # without -lm the lines of today
    LR.write_arpa(d / "lm.arpa", 2, {(c,): (-1.0 - 0.25 * c, -0.5) for c in range(1, 12)} | {(3, 4): (-0.1, None), (4, 3): (-0.2, None)}, toks)
    res1, nb1 = run(lm=str(d / "lm.arpa"), lmweight=0.7, lmbonus=0.3, lmeos=True)
    assert res1[0].Text == res0[0].Text and len(nb1) == 3
    fields = [(float(ln.split("score:")[1].split(" ")[0]), float(ln.split(" lm:")[1].split(" ")[0]), float(ln.split("loglik_sum:")[1]))
              for ln in nb1]
    assert [f[0] for f in fields] == sorted((f[0] for f in fields), reverse=True)
    for score, g, ll in fields:
        assert g != 0 and abs(score - (ll + g)) < 1e-5
