"""GPU: the n-best search over paraformer's top-k lists on the device (csrc/k_nbestsearch.hip) — the kernel alone
(pf_op_nbest_search) against the definition (tests/nbest_search_ref.py) BIT FOR BIT in its four forms (plain, hot words, language
model, both) and both thread forms, with ragged lists, poisoned unread slots, ties, a position without entries and canaries in
every output; a model whose arc lists hold thousands of entries; zero weights = the plain form; the engine in every math mode
against the definition fed its own lists; refusals; the recognizer with a pool of two engines and two caller threads; the CLI; and
the CTC setters, which keep refusing a paraformer."""
import io
import threading
import wave

import numpy as np
import pytest

import ctcbeam_lm_ref as LR
import nbest_search_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import LanguageModel, host_nbest
from oracle import frontend as fe
from oracle import glue

pytestmark = pytest.mark.gpu
EOS = S.PF_LM_EOS
SCORES, TOPK, BEAM = N.PF_DECODE_SCORES, N.PF_DECODE_TOPK, N.PF_DECODE_CTC_BEAM
V_IN = 14                                                    # the ids of the kernel inputs: 0 .. 13


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def native(model):
    return LanguageModel(model.order, model.ngrams, model.V, model.bos, model.eos, model.unk, model.oov, sorted(model.transparent))


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


_cache = {}


def the_model():
    """(definition, library) of the one small model of the kernel cases: order 3, bos / eos, a transparent id, a missing unigram."""
    if "lm" not in _cache:
        m = S.small_model(V_IN, 3, bos=1, eos=2, transparent=(5,), missing=(V_IN - 1,))
        _cache["lm"] = (m, native(m))
    return _cache["lm"]


def kernel_input(L, K):
    """One utterance [L, K]: seeded log-softmax lists, every third position with tied values, ragged n[l] in 1 .. K, and poison
    in every slot past n[l] (an id no table holds, NaN); its hot words spell listed ids."""
    if (L, K) not in _cache:
        rng = np.random.default_rng(500 + 10 * L + K)
        ids, val, n = S.log_softmax_lists(rng, L, K, V_IN)
        ids, val, n = ids.copy(), val.copy(), n.copy()
        for l in range(0, L, 3):
            val[l] = np.round(val[l] * 2) / 2                                     # halves: ties within and across positions
        for l in range(L):
            n[l] = int(rng.integers(1, K + 1))
            ids[l, n[l]:] = 2 ** 40 + 12345
            val[l, n[l]:] = np.nan
        hot = [(int(ids[0, 0]), int(ids[min(1, L - 1), int(n[min(1, L - 1)]) - 1])), (int(ids[L - 1, 0]), 3, 5), (int(ids[L // 2, 0]),),
               (2, 4, 6, 8)]
        _cache[(L, K)] = (ids, val, n, [tuple(max(c, 1) for c in w) for w in hot])
    return _cache[(L, K)]


FORMS = {"plain": (False, False), "hot": (True, False), "lm": (False, True), "hot+lm": (True, True)}


def form_args(form, hot):
    """(definition's model, library's model, alpha, beta, flags, hot words, boost) of a form."""
    with_hot, with_lm = FORMS[form]
    m, lm = the_model() if with_lm else (None, None)
    a, b, fl = ((0.3, 1.0, EOS) if with_hot else (0.5, 0.25, 0)) if with_lm else (0.0, 0.0, 0)
    return m, lm, a, b, fl, (hot if with_hot else ()), (1.5 if with_hot else 0.0)


def definition(L, K, W, form, tn):
    key = ("ref", L, K, W, form, min(max(tn, 0), L))
    if key not in _cache:
        ids, val, n, hot = kernel_input(L, K)
        m, _lm, a, b, fl, h, s = form_args(form, hot)
        _cache[key] = S.search(ids, val, n, tn, W, None, m, a, b, fl, h, s)
    return _cache[key]


def canaries(B, Nb, L):
    return (np.full((B, Nb, L), -77, np.int32), np.full((B, Nb), 12345.0, np.float64), np.full((B, Nb), 12345.0, np.float64),
            np.full((B, Nb), 12345.0, np.float64), np.full((B, Nb), -77, np.int32), np.full(B, -77, np.int32))


def check_utterance(r, b, want, Nb, L, K):
    """utterance b of a result: the definition's hypotheses bit for bit, fill values behind them, no canary left"""
    assert int(r.n_hyp[b]) == len(want)
    assert [h.key() for h in S.as_hyps(r, b)] == [h.key() for h in want]
    k = len(want)
    assert (r.ranks[b, :k] >= 0).all() and (r.ranks[b, :k] < K).all()
    assert (r.ranks[b, k:] == -1).all() and (r.score[b, k:] == -np.inf).all() and (r.loglik_sum[b, k:] == -np.inf).all()
    assert (r.lm_sum[b, k:] == 0).all() and (r.matched[b, k:] == 0).all()


# ---- 1: the kernel against the definition, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("W", [1, 4, 32, 33, 64])
@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("L", [1, 2, 5, 40])
def test_kernel_equals_definition(any_engine, L, K, W, form):
    """B = 5 over one input: token_num (L, 1, 0, L + 7) and a fifth utterance with an empty position; N = W and N = 1.  W * K <= 256
    takes the 256-thread forms (W = 32 with K = 8 sits on the threshold), W = 33 and 64 with K = 8 the 512-thread ones."""
    ids, val, n, hot = kernel_input(L, K)
    _m, lm, a, b, fl, h, s = form_args(form, hot)
    B = 5
    ids5, val5 = np.ascontiguousarray(np.stack([ids] * B)), np.ascontiguousarray(np.stack([val] * B))
    n5 = np.ascontiguousarray(np.stack([n] * B))
    n5[4, L - 1] = 0                                                              # no entry at the last position: no hypothesis
    tns = np.array([L, 1, 0, L + 7, L], np.int32)
    for Nb in sorted({W, 1}):
        r = any_engine.op_nbest_search(ids5, val5, n5, tns, W, Nb, lm, a, b, fl, h, s, out=canaries(B, Nb, L))
        for u in range(4):
            check_utterance(r, u, definition(L, K, W, form, int(tns[u]))[:Nb], Nb, L, K)
        check_utterance(r, 4, [], Nb, L, K)
        s32 = float(np.float32(s))
        for u in range(4):                                                        # the identity, bit for bit
            for i in range(int(r.n_hyp[u])):
                assert S.bits((r.loglik_sum[u, i] + s32 * int(r.matched[u, i])) + r.lm_sum[u, i]) == S.bits(r.score[u, i])


def test_the_cases_reach_what_they_are_for():
    """The table above, looked at through the definition: ties decide, hot words complete, the beam prunes."""
    ref = definition(40, 8, 64, "hot+lm", 40)
    assert len(ref) == 64 and max(h.matched for h in ref) >= 2
    plain = definition(40, 8, 4, "plain", 40)
    assert [h.ranks for h in plain] != [h.ranks for h in definition(40, 8, 4, "hot+lm", 40)]     # the fusion changes the list
    tied = definition(5, 4, 64, "plain", 5)
    assert len({S.bits(h.score) for h in tied}) < len(tied)


def test_nan_and_inf_among_the_listed_values(any_engine):
    ids, val, n, _ = kernel_input(5, 4)
    n = np.full(5, 4, np.int32)
    ok = np.where(np.isnan(val), np.float32(-9.0), val)
    rows = []
    for x in (np.nan, np.inf, -np.inf):
        v = ok.copy()
        v[3, 2] = x
        rows.append(v)
    r = any_engine.op_nbest_search(np.stack([np.where(ids > 100, 1, ids)] * 3), np.stack(rows), np.stack([n] * 3), np.array([5, 5, 5], np.int32), 8,
                                   out=canaries(3, 8, 5))
    assert r.n_hyp.tolist() == [0, 0, 8]                                          # -inf orders like any other value
    want = S.search(np.where(ids > 100, 1, ids), rows[2], n, 5, 8)
    check_utterance(r, 2, want, 8, 5, 4)
    check_utterance(r, 0, [], 8, 5, 4)
    check_utterance(r, 1, [], 8, 5, 4)
    r = any_engine.op_nbest_search(np.zeros((2, 0, 4), np.int64), np.zeros((2, 0, 4), np.float32), np.zeros((2, 0), np.int32),
                                   np.array([0, 3], np.int32), 4, out=canaries(2, 4, 0))
    assert r.n_hyp.tolist() == [0, 0] and (r.score == -np.inf).all()             # L = 0


# ---- 2: a model whose arc lists are thousands of entries long ---------------------------------------------------------------------
def test_kernel_with_a_large_model(any_engine):
    counts, gi, lp, bo = LR.big_model_arrays()
    lm = LanguageModel.from_arrays(3, counts, gi, lp, bo, LR.BIG_V, bos=1, eos=2, oov=-9.0)
    assert lm.image_bytes > 32 * 1024 * 1024
    model = LR.big_model()
    L, K, Wd = 40, 8, 16
    ids, val, n, hot = kernel_input(L, K)                                         # ids below 14: the contexts with the long lists
    for alpha, beta, flags, h, s in ((0.5, 0.0, 0, (), 0.0), (0.3, 1.0, EOS, hot, 1.5)):
        r = any_engine.op_nbest_search(ids[None], val[None], n[None], np.array([L], np.int32), Wd, None, lm, alpha, beta, flags, h, s,
                                       out=canaries(1, Wd, L))
        check_utterance(r, 0, S.search(ids, val, n, L, Wd, None, model, alpha, beta, flags, h, s), Wd, L, K)
    lm.close()


# ---- 3: no weight means no change ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,K,Wd", [(40, 8, 64), (40, 4, 32), (5, 4, 33), (2, 8, 4)])
def test_zero_weights_are_the_plain_form_bit_for_bit(any_engine, L, K, Wd):
    ids, val, n, hot = kernel_input(L, K)
    _m, lm = the_model()
    args = (ids[None], val[None], n[None], np.array([L], np.int32), Wd, None)
    plain = any_engine.op_nbest_search(*args)
    for r in (any_engine.op_nbest_search(*args, lm, 0.0, 0.0, EOS, out=canaries(1, Wd, L)),
              any_engine.op_nbest_search(*args, None, 0.0, 0.0, 0, hot, 0.0, out=canaries(1, Wd, L)),
              any_engine.op_nbest_search(*args, lm, 0.0, 0.0, 0, hot, 0.0, out=canaries(1, Wd, L))):
        assert (r.n_hyp == plain.n_hyp).all() and (r.ranks == plain.ranks).all() and (r.matched == 0).all()
        for x, y in ((r.score, plain.score), (r.loglik_sum, plain.loglik_sum), (r.lm_sum, plain.lm_sum), (r.loglik_sum, r.score)):
            assert (_u64(x) == _u64(y)).all()
    # and with a model in use on this engine the plain form answers what it answered before
    any_engine.op_nbest_search(*args, lm, 0.5, 0.25, EOS, hot, 2.0)
    again = any_engine.op_nbest_search(*args)
    assert (again.ranks == plain.ranks).all() and (_u64(again.score) == _u64(plain.score)).all()


def test_kernel_refusals(any_engine):
    ids, val, n, hot = kernel_input(5, 4)
    _m, lm = the_model()
    args = (ids[None], val[None], n[None], np.array([5], np.int32))
    for Wd, Nb in ((65, 1), (4, 5), (4, 0), (0, 0)):
        with pytest.raises(N.PfError) as ei:
            any_engine.op_nbest_search(*args, Wd, Nb)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (Wd, Nb)
    for a, b, f, h, s in ((-1.0, 0.0, 0, (), 0.0), (float("nan"), 0.0, 0, (), 0.0), (1.0, float("inf"), 0, (), 0.0), (1.0, 0.0, 2, (), 0.0),
                          (1.0, 0.0, 0, [(1, 2)], -1.0), (1.0, 0.0, 0, [(0, 2)], 1.0)):
        with pytest.raises(N.PfError) as ei:
            any_engine.op_nbest_search(*args, 4, None, lm, a, b, f, h, s)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (a, b, f, h, s)
    bad_n = n.copy()
    bad_n[2] = 5
    with pytest.raises(N.PfError) as ei:
        any_engine.op_nbest_search(ids[None], val[None], bad_n[None], np.array([5], np.int32), 4)
    assert ei.value.code == N.PF_ERR_INVALID_ARG


# ---- 4: the engine, a small synthetic paraformer, every math mode ----------------------------------------------------------------
PF_VOCAB = 64


def _pf_model():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=PF_VOCAB)
    return cfg, W.synth_weights(cfg, seed=3)


def _audio():
    return [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]


def _engine_model():
    if "pf_lm" not in _cache:
        _cache["pf_lm"] = S.small_model(PF_VOCAB, 3, bos=1, eos=2, missing=(PF_VOCAB - 1,), seed=8)
    return _cache["pf_lm"]


def _hot_from_lists(topk, token_num):
    """hot words that spell second-ranked ids of the first utterances' lists (ids >= 1)"""
    hot = []
    for b in range(min(2, topk.ids.shape[0])):
        nf = min(int(token_num[b]), topk.ids.shape[1])
        if nf >= 2:
            hot.append((int(topk.ids[b, 0, 1]), int(topk.ids[b, 1, 0])))
            hot.append((int(topk.ids[b, nf - 1, 1]), 7, 9))
    return [tuple(max(c, 1) for c in w) for w in hot]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_search_is_the_definition_of_its_own_lists(mode):
    import ctypes as C
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _pf_model()
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    Wd, NB, K = 16, 10, 4
    for e in (e0, e1):
        e.set_decode(TOPK)
        e.set_topk(K)
    model = _engine_model()
    lm = native(model)
    e1.set_nbest_lm(lm, 0.6, 0.2, 0)                                              # inert until a search is installed
    r_inert = e1.recognize(audio)
    assert r_inert.search is None
    e1.set_nbest_lm(None)
    e1.set_nbest_search(Wd, NB)
    r0 = e0.recognize(audio, want_logits=True)
    r1 = e1.recognize(audio, want_logits=True)
    B, L = r1.token_ids.shape
    print("mode %d: L=%d token_num=%s" % (mode, L, r1.token_num.tolist()))
    assert r0.search is None and r1.search is not None and r1.search.N == NB and r1.search.ranks.shape == (B, NB, L)

    def unchanged(r):
        np.testing.assert_array_equal(r.token_ids, r0.token_ids)
        np.testing.assert_array_equal(r.token_num, r0.token_num)
        np.testing.assert_array_equal(_bits32(r.scores), _bits32(r0.scores))
        np.testing.assert_array_equal(r.topk.ids, r0.topk.ids)
        np.testing.assert_array_equal(_bits32(r.topk.val), _bits32(r0.topk.val))
        np.testing.assert_array_equal(r.topk.n, r0.topk.n)
    unchanged(r1)
    np.testing.assert_array_equal(_bits32(r1.logits), _bits32(r0.logits))

    def against_definition(r, *fusion):
        for b in range(B):
            want = S.search(r.topk.ids[b], r.topk.val[b], r.topk.n[b], int(r.token_num[b]), Wd, NB, *fusion)
            assert int(r.search.n_hyp[b]) == len(want) >= 2
            assert [h.key() for h in S.as_hyps(r.search, b)] == [h.key() for h in want], (mode, b)
    against_definition(r1)
    for b in range(B):                                                            # nothing fused: pf_host_nbest's list
        nf = min(L, int(r1.token_num[b]))
        ranks, sc = host_nbest(r1.topk.val[b], r1.topk.n[b], nf, NB + 1)
        assert len(set(_u64(sc).tolist())) == len(sc), "the synthetic model's hypotheses tie: choose another seed"
        k = min(NB, len(sc))
        assert r1.search.n_hyp[b] == k and r1.search.ranks[b, :k].tolist() == np.asarray(ranks)[:k].tolist()
        assert _u64(r1.search.score[b, :k]).tolist() == _u64(sc[:k]).tolist()
        np.testing.assert_array_equal(r1.topk.ids[b, np.arange(L), r1.search.ranks[b, 0]], r1.token_ids[b])    # hypothesis 0 is the result
    # the model, the hot words, both: one search each; everything else stays bit for bit
    hot = _hot_from_lists(r1.topk, r1.token_num)
    e1.set_nbest_lm(lm, 0.6, 0.2, 0)
    r2 = e1.recognize(audio)
    unchanged(r2)
    against_definition(r2, model, 0.6, 0.2, 0)
    assert any(r2.search.ranks[b].tolist() != r1.search.ranks[b].tolist() for b in range(B))      # the model mattered
    e1.set_nbest_hotwords(hot, 2.0)
    r3 = e1.recognize(audio)
    unchanged(r3)
    against_definition(r3, model, 0.6, 0.2, 0, hot, 2.0)
    assert r3.search.matched.max() >= 2
    e1.set_nbest_lm(None)
    r4 = e1.recognize(audio)
    against_definition(r4, None, 0.0, 0.0, 0, hot, 2.0)
    e1.set_nbest_hotwords([], 0.0)
    # the same model again with other weights and the flag: no new upload, the new scores
    e1.set_nbest_lm(lm, 0.3, -0.1, EOS)
    against_definition(e1.recognize(audio), model, 0.3, -0.1, EOS)
    lm.close()                                                                    # the engine keeps its own reference
    against_definition(e1.recognize(audio), model, 0.3, -0.1, EOS)
    # cleared: the forward of before, and the fetch is refused
    e1.set_nbest_search(0)
    r5 = e1.recognize(audio)
    assert r5.search is None
    unchanged(r5)
    e1.recognize(audio[:1])
    nh = np.zeros(1, np.int32)
    assert e1._lib.pf_fetch_nbest_search(e1._h, None, None, None, None, None, nh.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == N.PF_ERR_INVALID_ARG
    e0.close(); e1.close()


def test_engine_refusals(sv_embed):
    from aliparaformerasr_amd.engine import Engine, EngineGroup
    lm = LanguageModel(1, {(1,): (-1.0, None)}, 3)
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=403)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    sv = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    sc = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    for eng in (sv, sc):
        for call in (lambda: eng.set_nbest_search(4, 2), lambda: eng.set_nbest_lm(lm, 0.5), lambda: eng.set_nbest_hotwords([(1, 2)], 1.0)):
            with pytest.raises(N.PfError) as ei:
                call()
            assert ei.value.code == N.PF_ERR_UNSUPPORTED
        eng.close()
    cfg, w = _pf_model()
    blob = W.pack_pfw(cfg, w)
    pf = Engine(weights=blob, cmvn=W.synth_cmvn(), device=0)
    for Wd, Nb in ((65, 1), (4, 5), (4, 0), (-1, 1)):
        with pytest.raises(N.PfError) as ei:
            pf.set_nbest_search(Wd, Nb)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (Wd, Nb)
    for a, b, f in ((-1.0, 0.0, 0), (float("nan"), 0.0, 0), (float("inf"), 0.0, 0), (1.0, float("inf"), 0), (1.0, 0.0, 4)):
        with pytest.raises(N.PfError) as ei:
            pf.set_nbest_lm(lm, a, b, f)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (a, b, f)
    for hot, boost in (([(1, 2)], -1.0), ([(1, 2)], float("nan")), ([(0, 2)], 1.0), ([(1, PF_VOCAB)], 1.0)):
        with pytest.raises(N.PfError) as ei:
            pf.set_nbest_hotwords(hot, boost)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, (hot, boost)
    for bit in (4, 64):                                                           # there is no decode bit for it
        assert pf._lib.pf_engine_set_decode(pf._h, TOPK | bit) == N.PF_ERR_INVALID_ARG
    # the CTC setters keep refusing a paraformer
    for call in (lambda: pf.set_ctc_lm(lm, 0.5), lambda: pf.set_ctc_hotwords([(1, 2)], 1.0), lambda: pf.set_decode(BEAM)):
        with pytest.raises(N.PfError) as ei:
            call()
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    # a group forward refuses the search as it refuses the other extras
    g = EngineGroup([0, 0], weights=blob, cmvn=W.synth_cmvn())
    h0 = g._lib.pf_group_engine(g._h, 0)
    assert g._lib.pf_engine_set_nbest_search(h0, 4, 2) == N.PF_OK
    with pytest.raises(N.PfError) as ei:
        g.recognize(_audio()[:2])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    g.close()
    lm.close()


# ---- 5: the recognizer and the CLI --------------------------------------------------------------------------------------------------
def _pf_dir(tmp_path):
    cfg, w = _pf_model()
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(PF_VOCAB - 3)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], toks


def _get(rec, audio, hotwords=None):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        if hotwords is not None:
            s.Hotwords = [list(w) for w in hotwords]
        streams.append(s)
    return streams, rec.GetResults(streams)


def _alts(streams):
    return [[(tuple(a.Ids), a.Score, a.HotwordTokens, a.LogLikSum, a.LmSum, a.Text) for a in s.Alternatives] for s in streams]


def _arpa(tmp_path, toks):
    """an ARPA file written by the existing helper from the engine cases' model, and the model its text holds"""
    m = _engine_model()
    LR.write_arpa(tmp_path / "lm.arpa", m.order, m.ngrams, toks)
    order, g, dropped, bos, eos, unk, tr = LR.read_arpa(tmp_path / "lm.arpa", toks)
    assert dropped == 0 and (bos, eos, unk) == (1, 2, -1)
    return str(tmp_path / "lm.arpa"), LR.Model(order, g, len(toks), bos, eos, unk, -10.0, tr)


def test_recognizer_search(tmp_path, monkeypatch):
    """An ARPA file, hot words from the streams, a pool of two engines and two caller threads, the Alternatives' fields and the
    identity, clearing, refusals."""
    from aliparaformerasr_amd.engine import Engine
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    monkeypatch.setenv("PF_RECOGNIZER_ENGINES", "2")
    NB, Wd, K = 6, 16, 4
    audio = _audio()
    paths, toks = _pf_dir(tmp_path)
    arpa, model = _arpa(tmp_path, toks)
    cfg, w = _pf_model()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)       # the same lists from an engine on the same container
    eng.set_decode(TOPK)
    eng.set_topk(K)
    r = eng.recognize(audio)
    hot = _hot_from_lists(r.topk, r.token_num)
    rec = OfflineRecognizer(*paths)
    rec.SetNBestSearch(Wd)
    rec.SetNBestLm(arpa, 0.6, 0.2, 0)
    rec.SetNBestHotwordBoost(2.0)
    s_in, res_in = _get(rec, audio, hot)
    assert _alts(s_in) == [[]] * 3                                                # inert until SetNBest(N > 1, K)
    rec.SetNBestSearch(0)
    rec.SetNBest(NB, K)
    s0, res0 = _get(rec, audio, hot)
    base = _alts(s0)                                                              # the host enumeration: no extras
    assert all(a[3] is None and a[4] is None and a[2] == 0 for u in base for a in u)
    rec.SetNBestSearch(Wd)
    sf, resf = _get(rec, audio, hot)
    want = _alts(sf)
    for b in range(3):
        assert sf[b].Tokens == s0[b].Tokens == r.token_ids[b].tolist() and sf[b].TokenAlternatives == s0[b].TokenAlternatives
        assert (resf[b].Text, resf[b].Tokens, resf[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        ref = S.search(r.topk.ids[b], r.topk.val[b], r.topk.n[b], int(r.token_num[b]), Wd, NB, model, 0.6, 0.2, 0, hot, 2.0)
        assert len(want[b]) == len(ref) >= 2
        for (ids, score, m, ll, g, text), h in zip(want[b], ref):
            assert list(ids) == [int(r.topk.ids[b, l, h.ranks[l]]) for l in range(r.L)]
            assert (S.bits(score), S.bits(ll), S.bits(g), m) == (S.bits(h.score), S.bits(h.loglik_sum), S.bits(h.lm_sum), h.matched)
            assert S.bits((ll + 2.0 * m) + g) == S.bits(score)                    # the identity
            assert text == glue.decode_multi_one(toks, list(ids), sf[b].Timestamps)[0]
    assert any([a[0] for a in want[b]] != [a[0] for a in base[b]] for b in range(3))               # the fusion mattered
    assert max(a[2] for u in want for a in u) >= 2
    errors = []

    def worker(i):
        try:
            for _ in range(3):
                assert _alts(_get(rec, audio, hot)[0]) == want
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert rec._lib.pf_recognizer_num_engines(rec._h) == 2                       # both engines uploaded the image and the table
    # the search alone lists what the enumeration lists (no two hypotheses of these inputs tie), with the extras filled
    rec.SetNBestLm(None)
    rec.SetNBestHotwordBoost(0.0)
    alone = _alts(_get(rec, audio, hot)[0])
    assert [[a[:2] + (a[5],) for a in u] for u in alone] == [[a[:2] + (a[5],) for a in u] for u in base]
    assert all(a[2] == 0 and a[4] == 0.0 and a[3] == a[1] for u in alone for a in u)
    rec.SetNBestSearch(0)
    assert _alts(_get(rec, audio, hot)[0]) == base
    for call in (lambda: rec.SetNBestSearch(65), lambda: rec.SetNBestSearch(-1), lambda: rec.SetNBestHotwordBoost(-1.0),
                 lambda: rec.SetNBestLm(arpa, -1.0), lambda: rec.SetNBestLm(arpa, 0.5, float("inf")), lambda: rec.SetNBestLm(arpa, 0.5, 0.0, 8)):
        with pytest.raises(N.PfError) as ei:
            call()
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        rec.SetNBestLm(str(tmp_path / "missing.arpa"))
    assert ei.value.code == N.PF_ERR_IO
    # SetVad beside it is refused, whichever comes second
    rec.SetNBest(0)
    rec.SetNBestSearch(Wd)
    with pytest.raises(N.PfError) as ei:
        rec.SetVad(True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.SetNBestSearch(0)
    rec.SetVad(True)
    with pytest.raises(N.PfError) as ei:
        rec.SetNBestSearch(Wd)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.SetVad(False)
    # the CTC setters keep refusing a paraformer
    for call in (lambda: rec.SetLm(arpa), lambda: rec.SetHotwordBoost(2.0), lambda: rec.SetCtcBeam(4, 8, 4)):
        with pytest.raises(N.PfError) as ei:
            call()
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.close()
    rec.Dispose()


def test_recognizer_refuses_sensevoice_and_seaco(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    sv_cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=403)
    sv_w = W.synth_weights(sv_cfg, seed=9)
    sv_w["embed.weight"] = sv_embed.astype(np.float32)
    sc_cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    for k, (cfg, w, V, yaml) in enumerate(((sv_cfg, sv_w, 403, "model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n"),
                                           (sc_cfg, W.synth_weights(sc_cfg, 21), 120, "frontend_conf:\n  dither: 0\n"))):
        d = tmp_path / str(k)
        d.mkdir()
        W.save_pfw(str(d / "model.pfw"), cfg, w)
        (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
        (d / "asr.yaml").write_text(yaml)
        toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(V - 3)]
        (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
        LR.write_arpa(d / "lm.arpa", 1, {(3,): (-1.0, None)}, toks)
        rec = OfflineRecognizer(*[str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
        for call in (lambda: rec.SetNBestSearch(8), lambda: rec.SetNBestLm(str(d / "lm.arpa")), lambda: rec.SetNBestHotwordBoost(1.0)):
            with pytest.raises(N.PfError) as ei:
                call()
            assert ei.value.code == N.PF_ERR_UNSUPPORTED
        rec.SetNBestSearch(0); rec.SetNBestLm(None); rec.SetNBestHotwordBoost(0.0)    # "off" is always fine
        rec.Dispose()


def test_cli_search(tmp_path):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "m"
    d.mkdir()
    _, toks = _pf_dir(d)
    arpa, _model = _arpa(d, toks)
    pcm = (np.clip(W.synth_audio(32000, 40), -1, 1) * 32767).astype("<i2")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())

    def run(**kw):
        out = io.StringIO()
        res = ex.offline_recognizer(method="one", model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=4, topk=4, **kw)
        return res, [ln for ln in out.getvalue().splitlines() if ln.startswith("nbest[")]
    res0, nb0 = run()
    assert len(nb0) == 4 and all(" lm:" not in ln and " hot:" not in ln for ln in nb0)             # without -search the lines of today
    res1, nb1 = run(search=16, lm=arpa, lmweight=0.7, lmbonus=0.3, hotboost=1.5)
    assert res1[0].Text == res0[0].Text and len(nb1) == 4
    fields = [(float(ln.split("score:")[1].split(" ")[0]), int(ln.split(" hot:")[1].split(" ")[0]), float(ln.split(" lm:")[1].split(" ")[0]),
               float(ln.split("loglik_sum:")[1])) for ln in nb1]
    assert [f[0] for f in fields] == sorted((f[0] for f in fields), reverse=True)
    for score, m, g, ll in fields:
        assert g != 0 and abs(score - (ll + 1.5 * m + g)) < 1e-5
    with pytest.raises(N.PfError) as ei:                                          # without -search every option does what it did
        run(lm=arpa, beam=8)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
