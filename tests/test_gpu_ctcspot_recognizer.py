"""GPU: phrase spotting behind the forward (Engine.set_spotter, OfflineRecognizer.SetKeywords) on the tiny SenseVoice model
of tests/test_gpu_ctcalign.py.  The engine's hits equal the host twin run on the log-prob rows that same forward left; the
recognizer's KeywordHits are the hits of the engine that ran the batch, frames converted exactly as pf_stream_alignment
converts them; every other result is what it is without a phrase list; the refusals answer the stated codes."""
import ctypes as C
import math

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import host_ctc_spot
from test_gpu_ctcalign import SV_VOCAB, _audio, _get, _sv_dir, _sv_model

pytestmark = pytest.mark.gpu
THR, HITS = math.log(0.001), 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ms(first, last):
    return [60 * max(first - 4, 0), 60 * max(last + 1 - 4, 0)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_hits_are_the_twin_on_its_own_rows(sv_embed, mode):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e0.set_decode(N.PF_DECODE_CTC)
    e1.set_decode(N.PF_DECODE_CTC)
    r0 = e0.recognize(audio, want_logits=True)
    greedy = [[int(v) for v in r0.ctc.ids[b, : r0.ctc.n[b]]] for b in range(3)]
    phrases = [g[:32] for g in greedy if g] + [[5], [5, 5], [6, 5], [7, 6, 5, 5]]
    e1.set_spotter(phrases, THR, HITS)
    r1 = e1.recognize(audio, want_logits=True)
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r1.logits), _bits(r0.logits))
    rows = [4 + e1.frontend(a).shape[0] for a in audio]                          # n_b: the prompt rows and the utterance's frames
    for b, nb in enumerate(rows):
        for k, y in enumerate(phrases):
            ref = host_ctc_spot(r1.logits[b, :nb], y, THR, HITS)
            assert r1.spot.n_hits[b, k] == ref.n_hits[0, 0], (mode, b, k)
            np.testing.assert_array_equal(r1.spot.begin_end[b, k], ref.begin_end[0, 0])
            np.testing.assert_array_equal(_bits(r1.spot.score[b, k]), _bits(ref.score[0, 0]))
    assert int(r1.spot.n_hits.sum()) >= 3 and (r1.spot.begin_end[:, :, :, 1] < np.array(rows)[:, None, None]).all()
    e1.set_spotter(None)                                                          # cleared: nothing extra comes back
    assert e1.recognize(audio).spot is None and e1._lib.pf_fetch_spot(e1._h, None, None, None) == N.PF_ERR_INVALID_ARG
    e0.close(); e1.close()


def test_recognizer_keyword_hits(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, toks = _sv_dir(tmp_path, sv_embed)
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    plain, ctc, rec = (OfflineRecognizer(*paths) for _ in range(3))
    ctc.SetDecode(ctc=True)
    sc, _ = _get(ctc, audio)
    s0, res0 = _get(plain, audio)
    whole = [s.Tokens[:32] for s in sc]                                           # phrases that are the whole decoded text
    assert min(len(t) for t in whole) >= 1
    phrases = whole + [[5, 6], toks[30] + toks[31]]                               # ids, and a line of text
    rec.SetKeywords(phrases, threshold=0.001, max_hits=HITS)
    rec.SetAlign(True)
    s1, res1 = _get(rec, audio, whole)
    lib, h = rec._lib, C.c_void_p(rec._lib.pf_recognizer_engine(rec._h))
    K = len(phrases)
    nh, be, sco = np.zeros((2, K), np.int32), np.zeros((2, K, HITS, 2), np.int32), np.zeros((2, K, HITS), np.float32)
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    first, last = np.zeros((2, 1, 32), np.int32), np.zeros((2, 1, 32), np.int32)
    N.check(lib.pf_fetch_align(h, None, None, None, None, first.ctypes.data_as(i32), last.ctypes.data_as(i32), None, 32, None, None))
    N.check(lib.pf_fetch_spot(h, nh.ctypes.data_as(i32), be.ctypes.data_as(i32), sco.ctypes.data_as(f32)))
    assert int(nh[:, :2].sum()) >= 2
    for b in range(2):
        assert s1[b].Tokens == s0[b].Tokens and s1[b].Timestamps == s0[b].Timestamps
        assert (res1[b].Text, res1[b].Tokens, res1[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        assert s0[b].KeywordHits is None
        # the conversion this test applies to the hits' frames is pf_stream_alignment's
        U = len(whole[b])
        al = s1[b].Alignment
        assert al.Ok == 1 and al.Timestamps == [_ms(first[b, 0, u], last[b, 0, u]) for u in range(U)]
        want = [(k, *_ms(*be[b, k, i]), math.exp(float(sco[b, k, i]) / (be[b, k, i, 1] - be[b, k, i, 0] + 1)))
                for k in range(K) for i in range(min(nh[b, k], HITS))]
        assert s1[b].KeywordHits == want
    rec.SetKeywords(None)                                                         # beside long-audio recognition, either order
    rec.SetAlign(False)
    rec.SetVad(True)
    with pytest.raises(N.PfError) as ei:
        rec.SetKeywords([[5]])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.SetVad(None)
    rec.SetKeywords([[5]])
    with pytest.raises(N.PfError) as ei:
        rec.SetVad(True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    for r in (plain, ctc, rec):
        r.Dispose()


def test_refusals(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pf = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        pf.set_spotter([[5]])                                                     # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    cfg, w = _sv_model(sv_embed)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    bad = [([[0]], THR, 4), ([[SV_VOCAB]], THR, 4), ([[5], []], THR, 4), ([[5] * (N.PF_SPOT_MAX_TOKENS + 1)], THR, 4), ([[5]], THR, 0),
           ([[5]], THR, N.PF_SPOT_MAX_HITS + 1), ([[5]], 0.1, 4), ([[5]], float("nan"), 4), ([[5]] * (N.PF_SPOT_MAX_KEYWORDS + 1), THR, 4)]
    for phrases, thr, hits in bad:
        with pytest.raises(N.PfError) as ei:
            eng.set_spotter(phrases, thr, hits)
        assert ei.value.code == (N.PF_ERR_CAPACITY if len(phrases) > N.PF_SPOT_MAX_KEYWORDS else N.PF_ERR_INVALID_ARG), (thr, hits)
    eng.close()
