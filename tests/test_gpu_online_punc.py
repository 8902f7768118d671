"""GPU: OnlineRecognizer.SetPuncModel — streaming punctuation through the recogniser, on the synthetic online
model of the other test_gpu_online_* files and a causal CT-Transformer of vocabulary 64.

  * Text / Tokens / TokenInfo are identical with the model attached, without it and after detaching.
  * after every GetResults the stream's committed words are the definition's (tests/punc_stream_ref.py committed_words over the
    stream's own token strings), Punctuated is the definition's assembly, and at the end PuncIds equal ONE pf_op_punc_stream_step
    over the same words — exactly, by the chunking property.
  * two interleaved streams equal each stream alone; with SetEndpoint a closed sentence carries its punctuated text and the next
    sentence starts a fresh context; InputFinished flushes; a GetResults with nothing new launches nothing.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import online_lockstep_ref as LR
import punc_ref as R
import punc_stream_ref as S
import vad_ref as V
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe

pytestmark = pytest.mark.gpu
YAML = ("model: paraformer\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n"
        "  snip_edges: false\n")
STEP = 4000
NONE = 1


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    d = tmp_path_factory.mktemp("onlinepunc")
    cfg, w = LR.model()
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text(YAML)
    (d / "tokens.txt").write_text("\n".join(LR.tokens()) + "\n", encoding="utf-8")
    pcfg = W.ct_transformer_config(vocab=64, n_layers=2)
    pw = W.synth_punc_weights(pcfg, seed=42)
    pcfg = S.causal_config(pcfg)
    (d / "punc.pfw").write_bytes(W.pack_pfw(pcfg, pw))
    (d / "offline_punc.pfw").write_bytes(W.pack_pfw(W.ct_transformer_config(vocab=64, n_layers=2), pw))
    m = E.load_punc_model(str(d / "punc.pfw"))
    ecfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = E.Engine(weights=W.pack_pfw(ecfg, W.synth_weights(ecfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    eng.set_punc_model(m)
    yield d, pcfg, m, eng
    eng.set_punc_model(None)
    eng.close()
    m.close()


def _rec(d, punc=True, token_info=False, max_context=0):
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    rec = OnlineRecognizer(str(d / "model.pfw"), "", str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))
    if token_info:
        rec.SetTokenInfo(True)
    if punc:
        rec.SetPuncModel(str(d / "punc.pfw"), max_context)
    return rec


def _feed(rec, streams, audio, finish=True, on_call=None):
    """4000-sample pieces to every stream, a GetResults per round; then InputFinished and three calls that drain the chunks"""
    calls = 0
    for off in range(0, max(len(a) for a in audio), STEP):
        for s, a in zip(streams, audio):
            if off < len(a):
                s.AddSamples(a[off: off + STEP])
        res = rec.GetResults(streams)
        if on_call:
            on_call(calls, res)
        calls += 1
    if finish:
        for s in streams:
            s.InputFinished()
        for _ in range(3):
            res = rec.GetResults(streams)
            if on_call:
                on_call(calls, res)
            calls += 1
    return calls


def _snapshot(s, text):
    return (text, tuple(s.Tokens), tuple((t.id, t.time_ms, t.entry, t.score_bits, t.flags) for t in s.TokenInfo))


def _op_marks(eng, m, pcfg, words, flush, max_context=S.DEFAULT_CONTEXT):
    """ONE pf_op_punc_stream_step over the words of one context history: the marks with the flush's edit applied, and the flags"""
    ids = R.word_ids(words, W.synth_punc_vocab(64))
    st = E.punc_stream_state(m, B=1)
    res, _, fm = eng.op_punc_stream_step(st, [ids], flush=[flush], max_context=max_context, want_logits=False)
    marks = res[0][0].tolist()
    if flush and fm[0] >= 0 and marks:
        marks[-1] = int(fm[0])
    return marks, res[0][1].tolist()


def _launches(lib, h):
    ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
    N.check(lib.pf_profile_get(h, b"punc_stream", C.byref(ms), C.byref(n), C.byref(fpl)))
    return n.value


@pytest.mark.parametrize("token_info", [False, True])
def test_text_tokens_and_token_info_do_not_change(rig, token_info):
    d, pcfg, m, eng = rig
    audio = [LR._audio(u) for u in range(2)]
    plain, punc = _rec(d, False, token_info), _rec(d, True, token_info)
    sp, sq = [plain.CreateOnlineStream() for _ in audio], [punc.CreateOnlineStream() for _ in audio]
    want = []
    _feed(plain, sp, audio, on_call=lambda k, res: want.append([_snapshot(s, r.Text) for s, r in zip(sp, res)]))
    got = []
    _feed(punc, sq, audio, on_call=lambda k, res: got.append([_snapshot(s, r.Text) for s, r in zip(sq, res)]))
    assert got == want and any(s.PuncIds for s in sq) and all(not s.PuncIds and s.Punctuated == "" for s in sp)
    # detaching is refused while a stream holds punctuation state, and works once they are gone; then nothing is left of it
    with pytest.raises(Exception) as ei:
        punc.SetPuncModel(None)
    assert getattr(ei.value, "code", None) == N.PF_ERR_UNSUPPORTED
    del sq
    gc.collect()
    punc.SetPuncModel(None)
    sq = [punc.CreateOnlineStream() for _ in audio]
    got = []
    _feed(punc, sq, audio, on_call=lambda k, res: got.append([_snapshot(s, r.Text) for s, r in zip(sq, res)]))
    assert got == want and all(not s.PuncIds and s.Punctuated == "" for s in sq)
    # a model that is not causal is refused
    with pytest.raises(Exception) as ei:
        punc.SetPuncModel(str(d / "offline_punc.pfw"))
    assert getattr(ei.value, "code", None) == N.PF_ERR_UNSUPPORTED
    with pytest.raises(Exception) as ei:
        punc.SetPuncModel(str(d / "punc.pfw"), 1)
    assert getattr(ei.value, "code", None) == N.PF_ERR_INVALID_ARG
    plain.Dispose()
    punc.Dispose()


@pytest.mark.parametrize("max_context", [0, 5])
def test_marks_equal_one_op_call_and_the_text_is_the_definitions(rig, max_context):
    d, pcfg, m, eng = rig
    toks = LR.tokens()
    audio = [LR._audio(u) for u in range(2)]
    mc = max_context or S.DEFAULT_CONTEXT
    rec = _rec(d, True, max_context=max_context)
    streams = [rec.CreateOnlineStream() for _ in audio]
    lib, h = N.load(), C.c_void_p(rec.engine_handle())
    launches = []
    history = [[] for _ in streams]

    def on_call(k, res):
        launches.append(_launches(lib, h))
        for u, (s, r) in enumerate(zip(streams, res)):
            words, held = S.committed_words([toks[i] for i in s.Tokens])
            ids = s.PuncIds
            assert S.online_decode_text([toks[i] for i in s.Tokens]) == r.Text
            if len(ids) == len(words) + 1:                       # the end-of-input flush took the held-back word too
                assert held is not None and k >= first_flush[0]
                words, held = words + [held], None
            assert len(ids) == len(words) == len(s.PuncFlags), (k, u)
            assert s.Punctuated == R.assemble(words + ([held] if held else []), ids + [NONE] * (held is not None), pcfg["punc_list"])[0], (k, u)
            prev = history[u][-1] if history[u] else []
            assert len(ids) >= len(prev) and ids[: max(len(prev) - 1, 0)] == prev[: max(len(prev) - 1, 0)]   # never revised (the flush edits the newest)
            history[u].append(ids)
    first_flush = [len(range(0, len(audio[0]), STEP))]
    N.check(lib.pf_profile_enable(h, 1))
    N.check(lib.pf_profile_reset(h))
    _feed(rec, streams, audio, on_call=on_call)
    # one launch per call at the most, and none in a call that brought no word and no flush (the last drain calls)
    steps = np.diff([0] + launches)
    assert set(steps.tolist()) <= {0, 1} and steps.sum() >= 3
    for u, s in enumerate(streams):
        words = R.split_words(S.online_decode_text([toks[i] for i in s.Tokens]))
        assert len(words) >= 8
        marks, flags = _op_marks(eng, m, pcfg, words, True, mc)
        assert s.PuncIds == marks and s.PuncFlags == flags, u
        if max_context == 5:
            assert 2 in flags or 1 in flags
    # nothing new: no launch, nothing changes
    before = [(s.Punctuated, s.PuncIds) for s in streams]
    rec.GetResults(streams)
    assert _launches(lib, h) == launches[-1] and [(s.Punctuated, s.PuncIds) for s in streams] == before
    N.check(lib.pf_profile_enable(h, 0))
    rec.Dispose()


def test_two_interleaved_streams_equal_each_alone(rig):
    d, pcfg, m, eng = rig
    audio = [LR._audio(u) for u in range(2)]
    alone = []
    for a in audio:
        rec = _rec(d)
        s = rec.CreateOnlineStream()
        _feed(rec, [s], [a])
        alone.append((s.Punctuated, s.PuncIds, s.PuncFlags, s.Tokens))
        rec.Dispose()
    rec = _rec(d)
    streams = [rec.CreateOnlineStream() for _ in audio]
    # interleaved: the streams take turns, one GetResults per stream and piece, then both finish together
    for off in range(0, len(audio[0]), STEP):
        for s, a in zip(streams, audio):
            s.AddSamples(a[off: off + STEP])
            rec.GetResults([s])
    for s in streams:
        s.InputFinished()
    for _ in range(3):
        rec.GetResults(streams[::-1])
    for s, want in zip(streams, alone):
        if s.Tokens == want[3]:                                   # (the decoder pads a batch to its longest member: the ids may differ)
            assert (s.Punctuated, s.PuncIds, s.PuncFlags) == want[:3]
    together = _rec(d)
    st = [together.CreateOnlineStream() for _ in audio]
    _feed(together, st, audio)
    for s, t in zip(streams, st):
        if s.Tokens == t.Tokens:
            assert (s.Punctuated, s.PuncIds, s.PuncFlags) == (t.Punctuated, t.PuncIds, t.PuncFlags)
    # whatever the ids, every stream's marks are those of ONE op call over its own words
    toks = LR.tokens()
    for s in streams + st:
        words = R.split_words(S.online_decode_text([toks[i] for i in s.Tokens]))
        assert (s.PuncIds, s.PuncFlags) == _op_marks(eng, m, pcfg, words, True)
    rec.Dispose()
    together.Dispose()


def test_a_closed_sentence_is_flushed_and_the_next_starts_fresh(rig):
    d, pcfg, m, eng = rig
    audio = [V.burst_audio(LR.SECONDS, list(b), 40 + i) for i, b in enumerate(LR.ENDPOINT_BURSTS[:2])]
    plain, rec = _rec(d, False), _rec(d)
    for r in (plain, rec):
        r.SetEndpoint(**LR.ENDPOINT_KEYS)
    sp, streams = [plain.CreateOnlineStream() for _ in audio], [rec.CreateOnlineStream() for _ in audio]
    _feed(plain, sp, audio)
    _feed(rec, streams, audio)
    closed = 0
    for s, p in zip(streams, sp):
        sens, want = s.Sentences, p.Sentences
        assert [(x.begin_ms, x.end_ms, x.kind, x.first_pass, x.text) for x in sens] == [(x.begin_ms, x.end_ms, x.kind, x.first_pass, x.text) for x in want]
        assert all(x.punctuated == "" and x.punc_ids == [] for x in want)
        for x in sens:
            words = R.split_words(x.first_pass)
            marks, _ = _op_marks(eng, m, pcfg, words, True)        # a fresh context per sentence, the held-back word included, the flush
            assert x.punc_ids == marks and x.punctuated == R.assemble(words, marks, pcfg["punc_list"])[0]
            closed += bool(words)
        words = R.split_words(S.online_decode_text([LR.tokens()[i] for i in s.Tokens]))
        assert (s.PuncIds, s.PuncFlags) == _op_marks(eng, m, pcfg, words, True)
    assert closed >= 2
    plain.Dispose()
    rec.Dispose()


def test_puncstream_option(rig, tmp_path):
    from aliparaformerasr_amd.examples import parse_args
    base = ["-type", "online", "-files", "a.wav"]
    assert parse_args(base + ["-puncstream", "p.pfw"])["puncstream"] == {"file": "p.pfw", "max_context": 0}
    assert parse_args(base + ["-puncstream", "p.pfw,max_context=50"])["puncstream"] == {"file": "p.pfw", "max_context": 50}
    for bad in (["-puncstream"], ["-puncstream", "p.pfw,max_context=1"], ["-puncstream", "p.pfw,window=3"], ["-puncstream", "p.pfw,max_context=x"]):
        with pytest.raises(ValueError):
            parse_args(base + bad)
    with pytest.raises(ValueError):
        parse_args(["-type", "offline", "-files", "a.wav", "-puncstream", "p.pfw"])
