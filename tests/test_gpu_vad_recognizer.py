"""GPU: long-audio recognition (OfflineRecognizer.SetVad) — every planned batch rebuilt from stream.Segments with plain streams
on a second recognizer, in plan order: each segment's ids, text, timestamps and scores must be identical, and the stitched
result must follow the rule of include/paraformer_hip.h (texts joined, tokens concatenated, times on the stream's clock).
A paraformer model (the 2 + 2 layer synthetic one) with scores, and a SenseVoice model with PF_DECODE_CTC."""
import numpy as np
import pytest

import vad_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe

pytestmark = pytest.mark.gpu
VOCAB = 300
CFG = dict(max_len=300, split_search=100, min_speech=50)
SEP = " | "


def _tokens(kind):
    if kind == "sensevoice":
        return ["<blank>", "<s>", "</s>", "<unk>"] + ["<|tag%d|>" % i for i in range(20)] + [chr(0x4E00 + i) for i in range(VOCAB - 24)]
    return ["<blank>", "<s>", "</s>", "<unk>"] + [chr(0x4E00 + 37 * i) for i in range(120)] + ["w%d" % i for i in range(VOCAB - 124)]


@pytest.fixture(scope="module", params=["paraformer", "sensevoice"])
def model(request, tmp_path_factory, sv_embed):
    kind = request.param
    d = tmp_path_factory.mktemp("vad_" + kind)
    if kind == "paraformer":
        cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB)
        w = W.synth_weights(cfg, seed=77)
        head = "model: paraformer\nuse_itn: false\n"
    else:
        cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=VOCAB)
        w = W.synth_weights(cfg, seed=9)
        w["embed.weight"] = sv_embed.astype(np.float32)
        b = np.array(w["ctc.bias"], np.float32)
        b[8:] -= 30                                               # a CTC head that emits blanks and repeats
        b[0] += 1.0
        w["ctc.bias"] = b
        head = "model: SenseVoiceSmall\nuse_itn: true\n"
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text(head + "frontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n  lfr_m: 7\n"
                                       "  lfr_n: 6\n  snip_edges: false\n")
    (d / "tokens.txt").write_text("\n".join(_tokens(kind)) + "\n", encoding="utf-8")
    return kind, [str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]


def _rec(model):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    kind, paths = model
    r = OfflineRecognizer(*paths)
    r.SetDecode(ctc=True) if kind == "sensevoice" else r.SetDecode(scores=True)
    return r


def _streams(r, audio):
    out = []
    for a in audio:
        s = r.CreateOfflineStream()
        s.AddSamples(a)
        out.append(s)
    return out


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def test_segments_forward_and_stitching(model):
    audio = [R.burst_audio(20, [(200, 500), (800, 1000), (1400, 1800)], 1), R.burst_audio(7, [(100, 400)], 2),
             (0.001 * np.random.default_rng(3).standard_normal(48000)).astype(np.float32)]
    rv, rp = _rec(model), _rec(model)
    rv.SetVad(CFG, batch_max=4, sep=SEP)
    sv = _streams(rv, audio)
    res = rv.GetResults(sv)
    segs = [s.Segments for s in sv]
    # the cut: ascending, inside the configured lengths, every burst covered; the 400-frame burst is split
    assert len(segs[0]) >= 4 and len(segs[1]) >= 2 and segs[2] == []
    for i, sl in enumerate(segs):
        prev = 0
        for g in sl:
            assert g.BeginMs % 10 == 0 and g.EndMs % 10 == 0 and prev <= g.BeginMs < g.EndMs <= 10 * ((len(audio[i]) + 80) // 160)
            assert 50 <= (g.EndMs - g.BeginMs) // 10 <= 300
            prev = g.EndMs
    # the plan: pooled in stream order, then time order
    pool = [(i, g) for i, sl in enumerate(segs) for g in sl]
    place, nb = R.long_plan([(g.EndMs - g.BeginMs) // 10 for _, g in pool], 4, 96000)
    assert [(g.Batch, g.Row) for _, g in pool] == place and nb >= 2
    # every batch again with plain streams holding the sample ranges, in plan order
    texts = {}
    for k in range(nb):
        rows = sorted((g.Row, i, g) for i, g in pool if g.Batch == k)
        cut = []
        for _row, i, g in rows:
            b0, e0 = R.sample_range((g.BeginMs // 10, g.EndMs // 10), len(audio[i]))
            cut.append(audio[i][b0:e0])
        ps = _streams(rp, cut)
        pres = rp.GetResults(ps)
        for (_row, i, g), p, pr in zip(rows, ps, pres):
            own = sv[i]
            assert own.Tokens[g.TokBegin:g.TokEnd] == p.Tokens, (k, g)
            assert _bits(own.Scores[g.TokBegin:g.TokEnd]) == _bits(p.Scores), (k, g)
            assert own.Timestamps[g.TokBegin:g.TokEnd] == [[x + g.BeginMs for x in t] for t in p.Timestamps], (k, g)
            assert g.Text == pr.Text, (k, g)
            texts[(i, g.BeginMs)] = pr
    # the stitched results
    for i, sl in enumerate(segs):
        parts = [texts[(i, g.BeginMs)] for g in sl]
        assert res[i].Text == SEP.join(p.Text for p in parts)
        assert res[i].TextLen == len(res[i].Text.encode("utf-16-le")) // 2
        assert res[i].Tokens == [t for p in parts for t in p.Tokens]
        assert res[i].Timestamps == [[x + g.BeginMs for x in t] for g, p in zip(sl, parts) for t in p.Timestamps]
        assert len(sv[i].Tokens) == (sl[-1].TokEnd if sl else 0) and len(sv[i].Scores) == len(sv[i].Tokens)
    assert (res[2].Text, res[2].Tokens, res[2].Timestamps, sv[2].Tokens, sv[2].Timestamps) == ("", [], [], [], [])
    assert any(len(sv[i].Tokens) > 0 for i in range(2))


def test_off_again_equals_never_set(model):
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    ra, rb = _rec(model), _rec(model)
    ra.SetVad(True)
    ra.GetResults(_streams(ra, [R.burst_audio(3, [(50, 200)], 4)]))
    ra.SetVad(None)
    sa, sb = _streams(ra, audio), _streams(rb, audio)
    qa, qb = ra.GetResults(sa), rb.GetResults(sb)
    for x, y, p, q in zip(sa, sb, qa, qb):
        assert (x.Tokens, x.Timestamps, _bits(x.Scores), x.Segments) == (y.Tokens, y.Timestamps, _bits(y.Scores), [])
        assert (p.Text, p.Tokens, p.Timestamps) == (q.Text, q.Tokens, q.Timestamps)


def test_refusals(model):
    from aliparaformerasr_amd.offline_recognizer import RecognizerException
    kind, _ = model
    r = _rec(model)
    r.SetVad(True)
    setters = [lambda q: q.SetNBest(1)]
    if kind == "sensevoice":
        setters += [lambda q: q.SetCtcBeam(4), lambda q: q.SetAlign(True)]
    for f in setters:
        with pytest.raises(N.PfError) as ei:                       # set second ...
            f(r)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
        q = _rec(model)
        f(q)
        with pytest.raises(N.PfError) as ei:                       # ... or first
            q.SetVad(True)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    for bad in (dict(window=0), dict(min_speech=11), dict(max_len=599)):
        with pytest.raises(N.PfError) as ei:
            r.SetVad(bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    # a stream that holds features only: the call fails inside Forward's try block
    s = r.CreateOfflineStream()
    s.AddSamples(W.synth_audio(16000, 1))
    s.AddSamples(W.synth_audio(16000, 2))
    with pytest.raises(RecognizerException, match="Offline recognition failed.*features"):
        r.GetResults([s])
    r.SetNBest(0)                                                  # turning the others off stays allowed
