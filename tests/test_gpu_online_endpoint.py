"""GPU: streaming endpointing and the second pass (OnlineRecognizer.SetEndpoint / SetSecondPass, OnlineStream.InputFinished /
Sentences / InSpeech; csrc/online.cpp, csrc/k_endpoint.hip) on the 3 + 3 layer synthetic streaming model of
tests/test_gpu_online.py and a 2 + 2 layer offline model as in tests/test_gpu_vad_recognizer.py.

Three streams of 8 s burst audio (tests/vad_ref.py burst_audio), two or three bursts each, fed in 4000-sample pieces; stream 2
ends inside a burst and its sample count is no multiple of 160.  Everything about the sentences is compared exactly: they
must be the definition (tests/endpoint_ref.py) applied to the levels (vad_ref.levels) of the rows the engine's own fbank op
returns for each 9600-sample chunk of the caller's audio — the same kernel on the same input as the streaming path — and
every second-pass result must be what a fresh offline recognizer gives plain streams of those sample ranges in the same
batches."""
import ctypes as C

import numpy as np
import pytest

import endpoint_ref as R
import vad_ref as V
from online_lockstep_ref import reset as _reset
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import online as oo

pytestmark = pytest.mark.gpu

VOCAB = 300
STEP = 4000
CHUNK = 9600
BURSTS = [[(100, 250), (400, 600)], [(50, 250), (400, 500), (600, 700)], [(100, 300), (650, 800)]]
KIND = {R.SILENCE: "silence", R.FORCED: "forced", R.FLUSH: "flush"}
YAML = "frontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n"


def _tokens():
    toks = ["<blank>", "<s>", "</s>", "<unk>"]
    cjk = [chr(0x4E00 + 37 * i) for i in range(120)]
    bpe = []
    for i in range(VOCAB - 4 - len(cjk)):
        w = "w%d" % i
        bpe.append(w + "@@" if i % 3 == 0 else ("▁" + w if i % 3 == 1 else w))
    return toks + cjk + bpe


def _write(d, cfg, w, head):
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text(head + YAML)
    (d / "tokens.txt").write_text("\n".join(_tokens()) + "\n", encoding="utf-8")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    on, off = tmp_path_factory.mktemp("ep_online"), tmp_path_factory.mktemp("ep_offline")
    cfg = W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=VOCAB)
    w = W.synth_weights(cfg, seed=31)
    w["predictor.out.bias"] = np.asarray([0.8], np.float32)          # ~0.6 per frame: a few tokens per 10-frame chunk
    _write(on, cfg, w, "model: paraformer\n")
    ocfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB)
    _write(off, ocfg, W.synth_weights(ocfg, seed=77), "model: paraformer\nuse_itn: false\n")
    return on, off, cfg, w


@pytest.fixture(scope="module")
def audio():
    a = [V.burst_audio(8, b, 40 + i) for i, b in enumerate(BURSTS)]
    a[2] = a[2][:127900]                                              # 799.4 frames: the last sentence ends at the sample count
    return a


def _online(models):
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    d = models[0]
    return OnlineRecognizer(str(d / "model.pfw"), "", str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))


def _offline(models):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    d = models[1]
    r = OfflineRecognizer(str(d / "model.pfw"), str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))
    r.SetDecode(scores=True)
    return r


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _levels(rec, a):
    """the levels of the caller's frames: per 9600-sample chunk (the last one zero-padded) the rows of the engine's own fbank op,
    of which the first ceil(samples / 160) are the caller's"""
    lib, h = N.load(), C.c_void_p(rec.engine_handle())
    out = []
    for off in range(0, len(a), CHUNK):
        piece = a[off: off + CHUNK]
        x = np.zeros(CHUNK, np.float32)
        x[: len(piece)] = piece
        rows, t = np.zeros((CHUNK // 160 + 2) * 80, np.float32), C.c_int32()
        N.check(lib.pf_fbank(h, x.ctypes.data_as(C.POINTER(C.c_float)), CHUNK, rows.ctypes.data_as(C.POINTER(C.c_float)), rows.size, t))
        assert t.value == 60
        out.append(V.levels(rows[: 60 * 80].reshape(60, 80)[: (len(piece) + 159) // 160]))
    return np.concatenate(out)


def _feed(rec, streams, audio, finish=True, on_call=None):
    """4000-sample pieces to every stream, a GetResults per round; then InputFinished and the calls that drain the chunks.
    Returns, per call, the number of sentences every stream has after it."""
    counts = []
    for off in range(0, max(len(a) for a in audio), STEP):
        for s, a in zip(streams, audio):
            if off < len(a):
                s.AddSamples(a[off: off + STEP])
        res = rec.GetResults(streams)
        counts.append([len(s.Sentences) for s in streams])
        if on_call:
            on_call(len(counts) - 1, res)
    if finish:
        for s in streams:
            s.InputFinished()
        for _ in range(3):
            rec.GetResults(streams)
            counts.append([len(s.Sentences) for s in streams])
    return counts


@pytest.fixture(scope="module")
def run(models, audio):
    """ONE pass with the endpoint and the second pass on, shared by the tests that only read it"""
    rec, off = _online(models), _offline(models)
    rec.SetEndpoint()
    rec.SetSecondPass(off)
    streams = [rec.CreateOnlineStream() for _ in audio]
    status = {}

    def on_call(k, res):
        if k == 29:                                                   # 120000 samples in: twelve chunks of the caller's, 720 frames
            status["in_speech"] = [s.InSpeech for s in streams]
            status["text"] = [r.Text for r in res]
    counts = _feed(rec, streams, audio, on_call=on_call)
    sentences = [s.Sentences for s in streams]
    yield rec, streams, sentences, counts, status
    rec.Dispose(); off.Dispose()


def test_sentences_equal_the_definition(run, audio):
    rec, streams, sentences, counts, status = run
    c = R.config()
    for i, a in enumerate(audio):
        lev = _levels(rec, a)
        assert len(lev) == (len(a) + 159) // 160 == 800
        want, _ = R.run(lev, 80, c, flush=True)
        got = [(s.begin_ms, s.end_ms, s.kind) for s in sentences[i]]
        assert got == [(10 * b, 10 * e, KIND[k]) for b, e, k in want], i
        # the status in the middle of the stream: after 720 frames
        st = R.new_state()
        _, ins, ob = R.update(st, lev[:720], False, 80, c)
        assert status["in_speech"][i] == (bool(ins), 10 * ob if ins else -1), i
    assert [len(s) for s in sentences] == [2, 3, 2]
    assert status["in_speech"][2][0] and status["in_speech"][1][0] and not status["in_speech"][0][0]
    # the bursts are found where they lie: a burst [f0, f1) gives about [f0 + 14 - pad_begin, f1 + 14 + pad_end) with the default
    # window (a frame or two more where an analysis window straddles the burst's edge)
    for i, sl in enumerate(sentences):
        for s, (f0, f1) in zip(sl, BURSTS[i]):
            assert 10 * (f0 - 20) <= s.begin_ms <= 10 * (f0 - 10), (i, s)
            assert 10 * (f1 + 15) <= s.end_ms <= 10 * (f1 + 25) or s.kind == "flush", (i, s)
    assert counts[-1] == counts[-2] == [2, 3, 2]                       # nothing comes after the flush


def test_input_finished_flushes_the_open_sentence(run, audio):
    rec, streams, sentences, counts, status = run
    last = sentences[2][-1]
    assert last.kind == "flush" and last.end_ms == 8000 and 6300 <= last.begin_ms <= 6400
    assert all(s.kind == "silence" for sl in sentences for s in sl if s is not last)
    assert counts[31] == [2, 2, 1]                                     # before InputFinished: 780 frames in, two sentences still open
    assert [s.InSpeech for s in streams] == [(False, -1)] * 3
    with pytest.raises(N.PfError) as ei:
        streams[2].AddSamples(np.zeros(100, np.float32))
    assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_second_pass_equals_plain_streams_in_the_same_batches(run, models, audio):
    rec, streams, sentences, counts, status = run
    rp = _offline(models)
    prev, n_batches, n_pairs = [0, 0, 0], 0, 0
    for now in counts:
        pool = [(i, j) for i in range(3) for j in range(prev[i], now[i])]        # the call's stream order, then time order
        prev = now
        if not pool:
            continue
        n_batches += 1
        n_pairs += len(pool) > 1
        ps = []
        for i, j in pool:
            s = sentences[i][j]
            b0, e0 = V.sample_range((s.begin_ms // 10, s.end_ms // 10), len(audio[i]))
            p = rp.CreateOfflineStream()
            p.AddSamples(audio[i][b0:e0])
            ps.append(p)
        pres = rp.GetResults(ps)
        for (i, j), p, pr in zip(pool, ps, pres):
            s = sentences[i][j]
            assert s.result is not None
            assert s.result.Tokens == p.Tokens and len(p.Tokens) > 0, (i, j)
            assert s.result.Timestamps == p.Timestamps, (i, j)
            assert _bits(s.result.Scores) == _bits(p.Scores), (i, j)
            assert s.text == pr.Text, (i, j)
            assert isinstance(s.first_pass, str)
    assert n_batches >= 5 and n_pairs >= 1                             # two sentences closed in one call at least once
    rp.Dispose()
    # stream 2's flushed sentence held the caller's samples up to the last one (it was rebuilt above with that range)
    assert V.sample_range((sentences[2][-1].begin_ms // 10, 800), len(audio[2]))[1] == 127900 == len(audio[2])


def test_without_a_second_pass_text_is_the_first_pass(models, audio):
    rec = _online(models)
    rec.SetEndpoint(end_silence=40)
    streams = [rec.CreateOnlineStream() for _ in audio[:2]]
    texts = []
    _feed(rec, streams, [a[:64000] for a in audio[:2]], on_call=lambda k, res: texts.append([r.Text for r in res]))
    n = 0
    for s in streams:
        for sen in s.Sentences:
            assert sen.result is None and sen.text == sen.first_pass
            n += 1
    assert n >= 2 and any(sen.first_pass for s in streams for sen in s.Sentences)
    rec.Dispose()


def test_reset_in_lockstep_with_the_oracle(models, audio):
    """(lengths and four ids in five; the exact comparison with the endpoint on: tests/test_gpu_online_lockstep.py)"""
    on, _, cfg, w = models
    rec = _online(models)
    rec.SetEndpoint(end_silence=40)                                    # sentences close inside the first 4.5 s
    orc = oo.OnlineRecognizer(cfg, w, W.synth_cmvn(), _tokens(), quant="fp16")
    streams = [rec.CreateOnlineStream() for _ in audio]
    ostreams = [orc.create_stream() for _ in audio]
    total = match = closed = 0
    last = [([], [])] * 3
    for off in range(0, 72000, STEP):
        for u in range(3):
            streams[u].AddSamples(audio[u][off: off + STEP])
            ostreams[u].add_samples(audio[u][off: off + STEP])
        before = [len(s.Sentences) for s in streams]
        rec.GetResults(streams)
        orc.get_results(ostreams)
        for u in range(3):
            if len(streams[u].Sentences) > before[u]:                  # a sentence closed in this call: the context is new
                assert streams[u].Tokens == [], (off, u)
                _reset(ostreams[u], cfg["dec_layers"])
                a, b = last[u]
                total += len(a); match += int((np.asarray(a) == np.asarray(b)).sum())
                closed += 1
            assert len(streams[u].Tokens) == len(ostreams[u].tokens), (off, u)
            last[u] = (streams[u].Tokens, list(ostreams[u].tokens))
    for a, b in last:
        total += len(a); match += int((np.asarray(a) == np.asarray(b)).sum())
    assert closed >= 3
    assert total > 20 and match / total > 0.8, (match, total)           # near-ties of a random-weight model may flip a few ids
    rec.Dispose()


def test_set_and_cleared_equals_never_set(models, audio):
    ra, rb = _online(models), _online(models)
    ra.SetEndpoint()
    warm = ra.CreateOnlineStream()
    _feed(ra, [warm], [audio[0][:32000]], finish=False)
    ra.SetEndpoint(False)
    sa, sb = [ra.CreateOnlineStream() for _ in range(2)], [rb.CreateOnlineStream() for _ in range(2)]
    n = 0
    for off in range(0, 48000, STEP):
        for u in range(2):
            sa[u].AddSamples(audio[u][off: off + STEP])
            sb[u].AddSamples(audio[u][off: off + STEP])
        qa, qb = ra.GetResults(sa), rb.GetResults(sb)
        for u in range(2):
            assert sa[u].Tokens == sb[u].Tokens and qa[u].Text == qb[u].Text, (off, u)
            n = max(n, len(sa[u].Tokens))
    assert n > 10 and all(s.Sentences == [] and s.InSpeech == (False, -1) for s in sa + sb)
    ra.Dispose(); rb.Dispose()


def test_refusals(models):
    rec, off = _online(models), _offline(models)
    off.SetVad(True)
    with pytest.raises(N.PfError) as ei:
        rec.SetSecondPass(off)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    off.SetVad(None)
    rec.SetSecondPass(off)
    rec.SetSecondPass(None)
    for bad in (dict(rise=-2), dict(min_speech=11), dict(pad_end=81), dict(max_len=30), dict(window=0)):
        with pytest.raises(N.PfError) as ei:
            rec.SetEndpoint(**bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    s = rec.CreateOnlineStream()
    s.AddSamples(np.zeros(5000, np.float32))
    s.InputFinished()
    with pytest.raises(N.PfError) as ei:
        s.AddSamples(np.zeros(10, np.float32))
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    rec.GetResults([s])
    assert s.Sentences == []
    rec.Dispose(); off.Dispose()
