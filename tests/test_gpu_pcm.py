"""GPU: PCM intake on the device (csrc/k_pcm.hip; Engine.op_pcm_convert / stage_pcm / recognize_pcm, OfflineStream.AddPcm,
`examples.py -intake device`) — the kernel against oracle.audio bit for bit, the same answers through the engine as the
float entry points give for the converted samples, the recognizer's device and host forms, two callers, and the CLI."""
import io
import threading

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import glue
from pcm_ref import FORMATS, RATES, bits_equal, expected, payload, wav_blob

pytestmark = pytest.mark.gpu
VOCAB = 300
CTC = N.PF_DECODE_CTC


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _i16(x):
    """float samples -> the 16-bit PCM a recorder would have stored, and the floats that PCM decodes to"""
    p = np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype("<i2")
    return p, (p.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


# ---- 1: the kernel against the oracle, bit for bit ------------------------------------------------------------------
def _check(eng, fmt, sr, ch, flag, n, seed=0, nan=False):
    data = payload(fmt, n, seed=seed, nan=nan)
    got = eng.op_pcm_convert(data, N.pcm_desc(sr, ch, fmt, flag))
    want = expected(data, sr, ch, fmt, flag)
    assert eng.pcm_num_samples(N.pcm_desc(sr, ch, fmt, flag), n) == want.size == got.size, (fmt, sr, ch, flag, n)
    if not bits_equal(got, want):
        bad = np.flatnonzero(_bits(got) != _bits(want))
        raise AssertionError("%s %d Hz %d ch flag=%d n=%d: %d of %d samples differ, first at %d: got %r want %r" %
                             (fmt, sr, ch, flag, n, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]]))


def test_kernel_equals_the_oracle_every_format_rate_channels_flag(any_engine):
    """No tolerance: every operation is an IEEE one with a single correct rounding — a mismatch means a contracted
    multiply-add or another operation order.  Short lengths: empty, below one quad, around one 400-sample frame, odd counts
    (for stereo: an unpaired trailing value)."""
    for fmt in FORMATS:
        for sr in RATES:
            for ch in (1, 2):
                for flag in (False, True):
                    for n in (0, 1, 2, 3, 399, 401, 1001, 1003):
                        _check(any_engine, fmt, sr, ch, flag, n, seed=sr // 25 + ch)


def test_kernel_equals_the_oracle_thirty_seconds(any_engine):
    """30 s of input: every grid-stride round, int indices up to 2.88 M values, float64 positions far from the origin.  Every
    rate x channel count as s16, and every format at a rate / channel count / flag that rotates with it."""
    for k, sr in enumerate(RATES):
        for ch in (1, 2):
            _check(any_engine, "s16", sr, ch, bool(k & 1), 30 * sr * ch + (ch - 1), seed=7)      # stereo: an unpaired value too
    for k, fmt in enumerate(FORMATS):
        sr, ch = RATES[(3 * k + 1) % len(RATES)], 1 + (k + 1) % 2
        _check(any_engine, fmt, sr, ch, bool(k & 2), 30 * sr * ch, seed=9)


def test_float32_nan_payloads_are_copied_at_the_native_rate(any_engine):
    """NaN payloads are not compared through the interpolation or the down-mix (x86 and the GPU may propagate them
    differently); the native-rate float32 path is a bit copy and must keep them, signalling ones and infinities included."""
    for ch in (1, 2):
        for n in (1, 5, 4003, 480000):
            _check(any_engine, "f32", 16000, ch, False, n, seed=3, nan=True)


def test_batch_table_mixed_formats_in_one_launch(any_engine):
    """stage_pcm's one launch over a table of different formats / rates equals the per-utterance conversions (read back through
    the front-end: equal samples give equal features)."""
    eng = any_engine
    specs = [("s16", 48000, 2, 96001), ("mulaw", 8000, 1, 8000), ("s24", 44100, 2, 88200), ("f64", 16000, 1, 16000),
             ("u8", 11025, 1, 11025), ("f32", 16000, 2, 32000)]
    datas = [payload(f, n, seed=21 + i) for i, (f, _sr, _ch, n) in enumerate(specs)]
    descs = [N.pcm_desc(sr, ch, f) for f, sr, ch, _n in specs]
    a = eng.recognize_pcm(datas, descs)
    b = eng.recognize([expected(d, sr, ch, f) for d, (f, sr, ch, _n) in zip(datas, specs)])
    np.testing.assert_array_equal(a.token_ids, b.token_ids)
    np.testing.assert_array_equal(a.token_num, b.token_num)


# ---- 2 / 3: the same answer through the engine ------------------------------------------------------------------------
def _same_result(a, b, what, logits_stable=True):
    np.testing.assert_array_equal(a.token_ids, b.token_ids, err_msg=what)
    np.testing.assert_array_equal(a.token_num, b.token_num, err_msg=what)
    if a.cif_peak is not None or b.cif_peak is not None:
        np.testing.assert_array_equal(_bits(a.cif_peak), _bits(b.cif_peak), err_msg=what)
    if logits_stable and a.logits is not None and b.logits is not None:
        np.testing.assert_array_equal(_bits(a.logits), _bits(b.logits), err_msg=what)


def _engine_case(cfg, w, mode, hotwords=None, decode=0, dither=0.0):
    """recognize_pcm and stage_pcm + run_staged + fetch against recognize of x_i16 / 32768.0f, on ONE engine."""
    from aliparaformerasr_amd.engine import Engine
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0, math_mode=mode, dither=dither, dither_seed=5)
    if decode:
        eng.set_decode(decode)
    pcm, flt = zip(*[_i16(W.synth_audio(n, 500 + u)) for u, n in enumerate((48000, 20000, 33000))])
    desc = N.pcm_desc(16000, 1, "s16")
    f1 = eng.recognize(list(flt), want_logits=True, hotwords=hotwords)
    f2 = eng.recognize(list(flt), want_logits=True, hotwords=hotwords)
    stable = dither == 0.0 and bool(np.array_equal(_bits(f1.logits), _bits(f2.logits)))
    print("math_mode %d kind %d: float path run-to-run logits bit-stable: %s" % (mode, eng.kind, stable))
    if dither == 0.0:
        _same_result(f1, f2, "float path twice", stable)
    p = eng.recognize_pcm(list(pcm), desc, want_logits=True, hotwords=hotwords)
    if dither == 0.0:
        _same_result(p, f1, "recognize_pcm vs recognize", stable)
        if decode & CTC:
            for x, y in ((p.ctc.n, f1.ctc.n), (p.ctc.ids, f1.ctc.ids), (p.ctc.first, f1.ctc.first), (p.ctc.last, f1.ctc.last)):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(_bits(p.ctc.score), _bits(f1.ctc.score))
        if hotwords is not None:
            eng.set_hotwords(hotwords)
        eng.stage_pcm(list(pcm), [desc] * 3)                 # one desc per utterance this time
        eng.run_staged()
        s = eng.fetch()
        _same_result(s, f1, "stage_pcm + run_staged + fetch vs recognize")
    eng.close()
    return p, f1


def test_engine_paraformer_pcm_equals_float():
    """s16 16 kHz mono: the int16 -> float round trip is exact, so ids, token_num and cif_peak must be equal, and the logits bit
    for bit wherever the float path itself repeats them bit for bit (it is run twice first; where it does not, only ids /
    token_num / cif_peak are asserted and the line printed above says so).  Default math mode and the int8 one."""
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB, timestamp_head=True)
    w = W.synth_weights(cfg, seed=31)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    for mode in (0, 2):
        p, f = _engine_case(cfg, w, mode)
        assert p.L > 1 and p.cif_peak is not None


def test_engine_dither_counters_follow_the_converted_length():
    """dither 1.0: the device draws noise from per-sample counters; a fresh engine with the same seed fed PCM must replay the
    features — and so the logits — of one fed the floats."""
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=1, vocab=VOCAB)
    blob = W.pack_pfw(cfg, W.synth_weights(cfg, seed=32))
    pcm, flt = _i16(W.synth_audio(40000, 77))
    outs = []
    for use_pcm in (False, True):
        eng = Engine(weights=blob, cmvn=W.synth_cmvn(), device=0, dither=1.0, dither_seed=5)
        outs.append(eng.recognize_pcm([pcm], N.pcm_desc(16000, 1, "s16"), want_logits=True) if use_pcm
                    else eng.recognize([flt], want_logits=True))
        eng.close()
    np.testing.assert_array_equal(outs[0].token_ids, outs[1].token_ids)
    np.testing.assert_array_equal(_bits(outs[0].logits), _bits(outs[1].logits))


def test_engine_sensevoice_ctc_lengths_come_from_n_out(sv_embed):
    """PF_DECODE_CTC stops each utterance at n_b = 4 + frames(n_out): tokens, frames and scores equal the float path's."""
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=403)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)
    b[8:] -= 30
    w["ctc.bias"] = b
    p, _f = _engine_case(cfg, w, 0, decode=CTC)
    assert p.ctc is not None and p.ctc.n.max() > 0


def test_engine_seaco_hotwords():
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    w = W.synth_weights(cfg, 21)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    w["seaco.output.bias"][111] += 2.6
    hw = np.asarray(glue.pad_list([[5, 6, 7], [9, 10], [1]]), np.int32)
    _engine_case(cfg, w, 0, hotwords=hw)


def test_engine_resampled_formats_equal_float_of_the_oracle_samples(any_engine):
    """44.1 kHz stereo s24 and 8 kHz mu-law through recognize_pcm equal recognize of the oracle-converted samples."""
    eng = any_engine
    x = W.synth_audio(2 * 44100, 61)
    t = np.arange(x.size)
    st = np.stack([x, 0.5 * x + 0.1 * np.sin(t / 37.0).astype(np.float32)], 1).reshape(-1)
    v24 = np.clip(np.round(st.astype(np.float64) * 8388608.0), -(1 << 23), (1 << 23) - 1).astype(np.int64)
    s24 = b"".join(int(v).to_bytes(4, "little", signed=True)[:3] for v in v24)
    mu = payload("mulaw", 24000, seed=4)
    for data, sr, ch, fmt in ((s24, 44100, 2, "s24"), (mu, 8000, 1, "mulaw")):
        want = expected(data, sr, ch, fmt)
        a = eng.recognize_pcm([data], N.pcm_desc(sr, ch, fmt), want_logits=True)
        b = eng.recognize([want], want_logits=True)
        f2 = eng.recognize([want], want_logits=True)
        _same_result(a, b, fmt, bool(np.array_equal(_bits(b.logits), _bits(f2.logits))))
        assert a.L > 0


# ---- 4 / 5: the recognizer --------------------------------------------------------------------------------------------
def _tokens():
    toks = ["<blank>", "<s>", "</s>", "<unk>"]
    cjk = [chr(0x4E00 + 37 * i) for i in range(120)]
    bpe = []
    for i in range(VOCAB - 4 - len(cjk)):
        wd = "w%d" % i
        bpe.append(wd + "@@" if i % 3 == 0 else ("▁" + wd if i % 3 == 1 else wd))
    return toks + cjk + bpe


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("pcm_model")
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB, timestamp_head=True)
    w = W.synth_weights(cfg, seed=78)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text("model: paraformer\nuse_itn: false\nfrontend_conf:\n  fs: 16000\n  window: hamming\n"
                                "  n_mels: 80\n  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n")
    (d / "tokens.txt").write_text("\n".join(_tokens()) + "\n", encoding="utf-8")
    return d


def _make(d):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    return OfflineRecognizer(modelFilePath=str(d / "model.pfw"), configFilePath=str(d / "asr.yaml"),
                             mvnFilePath=str(d / "am.mvn"), tokensFilePath=str(d / "tokens.txt"))


def _clips():
    """(data, sample_rate, channels, format) of a batch in mixed forms, with the oracle's samples for each"""
    out = []
    p16, _ = _i16(W.synth_audio(480000, 90))
    out.append((p16, 16000, 1, "s16"))                                                    # 30 s, a numpy array
    x48 = W.synth_audio(3 * 48000, 91)
    out.append((_i16(np.stack([x48, -0.25 * x48], 1).reshape(-1))[0].tobytes() + b"\x01\x02", 48000, 2, "s16"))   # an unpaired value
    out.append((payload("mulaw", 20000, seed=92), 8000, 1, "mulaw"))
    out.append((_i16(W.synth_audio(2 * 40000, 93))[0], 16000, 2, "s16"))                    # the quirk: stays interleaved
    out.append((W.synth_audio(44100, 94).astype("<f4"), 44100, 1, "f32"))
    out.append((payload("s24", 2 * 22050, seed=95), 22050, 2, "s24"))
    want = [expected(d.tobytes() if isinstance(d, np.ndarray) else d, sr, ch, f) for d, sr, ch, f in out]
    return out, want


def _entities(rec, streams):
    res = rec.GetResults(streams)
    return [(r.Text, r.Tokens, r.Timestamps) for r in res], [list(s.Tokens) for s in streams]


def _pcm_streams(rec, clips):
    ss = []
    for d, sr, ch, f in clips:
        s = rec.CreateOfflineStream()
        s.AddPcm(d, sr, ch, f)
        ss.append(s)
    return ss


def _float_streams(rec, want):
    ss = []
    for x in want:
        s = rec.CreateOfflineStream()
        s.AddSamples(x)
        ss.append(s)
    return ss


def test_recognizer_add_pcm_equals_add_samples_of_the_oracle_samples(model_dir, monkeypatch):
    """Text, Tokens, Timestamps and SpeechLength — in the device form (default), with PF_RECOGNIZER_DEVICE_STREAMS=0, and with the
    staged and the pageable upload (the switches of test_staged_upload_equals_the_synchronous_one)."""
    clips, want = _clips()
    monkeypatch.setenv("PF_RECOGNIZER_STAGING_MB", "0")
    r0 = _make(model_dir)
    fs = _float_streams(r0, want)
    len0 = [s.SpeechLength for s in fs]
    ent0, ids0 = _entities(r0, fs)
    assert all(len(t) > 2 for t in ids0) and len(set(len0)) > 1
    settings = [dict(PF_RECOGNIZER_STAGING_MB="0"), dict(PF_RECOGNIZER_DEVICE_STREAMS="0"),
                dict(PF_RECOGNIZER_STAGING_MB="16", PF_RECOGNIZER_STAGING_PIECE_KB="2048", PF_RECOGNIZER_STAGING_POLICY="always"),
                dict(PF_RECOGNIZER_STAGING_MB="1", PF_RECOGNIZER_STAGING_PIECE_KB="256", PF_RECOGNIZER_STAGING_POLICY="always"),
                dict(PF_RECOGNIZER_STAGING_MB="16", PF_RECOGNIZER_STAGING_PIECE_KB="1024", PF_RECOGNIZER_STAGING_POLICY="auto")]
    for env in settings:
        for k in ("PF_RECOGNIZER_STAGING_MB", "PF_RECOGNIZER_DEVICE_STREAMS", "PF_RECOGNIZER_STAGING_PIECE_KB", "PF_RECOGNIZER_STAGING_POLICY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = _make(model_dir)
        for rep in range(2):
            for d, sr, ch, f in clips[:3]:                       # dropped with their upload and kernel still in flight
                r.CreateOfflineStream().AddPcm(d, sr, ch, f)
            ss = _pcm_streams(r, clips)
            assert [s.SpeechLength for s in ss] == len0, env
            ent, ids = _entities(r, ss)
            assert ids == ids0 and ent == ent0, env
        r.Dispose()
    r0.Dispose()


def test_recognizer_second_add_pcm_appends_features(model_dir):
    """A second AddPcm appends FEATURES like a second AddSamples (OfflineStream.cs:43-54), whichever call came first."""
    clips, want = _clips()
    r = _make(model_dir)
    (d1, sr1, ch1, f1), (d2, sr2, ch2, f2) = clips[1], clips[2]
    a = r.CreateOfflineStream(); a.AddPcm(d1, sr1, ch1, f1); a.AddPcm(d2, sr2, ch2, f2)
    b = r.CreateOfflineStream(); b.AddSamples(want[1]); b.AddSamples(want[2])
    c = r.CreateOfflineStream(); c.AddSamples(want[1]); c.AddPcm(d2, sr2, ch2, f2)
    assert a.SpeechLength == b.SpeechLength == c.SpeechLength > 0
    ents = [_entities(r, [s]) for s in (a, b, c)]
    assert ents[0] == ents[1] == ents[2] and len(ents[0][1][0]) > 2
    r.Dispose()


def test_recognizer_adopts_a_public_constructor_stream_fed_pcm(model_dir):
    from aliparaformerasr_amd.offline_recognizer import ConfEntity, FrontendConfEntity, OfflineStream
    clips, want = _clips()
    r = _make(model_dir)
    conf = ConfEntity(FrontendConfEntity(dither=0.0))
    mine, refs = [], []
    for (d, sr, ch, f), x in list(zip(clips, want))[1:4]:
        s = OfflineStream(str(model_dir / "am.mvn"), conf)
        s.AddPcm(d, sr, ch, f)
        mine.append(s)
        t = r.CreateOfflineStream()
        t.AddSamples(x)
        refs.append(t)
    assert [s.SpeechLength for s in mine] == [s.SpeechLength for s in refs]
    assert _entities(r, mine) == _entities(r, refs)
    r.Dispose()


def test_recognizer_null_and_bad_pcm(model_dir):
    from aliparaformerasr_amd.offline_recognizer import ArgumentNullException
    r = _make(model_dir)
    s = r.CreateOfflineStream()
    with pytest.raises(ArgumentNullException):
        s.AddPcm(None, 16000)
    with pytest.raises(N.PfError) as ei:
        s.AddPcm(b"\0" * 64, 16000, channels=3)
    assert ei.value.code == N.PF_ERR_INVALID_ARG and s.SpeechLength == 0
    s.AddPcm(b"", 48000, 2)                                    # an empty block is an empty AddSamples
    assert s.SpeechLength == 0
    r.Dispose()


def test_two_threads_mixed_formats(model_dir):
    """Two caller threads on one recognizer, each with its own streams in mixed formats: the single-threaded results."""
    clips, want = _clips()
    r = _make(model_dir)
    halves = [(clips[0:3], want[0:3]), (clips[3:6], want[3:6])]
    solo = [_entities(r, _float_streams(r, w_)) for _c, w_ in halves]
    got, errs = [[], []], []

    def work(k):
        try:
            for _ in range(4):
                got[k].append(_entities(r, _pcm_streams(r, halves[k][0])))
        except Exception as ex:          # noqa: BLE001 — reported below, in the main thread
            errs.append(ex)
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        assert len(got[k]) == 4 and all(g == solo[k] for g in got[k])
    r.Dispose()


# ---- 6: the CLI --------------------------------------------------------------------------------------------------------
def _result_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith('{"text": "') or ln.endswith(".wav")]


def test_cli_intake_device_prints_the_host_lines(tmp_path):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "toy-model"
    d.mkdir()
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=1, vocab=150, timestamp_head=True)
    w = W.synth_weights(cfg, 44)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 5 * i) for i in range(146)] + ["<unk>"]
    (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    (d / "asr.yaml").write_text("model: paraformer\nfrontend_conf:\n  dither: 0.0\n")
    x = W.synth_audio(32000, 1)
    (d / "a.wav").write_bytes(wav_blob(16000, 1, "s16", _i16(x)[0].tobytes()))
    (d / "b.wav").write_bytes(wav_blob(16000, 2, "s16", _i16(np.stack([x, 0.5 * x], 1).reshape(-1))[0].tobytes(), odd_chunk=True))   # the quirk
    x48 = W.synth_audio(96000, 2)
    (d / "c.wav").write_bytes(wav_blob(48000, 2, "s16", _i16(np.stack([x48, 0.5 * x48], 1).reshape(-1))[0].tobytes(), extensible=True))
    for method in ("one", "batch"):
        outs = {}
        for intake in ("host", "device"):
            buf = io.StringIO()
            res = ex.offline_recognizer(method, "toy-model", "int8", 2, None, str(tmp_path), out=buf, intake=intake)
            assert len(res) == 3
            outs[intake] = buf.getvalue()
            assert "total_duration_milliseconds:6000" in outs[intake]                     # 2 s + 2 s + 2 s
        lines = _result_lines(outs["host"])
        assert len(lines) == 6 and lines == _result_lines(outs["device"])
        assert all(len(r.Tokens) > 0 for r in res)
