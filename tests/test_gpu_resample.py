"""GPU: the band-limited resampler of the PCM intake (csrc/k_resample.hip; PF_PCM_RESAMPLE_SINC through Engine.op_pcm_convert /
stage_pcm / recognize_pcm and OfflineStream.AddPcm(resample="sinc")) — bit-equal to its host twin, within the derived bound of
the float64 definition (tests/resample_ref.py), at every tile edge, bank path and configuration."""
import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
import resample_ref as R
from pcm_ref import bits_equal, payload

pytestmark = pytest.mark.gpu
FS, TILE = 16000, N.PF_RESAMPLE_TILE
FORMS = (("s16", 1, 0), ("s16", 2, 1), ("s24", 2, 0), ("f32", 1, 0))           # format, channels, unpaired trailing values


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


def _check(eng, data, sr, ch, fmt, cfg=None, **shape):
    """device == host twin bit for bit, and within the bound of the definition"""
    desc = N.pcm_desc(sr, ch, fmt, sinc=True)
    got = eng.op_pcm_convert(data, desc)
    host = N.host_pcm_convert(data, desc, cfg=cfg)
    assert bits_equal(got, host), (sr, ch, fmt, got.size, np.flatnonzero(got.view(np.uint32) != host.view(np.uint32))[:4])
    want, bound = R.resample(R.mono(data, sr, ch, fmt), sr, FS, **shape)
    ok = np.isfinite(want)
    assert got.size == want.size and np.all(np.abs(got[ok] - want[ok]) <= bound[ok])


def _n_mono_for(n_out, sr):       # the shortest input with n_out outputs (where the rate skips that length: the next one)
    n = int(n_out * sr / FS)
    while R.n_out_of(n, sr, FS) < n_out:
        n += 1
    return n


@pytest.mark.parametrize("sr", R.RATES)
def test_kernel_equals_the_host_twin_at_every_edge(eng, sr):
    H = R.shape(sr, FS)[2]
    lengths = [_n_mono_for(t, sr) for t in (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)] + [H - 1, H, H + 1]
    for k, n_mono in enumerate(lengths):
        fmt, ch, odd = FORMS[(k + sr // 1000) % 4]
        data = payload(fmt, n_mono * ch + odd, seed=sr // 100 + k)
        _check(eng, data, sr, ch, fmt)


def test_a_nan_poisons_exactly_the_outputs_that_read_it(eng):
    x = np.frombuffer(payload("f32", 4000, seed=8), "<f4").copy()
    x[1500] = np.nan
    got = eng.op_pcm_convert(x, N.pcm_desc(48000, 1, "f32", sinc=True))
    host = N.host_pcm_convert(x, N.pcm_desc(48000, 1, "f32", sinc=True))
    H = R.shape(48000, FS)[2]
    b = 3 * np.arange(got.size)
    reads = (b - H + 1 <= 1500) & (1500 <= b + H)
    assert np.array_equal(np.isnan(got), reads) and np.array_equal(np.isnan(host), reads)
    assert bits_equal(got[~reads], host[~reads])


def test_configurations_and_both_bank_paths(eng):
    data = payload("s16", 3000, seed=12)
    try:
        for sr, shape in ((11025, dict(zeros=32)),                             # a 179 KB bank: read from global memory
                          (11025, dict(zeros=24)),                             # 136 KB: in LDS behind the input tile
                          (48000, dict(zeros=1, rolloff=1.0, beta=0.0)), (8000, dict(zeros=1, rolloff=1.0, beta=0.0))):
            eng.set_resample(**shape)                                          # the next call uses the new bank
            _check(eng, data, sr, 1, "s16", cfg=N.resample_config(**shape), **shape)
        with pytest.raises(N.PfError) as ei:
            eng.set_resample(zeros=65)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    finally:
        eng.set_resample()
    _check(eng, data, 11025, 1, "s16")                                         # and the defaults again


def test_alias_is_gone_and_the_passband_is_kept_on_the_device(eng):
    n = np.arange(100, 1500)
    y = eng.op_pcm_convert(R.tone(10000, 48000, 4800), N.pcm_desc(48000, 1, "f32", sinc=True))
    assert np.sqrt(np.mean(y[n].astype(np.float64) ** 2)) < 1e-5
    y = eng.op_pcm_convert(R.tone(3000, 48000, 4800), N.pcm_desc(48000, 1, "f32", sinc=True))
    assert np.max(np.abs(y[n] - 0.5 * np.sin(2 * np.pi * 3000 * n / FS))) < 1e-5


def _i16(x):
    return np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype("<i2")


def test_one_batch_mixes_native_linear_flagged_and_empty_rows(eng):
    """every row's samples are its single-call samples (read back through the model: the same ids, lengths and, where the float
    path repeats them, logits); without a flagged row the launch census is the parent's"""
    rows = [(_i16(W.synth_audio(20000, 1)), 16000, 1, False), (_i16(W.synth_audio(2 * 48000, 2)), 48000, 2, False),
            (_i16(W.synth_audio(2 * 48000 + 1, 3)), 48000, 2, True), (_i16(W.synth_audio(30000, 4)), 11025, 1, True),
            (np.zeros(0, "<i2"), 44100, 1, True), (_i16(W.synth_audio(40000, 6)), 48000, 1, True)]
    datas = [r[0] for r in rows]
    descs = [N.pcm_desc(sr, ch, "s16", sinc=s) for _d, sr, ch, s in rows]
    single = [eng.op_pcm_convert(d, dc) for d, dc in zip(datas, descs)]
    assert all(bits_equal(x, N.host_pcm_convert(d, dc)) for x, d, dc in zip(single, datas, descs))
    census = []
    eng.profile(True)
    try:
        eng.profile_reset()
        a = eng.recognize_pcm(datas, descs, want_logits=True)
        census.append([eng.profile_get(c)[1] for c in ("pcm_to_samples", "resample_sinc")])
        eng.profile_reset()
        eng.stage_pcm(datas[:2], descs[:2])
        census.append([eng.profile_get(c)[1] for c in ("pcm_to_samples", "resample_sinc")])
    finally:
        eng.profile(False)
    assert census == [[1, 1], [1, 0]]
    b, b2 = eng.recognize(single, want_logits=True), eng.recognize(single, want_logits=True)
    np.testing.assert_array_equal(a.token_ids, b.token_ids)
    np.testing.assert_array_equal(a.token_num, b.token_num)
    if np.array_equal(b.logits.view(np.uint32), b2.logits.view(np.uint32)):
        np.testing.assert_array_equal(a.logits.view(np.uint32), b.logits.view(np.uint32))


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_model")
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=300, timestamp_head=True)
    w = W.synth_weights(cfg, seed=78)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text("model: paraformer\nfrontend_conf:\n  dither: 0\n")
    (d / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>", "<unk>"] + [chr(0x4E00 + 7 * i) for i in range(296)]) + "\n",
                                  encoding="utf-8")
    return d


@pytest.mark.parametrize("device_streams", ("1", "0"))
def test_recognizer_add_pcm_sinc_equals_add_samples_of_the_host_twin(model_dir, monkeypatch, device_streams):
    """the device and the host form, a non-default shape, SetVad on"""
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    monkeypatch.setenv("PF_RECOGNIZER_DEVICE_STREAMS", device_streams)
    d = model_dir
    rec = OfflineRecognizer(modelFilePath=str(d / "model.pfw"), configFilePath=str(d / "asr.yaml"), mvnFilePath=str(d / "am.mvn"),
                            tokensFilePath=str(d / "tokens.txt"))
    clips = [(_i16(W.synth_audio(3 * 48000, 91)), 48000, 1), (_i16(W.synth_audio(2 * 2 * 44100, 92)), 44100, 2)]

    def results(shape, vad):
        cfg = N.resample_config(**shape)
        rec.SetResampler(**shape)
        rec.SetVad(True if vad else None)
        out = []
        for use_pcm in (True, False):
            ss = []
            for x, sr, ch in clips:
                s = rec.CreateOfflineStream()
                if use_pcm:
                    s.AddPcm(x, sr, ch, "s16", resample="sinc")
                else:
                    s.AddSamples(N.host_pcm_convert(x, N.pcm_desc(sr, ch, "s16", sinc=True), cfg=cfg))
                ss.append(s)
            out.append([(r.Text, list(r.Tokens)) for r in rec.GetResults(ss)])
        assert out[0] == out[1] and (vad or all(len(t) > 2 for _x, t in out[0]))

    for shape, vad in (({}, False), (dict(zeros=8, beta=6.0), False), ({}, device_streams == "1")):   # (SetVad cuts device audio)
        results(shape, vad)
    rec.Dispose()
