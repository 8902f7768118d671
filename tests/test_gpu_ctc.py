"""GPU: opt-in SenseVoice CTC decoding on the device (csrc/k_ctc.hip, Engine.set_decode, OfflineRecognizer.SetDecode) —
the collapse kernel against the numpy reference (tests/ctc_ref.py) bit for bit, the engine's scores / CTC result against
its own per-frame output in all four math modes, against the CPU oracle, through every entry point, for the other model
kinds, through the recognizer mirror and with two callers on one engine."""
import ctypes as C
import threading

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from ctc_ref import collapse_ref, timestamps_ms
from oracle import frontend as fe
from oracle import glue
from oracle import model as om

pytestmark = pytest.mark.gpu
VOCAB = 403
AUDIO_N = (48000, 24000, 33000)
SCORES, CTC = N.PF_DECODE_SCORES, N.PF_DECODE_CTC


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """CtcResult == collapse_ref tuple, scores bit for bit (both cut / padded to the larger token count)."""
    n, ids, first, last, score = want
    np.testing.assert_array_equal(got.n, n)
    k = int(n.max()) if n.size else 0
    np.testing.assert_array_equal(got.ids[:, :k], ids[:, :k])
    np.testing.assert_array_equal(got.first[:, :k], first[:, :k])
    np.testing.assert_array_equal(got.last[:, :k], last[:, :k])
    np.testing.assert_array_equal(_bits(got.score[:, :k]), _bits(score[:, :k]))


def _sv_model(sv_embed, recipe):
    """The SenseVoice config of test_gpu_sensevoice.py with a CTC head that emits blanks and repeats: every id >= 8 is
    pushed down by 30 (recipe A), and the blank is lifted by 1.0 on top (recipe B)."""
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=VOCAB)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)
    b[8:] -= 30
    if recipe == "B":
        b[0] += 1.0
    w["ctc.bias"] = b
    return cfg, w


def _audio():
    return [W.synth_audio(n, 70 + u) for u, n in enumerate(AUDIO_N)]


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


# ---- 1 / 2: the kernel alone ---------------------------------------------------------------------------------------
def _scores(rng, shape):
    return (-rng.random(shape, dtype=np.float32) * 8 - 1e-3).astype(np.float32)


def test_collapse_kernel_crafted_runs(any_engine):
    rng = np.random.default_rng(1)
    T = 300
    rows = []
    a = np.zeros(T, np.int64); a[60:70] = 5                      # a run crossing frame 63 -> 64
    rows.append((a, T))
    a = np.zeros(T, np.int64); a[10:250] = 3                     # a run crossing several chunks
    rows.append((a, T))
    a = np.zeros(T, np.int64); a[3] = 2; a[100:104] = 2; a[290:] = 4      # blank stretches longer than 64
    rows.append((a, T))
    a = np.full(T, 6, np.int64); a[:40] = 1                      # a run cut at len (inside a chunk, and at a chunk edge)
    rows.append((a, 150))
    rows.append((a.copy(), 128))
    a = np.full(T, 7, np.int64)                                  # one token over the whole row
    rows.append((a, T))
    a = np.arange(T, dtype=np.int64) % 5                         # a start on (almost) every frame
    rows.append((a, T))
    a = np.zeros(T, np.int64); a[63] = 2; a[64] = 3; a[127] = 3; a[128] = 3    # changes exactly at chunk edges
    rows.append((a, T))
    rows.append((np.full(T, 2, np.int64), 0))                    # len 0
    ids = np.stack([r[0] for r in rows])
    lens = np.asarray([r[1] for r in rows], np.int32)
    sc = _scores(rng, ids.shape)
    got = any_engine.op_ctc_collapse(ids, sc, lens)
    want = collapse_ref(ids, sc, lens, cap=T)
    assert want[0].tolist()[:2] == [1, 1] and want[0][-1] == 0
    _same(got, want)
    # slots past n hold the fixed fill values
    np.testing.assert_array_equal(got.ids, want[1])
    np.testing.assert_array_equal(got.first, want[2])
    np.testing.assert_array_equal(got.last, want[3])
    np.testing.assert_array_equal(_bits(got.score), _bits(want[4]))


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 174, 504, 3001])
def test_collapse_kernel_property(any_engine, B, T):
    rng = np.random.default_rng(1000 * B + T)
    for trial in range(4):
        k = 2 + (trial + B + T) % 4                               # alphabet of 2 .. 5 symbols, blank (0) included
        ids = rng.integers(0, k, size=(B, T)).astype(np.int64)
        if trial % 2:                                             # sticky rows: runs of up to 200 frames
            for b in range(B):
                t = 0
                while t < T:
                    r = int(rng.integers(1, 200))
                    ids[b, t:t + r] = ids[b, t]
                    t += r
        lens = rng.integers(0, T + 1, size=B).astype(np.int32)
        if B == 1:
            lens[0] = (T, 0, T, lens[0])[trial]
        else:                                                     # every draw holds a full row and an empty one
            full = int(rng.integers(0, B))
            lens[full] = T
            lens[(full + 1 + int(rng.integers(0, B - 1))) % B] = 0
        sc = _scores(rng, ids.shape)
        got = any_engine.op_ctc_collapse(ids, sc, lens)
        want = collapse_ref(ids, sc, lens, cap=T)
        assert (want[0] <= lens).all()
        _same(got, want)


def test_collapse_kernel_capacity_and_clamped_lens(any_engine):
    ids = np.asarray([[1, 2, 3, 4, 5, 6]], np.int64)
    sc = _scores(np.random.default_rng(2), ids.shape)
    with pytest.raises(N.PfError) as ei:
        any_engine.op_ctc_collapse(ids, sc, [6], cap=4)
    assert ei.value.code == N.PF_ERR_CAPACITY
    _same(any_engine.op_ctc_collapse(ids, sc, [99]), collapse_ref(ids, sc, [6]))       # lens beyond T are clamped
    _same(any_engine.op_ctc_collapse(ids, sc, [-5]), collapse_ref(ids, sc, [0]))


# ---- 3 / 5: the engine against its own per-frame output, every math mode ---------------------------------------------
def _valid_rows(eng, audio):
    return np.asarray([4 + eng.num_frames(len(a)) for a in audio], np.int32)


def _run_stats(ids, nb):
    blanks = [int((ids[b, :nb[b]] == 0).sum()) for b in range(ids.shape[0])]
    runs = 0
    for b in range(ids.shape[0]):
        _, _, first, last, _ = collapse_ref(ids[b:b + 1], np.zeros_like(ids[b:b + 1], np.float32), nb[b:b + 1])
        runs += int(((last - first) >= 1).sum())
    return blanks, runs


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_ctc_is_the_collapse_of_its_own_frames(sv_embed, mode):
    """Recipe B.  With flags 3 the per-frame ids and log-probs stay bit-identical to an engine without flags,
    scores[b, t] is the stored log-prob of ids[b, t], and the fetched CTC result is collapse_ref(ids, scores, n_b).
    In math_mode 0 the batch must make that non-trivial: blanks in every utterance, repeated frames, two utterances
    shorter than the batch."""
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed, "B")
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e3 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e3.set_decode(SCORES | CTC)
    r0 = e0.recognize(audio, want_logits=True)
    r3 = e3.recognize(audio, want_logits=True)
    nb = _valid_rows(e3, audio)
    T = r3.L
    blanks, runs = _run_stats(r3.token_ids, nb)
    print("mode %d: T=%d n_b=%s blank frames=%s runs>=2 frames=%d collapsed=%s" % (mode, T, nb.tolist(), blanks, runs,
                                                                                 r3.ctc.n.tolist()))
    assert r0.scores is None and r0.ctc is None
    if mode == 0:
        assert min(blanks) >= 1 and runs >= 3 and (nb < T).any()
    assert T == int(nb.max())
    np.testing.assert_array_equal(r3.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r3.logits), _bits(r0.logits))
    gathered = np.take_along_axis(r3.logits, r3.token_ids[..., None], axis=-1)[..., 0]
    assert r3.scores.shape == (len(audio), T)
    np.testing.assert_array_equal(_bits(r3.scores), _bits(gathered))
    _same(r3.ctc, collapse_ref(r3.token_ids, r3.scores, nb))
    # without want_logits (the arg-max does not store the log-probs): the same scores and the same collapse
    r3b = e3.recognize(audio)
    np.testing.assert_array_equal(_bits(r3b.scores), _bits(r3.scores))
    _same(r3b.ctc, collapse_ref(r3.token_ids, r3.scores, nb))
    # flags back to 0: nothing extra comes back
    e3.set_decode(0)
    r = e3.recognize(audio)
    assert r.scores is None and r.ctc is None
    np.testing.assert_array_equal(r.token_ids, r0.token_ids)
    e0.close(); e3.close()


# ---- 4: against the CPU oracle ---------------------------------------------------------------------------------------
def test_engine_ctc_vs_oracle(sv_embed):
    """Recipe A, math_mode 0, the oracle's own features through pf_model_proj (the input the existing 2e-2 log-prob
    tolerance was established for).  For the utterances whose every valid frame has a top-two margin above 0.04 on the
    live oracle (the project's safe-frame rule) ids, first and last equal the collapse of the oracle's frames exactly and
    the scores agree within 2e-2."""
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed, "A")
    cmvn, audio = W.synth_cmvn(), _audio()
    conf = fe.FrontendConf(dither=0.0)
    feats = [glue.sensevoice_prepend(fe.wav_frontend(a, conf, cmvn[0], cmvn[1]), sv_embed, use_itn=True) for a in audio]
    nb = np.asarray([f.shape[0] for f in feats], np.int32)
    T = int(nb.max())
    speech = fe.pad_sequence(feats).reshape(len(audio), T, 560)
    ref = om.Oracle(om.ModelConfig(**cfg), w, quant="fp16").sensevoice(speech)["logits"]
    ids_ref = om.argmax_last(ref)
    srt = np.sort(ref, axis=-1)
    margin = srt[..., -1] - srt[..., -2]
    mins = [float(margin[b, :nb[b]].min()) for b in range(len(audio))]
    want = collapse_ref(ids_ref, srt[..., -1], nb)
    print("oracle: n_b=%s min margins=%s collapsed=%s" % (nb.tolist(), ["%.3f" % m for m in mins], want[0].tolist()))
    for b in (0, 2):
        assert mins[b] > 0.04, (b, mins[b])
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=cmvn, device=0, use_itn=True)
    eng.set_decode(CTC)
    got = eng.model_proj(feats).ctc
    for b in (0, 2):
        k = int(want[0][b])
        assert got.n[b] == k and k >= 1
        np.testing.assert_array_equal(got.ids[b, :k], want[1][b, :k])
        np.testing.assert_array_equal(got.first[b, :k], want[2][b, :k])
        np.testing.assert_array_equal(got.last[b, :k], want[3][b, :k])
        err = float(np.abs(got.score[b, :k] - want[4][b, :k]).max())
        print("utterance %d: %d tokens, max |dscore| %.3e" % (b, k, err))
        assert err < 2e-2, err
    eng.close()


# ---- 6: entry points ---------------------------------------------------------------------------------------------------
def test_entry_points_agree_on_the_valid_rows(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed, "B")
    cmvn, audio = W.synth_cmvn(), _audio()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=cmvn, device=0, use_itn=True)
    eng.set_decode(SCORES | CTC)
    feats = [glue.sensevoice_prepend(eng.frontend(a), sv_embed, use_itn=True) for a in audio]
    nb = np.asarray([f.shape[0] for f in feats], np.int32)
    np.testing.assert_array_equal(nb, _valid_rows(eng, audio))
    a = eng.recognize(audio)
    m = eng.model_proj(feats)
    np.testing.assert_array_equal(a.token_ids, m.token_ids)
    _same(m.ctc, (a.ctc.n, a.ctc.ids, a.ctc.first, a.ctc.last, a.ctc.score))
    _same(a.ctc, collapse_ref(a.token_ids, a.scores, nb))
    # the staged form (pf_stage_audio + pf_run_staged + pf_fetch) knows the sample counts too
    eng.stage_audio(audio)
    eng.run_staged()
    s = eng.fetch()
    _same(s.ctc, (a.ctc.n, a.ctc.ids, a.ctc.first, a.ctc.last, a.ctc.score))
    # pf_forward_feats has no lengths: every row of the batch is decoded
    T = int(nb.max())
    f = eng.forward_feats(fe.pad_sequence(feats).reshape(len(audio), T, 560))
    np.testing.assert_array_equal(f.token_ids, a.token_ids)
    _same(f.ctc, collapse_ref(f.token_ids, f.scores, np.full(len(audio), T, np.int32)))
    assert (f.ctc.n >= a.ctc.n).all()
    eng.close()


def test_fetch_status_codes(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed, "B")
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    lib, h = eng._lib, eng._h
    audio = _audio()
    n, n_max, L = np.zeros(3, np.int32), C.c_int32(), C.c_int32()
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    eng.recognize(audio)
    assert lib.pf_fetch_scores(h, None, 0, L) == N.PF_ERR_INVALID_ARG          # the forward ran without the flag
    assert lib.pf_fetch_ctc(h, None, None, None, None, 0, i32(n), n_max) == N.PF_ERR_INVALID_ARG
    assert lib.pf_engine_set_decode(h, 4) == N.PF_ERR_INVALID_ARG
    eng.set_decode(SCORES)
    r = eng.recognize(audio)
    assert r.scores is not None and r.ctc is None
    assert lib.pf_fetch_ctc(h, None, None, None, None, 0, i32(n), n_max) == N.PF_ERR_INVALID_ARG
    eng.set_decode(CTC)                                                         # implies SCORES
    r = eng.recognize(audio)
    assert r.scores is not None and r.ctc is not None
    assert lib.pf_fetch_ctc(h, None, None, None, None, 0, i32(n), n_max) == N.PF_OK
    assert n_max.value == int(r.ctc.n.max()) >= 2 and n.tolist() == r.ctc.n.tolist()
    ids = np.zeros((3, n_max.value - 1), np.int64)
    n[:] = 0
    assert lib.pf_fetch_ctc(h, ids.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, n_max.value - 1, i32(n),
                            n_max) == N.PF_ERR_CAPACITY
    assert n.tolist() == r.ctc.n.tolist()                                       # the size is reported with the error
    sc = np.zeros(4, np.float32)
    assert lib.pf_fetch_scores(h, sc.ctypes.data_as(C.POINTER(C.c_float)), 4, L) == N.PF_ERR_CAPACITY
    assert L.value == r.L
    eng.close()


# ---- 7: the other model kinds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_paraformer_scores_and_refusals(mode):
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=3, dec_layers=2, vocab=512)
    w = W.synth_weights(cfg, seed=11)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0, math_mode=mode)
    audio = [W.synth_audio(n, u) for u, n in enumerate((32000, 20000))]
    r0 = eng.recognize(audio, want_logits=True)
    with pytest.raises(N.PfError) as ei:
        eng.set_decode(CTC)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_decode(SCORES)
    r = eng.recognize(audio, want_logits=True)
    assert r.L == r0.L >= 1 and r.ctc is None
    np.testing.assert_array_equal(r.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r.logits), _bits(r0.logits))
    gathered = np.take_along_axis(r.logits, r.token_ids[..., None], axis=-1)[..., 0]
    np.testing.assert_array_equal(_bits(r.scores), _bits(gathered))
    np.testing.assert_array_equal(_bits(eng.recognize(audio).scores), _bits(gathered))
    eng.close()


def test_seaco_refuses_decode_flags():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    for flags in (SCORES, CTC, SCORES | CTC):
        with pytest.raises(N.PfError) as ei:
            eng.set_decode(flags)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_decode(0)
    eng.close()


# ---- 8: the recognizer mirror ------------------------------------------------------------------------------------------
def _toks():
    return ["<blank>", "<s>", "</s>", "<unk>"] + ["<|tag%d|>" % i for i in range(20)] + [chr(0x4E00 + i) for i in range(VOCAB - 24)]


@pytest.mark.parametrize("recipe", ["plain", "B"])
def test_recognizer_set_decode(tmp_path, sv_embed, recipe):
    """The temp-dir model of test_gpu_sensevoice.py (plain), and the same with the recipe-B head so that the collapse has
    blanks and repeats to work on; two streams of different length in one GetResults."""
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    if recipe == "plain":
        cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=VOCAB)
        w = W.synth_weights(cfg, seed=9)
        w["embed.weight"] = sv_embed.astype(np.float32)
    else:
        cfg, w = _sv_model(sv_embed, "B")
    cmvn = W.synth_cmvn()
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*cmvn))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = _toks()
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    paths = [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]

    def run(rec):
        streams = []
        for a in audio:
            s = rec.CreateOfflineStream()
            s.AddSamples(a)
            streams.append(s)
        nb = [4 + s.SpeechLength // 560 for s in streams]
        return streams, rec.GetResults(streams), nb

    r_plain, r_sc, r_ctc = (OfflineRecognizer(*paths) for _ in range(3))
    r_sc.SetDecode(scores=True)
    r_ctc.SetDecode(ctc=True)
    s0, res0, nb = run(r_plain)
    s1, res1, _ = run(r_sc)
    s2, res2, _ = run(r_ctc)
    L = max(nb)
    assert nb[1] < nb[0]
    for b in range(2):
        frames = np.asarray(s0[b].Tokens, np.int64)
        # without the option: today's output — one id per frame of the batch, {0, 0} timestamps, no scores
        assert frames.shape == (L,) and s0[b].Timestamps == [[0, 0]] * L and s0[b].Scores == []
        text, tlen, tk, _ = glue.decode_multi_one(toks, frames.tolist(), [[0, 0]] * L)
        assert (res0[b].Text, res0[b].TextLen, res0[b].Tokens) == (text, tlen, tk)
        # scores only: Tokens / Timestamps as today, Scores the [L] row
        assert s1[b].Tokens == frames.tolist() and s1[b].Timestamps == [[0, 0]] * L
        sc = np.asarray(s1[b].Scores, np.float32)
        assert sc.shape == (L,) and (sc <= 0).all()
        assert (res1[b].Text, res1[b].Tokens) == (res0[b].Text, res0[b].Tokens)
        # ctc: the collapse of those frames over the stream's own rows
        n, ids, first, last, score = collapse_ref(frames[None], sc[None], [nb[b]])
        k = int(n[0])
        print("recipe %s stream %d: %d frames (%d valid) -> %d tokens" % (recipe, b, L, nb[b], k))
        assert s2[b].Tokens == ids[0, :k].tolist()
        assert s2[b].Timestamps == timestamps_ms(first[0, :k], last[0, :k])
        got_sc = np.asarray(s2[b].Scores, np.float32)
        np.testing.assert_array_equal(_bits(got_sc), _bits(score[0, :k]))
        text, tlen, tk, _ = glue.decode_multi_one(toks, ids[0, :k].tolist(), timestamps_ms(first[0, :k], last[0, :k]))
        assert (res2[b].Text, res2[b].TextLen, res2[b].Tokens) == (text, tlen, tk)
    # switching the option off again restores today's output
    r_ctc.SetDecode()
    s3, res3, _ = run(r_ctc)
    for b in range(2):
        assert s3[b].Tokens == s0[b].Tokens and s3[b].Scores == [] and res3[b].Text == res0[b].Text
    for r in (r_plain, r_sc, r_ctc):
        r.Dispose()


def test_recognizer_refuses_ctc_for_paraformer(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    cmvn = W.synth_cmvn()
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, W.synth_weights(cfg, seed=3))
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*cmvn))
    (tmp_path / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
    (tmp_path / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(61)]) + "\n",
                                         encoding="utf-8")
    r = OfflineRecognizer(*[str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
    with pytest.raises(N.PfError) as ei:
        r.SetDecode(ctc=True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    r.SetDecode(scores=True)
    s = r.CreateOfflineStream()
    s.AddSamples(W.synth_audio(32000, 1))
    r.GetResult(s)
    assert len(s.Scores) == len(s.Tokens)
    r.Dispose()


# ---- 9: two callers, one engine ------------------------------------------------------------------------------------------
def test_two_threads_fetch_their_own_ctc_result(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed, "B")
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    eng.set_decode(SCORES | CTC)
    batches = [[W.synth_audio(n, 70 + u) for u, n in enumerate(AUDIO_N)],
               [W.synth_audio(n, 170 + u) for u, n in enumerate((20000, 40000))]]
    want = [eng.recognize(b) for b in batches]
    assert want[0].ctc.n.tolist() != want[1].ctc.n.tolist()
    errors = []

    def worker(i):
        try:
            for _ in range(6):
                r = eng.recognize(batches[i])          # learn L / fetch scores + CTC / fetch ids, all on this thread's slot
                np.testing.assert_array_equal(r.token_ids, want[i].token_ids)
                np.testing.assert_array_equal(_bits(r.scores), _bits(want[i].scores))
                _same(r.ctc, (want[i].ctc.n, want[i].ctc.ids, want[i].ctc.first, want[i].ctc.last, want[i].ctc.score))
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    eng.close()
