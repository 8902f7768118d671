"""GPU: the CT-Transformer punctuation model on the device (csrc/k_punc.hip) against the definition in numpy float64
(tests/punc_ref.py) and the host twins: released dimensions (d_model 256, 8 heads, FFN 1024, kernel 11, 6 classes), vocabulary
64, 1 / 2 / 4 layers, synthetic weights.

Batch independence is asserted bit for bit: every window length of punc_ref.LENGTHS run in one call and alone, a batch in both
orders, a second call.  The layer-0 input and the cut rule are exact.  The logits have no exact-answer inputs (LayerNorm,
softmax), so their tolerance is measured: punc_ref.emulate_f16 mirrors the kernel's rounding points, its deviation from float64
on these weights is computed here, and the device is allowed 4 x that (accumulation order, fp32 softmax and LayerNorm
statistics).  Measured on one MI355X (max |logit - float64| over all windows; emulation / device):
  1 layer   1.696e-03 / 1.618e-03      2 layers  2.145e-03 / 2.171e-03      4 layers  2.124e-03 / 2.193e-03
so the allowance of 4 x is 6.8e-03 .. 8.6e-03; 1721 / 1700 / 1694 of the 1742 positions have a float64 top-2 margin above twice
that and are asserted, and the device agreed on all but one of the others as well."""
import numpy as np
import pytest

import punc_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu
LAYERS = [1, 2, 4]


@pytest.fixture(scope="module")
def eng():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.set_punc_model(None)
    e.close()


@pytest.fixture(scope="module")
def models():
    """per layer count: config, weights, the loaded model, and the reference computed once: the emulation's deviation, the
    float64 margins and the float64 logits of every window of R.LENGTHS"""
    out = {}
    for nl in LAYERS:
        cfg = W.ct_transformer_config(vocab=64, n_layers=nl)
        w = W.synth_punc_weights(cfg, seed=5)
        out[nl] = (cfg, w, E.load_punc_model(W.pack_pfw(cfg, w)), R.deviation_and_margin(w, cfg))
    yield out
    for v in out.values():
        v[2].close()


def _windows(cfg):
    return [R.window_ids(T, cfg["vocab"], T) for T in R.LENGTHS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("nl", LAYERS)
def test_a_window_does_not_depend_on_its_batch(eng, models, nl):
    cfg, w, m, _ = models[nl]
    eng.set_punc_model(m)
    wins = _windows(cfg)
    P = cfg["n_punc"]
    total = sum(R.LENGTHS)
    buf = np.full(total * P + 256, np.nan, np.float32)
    together = eng.op_punc_logits(wins, out=buf)
    assert np.isnan(buf[total * P:]).all() and np.isfinite(buf[: total * P]).all()         # nothing beyond [rows, n_punc] is stored
    for T, ids, z in zip(R.LENGTHS, wins, together):
        assert z.shape == (T, P)
        alone = eng.op_punc_logits([ids])[0]
        assert _same(alone, z), T
    again = eng.op_punc_logits(wins)
    assert all(_same(a, b) for a, b in zip(again, together))
    batch = [R.window_ids(T, cfg["vocab"], 50 + T) for T in (5, 0, 70, 1, 131)]
    fwd, rev = eng.op_punc_logits(batch), eng.op_punc_logits(batch[::-1])[::-1]
    assert all(_same(a, b) for a, b in zip(fwd, rev))
    assert all(_same(eng.op_punc_logits([ids])[0], z) for ids, z in zip(batch, fwd))
    # an empty batch and a batch of empty windows launch nothing and store nothing
    assert eng.op_punc_logits([]) == [] and [z.shape for z in eng.op_punc_logits([batch[1], batch[1]])] == [(0, P)] * 2


@pytest.mark.parametrize("nl", LAYERS)
def test_layer0_input_and_cut_are_exact(eng, models, nl):
    cfg, w, m, _ = models[nl]
    eng.set_punc_model(m)
    wins = _windows(cfg)
    _, x0 = eng.op_punc_logits(wins, want_x0=True)
    e16 = w["embed.weight"].astype(np.float16).astype(np.float32)
    for ids, x in zip(wins, x0):
        assert _same(x, R.layer0_input(w, cfg, ids, embed=e16)), len(ids)
    for last in ([False] * len(wins), [True] * len(wins), [i % 2 == 0 for i in range(len(wins))]):
        p, cut, z = eng.op_punc_window(wins, last, want_logits=True)
        for b, ids in enumerate(wins):
            want_cut, want_p = E.host_punc_cut(m, R.argmax_ties_larger(z[b]), last[b])
            assert cut[b] == want_cut and p[b].tolist() == want_p.tolist(), (len(ids), last[b])


def test_cut_kernel_at_every_branch(eng, models):
    """The cut launch on marks of the test's choosing: a decoder of zero weights makes the arg-max the largest bias, and ties go
    to the larger index, so a one-layer model whose decoder bias is zero but for one class marks every word with that class."""
    cfg = W.ct_transformer_config(vocab=64, n_layers=1)
    w = W.synth_punc_weights(cfg, seed=5)
    for mark in (1, 2, 3):                                                             # "_", "，", "。"
        w2 = dict(w)
        w2["decoder.weight"] = np.zeros_like(w["decoder.weight"])
        w2["decoder.bias"] = np.zeros_like(w["decoder.bias"])
        w2["decoder.bias"][mark] = 1.0
        m = E.load_punc_model(W.pack_pfw(cfg, w2))
        eng.set_punc_model(m)
        lens = [0, 1, 3, 4, 5, 30, 200, 201, 492, 493, 512]
        wins = [R.window_ids(T, 64, T) for T in lens]
        for last in (False, True):
            p, cut = eng.op_punc_window(wins, [last] * len(wins))
            for b, T in enumerate(lens):
                want_cut, want_p = E.host_punc_cut(m, np.full(T, mark, np.int32), last)
                assert cut[b] == want_cut and p[b].tolist() == want_p.tolist(), (mark, T, last)
        eng.set_punc_model(None)
        m.close()


def test_argmax_ties_go_to_the_larger_index_on_the_device(eng):
    """exactly tied logits (a decoder of zero weights: every row's logits are the bias), in both lane halves of the kernel's
    arg-max (classes 0 - 3 and 4 - 5 lie in different halves) and across them"""
    cfg = W.ct_transformer_config(vocab=64, n_layers=1)
    w = W.synth_punc_weights(cfg, seed=5)
    wins = [R.window_ids(T, 64, T) for T in (1, 33, 70)]
    for bias, want in (([0, 1, 1, 0, 1, 0], 4), ([2, 2, 2, 2, 2, 2], 5), ([1, 1, 0, 0, 0, 0], 1), ([3, 0, 0, 0, 0, 0], 0), ([0, 0, 7, 7, 0, 0], 3)):
        w2 = dict(w)
        w2["decoder.weight"] = np.zeros_like(w["decoder.weight"])
        w2["decoder.bias"] = np.asarray(bias, np.float32)
        m = E.load_punc_model(W.pack_pfw(cfg, w2))
        eng.set_punc_model(m)
        p, cut, z = eng.op_punc_window(wins, [False] * 3, want_logits=True)
        for b in range(3):
            assert (z[b] == np.asarray(bias, np.float32)[None]).all()
            want_cut, want_p = E.host_punc_cut(m, np.full(len(wins[b]), want, np.int32), False)
            assert p[b].tolist() == want_p.tolist() and cut[b] == want_cut, (bias, b)
        eng.set_punc_model(None)
        m.close()


@pytest.mark.parametrize("nl", LAYERS)
def test_logits_within_four_times_the_emulation(eng, models, nl):
    cfg, w, m, (dev, margins, z64) = models[nl]
    eng.set_punc_model(m)
    got = eng.op_punc_logits(_windows(cfg))
    err = max(float(np.abs(g.astype(np.float64) - z).max()) for g, z in zip(got, z64) if len(z))
    print("punc n_layers=%d: emulation %.3e, device %.3e, allowed %.3e" % (nl, dev, err, 4 * dev))
    assert err <= 4 * dev
    # the punctuation ids wherever the float64 top-2 margin exceeds twice the allowed deviation; at most 5 % fall outside
    p_dev = np.concatenate([R.argmax_ties_larger(g) for g in got])
    p_ref = np.concatenate([R.argmax_ties_larger(z) for z in z64])
    safe = margins > 2 * 4 * dev
    assert (p_dev[safe] == p_ref[safe]).all()
    assert 1.0 - safe.mean() <= 0.05
    print("punc n_layers=%d: %d of %d positions asserted, %d of the rest agree" % (nl, int(safe.sum()), safe.size, int((p_dev[~safe] == p_ref[~safe]).sum())))


def test_an_overflowing_embedding_row_poisons_its_own_window_only(eng, models):
    """A row of 70000 is finite in the container and infinite in the f16 table: LayerNorm makes it NaN, attention spreads it over
    the window that holds it, and no other window of the batch changes a bit."""
    cfg, w, m, _ = models[2]
    w2 = dict(w)
    w2["embed.weight"] = w["embed.weight"].copy()
    w2["embed.weight"][3] = 70000.0
    bad = E.load_punc_model(W.pack_pfw(cfg, w2))
    clean = [np.array([i for i in R.window_ids(T, 64, 9 + T) if i != 3], np.int32) for T in (40, 70, 9)]
    dirty = clean[1].copy()
    dirty[17] = 3
    eng.set_punc_model(m)
    want = eng.op_punc_logits(clean)
    eng.set_punc_model(bad)
    got = eng.op_punc_logits([clean[0], dirty, clean[2], clean[1]])
    assert np.isnan(got[1]).all()
    assert _same(got[0], want[0]) and _same(got[2], want[2]) and _same(got[3], want[1])
    eng.set_punc_model(None)
    bad.close()


def test_end_to_end_loop_launch_census_and_detach(eng, models):
    cfg, w, m, _ = models[2]
    audio = [W.synth_audio(16000, 1)]
    before = eng.recognize(audio, want_logits=True)
    eng.profile(True)
    eng.profile_reset()
    eng.recognize(audio)
    classes = ("punc", "layernorm", "gemm_op", "fsmn", "cif_misc", "argmax", "attn_self", "vad", "vadnet", "fbank", "attn_op", "topk",
               "lfr_cmvn_pad", "gemm_qkv", "gemm_outffn", "gemm_out", "gemm_ffn2", "gemm_dec_ffn", "dec_mid", "attn_cross", "gemm_op_mid",
               "quantize", "lstm", "ts_misc", "pcm_to_samples")
    census_before = [eng.profile_get(c)[1] for c in classes]
    eng.profile(False)
    assert census_before[0] == 0 and sum(census_before) > 0

    eng.set_punc_model(m)
    lens = [0, 1, 19, 20, 21, 45, 230]
    texts = [R.window_ids(n, cfg["vocab"], 300 + n) for n in lens]
    eng.profile(True)
    eng.profile_reset()
    got, rounds = eng.punctuate(texts)
    census = [eng.profile_get(c)[1] for c in classes]
    eng.profile(False)
    assert rounds == 12 and census[0] == rounds * (2 + 2 * cfg["n_layers"]) and not any(census[1:])
    forward = lambda win: R.argmax_ties_larger(eng.op_punc_logits([win])[0])
    for ids, p in zip(texts, got):
        want, log = R.text_loop(ids, forward, cfg["punc_list"], cfg["sentence_end_id"])
        assert p.tolist() == want.tolist() and len(p) == len(ids)
        # the same loop with the host's cut rule in place of the definition's
        cache, out = np.zeros(0, np.int32), []
        for k in range((len(ids) + 19) // 20):
            win = np.concatenate([cache, ids[20 * k: 20 * k + 20]])
            cut, q = E.host_punc_cut(m, forward(win), k == (len(ids) + 19) // 20 - 1)
            out += q[: cut + 1].tolist()
            cache = win[cut + 1:]
        assert out == p.tolist()
    # through the text: words on the host, the loop on the device, the assembly on the host
    vocab = R.vocab_of(w)
    text = "".join(vocab[1:5]) + " wb hello " + "".join(vocab[6:10]) * 9 + " x"
    out_text, sent, p = eng.punctuate_text([text, ""])[0]
    want_text, want_sent, want_p = R.punctuate(text, vocab, forward, cfg["punc_list"], cfg["sentence_end_id"])
    assert (out_text, sent, p.tolist()) == (want_text, want_sent, want_p.tolist())
    assert eng.punctuate_text([""])[0][0] == ""

    # with the model attached the recogniser computes what it computed before; detached, so does its launch census
    mid = eng.recognize(audio, want_logits=True)
    assert np.array_equal(mid.token_ids, before.token_ids) and _same(mid.logits, before.logits)
    eng.set_punc_model(None)
    eng.profile(True)
    eng.profile_reset()
    after = eng.recognize(audio, want_logits=True)
    census_after = [eng.profile_get(c)[1] for c in classes]
    eng.profile(False)
    assert census_after == census_before
    assert np.array_equal(after.token_ids, before.token_ids) and _same(after.logits, before.logits)
    for call in (lambda: eng.op_punc_logits([texts[1]]), lambda: eng.punctuate([texts[1]])):
        with pytest.raises(N.PfError) as ei:
            call()
        assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_bad_arguments(eng, models):
    cfg, w, m, _ = models[1]
    eng.set_punc_model(m)
    for ids in (np.array([1, 64], np.int32), np.array([-1], np.int32), np.zeros(513, np.int32)):
        with pytest.raises(N.PfError) as ei:
            eng.op_punc_logits([ids])
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        eng.punctuate([np.array([64], np.int32)])
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    eng.set_punc_model(None)


# ---- recognizer --------------------------------------------------------------------------------------------------------------
VOCAB = 300


def _model_dir(d, **kw):
    from oracle import frontend as fe
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB, **kw)
    W.save_pfw(str(d / "model.pfw"), cfg, W.synth_weights(cfg, seed=77))
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text("model: paraformer\nuse_itn: false\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n"
                                "  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n")
    vocab = W.synth_punc_vocab(64)
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + [vocab[1 + i % 63] if i % 3 else chr(0x5000 + i) for i in range(VOCAB - 4)]
    (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]


def _streams(r, audio):
    out = []
    for a in audio:
        s = r.CreateOfflineStream()
        s.AddSamples(a)
        out.append(s)
    return out


@pytest.mark.parametrize("timestamps", [False, True])
def test_recognizer_punctuates_its_text(tmp_path, eng, models, timestamps):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    cfg, w, m, _ = models[2]
    paths = _model_dir(tmp_path, **(dict(timestamp_head=True) if timestamps else {}))
    W.save_pfw(str(tmp_path / "punc.pfw"), cfg, w)
    audio = [W.synth_audio(48000, 5), W.synth_audio(16000, 6), W.synth_audio(80000, 7)]
    r = OfflineRecognizer(*paths)
    ss = _streams(r, audio)
    plain = r.GetResults(ss)
    assert [s.Punctuated for s in ss] == [""] * 3 and all(s.Sentences == [] and s.PuncIds == [] for s in ss)
    r.SetPuncModel(str(tmp_path / "punc.pfw"))
    ss = _streams(r, audio)
    res = r.GetResults(ss)
    assert [(x.Text, x.Tokens, x.Timestamps) for x in res] == [(x.Text, x.Tokens, x.Timestamps) for x in plain]
    eng.set_punc_model(m)
    forward = lambda win: R.argmax_ties_larger(eng.op_punc_logits([win])[0])
    vocab = R.vocab_of(w)
    timed = 0
    for s, x in zip(ss, res):
        text, sent, p = R.punctuate(x.Text, vocab, forward, cfg["punc_list"], cfg["sentence_end_id"])
        assert s.Punctuated == text and s.PuncIds == p.tolist()
        assert [z.WordEnd for z in s.Sentences] == sent and [z.WordBegin for z in s.Sentences] == [0] + sent[:-1]
        assert "".join(z.Text for z in s.Sentences).replace(" ", "") == text.replace(" ", "")
        one_each = len(p) > 0 and len(x.Timestamps) == len(p) and any(list(t) != [0, 0] for t in x.Timestamps)   # ({0, 0}: no timestamps)
        timed += one_each
        for z in s.Sentences:
            assert z.Times == ([x.Timestamps[z.WordBegin][0], x.Timestamps[z.WordEnd - 1][1]] if one_each else [])
    assert sum(len(s.PuncIds) for s in ss) > 0
    if not timestamps:
        assert timed == 0
    print("punc recognizer timestamps=%s: %d of 3 streams carry sentence times; %r" % (timestamps, timed, ss[0].Punctuated[:60]))
    # with SetVad the stitched text is punctuated, once
    r.SetVad(True, batch_max=4, sep="")
    ss = _streams(r, audio[:1])
    res = r.GetResults(ss)
    text, sent, p = R.punctuate(res[0].Text, vocab, forward, cfg["punc_list"], cfg["sentence_end_id"])
    assert ss[0].Punctuated == text and ss[0].PuncIds == p.tolist()
    r.SetVad(None)
    # cleared: nothing is kept on the stream any more
    r.SetPuncModel(None)
    ss = _streams(r, audio)                                        # (the same batch: results depend on batch mates, quirk Q2)
    again = r.GetResults(ss)
    assert all(s.Punctuated == "" and s.Sentences == [] for s in ss) and [x.Text for x in again] == [x.Text for x in plain]
    eng.set_punc_model(None)
    r.Dispose()


# ---- a real model, opt-in --------------------------------------------------------------------------------------------------------
REAL_TEXT = "今天天气怎么样我们去公园吧 hello world 你吃饭了吗我还没有吃我们一起去吧好的那就这样我先走了明天见"


def test_real_model_file(tmp_path, eng):
    """PF_REAL_PUNC_MODEL=<model.pt | model.onnx>,<tokens.json | tokens.txt>: the file through the converter and the loader, a
    fixed text through the device loop; the device's logits of every window against the host twin within 4 x the f16
    emulation's deviation on those windows, the loop exactly the definition's over the device's own arg-max.  No such file
    exists where this was written: the test has never run against one."""
    import os
    spec = os.environ.get("PF_REAL_PUNC_MODEL", "")
    if "," not in spec:
        pytest.skip("set PF_REAL_PUNC_MODEL=<model.pt|model.onnx>,<tokens> to run against a real CT-Transformer")
    from aliparaformerasr_amd import convert as cv
    model_path, tokens_path = spec.split(",", 1)
    out = str(tmp_path / "punc.pfw")
    assert cv.main([model_path, out, "--kind", "cttransformer", "--tokens", tokens_path]) == 0
    cfg, w = W.load_pfw(out)
    m = E.load_punc_model(out)
    eng.set_punc_model(m)
    try:
        ids, words = E.host_punc_words(m, REAL_TEXT * 3)
        assert words == R.split_words(REAL_TEXT * 3) and ids.tolist() == R.word_ids(words, R.vocab_of(w)).tolist()
        forward = lambda win: R.argmax_ties_larger(eng.op_punc_logits([win])[0])
        want, log = R.text_loop(ids, forward, cfg["punc_list"], cfg["sentence_end_id"])
        (text, sent, p), = eng.punctuate_text([REAL_TEXT * 3])
        assert p.tolist() == want.tolist() and (text, sent) == R.assemble(words, want, cfg["punc_list"])
        host_text, host_p = E.host_punc_text(m, REAL_TEXT * 3)
        print("punc real model: device %r\n                 host   %r (%d of %d marks agree)" % (text, host_text, int((host_p == p).sum()), len(p)))
        for win, _, _ in log:
            z64 = E.host_punc_logits(m, win)
            dev = float(np.abs(R.emulate_f16(w, cfg, win) - z64).max())
            err = float(np.abs(eng.op_punc_logits([win])[0].astype(np.float64) - z64).max())
            print("punc real model: window of %d: emulation %.3e, device %.3e" % (len(win), dev, err))
            assert err <= 4 * dev
    finally:
        eng.set_punc_model(None)
        m.close()
