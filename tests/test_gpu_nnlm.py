"""GPU: the causal Transformer LM on the device (csrc/k_nnlm.hip) against the definition in numpy float64 (tests/nnlm_ref.py):
released d_model 512 / 8 heads / FFN 2048 / embedding 128, vocabularies 33 (one decoder block plus one channel) and 100 (a
ragged last block), 1 and 2 layers, synthetic weights.

Batch independence and causality are asserted bit for bit.  logp has no exact-answer inputs (LayerNorm, softmax), so its
tolerance is measured: nnlm_ref.emulate_f16 mirrors the kernel's rounding points, its deviation from float64 on these weights
(dev_f16) is computed here on the CPU, and the device is allowed 4 x that (accumulation order, fp32 softmax and LayerNorm
statistics).  Every call goes through pf_op_nnlm_logp, whose sentinels refuse a row that was not written and a cell beyond
[rows] / [B] that was; the plain pf_engine_nnlm_score is held to the same bits."""
import os

import numpy as np
import pytest

import nnlm_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu
GPU_CASES, gpu_case = R.GPU_CASES, R.gpu_case


@pytest.fixture(scope="module")
def eng():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.set_nnlm(None)
    e.close()


@pytest.fixture(scope="module")
def models():
    """per (V, n_layers): config, weights, the loaded model, and the reference computed once: dev_f16 and the float64 logp of
    every hypothesis of R.LENGTHS"""
    out = {}
    for V, nl in GPU_CASES:
        cfg, w = gpu_case(V, nl)
        out[V, nl] = (cfg, w, E.load_nnlm_model(W.pack_pfw(cfg, w)), R.deviation(w, cfg))
    yield out
    for v in out.values():
        v[2].close()


def _hyps(V):
    return [R.hyp_ids(n, V, n) for n in R.LENGTHS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _score(eng, hyps, **kw):
    return eng.nnlm_score(hyps, op=True, **kw)


@pytest.mark.parametrize("V,nl", GPU_CASES)
def test_a_hypothesis_does_not_depend_on_its_batch(eng, models, V, nl):
    cfg, w, m, _ = models[V, nl]
    eng.set_nnlm(m)
    hyps = _hyps(V)
    total = sum(n + 1 for n in R.LENGTHS)
    buf = np.full(total + 256, np.nan, np.float32)
    lm, together = _score(eng, hyps, out=buf)
    assert np.isnan(buf[total:]).all() and np.isfinite(buf[:total]).all() and (buf[:total] <= 0).all()
    for n, ids, lp, s in zip(R.LENGTHS, hyps, together, lm):
        lm1, alone = _score(eng, [ids])
        assert lp.shape == (n + 1,) and _same(alone[0], lp) and _bits(lm1)[0] == _bits(s), n
        assert _bits(s) == _bits(R.lm_sum_f32(lp, False))                      # the sequential float32 sum of the device's own logp
    lm_eos, again = _score(eng, hyps, eos=True)
    assert all(_same(a, b) for a, b in zip(again, together))
    assert all(_bits(s) == _bits(R.lm_sum_f32(lp, True)) for s, lp in zip(lm_eos, together))
    plain_lm, plain = eng.nnlm_score(hyps)                                      # pf_engine_nnlm_score: the same bits
    assert _same(plain_lm, lm) and all(_same(a, b) for a, b in zip(plain, together))
    batch = [R.hyp_ids(n, V, 50 + n) for n in (5, 0, 70, 1, 131)]
    (lf, fwd), (lr, rev) = _score(eng, batch), _score(eng, batch[::-1])
    assert all(_same(a, b) for a, b in zip(fwd, rev[::-1])) and _same(lf, lr[::-1])
    assert all(_same(_score(eng, [ids])[1][0], z) for ids, z in zip(batch, fwd))
    assert _score(eng, [])[1] == []


@pytest.mark.parametrize("V,nl", GPU_CASES)
def test_a_later_token_changes_nothing_before_it(eng, models, V, nl):
    cfg, w, m, _ = models[V, nl]
    eng.set_nnlm(m)
    for n, t in ((40, 0), (70, 31), (70, 32), (200, 63), (200, 64), (255, 254)):
        a = R.hyp_ids(n, V, 900 + n)
        b = a.copy()
        b[t] = (b[t] + 1) % V
        (_, (la, lb)) = _score(eng, [a, b])
        assert _same(la[:t], lb[:t]) and not _same(la[t:], lb[t:]), (n, t)


@pytest.mark.parametrize("V,nl", GPU_CASES)
def test_logp_within_four_times_the_emulation(eng, models, V, nl):
    cfg, w, m, (dev, z64) = models[V, nl]
    eng.set_nnlm(m)
    _, got = _score(eng, _hyps(V))
    err = max(float(np.abs(g.astype(np.float64) - z).max()) for g, z in zip(got, z64))
    print("nnlm V=%d n_layers=%d: emulation %.3e, device %.3e, allowed %.3e" % (V, nl, dev, err, 4 * dev))
    assert err <= 4 * dev


@pytest.mark.parametrize("V,nl", GPU_CASES)
def test_ranking(eng, models, V, nl):
    """pf_host_nnlm_fuse over the device's own lm_sum, against the float64 order wherever two adjacent float64 scores lie further
    apart than the band (at most 5 % lie inside it: tests/test_nnlm_cpu.py)"""
    cfg, w, m, (dev, _) = models[V, nl]
    eng.set_nnlm(m)
    lists = R.ranking_lists(V)
    lm_all, _ = _score(eng, [h for hyps, _ in lists for h in hyps], want_logp=False)
    for i, (hyps, base) in enumerate(lists):
        n = [len(h) for h in hyps]
        lm = lm_all[R.LIST_N * i: R.LIST_N * (i + 1)].astype(np.float64)
        score, order = E.host_nnlm_fuse(base, lm, n, R.WEIGHT, R.BONUS)
        want_s, want_o = R.fuse(base, lm, n, R.WEIGHT, R.BONUS)
        assert np.array_equal(score, want_s) and order.tolist() == want_o.tolist()
        s64, o64 = R.fuse(base, [R.lm_sum(R.logp64(w, cfg, h), False) for h in hyps], n, R.WEIGHT, R.BONUS)
        rank = np.argsort(order)                                                 # the device's place of every hypothesis
        for (a, b), unsafe in zip(zip(o64[:-1], o64[1:]), R.unsafe_pairs(s64, o64, n, dev)):
            assert unsafe or rank[a] < rank[b], (i, a, b)


def test_bad_arguments_and_detach(eng, models):
    cfg, w, m, _ = models[100, 1]
    eng.set_nnlm(m)
    for hyps in ([[1, 100]], [[-1]], [[0] * 256]):
        for op in (False, True):
            with pytest.raises(N.PfError) as ei:
                eng.nnlm_score(hyps, op=op)
            assert ei.value.code == N.PF_ERR_INVALID_ARG
    eng.profile(True)
    eng.profile_reset()
    eng.nnlm_score([[1, 2, 3], []])
    launches = eng.profile_get("nnlm")[1]
    eng.profile(False)
    assert launches == 2 + 2 * cfg["n_layers"]
    eng.set_nnlm(None)
    with pytest.raises(N.PfError) as ei:
        eng.nnlm_score([[1]])
    assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_real_model_file(tmp_path, eng):
    """PF_REAL_NNLM_MODEL=<model.pt>: the file through the converter and the loader, fixed hypotheses through the device; logp
    against the host twin within 4 x the f16 emulation's deviation on those hypotheses.  The architecture, the tensor names and
    sos = eos = V - 1 are remembered, not validated: no such file exists where this was written, and the test has never run
    against one."""
    path = os.environ.get("PF_REAL_NNLM_MODEL", "")
    if not path:
        pytest.skip("set PF_REAL_NNLM_MODEL=<model.pt> to run against a real Transformer LM")
    from aliparaformerasr_amd import convert as cv
    out = str(tmp_path / "lm.pfw")
    assert cv.main([path, out, "--kind", "transformerlm"]) == 0
    cfg, w = W.load_pfw(out)
    m = E.load_nnlm_model(out)
    eng.set_nnlm(m)
    try:
        for n in (0, 7, 40):
            ids = R.hyp_ids(n, cfg["vocab"], n)
            z64 = E.host_nnlm_logp(m, ids)
            dev = float(np.abs(R.emulate_f16(w, cfg, ids) - z64).max())
            err = float(np.abs(_score(eng, [ids])[1][0].astype(np.float64) - z64).max())
            print("nnlm real model: %d tokens: emulation %.3e, device %.3e" % (n, dev, err))
            assert err <= 4 * dev
    finally:
        eng.set_nnlm(None)
        m.close()


# ---- through OfflineRecognizer ---------------------------------------------------------------------------------------------------
def _model_dir(d, kind, sv_embed):
    from oracle import frontend as fe
    if kind == "sensevoice":
        V = 403
        cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=V)
        w = W.synth_weights(cfg, seed=9)
        w["embed.weight"] = sv_embed.astype(np.float32)
        b = np.array(w["ctc.bias"], np.float32)
        b[8:] -= 30
        b[0] += 1.0
        w["ctc.bias"] = b
        yaml = "model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n"
    else:
        V = 64
        cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=V)
        w = W.synth_weights(cfg, seed=3)
        yaml = "frontend_conf:\n  dither: 0\n"
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text(yaml)
    (d / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(V - 3)]) + "\n", encoding="utf-8")
    lm_cfg = W.transformer_lm_config(vocab=V, n_layers=1)
    lm_w = W.synth_nnlm_weights(lm_cfg, seed=11)
    W.save_pfw(str(d / "lm.pfw"), lm_cfg, lm_w)
    other = W.transformer_lm_config(vocab=V + 1, n_layers=1)
    W.save_pfw(str(d / "lm_other.pfw"), other, W.synth_nnlm_weights(other, seed=11))
    return [str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], lm_cfg, lm_w


def _get(rec, audio):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        streams.append(s)
    return streams, rec.GetResults(streams)


CLASSES = ("nnlm", "layernorm", "gemm_op", "fsmn", "cif_misc", "argmax", "attn_self", "fbank", "attn_op", "topk", "lfr_cmvn_pad",
           "gemm_qkv", "gemm_outffn", "gemm_out", "gemm_ffn2", "gemm_dec_ffn", "dec_mid", "attn_cross", "gemm_op_mid", "ts_misc",
           "pcm_to_samples", "ctc_collapse", "ctc_beam", "nbest_search", "quantize", "lstm")


def _census(rec, audio):
    """one GetResults on the recogniser's engine with the profile on: (streams, results, launches per class)"""
    import ctypes as C
    lib, h = rec._lib, C.c_void_p(rec._lib.pf_recognizer_engine(rec._h))
    N.check(lib.pf_profile_enable(h, 1))
    N.check(lib.pf_profile_reset(h))
    streams, res = _get(rec, audio)
    counts = []
    for c in CLASSES:
        ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
        N.check(lib.pf_profile_get(h, c.encode(), ms, n, fpl))
        counts.append(n.value)
    N.check(lib.pf_profile_enable(h, 0))
    return streams, res, counts


@pytest.mark.parametrize("kind,setup", [("paraformer", "nbest"), ("paraformer", "search"), ("sensevoice", "beam")])
def test_recognizer_rescores_its_alternatives(tmp_path, eng, sv_embed, kind, setup):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, lm_cfg, lm_w = _model_dir(tmp_path, kind, sv_embed)
    audio = [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]
    rec = OfflineRecognizer(*paths)
    if setup == "beam":
        rec.SetCtcBeam(4, 8, 4)
    else:
        rec.SetNBest(6, 4)
        if setup == "search":
            rec.SetNBestSearch(16)
    s0, res0, census0 = _census(rec, audio)
    assert census0[0] == 0 and sum(census0) > 0
    assert all(a.NnlmSum is None for s in s0 for a in s.Alternatives) and sum(len(s.Alternatives) for s in s0) >= 4
    weight, bonus = 0.7, 0.2
    with pytest.raises(N.PfError) as ei:
        rec.SetRescoreModel(str(tmp_path / "lm_other.pfw"))                      # another vocabulary
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    rec.SetRescoreModel(str(tmp_path / "lm.pfw"), weight, bonus, eos=True)
    with pytest.raises(N.PfError) as ei:
        rec.SetVad(True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    s1, res1, census1 = _census(rec, audio)                                      # one call over all alternatives of all streams,
    assert census1 == [2 + 2 * lm_cfg["n_layers"]] + census0[1:]                 # and the forward's own launches are the parent's
    m = E.load_nnlm_model(str(tmp_path / "lm.pfw"))
    eng.set_nnlm(m)
    for a, b, ra, rb in zip(s0, s1, res0, res1):
        assert (a.Tokens, a.Timestamps, a.Scores) == (b.Tokens, b.Timestamps, b.Scores)
        assert (ra.Text, ra.Tokens, ra.Timestamps) == (rb.Text, rb.Tokens, rb.Timestamps)
        old, new = a.Alternatives, b.Alternatives
        if not old:
            assert new == []
            continue
        lm, _ = eng.nnlm_score([x.Ids for x in old], eos=True, want_logp=False)
        base = [x.Score if x.LogLikSum is None else x.LogLikSum for x in old]
        score, order = E.host_nnlm_fuse(base, lm.astype(np.float64), [len(x.Ids) for x in old], weight, bonus)
        assert [x.Ids for x in new] == [old[i].Ids for i in order]               # a permutation, in pf_host_nnlm_fuse's order
        assert [x.Score for x in new] == score[order].tolist() and [x.NnlmSum for x in new] == lm.astype(np.float64)[order].tolist()
        assert [(x.Text, x.Tokens, x.LogLikSum, x.LmSum) for x in new] == [(old[i].Text, old[i].Tokens, old[i].LogLikSum, old[i].LmSum) for i in order]
    eng.set_nnlm(None)
    m.close()
    rec.SetRescoreModel(None)                                                    # detached: the parent's list, no LM launch
    s2, _, census2 = _census(rec, audio)
    assert census2 == census0
    assert [s.Alternatives for s in s2] == [s.Alternatives for s in s0]
    rec.Dispose()


def test_group_forward_refuses_an_attached_lm(models):
    from aliparaformerasr_amd.engine import EngineGroup
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    g = EngineGroup([0, 0], weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn())
    h0 = g._lib.pf_group_engine(g._h, 0)
    assert g._lib.pf_engine_set_nnlm(h0, models[100, 1][2]._h) == N.PF_OK
    with pytest.raises(N.PfError) as ei:
        g.recognize([W.synth_audio(20000, 41), W.synth_audio(16000, 42)])
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    assert g._lib.pf_engine_set_nnlm(h0, None) == N.PF_OK
    g.close()
