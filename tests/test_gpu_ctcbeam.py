"""GPU: the CTC prefix beam search on the device (csrc/k_ctcbeam.hip, Engine.set_decode(PF_DECODE_CTC_BEAM),
OfflineRecognizer.SetCtcBeam) — the kernel against the definition (tests/ctcbeam_ref.py) over the committed inputs, a fill
check, the engine in all four math modes against the definition fed the engine's own lists, refusals, the recognizer
mirror, two caller threads, the CLI.

Comparison rule: token lists and their order identical; scores within 16 * T * 2^-53 * max(1, |s|)."""
import io
import threading
import wave

import numpy as np
import pytest

import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import glue

pytestmark = pytest.mark.gpu
SCORES, CTC, TOPK, BEAM = N.PF_DECODE_SCORES, N.PF_DECODE_CTC, N.PF_DECODE_TOPK, N.PF_DECODE_CTC_BEAM
SV_VOCAB = 403


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, T):
    assert [h[0] for h in got] == [h[0] for h in want]
    for (_, a), (_, b) in zip(got, want):
        print("    score %.17g  reference %.17g  |diff| %.3g  tol %.3g" % (a, b, abs(a - b), R.tol(T, b)))
        assert abs(a - b) <= R.tol(T, b), (a, b, abs(a - b), R.tol(T, b))


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


# ---- 1: the kernel against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_kernel_equals_reference(any_engine, case):
    """B = 3 with lengths (T, 1, 0) over one input; N = W and N = 1; every output slot is overwritten (canary)."""
    lb, ids, val, n = R.case_arrays(case)
    T, K, Wd = case[2], case[4], case[5]
    rep = lambda a: np.ascontiguousarray(np.stack([a, a, a]))  # noqa: E731
    lens = np.array([T, 1, 0], np.int32)
    refs = [R.case_reference(case).beam, R.case_reference(case, 1).beam, [((), 0.0)]]
    for n_best in sorted({Wd, 1}):
        out = (np.full((3, n_best, T), 0x5A5A5A5A5A5A5A5A, np.int64), np.full((3, n_best), -77, np.int32),
               np.full((3, n_best), 12345.0, np.float64), np.full(3, -77, np.int32))
        r = any_engine.op_ctc_beam(rep(lb), rep(ids), rep(val), rep(n), lens, Wd, n_best, out=out)
        for b in range(3):
            want = refs[b][:n_best]
            print("  %s N=%d utterance %d: %d hypotheses" % (case[0], n_best, b, len(want)))
            assert r.n_hyp[b] == len(want)
            _same(r.hyps(b), want, max(int(lens[b]), 1))
            for i in range(n_best):                                               # fill values, no canary left
                k = int(r.len[b, i])
                assert 0 <= k <= T and (r.ids[b, i, k:] == -1).all() and (r.ids[b, i, :k] >= 1).all()
                if i >= r.n_hyp[b]:
                    assert k == 0 and r.score[b, i] == -np.inf


def test_kernel_lengths_beyond_the_batch_and_unread_rows(any_engine):
    """len is clamped to 0 .. T; rows at or beyond len[b] and list slots at or beyond n[t] are never read: NaN / garbage
    there changes nothing."""
    case = R.GPU_CASES[-1]
    lb, ids, val, n = R.case_arrays(case)
    T, K, Wd = case[2], case[4], case[5]
    half = T // 2
    lb2, ids2, val2, n2 = lb.copy(), ids.copy(), val.copy(), n.copy()
    lb2[half:] = np.nan
    ids2[half:] = 1
    val2[half:] = np.inf
    n2[half:] = 0
    rag = R.case_arrays(R.GPU_CASES[7])                                           # ragged: poison the slots past n[t]
    assert R.GPU_CASES[7][6] == "ragged"
    r_ids, r_val = rag[1].copy(), rag[2].copy()
    for t in range(rag[0].shape[0]):
        r_ids[t, rag[3][t]:] = 1
        r_val[t, rag[3][t]:] = np.inf
    r = any_engine.op_ctc_beam(np.stack([lb, lb2]), np.stack([ids, ids2]), np.stack([val, val2]), np.stack([n, n2]),
                               np.array([T + 5, half], np.int32), Wd)
    _same(r.hyps(0), R.case_reference(case).beam, T)
    _same(r.hyps(1), R.case_reference(case, half).beam, half)
    rc = R.GPU_CASES[7]
    r = any_engine.op_ctc_beam(rag[0][None], r_ids[None], r_val[None], rag[3][None], np.array([rc[2]], np.int32), rc[5])
    _same(r.hyps(0), R.case_reference(rc).beam, rc[2])
    # a frame without entries, a NaN blank: no hypotheses, fill values everywhere
    hole = n.copy()
    hole[3] = 0
    nan = lb.copy()
    nan[T - 1] = np.nan
    r = any_engine.op_ctc_beam(np.stack([lb, nan]), np.stack([ids, ids]), np.stack([val, val]), np.stack([hole, n]),
                               np.array([T, T], np.int32), Wd)
    assert r.n_hyp.tolist() == [0, 0] and (r.ids == -1).all() and (r.len == 0).all() and (r.score == -np.inf).all()


def test_kernel_shape_refusals(any_engine):
    lb, ids, val, n = R.case_arrays(R.GPU_CASES[-1])
    args = (lb[None], ids[None], val[None], n[None], np.array([12], np.int32))
    for Wd, nb in ((0, 0), (65, 1), (2, 3), (3, 0)):
        with pytest.raises(N.PfError) as ei:
            any_engine.op_ctc_beam(*args, Wd, nb)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        any_engine.op_ctc_beam(*args, 3, 3, cap=0)
    assert ei.value.code == N.PF_ERR_INVALID_ARG


# ---- 2: the engine, the tiny SenseVoice model of tests/test_gpu_topk.py, every math mode -------------------------------------
def _sv_model(sv_embed):
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=SV_VOCAB)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)
    b[8:] -= 30
    b[0] += 1.0
    w["ctc.bias"] = b
    return cfg, w


def _audio():
    return [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_beam_is_the_reference_of_its_own_lists(sv_embed, mode):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e0.set_decode(TOPK)
    e1.set_decode(BEAM)                                                          # implies TOPK and SCORES
    Wd, NB, K = 8, 5, 4
    e1.set_ctc_beam(Wd, NB)
    r0 = e0.recognize(audio, want_logits=True)
    r1 = e1.recognize(audio, want_logits=True)
    assert r0.beam is None and r1.beam is not None and r1.beam.N == NB
    # with the flag clear (TOPK alone) ids, scores, logits and lists are bit-identical
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r1.scores), _bits(r0.scores))
    np.testing.assert_array_equal(_bits(r1.logits), _bits(r0.logits))
    np.testing.assert_array_equal(r1.topk.ids, r0.topk.ids)
    np.testing.assert_array_equal(_bits(r1.topk.val), _bits(r0.topk.val))
    np.testing.assert_array_equal(r1.topk.n, r0.topk.n)
    rows = [4 + e1.frontend(a).shape[0] for a in audio]                          # n_b: the prompt rows and the utterance's frames
    assert max(rows) == r1.L and min(rows) < r1.L
    for b, nb in enumerate(rows):
        ref = R.beam_search(r1.logits[b, :nb, 0], r1.topk.ids[b, :nb], r1.topk.val[b, :nb], r1.topk.n[b, :nb], Wd, NB)
        print("  mode %d utterance %d: n_b=%d, %d hypotheses, decision gap %.3g" % (mode, b, nb, ref.n_hyp, ref.gap))
        assert r1.beam.n_hyp[b] == ref.n_hyp >= 2
        _same(r1.beam.hyps(b), ref.hyps, nb)
        lp = r1.logits[b, :nb].astype(np.float64)
        for labels, s in r1.beam.hyps(b):                                         # the search sums a subset of the alignments
            full = R.ctc_loglik(lp, labels)
            assert s <= full + R.tol(nb, full), (labels, s, full)
    # without want_logits the same list; CTC beside it changes neither
    r2 = e1.recognize(audio)
    assert [r2.beam.hyps(b) for b in range(3)] == [r1.beam.hyps(b) for b in range(3)]
    e1.set_decode(BEAM | CTC)
    r3 = e1.recognize(audio)
    assert r3.ctc is not None and [r3.beam.hyps(b) for b in range(3)] == [r1.beam.hyps(b) for b in range(3)]
    # the flag cleared: nothing extra comes back
    e1.set_decode(0)
    r = e1.recognize(audio)
    assert r.beam is None and r.topk is None and r.scores is None
    np.testing.assert_array_equal(r.token_ids, r0.token_ids)
    e0.close(); e1.close()


def test_status_codes_and_refusals(sv_embed):
    import ctypes as C
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pf = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        pf.set_decode(BEAM)                                                       # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    sc = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        sc.set_decode(BEAM)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    sc.close()
    cfg, w = _sv_model(sv_embed)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    lib, h = eng._lib, eng._h
    for bit in (4, 64):
        assert lib.pf_engine_set_decode(h, bit) == N.PF_ERR_INVALID_ARG
        assert lib.pf_engine_set_decode(h, BEAM | bit) == N.PF_ERR_INVALID_ARG
    for Wd, nb in ((4, 5), (0, 0), (65, 1), (8, 0), (-1, -1)):
        assert lib.pf_engine_set_ctc_beam(h, Wd, nb) == N.PF_ERR_INVALID_ARG, (Wd, nb)
    audio = _audio()[:2]
    mx = C.c_int32()
    eng.set_decode(TOPK)
    eng.recognize(audio)
    assert lib.pf_fetch_ctc_beam(h, None, None, None, 0, None, mx) == N.PF_ERR_INVALID_ARG   # the forward ran without the flag
    eng.set_decode(BEAM)
    eng.set_ctc_beam(6, 3)
    r = eng.recognize(audio)
    assert r.beam.N == 3 and r.topk is not None and r.scores is not None
    assert lib.pf_fetch_ctc_beam(h, None, None, None, 0, None, mx) == N.PF_OK and mx.value == int(r.beam.len.max()) >= 1
    ids = np.full((2, 3, mx.value), -7, np.int64)
    ln = np.full((2, 3), -7, np.int32)
    p = ids.ctypes.data_as(C.POINTER(C.c_int64))
    mx2 = C.c_int32()
    assert lib.pf_fetch_ctc_beam(h, p, ln.ctypes.data_as(C.POINTER(C.c_int32)), None, mx.value - 1, None, mx2) == N.PF_ERR_CAPACITY
    assert mx2.value == mx.value and (ids == -7).all()                            # the size comes with the error
    np.testing.assert_array_equal(ln, r.beam.len)
    assert lib.pf_fetch_ctc_beam(h, p, None, None, mx.value, None, None) == N.PF_OK
    np.testing.assert_array_equal(ids, r.beam.ids[:, :, : mx.value])
    eng.close()


# ---- 3: the recognizer mirror ---------------------------------------------------------------------------------------------------
def _sv_dir(tmp_path, sv_embed):
    cfg, w = _sv_model(sv_embed)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + ["<|tag%d|>" % i for i in range(20)] + [chr(0x4E00 + i) for i in range(SV_VOCAB - 24)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], toks


def _get(rec, audio):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        streams.append(s)
    return streams, rec.GetResults(streams)


def test_recognizer_ctc_beam(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, toks = _sv_dir(tmp_path, sv_embed)
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    plain, lists, rec = (OfflineRecognizer(*paths) for _ in range(3))
    NB, Wd, K = 4, 8, 4
    lists.SetNBest(1, K)                                                         # the per-frame lists the search reads
    lists.SetDecode(scores=True)
    rec.SetCtcBeam(NB, Wd, K)
    s0, res0 = _get(plain, audio)
    sl, _ = _get(lists, audio)
    s1, res1 = _get(rec, audio)
    for b in range(2):
        # Tokens, Timestamps, Scores and the text are what they are without the option
        assert s1[b].Tokens == s0[b].Tokens and s1[b].Timestamps == s0[b].Timestamps and s1[b].Scores == s0[b].Scores == []
        assert (res1[b].Text, res1[b].Tokens, res1[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        assert s0[b].Alternatives == []
        assert s1[b].TokenAlternatives == sl[b].TokenAlternatives
        alts = s1[b].Alternatives
        assert 2 <= len(alts) <= NB
        sc = [a.Score for a in alts]
        assert sc == sorted(sc, reverse=True) and len({tuple(a.Ids) for a in alts}) == len(alts)
        for a in alts:                                                            # the same DecodeMulti as the result
            text, _tlen, tk, _ = glue.decode_multi_one(toks, a.Ids, [[0, 0]] * len(a.Ids))
            assert (a.Text, a.Tokens) == (text, tk)
            assert all(i >= 1 for i in a.Ids)
    # the longest utterance fills the batch: its list is the definition's over the frames' lists and blank column
    b = 0
    ta = sl[b].TokenAlternatives
    ids = np.asarray([[p[0] for p in row] for row in ta], np.int64)
    val = np.asarray([[p[1] for p in row] for row in ta], np.float32)
    blank_rows = [(t, row) for t, row in enumerate(ta) if any(p[0] == 0 for p in row)]
    if len(blank_rows) == len(ta):                                                # the blank sits in every list: its column is known
        lb = np.asarray([next(p[1] for p in row if p[0] == 0) for row in ta], np.float32)
        ref = R.beam_search(lb, ids, val, np.full(len(ta), K, np.int32), Wd, NB)
        print("  the blank is listed at every frame: compared with the definition, decision gap %.3g" % ref.gap)
        _same([(tuple(a.Ids), a.Score) for a in s1[b].Alternatives], ref.hyps, len(ta))
    # refusals; off again
    for bad in ((65, 0, 4), (-1, 0, 4), (4, 3, 4), (4, 65, 4), (4, 8, 9)):
        with pytest.raises(N.PfError) as ei:
            rec.SetCtcBeam(*bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        rec.SetNBest(2, 4)                                                        # SetNBest keeps refusing N > 1 here
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.SetCtcBeam(0)
    s2, res2 = _get(rec, audio)
    assert s2[0].Alternatives == [] and s2[0].TokenAlternatives == [] and res2[0].Text == res0[0].Text
    for r in (plain, lists, rec):
        r.Dispose()


def test_recognizer_refuses_paraformer(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, W.synth_weights(cfg, seed=3))
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
    (tmp_path / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(61)]) + "\n", encoding="utf-8")
    rec = OfflineRecognizer(*[str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
    with pytest.raises(N.PfError) as ei:
        rec.SetCtcBeam(4, 8, 4)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.Dispose()


def test_two_threads_on_one_recognizer(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, _ = _sv_dir(tmp_path, sv_embed)
    rec = OfflineRecognizer(*paths)
    rec.SetCtcBeam(5, 8, 4)
    batches = [[W.synth_audio(32000, 5), W.synth_audio(20000, 6)], [W.synth_audio(26000, 91)]]

    def snapshot(streams, res):
        return [(r.Text, s.Tokens, [(a.Ids, a.Score, a.Text) for a in s.Alternatives]) for s, r in zip(streams, res)]
    want = [snapshot(*_get(rec, b)) for b in batches]
    assert want[0][0][2] != want[1][0][2] and len(want[0][0][2]) >= 2
    errors = []

    def worker(i):
        try:
            for _ in range(4):
                assert snapshot(*_get(rec, batches[i])) == want[i]
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    rec.Dispose()


def test_cli_prints_n_lines(tmp_path, sv_embed):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "m"
    d.mkdir()
    _sv_dir(d, sv_embed)
    pcm = (np.clip(W.synth_audio(32000, 40), -1, 1) * 32767).astype("<i2")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    texts = []
    for method in ("one", "batch"):
        out = io.StringIO()
        res = ex.offline_recognizer(method=method, model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=3, topk=4, beam=8)
        lines = out.getvalue().splitlines()
        nb = [ln for ln in lines if ln.startswith("nbest[")]
        assert len(res) == 1 and len(nb) == 3, out.getvalue()
        assert [ln.split("]")[0] for ln in nb] == ["nbest[%d" % i for i in range(3)]
        assert lines[lines.index(nb[0]) - 1].startswith('{"text": "%s"' % res[0].Text)          # under the usual result line
        sc = [float(ln.split("score:")[1].split(" ")[0]) for ln in nb]
        assert sc == sorted(sc, reverse=True)
        texts.append(res[0].Text)
    out = io.StringIO()
    res = ex.offline_recognizer(method="one", model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out)
    assert "nbest[" not in out.getvalue() and res[0].Text == texts[0]            # without -beam nothing changes
