"""GPU: top-k alternatives per position and the n-best list (csrc/k_topk.hip, Engine.set_decode(PF_DECODE_TOPK),
OfflineRecognizer.SetNBest) — the kernel against the numpy reference (tests/topk_ref.py) bit for bit over every register
form and input design, against the existing arg-max, the engine in all four math modes and through every entry point
against the reference of its own log-probs, the recognizer mirror, two caller threads, the CLI."""
import ctypes as C
import io
import threading
import wave

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import host_nbest
from ctc_ref import collapse_ref
from oracle import frontend as fe
from oracle import glue
from topk_ref import nbest_brute, topk_ref

pytestmark = pytest.mark.gpu
SCORES, CTC, TOPK = N.PF_DECODE_SCORES, N.PF_DECODE_CTC, N.PF_DECODE_TOPK
SV_VOCAB = 403
DESIGNS = ("random", "equal", "dup", "down", "up", "minf", "nan", "allnan")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


# ---- 1: the kernel against the reference -------------------------------------------------------------------------------
def _row(design, V, rng):
    if design == "random":
        return (rng.standard_normal(V) * 3).astype(np.float32)
    if design == "equal":
        return np.full(V, np.float32(-2.75))
    if design == "dup":
        # the row's largest value at i, i + 64, i + 256 (other lanes, other waves, the same thread's next register) and a
        # runner-up repeated the same way; the rest quantised so that further ties exist
        x = np.round(rng.standard_normal(V) * 4).astype(np.float32) / 4
        i = int(rng.integers(0, max(V - 256, 1)))
        for off, v in ((0, 50.0), (3, 49.0)):
            for d in (0, 64, 256, 257):
                if i + off + d < V:
                    x[i + off + d] = v
        return x
    if design == "down":
        return -np.arange(V, dtype=np.float32)
    if design == "up":
        return np.arange(V, dtype=np.float32) - V
    if design == "minf":
        x = np.full(V, -np.inf, np.float32)
        if rng.integers(0, 2) and V > 2:                 # a few finite entries, fewer than K = 8
            x[rng.choice(V, size=min(3, V), replace=False)] = rng.standard_normal(min(3, V)).astype(np.float32)
        return x
    if design == "nan":
        x = (rng.standard_normal(V) * 3).astype(np.float32)
        x[rng.random(V) < 0.02] = np.nan
        x[int(rng.integers(0, V))] = np.nan
        if V > 300:                                      # the best entries sit right behind NaN neighbours
            x[257] = np.nan; x[258] = 60.0; x[2] = np.nan
        return x
    return np.full(V, np.nan, np.float32)


def _run_kernel(eng, x, V, K):
    """pf_op_topk into canary-filled buffers; returned whole."""
    rows = x.shape[0]
    ids = np.full((rows, K), 0x5A5A5A5A5A5A5A5A, np.int64)
    val = np.full((rows, K), 12345.0, np.float32)
    n = np.full(rows, -77, np.int32)
    N.check(eng._lib.pf_op_topk(eng._h, x.ctypes.data_as(C.POINTER(C.c_float)), rows, V, x.shape[1], K,
                                ids.ctypes.data_as(C.POINTER(C.c_int64)), val.ctypes.data_as(C.POINTER(C.c_float)),
                                n.ctypes.data_as(C.POINTER(C.c_int32))))
    return ids, val, n


@pytest.mark.parametrize("V", [1, 7, 255, 256, 257, 8404, 9216, 9217, 25055, 25600, 25601])
def test_kernel_equals_reference(any_engine, V):
    """rows 1 and 3 of every design, and 65 rows cycling through the designs; K 1 / 4 / 8; ld = V and ld = V + 37 with
    NaN / +inf in the slack.  The reference is formed once per block at K = 8 (a smaller K is its prefix)."""
    rng = np.random.default_rng(V)
    blocks = [np.stack([_row(d, V, rng) for _ in range(r)]) for d in DESIGNS for r in (1, 3)]
    blocks.append(np.stack([_row(DESIGNS[i % len(DESIGNS)], V, rng) for i in range(65)]))
    assert sorted({b.shape[0] for b in blocks}) == [1, 3, 65]
    for y in blocks:
        ids8, val8, n8 = topk_ref(y, 8)
        wide = np.empty((y.shape[0], V + 37), np.float32)
        wide[:, :V] = y
        wide[:, V::2] = np.nan
        wide[:, V + 1::2] = np.inf
        for K in (1, 4, 8):
            want = (ids8[:, :K], val8[:, :K], np.minimum(n8, K))
            for x in (y, wide):
                ids, val, n = _run_kernel(any_engine, np.ascontiguousarray(x), V, K)
                np.testing.assert_array_equal(n, want[2])
                np.testing.assert_array_equal(ids, want[0])
                np.testing.assert_array_equal(_bits(val), _bits(want[1]))


def test_kernel_shape_refusals(any_engine):
    x = np.zeros((2, 8), np.float32)
    lib, h = any_engine._lib, any_engine._h
    ids, val, n = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.float32), np.zeros(2, np.int32)
    p = (x.ctypes.data_as(C.POINTER(C.c_float)),)
    o = (ids.ctypes.data_as(C.POINTER(C.c_int64)), val.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_int32)))
    for rows, V, ld, K in ((2, 8, 8, 0), (2, 8, 8, 9), (2, 9, 8, 4), (2, 0, 8, 4), (-1, 8, 8, 4)):
        assert lib.pf_op_topk(h, *p, rows, V, ld, K, *o) == N.PF_ERR_INVALID_ARG, (rows, V, ld, K)
    assert lib.pf_op_topk(h, *p, 0, 8, 8, 4, *o) == N.PF_OK                    # no rows: nothing to do
    assert lib.pf_op_topk(h, None, 2, 8, 8, 4, *o) == N.PF_ERR_INVALID_ARG


# ---- 2: the kernel against the existing arg-max --------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 257, 8404, 25055, 25601])
def test_rank0_is_the_argmax(any_engine, V):
    rng = np.random.default_rng(100 + V)
    rows = [_row(d, V, rng) for d in ("random", "equal", "dup", "down", "up", "minf", "minf", "dup") for _ in range(2)]
    x = np.stack(rows)
    assert not np.isnan(x).any()
    t = any_engine.op_topk(x, K=4)
    np.testing.assert_array_equal(t.ids[:, 0], any_engine.op_argmax(x))
    # the log-probs the pipeline's arg-max stores: rank 0 is its id, and the value is the stored entry
    z = np.stack([_row(d, V, rng) for d in ("random", "dup", "equal", "down") for _ in range(2)])
    y, ids = any_engine.op_logsoftmax_argmax(z, store=True)
    t = any_engine.op_topk(y, K=8)
    np.testing.assert_array_equal(t.ids[:, 0], ids)
    np.testing.assert_array_equal(_bits(t.val[:, 0]), _bits(np.take_along_axis(y, ids[:, None], 1)[:, 0]))
    want = topk_ref(y, 8)
    np.testing.assert_array_equal(t.ids, want[0])
    np.testing.assert_array_equal(_bits(t.val), _bits(want[1]))


# ---- 3: the engine, small seeded models, every math mode -----------------------------------------------------------------
def _pf_model():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    return cfg, W.synth_weights(cfg, seed=3)


def _sv_model(sv_embed):
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=SV_VOCAB)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)              # blanks and repeats for the CTC collapse (test_gpu_ctc.py recipe B)
    b[8:] -= 30
    b[0] += 1.0
    w["ctc.bias"] = b
    return cfg, w


def _pf_audio():
    return [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]


def _check_topk(r, K):
    """A result with logits: its top-k is the reference of those logits, rank 0 is the 1-best with its score."""
    B, L = r.token_ids.shape
    assert r.topk is not None and r.topk.K == K and r.topk.ids.shape == (B, L, K) and r.topk.n.shape == (B, L)
    want = topk_ref(r.logits, K)
    np.testing.assert_array_equal(r.topk.n, want[2])
    np.testing.assert_array_equal(r.topk.ids, want[0])
    np.testing.assert_array_equal(_bits(r.topk.val), _bits(want[1]))
    assert (r.topk.n == min(K, r.V)).all()
    np.testing.assert_array_equal(r.topk.ids[..., 0], r.token_ids)
    np.testing.assert_array_equal(_bits(r.topk.val[..., 0]), _bits(r.scores))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["paraformer", "sensevoice"])
def test_engine_topk_is_the_reference_of_its_own_logits(sv_embed, kind, mode):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _pf_model() if kind == "paraformer" else _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _pf_audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1.set_decode(TOPK)                                                       # implies SCORES
    r0 = e0.recognize(audio, want_logits=True)
    r1 = e1.recognize(audio, want_logits=True)
    print("%s mode %d: L=%d V=%d token_num=%s" % (kind, mode, r1.L, r1.V, r1.token_num.tolist()))
    assert r0.topk is None and r0.scores is None and r1.L >= 1
    # ids, logits, token_num bit-identical with the flag set and clear
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(r1.token_num, r0.token_num)
    np.testing.assert_array_equal(_bits(r1.logits), _bits(r0.logits))
    _check_topk(r1, 4)
    # scores as PF_DECODE_SCORES alone keeps them
    e0.set_decode(SCORES)
    np.testing.assert_array_equal(_bits(e0.recognize(audio).scores), _bits(r1.scores))
    # without want_logits: the same ids, scores and lists
    r2 = e1.recognize(audio)
    np.testing.assert_array_equal(r2.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r2.scores), _bits(r1.scores))
    np.testing.assert_array_equal(r2.topk.ids, r1.topk.ids)
    np.testing.assert_array_equal(_bits(r2.topk.val), _bits(r1.topk.val))
    np.testing.assert_array_equal(r2.topk.n, r1.topk.n)
    # K = 8 and K = 1
    for K in (8, 1):
        e1.set_topk(K)
        _check_topk(e1.recognize(audio, want_logits=True), K)
    # the flag cleared: nothing extra comes back, the ids stay
    e1.set_decode(0)
    r = e1.recognize(audio)
    assert r.topk is None and r.scores is None
    np.testing.assert_array_equal(r.token_ids, r0.token_ids)
    e0.close(); e1.close()


def test_engine_nbest_of_a_batch():
    """The n-best list from the engine's own lists: pf_host_nbest equals brute force on a window of positions, hypothesis 0
    is the 1-best, and positions at or beyond token_num never vary."""
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _pf_model()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    eng.set_decode(TOPK)
    eng.set_topk(3)
    r = eng.recognize(_pf_audio())
    B, L = r.token_ids.shape
    for b in range(B):
        n_free = min(L, int(r.token_num[b]))
        ranks, scores, hyp = host_nbest(r.topk.val[b], r.topk.n[b], n_free, 16, ids=r.topk.ids[b])
        assert len(ranks) == min(16, 3 ** n_free)
        np.testing.assert_array_equal(hyp[0], r.token_ids[b])
        assert (ranks[:, n_free:] == 0).all() and (np.diff(scores) <= 0).all()
        Lw = min(L, 5)                                                        # brute force over the first positions
        wr, ws = nbest_brute(r.topk.val[b, :Lw], r.topk.n[b, :Lw], min(n_free, Lw), 16)
        gr, gs = host_nbest(r.topk.val[b, :Lw], r.topk.n[b, :Lw], min(n_free, Lw), 16)
        assert [tuple(x) for x in gr.tolist()] == wr and gs.tolist() == ws
    eng.close()


# ---- 4: entry points -------------------------------------------------------------------------------------------------------
def _same_topk(a, b):
    np.testing.assert_array_equal(a.ids, b.ids)
    np.testing.assert_array_equal(_bits(a.val), _bits(b.val))
    np.testing.assert_array_equal(a.n, b.n)


def test_entry_points():
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _pf_model()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    eng.set_decode(TOPK)
    audio = _pf_audio()
    a = eng.recognize(audio, want_logits=True)                                 # pf_recognize
    _check_topk(a, 4)
    feats = [eng.frontend(x) for x in audio]
    m = eng.model_proj(feats, want_logits=True)                                # pf_model_proj
    _check_topk(m, 4)
    np.testing.assert_array_equal(m.token_ids, a.token_ids)
    _same_topk(m.topk, a.topk)
    T = max(f.shape[0] for f in feats)
    f = eng.forward_feats(fe.pad_sequence(feats).reshape(len(audio), T, -1), want_logits=True)    # pf_forward_feats
    _check_topk(f, 4)
    eng.stage_audio(audio)                                                     # pf_stage_audio + pf_run_staged + pf_fetch
    eng.run_staged()
    s = eng.fetch()
    np.testing.assert_array_equal(s.token_ids, a.token_ids)
    _same_topk(s.topk, a.topk)
    np.testing.assert_array_equal(_bits(s.scores), _bits(a.scores))
    eng.close()


def test_status_codes():
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _pf_model()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    lib, h = eng._lib, eng._h
    audio = _pf_audio()
    L, K = C.c_int32(), C.c_int32()
    eng.recognize(audio)
    assert lib.pf_fetch_topk(h, None, None, None, 0, L, K) == N.PF_ERR_INVALID_ARG        # the forward ran without the flag
    eng.set_decode(SCORES)
    eng.recognize(audio)
    assert lib.pf_fetch_topk(h, None, None, None, 0, L, K) == N.PF_ERR_INVALID_ARG
    for k in (0, 9, -1):
        assert lib.pf_engine_set_topk(h, k) == N.PF_ERR_INVALID_ARG
    assert lib.pf_engine_set_decode(h, TOPK | 64) == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        eng.set_decode(TOPK | CTC)                                                          # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_decode(TOPK)
    eng.set_topk(5)
    r = eng.recognize(audio)
    assert r.topk.K == 5 and r.scores is not None
    assert lib.pf_fetch_topk(h, None, None, None, 0, L, K) == N.PF_OK and (L.value, K.value) == (r.L, 5)
    rows = len(audio) * r.L
    ids = np.full((rows, 5), -7, np.int64)
    p = ids.ctypes.data_as(C.POINTER(C.c_int64))
    L.value = K.value = 0
    assert lib.pf_fetch_topk(h, p, None, None, rows - 1, L, K) == N.PF_ERR_CAPACITY
    assert (L.value, K.value) == (r.L, 5) and (ids == -7).all()                              # the sizes come with the error
    assert lib.pf_fetch_topk(h, p, None, None, rows, None, None) == N.PF_OK
    np.testing.assert_array_equal(ids.reshape(r.topk.ids.shape), r.topk.ids)
    _same_topk(eng.fetch_topk(len(audio)), r.topk)
    eng.close()


def test_seaco_refuses_the_flag():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        eng.set_decode(TOPK)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    eng.set_topk(8)                                                             # K alone is only a number
    eng.close()


# ---- 5: the recognizer mirror ------------------------------------------------------------------------------------------------
def _pf_dir(tmp_path):
    cfg, w = _pf_model()
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(61)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], toks


def _get(rec, audio):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        streams.append(s)
    rows = [4 + s.SpeechLength // 560 for s in streams]      # a SenseVoice stream's own rows (the prompt rows included)
    for s, n in zip(streams, rows):
        s.valid_rows = n
    return streams, rec.GetResults(streams)


def _alts_of(stream):
    ta = stream.TokenAlternatives
    ids = np.asarray([[p[0] for p in row] for row in ta], np.int64)
    val = np.asarray([[p[1] for p in row] for row in ta], np.float32)
    return ids, val


def test_recognizer_nbest(tmp_path):
    from aliparaformerasr_amd.engine import Engine
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, toks = _pf_dir(tmp_path)
    audio = _pf_audio()                                   # the third utterance fires fewer tokens than the batch's L
    NB, K = 12, 3
    plain, rec = OfflineRecognizer(*paths), OfflineRecognizer(*paths)
    rec.SetNBest(NB, K)
    s0, res0 = _get(plain, audio)
    s1, res1 = _get(rec, audio)
    # the same logits from an engine on the same container
    cfg, w = _pf_model()
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    r = eng.recognize(audio, want_logits=True)
    L = r.L
    want = topk_ref(r.logits, K)
    print("L=%d token_num=%s" % (L, r.token_num.tolist()))
    assert (r.token_num < L).any()
    for b in range(len(audio)):
        # Tokens, Timestamps, Scores and the text are what they are without the option
        assert s1[b].Tokens == s0[b].Tokens == r.token_ids[b].tolist()
        assert s1[b].Timestamps == s0[b].Timestamps and s1[b].Scores == s0[b].Scores == []
        assert (res1[b].Text, res1[b].Tokens, res1[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        assert s0[b].TokenAlternatives == [] and s0[b].Alternatives == []
        ids, val = _alts_of(s1[b])
        np.testing.assert_array_equal(ids, want[0][b])
        np.testing.assert_array_equal(_bits(val), _bits(want[1][b]))
        n_free = min(L, int(r.token_num[b]))
        ranks, scores, hyp = host_nbest(want[1][b], want[2][b], n_free, NB, ids=want[0][b])
        alts = s1[b].Alternatives
        assert len(alts) == len(ranks) == min(NB, K ** n_free)
        assert [a.Ids for a in alts] == hyp.tolist()
        assert [a.Score for a in alts] == scores.tolist()
        assert alts[0].Ids == s1[b].Tokens and (alts[0].Text, alts[0].Tokens) == (res1[b].Text, res1[b].Tokens)
        for a in alts:                                                         # the same DecodeMulti as the result
            text, _tlen, tk, _ = glue.decode_multi_one(toks, a.Ids, s1[b].Timestamps)
            assert (a.Text, a.Tokens) == (text, tk)
            assert a.Ids[n_free:] == s1[b].Tokens[n_free:]                     # nothing varies past the utterance's own count
        if len(alts) > 1:
            assert any(a.Ids != alts[0].Ids for a in alts[1:])
    # K alone (N = 1): token alternatives, no list; N = 0: everything off again
    rec.SetNBest(1, 2)
    s2, _ = _get(rec, audio)
    assert s2[0].Alternatives == [] and _alts_of(s2[0])[0].shape == (L, 2)
    np.testing.assert_array_equal(_alts_of(s2[0])[0], want[0][0][:, :2])
    rec.SetNBest(0)
    s3, res3 = _get(rec, audio)
    assert s3[0].TokenAlternatives == [] and s3[0].Alternatives == [] and res3[0].Text == res0[0].Text
    # with scores requested beside it, Scores stays the [L] row
    rec.SetDecode(scores=True)
    rec.SetNBest(4, 4)
    s4, _ = _get(rec, audio)
    np.testing.assert_array_equal(_bits(np.asarray(s4[0].Scores, np.float32)), _bits(_alts_of(s4[0])[1][:, 0]))
    assert len(s4[0].Alternatives) == 4
    for bad in ((65, 4), (-1, 4), (4, 9), (4, -1)):
        with pytest.raises(N.PfError) as ei:
            rec.SetNBest(*bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    eng.close()
    plain.Dispose(); rec.Dispose()


def test_recognizer_sensevoice_token_alternatives(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    cfg, w = _sv_model(sv_embed)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + ["<|tag%d|>" % i for i in range(20)] + [chr(0x4E00 + i) for i in range(SV_VOCAB - 24)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    paths = [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    r_frames, r_ctc, r_ref = (OfflineRecognizer(*paths) for _ in range(3))
    with pytest.raises(N.PfError) as ei:
        r_frames.SetNBest(2, 4)                                                 # an n-best list needs independent positions
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    r_frames.SetNBest(1, 4)                                                     # K alone is allowed
    r_frames.SetDecode(scores=True)
    r_ctc.SetDecode(ctc=True)
    r_ctc.SetNBest(1, 4)
    r_ref.SetDecode(ctc=True)
    sf, _ = _get(r_frames, audio)
    sc, resc = _get(r_ctc, audio)
    sr, resr = _get(r_ref, audio)
    for b in range(2):
        frames = np.asarray(sf[b].Tokens, np.int64)
        fs = np.asarray(sf[b].Scores, np.float32)
        f_ids, f_val = _alts_of(sf[b])                                          # without CTC: per frame
        assert f_ids.shape == (len(frames), 4) and sf[b].Alternatives == []
        np.testing.assert_array_equal(f_ids[:, 0], frames)
        np.testing.assert_array_equal(_bits(f_val[:, 0]), _bits(fs))
        assert (np.diff(f_val, axis=1) <= 0).all()
        # with CTC: Tokens / Timestamps / Scores / text as with CTC alone; per token the lists of the first frame of its
        # run whose score is the token's score bit for bit
        assert (sc[b].Tokens, sc[b].Timestamps, sc[b].Scores, resc[b].Text) == (sr[b].Tokens, sr[b].Timestamps, sr[b].Scores, resr[b].Text)
        n, ids, first, last, score = collapse_ref(frames[None], fs[None], [sc[b].valid_rows])
        k = int(n[0])
        assert sc[b].Tokens == ids[0, :k].tolist()
        t_ids, t_val = _alts_of(sc[b])
        assert t_ids.shape == (len(sc[b].Tokens), 4) and sc[b].Alternatives == []
        tok_sc = np.asarray(sc[b].Scores, np.float32)
        multi = 0
        for j in range(k):
            run = range(int(first[0, j]), int(last[0, j]) + 1)
            t = next(u for u in run if _bits(fs[u:u + 1])[0] == _bits(tok_sc[j:j + 1])[0])
            multi += len(run) > 1 and t != run[0]
            np.testing.assert_array_equal(t_ids[j], f_ids[t])
            np.testing.assert_array_equal(_bits(t_val[j]), _bits(f_val[t]))
            assert t_ids[j, 0] == sc[b].Tokens[j] and _bits(t_val[j, :1])[0] == _bits(tok_sc[j:j + 1])[0]
        print("stream %d: %d tokens, %d with their peak behind the run's first frame" % (b, k, multi))
    for r in (r_frames, r_ctc, r_ref):
        r.Dispose()


def test_two_threads_on_one_recognizer(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, _ = _pf_dir(tmp_path)
    rec = OfflineRecognizer(*paths)
    rec.SetNBest(6, 3)
    batches = [_pf_audio()[:2], [W.synth_audio(26000, 91)]]

    def snapshot(streams, res):
        return [(r.Text, s.Tokens, s.TokenAlternatives, [(a.Ids, a.Score, a.Text) for a in s.Alternatives]) for s, r in zip(streams, res)]
    want = [snapshot(*_get(rec, b)) for b in batches]
    assert want[0][0][3] != want[1][0][3] and len(want[0][0][3]) == 6
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


def test_cli_prints_n_lines(tmp_path):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "m"
    d.mkdir()
    _pf_dir(d)
    pcm = (np.clip(W.synth_audio(32000, 40), -1, 1) * 32767).astype("<i2")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    for method in ("one", "batch"):
        out = io.StringIO()
        res = ex.offline_recognizer(method=method, model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=5, topk=3)
        lines = out.getvalue().splitlines()
        nb = [ln for ln in lines if ln.startswith("nbest[")]
        assert len(res) == 1 and len(nb) == 5, out.getvalue()
        assert [ln.split("]")[0] for ln in nb] == ["nbest[%d" % i for i in range(5)]
        at = lines.index(nb[0])
        assert lines[at - 1].startswith('{"text": "%s"' % res[0].Text)           # under the usual result line
        assert nb[0].endswith("text:" + res[0].Text)
        sc = [float(ln.split("score:")[1].split(" ")[0]) for ln in nb]
        assert sc == sorted(sc, reverse=True)
    out = io.StringIO()
    ex.offline_recognizer(method="one", model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out)
    assert "nbest[" not in out.getvalue()
