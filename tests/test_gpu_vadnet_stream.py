"""GPU: the streaming FSMN-VAD model score (csrc/k_vadnet_stream.hip; Engine.op_vad_model_stream,
OnlineRecognizer.SetEndpointModel) — B streams per launch, each stream's history carried between calls in its state block.

No tolerance anywhere: the streaming levels and logits are DEFINED as the offline kernel's (csrc/k_vadnet.hip) over the whole
stream, released under the schedule of tests/vadnet_stream_ref.py, and both kernels run the same device functions
(csrc/vadnet_dev.h), so the comparison is on the bits.  The offline kernel is held to float64 by tests/test_gpu_vadnet.py; the
exact-answer test below holds this kernel to the float64 definition without going through the offline one.

Shapes: streams of MIXED_BATCH = [5, 0, 70, 1, 131] frames in one launch, fed n_new from {0, 1, 2, 3, 59, 60, 63, 64, 65} in a
rotation that differs per stream (a call's tile walk is 0, 1 or 2 tiles; 63 / 64 / 65 sit on the tile edge), one stream flushed
with its last rows while the others go on, the others by a call without rows.  Two models: the released dimensions and the small
awkward one of vadnet_ref (every dimension padded, lstride 2)."""
import ctypes as C

import numpy as np
import pytest

import endpoint_ref as EP
import vad_ref as V
import vadnet_ref as R
import vadnet_stream_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd import engine as E
from oracle import frontend as fe

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 3, 59, 60, 63, 64, 65]


@pytest.fixture(scope="module")
def eng80():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    """a front-end of 8 mel bins, for the small model (only the front-end geometry matters here: no forward runs)"""
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(56), device=0, n_mels=8)
    yield e
    e.close()


def _attach(eng, cfg, w):
    m = E.load_vad_model(W.pack_pfw(cfg, w))
    eng.set_vad_model(m)
    return m


def _engine_for(name, eng80, eng8):
    return eng80 if name == "released" else eng8


def _base(name):
    return {} if name == "released" else R.SMALL


def _plan(Ts, rot, flush_with_rows=(0,)):
    """the calls of a run: [(n_new [B], flush [B])].  Stream b's k-th call brings SIZES[(k + 2 b + 1 + rot) % 9] rows, cut to
    what it has left.  A stream in flush_with_rows is flushed in the call that brings its last rows (midway: the others go on),
    every other one by a later call that brings it nothing."""
    left, done, calls, k = list(Ts), [False] * len(Ts), [], 0
    while not all(done):
        n_new, flush = [], []
        for b in range(len(Ts)):
            c = 0 if done[b] else min(SIZES[(k + 2 * b + 1 + rot) % 9], left[b])
            f = (not done[b]) and ((left[b] == 0) or (b in flush_with_rows and c == left[b]))
            left[b] -= c
            done[b] = done[b] or f
            n_new.append(c); flush.append(f)
        calls.append((n_new, flush))
        k += 1
    return calls


def _run(eng, m, rows, calls, states=None, want_logits=True):
    """feeds the plan; returns per stream the concatenated levels and logits, the released counts per call, the final states"""
    B = len(rows)
    states = E.vad_model_stream_state(m, B) if states is None else states
    at, lev, z, cnt = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)], []
    for n_new, flush in calls:
        piece = [rows[b][at[b]: at[b] + n_new[b]] for b in range(B)]
        e, g = eng.op_vad_model_stream(states, piece, flush, want_logits=want_logits)
        cnt.append([len(x) for x in e])
        for b in range(B):
            at[b] += n_new[b]
            lev[b].append(e[b])
            if want_logits:
                z[b].append(g[b])
    O = m.dims["output_dim"]
    return ([np.concatenate(x) for x in lev], [np.concatenate(x).reshape(-1, O) for x in z] if want_logits else None, cnt, states)


# ---- 1: bit equality with the offline op ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seeds", [("released", (6, 7, 8)), ("small", (5, 6, 7))])
def test_bit_equal_to_the_offline_kernel(name, seeds, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    for seed in seeds:
        cfg, w = (R.released_model if name == "released" else R.small_model)(seed)
        rows = [R.fbank_like(T, cfg["n_mels"], 100 * seed + T) for T in R.MIXED_BATCH]
        calls = _plan(R.MIXED_BATCH, seed)
        used = {c for n_new, _ in calls for c in n_new}
        assert len(calls) >= 5 and len(used & set(SIZES)) >= 6, calls
        assert any(f[0] and n[0] > 0 and not all(fl) for n, f in calls for fl in [f])      # stream 0: flushed midway, with rows
        m = _attach(eng, cfg, w)
        try:
            want_z, want_e = eng.op_vad_model_logits(rows), eng.op_vad_model_levels(rows)
            lev, z, cnt, _ = _run(eng, m, rows, calls)
        finally:
            eng.set_vad_model(None)
            m.close()
        # the counts are the schedule's
        for b in range(len(rows)):
            fl_at = min(k for k, (_, f) in enumerate(calls) if f[b])
            assert [c[b] for c in cnt] == S.counts(cfg, [n[b] for n, _ in calls], flush_at=fl_at), (name, seed, b)
        for b, T in enumerate(R.MIXED_BATCH):
            assert z[b].shape == (T, cfg["output_dim"]) and lev[b].shape == (T,) and lev[b].dtype == np.int32
            np.testing.assert_array_equal(z[b].view(np.uint32), want_z[b].view(np.uint32), err_msg=str((name, seed, b)))
            np.testing.assert_array_equal(lev[b], want_e[b], err_msg=str((name, seed, b)))
        assert float(np.abs(want_z[4]).max()) > 0.1                      # not a trivial answer


# ---- 2: exact answers, without the offline kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "released"])
def test_exact_logits_in_chunks(name, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    cfg, w = R.exact_model(_base(name), seed=1)
    rows = [R.exact_rows(T, cfg["n_mels"], 7 * b + T) for b, T in enumerate(R.MIXED_BATCH)]
    want = []
    for x in rows:
        worst, integral = R.exact_worst(cfg, w, x)
        assert worst < 2048 and integral                                # the premise: nothing is lost in any rounding
        want.append(R.logits(cfg, w, x).astype(np.float32))
    m = _attach(eng, cfg, w)
    try:
        for rot in (0, 4):
            lev, z, cnt, _ = _run(eng, m, rows, _plan(R.MIXED_BATCH, rot))
            for b in range(len(rows)):
                assert z[b].shape == want[b].shape
                np.testing.assert_array_equal(z[b], want[b], err_msg=str((name, rot, b)))           # (no tolerance; -0 == 0)
                d = np.abs(lev[b].astype(np.int64) - R.levels_from_logits(cfg, z[b]))
                assert (d <= 1).all()                                   # the fp32 softmax against float64: test_gpu_vadnet.py
    finally:
        eng.set_vad_model(None)
        m.close()
    assert max(float(np.abs(z).max()) for z in want if z.size) > 30


# ---- 3: poison ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "released"])
def test_poison_reaches_the_frames_the_definition_names_across_calls(name, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    cfg, w = R.exact_model(_base(name), seed=2)
    rows = [R.exact_rows(T, cfg["n_mels"], 50 + b) for b, T in enumerate(R.MIXED_BATCH)]
    rows[2][10, :] = np.nan
    rows[2][10, 1::3] = np.inf
    rows[2][10, 2::3] = -np.inf
    want = [R.logits(cfg, w, x).astype(np.float32) for x in rows]
    bad = ~np.isfinite(want[2]).all(axis=1)
    # stream 2 in calls of 12, 3, 20 and 35 rows: frame 10 arrives in call 0, which releases levels 0 .. 9; levels 10 .. 12 see it
    # through the row tail, everything behind through the carried history
    chunks2 = [12, 3, 20, 35]
    calls = []
    for k, c in enumerate(chunks2):
        calls.append(([5 if k == 0 else 0, 0, c, 1 if k == 1 else 0, [60, 65, 6, 0][k]], [k == 0, False, False, k == 1, False]))
    calls.append(([0] * 5, [False, True, True, False, True]))
    first_later = S.released(cfg, 12, False)
    assert bad[8:13].all() and not bad[:8].any() and bad[first_later:].any() and bad.sum() < 70
    assert not (bad & ~S.poisoned_levels(cfg, 70, [10])).any()
    m = _attach(eng, cfg, w)
    try:
        lev, z, cnt, _ = _run(eng, m, rows, calls)
    finally:
        eng.set_vad_model(None)
        m.close()
    for b in range(len(rows)):
        fin = np.isfinite(want[b])
        assert z[b].shape == want[b].shape and (np.isfinite(z[b]) == fin).all(), b
        np.testing.assert_array_equal(z[b][fin], want[b][fin])
        if b != 2:
            assert fin.all()                                            # no other stream is touched
    assert (lev[2][bad] == -16384).all()                                # a frame whose softmax is not finite is silence
    np.testing.assert_array_less(np.abs(lev[2][~bad].astype(np.int64) - R.levels_from_logits(cfg, z[2][~bad])), 2)


# ---- 4: isolation ---------------------------------------------------------------------------------------------------------------
def test_streams_do_not_see_each_other(eng8, eng80):
    for name, eng in (("small", eng8), ("released", eng80)):
        cfg, w = (R.released_model if name == "released" else R.small_model)(6)
        rows = [R.fbank_like(T, cfg["n_mels"], 300 + T) for T in R.MIXED_BATCH]
        calls = _plan(R.MIXED_BATCH, 2)
        m = _attach(eng, cfg, w)
        try:
            lev, z, _, st = _run(eng, m, rows, calls)
            # stream 2: other rows, and a state that is not fresh (40 frames of something else went in before)
            other = list(rows)
            other[2] = R.fbank_like(70, cfg["n_mels"], 999) * 5
            st0 = E.vad_model_stream_state(m, len(rows))
            warm = st0[2:3].copy()
            eng.op_vad_model_stream(warm, [R.fbank_like(40, cfg["n_mels"], 1)], None)
            st0[2] = warm[0]
            lev2, z2, _, st2 = _run(eng, m, other, calls, states=st0)
        finally:
            eng.set_vad_model(None)
            m.close()
        assert not np.array_equal(z[2].view(np.uint32), z2[2][: z[2].shape[0]].view(np.uint32))
        for b in (0, 1, 3, 4):
            np.testing.assert_array_equal(z[b].view(np.uint32), z2[b].view(np.uint32))
            np.testing.assert_array_equal(lev[b], lev2[b])
            assert (st[b] == st2[b]).all(), (name, b)
        assert not st[1][:-4].any() and st[1][-4] == 1                   # a stream that never got a row: the flushed flag alone
        assert not (st[2] == st2[2]).all()


# ---- 5: launch count, ordering, state and error rules -----------------------------------------------------------------------------
def test_one_launch_whatever_B_and_any_stream_order(eng80):
    eng = eng80
    cfg, w = R.released_model(7)
    m = _attach(eng, cfg, w)
    try:
        for B in (1, 70):
            n_new = [(3 * b) % 7 + (64 if b == 5 else 0) for b in range(B)]      # 0 .. 6 rows, one stream with two tiles
            rows = [R.fbank_like(n, 80, 10 + b) for b, n in enumerate(n_new)]
            warm = [R.fbank_like(4 + b % 3, 80, 500 + b) for b in range(B)]
            flush = [b % 4 == 1 for b in range(B)]
            st = E.vad_model_stream_state(m, B)
            eng.op_vad_model_stream(st, warm, None)
            eng.profile(True)
            eng.profile_reset()
            sa = st.copy()
            la, za = eng.op_vad_model_stream(sa, rows, flush)
            _, launches, _ = eng.profile_get("vadnet_stream")
            assert launches == 1, (B, launches)
            assert eng.profile_get("vadnet")[1] == 0
            eng.profile(False)
            # the same streams listed in another order
            perm = np.random.default_rng(B).permutation(B)
            sb = np.ascontiguousarray(st[perm])
            lb, zb = eng.op_vad_model_stream(sb, [rows[p] for p in perm], [flush[p] for p in perm])
            for k, p in enumerate(perm):
                np.testing.assert_array_equal(za[p].view(np.uint32), zb[k].view(np.uint32))
                np.testing.assert_array_equal(la[p], lb[k])
                assert (sa[p] == sb[k]).all()
            for b in range(B):
                n0 = warm[b].shape[0]
                assert len(la[b]) == S.released(cfg, n0 + n_new[b], flush[b]) - S.released(cfg, n0, False)
    finally:
        eng.set_vad_model(None)
        m.close()


def test_state_and_error_rules_of_the_op(eng8, eng80):
    cfg, w = R.small_model(5)
    m = _attach(eng8, cfg, w)
    try:
        x = R.fbank_like(30, 8, 4)
        st = E.vad_model_stream_state(m, 2)
        assert st.shape[1] % 16 == 0 and not st.any()
        eng8.op_vad_model_stream(st, [x[:10], x[:7]], None)
        before = st.copy()
        e, _ = eng8.op_vad_model_stream(st, [x[:0], x[:0]], None)       # n_new = 0 without a flush: no byte changes
        assert [len(v) for v in e] == [0, 0] and (st == before).all()
        with pytest.raises(N.PfError) as ei:                            # too small a capacity: nothing launched, nothing changed
            eng8.op_vad_model_stream(st, [x[10:20], x[:0]], None, cap=3)
        assert ei.value.code == N.PF_ERR_CAPACITY and (st == before).all()
        e, _ = eng8.op_vad_model_stream(st, [x[10:20], x[:0]], [True, False])
        assert [len(v) for v in e] == [12, 0]
        flushed = st.copy()
        assert (flushed[1] == before[1]).all()
        e, _ = eng8.op_vad_model_stream(st, [x[:0], x[:0]], [True, False])      # a second flush without frames is a no-op
        assert [len(v) for v in e] == [0, 0] and (st == flushed).all()
        eng8.profile(True)
        eng8.profile_reset()
        with pytest.raises(N.PfError) as ei:                            # frames after a flush: nothing is launched
            eng8.op_vad_model_stream(st, [x[20:21], x[7:9]], None)
        assert ei.value.code == N.PF_ERR_INVALID_ARG and (st == flushed).all()
        assert eng8.profile_get("vadnet_stream")[1] == 0
        eng8.profile(False)
        big = flushed.copy()
        big[1, -8:].view(np.int32)[0] = N.PF_ENDPOINT_MAX_STREAM_FRAMES - 1
        keep = big.copy()
        with pytest.raises(N.PfError) as ei:
            eng8.op_vad_model_stream(big, [x[:0], x[:2]], None)
        assert ei.value.code == N.PF_ERR_CAPACITY and (big == keep).all()
    finally:
        eng8.set_vad_model(None)
        m.close()
    with pytest.raises(N.PfError) as ei:                                # no model attached
        eng8.op_vad_model_stream(np.zeros((1, 16), np.uint8), [np.zeros((1, 8), np.float32)], None)
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    # a model whose window does not fit the LDS is refused for streaming (it still serves the offline path)
    wide = W.fsmn_vad_config(lorder=129, lstride=2, proj_dim=256)
    mw = E.load_vad_model(W.pack_pfw(wide, W.synth_vad_weights(wide, 1)))
    eng80.set_vad_model(mw)
    try:
        with pytest.raises(N.PfError) as ei:
            eng80.op_vad_model_stream(E.vad_model_stream_state(mw, 1), [np.zeros((1, 80), np.float32)], None)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    finally:
        eng80.set_vad_model(None)
        mw.close()


# ---- 6: the recognizer ------------------------------------------------------------------------------------------------------------
VOCAB = 300
STEP = 4000
CHUNK = 9600
BURSTS = [[(100, 250), (400, 600)], [(50, 250), (400, 500), (600, 700)], [(100, 300), (650, 800)]]
KIND = {EP.SILENCE: "silence", EP.FORCED: "forced", EP.FLUSH: "flush"}
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
    on, off = tmp_path_factory.mktemp("epm_online"), tmp_path_factory.mktemp("epm_offline")
    cfg = W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=VOCAB)
    w = W.synth_weights(cfg, seed=31)
    w["predictor.out.bias"] = np.asarray([0.8], np.float32)          # ~0.6 per frame: a few tokens per 10-frame chunk
    _write(on, cfg, w, "model: paraformer\n")
    ocfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB)
    _write(off, ocfg, W.synth_weights(ocfg, seed=77), "model: paraformer\nuse_itn: false\n")
    return on, off


@pytest.fixture(scope="module")
def audio():
    a = [V.burst_audio(8, b, 40 + i) for i, b in enumerate(BURSTS)]
    a[2] = a[2][:127900]                                              # 799.4 frames: no multiple of 160 samples
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


def _caller_rows(rec, a):
    """the fbank rows of the caller's frames: per 9600-sample chunk (the last one zero-padded) the rows of the engine's own fbank
    op, of which the first ceil(samples / 160) are the caller's"""
    lib, h = N.load(), C.c_void_p(rec.engine_handle())
    out = []
    for off in range(0, len(a), CHUNK):
        piece = a[off: off + CHUNK]
        x = np.zeros(CHUNK, np.float32)
        x[: len(piece)] = piece
        rows, t = np.zeros((CHUNK // 160 + 2) * 80, np.float32), C.c_int32()
        N.check(lib.pf_fbank(h, x.ctypes.data_as(C.POINTER(C.c_float)), CHUNK, rows.ctypes.data_as(C.POINTER(C.c_float)), rows.size, t))
        assert t.value == 60
        out.append(rows[: 60 * 80].reshape(60, 80)[: (len(piece) + 159) // 160].copy())
    return np.concatenate(out)


def _offline_levels(rec, rows):
    """the offline op (k_vadnet.hip) of the recognizer's own engine, with the model the recognizer attached"""
    lib, h = N.load(), C.c_void_p(rec.engine_handle())
    x = np.ascontiguousarray(rows, np.float32)
    T, out = np.asarray([x.shape[0]], np.int32), np.zeros(x.shape[0], np.int32)
    N.check(lib.pf_op_vad_model_levels(h, x.ctypes.data_as(C.POINTER(C.c_float)), T.ctypes.data_as(C.POINTER(C.c_int32)), 1, 80,
                                       out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _feed(rec, streams, audio, finish=True):
    """4000-sample pieces to every stream, a GetResults per round; then InputFinished and the calls that drain the chunks.
    Returns, per call, the number of sentences every stream has after it."""
    counts = []
    for off in range(0, max(len(a) for a in audio), STEP):
        for s, a in zip(streams, audio):
            if off < len(a):
                s.AddSamples(a[off: off + STEP])
        rec.GetResults(streams)
        counts.append([len(s.Sentences) for s in streams])
    if finish:
        for s in streams:
            s.InputFinished()
        for _ in range(3):
            rec.GetResults(streams)
            counts.append([len(s.Sentences) for s in streams])
    return counts


def _detector_calls(n_samples, n_rounds, n_after=3):
    """What a stream hands the detector at every GetResults of _feed, restated from the stream's rules (csrc/online.cpp): a
    chunk of 9600 samples leaves the cache once MORE than 9600 are cached, one per AddSamples; the first chunk is the
    constructor's silence and brings the detector nothing; the first fbank row is repeated once in the decoder's queue; a
    GetResults decodes one 60-frame chunk per stream; InputFinished sends every cached chunk on, the last one zero-padded, of
    which the caller's ceil(samples / 160) rows go to the detector; the flush comes with the first GetResults after it that
    leaves less than a chunk undecoded.  Returns [(rows, flush)] per call."""
    q = dict(cache=CHUNK, chunks_in=0, speech=0, pending=0, fed=False, flushed=False)
    calls = []

    def input_speech(n_caller):
        if n_caller > 0:
            q["pending"] += min((n_caller + 159) // 160, 60)
            q["fed"] = True
        q["speech"] += 60 + (1 if q["chunks_in"] == 0 else 0)
        q["chunks_in"] += 1

    def get_results(finished):
        if q["speech"] >= 60:
            q["speech"] -= 60
        if q["flushed"]:
            calls.append((0, False))
            return
        fl = finished and q["cache"] == 0 and q["speech"] < 60 and q["fed"]
        calls.append((q["pending"], fl))
        q["pending"] = 0
        q["flushed"] = fl
    for k in range(n_rounds):
        if k * STEP < n_samples:
            q["cache"] += min(STEP, n_samples - k * STEP)
            if q["cache"] > CHUNK:
                q["cache"] -= CHUNK
                input_speech(0 if q["chunks_in"] == 0 else CHUNK)
        get_results(False)
    while q["cache"] > 0:
        take = min(CHUNK, q["cache"])
        q["cache"] -= take
        input_speech(0 if q["chunks_in"] == 0 else take)
    for _ in range(n_after):
        get_results(True)
    return calls


@pytest.fixture(scope="module")
def run(models, audio, tmp_path_factory):
    """ONE pass with the model endpoint and the second pass on, shared by the tests that only read it"""
    rec, off = _online(models), _offline(models)
    rows0 = _caller_rows(rec, audio[0])
    cfg, w = R.energy_model(rows0)
    path = str(tmp_path_factory.mktemp("epm_vad") / "vad.pfw")
    W.save_pfw(path, cfg, w)
    rec.SetEndpointModel(path)
    rec.SetEndpoint(E.endpoint_model_config())
    rec.SetSecondPass(off)
    streams = [rec.CreateOnlineStream() for _ in audio]
    counts = _feed(rec, streams, audio)
    yield rec, streams, [s.Sentences for s in streams], counts, (cfg, w, path)
    rec.Dispose(); off.Dispose()


def test_recognizer_sentences_and_their_calls_follow_the_schedule(run, audio):
    rec, streams, sentences, counts, (cfg, w, path) = run
    c = EP.config(rise=-1, abs_level=9830)
    n_rounds = (max(len(a) for a in audio) + STEP - 1) // STEP
    total = 0
    for i, a in enumerate(audio):
        rows = _caller_rows(rec, a)
        T = rows.shape[0]
        assert T == (len(a) + 159) // 160 == 800
        lev = _offline_levels(rec, rows)                               # over the whole stream: what every released level must be
        calls = _detector_calls(len(a), n_rounds)
        assert len(calls) == len(counts) and sum(n for n, _ in calls) == T and sum(f for _, f in calls) == 1
        # the detector over the released levels, call by call
        st, want, want_counts, n, rel, flushed = EP.new_state(), [], [], 0, 0, False
        for n_new, fl in calls:
            n += n_new
            flushed = flushed or fl
            now = S.released(cfg, n, flushed)
            ev, _, _ = EP.update(st, lev[rel: now], fl, 80, c)
            rel = now
            want += [tuple(int(v) for v in e) for e in ev]
            want_counts.append(len(want))
        assert rel == T
        got = [(s.begin_ms, s.end_ms, s.kind) for s in sentences[i]]
        assert got == [(10 * b, 10 * e, KIND[k]) for b, e, k in want], i
        assert [cnt[i] for cnt in counts] == want_counts, i             # ... and the call each of them appeared in
        total += len(got)
        # the event list itself does not depend on the schedule: the state machine sees the same levels in the same order
        assert [tuple(int(v) for v in e) for e in EP.run(lev, 80, c, flush=True)[0]] == want
    assert total >= 3 and all(len(s) >= 1 for s in sentences)          # the constructed model finds the bursts
    assert counts[-1] == counts[-2]                                     # nothing comes after the flush


def test_recognizer_second_pass_is_unchanged(run, models, audio):
    rec, streams, sentences, counts, _ = run
    rp = _offline(models)
    prev, n_batches = [0, 0, 0], 0
    for now in counts:
        pool = [(i, j) for i in range(3) for j in range(prev[i], now[i])]        # the call's stream order, then time order
        prev = now
        if not pool:
            continue
        n_batches += 1
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
            assert s.result is not None and s.result.Tokens == p.Tokens and len(p.Tokens) > 0, (i, j)
            assert s.result.Timestamps == p.Timestamps and s.text == pr.Text, (i, j)
            assert np.asarray(s.result.Scores, np.float32).view(np.uint32).tolist() == np.asarray(p.Scores, np.float32).view(np.uint32).tolist()
    assert n_batches >= 2
    rp.Dispose()


def test_recognizer_attach_then_detach_is_the_energy_endpoint_and_late_attach_is_refused(run, models, audio):
    path = run[4][2]
    ra, rb = _online(models), _online(models)
    ra.SetEndpointModel(path)
    ra.SetEndpointModel(None)                                          # before any stream fed the detector
    ra.SetEndpoint(end_silence=40)
    rb.SetEndpoint(end_silence=40)
    short = [a[:64000] for a in audio[:2]]
    sa, sb = [ra.CreateOnlineStream() for _ in short], [rb.CreateOnlineStream() for _ in short]
    ca, cb = _feed(ra, sa, short, finish=False), _feed(rb, sb, short, finish=False)
    assert ca == cb and ca[-1] != [0, 0]
    for u in range(2):
        assert [(s.begin_ms, s.end_ms, s.kind, s.first_pass) for s in sa[u].Sentences] == \
               [(s.begin_ms, s.end_ms, s.kind, s.first_pass) for s in sb[u].Sentences]
        assert sa[u].Tokens == sb[u].Tokens and sa[u].InSpeech == sb[u].InSpeech
    # live streams have fed the detector: neither attaching ...
    with pytest.raises(N.PfError) as ei:
        ra.SetEndpointModel(path)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    # ... nor, on the recognizer that runs the model, detaching
    with pytest.raises(N.PfError) as ei:
        run[0].SetEndpointModel(None)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    # a file that is no such container; a missing file
    with pytest.raises(N.PfError) as ei:
        rb.SetEndpointModel(str(models[0] / "model.pfw"))
    assert ei.value.code in (N.PF_ERR_INVALID_ARG, N.PF_ERR_UNSUPPORTED)
    with pytest.raises(N.PfError):
        rb.SetEndpointModel(str(models[0] / "missing.pfw"))
    ra.Dispose(); rb.Dispose()
