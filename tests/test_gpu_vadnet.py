"""GPU: the FSMN-VAD model score on the device (csrc/k_vadnet.hip; Engine.set_vad_model / op_vad_model_logits /
op_vad_model_levels / vad_segment, OfflineRecognizer.SetVadModel) against the definition in numpy float64
(tests/vadnet_ref.py).

Shapes: the kernel serves 64-row tiles, so utterances of 0, 1, 2, 3, lorder - 1, lorder, lorder + 1, 63, 64, 65 and 131 frames
go through it alone and all in one call, and the batch T = [5, 0, 70, 1, 131] puts utterance boundaries inside tiles.  Two
models: the released dimensions (400 / 140 / 250 / 128 / 248, 4 layers, lorder 20) and a small awkward one (n_mels 8, 12 / 20 /
16 / 5, lorder 3, lstride 2, 2 layers, two silence ids) on which every dimension is padded.

Tolerances.
  * exact-answer inputs (vadnet_ref.exact_model): none; the logits are bit-equal to the float64 answer.
  * level from logits: |e - rint((1 - 2 s) 16384)| <= 1 with s in float64 from the device's own logits.  Derived, not measured:
    an fp32 softmax over <= 256 terms is off by < 1.6e-5 relative, that is < 0.53 after the factor 32768, plus the rounding.
  * random weights: the numpy emulation of the kernel's float16 rounding points (vadnet_ref.emulate_f16) deviates from the
    float64 definition by at most 1.35e-3 (released dimensions, seeds 6-8) and 1.95e-3 (small model, seeds 5-7) on logits of
    magnitude <= 2.1, measured on the CPU over the inputs of this file; the device gets 4x the deviation measured at run time
    (asserted to stay inside those figures): the accumulation order differs, and a misplaced row or tile is off by O(1).
    Measured on an MI355X: 1.30e-3 .. 1.36e-3 (released), 1.30e-3 .. 1.95e-3 (small), i.e. at most 1.2x the emulation."""
import os

import numpy as np
import pytest

import vad_ref as V
import vadnet_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd import engine as E

pytestmark = pytest.mark.gpu
EMU_DEV = {"released": 1.35e-3, "small": 1.95e-3}                  # the recorded CPU figures (see above)


@pytest.fixture(scope="module")
def eng80():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    """a front-end of 8 mel bins, for the small model (only the front-end geometry matters to the detector: no forward runs)"""
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


def _lengths(name):
    return R.LENGTHS_RELEASED if name == "released" else R.LENGTHS_SMALL


def _base(name):
    return {} if name == "released" else R.SMALL


# ---- exact answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "released"])
def test_exact_logits_on_every_shape(name, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    cfg, w = R.exact_model(_base(name), seed=1)
    m = _attach(eng, cfg, w)
    try:
        n_mels = cfg["n_mels"]
        calls = [[T] for T in _lengths(name)] + [_lengths(name), R.MIXED_BATCH, [64, 64], [1] * 32]
        largest = 0.0
        for ci, Ts in enumerate(calls):
            rows = [R.exact_rows(T, n_mels, 1000 * ci + 7 * b + T) for b, T in enumerate(Ts)]
            want = []
            for x in rows:
                worst, integral = R.exact_worst(cfg, w, x)
                assert worst < 2048 and integral                        # the premise: nothing is lost in any rounding
                want.append(R.logits(cfg, w, x).astype(np.float32))
            got = eng.op_vad_model_logits(rows)
            for b, (g, z) in enumerate(zip(got, want)):
                assert g.shape == z.shape
                np.testing.assert_array_equal(g, z, err_msg=str((name, Ts, b)))        # (no tolerance; -0 == 0)
            largest = max([largest] + [float(np.abs(z).max()) for z in want if z.size])
        assert largest > 30                                             # not a trivial answer
    finally:
        eng.set_vad_model(None)
        m.close()


@pytest.mark.parametrize("name", ["small", "released"])
def test_poison_reaches_only_the_frames_the_definition_says(name, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    cfg, w = R.exact_model(_base(name), seed=2)
    m = _attach(eng, cfg, w)
    try:
        n_mels = cfg["n_mels"]
        rows = [R.exact_rows(T, n_mels, 50 + b) for b, T in enumerate(R.MIXED_BATCH)]
        rows[2][10, :] = np.nan
        rows[2][10, 1::3] = np.inf
        rows[2][10, 2::3] = -np.inf
        want = [R.logits(cfg, w, x).astype(np.float32) for x in rows]
        got = eng.op_vad_model_logits(rows)
        lev = eng.op_vad_model_levels(rows)
        bad = ~np.isfinite(want[2]).all(axis=1)
        reach = (cfg["lorder"] - 1) * cfg["lstride"] * cfg["n_layers"]
        assert bad[8:13].all() and not bad[:8].any() and not bad[13 + reach:].any() and bad.sum() < 70
        for b in range(len(rows)):
            fin = np.isfinite(want[b])
            assert (np.isfinite(got[b]) == fin).all(), b
            np.testing.assert_array_equal(got[b][fin], want[b][fin])
            if b != 2:
                assert fin.all()
        # a frame whose softmax is not finite is silence
        assert (lev[2][bad] == -16384).all()
        np.testing.assert_array_less(np.abs(lev[2][~bad].astype(np.int64) - R.levels_from_logits(cfg, got[2][~bad])), 2)
    finally:
        eng.set_vad_model(None)
        m.close()


# ---- random weights ------------------------------------------------------------------------------------------------------
def _random_case(name, seed):
    cfg, w = (R.released_model if name == "released" else R.small_model)(seed)
    rows = [R.fbank_like(T, cfg["n_mels"], 100 * seed + T) for T in R.MIXED_BATCH + [300]]
    return cfg, w, rows


@pytest.mark.parametrize("name,seeds", [("released", (6, 7, 8)), ("small", (5, 6, 7))])
def test_random_weights_logits_and_levels(name, seeds, eng80, eng8):
    eng = _engine_for(name, eng80, eng8)
    for seed in seeds:
        cfg, w, rows = _random_case(name, seed)
        want = [R.logits(cfg, w, x) for x in rows]
        emu = max(float(np.abs(R.emulate_f16(cfg, w, x) - z).max()) for x, z in zip(rows, want) if z.size)
        assert 0 < emu <= EMU_DEV[name], (name, seed, emu)             # the figure recorded in this file still holds
        m = _attach(eng, cfg, w)
        try:
            got = eng.op_vad_model_logits(rows)
            lev = eng.op_vad_model_levels(rows)
            alone = eng.op_vad_model_logits([rows[2]])[0]
        finally:
            eng.set_vad_model(None)
            m.close()
        dev = max(float(np.abs(g.astype(np.float64) - z).max()) for g, z in zip(got, want) if z.size)
        print("vadnet %s seed %d: emulation %.3e, device %.3e (allowed %.3e)" % (name, seed, emu, dev, 4 * emu))
        assert dev <= 4 * emu, (name, seed, dev, emu)
        # the level from the device's own logits
        for g, e in zip(got, lev):
            d = np.abs(e.astype(np.int64) - R.levels_from_logits(cfg, g))
            assert e.dtype == np.int32 and (d <= 1).all(), (name, seed, int(d.max()))
            assert (np.abs(e) <= 16384).all()
        # an utterance's result does not depend on its batch mates
        np.testing.assert_array_equal(alone.view(np.uint32), got[2].view(np.uint32))


# ---- end to end ------------------------------------------------------------------------------------------------------------
BURSTS = [(200, 500), (800, 1000), (1400, 1800)]


def _pairs(a):
    return [tuple(p) for p in np.asarray(a).tolist()]


def test_end_to_end_segments_profile_and_detach(eng80):
    eng = eng80
    audio = [V.burst_audio(20, BURSTS, 1), V.burst_audio(7, [(100, 400)], 2), np.zeros(0, np.float32)]
    rows = eng.op_fbank_batch(audio)
    assert [r.shape[0] for r in rows] == [2000, 700, 0]
    before = eng.vad_segment(audio)                                    # the energy form, never having had a model
    cfg, w = R.energy_model(rows[0])
    vc = E.vad_model_config()
    assert (vc.floor_pct, vc.abs_level) == (-1, 9830)
    vref = V.config(floor_pct=-1, abs_level=9830)
    m = _attach(eng, cfg, w)
    try:
        dev_levels = eng.op_vad_model_levels(rows)
        eng.profile(True)
        eng.profile_reset()
        got = eng.vad_segment(audio, vc)
        _, net_n, _ = eng.profile_get("vadnet")
        _, vad_n, _ = eng.profile_get("vad")
        _, fb_n, _ = eng.profile_get("fbank")
        eng.profile(False)
        assert (net_n, vad_n, fb_n) == (1 + cfg["n_layers"], 1, 1)
        # exactly steps 2-6 over the device's own levels
        assert [_pairs(g) for g in got] == [_pairs(E.host_vad_segments(e, 80, vc)) for e in dev_levels]
        # and the definition's segments, where the reference says the comparison is valid
        ref_levels = [R.levels(cfg, w, r) for r in rows]
        worst = max(int(np.abs(d.astype(np.int64) - r).max()) for d, r in zip(dev_levels, ref_levels) if r.size)
        emu = max(int(np.abs(R.levels_from_logits(cfg, R.emulate_f16(cfg, w, r)).astype(np.int64) - e).max())
                  for r, e in zip(rows, ref_levels) if e.size)
        tol = 4 * emu + 1
        print("vadnet end to end: level deviation emulation %d, device %d (allowed %d)" % (emu, worst, tol))
        assert worst <= tol
        for e in ref_levels:
            assert R.decisions_are_safe(e, vref, 80, 9830, tol)
        assert [_pairs(g) for g in got] == [V.segments(e, 80, vref) for e in ref_levels]
        assert [len(g) for g in got] == [3, 1, 0]
        for segs, bursts in zip(got, (BURSTS, [(100, 400)])):
            for (b, e), (f0, f1) in zip(_pairs(segs), bursts):
                assert abs(b - (f0 - 16)) <= 8 and abs(e - (f1 + 19)) <= 8, (segs, bursts)
        # refusals at attach time
        bad = W.fsmn_vad_config(n_mels=40)
        mb = E.load_vad_model(W.pack_pfw(bad, W.synth_vad_weights(bad, 1)))
        with pytest.raises(N.PfError) as ei:
            eng.set_vad_model(mb)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
        mb.close()
        assert [_pairs(g) for g in eng.vad_segment(audio, vc)] == [_pairs(g) for g in got]      # the attached model stayed
    finally:
        eng.set_vad_model(None)
        m.close()
    # detached: the energy path, bit for bit, with its own launch counts
    eng.profile(True)
    eng.profile_reset()
    after = eng.vad_segment(audio)
    assert eng.profile_get("vadnet")[1] == 0
    assert eng.profile_get("vad")[1] == 2
    eng.profile(False)
    assert [_pairs(g) for g in after] == [_pairs(g) for g in before]
    with pytest.raises(N.PfError) as ei:
        eng.op_vad_model_logits([rows[1]])
    assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_snip_edges_front_end_refuses_the_model():
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0, snip_edges=True)
    vcfg = W.fsmn_vad_config()
    m = E.load_vad_model(W.pack_pfw(vcfg, W.synth_vad_weights(vcfg, 1)))
    try:
        with pytest.raises(N.PfError) as ei:
            e.set_vad_model(m)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    finally:
        m.close()
        e.close()


def test_engine_create_refuses_a_vad_container():
    vcfg = W.fsmn_vad_config(**R.SMALL)
    with pytest.raises(N.PfError):
        E.Engine(weights=W.pack_pfw(vcfg, W.synth_vad_weights(vcfg, 1)), cmvn=W.synth_cmvn(), device=0)


# ---- recognizer --------------------------------------------------------------------------------------------------------------
VOCAB = 300
SEP = " | "


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from oracle import frontend as fe
    d = tmp_path_factory.mktemp("vadnet_rec")
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=VOCAB)
    W.save_pfw(str(d / "model.pfw"), cfg, W.synth_weights(cfg, seed=77))
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text("model: paraformer\nuse_itn: false\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n"
                                "  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n")
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + [chr(0x4E00 + 37 * i) for i in range(120)] + ["w%d" % i for i in range(VOCAB - 124)]
    (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return d, [str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]


def _streams(r, audio):
    out = []
    for a in audio:
        s = r.CreateOfflineStream()
        s.AddSamples(a)
        out.append(s)
    return out


def test_recognizer_with_the_model_score(model_dir, eng80):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    d, paths = model_dir
    audio = [V.burst_audio(20, BURSTS, 1), V.burst_audio(7, [(100, 400)], 2)]
    rows = eng80.op_fbank_batch(audio)
    cfg, w = R.energy_model(rows[0])
    W.save_pfw(str(d / "vad.pfw"), cfg, w)
    vc = E.vad_model_config()
    # what the segments must be: the engine-level call with the same model
    m = _attach(eng80, cfg, w)
    try:
        want = [_pairs(g) for g in eng80.vad_segment(audio, vc)]
    finally:
        eng80.set_vad_model(None)
        m.close()
    assert [len(x) for x in want] == [3, 1]
    energy = [_pairs(g) for g in eng80.vad_segment(audio, E.vad_config())]
    assert energy != want                                              # the two scores cut differently: the model is what ran
    rv, rp = OfflineRecognizer(*paths), OfflineRecognizer(*paths)
    rv.SetDecode(scores=True)
    rp.SetDecode(scores=True)
    rv.SetVadModel(str(d / "vad.pfw"))                                 # before SetVad: inert until then
    sv = _streams(rv, [W.synth_audio(32000, 5)])
    plain = rv.GetResults(sv)
    assert sv[0].Segments == [] and len(plain) == 1
    rv.SetVad(vc, batch_max=4, sep=SEP)
    sv = _streams(rv, audio)
    res = rv.GetResults(sv)
    segs = [s.Segments for s in sv]
    assert [[(g.BeginMs // 10, g.EndMs // 10) for g in sl] for sl in segs] == want
    # every batch again with plain streams over the same sample ranges, in plan order
    pool = [(i, g) for i, sl in enumerate(segs) for g in sl]
    place, nb = V.long_plan([(g.EndMs - g.BeginMs) // 10 for _, g in pool], 4, 96000)
    assert [(g.Batch, g.Row) for _, g in pool] == place
    texts = {}
    for k in range(nb):
        rws = sorted((g.Row, i, g) for i, g in pool if g.Batch == k)
        cut = [audio[i][slice(*V.sample_range((g.BeginMs // 10, g.EndMs // 10), len(audio[i])))] for _row, i, g in rws]
        ps = _streams(rp, cut)
        pres = rp.GetResults(ps)
        for (_row, i, g), p, pr in zip(rws, ps, pres):
            assert sv[i].Tokens[g.TokBegin:g.TokEnd] == p.Tokens and g.Text == pr.Text, (k, g)
            assert sv[i].Timestamps[g.TokBegin:g.TokEnd] == [[x + g.BeginMs for x in t] for t in p.Timestamps], (k, g)
            texts[(i, g.BeginMs)] = pr
    for i, sl in enumerate(segs):
        assert res[i].Text == SEP.join(texts[(i, g.BeginMs)].Text for g in sl)
        assert res[i].Tokens == [t for g in sl for t in texts[(i, g.BeginMs)].Tokens]
    # cleared: the energy score cuts again
    rv.SetVadModel(None)
    rv.SetVad(E.vad_config(), batch_max=4, sep=SEP)
    sv = _streams(rv, audio)
    rv.GetResults(sv)
    assert [[(g.BeginMs // 10, g.EndMs // 10) for g in s.Segments] for s in sv] == energy
    # refusals: a file that is no such container, a missing file
    with pytest.raises(N.PfError) as ei:
        rv.SetVadModel(paths[0])
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError):
        rv.SetVadModel(str(d / "missing.pfw"))


def test_model_reaches_an_engine_the_pool_creates_afterwards(model_dir, eng80, monkeypatch):
    """A caller that keeps engine 0 busy (through pf_recognizer_engine, which locks engine 0 without a lease) makes the next
    GetResults create the pool's second engine: the pool must have grown, and calls on either engine must cut with the model."""
    import ctypes as C
    import threading
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    monkeypatch.setenv("PF_RECOGNIZER_ENGINES", "2")
    d, paths = model_dir
    audio = [V.burst_audio(7, [(100, 400)], 2)]
    rows = eng80.op_fbank_batch([V.burst_audio(20, BURSTS, 1)])
    cfg, w = R.energy_model(rows[0])
    W.save_pfw(str(d / "vad2.pfw"), cfg, w)
    vc = E.vad_model_config()
    m = _attach(eng80, cfg, w)
    try:
        want = [_pairs(g) for g in eng80.vad_segment(audio, vc)]
    finally:
        eng80.set_vad_model(None)
        m.close()
    assert [len(x) for x in want] == [1]
    rv = OfflineRecognizer(*paths)
    lib = rv._lib
    assert lib.pf_recognizer_num_engines(rv._h) == 1
    rv.SetVadModel(str(d / "vad2.pfw"))                                # one engine exists now; the second comes later
    rv.SetVad(vc)

    def cut():
        sv = _streams(rv, audio)
        rv.GetResults(sv)
        return [[(g.BeginMs // 10, g.EndMs // 10) for g in s.Segments] for s in sv]
    assert cut() == want and lib.pf_recognizer_num_engines(rv._h) == 1
    # engine 0 kept busy: the model's launches over 200 000 caller rows, call after call, until told to stop
    h0 = C.c_void_p(lib.pf_recognizer_engine(rv._h))
    big = np.ascontiguousarray(np.tile(rows[0][:2000], (100, 1)), dtype=np.float32)
    T = np.array([big.shape[0]], np.int32)
    lev = np.zeros(big.shape[0], np.int32)
    stop, started, errors = threading.Event(), threading.Event(), []

    def hog():
        try:
            while not stop.is_set():
                started.set()
                N.check(lib.pf_op_vad_model_levels(h0, big.ctypes.data_as(C.POINTER(C.c_float)), T.ctypes.data_as(C.POINTER(C.c_int32)), 1, 80,
                                                   lev.ctypes.data_as(C.POINTER(C.c_int32))))
        except Exception as ex:                                        # noqa: BLE001 - reported by the main thread
            errors.append(repr(ex))
    th = threading.Thread(target=hog)
    th.start()
    try:
        assert started.wait(60)
        got = []
        for _ in range(40):                                            # engine 0's mutex is free only between two of the hog's calls
            got.append(cut())
            if lib.pf_recognizer_num_engines(rv._h) == 2:
                break
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert lib.pf_recognizer_num_engines(rv._h) == 2                   # the pool grew while engine 0 was held
    assert got == [want] * len(got)
    # both engines in use at once: two callers released together
    gate = threading.Barrier(2)
    out = [None, None]

    def work(k):
        try:
            gate.wait(60)
            out[k] = [cut() for _ in range(4)]
        except Exception as ex:                                        # noqa: BLE001
            errors.append(repr(ex))
    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    assert out == [[want] * 4] * 2
    rv.Dispose()


# ---- a real file, opt-in ---------------------------------------------------------------------------------------------------------
def test_real_vad_model_optin(eng80, tmp_path):
    """PF_REAL_VAD_MODEL=<vad.onnx or vad.pt>,<vad.mvn>: convert a real FSMN-VAD file and run it against the definition."""
    spec = os.environ.get("PF_REAL_VAD_MODEL", "")
    if not spec:
        pytest.skip("PF_REAL_VAD_MODEL is not set")
    from aliparaformerasr_amd import convert
    src, mvn = spec.split(",")
    out = str(tmp_path / "vad.pfw")
    assert convert.main([src, out, "--kind", "fsmnvad", "--mvn", mvn]) == 0
    cfg, w = W.load_pfw(out)
    rows = eng80.op_fbank_batch([V.burst_audio(7, [(100, 400)], 2)])
    m = E.load_vad_model(out)
    eng80.set_vad_model(m)
    try:
        got = eng80.op_vad_model_logits(rows)[0]
    finally:
        eng80.set_vad_model(None)
        m.close()
    want = R.logits(cfg, w, rows[0])
    emu = float(np.abs(R.emulate_f16(cfg, w, rows[0]) - want).max())
    assert float(np.abs(got - want).max()) <= 4 * emu
