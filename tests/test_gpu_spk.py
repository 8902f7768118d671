"""GPU: the CAM++ speaker embedding and the affinity on the device (csrc/k_spk.hip; Engine.set_spk_model / op_spk_embed /
op_spk_affinity) against the float64 definition (tests/spk_ref.py).

  * exact-answer inputs (spk_ref.exact_model / exact_rows): no rounding point loses anything on the way to the frames, which
    the test asserts on the reference first; the frames in front of the pooling are then bit-equal to the float64 answer at
    every window length that is an edge of the stride, of seg_len or of a 64-row tile, alone and in every grouping.
    Two deviations from the wording of the issue, both needed for its purpose: the premise asserted is "every rounding is
    lossless and below 2048" (a half-integer times the mask 1/2 is a quarter: "integer or half-integer" is not closed under
    the network), and the mask bias that stands for sigmoid = 1 is +64, not +32 (the float64 sigmoid of 32 is 1 - 1.3e-14).
  * random weights: the numpy emulation of the kernel's float16 rounding points deviates from float64 by `emu` (measured here,
    on the CPU); the device is allowed 4 x that on the embedding, the margin DESIGN 4.6k / 4.6l use.  Measured on one MI355X:
    see DESIGN 4.6m.
"""
import numpy as np
import pytest

import spk_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd import engine as E

pytestmark = pytest.mark.gpu

SMALL_T = [0, 1, 2, 3, 4, 5, 9, 10, 11, 126, 127, 128, 129, 130, 198, 199, 200, 201, 202, R.MAX_FRAMES]
MIXED = [5, 0, 70, 1, 131]


def _engine(n_mels):
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    return E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(7 * n_mels), device=0, n_mels=n_mels)


@pytest.fixture(scope="module")
def eng80():
    e = _engine(80)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = _engine(16)
    yield e
    e.close()


def _attach(eng, cfg, w):
    m = E.load_spk_model(W.pack_pfw(cfg, w))
    eng.set_spk_model(m)
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- exact answers -----------------------------------------------------------------------------------------------------
def _exact_case(base, Ts, seed):
    cfg, w = R.exact_model(base, seed=seed)
    rows = [R.exact_rows(T, cfg["n_mels"], 100 * seed + T) for T in Ts]
    want = []
    for x in rows:
        worst, lossless, same = R.exact_premise(cfg, w, x)
        assert worst < 2048 and lossless and same                       # the premise: nothing is lost in any rounding
        want.append(R.forward(cfg, w, x)["frames"].astype(np.float32))
    return cfg, w, rows, want


def test_exact_frames_small_model_every_length_and_grouping(eng16):
    cfg, w, rows, want = _exact_case(R.SMALL, SMALL_T, seed=1)
    m = _attach(eng16, cfg, w)
    try:
        emb_all, fr_all = eng16.op_spk_embed(rows, want_frames=True)
        assert max(float(np.abs(z).max()) for z in want if z.size) > 8    # not a trivial answer
        for b, T in enumerate(SMALL_T):
            assert fr_all[b].shape == want[b].shape == ((T + 1) // 2, R.frames_out_channels(cfg))
            np.testing.assert_array_equal(fr_all[b], want[b], err_msg="T = %d in one call" % T)
        assert not emb_all[0].any()                                        # T = 0: zeros
        for T in (1, 2):                                                   # T' = 1: the standard deviation is 0, and the statistics
            b = SMALL_T.index(T)                                           # (the one frame || zeros) are exact: the embedding is bit-equal
            ref = R.forward(cfg, w, rows[b])
            assert ref["frames"].shape[0] == 1 and np.isfinite(ref["emb"]).all()
            C = ref["frames"].shape[1]
            only_mean = ref["frames"][0] @ w["dense.weight"].astype(np.float64)[:, :C].T + w["dense.bias"]
            np.testing.assert_array_equal(ref["emb"], only_mean)
            np.testing.assert_array_equal(emb_all[b], ref["emb"].astype(np.float32), err_msg="T = %d" % T)
        for b, T in enumerate(SMALL_T):                                    # each alone: the same bits
            emb, fr = eng16.op_spk_embed([rows[b]], want_frames=True)
            np.testing.assert_array_equal(_bits(fr[0]), _bits(fr_all[b]), err_msg="T = %d alone" % T)
            np.testing.assert_array_equal(_bits(emb[0]), _bits(emb_all[b]), err_msg="T = %d alone" % T)
        mixed = [rows[SMALL_T.index(T)] if T in SMALL_T else R.exact_rows(T, cfg["n_mels"], 7 + T) for T in MIXED]
        ref = [R.forward(cfg, w, x)["frames"].astype(np.float32) for x in mixed]
        first = eng16.op_spk_embed(mixed, want_frames=True)
        back = eng16.op_spk_embed(mixed[::-1], want_frames=True)
        again = eng16.op_spk_embed(mixed, want_frames=True)
        for b in range(len(mixed)):
            np.testing.assert_array_equal(first[1][b], ref[b])
            for other_emb, other_fr in ((back[0][::-1], back[1][::-1]), again):
                np.testing.assert_array_equal(_bits(other_fr[b]), _bits(first[1][b]))
                np.testing.assert_array_equal(_bits(other_emb[b]), _bits(first[0][b]))
    finally:
        eng16.set_spk_model(None)
        m.close()


def test_exact_frames_released_dimensions(eng80):
    Ts = [1, 199, 200, 201, 75]                                            # T' = 1, 100, 100, 101 (the seg_len edge), 38
    cfg, w, rows, want = _exact_case(None, Ts, seed=2)
    m = _attach(eng80, cfg, w)
    try:
        emb_all, fr_all = eng80.op_spk_embed(rows, want_frames=True)
        for b, T in enumerate(Ts):
            np.testing.assert_array_equal(fr_all[b], want[b], err_msg="T = %d" % T)
        emb, fr = eng80.op_spk_embed([rows[3]], want_frames=True)
        np.testing.assert_array_equal(_bits(fr[0]), _bits(fr_all[3]))
        np.testing.assert_array_equal(_bits(emb[0]), _bits(emb_all[3]))
        assert max(float(np.abs(z).max()) for z in want) > 8
    finally:
        eng80.set_spk_model(None)
        m.close()


@pytest.mark.parametrize("name,Ts,vary", [("small", SMALL_T, (11, 130, 202, R.MAX_FRAMES)), ("released", [201, 199, 75], (201,))])
def test_exact_frames_with_a_mask_that_depends_on_the_segment(name, Ts, vary, eng80, eng16):
    """exact_model(segment_mask=True): the mask of half the channels of every block's last layer is 0 or 1 ACCORDING TO THE
    SEGMENT's context, exactly: the column and segment means, the divisor of a partial last segment (T' = 6 with seg_len 5;
    T' = 101 with 100) and the mask row a frame looks up are then held bit for bit"""
    eng = eng80 if name == "released" else eng16
    cfg, w = R.exact_model(None if name == "released" else R.SMALL, seed=4, segment_mask=True)
    rows = [R.exact_rows(T, cfg["n_mels"], 400 + T) for T in Ts]
    want = []
    for T, x in zip(Ts, rows):
        worst, lossless, same = R.exact_premise(cfg, w, x)
        assert worst < 2048 and lossless and same, T
        assert R.mask_varies(cfg, w, x) or T not in vary, T               # the masks of two segments do differ where they can
        want.append(R.forward(cfg, w, x)["frames"].astype(np.float32))
    m = _attach(eng, cfg, w)
    try:
        emb_all, fr_all = eng.op_spk_embed(rows, want_frames=True)
        alone = eng.op_spk_embed([rows[0 if name == "released" else Ts.index(130)]], want_frames=True)
    finally:
        eng.set_spk_model(None)
        m.close()
    for b, T in enumerate(Ts):
        np.testing.assert_array_equal(fr_all[b], want[b], err_msg="T = %d" % T)
    b = 0 if name == "released" else Ts.index(130)
    np.testing.assert_array_equal(_bits(alone[1][0]), _bits(fr_all[b]))


def test_a_poisoned_row_reaches_its_own_window_only(eng16):
    cfg, w, rows, want = _exact_case(R.SMALL, MIXED, seed=3)
    m = _attach(eng16, cfg, w)
    try:
        clean_emb, clean_fr = eng16.op_spk_embed(rows, want_frames=True)
        bad = [r.copy() for r in rows]
        bad[2][10, :] = np.nan
        bad[2][10, 1::3] = np.inf
        bad[2][10, 2::3] = -np.inf
        emb, fr = eng16.op_spk_embed(bad, want_frames=True)
        assert not np.isfinite(R.forward(cfg, w, bad[2])["emb"]).any()     # the definition: x - mean_t x is NaN in every row
        assert not np.isfinite(emb[2]).any() and not np.isfinite(fr[2]).any()
        for b in (0, 1, 3, 4):
            np.testing.assert_array_equal(_bits(emb[b]), _bits(clean_emb[b]))
            np.testing.assert_array_equal(_bits(fr[b]), _bits(clean_fr[b]))
    finally:
        eng16.set_spk_model(None)
        m.close()


# ---- random weights ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seeds,Ts", [("released", (6,), [150, 37, 1, 2, 301]), ("small", (5, 6, 7), [150, 37, 1, 2, 400, 11])])
def test_random_weights_embedding_within_four_emulation_deviations(name, seeds, Ts, eng80, eng16):
    eng = eng80 if name == "released" else eng16
    for seed in seeds:
        cfg, w = R.random_model(None if name == "released" else R.SMALL, seed)
        rows = [R.fbank_like(T, cfg["n_mels"], 100 * seed + T) for T in Ts]
        want = [R.forward(cfg, w, x) for x in rows]
        emus = [R.emulate_f16(cfg, w, x) for x in rows]
        emu = max(float(np.abs(e["emb"] - z["emb"]).max()) for e, z in zip(emus, want))
        emu_fr = max(float(np.abs(e["frames"] - z["frames"]).max()) for e, z in zip(emus, want))
        scale = max(float(np.abs(z["emb"]).max()) for z in want)
        assert 0 < emu < 0.05 * scale, (name, seed, emu, scale)
        m = _attach(eng, cfg, w)
        try:
            emb, fr = eng.op_spk_embed(rows, want_frames=True)
            alone = eng.op_spk_embed([rows[1]])
        finally:
            eng.set_spk_model(None)
            m.close()
        dev = max(float(np.abs(g.astype(np.float64) - z["emb"]).max()) for g, z in zip(emb, want))
        dev_fr = max(float(np.abs(g.astype(np.float64) - z["frames"]).max()) for g, z in zip(fr, want))
        print("spk %s seed %d: embedding emulation %.3e, device %.3e (allowed %.3e; largest value %.2f); frames emulation %.3e, "
              "device %.3e" % (name, seed, emu, dev, 4 * emu, scale, emu_fr, dev_fr))
        assert dev <= 4 * emu, (name, seed, dev, emu)
        assert dev_fr <= 4 * emu_fr, (name, seed, dev_fr, emu_fr)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(emb[1]))     # a window does not depend on its batch mates
        for b in (2, 3):                                                   # T' = 1 (the standard deviation is 0, not NaN) within the same allowance
            assert np.isfinite(emb[b]).all() and float(np.abs(emb[b] - want[b]["emb"]).max()) <= 4 * emu


# ---- affinity --------------------------------------------------------------------------------------------------------------
def test_affinity_against_float64_and_run_to_run(eng16):
    rng = np.random.default_rng(11)
    Edim = 192
    streams = [rng.standard_normal((n, Edim)).astype(np.float32) + 0.5 for n in (37, 1, 0, 130)]
    streams[0][5] = 0                                                     # a zero embedding: cosine 0 with everything
    got = eng16.op_spk_affinity(streams)
    again = eng16.op_spk_affinity(streams)
    # three fp32 sums of E terms each (u.v, u.u, v.v; Cauchy-Schwarz bounds the first by |u| |v|), two square roots, one
    # product, one division: |dS| <= E eps + |S| (E eps + 5 eps) <= (2 E + 5) 2^-24
    bound = (2 * Edim + 5) * 2.0 ** -24
    for s, e in enumerate(streams):
        assert got[s].shape == (e.shape[0], e.shape[0])
        np.testing.assert_array_equal(_bits(got[s]), _bits(again[s]))
        if e.shape[0]:
            ref = R.affinity(e)
            assert float(np.abs(got[s].astype(np.float64) - ref).max()) <= bound
            np.testing.assert_array_equal(_bits(got[s]), _bits(got[s].T.copy()))       # symmetric to the bit
    assert not got[0][5].any() and not got[0][:, 5].any()
    alone = eng16.op_spk_affinity([streams[3]])[0]
    np.testing.assert_array_equal(_bits(alone), _bits(got[3]))


# ---- end to end through the ops ----------------------------------------------------------------------------------------
def _reference_labels(cfg, w, rows, win):
    """the definition's run on the device's own fbank rows: (cosines, allowance, labels, speakers), after asserting the
    condition under which the device must give the same labels: no decision of the run lies within twice the allowance of the
    threshold or of its runner-up"""
    S_ref, allow = R.cosine_allowance(cfg, w, [rows[b:e] for _, b, e in win])
    labels, k, safe = R.label_decisions_are_safe(S_ref.astype(np.float32), allow)
    assert safe and 0 < allow < 0.01, allow
    return S_ref, allow, labels, k


def test_end_to_end_through_the_ops_labels_follow_the_sources(eng80):
    """two constructed sources, a constructed model (spk_ref.separating_model), the threshold deciding: the device's labels
    are the definition's, and the sources'"""
    eng = eng80
    audio = R.two_source_audio()
    rows = eng.op_fbank_batch([audio])[0]
    segs = [tuple(p) for p in np.asarray(eng.vad_segment([audio], E.vad_config(**R.TWO_SOURCE_VAD))[0]).tolist()]
    assert len(segs) == 4
    win, shift = E.host_spk_windows(segs, R.TWO_SOURCE_SPK)
    win = [tuple(x) for x in win.tolist()]
    assert shift == 100 and win == R.stream_windows(segs, **R.TWO_SOURCE_SPK)[0] and [x[0] for x in win] == [0, 1, 2, 3]
    cfg, w = R.separating_model()
    S_ref, allow, ref_labels, ref_k = _reference_labels(cfg, w, rows, win)
    m = _attach(eng, cfg, w)
    try:
        eng.profile(True)
        eng.profile_reset()
        emb = eng.op_spk_embed([rows[b:e] for _, b, e in win])
        n_embed = eng.profile_get("spk")[1]
        S = eng.op_spk_affinity([emb])[0]
        n_both = eng.profile_get("spk")[1]
        others = [eng.profile_get(c)[1] for c in ("vadnet", "punc", "vad", "fbank")]
        eng.profile(False)
    finally:
        eng.set_spk_model(None)
        m.close()
    assert n_embed == m.dims["launches"] == 15 and n_both == 16 and others == [0, 0, 0, 0]
    dS = float(np.abs(S.astype(np.float64) - S_ref).max())
    print("spk two sources: cosine allowance %.3e, device %.3e" % (allow, dS))
    assert dS <= allow
    scfg = {k: v for k, v in R.TWO_SOURCE_SPK.items()}
    labels, k = E.host_spk_cluster(S, scfg)
    assert k == ref_k == 2 and labels.tolist() == ref_labels.tolist() == [0, 1, 0, 1]
    assert labels.tolist() == R.cluster(S)[0].tolist()                     # and exactly the definition over the device's own S
    seg_lab = E.host_spk_segment_labels(segs, [x[0] for x in win], labels)
    assert seg_lab.tolist() == [0, 1, 0, 1]
    cent = E.host_spk_centroids(emb, labels, k)
    np.testing.assert_allclose(cent, R.centroids(emb, labels, k), atol=1e-6)


def test_attached_and_detached_engine_computes_what_it_did(eng80):
    """the recogniser's forward with the model attached, and after detaching: logits, ids and the launch census bit for bit
    those of the engine before it ever saw the model"""
    eng = eng80
    audio = [W.synth_audio(32000, u) for u in range(2)]

    def run():
        eng.profile(True)
        eng.profile_reset()
        res = eng.recognize(audio, want_logits=True)
        census = {c: eng.profile_get(c)[1] for c in ("spk", "fbank", "vad", "vadnet", "punc", "attn", "ffn", "norm", "misc", "frontend", "cif", "gemm")}
        eng.profile(False)
        return _bits(res.logits).copy(), np.asarray(res.token_ids).copy(), census
    before = run()
    assert before[2]["spk"] == 0 and sum(before[2].values()) > 0
    cfg, w = R.random_model(None, 4)
    m = _attach(eng, cfg, w)
    try:
        attached = run()
    finally:
        eng.set_spk_model(None)
        m.close()
    detached = run()
    for other in (attached, detached):
        np.testing.assert_array_equal(other[0], before[0])
        np.testing.assert_array_equal(other[1], before[1])
        assert other[2] == before[2]


def test_attach_refusals_and_detach(eng80, eng16):
    cfg, w = R.random_model(R.SMALL, 1)
    m = E.load_spk_model(W.pack_pfw(cfg, w))
    try:
        with pytest.raises(N.PfError) as ei:
            eng80.set_spk_model(m)                                         # n_mels 16 on a front-end of 80
        assert ei.value.code == N.PF_ERR_INVALID_ARG
        eng16.set_spk_model(m)
        x = R.fbank_like(30, 16, 1)
        with pytest.raises(N.PfError) as ei:
            eng16.op_spk_embed([R.fbank_like(R.MAX_FRAMES + 1, 16, 2)])
        assert ei.value.code == N.PF_ERR_INVALID_ARG
        a = eng16.op_spk_embed([x])
        eng16.set_spk_model(None)
        with pytest.raises(N.PfError) as ei:
            eng16.op_spk_embed([x])
        assert ei.value.code == N.PF_ERR_INVALID_ARG
        eng16.set_spk_model(m)
        np.testing.assert_array_equal(_bits(eng16.op_spk_embed([x])), _bits(a))
    finally:
        eng16.set_spk_model(None)
        m.close()


# ---- through OfflineRecognizer + SetVad ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec_paths(tmp_path_factory):
    from oracle import frontend as fe
    d = tmp_path_factory.mktemp("spk_rec")
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=300)
    W.save_pfw(str(d / "model.pfw"), cfg, W.synth_weights(cfg, seed=77))
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (d / "asr.yaml").write_text("model: paraformer\nuse_itn: false\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n"
                                "  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n")
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + [chr(0x4E00 + 37 * i) for i in range(120)] + ["w%d" % i for i in range(300 - 124)]
    (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    scfg, sw = R.separating_model()
    W.save_pfw(str(d / "cam.pfw"), scfg, sw)
    small = R.random_model(R.SMALL, 1)
    W.save_pfw(str(d / "cam16.pfw"), *small)
    return [str(d / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], str(d / "cam.pfw"), str(d / "cam16.pfw"), (scfg, sw)


def _recognise(rec, audio):
    streams = []
    for a in audio:
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        streams.append(s)
    res = rec.GetResults(streams)
    return streams, [(r.Text, list(r.Tokens), [list(t) for t in r.Timestamps]) for r in res]


def _census(rec, audio):
    """the launches per profile class of one GetResults on the recogniser's engine 0"""
    import ctypes as C
    lib = N.load()
    h = C.c_void_p(lib.pf_recognizer_engine(rec._h))
    N.check(lib.pf_profile_enable(h, 1))
    N.check(lib.pf_profile_reset(h))
    streams, res = _recognise(rec, audio)
    out = {}
    for c in ("spk", "fbank", "vad", "vadnet", "punc", "attn", "ffn", "norm", "misc", "frontend", "cif", "gemm"):
        ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
        N.check(lib.pf_profile_get(h, c.encode(), ms, n, fpl))
        out[c] = n.value
    N.check(lib.pf_profile_enable(h, 0))
    return streams, res, out


VAD_CFG = dict(max_len=300, split_search=100, min_speech=50)


def _segments(streams):
    return [[(g.BeginMs, g.EndMs, g.Batch, g.Row, g.TokBegin, g.TokEnd, g.Text) for g in s.Segments] for s in streams]


def test_recognizer_speaker_labels_end_to_end(rec_paths, eng80):
    """two constructed sources and the constructed model through OfflineRecognizer + SetVad, the threshold deciding"""
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, cam, cam16, (scfg, sw) = rec_paths
    audio = [R.two_source_audio(1), V_burst(7, [(100, 400)], 2), np.zeros(16000, np.float32)]
    plain = OfflineRecognizer(*paths)
    _, res_never, census_never = _census(plain, audio)                     # never saw the model, no VAD
    plain.SetVad(VAD_CFG)
    st_vad, res_vad, census_vad = _census(plain, audio)

    rec = OfflineRecognizer(*paths)
    with pytest.raises(N.PfError) as ei:
        rec.SetSpeakerModel(cam16)                                         # n_mels 16 on a front-end of 80
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError):
        rec.SetSpeakerModel(cam, dict(win=1000))
    rec.SetSpeakerModel(cam, R.TWO_SOURCE_SPK)
    st, res_inert, census_inert = _census(rec, audio)                      # attached, but no SetVad: inert
    assert res_inert == res_never and census_inert == census_never and census_inert["spk"] == 0
    assert all(s.SegmentSpeakers == [] and s.SpeakerWindows == [] and s.Segments == [] for s in st)
    rec.SetVad(VAD_CFG)
    st, res_on, census_on = _census(rec, audio)
    assert res_on == res_vad                                               # Text / Tokens / Timestamps unchanged with the model on
    assert _segments(st) == _segments(st_vad) and len(_segments(st)[0]) == 4      # and Segments
    # the census: one forward (15 launches) and one affinity launch; every other class as without the model
    assert census_on["spk"] == 16 and census_vad["spk"] == 0
    assert {k: v for k, v in census_on.items() if k != "spk"} == {k: v for k, v in census_vad.items() if k != "spk"}
    rows = eng80.op_fbank_batch(audio)
    m = _attach(eng80, scfg, sw)
    try:
        for i, (s, r) in enumerate(zip(st, rows)):
            segs = [(g.BeginMs // 10, g.EndMs // 10) for g in s.Segments]
            win, _ = E.host_spk_windows(segs, R.TWO_SOURCE_SPK)
            assert [(10 * b, 10 * e) for _, b, e in win.tolist()] == [w[:2] for w in s.SpeakerWindows]
            if not len(win):
                assert s.SegmentSpeakers == [-1] * len(segs) and s.SpeakerCentroids.shape[0] == 0
                continue
            # the same windows through the ops: the stream's labels are the definition over the device's own cosines
            emb = eng80.op_spk_embed([r[b:e] for _, b, e in win.tolist()])
            S = eng80.op_spk_affinity([emb])[0]
            labels, k = E.host_spk_cluster(S, R.TWO_SOURCE_SPK)
            assert labels.tolist() == R.cluster(S)[0].tolist() == [w[2] for w in s.SpeakerWindows]
            assert s.SegmentSpeakers == R.segment_labels(segs, win[:, 0].tolist(), labels.tolist()).tolist()
            np.testing.assert_allclose(s.SpeakerCentroids, R.centroids(emb, labels, k), atol=1e-5)
            if i == 0:
                # and the definition's own labels from its float64 embeddings, under the asserted margin condition
                S_ref, allow, ref_labels, ref_k = _reference_labels(scfg, sw, r, [tuple(x) for x in win.tolist()])
                assert float(np.abs(S.astype(np.float64) - S_ref).max()) <= allow
                assert [w[2] for w in s.SpeakerWindows] == ref_labels.tolist() and ref_k == k == 2
    finally:
        eng80.set_spk_model(None)
        m.close()
    assert st[0].SegmentSpeakers == [0, 1, 0, 1]                           # the sources, found by the threshold
    # what -spk prints: `[begin-end ms] spkN text` per segment, the plain line without the option
    from aliparaformerasr_amd.examples import _segment_lines
    lines = _segment_lines(st[0], True)
    assert [ln.split("] ")[1].split(" ")[0] for ln in lines] == ["spk0", "spk1", "spk0", "spk1"]
    assert [ln.replace("spk0 ", "").replace("spk1 ", "") for ln in lines] == _segment_lines(st[0])
    # detached: bit for bit a recogniser that never saw the model
    rec.SetSpeakerModel(None)
    st2, res_off, census_off = _census(rec, audio)
    assert res_off == res_vad and census_off == census_vad and _segments(st2) == _segments(st_vad)
    assert all(s.SegmentSpeakers == [] for s in st2)


def V_burst(seconds, bursts, seed):
    import vad_ref
    return vad_ref.burst_audio(seconds, bursts, seed)


def test_real_model_file_opt_in(eng80):
    """PF_REAL_SPK_MODEL=<campplus .bin / .pt>: the file through the converter, the loader and the device, against the
    definition within 4 x the emulation's deviation.  Skipped without the variable: no such file is part of this repository."""
    import os
    path = os.environ.get("PF_REAL_SPK_MODEL")
    if not path:
        pytest.skip("PF_REAL_SPK_MODEL is not set")
    from aliparaformerasr_amd import convert as CV
    cfg, w = CV.spk_to_pfw(path)
    rows = [R.fbank_like(T, cfg["n_mels"], T) for T in (150, 61)]
    want = [R.forward(cfg, w, x)["emb"] for x in rows]
    emu = max(float(np.abs(R.emulate_f16(cfg, w, x)["emb"] - z).max()) for x, z in zip(rows, want))
    m = _attach(eng80, cfg, w)
    try:
        emb = eng80.op_spk_embed(rows)
    finally:
        eng80.set_spk_model(None)
        m.close()
    dev = max(float(np.abs(g.astype(np.float64) - z).max()) for g, z in zip(emb, want))
    print("spk real model: emulation %.3e, device %.3e" % (emu, dev))
    assert dev <= 4 * emu
