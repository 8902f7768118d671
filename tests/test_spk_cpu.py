"""CPU: the speaker labels off the device — the definition (tests/spk_ref.py) against an independent torch module with
3D-Speaker's parameter names (tests/campplus_like.py), the converter (names, BatchNorm folding, refusals), the `.pfw` container
of kind "campplus" with its loader's refusals (once more in a stand-alone program under host sanitizers), the window plan,
pf_host_spk_cluster / _segment_labels / _centroids against the definition, and the -spk option.

float32 module against the float64 definition, measured: embedding 2.5e-6 (small dimensions, largest value 9.2) and 7.5e-5
(released dimensions, largest value 23.8); frames 2.2e-5 and 1.7e-4.  The test allows 4 x these."""
import os
import struct

import numpy as np
import pytest

from pfw_helpers import repack
import spk_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

F32_DEV = {"small": (2.5e-6, 2.2e-5), "released": (7.5e-5, 1.7e-4)}       # (embedding, frames), measured: see above


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_spk_model_load", "pf_spk_model_from_memory", "pf_spk_model_info", "pf_spk_model_free", "pf_spk_default",
                 "pf_engine_set_spk_model", "pf_host_spk_windows", "pf_host_spk_cluster", "pf_host_spk_segment_labels",
                 "pf_host_spk_centroids", "pf_op_spk_embed", "pf_op_spk_affinity", "pf_recognizer_set_spk_model",
                 "pf_stream_num_speakers", "pf_stream_segment_speaker", "pf_stream_speaker_centroid", "pf_stream_num_spk_windows",
                 "pf_stream_spk_window"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    lib.pf_spk_model_free(None)
    assert lib.pf_engine_set_spk_model(None, None) < 0
    assert lib.pf_spk_model_load(None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_version() == 6
    c = E.spk_config()
    assert (c.win, c.shift, c.min_frames, c.num_speakers, c.min_cluster) == (150, 75, 20, 0, 4) and c.threshold == 0.5
    assert N.PF_SPK_MAX_FRAMES == R.MAX_FRAMES >= 400 and N.PF_SPK_MAX_WINDOWS == R.MAX_WINDOWS == 8192


# ---- the like-module, the converter ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("small", 57), ("released", 150)])
def test_like_module_converter_and_definition_agree(name, T):
    torch = pytest.importorskip("torch")
    import campplus_like as L
    from aliparaformerasr_amd import convert as CV
    cfg = R.config(R.SMALL if name == "small" else None)
    net = L.random_module(cfg, 3)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    assert "head.layer1.0.shortcut.0.weight" in sd and "xvector.block1.tdnnd1.cam_layer.linear_local.weight" in sd
    assert "xvector.tdnn.linear.weight" in sd and "xvector.transit1.linear.weight" in sd and "xvector.dense.linear.weight" in sd
    cfg2, w = CV.spk_state_dict_to_pfw(sd, seg_len=cfg["seg_len"], dilations=cfg["dilations"])
    assert cfg2 == cfg and set(w) == set(W.spk_tensor_shapes(cfg))
    x = R.fbank_like(T, cfg["n_mels"], 4)
    ref = R.forward(cfg, w, x)
    fr32, e32 = L.embed(net, x)                                            # the unfolded float32 forward
    d_emb, d_fr = float(np.abs(e32 - ref["emb"]).max()), float(np.abs(fr32 - ref["frames"]).max())
    print("campplus_like %s: float32 against float64: embedding %.3e, frames %.3e" % (name, d_emb, d_fr))
    assert d_emb <= 4 * F32_DEV[name][0] and d_fr <= 4 * F32_DEV[name][1]
    # the folding itself: the float64 module on the same weights differs from the definition only by the fp32 rounding of the
    # folded tensors
    fr64, e64 = L.embed(L.random_module(cfg, 3, torch.float64), x, torch.float64)
    assert float(np.abs(e64 - ref["emb"]).max()) < 2e-5 and float(np.abs(fr64 - ref["frames"]).max()) < 1e-4
    # and the container loads
    E.load_spk_model(W.pack_pfw(cfg, w)).close()


def test_converter_refusals(tmp_path):
    pytest.importorskip("torch")
    import campplus_like as L
    from aliparaformerasr_amd import convert as CV
    cfg = R.config(R.SMALL)
    sd = {k: v.numpy() for k, v in L.random_module(cfg, 1).state_dict().items()}
    for gone in ("head.bn1.running_var", "head.layer2.0.shortcut.1.weight", "xvector.block2.tdnnd3.cam_layer.linear2.bias",
                 "xvector.transit3.linear.weight", "xvector.dense.nonlinear.batchnorm.running_mean"):
        with pytest.raises(ValueError, match="lacks"):
            CV.spk_state_dict_to_pfw({k: v for k, v in sd.items() if k != gone})
    bad = dict(sd)
    bad["xvector.block1.tdnnd2.linear1.weight"] = sd["xvector.block1.tdnnd2.linear1.weight"][:, :-1]
    with pytest.raises(ValueError, match="shape"):
        CV.spk_state_dict_to_pfw(bad)
    bad = dict(sd)
    bad["head.conv2.weight"] = sd["head.conv2.weight"] * np.nan
    with pytest.raises(ValueError, match="not finite"):
        CV.spk_state_dict_to_pfw(bad)
    extra = dict(sd)
    extra["xvector.block4.tdnnd1.linear1.weight"] = sd["xvector.block1.tdnnd1.linear1.weight"]
    with pytest.raises(ValueError, match="three dense blocks"):
        CV.spk_state_dict_to_pfw(extra)
    with pytest.raises(ValueError, match="not an ONNX"):
        CV.spk_to_pfw(str(tmp_path / "campplus.onnx"))


# ---- the container -----------------------------------------------------------------------------------------------------------
def _refusals():
    cfg, w = R.random_model(R.SMALL, 1)
    good = W.pack_pfw(cfg, w)

    def far(h): h["tensors"][3]["offset"] = 1 << 40
    def big(h): h["tensors"][-1]["nbytes"] = h["tensors"][-1]["nbytes"] + 4096
    def u8(h): h["tensors"][2]["dtype"] = "u8"
    def with_(**kw):
        c = W.campplus_config(**dict(R.SMALL, **kw))
        return W.pack_pfw(c, W.synth_spk_weights(c, 1))
    def raw(**kw): return W.pack_pfw(dict(cfg, **kw), w)
    def tensor(name, fn):
        w2 = {k: v.copy() for k, v in w.items()}
        w2[name] = fn(w2[name])
        return W.pack_pfw(cfg, w2)
    def nan(a): a.reshape(-1)[3] = np.nan; return a
    def inf(a): a.reshape(-1)[0] = np.inf; return a
    inv = [("short", good[:40]), ("cut tail", good[: len(good) - 237]), ("half", good[: len(good) // 2]), ("empty", b""),
           ("offset", repack(cfg, w, far)), ("nbytes", repack(cfg, w, big)), ("u8", repack(cfg, w, u8)),
           ("header length", good[:8] + struct.pack("<Q", (1 << 64) - 8) + good[16:]), ("magic", b"XXXX" + good[4:]),
           ("kind", raw(kind="fsmnvad")), ("nan", tensor("dense.bias", nan)), ("inf", tensor("head.conv1.weight", inf)),
           ("shape", tensor("block2.1.local.weight", lambda a: a[:, :, :2].copy())),
           ("missing", W.pack_pfw(cfg, {k: v for k, v in w.items() if k != "transit2.bn.shift"})),
           ("two blocks", raw(blocks=[2, 3])), ("dilations", raw(dilations=[1, 2, 0])), ("no seg_len", raw(seg_len=0)),
           ("blocks no list", raw(blocks=3))]
    uns = [("n_mels not 8", with_(n_mels=20)), ("n_mels", with_(n_mels=136)), ("m not 8", with_(m_channels=12)), ("m", with_(m_channels=72)),
           ("frame width", with_(n_mels=128, m_channels=40)), ("init", with_(init_channels=136)), ("bn", with_(bn_channels=130)),
           ("bn odd", with_(bn_channels=13)), ("growth", with_(growth=72)), ("layers", with_(blocks=(65, 1, 1), growth=2, init_channels=2)),
           ("dilation", with_(dilations=(1, 2, 9))), ("seg_len", with_(seg_len=3)), ("odd width", with_(init_channels=25, growth=8, blocks=(1, 1, 1))),
           ("width", with_(blocks=(2, 64, 2), growth=64)), ("embedding", with_(embedding=520))]
    return good, inv, uns


def test_container_refusals_and_supported_variants():
    good, inv, uns = _refusals()
    m = E.load_spk_model(good)
    assert m.dims["embedding"] == 20 and m.dims["frame_width"] == 19 and m.dims["launches"] == 15 and m.image_bytes > 0
    m.close()
    for name, blob in inv:
        with pytest.raises(N.PfError) as ei:
            E.load_spk_model(blob if blob else b"\0")
        assert ei.value.code == N.PF_ERR_INVALID_ARG, name
    for name, blob in uns:
        with pytest.raises(N.PfError) as ei:
            E.load_spk_model(blob)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED, name
    for kw in (None, dict(R.SMALL, seg_len=4, dilations=(8, 1, 3)), dict(R.SMALL, m_channels=64, n_mels=64), dict(R.SMALL, embedding=512),
               dict(R.SMALL, growth=64, blocks=(1, 1, 1), init_channels=128, bn_channels=128)):
        cfg, w = R.random_model(kw, 2)
        E.load_spk_model(W.pack_pfw(cfg, w)).close()                       # the released dimensions and the edges of the limits


def test_loader_under_sanitizers(tmp_path):
    """csrc/spk.cpp in a stand-alone program (tests/native/spk_sanitize.cpp) built with AddressSanitizer + UBSan on the host code,
    over a good container and every malformed one: no report, the library's own status codes; then the host half once."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "spk_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "spk_sanitize.cpp"),
                        os.path.join(cs, "spk.cpp"), os.path.join(cs, "pfw.cpp"), os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a compile error in the sources under test is a failure
        missing = any(t in b.stderr for t in ("libclang_rt.asan", "libclang_rt.ubsan", "cannot find -lclang_rt", "unsupported option '-fsanitize"))
        assert missing, b.stderr[-3000:]
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    good, inv, uns = _refusals()
    blobs = [good] + [x for _, x in inv] + [x for _, x in uns]
    paths = []
    for i, blob in enumerate(blobs):
        p = tmp_path / ("c%d.pfw" % i)
        p.write_bytes(blob)
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(blobs) + 1
    m = E.load_spk_model(good)
    assert lines[0] == "ok 16 8 24 8 12 20 19 %d" % m.image_bytes
    m.close()
    assert lines[1: 1 + len(inv)] == ["refused %d" % N.PF_ERR_INVALID_ARG] * len(inv)
    assert lines[1 + len(inv): -1] == ["refused %d" % N.PF_ERR_UNSUPPORTED] * len(uns)
    # the host half on the program's fixed inputs: what the definition gives
    segs = [(0, 19), (30, 50), (100, 250), (300, 451), (500, 724), (800, 1025), (2000, 2010)]
    win, shift = R.stream_windows(segs)
    n = len(win)
    S = np.array([[(0.9 - 0.01 * ((i + j) % 5)) if i % 2 == j % 2 else 0.1 for j in range(n)] for i in range(n)], np.float32)
    labels, K = R.cluster(S, min_cluster=2)
    seg_lab = R.segment_labels(segs, [w[0] for w in win], labels)
    head, lab, sl = lines[-1].split("|")
    assert head.split() == ["plan", str(n), str(shift), str(K)]
    assert [int(x) for x in lab.split()] == labels.tolist() and [int(x) for x in sl.split()] == seg_lab.tolist()


# ---- the window plan ---------------------------------------------------------------------------------------------------------
def test_window_plan_at_every_edge():
    d = R.DEFAULTS
    win, shift, mn = d["win"], d["shift"], d["min_frames"]
    expect = {mn - 1: [], mn: [(7, 7 + mn)], win: [(7, 7 + win)], win + 1: [(7, 7 + win), (8, 8 + win)],
              win + shift - 1: [(7, 7 + win), (7 + shift - 1, 7 + win + shift - 1)], win + shift: [(7, 7 + win), (7 + shift, 7 + win + shift)],
              win + 2 * shift + 1: [(7, 7 + win), (7 + shift, 7 + shift + win), (7 + 2 * shift, 7 + 2 * shift + win), (8 + 2 * shift, 8 + 2 * shift + win)]}
    for n, want in expect.items():
        assert R.windows(7, 7 + n, win, shift, mn) == want, n
        got, sh = E.host_spk_windows([(7, 7 + n)])
        assert [tuple(x[1:]) for x in got.tolist()] == want and sh == shift and all(x[0] == 0 for x in got.tolist()), n
    # several segments, other values
    segs = [(0, 19), (30, 50), (100, 250), (300, 451), (500, 724), (800, 1025), (2000, 2010)]
    for cfg in ({}, dict(win=40, shift=7, min_frames=3), dict(win=512, shift=1, min_frames=1)):
        kw = {k: cfg.get(k, d[k]) for k in ("win", "shift", "min_frames")}
        want, sh = R.stream_windows(segs, **kw)
        got, sh2 = E.host_spk_windows(segs, cfg or None)
        assert [tuple(x) for x in got.tolist()] == want and sh == sh2
    # the PF_SPK_MAX_WINDOWS rule: the shift doubles until the stream fits
    long = [(0, 150 + 75 * 8191)]                                          # exactly 8192 windows at the default shift
    got, sh = E.host_spk_windows(long)
    assert len(got) == 8192 and sh == 75
    long = [(0, 150 + 75 * 8192)]                                          # one more: the shift doubles once
    want, shr = R.stream_windows(long)
    got, sh = E.host_spk_windows(long)
    assert sh == shr == 150 and [tuple(x) for x in got.tolist()] == want and len(got) == 4097
    got, sh = E.host_spk_windows([(0, 4000000)], dict(shift=1))
    want, shr = R.stream_windows([(0, 4000000)], shift=1)
    assert sh == shr == 512 and len(got) == len(want) <= 8192 and tuple(got[-1]) == want[-1]
    for bad in (dict(win=0), dict(win=513), dict(shift=0), dict(min_frames=0), dict(min_frames=151), dict(num_speakers=-1)):
        with pytest.raises(N.PfError) as ei:
            E.host_spk_windows(segs, bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, bad


# ---- the clustering ----------------------------------------------------------------------------------------------------------
def _blocks(sizes, inside=0.9, across=0.1, order=None):
    n = sum(sizes)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    if order is not None:
        owner = owner[order]
    S = np.where(owner[:, None] == owner[None, :], inside, across).astype(np.float32)
    np.fill_diagonal(S, 1.0)
    return S, owner


def _same(S, **kw):
    d = R.DEFAULTS
    ref = R.cluster(S, **{k: kw.get(k, d[k]) for k in ("threshold", "num_speakers", "min_cluster")})
    got = E.host_spk_cluster(S, kw or None)
    assert got[0].tolist() == ref[0].tolist() and got[1] == ref[1], (kw, got, ref)
    return got


def test_cluster_constructed_matrices():
    S, owner = _blocks([5, 6])
    lab, k = _same(S)
    assert k == 2 and lab.tolist() == owner.tolist()
    order = np.random.default_rng(1).permutation(18)
    S, owner = _blocks([5, 6, 7], order=order)
    lab, k = _same(S)
    first = {}
    want = [first.setdefault(o, len(first)) for o in owner.tolist()]       # numbered by first window in time
    assert k == 3 and lab.tolist() == want
    # exact ties: every pair equal -> the smallest first index, then the smallest second index, at every step
    S = np.full((6, 6), 0.75, np.float32)
    lab, k = _same(S)
    assert k == 1 and lab.tolist() == [0] * 6
    lab, k = _same(S, num_speakers=3)
    assert k == 3 and lab.tolist() == [0, 0, 0, 0, 1, 2]                   # 0+1, then (0,1)+2, then +3: always the first pair
    S = np.full((5, 5), 0.1, np.float32)                                  # a tie in the first index, decided by the second
    S[0, 3] = S[3, 0] = S[0, 2] = S[2, 0] = 0.8
    lab, k = _same(S, min_cluster=1)
    assert lab.tolist() == [0, 1, 0, 2, 3]                                # (0, 2) before (0, 3); then ({0, 2}, 3) is at 0.45
    S[1, 4] = S[4, 1] = 0.8                                               # and a tie between two first indices
    lab, k = _same(S, num_speakers=4)
    assert lab.tolist() == [0, 1, 0, 2, 3]
    # one window, no window
    assert _same(np.ones((1, 1), np.float32))[0].tolist() == [0]
    lab, k = E.host_spk_cluster(np.zeros((0, 0), np.float32))
    assert lab.size == 0 and k == 0 and R.cluster(np.zeros((0, 0)))[1] == 0
    # all equal below the threshold: nobody merges; without a major cluster the minor ones stay
    lab, k = _same(np.full((5, 5), 0.2, np.float32))
    assert k == 5 and lab.tolist() == [0, 1, 2, 3, 4]
    # num_speakers forcing more merges than the threshold would, and fewer
    S, owner = _blocks([5, 6, 7])
    assert _same(S, num_speakers=2)[1] == 2 and _same(S, num_speakers=1)[1] == 1
    assert _same(S, num_speakers=5)[1] == 5 and _same(S, num_speakers=40)[1] == 18
    # minor clusters with a major one: they join the one they are most similar to
    S, owner = _blocks([6, 2, 5, 1])
    S[6:8, 8:13] = S[8:13, 6:8] = 0.3                                      # the pair leans to the second major
    S[13, 0:6] = S[0:6, 13] = 0.4                                          # the single one to the first
    lab, k = _same(S)
    assert k == 2 and lab.tolist() == [0] * 6 + [1] * 2 + [1] * 5 + [0]
    lab, k = _same(S, min_cluster=1)
    assert k == 4
    # a value that is not finite counts as -2
    S, _ = _blocks([4, 4])
    S[0, 1] = S[1, 0] = np.nan
    S[2, 5] = np.inf
    _same(S)


def test_cluster_random_matrices():
    rng = np.random.default_rng(0)
    for it in range(20):
        n = int(rng.integers(2, 60))
        A = rng.uniform(-0.2, 1.0, (n, n))
        A = ((A + A.T) / 2).astype(np.float32)
        if it % 3 == 0:
            A = np.round(A * 8) / 8                                        # many exact ties
        _same(A.astype(np.float32))
        _same(A.astype(np.float32), threshold=0.3, min_cluster=2)
        _same(A.astype(np.float32), num_speakers=int(rng.integers(1, 6)))


# ---- the two-source recording of the end-to-end tests ---------------------------------------------------------------------------
def test_two_source_reference_run_meets_the_margin_condition():
    """the constructed recording and model of the GPU end-to-end tests, in the definition alone (float64 fbank-to-labels on the
    CPU): the threshold finds the two sources, and no decision of the run lies within twice the cosine allowance (4 x the
    float16 emulation's deviation) of the threshold or of its runner-up, which is the condition under which the device's
    labels must equal these"""
    import fbank_ref as F
    import vad_ref as V
    rows = F.fbank_f32(R.two_source_audio())
    segs = V.segments(V.levels(rows), 80, V.config(**R.TWO_SOURCE_VAD))
    assert len(segs) == 4 and all(e - b <= R.TWO_SOURCE_SPK["win"] for b, e in segs)
    for (b, e), (b0, e0, _, _, _) in zip(segs, R.TWO_SOURCE_BURSTS):
        assert b <= b0 and e >= e0                                         # every burst inside its segment
    win, shift = R.stream_windows(segs, **R.TWO_SOURCE_SPK)
    assert [w[0] for w in win] == [0, 1, 2, 3] and shift == R.TWO_SOURCE_SPK["shift"]
    cfg, w = R.separating_model()
    S, allow = R.cosine_allowance(cfg, w, [rows[b:e] for _, b, e in win])
    margins = []
    labels, k = R.cluster(S.astype(np.float32), margins=margins)
    print("two sources: cosines %s, allowance %.3e, smallest margin %.3e" % (np.round(S[np.triu_indices(4, 1)], 4).tolist(), allow, min(margins)))
    assert k == 2 and labels.tolist() == [0, 1, 0, 1] == [0 if x[2] == "A" else 1 for x in R.TWO_SOURCE_BURSTS]
    assert 0 < allow < 0.01 and min(margins) > 2 * allow
    assert R.label_decisions_are_safe(S.astype(np.float32), allow)[2]
    assert S[0, 2] > 0.9 and S[1, 3] > 0.9 and max(S[0, 1], S[0, 3], S[1, 2], S[2, 3]) < 0.45
    # a cosine within the allowance of a decision is what the condition excludes
    assert not R.label_decisions_are_safe(S.astype(np.float32), 0.01)[2]


# ---- segment labels, centroids -------------------------------------------------------------------------------------------------
def test_segment_labels_and_centroids():
    segs = [(0, 100), (200, 300), (400, 500), (1000, 1100), (1150, 1200)]
    cases = [([0, 0, 0, 2, 2, 3], [1, 1, 0, 0, 1, 1], [1, 1, 0, 1, 1]),     # majority; a tie to the lower; 1 inherits from 0 (the nearer),
             ([2], [0], [0, 0, 0, 0, 0]),                                  # everyone from the one labelled segment
             ([0, 4], [0, 1], [0, 0, 0, 1, 1]),                            # 2: gaps 300 and 500 -> the earlier; 3: 50 to the later
             ([0, 3], [1, 0], [1, 1, 1, 0, 0]),                            # 1: 100 to 0, 700 to 3;  2: 300 / 500;  4 from 3
             ([], [], [-1] * 5), ([1], [-1], [-1] * 5)]
    for ws, wl, want in cases:
        assert R.segment_labels(segs, ws, wl).tolist() == want, (ws, wl)
        assert E.host_spk_segment_labels(segs, ws, wl).tolist() == want, (ws, wl)
    # a gap tie goes to the earlier segment
    segs2 = [(0, 100), (200, 300), (400, 500)]
    assert E.host_spk_segment_labels(segs2, [0, 2], [1, 0]).tolist() == R.segment_labels(segs2, [0, 2], [1, 0]).tolist() == [1, 1, 0]
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((9, 20)).astype(np.float32)
    emb[4] = 0
    labels = np.array([0, 1, 0, 2, 2, 1, 0, -1, 2], np.int32)
    got = E.host_spk_centroids(emb, labels, 4)
    want = R.centroids(emb, labels, 4)
    np.testing.assert_allclose(got, want, atol=1e-6)
    assert not got[3].any() and abs(float(np.linalg.norm(got[0])) - 1) < 1e-6
    assert E.host_spk_centroids(emb, labels, 0).shape == (0, 20)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_spk_option():
    from aliparaformerasr_amd.examples import parse_args, parse_spk_option
    base = ["-type", "offline", "-files", "a.wav"]
    cfg = parse_args(["-vad", "-spk", "cam.pfw"] + base)
    assert cfg["spk"] == {"file": "cam.pfw", "cfg": {}}
    cfg = parse_args(["-spk", "cam.pfw", "threshold=0.4,num_speakers=2,win=100", "-vad", "min_speech=30"] + base)
    assert cfg["spk"] == {"file": "cam.pfw", "cfg": {"threshold": 0.4, "num_speakers": 2, "win": 100}}
    assert "spk" not in parse_args(base)
    assert parse_spk_option("") == {}
    for bad in (["-spk"], ["-spk", "-files"]):
        with pytest.raises(ValueError, match="-spk takes"):
            parse_args(["-type", "offline", "-vad"] + bad)
    with pytest.raises(ValueError, match="-spk goes with -vad"):
        parse_args(["-spk", "cam.pfw"] + base)
    for text, msg in (("speakers=2", "Unknown -spk key"), ("win=x", "must be an integer"), ("threshold=high", "must be a number"),
                      ("threshold=nan", "must be a number"), ("win", "key=value")):
        with pytest.raises(ValueError, match=msg):
            parse_spk_option(text)
