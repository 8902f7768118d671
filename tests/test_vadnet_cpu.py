"""CPU: the FSMN-VAD model score off the device — the host twins (pf_host_vad_model_logits / _levels) against the definition
in numpy float64 (tests/vadnet_ref.py), the `.pfw` container of kind "fsmnvad" with its loader's refusals, the converter's
state-dict and ONNX routes (tests/fsmn_vad_like.py), pf_vad_model_config and the `-vadmodel` option."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from pfw_helpers import repack
import vad_ref as V
import vadnet_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import convert as cv
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

MODELS = {"small": R.small_model, "released": R.released_model}


@pytest.fixture(scope="module", params=["small", "released"])
def model(request):
    cfg, w = MODELS[request.param]()
    m = E.load_vad_model(W.pack_pfw(cfg, w))
    yield request.param, cfg, w, m
    m.close()


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_vad_model_load", "pf_vad_model_from_memory", "pf_vad_model_info", "pf_vad_model_sil_ids", "pf_vad_model_tensor",
                 "pf_vad_model_config", "pf_vad_model_free", "pf_host_vad_model_logits", "pf_host_vad_model_levels",
                 "pf_engine_set_vad_model", "pf_op_vad_model_logits", "pf_op_vad_model_levels", "pf_recognizer_set_vad_model"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    lib.pf_vad_model_free(None)
    assert lib.pf_engine_set_vad_model(None, None) < 0 and lib.pf_recognizer_set_vad_model(None, None) < 0
    assert lib.pf_vad_model_load(None, None) == N.PF_ERR_INVALID_ARG


# ---- the host twin -------------------------------------------------------------------------------------------------------
def test_host_twin_equals_the_definition(model):
    name, cfg, w, m = model
    assert m.dims == {k: cfg[k] for k in E.VAD_MODEL_DIMS} and m.sil_ids == cfg["sil_ids"]
    lengths = (R.LENGTHS_RELEASED if name == "released" else R.LENGTHS_SMALL) + [400]
    frames = excluded = 0
    for T in lengths:
        x = R.fbank_like(T, cfg["n_mels"], 31 * T + 1)
        z = E.host_vad_model_logits(m, x)
        want = R.logits(cfg, w, x)
        assert z.shape == want.shape == (T, cfg["output_dim"])
        if T:
            assert float(np.abs(z - want).max()) <= 1e-9
        v = R.unrounded_levels(cfg, want)
        keep = np.abs(v - np.floor(v) - 0.5) > 1e-6                  # not within 1e-6 of a half-integer
        frames += T
        excluded += int((~keep).sum())
        e = E.host_vad_model_levels(m, x)
        assert e.dtype == np.int32
        np.testing.assert_array_equal(e[keep], R.levels_from_logits(cfg, want)[keep])
    assert excluded <= frames // 1000                                 # at most 0.1 % of the frames are left out


def test_chunk_invariance_and_independence_of_batch_mates(model):
    name, cfg, w, m = model
    x = R.fbank_like(500, cfg["n_mels"], 9)
    whole = E.host_vad_model_logits(m, x)
    h = R.halo(cfg)
    assert h == cfg["n_layers"] * (cfg["lorder"] - 1) * cfg["lstride"] + 2
    for a, b in ((h + 120, h + 190), (250, 500)):
        # frames [a, b) with only the halo in front (and two frames behind: the LFR window looks (lfr_m - 1) / 2 ahead)
        right = min(b + 2, 500)
        part = E.host_vad_model_logits(m, x[a - h: right])
        np.testing.assert_allclose(part[h: h + (b - a)], whole[a:b], rtol=0, atol=1e-9)
        refp = R.logits(cfg, w, x[a - h: right])
        np.testing.assert_allclose(refp[h: h + (b - a)], R.logits(cfg, w, x)[a:b], rtol=0, atol=1e-9)
    # one frame less of halo is not enough for the definition (the bound is tight)
    short = R.logits(cfg, w, x[251 - h: 400])
    assert float(np.abs(short[h - 1] - R.logits(cfg, w, x)[250]).max()) > 1e-6
    # the twin takes ONE utterance: the same rows give the same answer whatever was computed before
    other = E.host_vad_model_logits(m, R.fbank_like(77, cfg["n_mels"], 10))
    assert other.shape[0] == 77
    np.testing.assert_array_equal(E.host_vad_model_logits(m, x), whole)


def test_poisoned_rows_follow_the_definition(model):
    name, cfg, w, m = model
    x = R.fbank_like(90, cfg["n_mels"], 4)
    x[10, 0], x[10, 1], x[10, 2] = np.nan, np.inf, -np.inf
    z, want = E.host_vad_model_logits(m, x), R.logits(cfg, w, x)
    assert (np.isfinite(z) == np.isfinite(want)).all()
    fin = np.isfinite(want)
    np.testing.assert_allclose(z[fin], want[fin], rtol=0, atol=1e-9)
    e = E.host_vad_model_levels(m, x)
    bad = ~np.isfinite(want).all(axis=1)
    assert bad[8:13].all() and not bad[:8].any() and (e[bad] == -16384).all()


def test_shape_refusals(model):
    name, cfg, w, m = model
    with pytest.raises(N.PfError) as ei:
        E.host_vad_model_logits(m, np.zeros((4, cfg["n_mels"] + 1), np.float32))
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        m.tensor("no.such.tensor")
    assert ei.value.code == N.PF_ERR_INVALID_ARG


# ---- the container ---------------------------------------------------------------------------------------------------------
def test_container_round_trip(model, tmp_path):
    name, cfg, w, m = model
    for k, a in w.items():
        np.testing.assert_array_equal(m.tensor(k), np.asarray(a, np.float32).reshape(-1), err_msg=k)
    path = str(tmp_path / "vad.pfw")
    W.save_pfw(path, cfg, w)
    m2 = E.load_vad_model(path)
    try:
        assert m2.dims == m.dims and m2.sil_ids == m.sil_ids and m2.image_bytes == m.image_bytes > 0
        for k in w:
            np.testing.assert_array_equal(m2.tensor(k), m.tensor(k))
    finally:
        m2.close()
    cfg2, w2 = W.load_pfw(path)
    assert cfg2 == json.loads(json.dumps(cfg)) and set(w2) == set(W.vad_tensor_shapes(cfg))


def _refused(blob, code=N.PF_ERR_INVALID_ARG):
    with pytest.raises(N.PfError) as ei:
        E.load_vad_model(blob)
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def test_malformed_containers_are_refused():
    cfg, w = R.small_model()
    good = W.pack_pfw(cfg, w)
    E.load_vad_model(good).close()
    # truncated: inside the magic, the header, the last tensor's data (its 20 bytes are followed by 236 of padding), further in
    for cut in (3, 15, 40, len(good) - 237, len(good) - 300, len(good) // 2):
        _refused(good[:cut])
    _refused(b"PFW2" + good[4:])
    _refused(good[:8] + struct.pack("<Q", 1 << 62) + good[16:])                  # a header length beyond the file
    _refused(good[:16] + b"{" * 10 + good[26:])                                 # a header that is no JSON
    # lying sizes: an extent outside the file, nbytes that disagrees with the shape, a negative offset
    def far(h): h["tensors"][3]["offset"] = 1 << 40
    def big(h): h["tensors"][-1]["nbytes"] = h["tensors"][-1]["nbytes"] + 4096
    def neg(h): h["tensors"][0]["offset"] = -256
    def mism(h): h["tensors"][2]["shape"] = [h["tensors"][2]["shape"][0] + 1, h["tensors"][2]["shape"][1]]
    for edit in (far, big, neg, mism):
        _refused(repack(cfg, w, edit))
    # wrong kind, a recogniser's container
    def kind(h): h["config"]["kind"] = "paraformer"
    _refused(repack(cfg, w, kind))
    pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=16)
    _refused(W.pack_pfw(pcfg, {"encoder.after_norm.weight": np.ones(512, np.float32)}))
    # a weight that is not finite, a shape that does not follow the dimensions, a missing tensor, a bad silence id
    for bad in (np.nan, np.inf):
        w2 = {k: v.copy() for k, v in w.items()}
        w2["fsmn.1.affine.weight"][3, 2] = bad
        _refused(W.pack_pfw(cfg, w2))
    w2 = dict(w); w2["in2.weight"] = w["in2.weight"][:, :-1]
    _refused(W.pack_pfw(cfg, w2))
    w2 = dict(w); w2["fsmn.0.taps"] = np.ascontiguousarray(w["fsmn.0.taps"].T)
    _refused(W.pack_pfw(cfg, w2))
    w2 = dict(w); del w2["out1.bias"]
    _refused(W.pack_pfw(cfg, w2))
    _refused(W.pack_pfw(dict(cfg, sil_ids=[0, cfg["output_dim"]]), w))
    _refused(W.pack_pfw(dict(cfg, sil_ids=[]), w))
    _refused(W.pack_pfw(dict(cfg, n_layers=0), w))
    # unsupported, not invalid
    _refused(W.pack_pfw(dict(cfg, rorder=1), w), N.PF_ERR_UNSUPPORTED)
    _refused(W.pack_pfw(dict(cfg, lfr_n=2), w), N.PF_ERR_UNSUPPORTED)
    _refused(W.pack_pfw(dict(cfg, lorder=200), w), N.PF_ERR_UNSUPPORTED)         # (lorder - 1) * lstride = 398 > 256
    wide = W.fsmn_vad_config(linear_dim=520)
    _refused(W.pack_pfw(wide, W.synth_vad_weights(wide, 1)), N.PF_ERR_UNSUPPORTED)
    with pytest.raises(N.PfError):
        E.load_vad_model("/nonexistent/vad.pfw")


# ---- the converter -----------------------------------------------------------------------------------------------------------
def _funasr_state_dict(cfg, w):
    sd = {}
    for pk, fk in cv.vad_name_map(cfg["n_layers"]).items():
        a = np.asarray(w[pk], np.float32)
        sd[fk] = a.T[:, None, :, None].copy() if pk.endswith(".taps") else a
    return sd


@pytest.mark.parametrize("name", ["small", "released"])
def test_state_dict_route(name, tmp_path):
    cfg, w = MODELS[name]()
    sd = _funasr_state_dict(cfg, w)
    assert "encoder.fsmn.0.fsmn_block.conv_left.weight" in sd and sd["encoder.fsmn.0.fsmn_block.conv_left.weight"].shape == \
        (cfg["proj_dim"], 1, cfg["lorder"], 1)
    cfg2, w2 = cv.vad_state_dict_to_pfw(sd, w["cmvn.shift"], w["cmvn.scale"], cfg["sil_ids"], cfg["lfr_m"], cfg["lstride"])
    assert cfg2 == cfg
    m = E.load_vad_model(W.pack_pfw(cfg2, w2))
    try:
        for k, a in w.items():
            np.testing.assert_array_equal(m.tensor(k), a.reshape(-1), err_msg=k)
    finally:
        m.close()
    del sd["encoder.out_linear2.linear.bias"]
    with pytest.raises(KeyError):
        cv.vad_state_dict_to_pfw(sd, w["cmvn.shift"], w["cmvn.scale"])
    sd = _funasr_state_dict(cfg, w)
    sd["encoder.fsmn.0.fsmn_block.conv_right.weight"] = sd["encoder.fsmn.0.fsmn_block.conv_left.weight"]
    with pytest.raises(ValueError, match="rorder"):
        cv.vad_state_dict_to_pfw(sd, w["cmvn.shift"], w["cmvn.scale"])


@pytest.mark.parametrize("name,opset", [("small", 17), ("small", 13), ("released", 17)])
def test_onnx_route_through_the_command_line(name, opset, tmp_path):
    """an export of tests/fsmn_vad_like.py (the small model has lstride = 2) -> convert's main -> load_vad_model: every
    tensor comes back; the torch module itself agrees with the definition"""
    torch = pytest.importorskip("torch")
    import fsmn_vad_like as L
    from aliparaformerasr_amd import onnx_reader as OR
    cfg, w = MODELS[name]()
    mod = L.FsmnVadLike(cfg)
    L.load_pfw_weights(mod, cfg, w)
    x = R.fbank_like(40, cfg["n_mels"], 2)
    u = R.splice(cfg, w, x, np.float32).astype(np.float32)
    z = mod.logits(torch.from_numpy(u[None])).detach().numpy()[0]
    assert float(np.abs(z - R.logits(cfg, w, x)).max()) < 2e-5
    blob = L.export(mod, opset=opset)
    g = OR.load(blob)
    assert g.inputs[0] == "speech"
    assert [i for i in g.inputs if i.startswith("in_cache")] == ["in_cache%d" % l for l in range(cfg["n_layers"])]
    assert [o for o in g.outputs if o.startswith("out_cache")] == ["out_cache%d" % l for l in range(cfg["n_layers"])]
    assert any(n.op_type == "Softmax" for n in g.nodes)               # the export ends in one; the converter passes over it
    assert not any(k.endswith("linear.weight") for k in g.initializers)          # the exporter anonymised the MatMul weights
    (tmp_path / "vad.onnx").write_bytes(blob)
    (tmp_path / "vad.mvn").write_text(W.format_mvn_text(w["cmvn.shift"], w["cmvn.scale"]))
    out = str(tmp_path / "out.pfw")
    args = [str(tmp_path / "vad.onnx"), out, "--kind", "fsmnvad", "--mvn", str(tmp_path / "vad.mvn"), "--sil",
            ",".join(str(i) for i in cfg["sil_ids"])]
    assert cv.main(args) == 0
    cfg2, _ = W.load_pfw(out)
    assert cfg2 == json.loads(json.dumps(cfg)) and cfg2["lstride"] == cfg["lstride"]
    m = E.load_vad_model(out)
    try:
        for k, a in w.items():
            np.testing.assert_array_equal(m.tensor(k), a.reshape(-1), err_msg=k)
    finally:
        m.close()
    assert cv.main([str(tmp_path / "vad.onnx"), out, "--kind", "fsmnvad"]) == 2    # --mvn is required


def test_pt_route_through_the_command_line(tmp_path):
    torch = pytest.importorskip("torch")
    cfg, w = R.small_model()
    sd = {k: torch.from_numpy(v) for k, v in _funasr_state_dict(cfg, w).items()}
    torch.save(sd, str(tmp_path / "vad.pt"))
    (tmp_path / "vad.mvn").write_text(W.format_mvn_text(w["cmvn.shift"], w["cmvn.scale"]))
    out = str(tmp_path / "out.pfw")
    assert cv.main([str(tmp_path / "vad.pt"), out, "--kind", "fsmnvad", "--mvn", str(tmp_path / "vad.mvn"), "--sil", "0,3",
                    "--lstride", "2"]) == 0
    cfg2, w2 = W.load_pfw(out)
    assert cfg2 == json.loads(json.dumps(cfg))
    for k in w:
        np.testing.assert_array_equal(w2[k], w[k])


def test_a_graph_of_another_shape_is_refused():
    from aliparaformerasr_amd import onnx_reader as OR
    g = OR.Graph()
    g.inputs = ["speech"]
    with pytest.raises(ValueError):
        cv.vad_onnx_to_state_dict(g)
    g.inputs = ["x"]
    with pytest.raises(ValueError):
        cv.vad_onnx_to_state_dict(g)


def test_mvn_parsing():
    rng = np.random.default_rng(3)
    shift, scale = rng.standard_normal(400).astype(np.float32), rng.uniform(0.1, 3, 400).astype(np.float32)
    s2, c2 = cv.parse_mvn_text(W.format_mvn_text(shift, scale))
    np.testing.assert_array_equal(s2, shift)
    np.testing.assert_array_equal(c2, scale)
    with pytest.raises(ValueError):
        cv.parse_mvn_text("<Nnet>\n</Nnet>\n")


# ---- the model's default configuration ------------------------------------------------------------------------------------------
def test_model_config_values_and_the_threshold_at_9830():
    c, d = E.vad_model_config(), E.vad_config()
    assert (c.floor_pct, c.abs_level) == (-1, 9830)
    for f in ("struct_size", "margin_q", "window", "on_count", "off_count", "pad_begin", "pad_end", "min_speech", "max_len", "split_search"):
        assert getattr(c, f) == getattr(d, f), f
    assert (c.window, c.on_count, c.off_count) == (20, 15, 15)
    # raw[t] = e[t] > 9830: a run at 9831 is speech, the same run at 9830 is not
    quiet, n = -16000, 100
    lev = lambda v: np.concatenate([np.full(100, quiet), np.full(n, v), np.full(100, quiet)]).astype(np.int32)
    assert [tuple(p) for p in E.host_vad_segments(lev(9831), 80, c).tolist()] == [(84, 219)]
    assert E.host_vad_segments(lev(9830), 80, c).tolist() == []
    assert [tuple(p) for p in E.host_vad_segments(lev(9831), 80, c).tolist()] == V.segments(lev(9831), 80, V.config(floor_pct=-1, abs_level=9830))
    # 14 frames above in a window of 20 do not switch on, 15 do; no percentile floor is involved (floor_pct = -1)
    mixed = lev(9830)
    mixed[100:114] = 9831
    assert E.host_vad_segments(mixed, 80, c).tolist() == []
    mixed[114] = 9831
    mixed[115:165] = 9831
    assert len(E.host_vad_segments(mixed, 80, c)) == 1


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_vadmodel_option():
    from aliparaformerasr_amd.examples import parse_args
    base = ["-type", "offline", "-files", "a.wav"]
    cfg = parse_args(base + ["-vad", "-vadmodel", "vad.pfw"])
    assert cfg["vadmodel"] == "vad.pfw" and cfg["vad"]["cfg"] == {}
    cfg = parse_args(base + ["-vadmodel", "m.pfw", "-vad", "abs_level=5000,pad_end=9"])
    assert cfg["vadmodel"] == "m.pfw" and cfg["vad"]["cfg"] == {"abs_level": 5000, "pad_end": 9}
    with pytest.raises(ValueError, match="-vadmodel goes with -vad"):
        parse_args(base + ["-vadmodel", "vad.pfw"])
    with pytest.raises(ValueError, match="-vadmodel takes"):
        parse_args(base + ["-vad", "-vadmodel"])
    with pytest.raises(ValueError, match="-vadmodel takes"):
        parse_args(base + ["-vad", "-vadmodel", "-files"])
    assert "vadmodel" not in parse_args(base + ["-vad"])


# ---- the loader once more, under sanitizers ------------------------------------------------------------------------------------------
def test_loader_under_sanitizers(tmp_path):
    """csrc/vadnet.cpp in a stand-alone program (tests/native/vadnet_sanitize.cpp) built with AddressSanitizer + UBSan on the host
    code, over a good container and the malformed ones: no report, the library's own status codes and levels."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "vadnet_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "vadnet_sanitize.cpp"),
                        os.path.join(cs, "vadnet.cpp"), os.path.join(cs, "pfw.cpp"), os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if b.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a compile error in the sources under test is a failure
        missing = any(t in b.stderr for t in ("libclang_rt.asan", "libclang_rt.ubsan", "cannot find -lclang_rt", "unsupported option '-fsanitize"))
        assert missing, b.stderr[-3000:]
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    cfg, w = R.small_model()
    good = W.pack_pfw(cfg, w)
    w_nan = {k: v.copy() for k, v in w.items()}
    w_nan["out2.bias"][1] = np.nan

    def far(h): h["tensors"][3]["offset"] = 1 << 40
    def big(h): h["tensors"][-1]["nbytes"] = h["tensors"][-1]["nbytes"] + 4096
    blobs = [good, good[:40], good[: len(good) - 237], good[: len(good) // 2], repack(cfg, w, far), repack(cfg, w, big),
             W.pack_pfw(cfg, w_nan), W.pack_pfw(dict(cfg, kind="paraformer"), w), W.pack_pfw(dict(cfg, rorder=2), w),
             good[:8] + struct.pack("<Q", (1 << 64) - 8) + good[16:], b""]
    paths = []
    for i, blob in enumerate(blobs):
        p = tmp_path / ("c%d.pfw" % i)
        p.write_bytes(blob)
        paths.append(str(p))
    r = subprocess.run([exe, str(cfg["n_mels"])] + paths, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(blobs)
    m = E.load_vad_model(good)
    try:
        rows = np.array([float(int(((k * 2654435761) & 0xFFFFFFFF) >> 24) % 13) * 0.5 - 4.0 for k in range(37 * cfg["n_mels"])],
                        np.float32).reshape(37, cfg["n_mels"])
        want = E.host_vad_model_levels(m, rows).tolist()
        assert lines[0].split() == ["ok", str(cfg["input_dim"]), str(cfg["output_dim"]), str(cfg["n_layers"]), str(m.image_bytes)] + [str(e) for e in want]
    finally:
        m.close()
    assert lines[1:] == ["refused %d" % N.PF_ERR_INVALID_ARG] * 7 + ["refused %d" % N.PF_ERR_UNSUPPORTED] + ["refused %d" % N.PF_ERR_INVALID_ARG] * 2
