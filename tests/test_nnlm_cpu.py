"""CPU: neural LM rescoring off the device — the host twin (pf_host_nnlm_logp) and the fusion (pf_host_nnlm_fuse) against the
definition in numpy float64 (tests/nnlm_ref.py); the `.pfw` container of kind "transformerlm" with its loader's refusals; the
converter's state-dict route; the loader once more under host sanitizers; and what the GPU test's tolerances rest on, asserted
on the reference alone."""
import os

import numpy as np
import pytest

import nnlm_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

SMALL = dict(vocab=37, embed=32, ffn=256)                  # the twin and the container do not need the released widths


def _model(n_layers=1, seed=5, **kw):
    cfg = W.transformer_lm_config(n_layers=n_layers, **dict(SMALL, **kw))
    return cfg, W.synth_nnlm_weights(cfg, seed=seed)


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_nnlm_model_load", "pf_nnlm_model_from_memory", "pf_nnlm_model_info", "pf_nnlm_model_free", "pf_engine_set_nnlm",
                 "pf_engine_nnlm_score", "pf_op_nnlm_logp", "pf_host_nnlm_logp", "pf_host_nnlm_fuse"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    lib.pf_nnlm_model_free(None)
    assert lib.pf_engine_set_nnlm(None, None) < 0
    assert lib.pf_nnlm_model_load(None, None) == N.PF_ERR_INVALID_ARG


@pytest.mark.parametrize("n_layers,kw", [(1, {}), (3, {}), (2, dict(vocab=2, embed=16)), (1, dict(vocab=64, embed=512, ffn=512))])
def test_host_logp_equals_the_definition(n_layers, kw):
    cfg, w = _model(n_layers, **kw)
    m = E.load_nnlm_model(W.pack_pfw(cfg, w))
    assert [m.dims[k] for k in ("vocab", "embed", "d_model", "heads", "ffn", "n_layers", "sos")] == \
        [cfg[k] for k in ("vocab", "embed", "d_model", "heads", "ffn", "n_layers")] + [cfg["vocab"] - 1]
    for n in (0, 1, 2, 7, 33, 70):
        ids = R.hyp_ids(n, cfg["vocab"], n)
        got, want = E.host_nnlm_logp(m, ids), R.logp64(w, cfg, ids)
        assert got.shape == want.shape == (n + 1,) and np.abs(got - want).max() <= 1e-9
    # causal: a later token changes nothing before it
    a = R.hyp_ids(20, cfg["vocab"], 1)
    b = a.copy()
    b[12] = (b[12] + 1) % cfg["vocab"]
    assert np.array_equal(E.host_nnlm_logp(m, a)[:12], E.host_nnlm_logp(m, b)[:12])
    m.close()


def test_fusion_and_sort():
    base, lm, n = [1.0, 2.0, 2.0, -1.0, 0.5], [0.0, -2.0, -2.0, 8.0, 1.0], [1, 2, 2, 3, 0]
    score, order = E.host_nnlm_fuse(base, lm, n, weight=0.5, bonus=0.0)
    assert score.tolist() == [1.0, 1.0, 1.0, 3.0, 1.0] and order.tolist() == [3, 0, 1, 2, 4]           # ties keep the list's order
    rng = np.random.default_rng(1)
    for N_ in (0, 1, 2, 17):
        base, lm, n = rng.standard_normal(N_), rng.standard_normal(N_).round(1), rng.integers(0, 4, N_)
        for weight, bonus in ((0.5, 0.0), (0.0, 1.0), (1.5, -0.25)):
            score, order = E.host_nnlm_fuse(base, lm, n, weight, bonus)
            want_s, want_o = R.fuse(base, lm, n, weight, bonus)
            assert np.array_equal(score, want_s) and order.tolist() == want_o.tolist() and np.isfinite(score).all()
    for bad in (dict(base=[np.nan]), dict(lm=[np.nan]), dict(weight=np.nan)):
        with pytest.raises(N.PfError) as ei:
            E.host_nnlm_fuse(bad.get("base", [0.0]), bad.get("lm", [0.0]), [1], bad.get("weight", 0.5))
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    # the eos flag: one more row in the sum
    lp = np.array([-1.5, -2.25, -0.125])
    assert R.lm_sum(lp, False) == -3.75 and R.lm_sum(lp, True) == -3.875
    assert R.lm_sum_f32(lp, False) == np.float32(-3.75) and R.lm_sum_f32(lp, True) == np.float32(-3.875)


def _refusals():
    cfg, w = _model(1)
    good = W.pack_pfw(cfg, w)

    def with_(**kw): return W.pack_pfw(dict(cfg, **kw), w)
    def tensor(name, fn):
        w2 = {k: v.copy() for k, v in w.items()}
        w2[name] = fn(w2[name])
        return W.pack_pfw(cfg, w2)
    def nan(a): a.reshape(-1)[3] = np.nan; return a
    inv = [("short", good[:40]), ("half", good[: len(good) // 2]), ("magic", b"XXXX" + good[4:]), ("kind", with_(kind="cttransformer")),
           ("nan", tensor("decoder.bias", nan)), ("shape", tensor("embed.weight", lambda a: a[:, :16].copy())),
           ("missing", W.pack_pfw(cfg, {k: v for k, v in w.items() if k != "after_norm.bias"})), ("no layers", with_(n_layers=0))]
    uns = [("d_model", with_(d_model=256)), ("heads", with_(heads=4)), ("ffn", with_(ffn=1000)), ("ffn large", with_(ffn=8192)),
           ("embed", with_(embed=24)), ("embed large", with_(embed=1024)), ("layers", with_(n_layers=25)), ("vocab", with_(vocab=1))]
    return good, inv, uns


def test_container_and_argument_refusals():
    good, inv, uns = _refusals()
    m = E.load_nnlm_model(good)
    for blobs, code in ((inv, N.PF_ERR_INVALID_ARG), (uns, N.PF_ERR_UNSUPPORTED)):
        for name, blob in blobs:
            with pytest.raises(N.PfError) as ei:
                E.load_nnlm_model(blob)
            assert ei.value.code == code, name
    for ids in ([37], [-1], [0] * 256):                       # an id >= V, a negative id, n > 255
        with pytest.raises(N.PfError) as ei:
            E.host_nnlm_logp(m, ids)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    assert E.host_nnlm_logp(m, [36] * 255).shape == (256,)
    m.close()


def test_converter_state_dict_route(tmp_path):
    torch = pytest.importorskip("torch")
    from aliparaformerasr_amd import convert as cv
    cfg, w = _model(2)
    sd = {"embed.weight": w["embed.weight"]}
    for dst, src in (("encoder.embed.0", "input.linear"), ("encoder.embed.1", "input.norm"), ("encoder.after_norm", "after_norm"),
                     ("decoder", "decoder")):
        sd[dst + ".weight"], sd[dst + ".bias"] = w[src + ".weight"], w[src + ".bias"]
    D = cfg["d_model"]
    for l in range(2):
        s, p = "encoder.encoders.%d." % l, "layers.%d." % l
        for i, x in enumerate("qkv"):
            sd[s + "self_attn.linear_%s.weight" % x] = w[p + "attn.qkv.weight"][i * D:(i + 1) * D]
            sd[s + "self_attn.linear_%s.bias" % x] = w[p + "attn.qkv.bias"][i * D:(i + 1) * D]
        for dst, src in (("norm1", "norm1"), ("norm2", "norm2"), ("self_attn.linear_out", "attn.out"), ("feed_forward.w_1", "ffn.w1"),
                         ("feed_forward.w_2", "ffn.w2")):
            sd[s + dst + ".weight"], sd[s + dst + ".bias"] = w[p + src + ".weight"], w[p + src + ".bias"]
    cfg2, w2 = cv.nnlm_state_dict_to_pfw(sd)
    assert cfg2 == cfg and set(w2) == set(w) and all(np.array_equal(w2[k], w[k]) for k in w)
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, str(tmp_path / "lm.pt"))
    assert cv.main([str(tmp_path / "lm.pt"), str(tmp_path / "lm.pfw"), "--kind", "transformerlm"]) == 0
    m = E.load_nnlm_model(str(tmp_path / "lm.pfw"))
    ids = R.hyp_ids(19, cfg["vocab"], 3)
    assert np.abs(E.host_nnlm_logp(m, ids) - R.logp64(w, cfg, ids)).max() <= 1e-9
    m.close()
    for drop in ("decoder.bias", "encoder.encoders.1.norm2.weight", "encoder.embed.1.bias"):
        with pytest.raises(ValueError):
            cv.nnlm_state_dict_to_pfw({k: v for k, v in sd.items() if k != drop})


def test_loader_under_sanitizers(tmp_path):
    """csrc/nnlm.cpp in a stand-alone program (tests/native/nnlm_sanitize.cpp) built with AddressSanitizer + UBSan on the host
    code, over a good container and the malformed ones: no report, the library's own status codes, logp and order."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "nnlm_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "nnlm_sanitize.cpp"),
                        os.path.join(cs, "nnlm.cpp"), os.path.join(cs, "pfw.cpp"), os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a compile error in the sources under test is a failure
        missing = any(t in b.stderr for t in ("libclang_rt.asan", "libclang_rt.ubsan", "cannot find -lclang_rt", "unsupported option '-fsanitize"))
        assert missing, b.stderr[-3000:]
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    good, inv, uns = _refusals()
    paths = []
    for i, blob in enumerate([good] + [x for _, x in inv] + [x for _, x in uns]):
        p = tmp_path / ("c%d.pfw" % i)
        p.write_bytes(blob)
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[1:] == ["refused %d" % N.PF_ERR_INVALID_ARG] * len(inv) + ["refused %d" % N.PF_ERR_UNSUPPORTED] * len(uns)
    cfg, w = _model(1)
    m = E.load_nnlm_model(good)
    head, tail = lines[0].split("|")
    assert head.split() == ["ok", str(cfg["vocab"]), str(cfg["embed"]), "1", str(m.image_bytes), "3012"]
    ids = [(7 * t + 3) % cfg["vocab"] for t in range(9)]
    assert [float(x) for x in tail.split()] == E.host_nnlm_logp(m, ids).tolist()[:9] + E.host_nnlm_logp(m, []).tolist()
    m.close()


# ---- what the GPU test's tolerances rest on (tests/test_gpu_nnlm.py uses these models and figures) -------------------------------
@pytest.mark.parametrize("V,n_layers", R.GPU_CASES)
def test_reference_deviation_and_ranking_cap(V, n_layers):
    """dev_f16 = max |emulate_f16 - float64| over logp is small and not zero, and at most 5 % of the adjacent pairs of the ranking
    lists lie inside the band 2 * weight * (n + 1) * 4 * dev_f16 in which the device may order them either way."""
    cfg, w = R.gpu_case(V, n_layers)
    dev, _ = R.deviation(w, cfg)
    assert 0 < dev < 0.02
    unsafe = []
    for hyps, base in R.ranking_lists(V):
        n = [len(h) for h in hyps]
        score, order = R.fuse(base, [R.lm_sum(R.logp64(w, cfg, h), False) for h in hyps], n, R.WEIGHT, R.BONUS)
        unsafe.append(R.unsafe_pairs(score, order, n, dev))
    unsafe = np.concatenate(unsafe)
    print("nnlm V=%d n_layers=%d: dev_f16 %.3e, %d of %d adjacent pairs inside the band" % (V, n_layers, dev, int(unsafe.sum()), unsafe.size))
    assert unsafe.mean() <= 0.05
