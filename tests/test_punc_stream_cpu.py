"""CPU: streaming punctuation.  The float64 host twin (pf_host_punc_stream_step, pf_host_punc_logits on a
causal model) against the numpy definition tests/punc_stream_ref.py: the network, every branch of the loop, the flush, the
committed words of the definition; the two new header keys of the container; the loader and the twin once more under host
sanitizers in a stand-alone program.  All vocabularies are 64."""
import os

import numpy as np
import pytest

import punc_ref as R
import punc_stream_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

UNK, NONE, COMMA, PERIOD, QUESTION, PAUSE = 0, 1, 2, 3, 4, 5
NR = S.NO_RESTARTS


def _model(n_layers, seed=42, kernel=11):
    cfg = W.ct_transformer_config(vocab=64, n_layers=n_layers, kernel=kernel)
    return S.causal_config(cfg), W.synth_punc_weights(cfg, seed=seed)


def _load(cfg, w):
    return E.load_punc_model(W.pack_pfw(cfg, w))


@pytest.fixture(scope="module")
def model():
    cfg, w = _model(2)
    m = _load(cfg, w)
    yield cfg, w, m
    m.close()


def _biased(cls, n_layers=1):
    """a model whose every word is marked `cls`: a zero decoder weight and a bias that picks the class"""
    cfg, w = _model(n_layers, seed=3)
    w = dict(w)
    w["decoder.weight"] = np.zeros_like(w["decoder.weight"])
    b = np.zeros(6, np.float32)
    b[cls] = 1.0
    w["decoder.bias"] = b
    return cfg, w


def _host(m, ids, calls, flush=False, max_context=S.DEFAULT_CONTEXT, flags=0):
    """the stream `ids` through the host twin in calls of the given sizes; the flush with the last call"""
    st = E.punc_stream_state(m, host=True)
    mk, mf, zs, at, fm = [], [], [], 0, -1
    for k, n in enumerate(calls):
        a, b, z, fm = E.host_punc_stream_step(m, st, ids[at: at + n], flush=flush and k == len(calls) - 1, max_context=max_context, flags=flags)
        mk.append(a); mf.append(b); zs.append(z)
        at += n
    assert at == len(ids)
    return np.concatenate(mk), np.concatenate(mf), np.concatenate(zs), fm, st


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_punc_model_causal", "pf_punc_stream_state_bytes", "pf_host_punc_stream_state_bytes", "pf_host_punc_stream_step",
                 "pf_op_punc_stream_step", "pf_host_online_committed_words", "pf_online_recognizer_set_punc_model",
                 "pf_online_stream_punctuated", "pf_online_stream_sentence_punctuated"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.pf_punc_stream_state_bytes(None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_op_punc_stream_step(None, None, None, None, None, 0, 0, 200, 0, None, None, None, None) < 0


def test_state_sizes(model):
    cfg, w, m = model
    assert m.causal and E.punc_stream_state(m).size == 2 * 256 * 2 * 256 * 2 + 16
    assert E.punc_stream_state(m, host=True).size == 2 * 256 * 2 * 256 * 8 + 16
    assert E.punc_stream_state(m, B=3).shape == (3, 2 * 256 * 2 * 256 * 2 + 16)


# ---- the tolerance the GPU test relies on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [1, 2, 3, 4])
def test_reference_margin_meets_the_cap(n_layers):
    """§4.6l's rule on the causal network: the allowance is 4 x the largest deviation of the f16 emulation from float64, and over
    the contexts of 1 .. 256 words at most 5 % of the positions have a float64 top-2 margin within twice the allowance.
    Measured (seed 42): 2.2e-3 / 2.1 %, 1.9e-3 / 1.9 %, 2.0e-3 / 2.4 %, 2.2e-3 / 1.9 % at 1, 2, 3, 4 layers."""
    cfg, w = _model(n_layers)
    dev, margins = S.deviation_and_margin(w, cfg)
    print("layers %d: emulation deviation %.3g, positions outside the margin %.2f %%" % (n_layers, dev, 100 * float((margins <= 8 * dev).mean())))
    assert 0 < dev < 0.05
    assert float((margins <= 2 * 4 * dev).mean()) <= 0.05


# ---- the network ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [1, 2, 4])
def test_host_twin_equals_the_definition(n_layers):
    cfg, w = _model(n_layers)
    m = _load(cfg, w)
    for T in ([1, 2, 10, 11, 12, 33, 65, 256] if n_layers == 2 else [1, 12, 65]):
        ids = R.window_ids(T, 64, T)
        z = S.logits64(w, cfg, ids)
        assert np.abs(E.host_punc_logits(m, ids) - z).max() <= 1e-9
        mk, mf, zs, fm, _ = _host(m, ids, [T], flags=NR)
        assert np.abs(zs - z).max() <= 1e-9 and fm == -1
        assert mk.tolist() == R.argmax_ties_larger(z).tolist() and not mf.any()
    m.close()


def test_prefix_property(model):
    """the logits of a context's first 20 words are those of the 20-word context"""
    cfg, w, m = model
    ids = R.window_ids(64, 64, 7)
    assert np.abs(S.logits64(w, cfg, ids)[:20] - S.logits64(w, cfg, ids[:20])).max() <= 1e-12
    assert np.abs(E.host_punc_logits(m, ids)[:20] - E.host_punc_logits(m, ids[:20])).max() <= 1e-12
    full = _host(m, ids, [64], flags=NR)[2]
    assert np.abs(full[:20] - _host(m, ids[:20], [20], flags=NR)[2]).max() <= 1e-12


@pytest.mark.parametrize("flags,max_context", [(NR, 200), (0, 9), (0, 200)])
def test_any_split_gives_the_same_stream(model, flags, max_context):
    cfg, w, m = model
    ids = R.window_ids(90, 64, 11)
    want = _host(m, ids, [90], flush=True, max_context=max_context, flags=flags)
    rng = np.random.default_rng(5)
    splits = [[1] * 90, [0, 45, 0, 45, 0], [89, 1], [1, 89]]
    for _ in range(3):
        cuts = np.sort(rng.integers(0, 91, size=6))
        splits.append(np.diff(np.concatenate([[0], cuts, [90]])).tolist())
    for calls in splits:
        got = _host(m, ids, calls, flush=True, max_context=max_context, flags=flags)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[3] == want[3], calls
        assert np.abs(got[2] - want[2]).max() <= 1e-12
        assert np.array_equal(got[4][-16:], want[4][-16:])


# ---- the loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_context", [2, 5, 39, 40, 256])
def test_loop_equals_the_definition(model, max_context):
    cfg, w, m = model
    ids = R.window_ids(40, 64, 3)
    ref = S.Stream(lambda c: S.logits64(w, cfg, c), cfg["punc_list"], cfg["sentence_end_id"], max_context=max_context)
    mk, mf, z, fm = ref.step(ids[:25])
    mk2, mf2, z2, fm2 = ref.step(ids[25:], flush=True)
    got = _host(m, ids, [25, 15], flush=True, max_context=max_context)
    assert got[0].tolist() == mk.tolist() + mk2.tolist() and got[1].tolist() == mf.tolist() + mf2.tolist()
    assert np.abs(got[2] - np.concatenate([z, z2])).max() <= 1e-9 and fm == -1 and got[3] == fm2
    # the rule alone over the twin's own logits
    p, f, _ = S.loop_from_logits(got[2], cfg["punc_list"], cfg["sentence_end_id"], max_context)
    assert p.tolist() == got[0].tolist() and f.tolist() == got[1].tolist()
    if max_context == 2:
        assert 2 in got[1].tolist() and 1 in got[1].tolist()


def test_sentence_ends_at_the_first_word_the_last_word_and_two_in_a_row(model):
    cfg, w, m = model
    first = R.argmax_ties_larger(np.stack([S.logits64(w, cfg, np.array([i], np.int32))[0] for i in range(64)]))
    ends = [i for i in range(64) if first[i] in (PERIOD, QUESTION)]
    plain = [i for i in range(64) if first[i] not in (PERIOD, QUESTION)]
    assert ends and plain
    e, x = ends[0], plain[0]
    ids = np.array([e, e, x, e], np.int32)                     # every word behind an end is the first of a fresh context
    mk, mf, _, fm, st = _host(m, ids, [4], flush=True)
    assert mf[:2].tolist() == [1, 1] and mk[0] == mk[1] == first[e]
    ref = S.Stream(lambda c: S.logits64(w, cfg, c), cfg["punc_list"], cfg["sentence_end_id"]).step(ids, flush=True)
    assert mk.tolist() == ref[0].tolist() and mf.tolist() == ref[1].tolist() and fm == ref[3]
    if mf[3] == 1:
        assert fm == -1 and st[-16:].view(np.int32).tolist() == [0, 0, 0, 0]


def test_forced_restarts_with_a_constant_mark():
    cfg, w = _biased(NONE)
    m = _load(cfg, w)
    ids = R.window_ids(256, 64, 1)
    for mc, n in ((2, 7), (255, 256), (256, 256), (256, 255)):
        mk, mf, _, fm, st = _host(m, ids[:n], [n], max_context=mc)
        assert mk.tolist() == [NONE] * n
        assert mf.tolist() == [2 if (i + 1) % mc == 0 else 0 for i in range(n)]
        assert st[-16:].view(np.int32).tolist() == [n % mc, NONE if n % mc else 0, 0, 0]
    m.close()


@pytest.mark.parametrize("cls", [UNK, NONE, COMMA, PERIOD, QUESTION, PAUSE])
def test_flush_on_each_class_and_on_an_empty_context(cls):
    cfg, w = _biased(cls)
    m = _load(cfg, w)
    ids = np.array([5, 6, 7], np.int32)
    mk, mf, _, fm, st = _host(m, ids, [3], flush=True)
    assert mk.tolist() == [cls] * 3
    want = {UNK: UNK, NONE: cfg["sentence_end_id"], COMMA: cfg["sentence_end_id"], PAUSE: cfg["sentence_end_id"], PERIOD: -1, QUESTION: -1}[cls]
    assert fm == want and mf.tolist() == ([1, 1, 1] if cls in (PERIOD, QUESTION) else [0, 0, 0])
    assert not st[-16:].any()
    # a flush in a call of its own finds the mark in the state; a second flush finds an empty context
    st = E.punc_stream_state(m, host=True)
    E.host_punc_stream_step(m, st, ids)
    assert E.host_punc_stream_step(m, st, [], flush=True)[3] == want
    assert E.host_punc_stream_step(m, st, [], flush=True)[3] == -1
    m.close()


def test_a_call_without_words_changes_no_state_byte(model):
    cfg, w, m = model
    st = E.punc_stream_state(m, host=True)
    E.host_punc_stream_step(m, st, R.window_ids(9, 64, 2), flags=NR)
    before = st.copy()
    mk, mf, z, fm = E.host_punc_stream_step(m, st, [], flags=NR)
    assert mk.size == 0 and fm == -1 and np.array_equal(st, before)


def test_argument_errors_change_nothing(model):
    cfg, w, m = model
    st = E.punc_stream_state(m, host=True)
    E.host_punc_stream_step(m, st, R.window_ids(9, 64, 2), flags=NR)
    before = st.copy()
    for kw, ids in ((dict(max_context=1), [1]), (dict(max_context=257), [1]), (dict(flags=2), [1]), (dict(), [64]), (dict(), [-1]),
                    (dict(flags=NR), np.zeros(248, np.int32)), (dict(max_context=9), [1])):
        with pytest.raises(N.PfError) as ei:
            E.host_punc_stream_step(m, st, ids, **kw)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, kw
        assert np.array_equal(st, before)
    E.host_punc_stream_step(m, st, np.zeros(247, np.int32), flags=NR)      # 9 + 247 = 256 fits


# ---- committed words: the host twin (online.cpp online_committed_words) against the definition ----------------------------------
TABLE = ["<blank>", "<s>", "</s>", "<unk>", "hel@@", "lo", "a", "b", "你", "好", "ok", "Wor@@", "ld", "x@@", "c@@", "d", "\u2581w1", "@@"]


def _both(model, toks, before=None):
    """the twin on the token strings `toks` (through TABLE) and the definition; returns the twin's answer after comparing"""
    ids = [TABLE.index(t) for t in toks]
    got = E.host_online_committed_words(model, TABLE, ids, before)
    assert got == S.committed_words(toks), toks
    return got


def test_committed_words(model):
    cfg, w, m = model
    assert _both(m, ["hel@@"]) == ([], "hel") and _both(m, ["hel@@", "lo"]) == (["hello"], None)
    assert _both(m, ["a", "hel@@"]) == (["a"], "hel") and _both(m, ["a", "hel@@", "<blank>"]) == (["a"], "hel")
    assert _both(m, ["你", "好"]) == (["你", "好"], None)
    assert _both(m, ["你", "ok", "好", "Wor@@", "ld"]) == (["你", "ok", "好", "world"], None)
    assert _both(m, []) == ([], None) and _both(m, ["<s>", "<unk>", "<blank>"]) == ([], None)
    assert _both(m, ["你", "</s>", "好", "x@@"]) == (["你"], None)
    assert _both(m, ["a", "b", "你", "c@@", "d"]) == (["a", "b", "你", "cd"], None)
    assert _both(m, ["a", "\u2581w1", "c@@", "\u2581w1", "x@@", "你"])[1] is None
    assert S.online_decode_text(["a", "b", "你", "c@@", "d"]) == "a b你cd"
    rng = np.random.default_rng(3)
    for _ in range(200):                                      # every prefix of a random token string: the committed words only grow
        toks = [TABLE[i] for i in rng.integers(0, len(TABLE) - 1, size=12) if i != 2]
        before = []
        for n in range(len(toks) + 1):
            now, _ = _both(m, toks[:n], before)
            assert S.check_prefix(before, now)
            before = now
    # a violated prefix
    before, _ = _both(m, ["a", "hel@@"])
    assert _both(m, ["a", "hel@@", "lo", "b"], before)[0] == ["a", "hello", "b"]
    assert not S.check_prefix(["a", "hel"], ["a", "hello", "b"])
    for bad, toks in ((["a", "hel"], ["a", "hel@@", "lo", "b"]), (["a", "b"], ["a"]), (["a"], ["a@@"] if "a@@" in TABLE else ["x@@"])):
        with pytest.raises(N.PfError) as ei:
            E.host_online_committed_words(m, TABLE, [TABLE.index(t) for t in toks], bad)
        assert ei.value.code == N.PF_ERR_RECOGNITION, bad
    with pytest.raises(N.PfError):
        E.host_online_committed_words(m, TABLE, [len(TABLE)])


# ---- the container ----------------------------------------------------------------------------------------------------------
def _containers():
    cfg0 = W.ct_transformer_config(vocab=64, n_layers=1)
    w = W.synth_punc_weights(cfg0, seed=42)
    old = W.pack_pfw(cfg0, w)
    with_ = lambda **kw: W.pack_pfw(dict(cfg0, **kw), w)
    good = [("old", old, 0, 5), ("explicit zeros", with_(causal=0, sanm_shift=0), 0, 5), ("causal", with_(causal=1, sanm_shift=5), 1, 10),
            ("causal kernel 3", W.pack_pfw(dict(W.ct_transformer_config(vocab=64, n_layers=1, kernel=3), causal=1, sanm_shift=1),
                                           W.synth_punc_weights(W.ct_transformer_config(vocab=64, n_layers=1, kernel=3), seed=42)), 1, 2)]
    uns = [("causal, centred taps", with_(causal=1)), ("causal, right = 1", with_(causal=1, sanm_shift=4)),
           ("shift without causal", with_(sanm_shift=5)), ("negative shift without causal", with_(sanm_shift=-1))]
    inv = [("causal 2", with_(causal=2, sanm_shift=5)), ("causal -1", with_(causal=-1)), ("shift past the kernel", with_(causal=1, sanm_shift=6)),
           ("shift before the kernel", with_(causal=0, sanm_shift=-6))]
    return cfg0, w, good, uns, inv


def test_container_keys():
    cfg0, w, good, uns, inv = _containers()
    ids = R.window_ids(23, 64, 1)
    for name, blob, causal, left in good:
        m = E.load_punc_model(blob)
        assert m.causal == bool(causal), name
        if name in ("old", "explicit zeros"):              # containers written before the keys existed behave bit for bit as they did
            assert np.abs(E.host_punc_logits(m, ids) - R.logits64(w, cfg0, ids)).max() <= 1e-9
            assert np.array_equal(E.host_punc_logits(m, ids), E.host_punc_logits(E.load_punc_model(good[0][1]), ids))
            for fn in (lambda: E.punc_stream_state(m), lambda: E.punc_stream_state(m, host=True),
                       lambda: E.host_punc_stream_step(m, np.zeros(1 << 20, np.uint8), [1])):
                with pytest.raises(N.PfError) as ei:
                    fn()
                assert ei.value.code == N.PF_ERR_UNSUPPORTED, name
        m.close()
    for name, blob in uns:
        with pytest.raises(N.PfError) as ei:
            E.load_punc_model(blob)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED, name
    for name, blob in inv:
        with pytest.raises(N.PfError) as ei:
            E.load_punc_model(blob)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, name


def test_kernel_3_and_fsmn_edges():
    for kernel, lens in ((3, [1, 2, 3, 4]), (11, [9, 10, 11, 12])):
        cfg, w = _model(1, kernel=kernel)
        m = _load(cfg, w)
        for T in lens:
            ids = R.window_ids(T, 64, T)
            assert np.abs(_host(m, ids, [T], flags=NR)[2] - S.logits64(w, cfg, ids)).max() <= 1e-9
        m.close()


def test_config_accepts_the_two_keys():
    cfg = W.ct_transformer_config(vocab=64, causal=1, sanm_shift=5)
    assert cfg["causal"] == 1 and cfg["sanm_shift"] == 5
    assert "causal" not in W.ct_transformer_config(vocab=64)
    with pytest.raises(KeyError):
        W.ct_transformer_config(lookahead=1)


def test_converter_causal_flag(tmp_path):
    torch = pytest.importorskip("torch")
    from aliparaformerasr_amd import convert as cv
    from ct_transformer_like import CTTransformerLike
    tokens = W.synth_punc_vocab(64)
    sd = CTTransformerLike(vocab=64, n_layers=1).state_dict()
    cfg, w = cv.punc_state_dict_to_pfw(sd, tokens, causal=True)
    assert cfg["causal"] == 1 and cfg["sanm_shift"] == 5
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    assert m.causal
    m.close()
    cfg0, _ = cv.punc_state_dict_to_pfw(sd, tokens)
    assert "causal" not in cfg0
    import json
    torch.save(sd, str(tmp_path / "model.pt"))
    (tmp_path / "tokens.json").write_text(json.dumps(tokens), encoding="utf-8")
    args = [str(tmp_path / "model.pt"), str(tmp_path / "out.pfw"), "--kind", "cttransformer", "--tokens", str(tmp_path / "tokens.json")]
    assert cv.main(args + ["--causal"]) == 0
    assert W.load_pfw(str(tmp_path / "out.pfw"))[0]["causal"] == 1
    (tmp_path / "model.onnx").write_bytes(b"\x08\x07")
    assert cv.main([str(tmp_path / "model.onnx")] + args[1:] + ["--causal"]) == 2


# ---- under sanitizers -------------------------------------------------------------------------------------------------------
def test_loader_and_twin_under_sanitizers(tmp_path):
    """csrc/punc.cpp in a stand-alone program (tests/native/punc_stream_sanitize.cpp) built with AddressSanitizer + UBSan on the
    host code: the containers with the new keys and a 300-word stream in calls of 0, 1, 7 and 64 words: no report, the
    library's own status codes, marks and flags."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "punc_stream_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "punc_stream_sanitize.cpp"),
                        os.path.join(cs, "punc.cpp"), os.path.join(cs, "pfw.cpp"), os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        missing = any(t in b.stderr for t in ("libclang_rt.asan", "libclang_rt.ubsan", "cannot find -lclang_rt", "unsupported option '-fsanitize"))
        assert missing, b.stderr[-3000:]
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    cfg0, w, good, uns, inv = _containers()
    blobs = [x[1] for x in good] + [x for _, x in uns] + [x for _, x in inv]
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
    assert len(lines) == len(blobs)
    assert lines[:2] == ["model 0 stream refused %d" % N.PF_ERR_UNSUPPORTED] * 2
    assert lines[4: 4 + len(uns)] == ["refused %d" % N.PF_ERR_UNSUPPORTED] * len(uns)
    assert lines[4 + len(uns):] == ["refused %d" % N.PF_ERR_INVALID_ARG] * len(inv)
    m = E.load_punc_model(good[2][1])
    ids = np.array([(k * 37 + 11) % 64 for k in range(300)], np.int32)
    mk, mf, _, fm, _ = _host(m, ids, [300], flush=True, max_context=50)
    head, marks, flags = lines[2].split("|")
    assert head.split() == ["ok", "1", "10", str(fm)]
    assert [int(x) for x in marks.split()] == mk.tolist() and [int(x) for x in flags.split()] == mf.tolist()
    m.close()
