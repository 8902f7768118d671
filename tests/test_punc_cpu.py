"""CPU: the punctuation feature off the device — the host twins (pf_host_punc_*) against the definition in numpy float64
(tests/punc_ref.py): the word split, the network, the cut rule at every branch, the text loop window for window, the assembly;
the `.pfw` container of kind "cttransformer" with its loader's refusals; the loader once more under host sanitizers."""
import json
import os
import struct

import numpy as np
import pytest

from pfw_helpers import repack
import punc_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W


def _model(n_layers, seed=5):
    cfg = W.ct_transformer_config(vocab=64, n_layers=n_layers)
    return cfg, W.synth_punc_weights(cfg, seed=seed)


@pytest.fixture(scope="module")
def model():
    cfg, w = _model(2)
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    yield cfg, w, m
    m.close()


def _forward64(cfg, w):
    return lambda win: R.argmax_ties_larger(R.logits64(w, cfg, win))


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_punc_model_load", "pf_punc_model_from_memory", "pf_punc_model_info", "pf_punc_model_free", "pf_host_punc_words",
                 "pf_host_punc_logits", "pf_host_punc_cut", "pf_host_punc_ids", "pf_host_punc_assemble", "pf_host_punc_text",
                 "pf_engine_set_punc_model", "pf_engine_punctuate", "pf_op_punc_logits", "pf_op_punc_window"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    lib.pf_punc_model_free(None)
    assert lib.pf_engine_set_punc_model(None, None) < 0
    assert lib.pf_punc_model_load(None, None) == N.PF_ERR_INVALID_ARG


def test_dimensions_and_ids(model):
    cfg, w, m = model
    for k in ("vocab", "d_model", "heads", "ffn", "kernel", "n_layers", "n_punc", "sentence_end_id"):
        assert m.dims[k] == cfg[k], k
    ix = R.punc_index(cfg["punc_list"])
    assert [m.dims["id_" + k] for k in ("unk", "none", "comma", "period", "question", "pause")] == [ix[k] for k in
                                                                                               ("unk", "none", "comma", "period", "question", "pause")]
    assert m.dims["unk_word"] == R.vocab_of(w).index("<unk>")


# ---- words ---------------------------------------------------------------------------------------------------------------
TEXTS = ["", " ", "\t\n ", "今天天气怎么样我们去公园吧 hello world", "hello", "a b  c\td", "丁丄wb丅", "wb丁wc", "😀", "a😀b 😀😀 c", "xéy",
         "  丁  ", "wb wc wd", "末尾 wb"]


@pytest.mark.parametrize("text", TEXTS)
def test_word_split(model, text):
    cfg, w, m = model
    ids, words = E.host_punc_words(m, text)
    want = R.split_words(text)
    assert words == want
    assert ids.tolist() == R.word_ids(want, R.vocab_of(w)).tolist()


def test_word_split_examples(model):
    cfg, w, m = model
    assert R.split_words("今天 hello world😀a") == ["今", "天", "hello", "world", "😀", "a"]
    assert R.split_words("xéy") == ["x", "é", "y"] and R.split_words(" \t") == []
    vocab = R.vocab_of(w)
    ids, words = E.host_punc_words(m, vocab[7] + vocab[5] + " zzzz " + vocab[10])
    assert ids.tolist() == [7, 5, m.dims["unk_word"], 10]


# ---- the network ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", [1, 2, 4])
def test_host_logits_equal_the_definition(n_layers):
    cfg, w = _model(n_layers)
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    for T in (0, 1, 2, 5, 6, 11, 12, 33, 70):
        ids = R.window_ids(T, cfg["vocab"], T)
        z, want = E.host_punc_logits(m, ids), R.logits64(w, cfg, ids)
        assert z.shape == want.shape == (T, cfg["n_punc"])
        if T:
            assert np.abs(z - want).max() <= 1e-9
    m.close()


def tied_decoder_model(bias):
    """a one-layer model whose decoder has zero weights: every row's logits ARE `bias`, ties included"""
    cfg, w = _model(1)
    w = dict(w)
    w["decoder.weight"] = np.zeros_like(w["decoder.weight"])
    w["decoder.bias"] = np.asarray(bias, np.float32)
    return cfg, w


def test_argmax_ties_go_to_the_larger_index():
    assert R.argmax_ties_larger(np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [5.0, 1.0, 1.0, 1.0]])).tolist() == [2, 3, 0]
    # the host twin's arg-max, through the loop: exactly tied logits
    for bias, want in (([0, 1, 1, 0, 1, 0], 4), ([2, 2, 2, 2, 2, 2], 5), ([1, 1, 0, 0, 0, 0], 1), ([3, 0, 0, 0, 0, 0], 0), ([0, 0, 7, 7, 0, 0], 3)):
        cfg, w = tied_decoder_model(bias)
        m = E.load_punc_model(W.pack_pfw(cfg, w))
        ids = R.window_ids(7, 64, 1)
        z = E.host_punc_logits(m, ids)
        assert (z == np.asarray(bias, np.float64)[None]).all()
        assert R.argmax_ties_larger(z).tolist() == [want] * 7
        got, wins = E.host_punc_ids(m, ids)                  # one window, the last: only its final mark may be edited
        assert got[:-1].tolist() == [want] * 6 and wins == [(7, 6)]
        assert got[-1] == R.cut_rule([want] * 7, True, cfg["punc_list"], cfg["sentence_end_id"])[1][-1]
        m.close()


@pytest.mark.parametrize("n_layers", [1, 2, 4])
def test_reference_margin_meets_the_cap(n_layers):
    """What the GPU test relies on: over its windows, at most 5 % of the positions have a float64 top-2 margin within twice the
    allowed logit deviation (allowed = 4 x the f16 emulation's deviation from float64)."""
    cfg, w = _model(n_layers)
    dev, margins, _ = R.deviation_and_margin(w, cfg)
    assert 0 < dev < 0.05
    assert float((margins <= 2 * 4 * dev).mean()) <= 0.05


# ---- the cut rule --------------------------------------------------------------------------------------------------------
NONE, COMMA, PERIOD, QUESTION, PAUSE = 1, 2, 3, 4, 5


def _both_cut(model, p, last):
    cfg, w, m = model
    cut, q = E.host_punc_cut(m, p, last)
    rc, rq = R.cut_rule(p, last, cfg["punc_list"], cfg["sentence_end_id"])
    assert cut == rc and q.tolist() == rq.tolist()
    return cut, q


def _p(n, **at):
    p = np.full(n, NONE, np.int32)
    for k, v in at.items():
        p[int(k[1:]) if not k.startswith("m") else n - int(k[1:])] = v       # i5 = index 5, m2 = index n - 2
    return p


def test_cut_found_at_the_edges_only_inside_2_to_n_minus_2(model):
    n = 30
    assert _both_cut(model, _p(n, i2=PERIOD), False)[0] == 2
    assert _both_cut(model, _p(n, m2=QUESTION), False)[0] == n - 2
    assert _both_cut(model, _p(n, i2=PERIOD, m2=PERIOD, i9=QUESTION), False)[0] == n - 2
    assert _both_cut(model, _p(n, i1=PERIOD), False)[0] == -1
    assert _both_cut(model, _p(n, m1=PERIOD), False)[0] == -1
    assert _both_cut(model, _p(n, i0=QUESTION, i1=PERIOD, m1=PERIOD, i7=COMMA, i8=PAUSE), False)[0] == -1
    for n in (0, 1, 2, 3, 4, 5):
        for mark in (PERIOD, COMMA, NONE):
            _both_cut(model, np.full(n, mark, np.int32), False)
            _both_cut(model, np.full(n, mark, np.int32), True)
    assert _both_cut(model, np.full(5, PERIOD, np.int32), False)[0] == 3 and _both_cut(model, np.full(4, PERIOD, np.int32), False)[0] == 2
    assert _both_cut(model, np.full(3, PERIOD, np.int32), False)[0] == -1


def test_comma_fallback_at_200_and_201(model):
    cut, q = _both_cut(model, _p(200, i50=COMMA, i120=COMMA), False)
    assert cut == -1 and q[120] == COMMA
    cut, q = _both_cut(model, _p(201, i50=COMMA, i120=COMMA), False)
    assert cut == 120 and q[120] == PERIOD and q[50] == COMMA
    cut, q = _both_cut(model, _p(201, i1=COMMA, m1=COMMA, i60=PAUSE), False)               # commas outside the range, a pause inside
    assert cut == -1
    cut, q = _both_cut(model, _p(300, i50=QUESTION, i120=COMMA), False)                    # a full stop below a comma wins
    assert cut == 50 and q[120] == COMMA


def test_hard_cut_at_492_and_493(model):
    assert _both_cut(model, _p(492), False)[0] == -1
    cut, q = _both_cut(model, _p(493), False)
    assert cut == 492 and (q == NONE).all()
    assert _both_cut(model, _p(512, i1=PERIOD), False)[0] == 511
    assert _both_cut(model, _p(512, i300=COMMA), False)[0] == 300
    # a cut that would leave more than 492 words behind it is overruled: the next window would pass 512
    for n, at, want in ((512, 19, 19), (512, 18, 511), (500, 7, 7), (500, 6, 499), (493, 2, 2), (496, 2, 495), (495, 2, 2), (495, 1, 494)):
        cut, q = _both_cut(model, _p(n, **{"i%d" % at: COMMA}), False)
        assert cut == want and q[at] == (PERIOD if want == at else COMMA), (n, at)
        assert _both_cut(model, _p(n, **{"i%d" % at: QUESTION}), False)[0] == want

def test_last_window_edits(model):
    for mark, want in ((COMMA, PERIOD), (PAUSE, PERIOD), (NONE, PERIOD), (PERIOD, PERIOD), (QUESTION, QUESTION), (0, 0)):
        cut, q = _both_cut(model, _p(7, m1=mark, i3=COMMA), True)
        assert cut == 6 and q[6] == want and q[3] == COMMA
    assert _both_cut(model, np.zeros(0, np.int32), True)[0] == -1


def test_cut_rule_on_random_marks(model):
    rng = np.random.default_rng(3)
    for n in (3, 17, 64, 199, 200, 201, 260, 492, 493, 512):
        for dense in (0.0, 0.02, 0.3):
            p = np.where(rng.random(n) < dense, rng.integers(0, 6, n), NONE).astype(np.int32)
            _both_cut(model, p, False)
            _both_cut(model, p, True)


# ---- the text loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 19, 20, 21, 40, 45, 230])
def test_loop_equals_the_reference_loop_window_for_window(model, n):
    cfg, w, m = model
    ids = R.window_ids(n, cfg["vocab"], 77 + n)
    got, wins = E.host_punc_ids(m, ids)
    want, log = R.text_loop(ids, _forward64(cfg, w), cfg["punc_list"], cfg["sentence_end_id"])
    assert wins == [(len(win), cut) for win, _, cut in log]
    assert len(wins) == (n + 19) // 20
    assert got.tolist() == want.tolist() and len(got) == n


def test_loop_carries_a_long_tail_in_the_definition():
    """The branches a random network rarely reaches, with a forward that never ends a sentence: the window grows by 20 until
    the comma rule (above 200) or the hard cut (above 492) fires, and never passes 512."""
    pl, se = W.CT_TRANSFORMER_CONFIG["punc_list"], 3
    ids = np.arange(1300, dtype=np.int32)
    out, log = R.text_loop(ids, lambda win: np.full(len(win), NONE, np.int32), list(pl), se)
    assert max(len(win) for win, _, _ in log) == 500 and len(out) == 1300
    assert [cut for win, _, cut in log if cut >= 0 and len(win) == 500] == [499, 499]
    out, log = R.text_loop(ids, lambda win: np.where(np.arange(len(win)) == 7, COMMA, NONE).astype(np.int32), list(pl), se)
    assert max(len(win) for win, _, _ in log) == 508 and len(out) == 1300 and (out == PERIOD).sum() >= 5
    assert log[10][2] == 7 and len(log[10][0]) == 220 and len(log[11][0]) == 232            # the tail grows by 12 a round ...
    assert [(len(win), cut) for win, _, cut in log if len(win) >= 496][:2] == [(496, 7), (508, 507)]      # ... until the hard cut ends it


def test_text_and_sentences(model):
    cfg, w, m = model
    vocab = R.vocab_of(w)
    text = "".join(vocab[1:4]) + " wb  hello" + "".join(vocab[6:9]) + " x 😀" + vocab[11] * 25
    fwd = _forward64(cfg, w)
    want_text, want_sent, want_p = R.punctuate(text, vocab, fwd, cfg["punc_list"], cfg["sentence_end_id"])
    got_text, got_p = E.host_punc_text(m, text)
    assert got_p.tolist() == want_p.tolist() and got_text == want_text
    a_text, a_sent = E.host_punc_assemble(m, text, got_p)
    assert a_text == want_text and a_sent == want_sent and a_sent[-1] == len(got_p)
    assert E.host_punc_text(m, "")[0] == "" and E.host_punc_text(m, "  ")[1].size == 0


def test_assembly_rules(model):
    cfg, w, m = model
    text = "丁 wb wc丄 wd"
    words = R.split_words(text)
    assert words == ["丁", "wb", "wc", "丄", "wd"]
    for p in ([COMMA, COMMA, PERIOD, QUESTION, PAUSE], [NONE, 0, QUESTION, PAUSE, PERIOD], [PERIOD, PAUSE, NONE, NONE, QUESTION]):
        got, sent = E.host_punc_assemble(m, text, p)
        want, wsent = R.assemble(words, p, cfg["punc_list"])
        assert got == want and sent == wsent
    assert R.assemble(words, [COMMA, COMMA, PERIOD, QUESTION, PAUSE], cfg["punc_list"]) == ("丁，wb, wc.丄？wd,", [3, 4, 5])
    assert R.assemble(words, [NONE, 0, NONE, NONE, NONE], cfg["punc_list"]) == ("丁wb wc丄wd", [5])


# ---- the container -------------------------------------------------------------------------------------------------------
def _refusals():
    cfg, w = _model(1)
    good = W.pack_pfw(cfg, w)

    def far(h): h["tensors"][3]["offset"] = 1 << 40
    def big(h): h["tensors"][-1]["nbytes"] = h["tensors"][-1]["nbytes"] + 4096
    def with_(**kw): return W.pack_pfw(dict(cfg, **kw), w)
    def tensor(name, fn):
        w2 = {k: v.copy() for k, v in w.items()}
        w2[name] = fn(w2[name])
        return W.pack_pfw(cfg, w2)
    def nan(a): a.reshape(-1)[3] = np.nan; return a
    def inf(a): a.reshape(-1)[0] = np.inf; return a
    vocab = R.vocab_of(w)
    enc = lambda words: np.frombuffer("\n".join(words).encode("utf-8"), dtype=np.uint8).copy()
    inv = [("short", good[:40]), ("cut tail", good[: len(good) - 237]), ("half", good[: len(good) // 2]), ("empty", b""),
           ("offset", repack(cfg, w, far)), ("nbytes", repack(cfg, w, big)),
           ("header length", good[:8] + struct.pack("<Q", (1 << 64) - 8) + good[16:]), ("magic", b"XXXX" + good[4:]),
           ("kind", with_(kind="fsmnvad")), ("nan", tensor("decoder.bias", nan)), ("inf", tensor("embed.weight", inf)),
           ("shape", tensor("layers.0.attn.fsmn.weight", lambda a: a[:, :9].copy())),
           ("missing", W.pack_pfw(cfg, {k: v for k, v in w.items() if k != "after_norm.bias"})),
           ("no vocab", W.pack_pfw(cfg, {k: v for k, v in w.items() if k != "vocab"})),
           ("vocab count", tensor("vocab", lambda a: enc(vocab[:-1]))), ("vocab twice", tensor("vocab", lambda a: enc(vocab[:-1] + [vocab[3]]))),
           ("vocab unk", tensor("vocab", lambda a: enc(["<UNK>"] + vocab[1:]))), ("vocab empty word", tensor("vocab", lambda a: enc(vocab[:-1] + [""]))),
           ("no unk mark", with_(punc_list=["<x>", "_", "，", "。", "？", "、"])), ("no underscore", with_(punc_list=["<unk>", "-", "，", "。", "？", "、"])),
           ("mark twice", with_(punc_list=["<unk>", "_", "，", "。", "。", "、"])), ("sentence end", with_(sentence_end_id=6)),
           ("sentence end negative", with_(sentence_end_id=-1)), ("no layers", with_(n_layers=0))]
    uns = [("d_model", with_(d_model=128)), ("heads", with_(heads=4)), ("ffn", with_(ffn=1000)), ("ffn large", with_(ffn=8192)),
           ("even kernel", with_(kernel=10)), ("kernel", with_(kernel=33)), ("layers", with_(n_layers=9)), ("one class", with_(punc_list=["<unk>"])),
           ("classes", with_(punc_list=["<unk>", "_"] + ["m%d" % i for i in range(31)]))]
    return good, inv, uns


def test_container_refusals():
    good, inv, uns = _refusals()
    E.load_punc_model(good).close()
    for name, blob in inv:
        with pytest.raises(N.PfError) as ei:
            E.load_punc_model(blob if blob else b"\0")
        assert ei.value.code == N.PF_ERR_INVALID_ARG, name
    for name, blob in uns:
        with pytest.raises(N.PfError) as ei:
            E.load_punc_model(blob)
        assert ei.value.code == N.PF_ERR_UNSUPPORTED, name


def test_supported_variants_load():
    for kw in (dict(kernel=31, n_layers=1), dict(kernel=1, n_layers=1, ffn=256), dict(n_layers=1, punc_list=["_", "<unk>"], sentence_end_id=0),
               dict(n_layers=1, ffn=2048, punc_list=["<unk>", "_"] + ["m%d" % i for i in range(30)])):
        cfg = W.ct_transformer_config(vocab=16, **kw)
        w = W.synth_punc_weights(cfg, seed=1)
        m = E.load_punc_model(W.pack_pfw(cfg, w))
        ids = R.window_ids(23, 16, 1)
        assert np.abs(E.host_punc_logits(m, ids) - R.logits64(w, cfg, ids)).max() <= 1e-9
        p = R.argmax_ties_larger(R.logits64(w, cfg, ids))
        for last in (False, True):
            cut, q = E.host_punc_cut(m, p, last)
            rc, rq = R.cut_rule(p, last, cfg["punc_list"], cfg["sentence_end_id"])
            assert cut == rc and q.tolist() == rq.tolist()
        m.close()


def test_loader_under_sanitizers(tmp_path):
    """csrc/punc.cpp in a stand-alone program (tests/native/punc_sanitize.cpp) built with AddressSanitizer + UBSan on the host
    code, over a good container and the malformed ones: no report, the library's own status codes, text and ids."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "punc_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "punc_sanitize.cpp"),
                        os.path.join(cs, "punc.cpp"), os.path.join(cs, "pfw.cpp"), os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"),
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
    assert len(lines) == len(blobs)
    assert lines[1: 1 + len(inv)] == ["refused %d" % N.PF_ERR_INVALID_ARG] * len(inv)
    assert lines[1 + len(inv):] == ["refused %d" % N.PF_ERR_UNSUPPORTED] * len(uns)
    # the good one: the same text and ids as the library loaded into this process gives
    cfg, w = _model(1)
    m = E.load_punc_model(good)
    text = "丁七 wb 丈三  hello 😀上下 wc wd\t丁"
    ids, _ = E.host_punc_words(m, text)
    p4, wins = E.host_punc_ids(m, np.tile(ids, 4))
    head, out, tail = lines[0].split("|")
    assert head.split()[:4] == ["ok", str(cfg["vocab"]), str(cfg["n_punc"]), "1"] and int(head.split()[5]) == len(wins) == 3
    assert [int(x) for x in tail.split()] == p4.tolist()
    assert out == E.host_punc_assemble(m, text, p4[: len(ids)])[0]
    m.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_punc_option():
    from aliparaformerasr_amd.examples import parse_args
    base = ["-type", "offline", "-files", "a.wav"]
    assert parse_args(base + ["-punc", "punc.pfw"])["punc"] == "punc.pfw"
    cfg = parse_args(["-punc", "p.pfw", "-vad"] + base)
    assert cfg["punc"] == "p.pfw" and "vad" in cfg
    assert "punc" not in parse_args(base)
    for bad in (["-punc"], ["-punc", "-files"]):
        with pytest.raises(ValueError, match="-punc takes"):
            parse_args(["-type", "offline"] + bad)
    with pytest.raises(ValueError, match="-punc is an offline option"):
        parse_args(["-type", "online", "-files", "a.wav", "-punc", "p.pfw"])


def test_punc_lines():
    from aliparaformerasr_amd.examples import _punc_lines
    from aliparaformerasr_amd.offline_recognizer import Sentence

    class St:
        Punctuated = "丁，wb."
        Sentences = [Sentence(0, 2, [10, 250], "丁，wb."), Sentence(2, 3, [], "丄")]
    assert _punc_lines(St()) == ["punctuated: 丁，wb.", "  [10-250 ms] 丁，wb.", "  丄"]


# ---- the converter (state-dict route) --------------------------------------------------------------------------------------------
def test_converter_state_dict_route(tmp_path):
    import torch
    from aliparaformerasr_amd import convert as cv
    from ct_transformer_like import CTTransformerLike
    net = CTTransformerLike(vocab=64, n_layers=3, seed=4)
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    tokens = W.synth_punc_vocab(64)
    cfg, w = cv.punc_state_dict_to_pfw(sd, tokens)
    assert (cfg["vocab"], cfg["d_model"], cfg["ffn"], cfg["kernel"], cfg["n_layers"], cfg["n_punc"], cfg["sentence_end_id"]) == (64, 256, 1024, 11, 3, 6, 3)
    assert np.array_equal(w["layers.0.attn.qkv.weight"], sd["encoder.encoders0.0.self_attn.linear_q_k_v.weight"])
    assert np.array_equal(w["layers.2.ffn.w2.bias"], sd["encoder.encoders.1.feed_forward.w_2.bias"])
    assert np.array_equal(w["layers.1.attn.fsmn.weight"], sd["encoder.encoders.0.self_attn.fsmn_block.weight"][:, 0, :])
    m = E.load_punc_model(W.pack_pfw(cfg, w))
    ids = R.window_ids(41, 64, 2)
    assert np.abs(E.host_punc_logits(m, ids) - R.logits64(w, cfg, ids)).max() <= 1e-9
    m.close()
    # through the command line, tokens as JSON and as lines
    torch.save(net.state_dict(), str(tmp_path / "model.pt"))
    (tmp_path / "tokens.json").write_text(json.dumps(tokens), encoding="utf-8")
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n", encoding="utf-8")
    for tk in ("tokens.json", "tokens.txt"):
        assert cv.main([str(tmp_path / "model.pt"), str(tmp_path / "out.pfw"), "--kind", "cttransformer", "--tokens", str(tmp_path / tk)]) == 0
        cfg2, w2 = W.load_pfw(str(tmp_path / "out.pfw"))
        assert cfg2 == json.loads(json.dumps(cfg)) and all(np.array_equal(w2[k], w[k]) for k in w)
    assert cv.main([str(tmp_path / "model.pt"), str(tmp_path / "out.pfw"), "--kind", "cttransformer"]) == 2
    for drop in ("decoder.bias", "encoder.encoders.1.norm2.weight", "embed.weight"):
        with pytest.raises(ValueError):
            cv.punc_state_dict_to_pfw({k: v for k, v in sd.items() if k != drop}, tokens)
    with pytest.raises(ValueError):
        cv.punc_state_dict_to_pfw(sd, tokens[:-1])


@pytest.mark.parametrize("opset,n_layers", [(17, 2), (13, 2), (17, 4)])
def test_converter_onnx_route(tmp_path, opset, n_layers):
    """an export of tests/ct_transformer_like.py -> convert's main -> load_punc_model: every tensor comes back as the state-dict
    route gives it; the torch module itself agrees with the definition; a graph of another shape is refused"""
    torch = pytest.importorskip("torch")
    import ct_transformer_like as L
    from aliparaformerasr_amd import convert as cv
    from aliparaformerasr_amd import onnx_reader as OR
    net = L.CTTransformerLike(vocab=64, n_layers=n_layers, seed=9)
    tokens = W.synth_punc_vocab(64)
    cfg, w = cv.punc_state_dict_to_pfw({k: v.detach().numpy() for k, v in net.state_dict().items()}, tokens)
    ids = R.window_ids(37, 64, 3)
    assert float(np.abs(L.logits(net, ids) - R.logits64(w, cfg, ids)).max()) < 2e-4          # float32 torch against float64
    blob = L.export(net, opset=opset)
    g = OR.load(blob)
    assert g.inputs[0] == "text"
    assert not any(k.endswith(("linear_q_k_v.weight", "w_1.weight", "decoder.weight")) for k in g.initializers)   # anonymised by the exporter
    assert any(n.op_type == "LayerNormalization" for n in g.nodes) == (opset >= 17)
    (tmp_path / "model.onnx").write_bytes(blob)
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n", encoding="utf-8")
    assert cv.main([str(tmp_path / "model.onnx"), str(tmp_path / "out.pfw"), "--kind", "cttransformer", "--tokens", str(tmp_path / "tokens.txt")]) == 0
    cfg2, w2 = W.load_pfw(str(tmp_path / "out.pfw"))
    assert cfg2 == json.loads(json.dumps(cfg)) and set(w2) == set(w)
    for k in w:
        assert np.array_equal(w2[k], w[k]), k
    m = E.load_punc_model(str(tmp_path / "out.pfw"))
    assert np.abs(E.host_punc_logits(m, ids) - R.logits64(w, cfg, ids)).max() <= 1e-9
    m.close()
    # graphs of another shape
    import fsmn_vad_like as VL
    import vadnet_ref as VR
    vcfg, vw = VR.small_model()
    vmod = VL.FsmnVadLike(vcfg)
    VL.load_pfw_weights(vmod, vcfg, vw)
    with pytest.raises(ValueError, match="cttransformer"):
        cv.punc_onnx_to_state_dict(OR.load(VL.export(vmod, opset=opset)))

    class TwoHeads(torch.nn.Module):                       # a CT-Transformer with a second Linear behind the decoder
        def __init__(self):
            super().__init__()
            self.inner, self.extra = net, torch.nn.Linear(6, 6)

        def forward(self, text):
            return self.extra(self.inner(text))
    from funasr_like import export_onnx
    with pytest.raises(ValueError, match="cttransformer"):
        cv.punc_onnx_to_state_dict(OR.load(export_onnx(TwoHeads(), (torch.zeros(1, 9, dtype=torch.long),), ["text"], ["logits"], None, opset)))
