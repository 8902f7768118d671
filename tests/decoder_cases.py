"""The decoder-stack case table: the smallest models and inputs that reach every form the decoder walks of
csrc/engine*.cpp select between — shared by tests/test_gpu_launch_census.py and tools/decoder_census.py.

Models (synthetic, seeded):
  P  paraformer, 2 encoder / 3 decoder layers, vocab 300, seed 19, predictor.out.bias -0.2
     (the model of test_gpu_pipeline_kernels.py::test_decoder_middle_in_one_launch)
  S  SeACo paraformer with the timestamp head, the model of tests/test_gpu_seaco.py (seed 21, vocab 120, NO-BIAS 111)
  O  the streaming model and decoder-seam inputs of test_gpu_online.py::test_online_encoder_and_decoder_seams
  V  SenseVoice, 3 encoder + 2 tp layers, vocab 403 (no multiple of 4), seed 9: the model of tests/test_gpu_sensevoice.py.  Its
     "decoder" rows are those of the CTC head, B * (T + 4)
  C  paraformer with cif_variant="cumsum", 2 encoder / 1 decoder layers, vocab 128, seed 23
Audio (W.synth_audio(n, 300 + u)):
  long   18 utterances of [24, 9, 17, 0.25, 30, 13] s x 3: B * L > 512 decoder rows — the persistent / fused forms of the f16
         ASR decoder, live (hi | lo') operand pairs in math_mode 3
  short  (40000, 31000, 36000) samples: B * L <= 129 — the short-input forms
Which side of 512 the decoder row count B * L falls on is a CONDITION of a case (`check_rows`), not something to tune.

Every offline case runs with want_logits=True; `ids_only` cases are also run without."""
import collections
import contextlib
import functools
import os

import numpy as np

ROW_THRESHOLD = 512
HOTWORDS = [[5, 6, 7], [9, 10], list(range(30, 42)), [1]]
LONG_SECONDS = [24, 9, 17, 0.25, 30, 13] * 3
SHORT_SAMPLES = (40000, 31000, 36000)

# every profile class of the engine (prof_begin / gemm / qgemm / cls32_ names in csrc/engine*.cpp)
CLASSES = ("argmax", "attn32_cross", "attn32_self", "attn_cross", "attn_op", "attn_seaco", "attn_self", "cif_misc",
           "ctc_collapse", "dec_mid", "fbank", "fsmn", "gemm32_cif", "gemm32_dec", "gemm32_ffn1", "gemm32_ffn2",
           "gemm32_misc", "gemm32_out", "gemm32_qkv", "gemm32_vocab", "gemm_cif", "gemm_dec_ffn", "gemm_dec_ffn1",
           "gemm_dec_ffn2", "gemm_dec_kv", "gemm_dec_out", "gemm_dec_q", "gemm_ffn1", "gemm_ffn2", "gemm_op", "gemm_out",
           "gemm_outffn", "gemm_qkv", "gemm_seaco", "gemm_ts", "gemm_vocab", "layernorm", "lfr_cmvn_pad", "lstm",
           "pcm_to_samples", "quantize", "seaco_embed", "seaco_merge", "topk", "ts_misc")

Case = collections.namedtuple("Case", "name model audio mode hotwords env ids_only")


def _case(model, audio, mode, hotwords=False, env=None, ids_only=False):
    name = "%s-%s%s-m%d%s" % (model, audio, "-hw" if hotwords else "", mode,
                              "".join("-%s=%s" % kv for kv in sorted((env or {}).items())))
    return Case(name, model, audio, mode, hotwords, env or {}, ids_only)


OFFLINE = (
    _case("P", "long", 0, ids_only=True),                   # 1  split FFN | fused middle | cross-attention, out-projection chain
    _case("P", "short", 0),                                 # 2  short-input forms
    _case("P", "long", 0, env={"PF_DEC_MID": "0"}),         # 3  the fsmn_dec_ln fall-back
    _case("S", "short", 0, hotwords=True),                  # 4  bias decoder behind the short-input ASR decoder
    _case("S", "long", 0, hotwords=True),                   # 5  ... behind the fused one (S's own predictor bias: see check_rows)
    _case("S", "short", 0),                                 # 6  no hot words: the bias branch is skipped
    _case("P", "long", 1), _case("P", "long", 3),           # 7  fp32 graph; mode 3 with live operand pairs
    _case("S", "long", 1, hotwords=True), _case("S", "long", 3, hotwords=True),   # 8
    _case("S", "short", 3, hotwords=True),                  # 9  the two-launch product at or below the threshold
    _case("P", "short", 2), _case("P", "long", 2),          # 10 int8
    _case("S", "short", 2, hotwords=True), _case("S", "long", 2, hotwords=True),
    _case("V", "short", 0), _case("V", "short", 1), _case("V", "short", 2), _case("V", "short", 3),   # 11 the CTC head per arithmetic
    _case("V", "long", 0), _case("V", "long", 2),
    _case("C", "short", 0), _case("C", "short", 1), _case("C", "short", 2),   # 12 the cumsum scan and gather per arithmetic
)
BY_NAME = {c.name: c for c in OFFLINE}


@functools.lru_cache(maxsize=None)
def model(which):
    from aliparaformerasr_amd import weights as W
    if which == "P":
        cfg = W.paraformer_large_config(enc_layers=2, dec_layers=3, vocab=300)
        w = W.synth_weights(cfg, seed=19)
        w["predictor.out.bias"] = np.asarray([-0.2], np.float32)
    elif which == "S":
        cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
        w = W.synth_weights(cfg, 21)
        w["predictor.out.bias"] = np.asarray([0.0], np.float32)
        w["seaco.output.bias"][111] += 2.6
    elif which == "V":
        cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=403)
        w = W.synth_weights(cfg, seed=9)
    elif which == "C":
        cfg = W.paraformer_large_config(enc_layers=2, dec_layers=1, vocab=128, cif_variant="cumsum")
        w = W.synth_weights(cfg, seed=23)
    else:
        assert which == "O", which
        cfg = W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=300)
        w = W.synth_weights(cfg, seed=31)
        w["predictor.out.bias"] = np.asarray([0.8], np.float32)
    return cfg, w, W.pack_pfw(cfg, w), W.synth_cmvn()


@functools.lru_cache(maxsize=None)
def audio(which):
    from aliparaformerasr_amd import weights as W
    lens = [int(16000 * s) for s in LONG_SECONDS] if which == "long" else list(SHORT_SAMPLES)
    return [W.synth_audio(n, 300 + u) for u, n in enumerate(lens)]


def hotwords():
    from oracle import glue
    return np.asarray(glue.pad_list(HOTWORDS), np.int32)


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def engine(case_or_model, mode=0, env=None):
    """A fresh engine for a case (or for model `O`); environment switches are set before it is constructed."""
    from aliparaformerasr_amd.engine import Engine
    if isinstance(case_or_model, Case):
        which, mode, env = case_or_model.model, case_or_model.mode, case_or_model.env
    else:
        which = case_or_model
    cfg, w, blob, cmvn = model(which)
    with _environment(env or {}):
        eng = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    try:
        yield eng
    finally:
        eng.close()


def forward(eng, case, want_logits=True):
    return eng.recognize(audio(case.audio), want_logits=want_logits, hotwords=hotwords() if case.hotwords else None)


def check_rows(case, res):
    """The decoder row count B * L and the assertion that it lies on the case's side of the threshold."""
    rows = len(audio(case.audio)) * int(res.L)
    if case.audio == "long":
        assert rows > ROW_THRESHOLD, (case.name, rows)
    else:
        assert 0 < rows <= ROW_THRESHOLD, (case.name, rows)
    return rows


def launch_census(case):
    """{'rows': B * L, 'launches': {class: count}} of ONE profiled forward on a fresh engine (classes that ran)."""
    with engine(case) as eng:
        eng.profile(True)
        eng.profile_reset()
        res = forward(eng, case)
        counts = {c: int(eng.profile_get(c)[1]) for c in CLASSES}
        eng.profile(False)
    return {"rows": check_rows(case, res), "launches": {c: n for c, n in counts.items() if n}}


def online_inputs():
    """enc, embeds, lens, caches of the decoder seam (case O): B = 3, Tc = 20, L = 4, lens [4, 2, 0], rng seed 3."""
    from oracle import model as om
    from oracle import online as oo
    cfg, w, _, _ = model("O")
    g = oo.OnlineGraphs(om.Oracle(om.ModelConfig(**cfg), w, quant="fp16"))
    rng = np.random.default_rng(3)
    B, Tc, L = 3, 20, 4
    speech = (rng.standard_normal((B, Tc, 560)) * 4).astype(np.float32)
    speech[1, :10] = oo.SENTINEL
    enc, _ = g.encoder(speech)
    emb = rng.standard_normal((B, L, 512)).astype(np.float32)
    lens = np.asarray([4, 2, 0], np.int32)
    for b in range(B):
        emb[b, lens[b]:] = 0
    caches = [rng.standard_normal((B, 512, 10)).astype(np.float32) for _ in range(cfg["dec_layers"])]
    return np.ascontiguousarray(enc, np.float32), emb, lens, caches
