"""Weight container (.pfw) and the seeded synthetic-weight generator.

The reference loads ``model.onnx`` through onnxruntime
(``AliParaformerAsr/OfflineModel.cs:35-70``); this build loads a flat
little-endian container instead:

    bytes 0..3   magic  b"PFW1"
    bytes 4..7   u32    version (1)
    bytes 8..15  u64    header_len
    header_len bytes of UTF-8 JSON:
        {"config": {...ModelConfig...},
         "tensors": [{"name", "dtype": "f32" | "u8", "shape": [...], "offset", "nbytes"}, ...]}
    zero padding to a 256-byte boundary, then tensor data; every ``offset`` is
    relative to the start of the data section and 256-byte aligned.

Linear weights use the [out, in] (= [N, K]) layout, depthwise FSMN kernels
[D, k], the CIF conv [out, in, k].  The native library converts GEMM operands
to its 16-bit MFMA layout at load time; the file always carries float32.
A container made from an int8 export (``model.int8.onnx``, the reference CLI's
default, Program.cs:98-101) additionally carries, per quantised Linear, the
stored bytes ``<linear>.weight_q`` (u8 [N, K]), ``<linear>.weight_zp`` (u8 [N])
and ``<linear>.weight_scale`` (f32 [N]); ``math_mode 2`` multiplies those bytes
as they are, ``<linear>.weight`` beside them is their de-quantised float32 image
(math modes 0 / 1).

Tensor inventory follows SURVEY.md §8a ("Tensor inventory for the
synthetic-weight generator").

A container of kind "fsmnvad" holds a voice-activity model instead of a
recogniser (fsmn_vad_config / vad_tensor_shapes / synth_vad_weights below;
the definition is tests/vadnet_ref.py): it is loaded with
engine.load_vad_model, never handed to an Engine as its weights.  The same
holds for kind "cttransformer", the punctuation model (ct_transformer_config
/ punc_tensor_shapes / synth_punc_weights; tests/punc_ref.py;
engine.load_punc_model): its vocabulary travels as the u8 tensor "vocab".
Kind "campplus" is the speaker-embedding model (campplus_config /
spk_tensor_shapes / synth_spk_weights; tests/spk_ref.py;
engine.load_spk_model).
"""
from __future__ import annotations

import json
import struct

import numpy as np

MAGIC = b"PFW1"
ALIGN = 256

DEFAULT_CONFIG = dict(
    kind="paraformer", feat_dim=560, d_model=512, heads=4, ffn=2048, enc_layers=50,
    tp_layers=0, kernel=11, dec_layers=16, vocab=8404, cif_threshold=1.0, cif_tail=0.45,
    cif_l_order=1, cif_r_order=1, cif_smooth=1.0, cif_noise=0.0, timestamp_head=False,
    seaco=False, use_itn=False,
    # BiCIF timestamp head (CifPredictorV3): ConvTranspose1d x3 upsample -> BiLSTM -> Linear(1024,1)
    cif_smooth2=0.25, cif_noise2=0.01, upsample=3,
    # SeACo (kind "seacoparaformer", seaco=True): hotword embedder Embedding + LSTM(512) x seaco_lstm_layers,
    # bias decoder = SAN-M decoder without input/output layer attending bias_embed, hotword_output_layer
    seaco_layers=4, seaco_ffn=1024, seaco_kernel=21, seaco_lstm_layers=2, seaco_nobias=8377,
    # CIF export variant: "loop" = sequential integrate-and-fire, "cumsum" = FunASR cif_v1_export (prefix sums)
    cif_variant="loop",
    # math_mode 2 on a container WITHOUT stored int8 bytes (the synthetic models): Linear name prefixes that stay float,
    # e.g. ["decoder.output", "seaco.output"] for the MatMuls FunASR's export excludes from quantize_dynamic.  A container
    # converted from an int8 export does not need it: a Linear is quantised iff its `<name>.weight_q` bytes are present.
    int8_exclude=(),
)


def make_config(**kw) -> dict:
    cfg = dict(DEFAULT_CONFIG)
    for k, v in kw.items():
        if k not in cfg:
            raise KeyError(k)
        cfg[k] = v
    cfg["int8_exclude"] = [str(e) for e in cfg["int8_exclude"]]      # a JSON array in the container header
    return cfg


def paraformer_large_config(**kw) -> dict:
    return make_config(**kw)


def seaco_paraformer_config(**kw) -> dict:
    base = dict(kind="seacoparaformer", seaco=True, timestamp_head=True)
    base.update(kw)
    return make_config(**base)


def sensevoice_small_config(**kw) -> dict:
    base = dict(kind="sensevoicesmall", enc_layers=50, tp_layers=20, dec_layers=0, vocab=25055)
    base.update(kw)
    return make_config(**base)


def _linear(rng, out_f, in_f, bias=True, prefix=""):
    d = {prefix + ".weight": (rng.standard_normal((out_f, in_f), dtype=np.float32)
                              / np.float32(np.sqrt(in_f))).astype(np.float32)}
    if bias:
        d[prefix + ".bias"] = (0.1 * rng.standard_normal(out_f, dtype=np.float32)).astype(np.float32)
    return d


def _ln(rng, n, prefix, jitter=True):
    # gamma = 1, beta = 0 per SURVEY §8d; a small seeded jitter keeps gamma/beta
    # handling observable in parity tests (a kernel that ignores beta would
    # otherwise pass).
    g = np.ones(n, np.float32)
    b = np.zeros(n, np.float32)
    if jitter:
        g = (g + 0.05 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        b = (0.05 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    return {prefix + ".weight": g, prefix + ".bias": b}


def _enc_layer(rng, cfg, prefix, d_in):
    D, F, K = cfg["d_model"], cfg["ffn"], cfg["kernel"]
    w = {}
    w.update(_ln(rng, d_in, prefix + ".norm1"))
    w.update(_linear(rng, 3 * D, d_in, prefix=prefix + ".attn.qkv"))
    w[prefix + ".attn.fsmn.weight"] = (0.1 * rng.standard_normal((D, K), dtype=np.float32)).astype(np.float32)
    w.update(_linear(rng, D, D, prefix=prefix + ".attn.out"))
    w.update(_ln(rng, D, prefix + ".norm2"))
    w.update(_linear(rng, F, D, prefix=prefix + ".ffn.w1"))
    w.update(_linear(rng, D, F, prefix=prefix + ".ffn.w2"))
    return w


def synth_weights(cfg: dict, seed: int = 42) -> dict:
    """Seeded synthetic weights: Linear N(0, 1/sqrt(fan_in)), FSMN N(0, 0.1),
    LN gamma~1 beta~0, CIF output bias set so mean(alpha) ~ 0.3 (5 tokens/s)."""
    rng = np.random.default_rng(seed)
    D, F, K, V = cfg["d_model"], cfg["ffn"], cfg["kernel"], cfg["vocab"]
    w = {}
    for i in range(cfg["enc_layers"]):
        w.update(_enc_layer(rng, cfg, f"encoder.layers.{i}", cfg["feat_dim"] if i == 0 else D))
    w.update(_ln(rng, D, "encoder.after_norm"))
    for i in range(cfg["tp_layers"]):
        w.update(_enc_layer(rng, cfg, f"encoder.tp_layers.{i}", D))
    if cfg["tp_layers"]:
        w.update(_ln(rng, D, "encoder.tp_norm"))
    if cfg["kind"] == "sensevoicesmall":
        w.update(_linear(rng, V, D, prefix="ctc"))
        w["embed.weight"] = (0.5 * rng.standard_normal((16, cfg["feat_dim"]), dtype=np.float32)).astype(np.float32)
        return w
    # CIF predictor
    ksz = cfg["cif_l_order"] + cfg["cif_r_order"] + 1
    w["predictor.conv.weight"] = (rng.standard_normal((D, D, ksz), dtype=np.float32)
                                  / np.float32(np.sqrt(D * ksz))).astype(np.float32)
    w["predictor.conv.bias"] = (0.1 * rng.standard_normal(D, dtype=np.float32)).astype(np.float32)
    w["predictor.out.weight"] = (rng.standard_normal((1, D), dtype=np.float32)
                                 / np.float32(np.sqrt(D))).astype(np.float32)
    # calibrated on the seed-42 paraformer-large geometry so that sum(alpha) ~ 150 for 30 s (5 tokens/s)
    w["predictor.out.bias"] = np.asarray([-1.35], np.float32)
    if cfg.get("timestamp_head"):
        up = cfg["upsample"]
        w["predictor.upsample.weight"] = (rng.standard_normal((D, D, up), dtype=np.float32) / np.float32(np.sqrt(D))).astype(np.float32)
        w["predictor.upsample.bias"] = (0.1 * rng.standard_normal(D, dtype=np.float32)).astype(np.float32)
        for sfx in ("", "_reverse"):
            for nm in ("weight_ih", "weight_hh"):
                w["predictor.blstm.%s%s" % (nm, sfx)] = (rng.standard_normal((4 * D, D), dtype=np.float32) / np.float32(np.sqrt(D))).astype(np.float32)
            for nm in ("bias_ih", "bias_hh"):
                w["predictor.blstm.%s%s" % (nm, sfx)] = (0.1 * rng.standard_normal(4 * D, dtype=np.float32)).astype(np.float32)
        w["predictor.out2.weight"] = (rng.standard_normal((1, 2 * D), dtype=np.float32) * np.float32(4.0 / np.sqrt(2 * D))).astype(np.float32)
        w["predictor.out2.bias"] = np.asarray([0.3], np.float32)
    # decoder
    for i in range(cfg["dec_layers"]):
        p = f"decoder.layers.{i}"
        w.update(_ln(rng, D, p + ".norm1"))
        w.update(_linear(rng, F, D, prefix=p + ".ffn.w1"))
        w.update(_ln(rng, F, p + ".ffn.norm"))
        w.update(_linear(rng, D, F, bias=False, prefix=p + ".ffn.w2"))
        w.update(_ln(rng, D, p + ".norm2"))
        w[p + ".fsmn.weight"] = (0.1 * rng.standard_normal((D, K), dtype=np.float32)).astype(np.float32)
        w.update(_ln(rng, D, p + ".norm3"))
        w.update(_linear(rng, D, D, prefix=p + ".src.q"))
        w.update(_linear(rng, 2 * D, D, prefix=p + ".src.kv"))
        w.update(_linear(rng, D, D, prefix=p + ".src.out"))
    p = "decoder.final"
    w.update(_ln(rng, D, p + ".norm1"))
    w.update(_linear(rng, F, D, prefix=p + ".ffn.w1"))
    w.update(_ln(rng, F, p + ".ffn.norm"))
    w.update(_linear(rng, D, F, bias=False, prefix=p + ".ffn.w2"))
    w.update(_ln(rng, D, "decoder.after_norm"))
    w.update(_linear(rng, V, D, prefix="decoder.output"))
    if cfg.get("seaco"):
        Fs, Ks = cfg["seaco_ffn"], cfg["seaco_kernel"]
        w["seaco.embed.weight"] = (0.5 * rng.standard_normal((V, D), dtype=np.float32)).astype(np.float32)
        for l in range(cfg["seaco_lstm_layers"]):
            for nm in ("weight_ih", "weight_hh"):
                w["seaco.lstm.l%d.%s" % (l, nm)] = (rng.standard_normal((4 * D, D), dtype=np.float32) / np.float32(np.sqrt(D))).astype(np.float32)
            for nm in ("bias_ih", "bias_hh"):
                w["seaco.lstm.l%d.%s" % (l, nm)] = (0.1 * rng.standard_normal(4 * D, dtype=np.float32)).astype(np.float32)
        for i in range(cfg["seaco_layers"]):
            p = f"seaco.decoder.layers.{i}"
            w.update(_ln(rng, D, p + ".norm1"))
            w.update(_linear(rng, Fs, D, prefix=p + ".ffn.w1"))
            w.update(_ln(rng, Fs, p + ".ffn.norm"))
            w.update(_linear(rng, D, Fs, bias=False, prefix=p + ".ffn.w2"))
            w.update(_ln(rng, D, p + ".norm2"))
            w[p + ".fsmn.weight"] = (0.1 * rng.standard_normal((D, Ks), dtype=np.float32)).astype(np.float32)
            w.update(_ln(rng, D, p + ".norm3"))
            w.update(_linear(rng, D, D, prefix=p + ".src.q"))
            w.update(_linear(rng, 2 * D, D, prefix=p + ".src.kv"))
            w.update(_linear(rng, D, D, prefix=p + ".src.out"))
        p = "seaco.decoder.final"
        w.update(_ln(rng, D, p + ".norm1"))
        w.update(_linear(rng, Fs, D, prefix=p + ".ffn.w1"))
        w.update(_ln(rng, Fs, p + ".ffn.norm"))
        w.update(_linear(rng, D, Fs, bias=False, prefix=p + ".ffn.w2"))
        w.update(_ln(rng, D, "seaco.decoder.after_norm"))
        w.update(_linear(rng, V, D, prefix="seaco.output"))
    return w


FSMN_VAD_CONFIG = dict(
    kind="fsmnvad", n_mels=80, lfr_m=5, lfr_n=1, input_dim=400, affine_dim=140, linear_dim=250, proj_dim=128, output_dim=248,
    n_layers=4, lorder=20, lstride=1, rorder=0, sil_ids=(0,),
)


def fsmn_vad_config(**kw) -> dict:
    """The config of a `.pfw` of kind "fsmnvad" (the FSMN-VAD model score of the voice-activity segmentation; the definition is
    tests/vadnet_ref.py).  The defaults are the dimensions of FunASR's released model; input_dim follows n_mels * lfr_m unless
    given."""
    cfg = dict(FSMN_VAD_CONFIG)
    for k, v in kw.items():
        if k not in cfg:
            raise KeyError(k)
        cfg[k] = v
    if "input_dim" not in kw:
        cfg["input_dim"] = int(cfg["n_mels"]) * int(cfg["lfr_m"])
    cfg["sil_ids"] = [int(i) for i in cfg["sil_ids"]]
    return cfg


def vad_tensor_shapes(cfg: dict) -> dict:
    """name -> shape of every tensor of an "fsmnvad" container.  Linear weights are [out, in]; the FSMN taps are [lorder, proj]
    (taps[k] weighs the frame (lorder - 1 - k) * lstride back)."""
    I, A, L, P, O = (int(cfg[k]) for k in ("input_dim", "affine_dim", "linear_dim", "proj_dim", "output_dim"))
    sh = {"cmvn.shift": (I,), "cmvn.scale": (I,), "in1.weight": (A, I), "in1.bias": (A,), "in2.weight": (L, A), "in2.bias": (L,)}
    for l in range(int(cfg["n_layers"])):
        sh["fsmn.%d.linear.weight" % l] = (P, L)
        sh["fsmn.%d.taps" % l] = (int(cfg["lorder"]), P)
        sh["fsmn.%d.affine.weight" % l] = (L, P)
        sh["fsmn.%d.affine.bias" % l] = (L,)
    sh.update({"out1.weight": (A, L), "out1.bias": (A,), "out2.weight": (O, A), "out2.bias": (O,)})
    return sh


def synth_vad_weights(cfg: dict, seed: int = 42) -> dict:
    """Seeded synthetic FSMN-VAD weights: Linear N(0, 1 / sqrt(fan_in)), biases N(0, 0.1), taps N(0, 0.1), a CMVN that
    brings fbank-like rows (about N(-4, 3)) near N(0, 1)."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in vad_tensor_shapes(cfg).items():
        if name == "cmvn.shift":
            a = 4.0 + 0.5 * rng.standard_normal(shape)
        elif name == "cmvn.scale":
            a = rng.uniform(0.25, 0.4, shape)
        elif name.endswith(".taps"):
            a = 0.1 * rng.standard_normal(shape)
        elif name.endswith(".bias"):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(shape[1])
        w[name] = a.astype(np.float32)
    return w


CT_TRANSFORMER_CONFIG = dict(
    kind="cttransformer", vocab=272727, d_model=256, heads=8, ffn=1024, kernel=11, n_layers=4,
    punc_list=("<unk>", "_", "，", "。", "？", "、"), sentence_end_id=3,
)


def ct_transformer_config(**kw) -> dict:
    """The config of a `.pfw` of kind "cttransformer" (the punctuation model; the definition is tests/punc_ref.py).  The
    defaults are the dimensions of FunASR's released punc_ct-transformer_zh-cn-common-vocab272727 as remembered, not read from
    a file.  Two optional keys make the streaming form (tests/punc_stream_ref.py): causal (0 / 1) and sanm_shift, the FSMN
    taps moved to the left of the word ((kernel - 1) / 2 for a causal model); a config without them writes the container it
    always wrote."""
    cfg = dict(CT_TRANSFORMER_CONFIG)
    for k, v in kw.items():
        if k not in cfg and k not in ("causal", "sanm_shift"):
            raise KeyError(k)
        cfg[k] = v
    cfg["punc_list"] = [str(s) for s in cfg["punc_list"]]
    cfg["n_punc"] = len(cfg["punc_list"])
    return cfg


def punc_tensor_shapes(cfg: dict) -> dict:
    """name -> shape of every float tensor of a "cttransformer" container (the vocabulary strings travel beside them as the
    u8 tensor "vocab": the UTF-8 words joined by newlines)."""
    D, F, K, P = (int(cfg[k]) for k in ("d_model", "ffn", "kernel", "n_punc"))
    sh = {"embed.weight": (int(cfg["vocab"]), D)}
    for l in range(int(cfg["n_layers"])):
        p = "layers.%d." % l
        sh.update({p + "norm1.weight": (D,), p + "norm1.bias": (D,), p + "attn.qkv.weight": (3 * D, D), p + "attn.qkv.bias": (3 * D,),
                   p + "attn.fsmn.weight": (D, K), p + "attn.out.weight": (D, D), p + "attn.out.bias": (D,),
                   p + "norm2.weight": (D,), p + "norm2.bias": (D,), p + "ffn.w1.weight": (F, D), p + "ffn.w1.bias": (F,),
                   p + "ffn.w2.weight": (D, F), p + "ffn.w2.bias": (D,)})
    sh.update({"after_norm.weight": (D,), "after_norm.bias": (D,), "decoder.weight": (P, D), "decoder.bias": (P,)})
    return sh


def synth_punc_vocab(n: int) -> list:
    """n distinct words: "<unk>" first, then CJK characters from U+4E00, every fifth entry a lower-case ASCII word."""
    out = ["<unk>"]
    for i in range(1, n):
        if i % 5 == 0:
            s, k = "", i // 5
            while True:
                s += chr(ord("a") + k % 26)
                k //= 26
                if k == 0:
                    break
            out.append("w" + s)
        else:
            out.append(chr(0x4E00 + i + (0x800 if 0x4E00 + i >= 0xD800 else 0)))      # (stepping over the surrogate range)
    return out


def synth_punc_weights(cfg: dict, seed: int = 42, decoder_scale: float = 1.0) -> dict:
    """Seeded synthetic CT-Transformer weights: the encoder layers as synth_weights draws them, the embedding N(0, 1 / 16)
    (so that embed * sqrt(d_model) is about N(0, 1)), the decoder N(0, decoder_scale / sqrt(d_model)) and "vocab":
    synth_punc_vocab.  decoder_scale scales the float64 top-2 margin and the f16 error of the logits alike, so it does not
    change the share of positions whose margin clears the error; at 1 that share is above 95 % (tests/test_punc_cpu.py)."""
    rng = np.random.default_rng(seed)
    D = int(cfg["d_model"])
    w = {"embed.weight": (rng.standard_normal((int(cfg["vocab"]), D), dtype=np.float32) / np.float32(16.0)).astype(np.float32)}
    for l in range(int(cfg["n_layers"])):
        w.update(_enc_layer(rng, cfg, "layers.%d" % l, D))
    w.update(_ln(rng, D, "after_norm"))
    dec = _linear(rng, int(cfg["n_punc"]), D, prefix="decoder")
    dec["decoder.weight"] = (dec["decoder.weight"] * np.float32(decoder_scale)).astype(np.float32)
    w.update(dec)
    w["vocab"] = np.frombuffer("\n".join(synth_punc_vocab(int(cfg["vocab"]))).encode("utf-8"), dtype=np.uint8).copy()
    return w


CAMPPLUS_CONFIG = dict(
    kind="campplus", n_mels=80, m_channels=32, init_channels=128, growth=32, bn_channels=128, blocks=(12, 24, 16),
    dilations=(1, 2, 2), seg_len=100, embedding=192,
)


def campplus_config(**kw) -> dict:
    """The config of a `.pfw` of kind "campplus" (the speaker-embedding model; the definition is tests/spk_ref.py).  The
    defaults are the dimensions of 3D-Speaker's released speech_campplus_sv_zh-cn_16k-common as remembered, not read from a
    file."""
    cfg = dict(CAMPPLUS_CONFIG)
    for k, v in kw.items():
        if k not in cfg:
            raise KeyError(k)
        cfg[k] = v
    cfg["blocks"] = [int(n) for n in cfg["blocks"]]
    cfg["dilations"] = [int(d) for d in cfg["dilations"]]
    return cfg


def spk_channel_plan(cfg: dict) -> list:
    """[(channels into block b, channels behind its last layer)] for the three dense blocks; a transit halves the second."""
    C, plan = int(cfg["init_channels"]), []
    for n in cfg["blocks"]:
        plan.append((C, C + int(n) * int(cfg["growth"])))
        C = plan[-1][1] // 2
    return plan


def spk_tensor_shapes(cfg: dict) -> dict:
    """name -> shape of every tensor of a "campplus" container.  Every BatchNorm that can be folded is folded at convert time:
    a convolution or Linear carries the folded scale in its weight and the folded shift as its bias; a BatchNorm that a ReLU
    follows (bn1 of a dense layer, a transit's, the last one) stays as `scale` / `shift`.  Convolutions are [out, in, kf, kt]
    (frequency, time), the TDNN and the dense layers' local convolution [out, in, k], Linear [out, in]."""
    m, I, g, bn, E = (int(cfg[k]) for k in ("m_channels", "init_channels", "growth", "bn_channels", "embedding"))
    sh = {"head.conv1.weight": (m, 1, 3, 3), "head.conv1.bias": (m,)}
    for layer in (1, 2):
        for blk in (0, 1):
            p = "head.layer%d.%d." % (layer, blk)
            sh.update({p + "conv1.weight": (m, m, 3, 3), p + "conv1.bias": (m,), p + "conv2.weight": (m, m, 3, 3), p + "conv2.bias": (m,)})
            if blk == 0:
                sh.update({p + "shortcut.weight": (m, m, 1, 1), p + "shortcut.bias": (m,)})
    sh.update({"head.conv2.weight": (m, m, 3, 3), "head.conv2.bias": (m,)})
    sh.update({"tdnn.weight": (I, m * (int(cfg["n_mels"]) // 8), 5), "tdnn.bias": (I,)})
    for b, ((C0, C1), n) in enumerate(zip(spk_channel_plan(cfg), cfg["blocks"])):
        for l in range(int(n)):
            C, p = C0 + l * g, "block%d.%d." % (b + 1, l)
            sh.update({p + "bn1.scale": (C,), p + "bn1.shift": (C,), p + "linear1.weight": (bn, C), p + "linear1.bias": (bn,),
                       p + "local.weight": (g, bn, 3), p + "cam1.weight": (bn // 2, bn), p + "cam1.bias": (bn // 2,),
                       p + "cam2.weight": (g, bn // 2), p + "cam2.bias": (g,)})
        p = "transit%d." % (b + 1)
        sh.update({p + "bn.scale": (C1,), p + "bn.shift": (C1,), p + "weight": (C1 // 2, C1)})
    C = spk_channel_plan(cfg)[-1][1] // 2
    sh.update({"out_bn.scale": (C,), "out_bn.shift": (C,), "dense.weight": (E, 2 * C), "dense.bias": (E,)})
    return sh


def synth_spk_weights(cfg: dict, seed: int = 42) -> dict:
    """Seeded synthetic CAM++ weights: weights N(0, sqrt(2 / fan_in)) (a ReLU follows nearly every product), biases and shifts
    N(0, 0.1), scales U(0.8, 1.2)."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in spk_tensor_shapes(cfg).items():
        if name.endswith(".scale"):
            a = rng.uniform(0.8, 1.2, shape)
        elif name.endswith((".bias", ".shift")):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) * np.sqrt(2.0 / float(np.prod(shape[1:])))
        w[name] = a.astype(np.float32)
    return w


def synth_cmvn(dim: int = 560, seed: int = 7):
    """CMVN shift ~ N(-8, 1), scale ~ U(0.1, 0.3)."""
    rng = np.random.default_rng(seed)
    shift = (-8.0 + rng.standard_normal(dim)).astype(np.float32)
    scale = rng.uniform(0.1, 0.3, dim).astype(np.float32)
    return shift, scale


def format_mvn_text(shift, scale) -> str:
    """An am.mvn in the kaldi-nnet text layout WavFrontend.LoadCmvn reads (AliParaformerAsr/WavFrontend.cs:113-157):
    <AddShift> / <Rescale> blocks whose <LearnRateCoef> line carries the vector between '[' and ']'."""
    dim = len(shift)

    def vec(v):
        return " ".join(repr(float(np.float32(x))) for x in v)
    return ("<Nnet> \n"
            f"<Splice> {dim} {dim}\n[ 0 ]\n"
            f"<AddShift> {dim} {dim} \n"
            f"<LearnRateCoef> 0 [ {vec(shift)} ]\n"
            f"<Rescale> {dim} {dim}\n"
            f"<LearnRateCoef> 0 [ {vec(scale)} ]\n"
            "</Nnet> \n")


def synth_tokens(vocab: int):
    """A tokens.txt of `vocab` lines in the shape of the real ones: <blank> <s> </s>, CJK characters, BPE pieces with
    '@@' continuations and '▁' word starts (what DecodeMulti's branches act on, OfflineRecognizer.cs:304-418), <unk> last."""
    toks = ["<blank>", "<s>", "</s>"]
    n_cjk = min(max(vocab - 4, 0) * 3 // 4, 0x9FA5 - 0x4E00)
    toks += [chr(0x4E00 + i) for i in range(n_cjk)]
    i = 0
    while len(toks) < vocab - 1:
        w = "w%d" % i
        toks.append(w + "@@" if i % 3 == 0 else ("\u2581" + w if i % 3 == 1 else w))
        i += 1
    toks.append("<unk>")
    return toks[:vocab]


def synth_model_dir(path: str, cfg: dict, weights: dict, cmvn=None, dither: float = 0.0, int8_name: bool = False) -> dict:
    """Writes what `new OfflineRecognizer(modelFilePath, configFilePath, mvnFilePath, tokensFilePath)` takes
    (OfflineRecognizer.cs:23) for a synthetic model: model[.int8].pfw, asr.yaml, am.mvn, tokens.txt.  Returns the paths."""
    import os
    os.makedirs(path, exist_ok=True)
    shift, scale = cmvn if cmvn is not None else synth_cmvn()
    out = {"model": os.path.join(path, "model.int8.pfw" if int8_name else "model.pfw"), "config": os.path.join(path, "asr.yaml"),
           "mvn": os.path.join(path, "am.mvn"), "tokens": os.path.join(path, "tokens.txt")}
    save_pfw(out["model"], cfg, weights)
    kind = cfg.get("kind", "paraformer")
    with open(out["config"], "w") as f:
        f.write("model: %s\nuse_itn: %s\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: %r\n"
                "  lfr_m: 7\n  lfr_n: 6\n  snip_edges: false\n" % (kind, "true" if cfg.get("use_itn") else "false", float(dither)))
    with open(out["mvn"], "w") as f:
        f.write(format_mvn_text(shift, scale))
    with open(out["tokens"], "w", encoding="utf-8") as f:
        f.write("\n".join(synth_tokens(int(cfg["vocab"]))) + "\n")
    return out


def synth_audio(n_samples: int, utt: int, seed: int = 1234) -> np.ndarray:
    """SURVEY §8d synthetic utterance: 0.1*N(0,1) noise + 3 sinusoids 100-4000 Hz,
    float32 in [-1, 1), default_rng(seed + utt)."""
    rng = np.random.default_rng(seed + utt)
    x = 0.1 * rng.standard_normal(n_samples)
    t = np.arange(n_samples) / 16000.0
    for _ in range(3):
        f = rng.uniform(100.0, 4000.0)
        a = rng.uniform(0.05, 0.2)
        ph = rng.uniform(0, 2 * np.pi)
        x = x + a * np.sin(2 * np.pi * f * t + ph)
    return np.clip(x, -0.999, 0.999).astype(np.float32)


def pack_pfw(cfg: dict, weights: dict) -> bytes:
    tensors = []
    off = 0
    chunks = []
    for name, arr in weights.items():
        u8 = isinstance(arr, np.ndarray) and arr.dtype == np.uint8      # `<linear>.weight_q` / `.weight_zp`: stored bytes of an int8 export
        a = np.ascontiguousarray(arr, dtype=np.uint8 if u8 else np.float32)
        nbytes = a.nbytes
        tensors.append({"name": name, "dtype": "u8" if u8 else "f32", "shape": list(a.shape), "offset": off, "nbytes": nbytes})
        chunks.append((off, a))
        off += (nbytes + ALIGN - 1) // ALIGN * ALIGN
    header = json.dumps({"config": cfg, "tensors": tensors}).encode("utf-8")
    pre = 16 + len(header)
    pad = (-pre) % ALIGN
    out = bytearray(pre + pad + off)
    out[0:4] = MAGIC
    struct.pack_into("<IQ", out, 4, 1, len(header))
    out[16:16 + len(header)] = header
    base = pre + pad
    for o, a in chunks:
        out[base + o: base + o + a.nbytes] = a.tobytes()
    return bytes(out)


def save_pfw(path: str, cfg: dict, weights: dict) -> None:
    with open(path, "wb") as f:
        f.write(pack_pfw(cfg, weights))


def load_pfw(path_or_bytes):
    data = path_or_bytes
    if isinstance(path_or_bytes, str):
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    if data[:4] != MAGIC:
        raise ValueError("not a PFW1 container")
    _ver, hlen = struct.unpack_from("<IQ", data, 4)
    hdr = json.loads(data[16:16 + hlen].decode("utf-8"))
    base = (16 + hlen + ALIGN - 1) // ALIGN * ALIGN
    w = {}
    for t in hdr["tensors"]:
        if t.get("dtype", "f32") == "u8":
            a = np.frombuffer(data, dtype=np.uint8, count=t["nbytes"], offset=base + t["offset"])
        else:
            a = np.frombuffer(data, dtype=np.float32, count=t["nbytes"] // 4, offset=base + t["offset"])
        w[t["name"]] = a.reshape(t["shape"]).copy()
    return hdr["config"], w
