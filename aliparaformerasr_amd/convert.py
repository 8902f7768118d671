"""FunASR PyTorch checkpoint (state_dict) -> PFW1 container.

The reference consumes ONNX exports of FunASR models (README.EN.md:233); every export is produced from a FunASR
PyTorch checkpoint (`model.pt`) whose parameter names are fixed by the public FunASR module definitions
(SANMEncoder / CifPredictorV2|V3 / ParaformerSANMDecoder / SeacoParaformer / SenseVoiceSmall).  This module maps
those names onto the PFW tensor inventory of `aliparaformerasr_amd/weights.py`.  It is a NAME/LAYOUT mapping only
(no arithmetic); ONNX graph-walk ingestion incl. the int8 variants stays a "next" item.

NOT VALIDATED AGAINST A REAL CHECKPOINT: no FunASR file exists in the build image; the table below is restated
from the public FunASR sources and exercised by a round-trip test on synthetic tensors (tests/test_weights.py).
Every tensor is shape-checked against the target geometry, and unknown / missing names are reported, so a
mismatch with a real file fails loudly instead of producing a silently wrong model.

    python -m aliparaformerasr_amd.convert model.pt out.pfw [--kind paraformer|seacoparaformer|sensevoicesmall]
                                                           [--timestamp]
    python -m aliparaformerasr_amd.convert model.int8.onnx out.pfw [--eb model_eb.int8.onnx] [--kind ...]
        (ONNX graph walk, see onnx_to_state_dict; an int8 file's stored bytes are carried beside their float image)
    python -m aliparaformerasr_amd.convert vad.onnx|vad.pt out.pfw --kind fsmnvad --mvn vad.mvn [--sil 0,...] [--lfr-m 5]
    python -m aliparaformerasr_amd.convert punc.pt|punc.onnx out.pfw --kind cttransformer --tokens tokens.json [--heads 8] [--causal]
    python -m aliparaformerasr_amd.convert campplus.bin|.pt out.pfw --kind campplus [--seg-len 100] [--dilations 1,2,2]
        (FunASR's FSMN-VAD, the model score of the voice-activity segmentation: vad_state_dict_to_pfw / vad_onnx_to_state_dict.
         NO REAL FSMN-VAD FILE HAS BEEN THROUGH THIS ROUTE: the names are restated from the public FunASR sources and
         exercised on tests/fsmn_vad_like.py)
"""
from __future__ import annotations

import re
import sys

import numpy as np

from . import weights as W

_ENC = {  # PFW suffix -> FunASR suffix inside an encoder block
    "norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias",
    "attn.qkv.weight": "self_attn.linear_q_k_v.weight", "attn.qkv.bias": "self_attn.linear_q_k_v.bias",
    "attn.fsmn.weight": "self_attn.fsmn_block.weight",
    "attn.out.weight": "self_attn.linear_out.weight", "attn.out.bias": "self_attn.linear_out.bias",
    "ffn.w1.weight": "feed_forward.w_1.weight", "ffn.w1.bias": "feed_forward.w_1.bias",
    "ffn.w2.weight": "feed_forward.w_2.weight", "ffn.w2.bias": "feed_forward.w_2.bias",
}
_DEC = {
    "norm1.weight": "norm1.weight", "norm1.bias": "norm1.bias", "norm2.weight": "norm2.weight", "norm2.bias": "norm2.bias",
    "norm3.weight": "norm3.weight", "norm3.bias": "norm3.bias",
    "ffn.w1.weight": "feed_forward.w_1.weight", "ffn.w1.bias": "feed_forward.w_1.bias",
    "ffn.norm.weight": "feed_forward.norm.weight", "ffn.norm.bias": "feed_forward.norm.bias",
    "ffn.w2.weight": "feed_forward.w_2.weight",
    "fsmn.weight": "self_attn.fsmn_block.weight",
    "src.q.weight": "src_attn.linear_q.weight", "src.q.bias": "src_attn.linear_q.bias",
    "src.kv.weight": "src_attn.linear_k_v.weight", "src.kv.bias": "src_attn.linear_k_v.bias",
    "src.out.weight": "src_attn.linear_out.weight", "src.out.bias": "src_attn.linear_out.bias",
}
_DEC_FINAL = {k: v for k, v in _DEC.items() if k.startswith(("norm1", "ffn"))}


def name_map(cfg: dict) -> dict:
    """PFW tensor name -> FunASR state_dict key, for the geometry in cfg."""
    m = {}
    for i in range(cfg["enc_layers"]):
        src = "encoder.encoders0.0" if i == 0 else "encoder.encoders.%d" % (i - 1)
        for a, b in _ENC.items():
            m["encoder.layers.%d.%s" % (i, a)] = "%s.%s" % (src, b)
    m["encoder.after_norm.weight"], m["encoder.after_norm.bias"] = "encoder.after_norm.weight", "encoder.after_norm.bias"
    for i in range(cfg["tp_layers"]):
        for a, b in _ENC.items():
            m["encoder.tp_layers.%d.%s" % (i, a)] = "encoder.tp_encoders.%d.%s" % (i, b)
    if cfg["tp_layers"]:
        m["encoder.tp_norm.weight"], m["encoder.tp_norm.bias"] = "encoder.tp_norm.weight", "encoder.tp_norm.bias"
    if cfg["kind"] == "sensevoicesmall":
        m["ctc.weight"], m["ctc.bias"] = "ctc.ctc_lo.weight", "ctc.ctc_lo.bias"
        m["embed.weight"] = "embed.weight"
        return m
    m["predictor.conv.weight"], m["predictor.conv.bias"] = "predictor.cif_conv1d.weight", "predictor.cif_conv1d.bias"
    m["predictor.out.weight"], m["predictor.out.bias"] = "predictor.cif_output.weight", "predictor.cif_output.bias"
    if cfg.get("timestamp_head"):
        m["predictor.upsample.weight"], m["predictor.upsample.bias"] = "predictor.upsample_cnn.weight", "predictor.upsample_cnn.bias"
        for sfx in ("", "_reverse"):
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                m["predictor.blstm.%s%s" % (nm, sfx)] = "predictor.blstm.%s_l0%s" % (nm, sfx)
        m["predictor.out2.weight"], m["predictor.out2.bias"] = "predictor.cif_output2.weight", "predictor.cif_output2.bias"
    for i in range(cfg["dec_layers"]):
        for a, b in _DEC.items():
            m["decoder.layers.%d.%s" % (i, a)] = "decoder.decoders.%d.%s" % (i, b)
    for a, b in _DEC_FINAL.items():
        m["decoder.final.%s" % a] = "decoder.decoders3.0.%s" % b
    m["decoder.after_norm.weight"], m["decoder.after_norm.bias"] = "decoder.after_norm.weight", "decoder.after_norm.bias"
    m["decoder.output.weight"], m["decoder.output.bias"] = "decoder.output_layer.weight", "decoder.output_layer.bias"
    if cfg.get("seaco"):
        m["seaco.embed.weight"] = "bias_embed.weight"
        for l in range(cfg["seaco_lstm_layers"]):
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                m["seaco.lstm.l%d.%s" % (l, nm)] = "bias_encoder.%s_l%d" % (nm, l)
        for i in range(cfg["seaco_layers"]):
            for a, b in _DEC.items():
                m["seaco.decoder.layers.%d.%s" % (i, a)] = "seaco_decoder.decoders.%d.%s" % (i, b)
        for a, b in _DEC_FINAL.items():
            m["seaco.decoder.final.%s" % a] = "seaco_decoder.decoders3.0.%s" % b
        m["seaco.decoder.after_norm.weight"] = "seaco_decoder.after_norm.weight"
        m["seaco.decoder.after_norm.bias"] = "seaco_decoder.after_norm.bias"
        m["seaco.output.weight"], m["seaco.output.bias"] = "hotword_output_layer.weight", "hotword_output_layer.bias"
    return m


def _layout(pfw_name: str, a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, np.float32)
    if pfw_name.endswith("fsmn.weight") and a.ndim == 3:            # depthwise Conv1d [D,1,k] -> [D,k]
        a = a[:, 0, :]
    return np.ascontiguousarray(a)


def infer_config(sd: dict, kind: str = "paraformer", timestamp: bool | None = None) -> dict:
    """Geometry from the checkpoint itself (layer counts, vocabulary, kernel sizes)."""
    def count(pat):
        ids = {int(m.group(1)) for k in sd for m in [re.match(pat, k)] if m}
        return max(ids) + 1 if ids else 0
    kw = dict(kind=kind, enc_layers=1 + count(r"encoder\.encoders\.(\d+)\."), tp_layers=count(r"encoder\.tp_encoders\.(\d+)\."))
    kw["kernel"] = int(np.asarray(sd["encoder.encoders0.0.self_attn.fsmn_block.weight"]).shape[-1])
    kw["ffn"] = int(np.asarray(sd["encoder.encoders0.0.feed_forward.w_1.weight"]).shape[0])
    kw["feat_dim"] = int(np.asarray(sd["encoder.encoders0.0.self_attn.linear_q_k_v.weight"]).shape[1])
    if kind == "sensevoicesmall":
        kw.update(dec_layers=0, vocab=int(np.asarray(sd["ctc.ctc_lo.weight"]).shape[0]))
        return W.make_config(**kw)
    kw["dec_layers"] = count(r"decoder\.decoders\.(\d+)\.")
    kw["vocab"] = int(np.asarray(sd["decoder.output_layer.weight"]).shape[0])
    kw["timestamp_head"] = ("predictor.upsample_cnn.weight" in sd) if timestamp is None else bool(timestamp)
    if kind == "seacoparaformer":
        kw.update(seaco=True, seaco_layers=count(r"seaco_decoder\.decoders\.(\d+)\."),
                  seaco_ffn=int(np.asarray(sd["seaco_decoder.decoders.0.feed_forward.w_1.weight"]).shape[0]),
                  seaco_kernel=int(np.asarray(sd["seaco_decoder.decoders.0.self_attn.fsmn_block.weight"]).shape[-1]),
                  seaco_lstm_layers=count(r"bias_encoder\.weight_ih_l(\d+)$"))
    return W.make_config(**kw)


def state_dict_to_pfw(sd: dict, cfg: dict) -> dict:
    """-> PFW weight dict; raises KeyError listing every missing checkpoint key, ValueError on a shape clash
    with the synthetic inventory of the same geometry (which is what the engine will bind)."""
    nm = name_map(cfg)
    missing = [v for v in nm.values() if v not in sd]
    if missing:
        raise KeyError("checkpoint lacks %d expected tensors, e.g. %s" % (len(missing), missing[:5]))
    out = {k: _layout(k, sd[v]) for k, v in nm.items()}
    probe = dict(cfg, vocab=min(cfg["vocab"], 64))                  # shapes only: keep the reference inventory small
    ref = W.synth_weights(probe, 0)
    for k, a in out.items():
        want = list(ref[k].shape)
        got = list(a.shape)
        if k in ("decoder.output.weight", "decoder.output.bias", "ctc.weight", "ctc.bias", "seaco.output.weight",
                 "seaco.output.bias", "seaco.embed.weight"):
            want[0] = got[0]                                        # vocabulary-sized
        if want != got:
            raise ValueError("%s: shape %s, expected %s" % (k, got, want))
    for k, v in nm.items():                                         # an int8 export's stored bytes travel beside the float image
        if v + "_q" in sd and v + "_zp" in sd and v + "_scale" in sd and np.asarray(sd[v + "_q"]).shape == out[k].shape:
            out[k + "_q"] = np.ascontiguousarray(sd[v + "_q"], np.uint8)
            out[k + "_zp"] = np.ascontiguousarray(sd[v + "_zp"], np.uint8)
            out[k + "_scale"] = np.ascontiguousarray(sd[v + "_scale"], np.float32)
    return out


# ------------------------------------------------------------------ ONNX ingestion ---------
_LSTM_IOFC_TO_IFGO = (0, 2, 3, 1)      # ONNX LSTM gate blocks are i,o,f,c; PyTorch (and the engine) use i,f,g(=c),o


def _reorder_gates(a, H):
    blocks = [a[k * H:(k + 1) * H] for k in range(4)]
    return np.concatenate([blocks[k] for k in _LSTM_IOFC_TO_IFGO], axis=0)


_Q_SUFFIXES = ("_q", "_zp", "_scale")         # `<linear>.weight` + suffix: the stored bytes of a quantised Linear


def onnx_to_state_dict(graph, expected_names) -> dict:
    """Initializers of a FunASR ONNX export -> {FunASR parameter name: float32 array}.

    * `X_quantized` + `X_scale` + `X_zero_point` (onnxruntime quantize_dynamic naming) are de-quantised to X (what
      math modes 0 / 1 multiply) AND carried as stored: `<linear>.weight_q` (uint8 [N, K]; a signed export's bytes are
      shifted by 128 together with the zero point, which leaves q - zp unchanged), `<linear>.weight_zp` (uint8 [N]),
      `<linear>.weight_scale` (float32 [N]; a per-tensor scale is repeated) — what math_mode 2 multiplies.
    * torch.onnx exports nn.Linear on 3-D inputs as MatMul(x, W^T) with an anonymous initializer followed by
      Add(bias): the weight is named after the bias it feeds; the bias-free decoder `feed_forward.w_2` is named
      after the `feed_forward.norm` LayerNorm that produces its input.
    * LSTM nodes carry W/R/B in ONNX layout [dirs, 4H, ...] with gate order i,o,f,c: split per direction, gates
      re-ordered; bidirectional -> predictor.blstm (BiCIF), unidirectional -> bias_encoder layers in graph order.
    * names are matched on suffixes against `expected_names` (export wrappers prepend / insert module names).
    Unvalidated against a real export (none exists in the build image); everything unmatched is ignored here and
    reported by state_dict_to_pfw as missing."""
    ini = dict(graph.initializers)
    flt = {}
    stored = {}                      # base -> (q uint8 [K, N], zp uint8 [N], scale float32 [N]) of a 2-D quantised MatMul operand
    for name, arr in ini.items():
        if name.endswith("_quantized") and (name[:-10] + "_scale") in ini:
            base = name[:-10]
            scale = np.asarray(ini[base + "_scale"], np.float32)
            zpi = np.asarray(ini.get(base + "_zero_point", 0))
            zp = zpi.astype(np.float32)
            flt[base] = ((arr.astype(np.float32) - zp) * scale).astype(np.float32)
            if arr.ndim == 2 and arr.dtype in (np.uint8, np.int8) and scale.size in (1, arr.shape[1]) and zpi.size in (1, arr.shape[1]):
                shift = 128 if arr.dtype == np.int8 else 0
                stored[base] = ((arr.astype(np.int32) + shift).astype(np.uint8),
                                np.broadcast_to((zpi.astype(np.int32) + shift).astype(np.uint8).reshape(-1), (arr.shape[1],)).copy(),
                                np.broadcast_to(scale.reshape(-1), (arr.shape[1],)).astype(np.float32).copy())
        elif arr.dtype in (np.float32, np.float16, np.float64) and not name.endswith(("_scale", "_zero_point")):
            flt[name] = arr.astype(np.float32)

    def base_of(n):
        return n[:-10] if n.endswith("_quantized") else n

    sd = dict(flt)
    through = ("Cast", "Mul", "Add", "Reshape", "DynamicQuantizeLinear", "Identity")
    for node in graph.nodes:
        if node.op_type in ("MatMul", "MatMulInteger") and len(node.inputs) >= 2 and base_of(node.inputs[1]) in flt:
            wt = flt[base_of(node.inputs[1])]
            target = None
            frontier, depth = [node.outputs[0]], 0
            while frontier and depth < 5 and target is None:              # forward: the bias Add
                nxt = []
                for val in frontier:
                    for c in graph.consumers(val):
                        if c.op_type == "Add":
                            for i in c.inputs:
                                if i in flt and i.endswith(".bias") and flt[i].ndim == 1 and flt[i].shape[0] == wt.shape[-1]:
                                    target = i[:-4] + "weight"
                        if c.op_type in through:
                            nxt += c.outputs
                frontier, depth = nxt, depth + 1
            if target is None:                                             # backward: bias-free w_2 after feed_forward.norm
                val, depth = node.inputs[0], 0
                while val and depth < 8 and target is None:
                    pr = graph.producer(val)
                    if pr is None:
                        break
                    for i in pr.inputs:
                        if i in flt and ".feed_forward.norm." in i:
                            target = i.split(".feed_forward.norm.")[0] + ".feed_forward.w_2.weight"
                    val, depth = (pr.inputs[0] if pr.inputs else None), depth + 1
            if target is not None and target not in sd:
                sd[target] = np.ascontiguousarray(wt.T)
                if base_of(node.inputs[1]) in stored:
                    q, zp, sc = stored[base_of(node.inputs[1])]
                    sd[target + "_q"], sd[target + "_zp"], sd[target + "_scale"] = np.ascontiguousarray(q.T), zp, sc
    uni = 0
    for node in graph.nodes:
        if node.op_type != "LSTM" or len(node.inputs) < 3:
            continue
        Wt, Rt = flt.get(base_of(node.inputs[1])), flt.get(base_of(node.inputs[2]))
        Bt = flt.get(base_of(node.inputs[3])) if len(node.inputs) > 3 and node.inputs[3] else None
        if Wt is None or Rt is None:
            continue
        H = Rt.shape[-1]
        bidir = str(node.attrs.get("direction", "forward")) == "bidirectional" or Wt.shape[0] == 2
        for d in range(Wt.shape[0]):
            if bidir:
                pre, sfx = "predictor.blstm.", "_l0" + ("_reverse" if d == 1 else "")
            else:
                pre, sfx = "bias_encoder.", "_l%d" % uni
            sd[pre + "weight_ih" + sfx] = _reorder_gates(Wt[d], H)
            sd[pre + "weight_hh" + sfx] = _reorder_gates(Rt[d], H)
            if Bt is not None:
                sd[pre + "bias_ih" + sfx] = _reorder_gates(Bt[d][:4 * H], H)
                sd[pre + "bias_hh" + sfx] = _reorder_gates(Bt[d][4 * H:], H)
        if not bidir:
            uni += 1
    # suffix normalisation onto the expected FunASR names
    out = {}
    aliases = {"embedding.weight": "bias_embed.weight", "embed.weight": "embed.weight"}
    exp = sorted(expected_names, key=len, reverse=True)
    for k, v in sd.items():
        sfx = next((x for x in _Q_SUFFIXES if k.endswith(".weight" + x)), "")
        k0 = k[:len(k) - len(sfx)]
        cands = {k0, k0.replace(".model.", "."), aliases.get(k0, k0)}
        for e in exp:
            if any(c == e or c.endswith("." + e) for c in cands):
                out.setdefault(e + sfx, v)
                break
    return out


def onnx_to_pfw(model_path, eb_path=None, kind="paraformer", timestamp=None):
    """model.onnx / model.int8.onnx (+ model_eb*.onnx for SeACo) -> (cfg, PFW weights)."""
    from . import onnx_reader as R
    graphs = [R.load(model_path)] + ([R.load(eb_path)] if eb_path else [])
    # every name any supported geometry could ask for (layer indices bounded generously; unmatched ones are simply absent)
    probe = W.make_config(kind=kind, enc_layers=64, tp_layers=32 if kind == "sensevoicesmall" else 0, dec_layers=32,
                          timestamp_head=True, seaco=(kind == "seacoparaformer"), seaco_layers=8, seaco_lstm_layers=4)
    expected = set(name_map(probe).values())
    sd = {}
    for g in graphs:
        sd.update(onnx_to_state_dict(g, expected))
    cfg = infer_config(sd, kind, timestamp)
    wts = state_dict_to_pfw(sd, cfg)
    # an int8 export: record which Linears the export left in float (FunASR passes nodes_to_exclude to quantize_dynamic).
    # The engine and the oracle decide by the stored bytes themselves; the key documents the set in the container.
    if any(k.endswith(".weight_q") for k in wts):
        lin = [k[:-7] for k, v in wts.items() if k.endswith(".weight") and np.asarray(v).ndim == 2 and k[:-7] + ".bias" in wts
               or k.endswith(".ffn.w2.weight")]
        cfg["int8_exclude"] = tuple(sorted(n for n in lin if n + ".weight_q" not in wts))
    return cfg, wts


# ------------------------------------------------------------------ FSMN-VAD ---------
def parse_mvn_text(text: str):
    """(shift, scale) float32 of an am.mvn / vad.mvn in the kaldi-nnet text layout (weights.format_mvn_text): the vectors
    between '[' and ']' on the <LearnRateCoef> lines that follow <AddShift> and <Rescale>."""
    out = {}
    lines = text.splitlines()
    for i, ln in enumerate(lines):
        tag = ln.split()[0] if ln.split() else ""
        if tag in ("<AddShift>", "<Rescale>"):
            for nxt in lines[i + 1: i + 3]:
                if nxt.lstrip().startswith("<LearnRateCoef>") and "[" in nxt and "]" in nxt:
                    out[tag] = np.asarray([float(x) for x in nxt[nxt.index("[") + 1: nxt.rindex("]")].split()], np.float32)
                    break
    if "<AddShift>" not in out or "<Rescale>" not in out or out["<AddShift>"].shape != out["<Rescale>"].shape:
        raise ValueError("mvn: no <AddShift> / <Rescale> vectors of one length")
    return out["<AddShift>"], out["<Rescale>"]


def vad_name_map(n_layers: int) -> dict:
    """PFW tensor name -> FunASR FSMN-VAD state_dict key (funasr.models.fsmn_vad_streaming.encoder.FSMN under `encoder.`)."""
    m = {}
    for a in ("in1", "in2", "out1", "out2"):
        f = {"in1": "in_linear1", "in2": "in_linear2", "out1": "out_linear1", "out2": "out_linear2"}[a]
        m[a + ".weight"], m[a + ".bias"] = "encoder.%s.linear.weight" % f, "encoder.%s.linear.bias" % f
    for l in range(n_layers):
        m["fsmn.%d.linear.weight" % l] = "encoder.fsmn.%d.linear.linear.weight" % l
        m["fsmn.%d.taps" % l] = "encoder.fsmn.%d.fsmn_block.conv_left.weight" % l
        m["fsmn.%d.affine.weight" % l] = "encoder.fsmn.%d.affine.linear.weight" % l
        m["fsmn.%d.affine.bias" % l] = "encoder.fsmn.%d.affine.linear.bias" % l
    return m


def vad_state_dict_to_pfw(sd: dict, shift, scale, sil_ids=(0,), lfr_m: int = 5, lstride: int = 1):
    """FunASR FSMN-VAD state dict (+ the vad.mvn vectors) -> (cfg, PFW weights) of kind "fsmnvad".  The depthwise
    conv_left.weight [proj, 1, lorder, 1] becomes taps [lorder, proj]; lstride is the conv's dilation, which a state dict does
    not carry (the ONNX route reads it from the graph).  KeyError lists missing keys; ValueError on a shape clash or a
    right-context block (conv_right: rorder > 0 is not supported)."""
    sd = {k: np.asarray(v, np.float32) for k, v in sd.items()}
    if any(".conv_right." in k for k in sd):
        raise ValueError("fsmnvad: the checkpoint has conv_right tensors (rorder > 0), which is not supported")
    ids = {int(m.group(1)) for k in sd for m in [re.match(r"encoder\.fsmn\.(\d+)\.", k)] if m}
    n_layers = max(ids) + 1 if ids else 0
    nm = vad_name_map(n_layers)
    missing = [v for v in nm.values() if v not in sd]
    if missing or not n_layers:
        raise KeyError("checkpoint lacks %d expected tensors, e.g. %s" % (len(missing), missing[:5]))
    conv = sd[nm["fsmn.0.taps"]]
    if conv.ndim != 4 or conv.shape[1] != 1 or conv.shape[3] != 1:
        raise ValueError("fsmnvad: conv_left.weight has shape %s, expected [proj, 1, lorder, 1]" % (list(conv.shape),))
    shift, scale = np.asarray(shift, np.float32).reshape(-1), np.asarray(scale, np.float32).reshape(-1)
    I = int(sd[nm["in1.weight"]].shape[1])
    if I % lfr_m:
        raise ValueError("fsmnvad: input width %d is no multiple of lfr_m %d" % (I, lfr_m))
    cfg = W.fsmn_vad_config(n_mels=I // lfr_m, lfr_m=lfr_m, affine_dim=int(sd[nm["in1.weight"]].shape[0]),
                            linear_dim=int(sd[nm["in2.weight"]].shape[0]), proj_dim=int(conv.shape[0]),
                            output_dim=int(sd[nm["out2.weight"]].shape[0]), n_layers=n_layers, lorder=int(conv.shape[2]),
                            lstride=int(lstride), sil_ids=tuple(int(i) for i in sil_ids))
    out = {"cmvn.shift": shift, "cmvn.scale": scale}
    for k, v in nm.items():
        a = sd[v]
        out[k] = np.ascontiguousarray(a[:, 0, :, 0].T if k.endswith(".taps") else a)
    for k, want in W.vad_tensor_shapes(cfg).items():
        if tuple(out[k].shape) != tuple(want):
            raise ValueError("%s: shape %s, expected %s" % (k, list(out[k].shape), list(want)))
    if any(not 0 <= i < cfg["output_dim"] for i in cfg["sil_ids"]):
        raise ValueError("fsmnvad: a silence id is outside [0, output_dim)")
    return cfg, out


def vad_onnx_to_state_dict(graph):
    """A FunASR FSMN-VAD ONNX export -> ({FunASR parameter name: float32 array}, lstride).  The exporter anonymises the MatMul
    weights, so the graph is walked from `speech` in node order: MatMul nodes whose second operand is a 2-D initialiser and
    Conv nodes with a 4-D initialiser, in the order in_linear1, in_linear2, (linear, conv_left, affine) per block, out_linear1,
    out_linear2; a bias is the 1-D initialiser of the Add that consumes the MatMul.  The in_cache* / out_cache* inputs and
    outputs and the trailing Softmax carry no parameters and are passed over.  ValueError when the sequence does not have
    that shape."""
    ini = graph.initializers
    if "speech" not in graph.inputs:
        raise ValueError("fsmnvad: the graph has no input named speech")
    seq = []
    for node in graph.nodes:
        if node.op_type == "MatMul" and len(node.inputs) == 2 and node.inputs[1] in ini and ini[node.inputs[1]].ndim == 2:
            bias = None
            for c in graph.consumers(node.outputs[0]):
                if c.op_type == "Add":
                    for i in c.inputs:
                        if i in ini and ini[i].ndim == 1 and ini[i].shape[0] == ini[node.inputs[1]].shape[1]:
                            bias = np.asarray(ini[i], np.float32)
            seq.append(("mm", np.ascontiguousarray(np.asarray(ini[node.inputs[1]], np.float32).T), bias))
        elif node.op_type == "Conv" and len(node.inputs) >= 2 and node.inputs[1] in ini and ini[node.inputs[1]].ndim == 4:
            dil = node.attrs.get("dilations") or [1, 1]
            seq.append(("conv", np.asarray(ini[node.inputs[1]], np.float32), int(dil[0])))
    kinds = "".join("c" if s[0] == "conv" else ("B" if s[2] is not None else "m") for s in seq)
    mt = re.fullmatch(r"BB((?:mcB)+)BB", kinds)
    if not mt:
        raise ValueError("fsmnvad: the graph's MatMul / Conv sequence %r is not in_linear1, in_linear2, (linear, conv_left, affine)*, "
                         "out_linear1, out_linear2" % kinds)
    n_layers = len(mt.group(1)) // 3
    sd = {}

    def put(prefix, s):
        sd[prefix + ".weight"] = s[1]
        if s[2] is not None:
            sd[prefix + ".bias"] = s[2]
    put("encoder.in_linear1.linear", seq[0]); put("encoder.in_linear2.linear", seq[1])
    strides = set()
    for l in range(n_layers):
        lin, conv, aff = seq[2 + 3 * l: 5 + 3 * l]
        put("encoder.fsmn.%d.linear.linear" % l, lin)
        sd["encoder.fsmn.%d.fsmn_block.conv_left.weight" % l] = conv[1]
        strides.add(conv[2])
        put("encoder.fsmn.%d.affine.linear" % l, aff)
    put("encoder.out_linear1.linear", seq[-2]); put("encoder.out_linear2.linear", seq[-1])
    if len(strides) != 1:
        raise ValueError("fsmnvad: the blocks have different dilations %s" % sorted(strides))
    return sd, strides.pop()


def vad_to_pfw(model_path, mvn_path, sil_ids=(0,), lfr_m=5, lstride=1):
    with open(mvn_path, "r") as f:
        shift, scale = parse_mvn_text(f.read())
    if str(model_path).endswith(".onnx"):
        from . import onnx_reader as R
        sd, lstride = vad_onnx_to_state_dict(R.load(model_path))
    else:
        import torch
        sd = torch.load(model_path, map_location="cpu")
        sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
        sd = {k: v.float().numpy() for k, v in sd.items() if hasattr(v, "numpy")}
    return vad_state_dict_to_pfw(sd, shift, scale, sil_ids, lfr_m, lstride)


def punc_state_dict_to_pfw(sd: dict, tokens, punc_list=None, sentence_end_id=None, heads: int = 8, causal: bool = False):
    """FunASR CT-Transformer state dict (+ the vocabulary) -> (cfg, PFW weights) of kind "cttransformer".  causal: the
    streaming form (the same tensors; the header says causal = 1 and sanm_shift = (kernel - 1) / 2, all FSMN taps to the left).  FunASR's names:
    embed.weight (or embed.0.weight), encoder.encoders0.0.* for the first block and encoder.encoders.N.* for block N + 1, each
    with norm1, self_attn.linear_q_k_v, self_attn.fsmn_block.weight [d_model, 1, kernel], self_attn.linear_out, norm2,
    feed_forward.w_1 / w_2; encoder.after_norm; decoder.  Refuses anything else: no silent defaults for a missing tensor."""
    sd = {k: np.asarray(v, dtype=np.float32) for k, v in sd.items()}
    emb = sd.get("embed.weight", sd.get("embed.0.weight"))
    if emb is None or emb.ndim != 2:
        raise ValueError("cttransformer: the checkpoint has no embed.weight [vocab, d_model]")
    tokens = [str(t) for t in tokens]
    if len(tokens) != emb.shape[0]:
        raise ValueError("cttransformer: %d tokens for an embedding of %d rows" % (len(tokens), emb.shape[0]))
    blocks = ["encoder.encoders0.0."] if any(k.startswith("encoder.encoders0.0.") for k in sd) else []
    n = 0
    while any(k.startswith("encoder.encoders.%d." % n) for k in sd):
        blocks.append("encoder.encoders.%d." % n)
        n += 1
    if not blocks:
        raise ValueError("cttransformer: the checkpoint has no encoder.encoders0.0.* / encoder.encoders.N.* blocks")
    punc_list = list(punc_list or W.CT_TRANSFORMER_CONFIG["punc_list"])

    def get(name):
        if name not in sd:
            raise ValueError("cttransformer: the checkpoint lacks " + name)
        return sd[name]
    w = {"embed.weight": emb}
    for l, b in enumerate(blocks):
        p = "layers.%d." % l
        for src, dst in (("norm1", "norm1"), ("self_attn.linear_q_k_v", "attn.qkv"), ("self_attn.linear_out", "attn.out"), ("norm2", "norm2"),
                         ("feed_forward.w_1", "ffn.w1"), ("feed_forward.w_2", "ffn.w2")):
            w[p + dst + ".weight"] = get(b + src + ".weight")
            w[p + dst + ".bias"] = get(b + src + ".bias")
        f = get(b + "self_attn.fsmn_block.weight")
        if f.ndim != 3 or f.shape[1] != 1:
            raise ValueError("cttransformer: fsmn_block.weight has shape %s, expected [d_model, 1, kernel]" % (list(f.shape),))
        w[p + "attn.fsmn.weight"] = f[:, 0, :]
    for src, dst in (("encoder.after_norm", "after_norm"), ("decoder", "decoder")):
        w[dst + ".weight"] = get(src + ".weight")
        w[dst + ".bias"] = get(src + ".bias")
    if w["decoder.weight"].shape[0] != len(punc_list):
        raise ValueError("cttransformer: the decoder has %d classes, punc_list %d" % (w["decoder.weight"].shape[0], len(punc_list)))
    if sentence_end_id is None:
        sentence_end_id = punc_list.index("\u3002") if "\u3002" in punc_list else -1
    cfg = W.ct_transformer_config(vocab=int(emb.shape[0]), d_model=int(emb.shape[1]), heads=int(heads), ffn=int(w["layers.0.ffn.w1.weight"].shape[0]),
                                  kernel=int(w["layers.0.attn.fsmn.weight"].shape[1]), n_layers=len(blocks), punc_list=punc_list,
                                  sentence_end_id=int(sentence_end_id))
    if causal:
        cfg.update(causal=1, sanm_shift=(int(cfg["kernel"]) - 1) // 2)
    for name, shape in W.punc_tensor_shapes(cfg).items():
        if tuple(w[name].shape) != tuple(shape):
            raise ValueError("cttransformer: %s has shape %s, expected %s" % (name, list(w[name].shape), list(shape)))
    w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}
    w["vocab"] = np.frombuffer("\n".join(tokens).encode("utf-8"), dtype=np.uint8).copy()
    return cfg, w


def punc_onnx_to_state_dict(graph) -> dict:
    """A FunASR CT-Transformer ONNX export -> {FunASR parameter name: float32 array}, through the walk the Paraformer encoder's
    export goes through (onnx_to_state_dict: the anonymous MatMul weights are named after the bias their Add carries).  Refuses
    (ValueError) a graph that is not an embedding Gather followed by SAN-M blocks and one more Linear: per block one Softmax, one
    depthwise Conv whose weight is [d_model, 1, kernel] and four MatMuls against 2-D initialisers, plus the decoder's."""
    blocks = ["encoder.encoders0.0."] + ["encoder.encoders.%d." % n for n in range(64)]
    parts = ("norm1", "self_attn.linear_q_k_v", "self_attn.linear_out", "norm2", "feed_forward.w_1", "feed_forward.w_2")
    expected = {"embed.weight", "encoder.after_norm.weight", "encoder.after_norm.bias", "decoder.weight", "decoder.bias"}
    for b in blocks:
        expected |= {b + q + sfx for q in parts for sfx in (".weight", ".bias")} | {b + "self_attn.fsmn_block.weight"}
    sd = {k: v for k, v in onnx_to_state_dict(graph, expected).items() if not k.endswith(_Q_SUFFIXES)}
    ini = graph.initializers
    n_blocks = len({k.split("self_attn.fsmn_block.weight")[0] for k in sd if k.endswith("self_attn.fsmn_block.weight")})
    gathers = [n for n in graph.nodes if n.op_type == "Gather" and n.inputs and n.inputs[0] in ini and np.asarray(ini[n.inputs[0]]).ndim == 2]
    softmax = sum(1 for n in graph.nodes if n.op_type == "Softmax")
    convs = [n for n in graph.nodes if n.op_type == "Conv"]
    mms = sum(1 for n in graph.nodes if n.op_type == "MatMul" and len(n.inputs) == 2 and n.inputs[1] in ini and np.asarray(ini[n.inputs[1]]).ndim == 2)
    if "embed.weight" not in sd or len(gathers) != 1 or n_blocks < 1 or softmax != n_blocks or len(convs) != n_blocks or mms != 4 * n_blocks + 1:
        raise ValueError("cttransformer: the graph is not an embedding followed by SAN-M blocks and a decoder (%d embedding Gather, %d "
                         "fsmn_block weights, %d Softmax, %d Conv, %d MatMul against a matrix)" % (len(gathers), n_blocks, softmax, len(convs), mms))
    d = sd["embed.weight"].shape[1]
    for n in convs:
        wt = np.asarray(ini.get(n.inputs[1], np.zeros(0))) if len(n.inputs) > 1 else np.zeros(0)
        if wt.ndim != 3 or wt.shape[0] != d or wt.shape[1] != 1 or int(n.attrs.get("group", 1)) != d:
            raise ValueError("cttransformer: a Conv of the graph is not a depthwise FSMN block over d_model channels")
    return sd


def punc_to_pfw(model_path, tokens_path, heads=8, causal=False):
    """model.pt | model.onnx + tokens -> (cfg, PFW weights) of kind "cttransformer".  causal: the state-dict route only (an
    ONNX export has its masks and its FSMN padding baked into the graph, and the walk does not read them)."""
    if str(model_path).endswith(".onnx"):
        if causal:
            raise ValueError("cttransformer: --causal works on a state dict (model.pt); an ONNX export does not say how it masks")
        from . import onnx_reader as R
        sd = punc_onnx_to_state_dict(R.load(model_path))
    else:
        import torch
        sd = torch.load(model_path, map_location="cpu")
        sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
        sd = {k: v.float().numpy() for k, v in sd.items() if hasattr(v, "numpy")}
    return punc_state_dict_to_pfw(sd, read_punc_tokens(tokens_path), heads=heads, causal=causal)


def read_punc_tokens(path):
    """tokens.json (a JSON list of strings) or a text file with one token per line."""
    import json
    with open(path, "r", encoding="utf-8") as f:
        text = f.read()
    if text.lstrip().startswith("["):
        return [str(t) for t in json.loads(text)]
    return [ln for ln in text.split("\n") if ln != ""]


def spk_state_dict_to_pfw(sd: dict, seg_len: int = 100, dilations=(1, 2, 2), eps: float = 1e-5):
    """3D-Speaker CAMPPlus state dict -> (cfg, PFW weights) of kind "campplus" (weights.spk_tensor_shapes).  3D-Speaker's names
    as remembered: head.conv1 / head.bn1, head.layerL.B.{conv1, bn1, conv2, bn2, shortcut.0 (conv), shortcut.1 (bn)}, head.conv2 /
    head.bn2; xvector.tdnn.{linear, nonlinear.batchnorm}; xvector.blockK.tdnndN.{nonlinear1.batchnorm, linear1, nonlinear2.batchnorm,
    cam_layer.linear_local, cam_layer.linear1, cam_layer.linear2}; xvector.transitK.{nonlinear.batchnorm, linear};
    xvector.out_nonlinear.batchnorm; xvector.dense.{linear, nonlinear.batchnorm (no affine)}.  Every BatchNorm is folded with
    `eps` (a dict name -> eps overrides it per BatchNorm): into the convolution or Linear in front of it where nothing stands
    between, else it stays as scale / shift.  seg_len and the dilations are not in a state dict.  Missing or misshapen tensors
    are refused.  No real file has been through this function."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}

    def get(name):
        if name not in sd:
            raise ValueError("campplus: the checkpoint lacks " + name)
        return sd[name]

    def bn(prefix, affine=True):
        e = eps.get(prefix, 1e-5) if isinstance(eps, dict) else eps
        var, mean = get(prefix + ".running_var"), get(prefix + ".running_mean")
        scale = 1.0 / np.sqrt(var + e)
        if affine:
            scale = scale * get(prefix + ".weight")
        shift = (get(prefix + ".bias") if affine else 0.0) - mean * scale
        return scale, shift

    def fold(conv, norm, out, w, affine=True, squeeze=False):
        k = get(conv + ".weight")
        if squeeze:
            if k.ndim != 3 or k.shape[2] != 1:
                raise ValueError("campplus: %s.weight has shape %s, expected [out, in, 1]" % (conv, list(k.shape)))
            k = k[:, :, 0]
        scale, shift = bn(norm, affine)
        if scale.shape != (k.shape[0],):
            raise ValueError("campplus: %s has %d channels, %s.weight %d rows" % (norm, scale.shape[0], conv, k.shape[0]))
        w[out + ".weight"] = k * scale.reshape((-1,) + (1,) * (k.ndim - 1))
        w[out + ".bias"] = shift + (get(conv + ".bias") * scale if conv + ".bias" in sd else 0.0)

    import re
    c1 = get("head.conv1.weight")
    tw = get("xvector.tdnn.linear.weight")
    if c1.ndim != 4 or tw.ndim != 3 or tw.shape[1] % c1.shape[0] != 0:
        raise ValueError("campplus: head.conv1.weight / xvector.tdnn.linear.weight have shapes %s / %s" % (list(c1.shape), list(tw.shape)))
    blocks = [len({int(m.group(1)) for m in (re.match(r"xvector\.block%d\.tdnnd(\d+)\." % b, k) for k in sd) if m}) for b in (1, 2, 3)]
    if min(blocks) < 1 or any(re.match(r"xvector\.block4\.", k) for k in sd):
        raise ValueError("campplus: the checkpoint does not have exactly three dense blocks")
    l1 = get("xvector.block1.tdnnd1.cam_layer.linear_local.weight")
    cfg = W.campplus_config(n_mels=8 * (tw.shape[1] // c1.shape[0]), m_channels=c1.shape[0], init_channels=tw.shape[0], growth=l1.shape[0],
                            bn_channels=l1.shape[1], blocks=blocks, dilations=[int(d) for d in dilations], seg_len=int(seg_len),
                            embedding=get("xvector.dense.linear.weight").shape[0])
    w = {}
    fold("head.conv1", "head.bn1", "head.conv1", w)
    for layer in (1, 2):
        for blk in (0, 1):
            p = "head.layer%d.%d." % (layer, blk)
            fold(p + "conv1", p + "bn1", p + "conv1", w)
            fold(p + "conv2", p + "bn2", p + "conv2", w)
            if blk == 0:
                fold(p + "shortcut.0", p + "shortcut.1", p + "shortcut", w)
    fold("head.conv2", "head.bn2", "head.conv2", w)
    fold("xvector.tdnn.linear", "xvector.tdnn.nonlinear.batchnorm", "tdnn", w)
    for b in (1, 2, 3):
        for l in range(blocks[b - 1]):
            s, o = "xvector.block%d.tdnnd%d." % (b, l + 1), "block%d.%d." % (b, l)
            w[o + "bn1.scale"], w[o + "bn1.shift"] = bn(s + "nonlinear1.batchnorm")
            fold(s + "linear1", s + "nonlinear2.batchnorm", o + "linear1", w, squeeze=True)
            w[o + "local.weight"] = get(s + "cam_layer.linear_local.weight")
            for src, dst in (("linear1", "cam1"), ("linear2", "cam2")):
                k = get(s + "cam_layer." + src + ".weight")
                w[o + dst + ".weight"] = k[:, :, 0] if k.ndim == 3 and k.shape[2] == 1 else k
                w[o + dst + ".bias"] = get(s + "cam_layer." + src + ".bias")
        s, o = "xvector.transit%d." % b, "transit%d." % b
        w[o + "bn.scale"], w[o + "bn.shift"] = bn(s + "nonlinear.batchnorm")
        k = get(s + "linear.weight")
        w[o + "weight"] = k[:, :, 0] if k.ndim == 3 and k.shape[2] == 1 else k
    w["out_bn.scale"], w["out_bn.shift"] = bn("xvector.out_nonlinear.batchnorm")
    fold("xvector.dense.linear", "xvector.dense.nonlinear.batchnorm", "dense", w, affine=False, squeeze=True)
    shapes = W.spk_tensor_shapes(cfg)
    for name, shape in shapes.items():
        if tuple(np.shape(w[name])) != tuple(shape):
            raise ValueError("campplus: %s has shape %s, expected %s" % (name, list(np.shape(w[name])), list(shape)))
        if not np.isfinite(w[name]).all():
            raise ValueError("campplus: %s holds a value that is not finite" % name)
    return cfg, {name: np.ascontiguousarray(w[name], dtype=np.float32) for name in shapes}


def spk_to_pfw(model_path, seg_len=100, dilations=(1, 2, 2)):
    """campplus.bin | .pt (a state dict; an ONNX route does not exist) -> (cfg, PFW weights) of kind "campplus"."""
    if str(model_path).endswith(".onnx"):
        raise ValueError("campplus: the converter reads a state dict (.bin / .pt), not an ONNX export")
    import torch
    sd = torch.load(model_path, map_location="cpu")
    sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
    sd = {k: v.double().numpy() for k, v in sd.items() if hasattr(v, "numpy")}
    return spk_state_dict_to_pfw(sd, seg_len, dilations)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 2:
        print(__doc__)
        return 2
    kind, ts = "paraformer", None
    if "--kind" in argv:
        kind = argv[argv.index("--kind") + 1]
    if kind == "fsmnvad":
        if "--mvn" not in argv:
            print("--kind fsmnvad needs --mvn vad.mvn (the model's own CMVN)")
            return 2
        sil = tuple(int(x) for x in argv[argv.index("--sil") + 1].split(",")) if "--sil" in argv else (0,)
        lfr_m = int(argv[argv.index("--lfr-m") + 1]) if "--lfr-m" in argv else 5
        lstride = int(argv[argv.index("--lstride") + 1]) if "--lstride" in argv else 1
        cfg, wts = vad_to_pfw(argv[0], argv[argv.index("--mvn") + 1], sil, lfr_m, lstride)
        W.save_pfw(argv[1], cfg, wts)
        print("wrote %s (%s, %d tensors)" % (argv[1], cfg["kind"], len(wts)))
        return 0
    if kind == "campplus":
        seg_len = int(argv[argv.index("--seg-len") + 1]) if "--seg-len" in argv else 100
        dil = tuple(int(x) for x in argv[argv.index("--dilations") + 1].split(",")) if "--dilations" in argv else (1, 2, 2)
        cfg, wts = spk_to_pfw(argv[0], seg_len, dil)
        W.save_pfw(argv[1], cfg, wts)
        print("wrote %s (%s, %d tensors)" % (argv[1], cfg["kind"], len(wts)))
        return 0
    if kind == "cttransformer":
        if "--tokens" not in argv:
            print("--kind cttransformer needs --tokens tokens.json (or a file with one token per line)")
            return 2
        heads = int(argv[argv.index("--heads") + 1]) if "--heads" in argv else 8
        try:
            cfg, wts = punc_to_pfw(argv[0], argv[argv.index("--tokens") + 1], heads, causal="--causal" in argv)
        except ValueError as ex:
            if "--causal" not in str(ex):
                raise
            print(ex)
            return 2
        W.save_pfw(argv[1], cfg, wts)
        print("wrote %s (%s, %d tensors)" % (argv[1], cfg["kind"], len(wts)))
        return 0
    if "--timestamp" in argv:
        ts = True
    if argv[0].endswith(".onnx"):
        eb = argv[argv.index("--eb") + 1] if "--eb" in argv else None
        cfg, wts = onnx_to_pfw(argv[0], eb, kind, ts)
        W.save_pfw(argv[1], cfg, wts)
        print("wrote %s (%s, %d tensors, from ONNX)" % (argv[1], cfg["kind"], len(wts)))
        return 0
    import torch
    sd = torch.load(argv[0], map_location="cpu")
    sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
    sd = {k: v.float().numpy() for k, v in sd.items() if hasattr(v, "numpy")}
    cfg = infer_config(sd, kind, ts)
    W.save_pfw(argv[1], cfg, state_dict_to_pfw(sd, cfg))
    print("wrote %s (%s, %d tensors)" % (argv[1], cfg["kind"], len(name_map(cfg))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
