"""The definition of streaming punctuation (paraformer_hip.h "Punctuation, streaming") in numpy float64: the
causal CT-Transformer on a context, the stream loop with its two restarts and the flush, and the committed words of a
streaming recogniser's partial text.  The host twin (csrc/punc.cpp host_punc_stream_step) and the device form
(csrc/k_punc_stream.hip) are tested against this file; it shares no code with either, and takes from tests/punc_ref.py only
what both definitions share (the layer-0 input, the LayerNorm, the roundings, the arg-max, the word split, the assembly).

The definition is this project's.  The dimensions of FunASR's punc_ct-transformer_zh-cn-common-vad_realtime-vocab272727 are as
remembered; its "vad mask" between cached and new words is implied by a causal mask in every layer; whether its last layer
is causal could not be checked.  Nothing here is validated on a real model."""
import numpy as np

import punc_ref as R

MAX_CONTEXT = 256
DEFAULT_CONTEXT = 200
NO_RESTARTS = 1


def causal_config(cfg: dict) -> dict:
    """cfg with the two header keys of the streaming form."""
    return dict(cfg, causal=1, sanm_shift=(int(cfg["kernel"]) - 1) // 2)


def _network(w, cfg, ids, q):
    """The causal network on ONE context (all of it at once): logits [n, n_punc].  q: the rounding applied at the device
    form's rounding points R0 .. R5 (identity: the definition)."""
    D, H, K, NL = (int(cfg[k]) for k in ("d_model", "heads", "kernel", "n_layers"))
    T = len(ids)
    assert T <= MAX_CONTEXT
    if T == 0:
        return np.zeros((0, int(cfg["n_punc"])), np.float64)
    dh = D // H
    lin = lambda x, name: x @ q(w[name + ".weight"]).T + w[name + ".bias"].astype(np.float64)
    x = R.layer0_input(w, cfg, ids, embed=q(w["embed.weight"])).astype(np.float64)      # position = index in the context + 1
    mask = np.tril(np.ones((T, T), bool))                                               # key j <= query i
    for l in range(NL):
        p = "layers.%d." % l
        xn = q(R._ln(x, w[p + "norm1.weight"], w[p + "norm1.bias"]))
        qkv = lin(xn, p + "attn.qkv")
        qh, kh, vh = q(qkv[:, :D] * dh ** -0.5), q(qkv[:, D:2 * D]), q(qkv[:, 2 * D:])
        taps = w[p + "attn.fsmn.weight"].astype(np.float64)                              # [D, K]
        vp = np.concatenate([np.zeros((K - 1, D)), vh], axis=0)                          # a source before index 0 is skipped
        f = vh.copy()
        for j in range(K):
            f += taps[:, j][None, :] * vp[j: j + T]                                      # v_{t - (K - 1) + j}
        ctx = np.zeros((T, D))
        for h in range(H):
            s = qh[:, h * dh:(h + 1) * dh] @ kh[:, h * dh:(h + 1) * dh].T
            s = np.where(mask, s, -np.inf)
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            ctx[:, h * dh:(h + 1) * dh] = (q(e) @ vh[:, h * dh:(h + 1) * dh]) / e.sum(axis=-1, keepdims=True)
        x = x + (lin(q(ctx), p + "attn.out") + f)
        xn = q(R._ln(x, w[p + "norm2.weight"], w[p + "norm2.bias"]))
        hid = q(np.maximum(lin(xn, p + "ffn.w1"), 0.0))
        x = x + lin(hid, p + "ffn.w2")
    xn = q(R._ln(x, w["after_norm.weight"], w["after_norm.bias"]))
    return lin(xn, "decoder")


def logits64(w, cfg, ids) -> np.ndarray:
    return _network(w, cfg, ids, R._ident)


def emulate_f16(w, cfg, ids) -> np.ndarray:
    return _network(w, cfg, ids, R._h)


class Stream:
    """One stream of the loop.  forward(context ids) -> logits [n, n_punc] of the whole context (the last row is the new
    word's: the logits of word t depend on w_0 .. w_t alone)."""

    def __init__(self, forward, punc_list, sentence_end_id, max_context=DEFAULT_CONTEXT, no_restarts=False):
        assert 2 <= max_context <= MAX_CONTEXT
        self.forward, self.ix, self.end = forward, R.punc_index(punc_list), int(sentence_end_id)
        self.max_context, self.no_restarts = int(max_context), bool(no_restarts)
        self.context, self.last = [], 0

    def step(self, ids, flush=False):
        """(marks [n], mark_flags [n], logits [n, n_punc], flush_mark)"""
        marks, flags, zs = [], [], []
        for i in ids:
            self.context.append(int(i))
            assert len(self.context) <= MAX_CONTEXT
            z = self.forward(np.array(self.context, np.int32))[-1]
            p = int(R.argmax_ties_larger(z[None, :])[0])
            f = 0
            self.last = p
            if not self.no_restarts:
                if p >= 0 and p in (self.ix["period"], self.ix["question"]):
                    f, self.context = 1, []
                elif len(self.context) == self.max_context:
                    f, self.context = 2, []
            marks.append(p); flags.append(f); zs.append(z)
        fm = -1
        if flush:
            if self.context:
                fm = self.end if self.last in (self.ix["none"], self.ix["comma"], self.ix["pause"]) else self.last
            self.context = []
        P = len(zs[0]) if zs else 0
        return np.array(marks, np.int32), np.array(flags, np.int32), np.array(zs, np.float64).reshape(len(zs), P), fm


def loop_from_logits(z, punc_list, sentence_end_id, max_context=DEFAULT_CONTEXT, count=0):
    """The rule alone over given per-word logits (each row already computed in the context the rule implies):
    (marks, mark_flags, the count behind the last word)."""
    ix = R.punc_index(punc_list)
    p = R.argmax_ties_larger(np.asarray(z))
    flags, n = [], int(count)
    for v in p.tolist():
        n += 1
        if v in (ix["period"], ix["question"]) and v >= 0:
            flags.append(1); n = 0
        elif n == max_context:
            flags.append(2); n = 0
        else:
            flags.append(0)
    return p, np.array(flags, np.int32), n


# ---- committed words: the words of a streaming partial text that later pieces cannot change
_BAR = "\u2581"
_SILENT = ("<s>", "<blank>", "<unk>")


def online_decode_text(tokens) -> str:
    """The text of a streaming recogniser's token strings (online.cpp online_decode_text): "</s>" ends it; a token that is all
    CJK (U+4E00 .. U+9FA5) is appended as it is, any other between two bars; "@@" in front of a bar joins the pieces, two bars
    become one space, ASCII letters are lowered."""
    text = ""
    for tk in tokens:
        if tk == "</s>":
            break
        if tk in _SILENT:
            continue
        text += tk if tk and all(0x4E00 <= ord(c) <= 0x9FA5 for c in tk) else _BAR + tk + _BAR
    text = text.replace("@@" + _BAR + _BAR, "").replace("@@" + _BAR, "").replace(_BAR + _BAR, " ").replace(_BAR, "")
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in text)


def committed_words(tokens):
    """(the committed words, the held-back word or None): the words of online_decode_text(tokens); while the last token that
    contributes text ends in "@@" the last word is held back, because the next piece changes it."""
    spoken = []
    for tk in tokens:
        if tk == "</s>":
            break
        if tk not in _SILENT:
            spoken.append(tk)
    words = R.split_words(online_decode_text(tokens))
    if spoken and spoken[-1].endswith("@@") and words:
        return words[:-1], words[-1]
    return words, None


def check_prefix(before, now):
    """The committed words of one call must be a prefix of the next call's."""
    return list(now[: len(before)]) == list(before)


CONTEXTS = [1, 2, 10, 11, 12, 31, 32, 33, 63, 64, 65, 129, 255, 256]


def deviation_and_margin(w, cfg, lengths=CONTEXTS):
    """Over the contexts window_ids(T, vocab, T), no restarts: (the largest |emulate_f16 - logits64|, the float64 top-2 margins
    of all positions)."""
    dev, margins = 0.0, []
    for T in lengths:
        ids = R.window_ids(T, int(cfg["vocab"]), T)
        z = logits64(w, cfg, ids)
        dev = max(dev, float(np.abs(emulate_f16(w, cfg, ids) - z).max()))
        s = np.sort(z, axis=1)
        margins.append(s[:, -1] - s[:, -2])
    return dev, np.concatenate(margins)
