"""The definition of the punctuation feature (paraformer_hip.h "Punctuation") in numpy float64: the word
split, the CT-Transformer network, the cut rule, the text loop and the assembly of the output text.  The host twins
(csrc/punc.cpp) and the device form (csrc/k_punc.hip) are tested against this file; it shares no code with either.

The text rules are this project's definition, restated from FunASR's CTTransformer.inference from memory; no FunASR code and
no released model file was at hand.  `emulate_f16` is the same network with the device form's stated rounding points (the
head of k_punc.hip) and float64 everywhere else: its distance from `logits64` is what the f16 operands cost, and the GPU
test's tolerance is 4 x that distance."""
import math

import numpy as np

MINI = 20
COMMA_WINDOW = 200
HARD_WINDOW = 492
MAX_WINDOW = 512
LN_EPS = 1e-12
F32 = np.float32
_WS = b" \t\n\v\f\r"


def split_words(text: str) -> list:
    """Split at ASCII whitespace; inside a piece every character longer than one byte in UTF-8 is a word of its own and every
    maximal run of one-byte characters is one word."""
    out, run = [], ""
    for ch in text:
        one = len(ch.encode("utf-8")) == 1
        if one and ch.encode("utf-8") in _WS:
            if run:
                out.append(run)
            run = ""
        elif one:
            run += ch
        else:
            if run:
                out.append(run)
            run = ""
            out.append(ch)
    if run:
        out.append(run)
    return out


def word_ids(words, vocab) -> np.ndarray:
    index = {w: i for i, w in enumerate(vocab)}
    unk = index["<unk>"]
    return np.array([index.get(w, unk) for w in words], dtype=np.int32)


def sinusoidal_pe(T: int, depth: int) -> np.ndarray:
    """oracle/model.py sinusoidal_pe: positions 1 .. T, [sin || cos], in its float32 steps, with ONE difference: exp, sin and
    cos are evaluated in float64 on the float32 argument and rounded once.  numpy's float32 forms of these functions are
    vectorised per CPU and differ from host to host in the last bit (on the machine this was written on in 9 % of the
    entries), which a definition that is compared bit for bit cannot inherit."""
    half = depth // 2
    inc = F32(math.log(10000.0) / (half - 1))
    inv = np.exp((np.arange(half, dtype=F32) * (-inc)).astype(F32).astype(np.float64)).astype(F32)
    pos = np.arange(1, T + 1, dtype=F32)
    st = (pos[:, None] * inv[None, :]).astype(F32).astype(np.float64)
    return np.concatenate([np.sin(st), np.cos(st)], axis=1).astype(F32)


def layer0_input(w, cfg, ids, embed=None) -> np.ndarray:
    """fp32(embed[id]) * sqrt(d_model), then + pe: two float32 roundings.  embed: the table to gather from (default: as given)."""
    D = int(cfg["d_model"])
    e = (w["embed.weight"] if embed is None else embed).astype(F32)
    ids = np.asarray(ids, dtype=np.int64)
    x = (e[ids] * F32(math.sqrt(D))).astype(F32)
    return (x + sinusoidal_pe(len(ids), D)).astype(F32)


def _h(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def _ident(x):
    return np.asarray(x, dtype=np.float64)


def _ln(x, g, b):
    mu = x.mean(axis=-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + LN_EPS) * g.astype(np.float64) + b.astype(np.float64)


def _network(w, cfg, ids, q):
    """q: the rounding applied at the device form's rounding points (identity: the definition)."""
    D, H, K, NL = (int(cfg[k]) for k in ("d_model", "heads", "kernel", "n_layers"))
    T = len(ids)
    P = int(cfg["n_punc"])
    if T == 0:
        return np.zeros((0, P), np.float64)
    dh, left = D // H, (K - 1) // 2
    lin = lambda x, name: x @ q(w[name + ".weight"]).T + w[name + ".bias"].astype(np.float64)
    x = layer0_input(w, cfg, ids, embed=q(w["embed.weight"])).astype(np.float64)
    for l in range(NL):
        p = "layers.%d." % l
        xn = q(_ln(x, w[p + "norm1.weight"], w[p + "norm1.bias"]))
        qkv = lin(xn, p + "attn.qkv")
        qh, kh, vh = q(qkv[:, :D] * dh ** -0.5), q(qkv[:, D:2 * D]), q(qkv[:, 2 * D:])
        taps = w[p + "attn.fsmn.weight"].astype(np.float64)                      # [D, K]
        vp = np.concatenate([np.zeros((left, D)), vh, np.zeros((K - 1 - left, D))], axis=0)
        f = vh.copy()
        for j in range(K):
            f += taps[:, j][None, :] * vp[j: j + T]
        ctx = np.zeros((T, D))
        for h in range(H):
            s = qh[:, h * dh:(h + 1) * dh] @ kh[:, h * dh:(h + 1) * dh].T
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            ctx[:, h * dh:(h + 1) * dh] = (q(e) @ vh[:, h * dh:(h + 1) * dh]) / e.sum(axis=-1, keepdims=True)
        x = x + (lin(q(ctx), p + "attn.out") + f)
        xn = q(_ln(x, w[p + "norm2.weight"], w[p + "norm2.bias"]))
        hid = q(np.maximum(lin(xn, p + "ffn.w1"), 0.0))
        x = x + lin(hid, p + "ffn.w2")
    xn = q(_ln(x, w["after_norm.weight"], w["after_norm.bias"]))
    return lin(xn, "decoder")


def logits64(w, cfg, ids) -> np.ndarray:
    """The network of the definition on one window: [T, n_punc] float64."""
    return _network(w, cfg, ids, _ident)


def emulate_f16(w, cfg, ids) -> np.ndarray:
    """The same with the device form's rounding points R0, R0e, R1 .. R5 (k_punc.hip) and float64 elsewhere."""
    return _network(w, cfg, ids, _h)


def argmax_ties_larger(z) -> np.ndarray:
    z = np.asarray(z)
    if z.shape[0] == 0:
        return np.zeros(0, np.int32)
    P = z.shape[1]
    return (P - 1 - np.argmax(z[:, ::-1], axis=1)).astype(np.int32)


def punc_index(punc_list) -> dict:
    g = lambda s: punc_list.index(s) if s in punc_list else -1
    return dict(unk=g("<unk>"), none=g("_"), comma=g("，"), period=g("。"), question=g("？"), pause=g("、"))


def cut_rule(p, last: bool, punc_list, sentence_end_id: int):
    """Steps 3 - 7 of the text loop and the last-window edits on one window's p: (cut, the edited p)."""
    ix = punc_index(punc_list)
    p = np.array(p, dtype=np.int32)
    n = len(p)
    if n == 0:
        return -1, p
    if last:
        if p[-1] in (ix["none"], ix["comma"], ix["pause"]) and p[-1] >= 0:
            p[-1] = sentence_end_id
        return n - 1, p
    cut, comma = -1, -1
    for i in range(n - 2, 1, -1):
        if p[i] >= 0 and p[i] in (ix["period"], ix["question"]):
            cut = i
            break
        if comma < 0 and p[i] == ix["comma"]:
            comma = i
    by_comma = cut < 0 and n > COMMA_WINDOW and comma >= 0
    if by_comma:
        cut = comma
    # the hard cut: no cut, or a tail behind the cut that is longer than HARD_WINDOW (such a tail plus the next mini-sentence
    # would pass MAX_WINDOW, which the hard cut exists to prevent)
    if n > HARD_WINDOW and (cut < 0 or n - 1 - cut > HARD_WINDOW):
        return n - 1, p
    if by_comma:
        p[cut] = sentence_end_id
    return cut, p


def text_loop(ids, forward, punc_list, sentence_end_id: int):
    """The loop over one text.  forward(window ids) -> p [n].  Returns (punc_ids [n], [(window ids, p after edits, cut)])."""
    ids = np.asarray(ids, dtype=np.int32)
    out, log, cache = [], [], np.zeros(0, np.int32)
    n_mini = (len(ids) + MINI - 1) // MINI
    for m in range(n_mini):
        win = np.concatenate([cache, ids[m * MINI:(m + 1) * MINI]])
        assert len(win) <= MAX_WINDOW
        cut, p = cut_rule(forward(win), m == n_mini - 1, punc_list, sentence_end_id)
        log.append((win, p, cut))
        out.extend(p[: cut + 1].tolist())
        cache = win[cut + 1:]
    return np.array(out, dtype=np.int32), log


def assemble(words, punc_ids, punc_list):
    """(the output text, [one past the last word of each sentence])."""
    ix = punc_index(punc_list)
    ascii_marks = {ix["comma"]: ",", ix["period"]: ".", ix["question"]: "?", ix["pause"]: ","}
    ascii_marks.pop(-1, None)
    one = lambda w: len(w[0].encode("utf-8")) == 1
    s, sent = "", []
    for i, wd in enumerate(words):
        if i > 0 and one(wd) and one(words[i - 1]):
            s += " "
        s += wd
        p = int(punc_ids[i])
        if p not in (ix["none"], ix["unk"]):
            s += ascii_marks[p] if (one(wd) and p in ascii_marks) else punc_list[p]
        if (p >= 0 and p in (ix["period"], ix["question"])) or i + 1 == len(words):
            sent.append(i + 1)
    return s, sent


def vocab_of(w) -> list:
    return bytes(np.asarray(w["vocab"], dtype=np.uint8)).decode("utf-8").split("\n")


def window_ids(T: int, vocab: int, seed: int) -> np.ndarray:
    """A seeded window of T ids in [0, vocab)."""
    return np.random.default_rng(1000 + seed).integers(0, vocab, size=T).astype(np.int32)


# the window lengths of the GPU test: every tile edge of the row kernel (64) and of the attention kernel (32 keys, 64 queries),
# lengths around the FSMN reach (5 taps each side at kernel 11) and the largest window
LENGTHS = [0, 1, 2, 5, 6, 10, 11, 12, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512]


def deviation_and_margin(w, cfg, lengths=LENGTHS):
    """Over the windows window_ids(T, vocab, T): (the largest |emulate_f16 - logits64|, the float64 top-2 margins of all
    positions, the float64 logits per window)."""
    dev, margins, zs = 0.0, [], []
    for T in lengths:
        ids = window_ids(T, int(cfg["vocab"]), T)
        z = logits64(w, cfg, ids)
        zs.append(z)
        if T:
            dev = max(dev, float(np.abs(emulate_f16(w, cfg, ids) - z).max()))
            s = np.sort(z, axis=1)
            margins.append(s[:, -1] - s[:, -2])
    return dev, np.concatenate(margins), zs


def punctuate(text, vocab, forward, punc_list, sentence_end_id):
    words = split_words(text)
    p, _ = text_loop(word_ids(words, vocab), forward, punc_list, sentence_end_id)
    return assemble(words, p, punc_list) + (p,)
