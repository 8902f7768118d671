"""The definition of neural LM rescoring (paraformer_hip.h "Neural LM rescoring") in numpy float64: the causal
Transformer LM on one hypothesis, the LM sum, and the fusion into an n-best list.  The host twin (csrc/nnlm.cpp) and the device
form (csrc/k_nnlm.hip) are tested against this file; it shares no code with either.

The network is ESPnet's TransformerLM restated from memory; no ESPnet code and no released model file was at hand.
`emulate_f16` is the same network with the device form's stated rounding points (the head of k_nnlm.hip) and float64
everywhere else: its distance from `logp64` is what the f16 operands cost, and the GPU test's tolerance is 4 x that distance."""
import numpy as np

LN_EPS = 1e-12
MAX_TOKENS = 255


def _h(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def _ident(x):
    return np.asarray(x, dtype=np.float64)


def _ln(x, g, b):
    mu = x.mean(axis=-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + LN_EPS) * g.astype(np.float64) + b.astype(np.float64)


def rows_of(ids, V):
    """(input rows [sos, y_1 .. y_n], targets [y_1 .. y_n, eos]); sos = eos = V - 1"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    assert len(ids) <= MAX_TOKENS and ((ids >= 0) & (ids < V)).all()
    return np.concatenate([[V - 1], ids]), np.concatenate([ids, [V - 1]])


def _network(w, cfg, ids, q):
    """q: the rounding applied at the device form's rounding points (identity: the definition).  logp [n + 1] float64."""
    V, D, H, NL = (int(cfg[k]) for k in ("vocab", "d_model", "heads", "n_layers"))
    inp, tgt = rows_of(ids, V)
    T, dh = len(inp), D // H
    lin = lambda x, name: x @ q(w[name + ".weight"]).T + w[name + ".bias"].astype(np.float64)
    x = np.maximum(_ln(lin(q(w["embed.weight"])[inp], "input.linear"), w["input.norm.weight"], w["input.norm.bias"]), 0.0)
    causal = np.tril(np.ones((T, T), bool))
    for l in range(NL):
        p = "layers.%d." % l
        qkv = lin(q(_ln(x, w[p + "norm1.weight"], w[p + "norm1.bias"])), p + "attn.qkv")
        qh, kh, vh = q(qkv[:, :D] * dh ** -0.5), q(qkv[:, D:2 * D]), q(qkv[:, 2 * D:])
        ctx = np.zeros((T, D))
        for h in range(H):
            c = slice(h * dh, (h + 1) * dh)
            s = np.where(causal, qh[:, c] @ kh[:, c].T, -np.inf)
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            ctx[:, c] = (q(e) @ vh[:, c]) / e.sum(axis=-1, keepdims=True)
        x = x + lin(q(ctx), p + "attn.out")
        hid = q(np.maximum(lin(q(_ln(x, w[p + "norm2.weight"], w[p + "norm2.bias"])), p + "ffn.w1"), 0.0))
        x = x + lin(hid, p + "ffn.w2")
    z = lin(q(_ln(x, w["after_norm.weight"], w["after_norm.bias"])), "decoder")
    mx = z.max(axis=-1)
    return z[np.arange(T), tgt] - (mx + np.log(np.exp(z - mx[:, None]).sum(axis=-1)))


def logp64(w, cfg, ids) -> np.ndarray:
    """logp[t] = log P(target_t | input_0 .. t) of one hypothesis: [n + 1] float64."""
    return _network(w, cfg, ids, _ident)


def emulate_f16(w, cfg, ids) -> np.ndarray:
    """The same with the device form's rounding points R0, R0e, R1 .. R5 (k_nnlm.hip) and float64 elsewhere."""
    return _network(w, cfg, ids, _h)


def lm_sum(logp, eos: bool) -> float:
    """logp[0 .. n - 1], plus the eos row logp[n] iff eos"""
    return float(np.sum(logp[:-1]) + (logp[-1] if eos else 0.0))


def lm_sum_f32(logp, eos: bool) -> np.float32:
    """the sequential float32 sum the device takes"""
    s = np.float32(0.0)
    for v in np.asarray(logp, np.float32)[: len(logp) - (0 if eos else 1)]:
        s = np.float32(s + v)
    return s


def fuse(base, lm, n_tokens, weight, bonus):
    """(score' = base + weight * lm_sum + bonus * n, the stable order by score' descending)"""
    score = np.asarray(base, np.float64) + weight * np.asarray(lm, np.float64) + bonus * np.asarray(n_tokens, np.float64)
    return score, np.argsort(-score, kind="stable").astype(np.int32)


# the hypothesis lengths of the GPU test: the 32-row tile edges, the 64-query tile edges and the cap
LENGTHS = [0, 1, 2, 30, 31, 32, 62, 63, 64, 65, 127, 128, 254, 255]


def hyp_ids(n: int, V: int, seed: int) -> np.ndarray:
    """A seeded hypothesis of n ids in [0, V); from n = 4 on its first ids are 0, 31, 32 and V - 1: the targets at the first
    and last channel of the decoder's first block, the first of its second, and the last of the vocabulary."""
    ids = np.random.default_rng(2000 + seed).integers(0, V, size=n).astype(np.int32)
    if n >= 4:
        ids[:4] = [0, min(31, V - 1), min(32, V - 1), V - 1]
    return ids


def deviation(w, cfg, lengths=LENGTHS):
    """Over the hypotheses hyp_ids(n, V, n): (the largest |emulate_f16 - logp64| over all rows, the float64 logp per hypothesis)."""
    dev, zs = 0.0, []
    for n in lengths:
        ids = hyp_ids(n, int(cfg["vocab"]), n)
        z = logp64(w, cfg, ids)
        zs.append(z)
        dev = max(dev, float(np.abs(emulate_f16(w, cfg, ids) - z).max()))
    return dev, zs


# the GPU test's models: released d_model / heads / ffn / embed, one decoder block plus one channel and a ragged last block
GPU_CASES = [(33, 1), (33, 2), (100, 1), (100, 2)]


def gpu_case(V, n_layers):
    from aliparaformerasr_amd import weights as W
    cfg = W.transformer_lm_config(vocab=V, n_layers=n_layers)
    return cfg, W.synth_nnlm_weights(cfg, seed=5)


# the n-best lists of the ranking test: LISTS lists of LIST_N hypotheses of 3 .. 12 tokens, acoustic scores N(0, 8)
LISTS, LIST_N, WEIGHT, BONUS = 12, 6, 0.5, 0.1


def ranking_lists(V: int):
    """[(hypotheses, base scores float64)] with fixed seeds"""
    rng = np.random.default_rng(77)
    out = []
    for i in range(LISTS):
        hyps = [hyp_ids(int(rng.integers(3, 13)), V, 500 + LIST_N * i + j) for j in range(LIST_N)]
        out.append((hyps, 8.0 * rng.standard_normal(LIST_N)))
    return out


def unsafe_pairs(score, order, n_tokens, dev, weight=WEIGHT):
    """of the adjacent pairs of a fused list (in its order): True where the float64 scores lie within
    2 * weight * (n + 1) * 4 * dev of each other (n: the longer of the two), so the f16 form may order them either way"""
    a, b = order[:-1], order[1:]
    n = np.maximum(np.asarray(n_tokens)[a], np.asarray(n_tokens)[b])
    return np.abs(score[a] - score[b]) <= 2 * weight * (n + 1) * 4 * dev
