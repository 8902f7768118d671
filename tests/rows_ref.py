"""Float64 definitions and derived error bounds for the row kernels — csrc/k_norm.hip (launch_layernorm, launch_posenc_ln_tab,
launch_layernorm_f16) and the non-CIF half of csrc/k_misc.hip (launch_fsmn_dec_stream, launch_embed_gather, launch_add_to_f16,
launch_seaco_merge) — and the inputs of the streaming-seam tests.  TEST INFRASTRUCTURE ONLY: tests/test_gpu_rows_conformance.py
and tests/test_gpu_online.py compare the device with what stands here, tests/test_rows_ref_cpu.py compares what stands here with
independent formulations (torch float64 layer_norm, the conv1d form of oracle/online.py, om.argmax_last) and shows that the
streaming cases tell a wrong cache rotation, a late mask and an unmasked cache from the right answer.

Guarded buffers.  Every pf_op_* of this suite returns its result between OP_GUARD_ROWS canary rows (and, where the row stride is
wider than the result, beside canary columns): body() cuts the result out, assert_guards() demands the canary everywhere else.

LayerNorm.  Definition gemm_ref.ln_ref, bound gemm_ref.ln_bound (its derivation stands there).  ln_bound is void for a row
whose offset dwarfs its spread (the A / s term), yet the kernels subtract the row's first element before anything else, and for
offset_rows() that difference is exact in fp32 (every element is C + 2 k with C an even integer in [2^24, 2^25), where fp32
counts in twos, and lies within a factor 2 of the first: Sterbenz).  LayerNorm is shift-invariant, so such a row is bound by
ln_bound(x - x0, g, b) around ln_ref(x - x0, g, b).  A constant row gives d = 0, mean 0, var 0, y = 0 * 1e6 * g + b = b: beta,
bit for bit.

Position encoding.  y = LN(fl32(fl32(x * s) + pe)), s = fl32(sqrt(512)), pe = oracle.model.sinusoidal_pe (positions 1 .. T).  The
float64 reference takes LN(x * s + pe) unrounded; the input then differs by the two fp32 roundings, 2^-24 (|x s| + |x s + pe|), and
by the engine's table against the oracle's: both form inv = exp(fl32(i * -inc)) and st = fl32(pos * inv) in fp32 from the same
argument, with exp and sin / cos from different libraries (each within an ulp): st differs by at most 3 ulps, 3 * 2^-23 st,
which sin and cos pass on at slope <= 1, plus an ulp of the result, 2^-23.  layer_ref.ln_input_bound turns that into a bound on the
normalised row, next to ln_bound for the kernel's own arithmetic.

Streaming FSMN (kernels.h, oracle/online.py:decoder).  xc[b, c, :] = [cache_in[b, c, :] | tn[b, l, c] * m_l], m_l = (l < len[b]):
    x[b, l, c] += sum_j taps[j, c] * xc[l + j] + tn[b, l, c]      for l < min(len[b], L)
    cache_out[b, c, :] = xc[L : L + K - 1]                          (a copy: bit-exact)
K products summed in order, the identity term, the add into x: each term meets at most K + 2 roundings, so
|err| <= (K + 2) 2^-24 (sum_j |w_j| |xc_{l+j}| + |tn_l| + |x_l|).

add_to_f16 is f16(fl32(a + b)): two roundings.  double_rounding_pairs() gives operands whose float64 sum, rounded to f16 at once,
lands on the other neighbour.

seaco_merge is an integer rule (merge_ref): a row is replaced iff some earlier entry is >= dha[nobias], or some later entry is >
it (together: the first-index arg-max is not nobias; a NaN elsewhere wins no comparison), or dha[nobias] is NaN, or nobias lies
outside [0, V).  embed_gather returns table rows, ids clamped to [0, vocab - 1]."""
import numpy as np

import gemm_ref as G
import layer_ref as LR

OP_GUARD_ROWS = 2
CANARY32 = 0x7FC5A5A5
CANARY16 = 0x7E5A
LOG = {}                                          # worst |err| / bound per kernel and output form (printed by the GPU suite)

ln_ref, ln_bound = G.ln_ref, G.ln_bound


def note(key, ratio):
    LOG[key] = max(LOG.get(key, 0.0), float(ratio))
    return ratio


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ guarded buffers
def body(buf, rows, cols=None):
    """the result inside a guarded buffer: rows [G, G + rows), columns [0, cols)"""
    assert buf.shape[0] == rows + 2 * OP_GUARD_ROWS, (buf.shape, rows)
    out = buf[OP_GUARD_ROWS: OP_GUARD_ROWS + rows]
    return out if cols is None or out.ndim == 1 else out[:, :cols]


def assert_guards(buf, rows, cols=None, what="", pad=None):
    """the canary in every guard row and, cols given, in columns [cols, ld) of the result rows (pad: the value those columns
    must hold instead, where the kernel defines one)"""
    canary = {2: CANARY16, 4: CANARY32, 8: (CANARY32 << 32) | CANARY32}[buf.dtype.itemsize]
    b = bits(buf)
    g = OP_GUARD_ROWS
    for name, part, r0 in (("front", b[:g], -g), ("back", b[g + rows:], rows)):
        bad = np.argwhere(part != canary)
        assert not len(bad), "%s: the %s guard was written at row %d%s" % (what, name, r0 + bad[0][0], " column %d" % bad[0][1] if b.ndim > 1 else "")
    assert b.shape[0] == rows + 2 * g
    if cols is not None and b.ndim > 1 and b.shape[1] > cols:
        side = b[g: g + rows, cols:]
        bad = np.argwhere(side != (canary if pad is None else pad))
        assert not len(bad), "%s: column %d of row %d holds 0x%X" % (what, cols + bad[0][1] if len(bad) else 0, bad[0][0] if len(bad) else 0,
                                                                     int(side[tuple(bad[0])]) if len(bad) else 0)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_params(D, seed):
    r = np.random.default_rng([seed, D, 1])
    return (1 + 0.1 * r.standard_normal(D)).astype(np.float32), (0.1 * r.standard_normal(D)).astype(np.float32)


def ln_rows(M, D, seed):
    """random rows with per-row gains 10^U(-1, 1) and offsets (the rows of the fp32 suite)"""
    r = np.random.default_rng([seed, M, D])
    return (r.standard_normal((M, D)) * 10.0 ** r.uniform(-1, 1, (M, 1)) + r.standard_normal((M, 1))).astype(np.float32)


def offset_rows(n, D, seed):
    """rows C + 2 k_i, C an even integer within 1.7e7 (1 +- 1e-3), k_i integers in [-40, 40]: exact in fp32, x - x[0] exact"""
    r = np.random.default_rng([seed, n, D, 2])
    C = 2 * np.round(1.7e7 * (1 + 1e-3 * r.uniform(-1, 1, (n, 1))) / 2)
    x = C + 2 * r.integers(-40, 41, (n, D))
    x32 = x.astype(np.float32)
    assert (x32.astype(np.float64) == x).all() and (x >= 2.0 ** 24).all() and (x < 2.0 ** 25).all()
    return x32


def ln_cases(rows, D, seed, specials=True):
    """x [rows, D] float32 and kind [rows] (0 random, 1 large offset, 2 constant): with `specials` two large-offset rows and one
    constant row lie among the last three rows (as many of them as there are rows)"""
    x = ln_rows(rows, D, seed)
    kind = np.zeros(rows, np.int32)
    if specials:
        off = offset_rows(2, D, seed)
        for i, (r, k) in enumerate(((rows - 1, 1), (rows - 2, 2), (rows - 3, 1))):
            if r < 0:
                break
            kind[r] = k
            x[r] = off[i // 2] if k == 1 else np.float32(-1.7e7 * (1 + 1e-3 * (seed % 7)))
    return x, kind


def ln_expect(x, kind, g, b, half):
    """(reference, bound) float64 [rows, D]; a constant row: reference fl(beta) (f16(beta) with half), bound 0"""
    x64 = np.asarray(x, np.float64)
    xs = np.where((kind == 1)[:, None], x64 - x64[:, :1], x64)          # exact in fp32 for the large-offset rows
    ref, bnd = ln_ref(xs, g, b), ln_bound(xs, g, b, half=half)
    const = kind == 2
    if const.any():
        assert (x64[const] == x64[const][:, :1]).all()
        beta = np.asarray(b, np.float32)
        ref[const] = (f16(beta) if half else beta).astype(np.float64)
        bnd[const] = 0.0
    return ref, bnd


def assert_ln(got, ref, bnd, what):
    """|got - ref| <= bnd (a zero bound: equality); returns the worst |err| / bound over the rows with a bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bnd)
    if bad.any():
        m, n = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements out of bound; first at (row %d, column %d): got %r, want %r, |err| %.3e > %.3e"
                             % (what, int(bad.sum()), bad.size, m, n, float(got[m, n]), float(ref[m, n]), float(err[m, n]), float(bnd[m, n])))
    live = bnd > 0
    return float((err[live] / bnd[live]).max()) if live.any() else 0.0


XSCALE = np.float32(np.sqrt(np.float32(512.0)))


def posenc_case(B, T, seed, F=560):
    """x [B, T, F]: per-frame gains 10^U(-2.5, 0.5), so that in some frames the table weighs as much as x * sqrt(512)"""
    r = np.random.default_rng([seed, B, T])
    return (r.standard_normal((B, T, F)) * 10.0 ** r.uniform(-2.5, 0.5, (B, T, 1))).astype(np.float32)


def posenc_expect(x, g, b, first_pos=1):
    """x [B, T, F] -> (reference, bound) [B T, F] of the f16 LayerNorm(x * sqrt(512) + PE(t + 1)) (module docstring);
    first_pos != 1 is the wrong answer of a table read one row off"""
    from oracle import model as om
    B, T, F = x.shape
    half = F // 2
    pe = om.sinusoidal_pe(T + first_pos - 1, F).numpy().astype(np.float64)[first_pos - 1:] if first_pos >= 1 else \
        np.concatenate([np.tile(np.r_[np.zeros(half), np.ones(half)], (1, 1)), om.sinusoidal_pe(T, F).numpy().astype(np.float64)])[:T]
    inc = np.float32(np.log(10000.0) / (half - 1))
    st = np.arange(1, T + 1, dtype=np.float64)[:, None] * np.exp(np.arange(half, dtype=np.float64) * -float(inc))[None, :]
    bpe = np.tile(3 * 2.0 ** -23 * st + 2.0 ** -23, (1, 2))
    xs = np.asarray(x, np.float64) * float(XSCALE)
    v = xs + pe[None]
    bx = (2.0 ** -24 * (np.abs(xs) + np.abs(v)) + bpe[None]).reshape(B * T, F)
    v = v.reshape(B * T, F)
    ref = ln_ref(v, g, b)
    lnb = ln_bound(v, g, b, half=True)
    return ref, lnb + (1 + 2.0 ** -10) * LR.ln_input_bound(v, bx, g)


# ------------------------------------------------------------------------------------------------ streaming FSMN
def fsmn_stream_ref(tn, taps, lens, cache_in, x):
    """-> x_out [B, L, D] float64, cache_out [B, D, K - 1] float32 (exact), bound [B, L, D] (0 on the rows that keep their bits)"""
    tn64, w, c64, x64 = (np.asarray(t, np.float64) for t in (tn, taps, cache_in, x))
    B, L, D = tn64.shape
    K = w.shape[0]
    n = np.minimum(np.maximum(np.asarray(lens), 0), L)
    m = (np.arange(L)[None, :] < n[:, None])
    xc = np.concatenate([c64, np.where(m[:, :, None], tn64, 0.0).transpose(0, 2, 1)], axis=2)   # [B, D, K - 1 + L]; masked: +0, not tn * 0
    out, bnd = x64.copy(), np.zeros_like(x64)
    for l in range(L):
        win = xc[:, :, l: l + K]                                                               # [B, D, K]
        y = (win * w.T[None]).sum(axis=2) + tn64[:, l]
        mag = (np.abs(win) * np.abs(w.T[None])).sum(axis=2) + np.abs(tn64[:, l]) + np.abs(x64[:, l])
        out[:, l] = np.where(m[:, l, None], x64[:, l] + y, x64[:, l])
        bnd[:, l] = np.where(m[:, l, None], (K + 2) * 2.0 ** -24 * mag, 0.0)
    return out, xc[:, :, L:].astype(np.float32), bnd


def fsmn_stream_case(B, L, k, lens, seed, zero_cache=False, D=512):
    r = np.random.default_rng([seed, B, L, k])
    tn = r.standard_normal((B, L, D)).astype(np.float32)
    x = r.standard_normal((B, L, D)).astype(np.float32)
    taps = (0.1 * r.standard_normal((k, D))).astype(np.float32)
    cache = np.zeros((B, D, k - 1), np.float32) if zero_cache else r.standard_normal((B, D, k - 1)).astype(np.float32)
    return tn, taps, np.asarray(lens, np.int32), cache, x


# ------------------------------------------------------------------------------------------------ add_to_f16, embed_gather
def add_to_f16_ref(a, b):
    return (np.asarray(a, np.float32) + np.asarray(b, np.float32)).astype(np.float32).astype(np.float16)


def double_rounding_pairs(n, seed):
    """(a, b) float32 [n]: a = +-2^e (1 + (2 q + 1) 2^-11) lies midway between two f16 neighbours, b = +-2^(e - 30) pushes the
    exact sum off the midpoint; fl32(a + b) == a, so the two-step result is the even neighbour whatever the sign of b, the
    one-step rounding of the float64 sum follows b"""
    r = np.random.default_rng([seed, n])
    e = r.integers(-8, 9, n)
    q = r.integers(0, 512, n)
    sa, sb = r.choice([-1.0, 1.0], n), r.choice([-1.0, 1.0], n)
    a = sa * np.ldexp(1 + (2 * q + 1) * 2.0 ** -11, e)
    b = sb * np.ldexp(1.0, e - 30)
    return a.astype(np.float32), b.astype(np.float32)


def embed_ref(table, ids):
    t = np.asarray(table, np.float32)
    rows = t[np.clip(np.asarray(ids, np.int64), 0, t.shape[0] - 1)]
    return rows, rows.astype(np.float16)


# ------------------------------------------------------------------------------------------------ seaco_merge
def merge_replace(dha, V, nobias):
    """bool [rows]: the rule of the module docstring, comparison by comparison"""
    x = np.asarray(dha, np.float32)[:, :V]
    if not 0 <= nobias < V:
        return np.ones(x.shape[0], bool)
    ref = x[:, nobias: nobias + 1]
    with np.errstate(invalid="ignore"):
        return (x[:, :nobias] >= ref).any(axis=1) | (x[:, nobias + 1:] > ref).any(axis=1) | np.isnan(ref[:, 0])


def merge_ref(dha, dha_ids, V, nobias, copy_logits, logits, ids):
    """-> (logits, ids) after the merge, every other cell with the bits it had"""
    lo, io = np.array(logits, np.float32, copy=True), np.array(ids, np.int64, copy=True)
    rep = merge_replace(dha, V, nobias)
    io[rep] = np.asarray(dha_ids, np.int64)[rep]
    if copy_logits:
        lo[rep, :V] = np.asarray(dha, np.float32)[rep, :V]
    return lo, io


MERGE_CLASSES = ("unique", "tie_before", "tie_after", "bigger_last", "bigger_pad", "nan_nobias", "nan_elsewhere", "bigger_first")


def merge_case(V, nobias, seed):
    """steered rows for one (V, nobias): dict(dha [rows, ld], ld, cls [rows], want [rows] bool — None where (V, nobias) leaves the
    class no room and the row is an unsteered random one).  ld = round_up(V, 4) + 4; dha[r, nobias] = 1 is the reference value,
    everything else in [0, 0.9) unless the class says otherwise; the pad columns [V, ld) hold 0.5 except in bigger_pad."""
    ld = (V + 3) // 4 * 4 + 4
    r = np.random.default_rng([seed, V, nobias + 7])
    inside = 0 <= nobias < V
    rows = []
    for cls in MERGE_CLASSES:
        for rep in range(2):
            x = np.full(ld, 0.5, np.float32)
            x[:V] = r.uniform(0, 0.9, V).astype(np.float32)
            want = not inside
            if inside:
                x[nobias] = 1.0
                before = np.arange(0, nobias)
                after = np.arange(nobias + 1, V)
                pick = lambda idx: int(idx[0] if rep == 0 else idx[-1])
                if cls == "unique":
                    want = False
                elif cls == "tie_before":
                    want = None
                    if len(before):
                        x[pick(before)] = 1.0; want = True
                elif cls == "tie_after":
                    want = None
                    if len(after):
                        x[pick(after)] = 1.0; want = False
                elif cls == "bigger_last":
                    want = None
                    if nobias != V - 1:
                        x[V - 1] = 2.0; want = True
                elif cls == "bigger_pad":
                    x[V:] = 3.0 if rep == 0 else np.inf; want = False
                elif cls == "nan_nobias":
                    x[nobias] = np.nan; want = True
                elif cls == "nan_elsewhere":
                    want = None
                    other = before if (rep == 0 and len(before)) else after
                    if len(other):
                        x[pick(other)] = np.nan; want = False
                elif cls == "bigger_first":
                    want = None
                    if nobias != 0:
                        x[0] = 1.0 + 2.0 ** -23; want = True
            rows.append((cls, x, want))
    dha = np.stack([x for _, x, _ in rows])
    rule = merge_replace(dha, V, nobias)
    want = np.asarray([rule[i] if w is None else w for i, (_, _, w) in enumerate(rows)], bool)
    return dict(dha=dha, ld=ld, cls=[c for c, _, _ in rows], want=want, steered=np.asarray([w is not None for _, _, w in rows], bool))


# ------------------------------------------------------------------------------------------------ streaming seams
ONLINE_TOL = dict(act=1e-2, alphas=3e-3, logp=2e-2, cache=1e-2)      # the header of tests/test_gpu_online.py
CACHE_GAIN = 1.0
# (L, lens): B = 3, ragged with a 0; the last: nobody has a token.  The FSMN looks back only (xc[l .. l + 10] = positions l - 10 .. l),
# so a mask that ends one position late shows in the compared quantities only through the cache, i.e. where len >= L - 10:
# with lens (25, 7, 0) it moved nothing at all (tests/test_rows_ref_cpu.py), hence the 18.
DEC_CASES = (
    (1, (1, 0, 1)), (10, (10, 4, 0)), (11, (11, 3, 0)), (25, (25, 18, 0)), (4, (0, 0, 0)))
MUTATIONS = ("rotate", "late_mask", "unmasked_cache")


def online_decoder_inputs(L, lens, n_layers, seed=17, gain=CACHE_GAIN, D=512):
    r = np.random.default_rng([seed, L, n_layers])
    B = len(lens)
    emb = r.standard_normal((B, L, D)).astype(np.float32)
    for b in range(B):
        emb[b, lens[b]:] = 0
    caches = [(gain * r.standard_normal((B, D, 10))).astype(np.float32) for _ in range(n_layers)]
    return emb, np.asarray(lens, np.int32), caches


def online_decoder(g, enc, embeds, lens, caches, mutation=None):
    """oracle.online.OnlineGraphs.decoder restated with its FSMN seam open: mutation None is that function, bit for bit;
    "rotate" reads the cache rotated by one column, "late_mask" masks from position len + 1 on, "unmasked_cache" takes the new
    cache from the unmasked tn."""
    import torch
    import torch.nn.functional as Fn
    from oracle import model as om
    o, c = g.o, g.o.cfg
    q = o.q
    memory = torch.as_tensor(enc, dtype=torch.float32)
    x = torch.as_tensor(embeds, dtype=torch.float32)
    B, L, D = x.shape
    ln = torch.as_tensor(np.asarray(lens), dtype=torch.int64)
    if mutation == "late_mask":
        ln = ln + 1
    mask = (torch.arange(L)[None, :] < ln[:, None]).to(torch.float32).unsqueeze(-1)
    dk = D // c.heads
    new_caches = []
    for i in range(c.dec_layers):
        p = f"decoder.layers.{i}"
        t = o.ffn_dec(o.ln(x, p + ".norm1"), p)
        raw = o.ln(t, p + ".norm2")
        tn = raw * mask
        cin = torch.as_tensor(caches[i], dtype=torch.float32)
        if mutation == "rotate":
            cin = torch.roll(cin, 1, dims=2)
        xc = torch.cat([cin, tn.transpose(1, 2)], dim=2)
        src = torch.cat([cin, raw.transpose(1, 2)], dim=2) if mutation == "unmasked_cache" else xc
        new_caches.append(src[:, :, -(c.kernel - 1):].numpy().copy())
        y = Fn.conv1d(xc, o.w[p + ".fsmn.weight"].unsqueeze(1), groups=D).transpose(1, 2)
        x = x + (y + tn) * mask
        xn = o.ln(x, p + ".norm3")
        qq = o.lin(xn, p + ".src.q")
        kv = o.lin(memory, p + ".src.kv")
        k, v = torch.split(kv, D, dim=-1)
        x = x + o.lin(o.mha(q(qq * (dk ** -0.5)), q(k), q(v)), p + ".src.out")
    x = o.ffn_dec(o.ln(x, "decoder.final.norm1"), "decoder.final")
    hid = o.ln(x, "decoder.after_norm")
    return om.log_softmax(o.lin(hid, "decoder.output")).numpy(), new_caches


def separation(ref, mut, lens):
    """how far a mutated answer lies from the right one in the quantities the seam test compares, in units of their tolerances:
    log-probs on the valid positions, every layer's cache"""
    (lp, c), (lpm, cm) = ref, mut
    L = lp.shape[1]
    valid = np.arange(L)[None, :] < np.asarray(lens)[:, None]
    d = [np.abs(a - b).max() / ONLINE_TOL["cache"] for a, b in zip(c, cm)]
    if valid.any():
        d.append(np.abs(lp - lpm)[valid].max() / ONLINE_TOL["logp"])
    return float(max(d))
