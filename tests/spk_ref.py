"""The definition of the speaker labels, numpy float64: the CAM++ embedding network on a window of fbank
rows, the window plan, the affinity, the clustering, the segment labels and the centroids.  csrc/k_spk.hip, csrc/spk.cpp and
the header section "Speaker labels" are held against this file.

Stated from memory of 3D-Speaker's CAMPPlus (speech_campplus_sv_zh-cn_16k-common, 192-d); no dimension, threshold or
front-end detail is validated on a real model.  Every BatchNorm that can be folded is folded at convert time (see
weights.spk_tensor_shapes for the container's tensors).

emulate_f16 is `forward(..., f16=True)`: the device's rounding points, everything else fp32 or better:
  R0 every product's weights, once, at attach time        R5 the bottleneck tile b = ReLU(W1 h + c1)
  R1 the input x - mean_t x                               R6 the context mean_t b + segment mean of b
  R2 every head convolution's output (after the ReLU)     R7 the mask's hidden layer ReLU(W2 c + b2)
  R3 the TDNN's output                                    R8 a dense layer's output local * mask
  R4 h = ReLU(s X + b) in front of a dense layer's        R9 a transit's output
     bottleneck product and in front of a transit         R10 the pooled statistics in front of the embedding product
The frames (the last ReLU(BN)) and the embedding are fp32.
"""
import numpy as np

from aliparaformerasr_amd import weights as W

SMALL = dict(n_mels=16, m_channels=8, init_channels=24, growth=8, bn_channels=12, blocks=(2, 3, 2), dilations=(1, 2, 2), seg_len=5,
             embedding=20)
MAX_FRAMES = 512               # PF_SPK_MAX_FRAMES
MAX_WINDOWS = 8192             # PF_SPK_MAX_WINDOWS
DEFAULTS = dict(win=150, shift=75, min_frames=20, threshold=0.5, num_speakers=0, min_cluster=4)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _relu(v):
    return np.where(v < 0, 0.0, v)                   # keeps a NaN


def _conv3x3(x, w, sf):
    """x [C, F, T], w [O, C, 3, 3] (frequency, time), pad 1, stride (sf, 1) -> [O, ceil(F / sf), T]"""
    C, F, T = x.shape
    Fo = (F + sf - 1) // sf
    xp = np.zeros((C, F + 2, T + 2))
    xp[:, 1:-1, 1:-1] = x
    cols = np.empty((C, 3, 3, Fo, T))
    for df in range(3):
        for dt in range(3):
            cols[:, df, dt] = xp[:, df:df + sf * (Fo - 1) + 1:sf, dt:dt + T]
    return np.tensordot(w, cols, axes=([1, 2, 3], [0, 1, 2]))


def frames_out_channels(cfg):
    return W.spk_channel_plan(cfg)[-1][1] // 2


def forward(cfg, w, rows, f16=False, trace=None):
    """One window: rows [T, n_mels] fp32 -> {"frames": [ceil(T / 2), C] (the last ReLU(BN), in front of the pooling),
    "emb": [embedding]}.  f16: with the device's rounding points.  trace (a dict, with f16): "worst" the largest magnitude that
    met a float16 rounding, "lossless" whether every such rounding changed nothing; R6, R7 and R10 are left out of both: a mean
    over 3 or 5 frames is no dyadic number; exact_model keeps the mask independent of them, and R10 lies behind the frames."""
    x = np.asarray(rows, np.float32).astype(np.float64)
    T, E = x.shape[0], int(cfg["embedding"])
    m, g, S = int(cfg["m_channels"]), int(cfg["growth"]), int(cfg["seg_len"])
    assert x.shape[1] == int(cfg["n_mels"]) and x.shape[1] % 8 == 0
    if T == 0:
        return {"frames": np.zeros((0, frames_out_channels(cfg))), "emb": np.zeros(E)}
    r32 = _f32 if f16 else (lambda a: a)

    def q(a, traced=True):
        if not f16:
            return a
        a = np.asarray(a, np.float64)
        with np.errstate(over="ignore"):
            b = a.astype(np.float32).astype(np.float16).astype(np.float64)
        if trace is not None and traced:
            fin = a[np.isfinite(a)]
            trace["worst"] = max(trace.get("worst", 0.0), float(np.abs(fin).max()) if fin.size else 0.0)
            trace["lossless"] = trace.get("lossless", True) and bool(np.array_equal(a, b, equal_nan=True))
        return b

    def Wt(n):
        a = w[n].astype(np.float64)
        return a.astype(np.float16).astype(np.float64) if f16 else a          # R0 (fp32 -> f16)

    def Bv(n):
        return w[n].astype(np.float64)

    def conv(a, n, sf):
        return _conv3x3(a, Wt(n + ".weight"), sf) + Bv(n + ".bias")[:, None, None]

    a = q(r32(x - r32(x.mean(axis=0)))).T[None]                            # R1; the image [1, F, T]
    a = q(_relu(conv(a, "head.conv1", 1)))                                  # R2, here and below
    for layer in (1, 2):
        p = "head.layer%d." % layer
        y = q(_relu(conv(a, p + "0.conv1", 2)))
        sc = np.tensordot(Wt(p + "0.shortcut.weight")[:, :, 0, 0], a[:, ::2, :], axes=(1, 0)) + Bv(p + "0.shortcut.bias")[:, None, None]
        a = q(_relu(conv(y, p + "0.conv2", 1) + sc))
        y = q(_relu(conv(a, p + "1.conv1", 1)))
        a = q(_relu(conv(y, p + "1.conv2", 1) + a))
    a = q(_relu(conv(a, "head.conv2", 2)))                                  # [m, F / 8, T]
    fr = a.reshape(m * a.shape[1], T).T                                     # frames of channel c * (F / 8) + f

    Tp = (T + 1) // 2
    wt = Wt("tdnn.weight")
    frp = np.zeros((T + 4, fr.shape[1]))
    frp[2:T + 2] = fr
    X = sum(frp[k:k + 2 * Tp:2] @ wt[:, :, k].T for k in range(5)) + Bv("tdnn.bias")
    X = q(_relu(X))                                                         # R3
    seg_of = np.arange(Tp) // S
    for b, n in enumerate(cfg["blocks"]):
        d = int(cfg["dilations"][b])
        for l in range(int(n)):
            p = "block%d.%d." % (b + 1, l)
            h = q(_relu(r32(X * Bv(p + "bn1.scale") + Bv(p + "bn1.shift"))))                    # R4
            bt = q(_relu(h @ Wt(p + "linear1.weight").T + Bv(p + "linear1.bias")))              # R5
            bp = np.zeros((Tp + 2 * d, bt.shape[1]))
            bp[d:d + Tp] = bt
            wl = Wt(p + "local.weight")
            local = sum(bp[k * d:k * d + Tp] @ wl[:, :, k].T for k in range(3))
            tot = r32(bt.mean(axis=0))
            ctx = np.stack([q(r32(tot + r32(bt[s0:min(s0 + S, Tp)].mean(axis=0))), False) for s0 in range(0, Tp, S)])   # R6
            hid = q(_relu(ctx @ Wt(p + "cam1.weight").T + Bv(p + "cam1.bias")), False)         # R7
            z = r32(hid @ Wt(p + "cam2.weight").T + Bv(p + "cam2.bias"))
            with np.errstate(over="ignore"):
                mask = r32(1.0 / (1.0 + np.exp(-z)))
            if trace is not None:
                trace.setdefault("ctx", {})[p] = ctx
                trace["mask_exact"] = trace.get("mask_exact", True) and bool(np.isin(mask, (0.0, 0.5, 1.0)).all() and
                                                                             ((z <= -1000) | (z == 0) | (z >= 64)).all())
                trace["mask_varies"] = trace.get("mask_varies", False) or bool((mask != mask[:1]).any())
            X = np.concatenate([X, q(r32(local) * mask[seg_of])], axis=1)                       # R8
        p = "transit%d." % (b + 1)
        h = q(_relu(r32(X * Bv(p + "bn.scale") + Bv(p + "bn.shift"))))                          # R4
        X = q(h @ Wt(p + "weight").T)                                                           # R9
    frames = r32(_relu(r32(X * Bv("out_bn.scale") + Bv("out_bn.shift"))))
    mean = r32(frames.mean(axis=0))
    std = np.zeros_like(mean) if Tp == 1 else r32(np.sqrt(r32(((frames - mean) ** 2).sum(axis=0) / (Tp - 1))))
    emb = r32(q(np.concatenate([mean, std]), False) @ Wt("dense.weight").T + Bv("dense.bias"))        # R10
    return {"frames": frames, "emb": emb}


def emulate_f16(cfg, w, rows, trace=None):
    return forward(cfg, w, rows, f16=True, trace=trace)


# ---- models and inputs for the tests --------------------------------------------------------------------------------------
def config(base=None):
    return W.campplus_config(**(base or {}))


def random_model(base=None, seed=1):
    cfg = config(base)
    return cfg, W.synth_spk_weights(cfg, seed)


def fbank_like(T, n_mels, seed):
    """rows like the engine's log-mel output: about N(6, 3), slowly varying in time"""
    rng = np.random.default_rng(seed)
    a = 6.0 + 2.0 * rng.standard_normal((1, n_mels)) + 2.0 * rng.standard_normal((T, n_mels))
    return a.astype(np.float32)


def exact_model(base=None, seed=1, segment_mask=False):
    """Weights on which no rounding loses anything (see exact_premise): sparse, in {0, +-1} (+-1/2 as well in head.conv1, whose
    input is integral), biases and shifts in {0, 1}, scales in {1, -1}; the mask's second product is zero and its bias is 0 on
    a layer's first channel (sigmoid = 1/2 exactly) and +64 elsewhere (1 exactly in fp32 AND in float64: at +32 the float64
    sigmoid is 1 - 1.3e-14, which a later ReLU(x - x') can turn into a difference that fp32 does not have); a later layer of the same block does
    not read a halved channel, so that the halvings do not compound beyond one per block.
    segment_mask: in the last layer of every block the upper half of the channels gets a mask that DEPENDS ON THE SEGMENT and is
    still exact: hidden unit j is ReLU(64 (c[k_j] - theta_j)) with theta_j an eighth of a float16 step above a float16 number (in the middle
    of what column k_j takes over the segments of a probe window), so
    the float16 context gives either 0 or at least 56 steps (>= 0.1); the mask is sigmoid(32768 hidden - 2000): 0 (the float64
    and the fp32 exponential both overflow) or 1."""
    cfg = config(base)
    rng = np.random.default_rng(seed)
    g = int(cfg["growth"])
    deep = sum(cfg["blocks"]) > 8
    w = {}
    for name, shape in W.spk_tensor_shapes(cfg).items():
        if name.endswith(".scale"):
            a = rng.choice([1.0, 1.0, 1.0, -1.0], shape)
        elif name.endswith((".bias", ".shift")):
            a = rng.choice([0.0, 1.0], shape)
        else:
            a = np.zeros(shape)
            flat = a.reshape(shape[0], -1)
            nnz = 1 if (deep and name.startswith("block")) else 2
            vals = [1.0, -1.0, 0.5, -0.5] if name == "head.conv1.weight" else [1.0, -1.0]
            for r in range(shape[0]):
                cols = rng.choice(flat.shape[1], size=min(nnz, flat.shape[1]), replace=False)
                flat[r, cols] = rng.choice(vals, len(cols))
        w[name] = a.astype(np.float32)
    for b, ((C0, _), n) in enumerate(zip(W.spk_channel_plan(cfg), cfg["blocks"])):
        for l in range(int(n)):
            p = "block%d.%d." % (b + 1, l)
            w[p + "cam2.weight"][:] = 0
            w[p + "cam2.bias"][:] = 64
            w[p + "cam2.bias"][0] = 0
            for k in range(l):
                col = C0 + k * g                                  # layer k's halved channel
                lw = w[p + "linear1.weight"]
                moved = lw[:, col].copy()
                lw[:, col] = 0
                lw[:, col + 1] += moved * (lw[:, col + 1] == 0)   # (keeps the row's weight on a neighbour that is not halved)
    if segment_mask:
        bn = int(cfg["bn_channels"])
        probe = exact_rows(130, cfg["n_mels"], 977)
        for b, n in enumerate(cfg["blocks"]):                  # block by block: a later block's context depends on the earlier masks
            p = "block%d.%d." % (b + 1, int(n) - 1)
            tr = {}
            emulate_f16(cfg, w, probe, trace=tr)
            ctx = tr["ctx"][p]
            order = np.argsort(-(ctx.max(axis=0) - ctx.min(axis=0)), kind="stable")
            for j in range(bn // 2):
                c = int(order[j % 3])                          # the three columns that differ most between the probe's segments
                mid = float(np.float16(0.5 * (ctx[:, c].max() + ctx[:, c].min())))
                mid = max(mid, 2.0)
                theta = mid + 2.0 ** (np.floor(np.log2(mid)) - 10) / 8
                w[p + "cam1.weight"][j, :] = 0
                w[p + "cam1.weight"][j, c] = 64
                w[p + "cam1.bias"][j] = -64 * theta
            for ch in range(g // 2, g):
                w[p + "cam2.weight"][ch, ch % (bn // 2)] = 32768
                w[p + "cam2.bias"][ch] = -2000
    return cfg, w


def exact_rows(T, n_mels, seed):
    """small integers whose every column has an integral mean: x[t, f] = base[f] + d[t, f] with sum_t d = 0"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-2, 3, (T, n_mels)).astype(np.float64)
    if T:
        d[-1] -= d.sum(axis=0)
    return (rng.integers(-3, 4, (1, n_mels)) + d).astype(np.float32)


def exact_premise(cfg, w, rows):
    """(worst magnitude at a rounding on the way to the frames, every such rounding lossless and every mask exactly 0, 1/2 or
    1 with its argument far from where float64 and fp32 differ, the float64 frames equal the emulation's)"""
    tr = {}
    a, b = forward(cfg, w, rows), emulate_f16(cfg, w, rows, trace=tr)
    return tr.get("worst", 0.0), tr.get("lossless", True) and tr.get("mask_exact", True), bool(np.array_equal(a["frames"], b["frames"]))


def mask_varies(cfg, w, rows):
    """whether some layer's mask differs between two segments of this window"""
    tr = {}
    emulate_f16(cfg, w, rows, trace=tr)
    return tr.get("mask_varies", False)


# ---- the window plan --------------------------------------------------------------------------------------------------------
def windows(b, e, win=150, shift=75, min_frames=20):
    n = e - b
    if n < min_frames:
        return []
    if n <= win:
        return [(b, e)]
    out = [(b + k * shift, b + k * shift + win) for k in range((n - win) // shift + 1)]
    if out[-1][1] != e:
        out.append((e - win, e))
    return out


def stream_windows(segs, win=150, shift=75, min_frames=20, max_windows=MAX_WINDOWS):
    """segs [(b, e)] frames -> ([(segment, begin, end)], the shift used): the shift doubles until the stream has at most
    max_windows windows; a shift of 2^30 or more is not doubled again, the first max_windows windows are kept"""
    while True:
        out = [(i, wb, we) for i, (b, e) in enumerate(segs) for wb, we in windows(b, e, win, shift, min_frames)]
        if len(out) <= max_windows:
            return out, shift
        if shift >= 1 << 30:
            return out[:max_windows], shift
        shift *= 2


# ---- affinity, clustering, labels -----------------------------------------------------------------------------------------
def affinity(emb):
    """cosine of every pair, float64; a zero vector has cosine 0 with everything"""
    e = np.asarray(emb, np.float64)
    n = np.sqrt((e * e).sum(axis=1))
    d = n[:, None] * n[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, (e @ e.T) / d, 0.0)


def cluster(S, threshold=0.5, num_speakers=0, min_cluster=4, margins=None):
    """S [N, N] fp32 (its upper triangle is read; a value that is not finite counts as -2) -> (labels [N] int32, speakers).
    margins (a list): receives, per decision, the gap between the winning similarity and its runner-up and, without
    num_speakers, its distance from the threshold (the stop decision included).
    With num_speakers > 0 the threshold is not consulted and the rule for minor clusters does not run."""
    S = np.asarray(S, np.float32).astype(np.float64)
    N = S.shape[0]
    if N == 0:
        return np.zeros(0, np.int32), 0
    sim = np.where(np.isfinite(S), S, -2.0)
    sim = np.triu(sim, 1) + np.triu(sim, 1).T
    alive, size, member = list(range(N)), [1] * N, {i: [i] for i in range(N)}
    while len(alive) > 1 and not (num_speakers > 0 and len(alive) <= num_speakers):
        best, bi, bj, second = -np.inf, -1, -1, -np.inf
        for ai, i in enumerate(alive):
            for j in alive[ai + 1:]:
                s = sim[i, j]
                if s > best:
                    second, best, bi, bj = best, s, i, j
                elif s > second:
                    second = s
        if margins is not None:
            margins.append(best - second)
            if num_speakers <= 0:
                margins.append(abs(best - threshold))
        if num_speakers <= 0 and best < threshold:
            break
        for c in alive:
            if c != bi and c != bj:
                v = (size[bi] * sim[bi, c] + size[bj] * sim[bj, c]) / (size[bi] + size[bj])
                sim[bi, c] = sim[c, bi] = v
        size[bi] += size[bj]
        member[bi] += member.pop(bj)
        alive.remove(bj)
    if num_speakers <= 0:
        major = [c for c in alive if size[c] >= min_cluster]
        if major:
            for c in [c for c in alive if size[c] < min_cluster]:
                t = max(major, key=lambda k: (sim[c, k], -k))
                member[t] += member.pop(c)
                alive.remove(c)
    labels = np.full(N, -1, np.int32)
    for k, c in enumerate(sorted(alive, key=lambda c: min(member[c]))):
        labels[member[c]] = k
    return labels, len(alive)


def segment_labels(segs, win_seg, win_label):
    """segs [(b, e)] in time order, win_seg / win_label per window -> the label per segment: the one most of its windows hold
    (ties to the lower); a segment without a window takes the label of the nearest labelled segment (the gap between the
    two, ties to the earlier), -1 if there is none"""
    n = len(segs)
    out = np.full(n, -1, np.int32)
    for i in range(n):
        ls = [int(l) for s, l in zip(win_seg, win_label) if s == i and l >= 0]
        if ls:
            cnt = np.bincount(ls)
            out[i] = int(np.argmax(cnt))
    have = [i for i in range(n) if out[i] >= 0]
    res = out.copy()
    for i in range(n):
        if out[i] < 0 and have:
            gap = lambda j: (segs[i][0] - segs[j][1]) if j < i else (segs[j][0] - segs[i][1])
            res[i] = out[min(have, key=lambda j: (gap(j), j))]
    return res


def centroids(emb, labels, K):
    """the L2-normalised mean of each speaker's L2-normalised embeddings [K, E] (a zero vector stays zero)"""
    e = np.asarray(emb, np.float64)
    n = np.sqrt((e * e).sum(axis=1, keepdims=True))
    e = np.where(n > 0, e / np.where(n > 0, n, 1.0), 0.0)
    out = np.zeros((K, e.shape[1]))
    for k in range(K):
        sel = e[np.asarray(labels) == k]
        if len(sel):
            c = sel.mean(axis=0)
            nc = np.sqrt((c * c).sum())
            out[k] = c / nc if nc > 0 else 0.0
    return out


# ---- a constructed model and recording for the end-to-end tests ----------------------------------------------------------------
def separating_model():
    """Released dimensions, constructed (not trained) weights whose embedding is (how much the mel bins 0, 8, .. 32 move from
    frame to frame, the same for the bins 40, 48, .. 72, 0, ..).  The network subtracts a window's mean spectrum, so two sources
    can only differ in how their spectrum MOVES: conv1 splits x[t] - x[t - 1] into its positive and its negative part, every
    later convolution of the head passes its input's even frequencies on, the TDNN sums each band over the two parts and two
    frames, less SEPARATING_BIAS (above the frame-to-frame noise of a quiet floor) and clipped at 0; the dense layers add nothing
    and the transits carry channels 0 and 1 through to the pooling, whose means are the embedding."""
    cfg = config()
    w = {k: np.zeros(s, np.float32) for k, s in W.spk_tensor_shapes(cfg).items()}
    for k in w:
        if k.endswith(".scale"):
            w[k][:] = 1
    w["head.conv1.weight"][0, 0, 1, 1], w["head.conv1.weight"][0, 0, 1, 0] = 1, -1     # [out, in, frequency, time]: x[t] - x[t - 1]
    w["head.conv1.weight"][1, 0, 1, 1], w["head.conv1.weight"][1, 0, 1, 0] = -1, 1
    eye = np.eye(cfg["m_channels"], dtype=np.float32)
    for layer in (1, 2):
        w["head.layer%d.0.shortcut.weight" % layer][:, :, 0, 0] = eye
    w["head.conv2.weight"][:, :, 1, 1] = eye
    F8 = cfg["n_mels"] // 8
    for c in (0, 1):
        w["tdnn.weight"][0, c * F8: c * F8 + F8 // 2, 1:3] = 3     # (the narrow low bins move less than the wide high ones)
        w["tdnn.weight"][1, c * F8 + F8 // 2: (c + 1) * F8, 1:3] = 1
    w["tdnn.bias"][:2] = -SEPARATING_BIAS
    for b in (1, 2, 3):
        w["transit%d.weight" % b][0, 0] = w["transit%d.weight" % b][1, 1] = 1
    w["dense.weight"][0, 0] = w["dense.weight"][1, 1] = 1
    return cfg, w


SEPARATING_BIAS = 16.0
# (first frame, end frame, source, the switched band's level in its quiet phase, the other band's: 1 = steady)
TWO_SOURCE_BURSTS = [(100, 180, "A", 0.01, 1.0), (330, 410, "B", 0.01, 1.0), (560, 640, "A", 0.03, 1.0), (790, 870, "B", 0.02, 1.0)]
TWO_SOURCE_FADE = 25                        # frames over which a burst rises from the floor and falls back to it
TWO_SOURCE_VAD = dict(min_speech=50)
TWO_SOURCE_SPK = dict(win=200, shift=100)   # one window per segment


def two_source_audio(seed=1):
    """10 s at 16 kHz: four bursts over the same two combs 40 dB below them (a floor of noise would move from frame to frame; the
    comb does not).  A burst is two combs of 100 Hz harmonics (one period per
    frame shift, so a steady comb gives the same fbank row in every frame): 100 .. 1500 Hz and 1600 .. 7000 Hz.  Source A keeps
    the low comb steady and switches the high one between full and its quiet level every 4 frames; source B does the opposite.
    Every burst fades in and out."""
    rng = np.random.default_rng(seed)
    n = 160000
    t = np.arange(n) / 16000.0
    lo = sum(np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) for f in range(100, 1501, 100)) * 0.01
    hi = sum(np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) for f in range(1600, 7001, 100)) * 0.01
    x = 0.01 * (lo + hi) + 1e-6 * rng.standard_normal(n)
    for b, e, src, quiet, other in TWO_SOURCE_BURSTS:
        # the burst fades in and out over TWO_SOURCE_FADE frames, evenly in log level: a step of 40 dB at its edges would move
        # both bands alike and as much as the switching does
        sl = slice((b - TWO_SOURCE_FADE) * 160, (e + TWO_SOURCE_FADE) * 160)
        k = np.arange((e - b + 2 * TWO_SOURCE_FADE) * 160) / 160.0 - TWO_SOURCE_FADE
        rise = np.clip(np.minimum(k, (e - b) - k) / TWO_SOURCE_FADE + 1.0, 0.0, 1.0)
        gain = 0.99 * 100.0 ** (rise - 1.0)                      # 0.0099 at the ends (the floor's 0.01 on top makes 0.0199), 0.99 inside
        env = np.where((np.floor(k).astype(np.int64) // 4) % 2 == 0, 1.0, quiet)
        env = np.where((k >= 0) & (k < e - b), env, 1.0)
        env2 = np.where(((np.floor(k).astype(np.int64) + 2) // 4) % 2 == 0, 1.0, other)      # the other band, two frames out of step
        env2 = np.where((k >= 0) & (k < e - b), env2, 1.0)
        x[sl] += gain * ((lo[sl] * env2 + hi[sl] * env) if src == "A" else (lo[sl] * env + hi[sl] * env2))
    return np.clip(x, -0.999, 0.999).astype(np.float32)


def label_decisions_are_safe(S, allowance, **kw):
    """(labels, speakers, safe): cluster(S) and whether no decision of that run lies within twice `allowance` of the threshold
    or of its runner-up: an S' within `allowance` of S everywhere then takes the same decisions.  (After a merge the
    similarities are averages of entries of S, so they move by at most `allowance` too.)"""
    mg = []
    labels, k = cluster(S, margins=mg, **kw)
    return labels, k, bool(mg) and min(mg) > 2 * allowance


def cosine_allowance(cfg, w, windows):
    """(the definition's cosines, what the device may move one by): 4 x the deviation of the float16 emulation's cosines from
    the definition's, the margin the embedding itself is given"""
    a = affinity(np.stack([forward(cfg, w, x)["emb"] for x in windows]))
    b = affinity(np.stack([emulate_f16(cfg, w, x)["emb"] for x in windows]))
    return a, 4 * float(np.abs(a - b).max())
