"""The definition of the FSMN-VAD model score in numpy float64 (include/paraformer_hip.h "Voice-activity segmentation, model
score"): the second form of step 1 of the detector of tests/vad_ref.py.  Steps 2-6 stay what they are.

A model is (cfg, w): the config and the tensor dict of a `.pfw` of kind "fsmnvad" (aliparaformerasr_amd/weights.py
fsmn_vad_config / synth_vad_weights).  Everything below is for ONE utterance: rows [T, n_mels] fbank, frames t = 0 .. T-1.

    u[t]   = concat_j x[clamp(t - (lfr_m - 1) // 2 + j, 0, T - 1)], j = 0 .. lfr_m - 1;  then (u + shift) * scale
    a      = ReLU(in2(in1(u)))                                    (both affine with bias)
    layer  p = linear(a) (no bias);  m[t] = p[t] + sum_k taps[k] * p[t - (lorder - 1 - k) * lstride] (rows before frame 0 are
           zeros);  a = ReLU(affine(m))
    z      = out2(out1(a))
    s      = sum over sil_ids of softmax(z);  e[t] = rint((1 - 2 s) * 16384), half to even; a value that is not finite gives
           -16384 (silence)

`emulate_f16` restates the device kernel's arithmetic (csrc/k_vadnet.hip): float32 everywhere, operands of the matrix
products rounded to float16 at the kernel's rounding points R0 .. R6.  It is what the GPU test derives its tolerance from."""
import numpy as np

LEVEL_ONE = 16384


def _f64(a):
    return np.asarray(a, np.float64)


def lfr_index(T, lfr_m):
    left = (lfr_m - 1) // 2
    if T == 0:
        return np.zeros((0, lfr_m), np.int64)
    return np.clip(np.arange(T)[:, None] - left + np.arange(lfr_m)[None, :], 0, T - 1)


def splice(cfg, w, rows, dt=np.float64):
    x = np.asarray(rows, dt)
    T = x.shape[0]
    assert x.ndim == 2 and x.shape[1] * cfg["lfr_m"] == cfg["input_dim"], (x.shape, cfg["lfr_m"], cfg["input_dim"])
    u = x[lfr_index(T, cfg["lfr_m"])].reshape(T, cfg["input_dim"])
    with np.errstate(invalid="ignore", over="ignore"):
        return (u + np.asarray(w["cmvn.shift"], dt)) * np.asarray(w["cmvn.scale"], dt)


def fsmn(p, taps, lstride):
    """m[t] = p[t] + sum_k taps[k] * p[t - (lorder - 1 - k) * lstride]; taps [lorder, proj]"""
    T, lorder = p.shape[0], taps.shape[0]
    m = p.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(lorder):
            d = (lorder - 1 - k) * lstride
            if d < T:
                m[d:] += taps[k] * p[: T - d]
    return m


def _relu(a):
    return np.where(a < 0, 0, a)                     # NaN stays NaN (np.maximum would do too; the kernel writes x < 0 ? 0 : x)


def logits(cfg, w, rows, trace=None):
    """[T, output_dim] float64.  trace: a list that receives every array the device kernel rounds to float16 (R1 .. R6)"""
    def note(a):
        if trace is not None:
            trace.append(a)
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        a = note(splice(cfg, w, rows))
        a = note(a @ _f64(w["in1.weight"]).T + _f64(w["in1.bias"]))
        a = note(_relu(a @ _f64(w["in2.weight"]).T + _f64(w["in2.bias"])))
        for l in range(cfg["n_layers"]):
            p = a @ _f64(w["fsmn.%d.linear.weight" % l]).T
            m = note(fsmn(p, _f64(w["fsmn.%d.taps" % l]), cfg["lstride"]))
            a = note(_relu(m @ _f64(w["fsmn.%d.affine.weight" % l]).T + _f64(w["fsmn.%d.affine.bias" % l])))
        a = note(a @ _f64(w["out1.weight"]).T + _f64(w["out1.bias"]))
        return a @ _f64(w["out2.weight"]).T + _f64(w["out2.bias"])


def unrounded_levels(cfg, z):
    """(1 - 2 s) * 16384 in float64 from logits z [T, output_dim]; NaN where the softmax is not finite"""
    z = _f64(z)
    if z.shape[0] == 0:
        return np.zeros(0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ex = np.exp(z - np.max(z, axis=1, keepdims=True))
        s = ex[:, list(cfg["sil_ids"])].sum(axis=1) / ex.sum(axis=1)
        return (1.0 - 2.0 * s) * LEVEL_ONE


def levels_from_logits(cfg, z):
    v = unrounded_levels(cfg, z)
    ok = np.isfinite(v)
    out = np.full(v.shape, -LEVEL_ONE, np.int32)
    out[ok] = np.rint(v[ok]).astype(np.int32)
    return out


def levels(cfg, w, rows):
    return levels_from_logits(cfg, logits(cfg, w, rows))


def halo(cfg):
    """frames in front of frame a that frames >= a depend on"""
    return cfg["n_layers"] * (cfg["lorder"] - 1) * cfg["lstride"] + (cfg["lfr_m"] - 1) // 2


# ---- the device kernel's arithmetic --------------------------------------------------------------------------------
def _h(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _mm(a16, wt):
    """float16-valued operands (held in float32), float32 accumulation"""
    with np.errstate(invalid="ignore", over="ignore"):
        return a16 @ _h(wt).T                                          # R0: the weight image is float16


def emulate_f16(cfg, w, rows):
    """[T, output_dim] float32: the logits as k_vadnet.hip computes them, up to the order of the float32 sums"""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        a = _h(splice(cfg, w, rows, f))                                                                  # R1
        a = _h(_mm(a, w["in1.weight"]) + np.asarray(w["in1.bias"], f))                                   # R2
        a = _h(_relu(_mm(a, w["in2.weight"]) + np.asarray(w["in2.bias"], f)))                            # R3
        for l in range(cfg["n_layers"]):
            p = _mm(a, w["fsmn.%d.linear.weight" % l])                                                   # stored as float32
            m = _h(fsmn(p, np.asarray(w["fsmn.%d.taps" % l], f), cfg["lstride"]))                        # R4
            a = _h(_relu(_mm(m, w["fsmn.%d.affine.weight" % l]) + np.asarray(w["fsmn.%d.affine.bias" % l], f)))   # R5
        a = _h(_mm(a, w["out1.weight"]) + np.asarray(w["out1.bias"], f))                                 # R6
        return (_mm(a, w["out2.weight"]) + np.asarray(w["out2.bias"], f)).astype(f)


# ---- models and inputs shared by the CPU and the GPU tests ------------------------------------------------------------
SMALL = dict(n_mels=8, lfr_m=5, affine_dim=12, linear_dim=20, proj_dim=16, output_dim=5, lorder=3, lstride=2, n_layers=2,
             sil_ids=[0, 3])
LENGTHS_SMALL = [0, 1, 2, 3, 4, 5, 63, 64, 65, 131]                  # lorder - 1, lorder, lorder + 1 = 2, 3, 4
LENGTHS_RELEASED = [0, 1, 2, 3, 19, 20, 21, 63, 64, 65, 131]
MIXED_BATCH = [5, 0, 70, 1, 131]


def small_model(seed=5):
    from aliparaformerasr_amd import weights as W
    cfg = W.fsmn_vad_config(**SMALL)
    return cfg, W.synth_vad_weights(cfg, seed)


def released_model(seed=6):
    from aliparaformerasr_amd import weights as W
    cfg = W.fsmn_vad_config()
    return cfg, W.synth_vad_weights(cfg, seed)


def fbank_like(T, n_mels, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, n_mels)) * 3 - 4).astype(np.float32)


def exact_model(base, seed):
    """A model on which the device kernel must give the float64 answer bit for bit: weights and biases in {0, +-1, +-2,
    +-1/2} with two or three non-zeros per row at random columns, two FSMN taps of +-1 per channel (the oldest always among
    them), scale a power of two, shift even integers.  With `exact_rows` every value the kernel rounds to float16 is an integer
    below 2048, so no rounding loses anything and every float32 sum is exact in any order (`exact_worst` asserts it)."""
    from aliparaformerasr_amd import weights as W
    cfg = W.fsmn_vad_config(**base)
    rng = np.random.default_rng(seed)

    def sparse(n_out, n_in, nz, vals):
        a = np.zeros((n_out, n_in), np.float32)
        for r in range(n_out):
            c = rng.choice(n_in, size=min(nz, n_in), replace=False)
            a[r, c] = rng.choice(np.asarray(vals, np.float32), size=c.size)
        return a

    def ints(n, lo, hi):
        return rng.integers(lo, hi + 1, n).astype(np.float32)
    one = (1, -1)
    w = {"cmvn.shift": 2 * ints(cfg["input_dim"], -1, 1), "cmvn.scale": rng.choice(np.array([1, 2], np.float32), cfg["input_dim"])}
    w["in1.weight"], w["in1.bias"] = sparse(cfg["affine_dim"], cfg["input_dim"], 3, (1, -1, 2, -2, 0.5, -0.5)), ints(cfg["affine_dim"], -2, 2)
    w["in2.weight"], w["in2.bias"] = sparse(cfg["linear_dim"], cfg["affine_dim"], 2, one), ints(cfg["linear_dim"], -1, 1)
    for l in range(cfg["n_layers"]):
        w["fsmn.%d.linear.weight" % l] = sparse(cfg["proj_dim"], cfg["linear_dim"], 2 if l == 0 else 1, one)
        t = np.zeros((cfg["lorder"], cfg["proj_dim"]), np.float32)
        for c in range(cfg["proj_dim"]):
            t[int(rng.integers(0, cfg["lorder"])), c] = rng.choice(np.asarray(one, np.float32))
            t[0, c] = rng.choice(np.asarray(one, np.float32))
        w["fsmn.%d.taps" % l] = t
        w["fsmn.%d.affine.weight" % l] = sparse(cfg["linear_dim"], cfg["proj_dim"], 2 if l < 2 else 1, one)
        w["fsmn.%d.affine.bias" % l] = ints(cfg["linear_dim"], -2, 1)
    w["out1.weight"], w["out1.bias"] = sparse(cfg["affine_dim"], cfg["linear_dim"], 2, one), ints(cfg["affine_dim"], -1, 1)
    w["out2.weight"], w["out2.bias"] = sparse(cfg["output_dim"], cfg["affine_dim"], 2, (1, -1, 2, -2)), ints(cfg["output_dim"], -2, 2)
    return cfg, w


def exact_rows(T, n_mels, seed):
    """even integers in [-2, 2], mostly zero"""
    rng = np.random.default_rng(seed)
    return (2 * rng.integers(-1, 2, (T, n_mels)) * (rng.random((T, n_mels)) < 0.5)).astype(np.float32)


def exact_worst(cfg, w, rows):
    """the largest |value| the kernel rounds to float16 on these rows, and whether every one of them is an integer: the
    exact-answer tests assert (< 2048, True), which makes every rounding lossless and every float32 sum exact"""
    tr = []
    z = logits(cfg, w, rows, tr)
    tr.append(z)
    fin = [a[np.isfinite(a)] for a in tr]
    return max([float(np.abs(a).max()) for a in fin if a.size] + [0.0]), all(bool((a == np.rint(a)).all()) for a in fin)


# ---- a constructed (not trained) discriminating model for the end-to-end tests -------------------------------------------
ENERGY = dict(n_mels=80, lfr_m=5, affine_dim=8, linear_dim=16, proj_dim=8, output_dim=2, n_layers=2, lorder=4, lstride=1, sil_ids=[0])


def energy_model(rows, seed=3):
    """Non-negative weights up to out_linear1 make the hidden sum h[t] grow with the (smoothed) log-mel level of the frame;
    the silence row of out_linear2 is -g * h + b, the other row 0, with g and b set from `rows` ([T, 80] fbank holding quiet and
    loud stretches) so that p_sil = 0.2 half way between the 10th and the 90th percentile of h and moves by a logit of 4 to
    either of them: quiet frames get p_sil = 0.93, loud ones 0.005."""
    from aliparaformerasr_amd import weights as W
    cfg = W.fsmn_vad_config(**ENERGY)
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in W.vad_tensor_shapes(cfg).items():
        if name == "cmvn.shift":
            a = np.full(shape, 16.0)
        elif name == "cmvn.scale":
            a = np.full(shape, 1.0 / 16)
        elif name.endswith(".bias"):
            a = np.zeros(shape)
        elif name.endswith(".taps"):
            a = 0.1 * rng.uniform(0.8, 1.2, shape)
        else:
            a = rng.uniform(0.8, 1.2, shape) / shape[1]
        w[name] = a.astype(np.float32)
    w["out2.weight"] = np.zeros((2, cfg["affine_dim"]), np.float32)
    tr = []
    logits(cfg, w, rows, tr)
    h = tr[-1].sum(axis=1)                                            # the sum of out_linear1's outputs
    lo, hi = np.percentile(h, 10), np.percentile(h, 90)
    g = 8.0 / (hi - lo)
    w["out2.weight"][0, :] = np.float32(-g)
    w["out2.bias"] = np.array([np.log(0.25) + g * (lo + hi) / 2, 0.0], np.float32)
    return cfg, w


def near_threshold(levels_ref, abs_level, tol):
    return np.abs(np.asarray(levels_ref, np.int64) - abs_level) <= tol


def decisions_are_safe(levels_ref, cfg_vad, n_mels, abs_level, tol, max_share=0.02):
    """The condition under which segments over approximate levels must equal segments over the reference levels: at most
    max_share of the frames lie within tol of abs_level, and pushing all of them to either side changes no segment."""
    import vad_ref as V
    e = np.asarray(levels_ref, np.int32)
    near = near_threshold(e, abs_level, tol)
    if e.size and near.mean() > max_share:
        return False
    want = V.segments(e, n_mels, cfg_vad)
    up, dn = e.copy(), e.copy()
    up[near], dn[near] = abs_level + tol + 1, abs_level - tol - 1
    return V.segments(up, n_mels, cfg_vad) == want and V.segments(dn, n_mels, cfg_vad) == want
