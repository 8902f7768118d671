"""numpy statement of the (Bi)LSTM recurrence of the two heads and of the timestamp head's tail (csrc/k_bicif.hip, csrc/k_fp32.hip),
shared by tests/test_lstm_ref_cpu.py (which pins it against torch.nn.LSTM and the oracle) and tests/test_gpu_lstm.py.

lstm_ref runs on prepared gate inputs xg = x W_ih^T + b_ih + b_hh, as the kernels do.  `operands` says how W_hh and h_{t-1} are
rounded before the recurrent product, and only there (xg, the cell state and the returned h are never rounded):
  "f16"   both to f16                                              (lstm_step_kernel, lstm_ring_kernel<false>)
  "pair"  hi = f16(x), lo' = f16((x - hi) * 2048), value hi + lo' / 2048 — 22 mantissa bits   (lstm_ring_kernel<true>)
  "exact" nothing                                                  (launch_gemm_f32 + lstm_cell_f32_kernel)
`dtype` is the arithmetic everything else runs in: float64 is the reference proper; a float32 rerun of the same model is how the
tests size their bounds (its distance from the float64 run is what fp32 evaluation order and re-rounding flips cost)."""
import numpy as np

F32 = np.float32


def round_operand(x, operands, dtype):
    if operands == "exact":
        return x.astype(dtype)
    hi = x.astype(np.float16)
    if operands == "f16":
        return hi.astype(dtype)
    if operands == "pair":
        lo = ((x.astype(np.float64) - hi.astype(np.float64)) * 2048.0).astype(np.float16)
        return (hi.astype(np.float64) + lo.astype(np.float64) / 2048.0).astype(dtype)      # 22 bits: exact in float32 too
    raise ValueError(operands)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))                   # (numpy keeps the array's dtype)


def stale_units(units):
    """hook for lstm_ref: the recurrent input of `units` comes from one step too early (h_{s-2} instead of h_{s-1}) — what
    the other workgroups see when one producer's 16-byte granule of the ring is read before it was rewritten."""
    units = np.asarray(units)

    def hook(d, step, h1, h2):
        h = h1.copy()
        h[:, units] = h2[:, units]
        return h
    return hook


def lstm_ref(xg, whh, ndir, dtype=np.float64, operands="exact", hook=None, gate_order=(0, 1, 2, 3)):
    """xg [B, T3, ndir * 4D] (PyTorch gate order i, f, g, o; directions side by side), whh [ndir, 4D, D] -> hout [B, T3, ndir * D]
    in `dtype`.  Direction 1 runs backwards in time.  hook(d, step, h_{s-1}, h_{s-2}) -> the h the recurrent product of step s
    reads (tests: a deliberately wrong exchange).  gate_order permutes which 4D block is read as i, f, g, o (tests only)."""
    xg = np.asarray(xg)
    whh = np.asarray(whh)
    B, T3, G = xg.shape
    D = whh.shape[2]
    assert whh.shape == (ndir, 4 * D, D) and G == ndir * 4 * D
    out = np.zeros((B, T3, ndir * D), dtype)
    gi, gf, gg, go = gate_order
    for d in range(ndir):
        Wt = np.ascontiguousarray(round_operand(whh[d], operands, dtype).T)                # [D, 4D]
        h = np.zeros((B, D), dtype)
        h2 = np.zeros((B, D), dtype)
        c = np.zeros((B, D), dtype)
        for step in range(T3):
            t = step if d == 0 else T3 - 1 - step
            hin = hook(d, step, h, h2) if hook is not None else h
            g = xg[:, t, d * 4 * D:(d + 1) * 4 * D].astype(dtype) + round_operand(hin, operands, dtype) @ Wt
            c = _sigmoid(g[:, gf * D:(gf + 1) * D]) * c + _sigmoid(g[:, gi * D:(gi + 1) * D]) * np.tanh(g[:, gg * D:(gg + 1) * D])
            h2 = h
            h = _sigmoid(g[:, go * D:(go + 1) * D]) * np.tanh(c)
            assert h.dtype == dtype
            out[:, t, d * D:(d + 1) * D] = h
    return out


def us_alpha_ref(hout, w, b0, smooth, noise, dtype=np.float64):
    """relu(sigmoid(hout w + b0) * smooth - noise): hout [..., W], w [W] -> [...] in `dtype` (us_alpha_kernel)."""
    z = np.asarray(hout).astype(dtype) @ np.asarray(w).astype(dtype).reshape(-1) + dtype(b0)
    return np.maximum(_sigmoid(z) * dtype(smooth) - dtype(noise), dtype(0))


def us_sums(a):
    """The float32 row sums of a [B, T3] float32 with the sum carried in float64 and rounded once, in two orders: sequential,
    and us_peak_kernel's (lane l of 64 adds a[l], a[l + 64], ... in order; then s += shfl_xor(s, o) for o = 32 .. 1).  Where the
    two agree the kernel's sum does not depend on its order at float32, and us_peak_ref can be compared bit for bit."""
    a = np.asarray(a, F32)
    B, T3 = a.shape
    seq = np.zeros(B, np.float64)
    for t in range(T3):
        seq += a[:, t].astype(np.float64)
    lanes = np.zeros((B, 64), np.float64)
    for t0 in range(0, T3, 64):
        n = min(64, T3 - t0)
        lanes[:, :n] += a[:, t0:t0 + n].astype(np.float64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return seq.astype(F32), lanes[:, 0].astype(F32)


def cif_integrate_ref(alphas, thr):
    """cif_wo_hidden in float32: integrate += alpha; peak[t] = integrate (recorded BEFORE the reset); integrate -= thr once it
    has reached thr — operation by operation as us_peak_kernel and Oracle.us_alphas_peak."""
    a = np.asarray(alphas, F32)
    thr = F32(thr)
    peak = np.zeros_like(a)
    for b in range(a.shape[0]):
        integ = F32(0.0)
        for t in range(a.shape[1]):
            integ = F32(integ + a[b, t])
            peak[b, t] = integ
            if integ >= thr:
                integ = F32(integ - thr)
    return peak


def us_peak_ref(alphas_raw, token_num, thr):
    """alphas = alphas_raw * (float32(token_num) / sum), the sum carried in float64 and rounded to float32 once; peak =
    cif_integrate_ref(alphas, thr).  float32 throughout, one rounding per operation.  -> (alphas, peak) [B, T3] float32."""
    a = np.asarray(alphas_raw, F32)
    s = us_sums(a)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.asarray(token_num).astype(F32) / s).astype(F32)
    al = (a * ratio[:, None]).astype(F32)
    return al, cif_integrate_ref(al, thr)
