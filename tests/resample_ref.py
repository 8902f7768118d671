"""The definition of the band-limited resampler (PF_PCM_RESAMPLE_SINC; include/paraformer_hip.h "PCM intake"): numpy float64,
nothing but the formulas.  Output i depends only on i and the input: a window that starts anywhere gives the same value."""
import math

import numpy as np

from oracle import audio as oa
from pcm_ref import wav_blob

DEFAULTS = dict(zeros=24, rolloff=0.94, beta=10.0)
RATES = (8000, 11025, 32000, 44100, 48000, 96000)


def i0(x):                                           # modified Bessel function, order 0, by its power series
    x = np.asarray(x, np.float64)
    q, term, total = 0.25 * x * x, np.ones_like(x), np.ones_like(x)
    for m in range(1, 500):
        term = term * q / (m * m)
        total = total + term
        if np.all(term < 1e-17 * total):
            break
    return total


def shape(sr, fs, zeros=24, rolloff=0.94, beta=10.0):   # -> L, M, H, c
    g = math.gcd(sr, fs)
    L, M = fs // g, sr // g
    c = rolloff * min(1.0, L / M)
    return L, M, int(math.ceil(zeros / c)), c


def bank(sr, fs, zeros=24, rolloff=0.94, beta=10.0):    # h[p][k] in float64, [L, taps]
    L, _M, H, c = shape(sr, fs, zeros, rolloff, beta)
    tau = (np.arange(2 * H)[None, :] - (H - 1)) - np.arange(L)[:, None] / L
    u = tau * c / zeros
    w = np.where(np.abs(u) < 1, i0(beta * np.sqrt(np.maximum(1 - u * u, 0))) / i0(beta), 0.0)
    return c * np.sinc(c * tau) * w


def n_out_of(n_mono, sr, fs):
    return int(np.rint(n_mono / (sr / fs))) if n_mono else 0          # Round, half to even: pcm_plan's


def resample(m, sr, fs, n_out=None, first=0, origin=0, **cfg):
    """Outputs first .. first + n_out - 1 of the mono float32 sequence whose sample `origin` is m[0] (zeros elsewhere) -> (y in
    float64, the bound on |y32 - y| of a float32 bank and a chain of taps fused multiply-adds)."""
    cfg = {**DEFAULTS, **cfg}
    L, M, H, _c = shape(sr, fs, **cfg)
    h = bank(sr, fs, **cfg)
    m = np.asarray(m, np.float32).astype(np.float64)
    n_out = n_out_of(m.size, sr, fs) if n_out is None else n_out
    i = first + np.arange(n_out, dtype=np.int64)
    idx = ((i * M) // L)[:, None] - H + 1 + np.arange(2 * H)[None, :] - origin
    win = np.where((idx >= 0) & (idx < m.size), m[np.clip(idx, 0, max(m.size - 1, 0))] if m.size else 0.0, 0.0)
    hp = h[(i * M) % L]
    with np.errstate(invalid="ignore"):
        return (hp * win).sum(1), (2 * H + 2) * 2.0 ** -24 * (np.abs(hp) * np.abs(win)).sum(1)


def mono(data, sr, ch, fmt):                         # the decoded, down-mixed float32 sequence the resampler reads
    x = oa.decode_wav(wav_blob(sr, ch, fmt, data))[0]
    if ch == 2:
        n = x.size // 2
        x = ((x[0:2 * n:2] + x[1:2 * n:2]) * np.float32(0.5)).astype(np.float32)
    return x


def tone(freq, sr, n, amp=0.5):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / sr)).astype(np.float32)
