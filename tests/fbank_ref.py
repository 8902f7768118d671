"""The kaldi fbank as a definition: the published steps (feature-window.cc / feature-fbank.cc / mel-computations.cc,
with the options the reference passes, as oracle/frontend.py states them) with EVERY intermediate in float64, and the
error model the device kernel is judged by.  Plain numpy; imported by tests/test_fbank_ref_cpu.py and
tests/test_gpu_fbank_conformance.py.

    fbank64(x, window, snip_edges, n_mels) -> E [T, n_mels] linear mel energies, R0 [T] = sum of the raw frame squared
    bound(E, R0)                           -> what one unit of k allows per frame and bin (see bound())
    fbank_f32(x, ...)                      -> the float32 restatement k is measured with (oracle steps, float32 rfft)
    signal(name, n) / SIGNALS / LENGTHS    -> the suite's inputs

What stays float32 on purpose: the input samples, the constant 0.97f, the stored window and the stored mel weights —
they are DATA of the definition (kaldi keeps them as float), not arithmetic.  The weights are
oracle.frontend.mel_banks(..., libm_log=True): 1127 logf(1 + f / 700) with a correctly rounded logf, as kaldi's float code
and the engine's host code get from libm.  The oracle's default weights go through numpy's float32 log (up to 2 ulp off,
69 of 501 weights of the 80-bin bank moved by up to 1.4e-5 — thirty times what this suite resolves); they stay the default
because the committed golden files were written with them (tests/test_fbank_ref_cpu.py states the distance).
"""
import functools

import numpy as np

from oracle import frontend as fe

FRAME_LEN, FRAME_SHIFT, NFFT = 400, 160, 512
FLT_EPSILON = float(np.float32(1.1920929e-07))
LOG_FLOOR = float(np.log(FLT_EPSILON))
QUIET = 4.0 * FLT_EPSILON                     # bins at or below this are judged against the floor
WINDOWS = ("hamming", "hanning", "povey", "rectangular")
# k of the conformance bound.  MEASURED_F32 = the worst ratio() of fbank_f32 (below) against fbank64 over every window,
# both framings, n_mels 40 / 80 / 128 and every case of cases() — measured on a CPU, never on the device
# (tests/test_fbank_ref_cpu.py re-measures it).  16 of it is the float32 rounding of a logarithm between 16 and 32 (half an
# ulp = 2^-20) at the frame's loudest bin, where bound() allows 2^-24 per unit of k.  K = 4 x that: the margin for another
# butterfly order and float32 twiddles.
MEASURED_F32 = 19.64
K = 4.0 * MEASURED_F32


def n_frames(n, snip_edges):
    """kaldi NumFrames(flush = true), stated on its own (the CPU test compares it with oracle.frontend.num_frames)."""
    if snip_edges:
        return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT
    return int(np.floor(n / FRAME_SHIFT + 0.5))            # round half up of n / shift


def frame_index(n, snip_edges):
    """[T, 400] sample index of every frame element; kaldi ExtractWindow's reflection loop when snip_edges is false."""
    t = n_frames(n, snip_edges)
    start = FRAME_SHIFT * np.arange(t, dtype=np.int64)
    if not snip_edges:
        start = start + (FRAME_SHIFT // 2 - FRAME_LEN // 2)
    idx = start[:, None] + np.arange(FRAME_LEN, dtype=np.int64)[None, :]
    while t and ((idx < 0) | (idx >= n)).any():            # while (s < 0 || s >= n) s = s < 0 ? -s - 1 : 2 n - 1 - s
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return idx


@functools.lru_cache(maxsize=None)
def _window64(window):
    return fe.window_function(window).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _mel64(n_mels):
    return fe.mel_banks(n_mels, 16000, libm_log=True).astype(np.float64)


def fbank64(x, window="hamming", snip_edges=False, n_mels=80):
    x = np.asarray(x, np.float32).astype(np.float64) * 32768.0
    idx = frame_index(x.shape[0], snip_edges)
    if idx.shape[0] == 0:
        return np.zeros((0, n_mels)), np.zeros(0)
    raw = x[idx]                                                         # [T, 400]
    r0 = (raw * raw).sum(axis=1)
    d = raw - raw.sum(axis=1, keepdims=True) / FRAME_LEN                 # remove_dc_offset over the 400 samples
    c = float(np.float32(0.97))
    pre = np.empty_like(d)
    pre[:, 1:] = d[:, 1:] - c * d[:, :-1]
    pre[:, 0] = d[:, 0] - c * d[:, 0]
    padded = np.zeros((raw.shape[0], NFFT))
    padded[:, :FRAME_LEN] = pre * _window64(window)[None, :]
    spec = np.fft.rfft(padded, axis=1)[:, : NFFT // 2]                   # bins 0 .. 255
    power = spec.real ** 2 + spec.imag ** 2
    return power @ _mel64(n_mels).T, r0


def log_mel(E):
    return np.log(np.maximum(E, FLT_EPSILON))


def bound(E, R0):
    """2^-24 sqrt(max(max_m E[t, m], R0[t]) / E[t, m]) — the allowance per unit of k.  A float32 transform leaves an
    amplitude error proportional to the largest amplitude of the frame, so the relative error of a bin's energy (= the
    error of its logarithm) grows as sqrt(E_max / E_bin); R0 stands for the float32 mean removal of a large DC offset.
    Bins at or below QUIET are judged against the floor with E clamped to FLT_EPSILON (the literal quotient is unbounded
    as E -> 0)."""
    top = np.maximum(E.max(axis=1), R0)[:, None]
    return 2.0 ** -24 * np.sqrt(top / np.maximum(E, FLT_EPSILON))


def ratio(got, E, R0):
    """per element: the error of `got` (log-mel, [T, n_mels]) in units of bound(); a kernel passes when max <= k.
    E > QUIET: against log E.  Otherwise against the floor — and a value AT the floor (within 1e-6 of log FLT_EPSILON:
    the two float32 neighbours of it, whichever a logf returns) counts as 0."""
    got = np.asarray(got, np.float64)
    assert got.shape == E.shape, (got.shape, E.shape)
    if got.size == 0:
        return np.zeros(E.shape)
    quiet = E <= QUIET
    want = np.where(quiet, LOG_FLOOR, np.log(np.where(quiet, 1.0, E)))
    err, b = np.abs(got - want), bound(E, R0)
    with np.errstate(divide="ignore", invalid="ignore"):                 # silence: nothing is allowed, b == 0
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    at_floor = np.abs(got - LOG_FLOOR) <= 1e-6
    r[quiet & at_floor] = 0.0
    return np.where(np.isfinite(got), r, np.inf)


def fbank_f32(x, window="hamming", snip_edges=False, n_mels=80):
    """oracle.frontend.kaldi_fbank step for step (float32 roundings where kaldi rounds) with the transform done by
    torch.fft.rfft on float32: the measuring stick for k — what ANY float32 evaluation of the definition costs."""
    import torch
    x = (np.asarray(x, np.float32) * np.float32(32768.0)).astype(np.float32)
    frames = fe.extract_frames(x, snip_edges)
    if frames.shape[0] == 0:
        return np.zeros((0, n_mels), np.float32)
    mean = (frames.sum(axis=1, dtype=np.float32) / np.float32(FRAME_LEN)).astype(np.float32)
    frames = (frames - mean[:, None]).astype(np.float32)
    pre = np.empty_like(frames)
    pre[:, 1:] = frames[:, 1:] - fe.PREEMPH * frames[:, :-1]
    pre[:, 0] = frames[:, 0] - fe.PREEMPH * frames[:, 0]
    pre = (pre.astype(np.float32) * fe.window_function(window)[None, :]).astype(np.float32)
    padded = np.zeros((pre.shape[0], NFFT), np.float32)
    padded[:, :FRAME_LEN] = pre
    spec = torch.fft.rfft(torch.from_numpy(padded), dim=1)
    assert spec.dtype == torch.complex64
    power = (spec.real ** 2 + spec.imag ** 2).numpy().astype(np.float32)[:, : NFFT // 2]
    mel = power @ _mel64(n_mels).T.astype(np.float32)                    # the stored weights are float32 values
    return np.log(np.maximum(mel.astype(np.float32), fe.FLT_EPSILON)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the suite's inputs
SIGNALS = ("synth", "white", "quiet", "tone_off_bin", "tone_on_bin", "square", "dc_noise", "impulses")
LENGTHS = {False: (80, 81, 159, 199, 239, 400, 401, 559, 560, 16000), True: (399, 400, 559, 560, 16000)}
IMPULSE_PERIOD, IMPULSE_FIRST = 997, 500


@functools.lru_cache(maxsize=None)
def signal(name, n):
    """float32 [n], read-only, the same on every call; every family is the head of its 16000-sample version"""
    from aliparaformerasr_amd import weights as W
    full = 16000
    assert n <= full
    rng = np.random.default_rng([SIGNALS.index(name), 77])
    t = np.arange(full) / 16000.0
    if name == "synth":
        x = W.synth_audio(full, 3)
    elif name == "white":
        x = 0.1 * rng.standard_normal(full)
    elif name == "quiet":
        x = 3e-5 * rng.standard_normal(full)
    elif name == "tone_off_bin":
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t + 0.3)
    elif name == "tone_on_bin":
        x = 0.5 * np.sin(2 * np.pi * (37 * 16000.0 / NFFT) * t + 0.3)      # exactly FFT bin 37
    elif name == "square":
        x = np.where(np.sin(2 * np.pi * 440.0 * t) >= 0, 1.0, -1.0)       # full scale: +-32768 after scaling
    elif name == "dc_noise":
        x = 0.9 + 1e-3 * rng.standard_normal(full)
    elif name == "impulses":
        x = np.zeros(full)
        x[IMPULSE_FIRST::IMPULSE_PERIOD] = 0.5
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(np.asarray(x, np.float32)[:n])
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def reference(name, n, window, snip_edges, n_mels=80):
    """(E, R0) of signal(name, n): computed once, shared, read-only"""
    E, r0 = fbank64(signal(name, n), window, snip_edges, n_mels)
    E.flags.writeable = False
    r0.flags.writeable = False
    return E, r0


def cases(snip_edges):
    """(name, n) of part (a): every family at 1 s, and every edge length on the three families whose edge frames differ
    most (speech-like, a large DC offset that reflection must carry, impulses that reflection moves)"""
    out = [(s, 16000) for s in SIGNALS]
    for n in LENGTHS[snip_edges]:
        if n != 16000:
            out += [(s, n) for s in ("synth", "dc_noise", "impulses", "square")]
    return out
