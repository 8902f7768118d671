"""CPU: the host twin of the streaming PCM intake (pf_host_pcm_stream_*, csrc/hostutil.cpp PcmStream).  For every way of cutting
the bytes into pushes the emitted samples are, bit for bit, pf_host_pcm_convert of the concatenated bytes, and nothing is ever
emitted that the final sequence does not contain.  The one-shot itself is held to the definitions: the linear rule to a numpy
float64 restatement (bit for bit), the band-limited rule to tests/resample_ref.py within its derived bound."""
import ctypes as C

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
import resample_ref as R
from pcm_ref import bits_equal, payload

FS = 16000
RATES = (8000, 11025, 44100, 48000, 96000)
BPV = {"s16": 2, "s24": 3, "f32": 4, "mulaw": 1}


def cuts_of(n_bytes, fb, taps, seed):
    """Byte offsets at which the payload is cut: seeded random ones and the hand-made ones of the issue."""
    rng = np.random.default_rng([seed, n_bytes])
    out = [sorted(rng.integers(0, n_bytes + 1, k).tolist()) for k in (3, 9)]
    out.append([0, 0, (taps - 1) * fb, (2 * taps - 1) * fb, (3 * taps) * fb])          # an empty push; taps - 1, taps, taps + 1 frames
    out.append([1, fb + 1, n_bytes // 2 + 1, n_bytes - 1])                            # pushes that split a frame
    if n_bytes <= 400 * fb:
        out.append(list(range(fb, n_bytes, fb)))                                     # one frame per push
    return [sorted(min(max(c, 0), n_bytes) for c in cut) for cut in out]


def stream_all(data, desc, cut, whole):
    """Pushes data in the pieces `cut` names, asserting the prefix property after every push; returns the total."""
    ps, got = N.HostPcmStream(desc, FS), np.zeros(0, np.float32)
    for a, b in zip([0] + cut, cut + [len(data)]):
        got = np.concatenate([got, ps.push(data[a:b])])
        assert got.size <= whole.size and bits_equal(got, whole[:got.size])
    return np.concatenate([got, ps.finish()])


def linear_ref(m, sr):
    """Resample's interpolation in numpy float64: two products and a sum, each rounded."""
    m = m.astype(np.float64)
    ratio = sr / FS
    i = np.arange(R.n_out_of(m.size, sr, FS), dtype=np.float64)
    pos = i * ratio
    idx = pos.astype(np.int64)
    fr, last = pos - idx, m.size - 1
    inner = (1 - fr) * m[np.minimum(idx, last)] + fr * m[np.minimum(idx + 1, last)]
    return np.where(idx >= last, m[last] if m.size else 0.0, inner).astype(np.float32)


@pytest.mark.parametrize("sinc", (False, True), ids=("linear", "sinc"))
@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("fmt", sorted(BPV))
@pytest.mark.parametrize("sr", RATES)
def test_every_cut_gives_the_one_shot_conversion(sr, fmt, ch, sinc):
    _L, _M, H, _c = R.shape(sr, FS)
    desc = N.pcm_desc(sr, ch, fmt, sinc=sinc)
    lengths = [0, 1, 2, H - 1, H, H + 1, 3 * H + 7] + ([6 * 50 + 3, 6 * 150 + 3] if sr == 96000 else [])   # 96 kHz: Round's half-to-even case
    for n_mono in lengths:
        nv = n_mono if ch == 1 else 2 * n_mono + 1                                    # stereo: an unpaired trailing value
        data = payload(fmt, nv, seed=sr // 100 + ch)
        whole = N.host_pcm_convert(data, desc)
        m = R.mono(data, sr, ch, fmt)
        if sinc:
            want, bound = R.resample(m, sr, FS)
            assert whole.size == want.size and np.all(np.abs(whole - want) <= bound)
        else:
            assert bits_equal(whole, linear_ref(m, sr))
        for cut in cuts_of(len(data), BPV[fmt] * ch, 2 * H, seed=n_mono):
            assert bits_equal(stream_all(data, desc, cut, whole), whole), (n_mono, cut)


@pytest.mark.parametrize("flag", (False, True))
def test_the_native_rate_stays_interleaved_unless_asked(flag):
    data = payload("s16", 2 * 333 + 1, seed=5)
    desc = N.pcm_desc(FS, 2, "s16", downmix_always=flag)
    whole = N.host_pcm_convert(data, desc)
    assert whole.size == (333 if flag else 667)
    assert bits_equal(stream_all(data, desc, [1, 3, 700, 701], whole), whole)


def test_refusals_and_symbols():
    lib, h, n = N.load(), C.c_void_p(), C.c_int64()
    for name in ("pf_online_stream_add_pcm", "pf_online_recognizer_set_resample", "pf_op_online_pcm_step", "pf_host_pcm_stream_state_bytes"):
        assert hasattr(lib, name)
    assert lib.pf_host_pcm_stream_create(C.byref(N.pcm_desc(8000, 3, "s16")), FS, None, C.byref(h)) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_pcm_stream_create(C.byref(N.pcm_desc(16001, 1, "s16", sinc=True)), FS, None, C.byref(h)) == N.PF_ERR_UNSUPPORTED   # L = 16000
    wide = N.resample_config(64, 0.05, 10.0)                                          # more than 1024 taps
    assert lib.pf_host_pcm_stream_create(C.byref(N.pcm_desc(48000, 1, "s16", sinc=True)), FS, C.byref(wide), C.byref(h)) == N.PF_ERR_UNSUPPORTED
    ps = N.HostPcmStream(N.pcm_desc(8000, 1, "s16"), FS)
    ps.finish()
    assert lib.pf_host_pcm_stream_push(ps._h, b"\0\0", 2, None, 0, C.byref(n)) == N.PF_ERR_INVALID_ARG   # bytes after the end
