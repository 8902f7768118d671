"""CPU: the host twin of the band-limited resampler (pf_host_resample_sinc, pf_host_pcm_convert with PF_PCM_RESAMPLE_SINC) against
the float64 definition (tests/resample_ref.py) within the derived bound; alias, chunk invariance, errors, CLI, the linear rule."""
import ctypes as C

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import examples as ex
import resample_ref as R
from pcm_ref import bits_equal, expected, payload

FS = 16000


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("ch", (1, 2))
def test_host_twin_within_the_bound_of_the_definition(sr, ch):
    _L, _M, H, _c = R.shape(sr, FS)
    for n_mono in (0, 1, 2, H - 1, H, H + 1, 2 * H + 1, 700):
        nv = n_mono if ch == 1 else 2 * n_mono + 1                        # stereo: an unpaired trailing value
        data = payload("s16", nv, seed=sr // 100 + ch)
        y = N.host_pcm_convert(data, N.pcm_desc(sr, ch, "s16", sinc=True))
        m = R.mono(data, sr, ch, "s16")
        want, bound = R.resample(m, sr, FS)
        assert y.size == want.size and np.all(np.abs(y - want) <= bound)
        x = np.frombuffer(data, "<i2").astype(np.float32) / np.float32(32768.0)
        assert bits_equal(y, N.host_resample_sinc(x, sr, FS, ch))


def test_alias_is_gone_and_the_passband_is_kept():
    n = np.arange(100, 1500)
    y = N.host_resample_sinc(R.tone(10000, 48000, 4800), 48000, FS)
    assert np.sqrt(np.mean(y[n].astype(np.float64) ** 2)) < 1e-5          # the definition leaves 1.4e-6, the linear rule 0.354
    y = N.host_resample_sinc(R.tone(3000, 48000, 4800), 48000, FS)
    assert np.max(np.abs(y[n] - 0.5 * np.sin(2 * np.pi * 3000 * n / FS))) < 1e-5


@pytest.mark.parametrize("sr", (11025, 48000))
def test_output_depends_only_on_its_index_and_window(sr):
    L, M, H, _c = R.shape(sr, FS)
    m = R.mono(payload("s16", 2000, seed=5), sr, 1, "s16")
    full = N.host_resample_sinc(m, sr, FS)
    q, cut = 2, N.host_resample_sinc(m[2 * M:], sr, FS)                         # the same outputs, q * L later, where no zero is read
    i0 = -(-(H - 1) * L // M)
    assert cut.size - i0 > 20 and bits_equal(cut[i0:full.size - q * L], full[q * L + i0:][:cut.size - i0])
    want, bound = R.resample(m[q * M:], sr, FS, n_out=8, first=q * L + i0, origin=q * M)
    assert np.all(np.abs(full[q * L + i0:][:8] - want) <= bound)


def test_argument_and_limit_errors():
    lib, n = N.load(), C.c_int64()
    x = np.zeros(8, np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    for bad in (dict(zeros=0), dict(zeros=65), dict(rolloff=0.0), dict(rolloff=1.5), dict(rolloff=float("nan")), dict(beta=-1.0),
                dict(beta=21.0), dict(beta=float("inf"))):
        assert lib.pf_host_resample_sinc(fp, 8, 8000, FS, 1, C.byref(N.resample_config(**bad)), None, 0, C.byref(n)) == N.PF_ERR_INVALID_ARG, bad
    cfg = N.resample_config()
    cfg.struct_size = 8
    assert lib.pf_host_resample_sinc(fp, 8, 8000, FS, 1, C.byref(cfg), None, 0, C.byref(n)) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_resample_sinc(fp, 8, 16001, FS, 1, None, None, 0, C.byref(n)) == N.PF_ERR_UNSUPPORTED            # L = 16000
    assert lib.pf_pcm_num_samples(C.byref(N.pcm_desc(16001, 1, "s16", sinc=True)), FS, 8, C.byref(n)) == N.PF_ERR_UNSUPPORTED
    assert lib.pf_pcm_num_samples(C.byref(N.pcm_desc(16001, 1, "s16")), FS, 8, C.byref(n)) == 0
    wide = N.resample_config(zeros=64, rolloff=0.1)                                                                    # 1280 taps
    assert lib.pf_host_resample_sinc(fp, 8, 8000, FS, 1, C.byref(wide), None, 0, C.byref(n)) == N.PF_ERR_UNSUPPORTED
    assert N.host_resample_sinc(x, 8000, FS, cfg=N.resample_config(zeros=1, rolloff=1.0, beta=0.0)).size == 16


def test_cli_flag():
    base = ["-type", "offline"]
    assert ex.parse_args(base + ["-resample", "sinc", "-intake", "device"])["resample"] == "sinc"
    assert "resample" not in ex.parse_args(base) and ex.parse_args(base + ["-resample", "LINEAR"])["resample"] == "linear"
    with pytest.raises(ValueError):
        ex.parse_args(base + ["-resample", "cubic"])


@pytest.mark.parametrize("sr,ch", ((48000, 2), (11025, 1), (16000, 2)))
def test_flag_clear_is_the_linear_rule_bit_for_bit(sr, ch):
    data = payload("s16", 2001, seed=3)
    want = expected(data, sr, ch, "s16")
    assert bits_equal(N.host_pcm_convert(data, N.pcm_desc(sr, ch, "s16")), want)
    n = C.c_int64()
    for sinc in (False, True):                                            # the length never changes; the flag is inert at 16 kHz
        N.check(N.load().pf_pcm_num_samples(C.byref(N.pcm_desc(sr, ch, "s16", sinc=sinc)), FS, 2001, C.byref(n)))
        assert n.value == want.size
    if sr == FS:
        assert bits_equal(N.host_pcm_convert(data, N.pcm_desc(sr, ch, "s16", sinc=True)), want)
