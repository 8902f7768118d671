"""CPU: the PCM intake without a device — the new C ABI symbols, pf_pcm_num_samples against the oracle's lengths,
pf_host_wav_info against oracle.audio.decode_wav (every format, EXTENSIBLE, odd chunks, lying sizes, malformed files), the host
form of pf_stream_add_pcm on a stream that belongs to no recognizer, the argument checks, and the `-intake` option of the
examples harness."""
import ctypes as C

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import examples as ex
from oracle import audio as oa
from pcm_ref import FORMATS, RATES, expected, payload, wav_blob

NEW = ("pf_pcm_num_samples", "pf_op_pcm_convert", "pf_stage_pcm", "pf_recognize_pcm", "pf_stream_add_pcm", "pf_host_wav_info")


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_new_symbols_are_exported_and_declared(lib):
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert [N.PCM_FORMATS[k][0] for k in ("u8", "s16", "s24", "s32", "f32", "f64", "alaw", "mulaw")] == list(range(1, 9))
    assert N.PF_PCM_DOWNMIX_ALWAYS == 1 and C.sizeof(N.PfPcmDesc) == 32
    assert lib.pf_version() == 6                      # additions only: the ABI number stays


def _num(lib, sr, ch, n, flag=False, fmt="s16", fs=16000):
    out = C.c_int64(-1)
    N.check(lib.pf_pcm_num_samples(C.byref(N.pcm_desc(sr, ch, fmt, flag)), fs, n, C.byref(out)))
    return out.value


def _oracle_len(sr, ch, n, flag):
    """len(oracle.audio.resample(...)) off the native rate; the decoded (or, with the flag, down-mixed) length at it"""
    if sr != 16000:
        return oa.resample(np.zeros(n, np.float32), sr, 16000, ch).size
    return n // 2 if (ch == 2 and flag) else n


def test_num_samples_equals_the_oracle_lengths(lib):
    for sr in RATES:
        for ch in (1, 2):
            for flag in (False, True):
                for n in (0, 1, 2, 3, 4411, 480001):
                    assert _num(lib, sr, ch, n, flag) == _oracle_len(sr, ch, n, flag), (sr, ch, flag, n)
    # n / ratio on .5 exactly: 32 kHz -> 16 kHz, 5 and 7 mono values -> Round(2.5) = 2, Round(3.5) = 4 (half to even)
    assert (_num(lib, 32000, 1, 5), _num(lib, 32000, 1, 7)) == (2, 4)
    assert _num(lib, 32000, 2, 10) == 2 and _num(lib, 32000, 2, 11) == 2          # the unpaired value is dropped first
    assert oa.resample(np.zeros(5, np.float32), 32000, 16000, 1).size == 2
    # the count does not depend on the sample format
    assert {_num(lib, 44100, 2, 88201, fmt=f) for f in FORMATS} == {_oracle_len(44100, 2, 88201, False)}


def _info(lib, path):
    d = N.PfPcmDesc(); off = C.c_int64(-1); nb = C.c_int64(-1); dur = C.c_double(-1)
    rc = lib.pf_host_wav_info(str(path).encode(), C.byref(d), C.byref(off), C.byref(nb), C.byref(dur))
    return rc, d, off.value, nb.value, dur.value


def test_wav_info_matches_the_oracle_decoder(lib, tmp_path):
    p = tmp_path / "a.wav"
    k = 0
    for fmt in FORMATS:
        for ext in (False, True):
            for odd in (False, True):
                sr, ch = RATES[k % len(RATES)], 1 + k % 2
                k += 1
                data = payload(fmt, 600 + k, seed=k)
                blob = wav_blob(sr, ch, fmt, data, extensible=ext, odd_chunk=odd)
                p.write_bytes(blob)
                rc, d, off, nb, dur = _info(lib, p)
                assert rc == 0, (fmt, ext, odd)
                x, osr, och, odur = oa.decode_wav(blob)
                assert (d.struct_size, d.format, d.sample_rate, d.channels, d.flags) == (32, N.PCM_FORMATS[fmt][0], osr, och, 0)
                assert blob[off: off + nb] == data and abs(dur - odur) < 1e-9
                assert nb // N.PCM_FORMATS[fmt][1] == x.size
                # and the examples' reader hands exactly that payload on
                raw, gsr, gch, gname, gdur = ex.get_file_pcm(str(p))
                assert (gsr, gch, gname, gdur) == (sr, ch, fmt, dur) and raw == data[: len(data) // N.PCM_FORMATS[fmt][1] * N.PCM_FORMATS[fmt][1]]
    # a data chunk that claims more than the file holds is clamped to the file (the host decoder's rule)
    data = payload("s16", 100)
    blob = wav_blob(22050, 2, "s16", data, data_size=0xFFFFFFF0)
    p.write_bytes(blob)
    rc, d, off, nb, dur = _info(lib, p)
    assert rc == 0 and nb == len(data) and blob[off:] == data
    assert abs(dur - oa.decode_wav(blob)[3]) < 1e-9
    # a chunk in front of `data` that is longer than the header region the reader looks at first
    blob = wav_blob(44100, 1, "s24", payload("s24", 50), odd_chunk=True, junk=70001)
    p.write_bytes(blob)
    rc, d, off, nb, dur = _info(lib, p)
    assert rc == 0 and (d.format, d.sample_rate, off, nb) == (N.PF_PCM_S24, 44100, len(blob) - 150, 150)
    assert oa.decode_wav(blob)[0].size == 50
    # NULL outputs are allowed; a missing file, a non-wav and an unsupported format answer a status
    assert lib.pf_host_wav_info(str(p).encode(), None, None, None, None) == 0
    assert lib.pf_host_wav_info(None, None, None, None, None) == N.PF_ERR_INVALID_ARG
    assert _info(lib, tmp_path / "missing.wav")[0] == N.PF_ERR_IO
    p.write_bytes(b"hello, this is not audio at all")
    assert _info(lib, p)[0] == N.PF_ERR_FORMAT
    bad = bytearray(wav_blob(16000, 1, "s16", data)); bad[20:22] = (2).to_bytes(2, "little")      # WAVE_FORMAT_ADPCM
    p.write_bytes(bytes(bad))
    assert _info(lib, p)[0] == N.PF_ERR_UNSUPPORTED


def test_wav_info_survives_malformed_files(lib, tmp_path):
    """The truncations and byte flips of test_wav_reader_survives_malformed_files (tests/test_harness_cpu.py): a status either
    way, consistent with pf_host_wav_read, and a payload that lies inside the file — never a crash."""
    rng = np.random.default_rng(11)
    vals = rng.integers(-3000, 3000, 4000).astype("<i2").tobytes()
    blob = bytearray(wav_blob(22050, 2, "s16", vals)[:36] + b"LIST" + (4).to_bytes(4, "little") + b"abcd" + b"data" +
                     len(vals).to_bytes(4, "little") + vals)
    cases = [bytes(blob[:k]) for k in (0, 3, 11, 12, 19, 20, 35, 36, 43, 44, 45, 60, len(blob) - 1)]
    for _ in range(200):
        b = bytearray(blob)
        for _k in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, 64))] = int(rng.integers(0, 256))
        cases.append(bytes(b))
    big = bytearray(blob); big[52:56] = (0xFFFFFFF0).to_bytes(4, "little")      # data chunk claims 4 GiB
    cases.append(bytes(big))
    p = tmp_path / "m.wav"
    ok = err = 0
    n = C.c_int64(); sr = C.c_int32(); ch = C.c_int32(); dur = C.c_double()
    for c in cases:
        p.write_bytes(c)
        rc, d, off, nb, _dur = _info(lib, p)
        rc_read = lib.pf_host_wav_read(str(p).encode(), None, 0, n, sr, ch, dur)
        # the header walk is shared: what it refuses the reader refuses alike; the reader may refuse more (it also resamples:
        # three channels are a header pf_host_wav_info reports and Resample rejects)
        assert rc == rc_read or (rc == 0 and rc_read == N.PF_ERR_INVALID_ARG)
        if rc == 0:
            ok += 1
            assert 0 <= off and 0 <= nb and off + nb <= len(c)
            assert d.format in range(1, 9) and d.sample_rate > 0 and d.channels > 0
            if rc_read == 0:
                assert (d.sample_rate, d.channels) == (sr.value, ch.value)
        else:
            err += 1
            assert rc in (N.PF_ERR_FORMAT, N.PF_ERR_UNSUPPORTED, N.PF_ERR_IO)
    assert ok > 0 and err > 0


def _unowned_stream(lib):
    h = C.c_void_p()
    N.check(lib.pf_stream_create(None, 0, 0, 0, 0, 0, C.c_float(0.0), None, C.byref(h)))
    return h


def _speech_length(lib, h):
    n = C.c_int32(-1)
    N.check(lib.pf_stream_num_feature_floats(h, C.byref(n)))
    return n.value


def test_public_constructor_stream_takes_pcm_on_the_host(lib):
    """pf_stream_create: no recognizer, no device.  48 kHz stereo s16 through pf_stream_add_pcm reports the SpeechLength that
    AddSamples of the oracle-converted samples reports."""
    data = payload("s16", 2 * 48000 + 1, seed=5)                     # one second, and an unpaired value
    want = expected(data, 48000, 2, "s16")
    assert want.size == 16000
    a, b = _unowned_stream(lib), _unowned_stream(lib)
    raw = np.frombuffer(data, np.uint8)
    N.check(lib.pf_stream_add_pcm(a, raw.ctypes.data, raw.size // 2, C.byref(N.pcm_desc(48000, 2, "s16"))))
    N.check(lib.pf_stream_add_samples(b, want.ctypes.data_as(C.POINTER(C.c_float)), want.size))
    assert _speech_length(lib, a) == _speech_length(lib, b) > 0
    # the quirk and the flag: 16 kHz stereo stays interleaved by default, is halved with PF_PCM_DOWNMIX_ALWAYS
    c, d = _unowned_stream(lib), _unowned_stream(lib)
    N.check(lib.pf_stream_add_pcm(c, raw.ctypes.data, 64000, C.byref(N.pcm_desc(16000, 2, "s16"))))
    N.check(lib.pf_stream_add_pcm(d, raw.ctypes.data, 64000, C.byref(N.pcm_desc(16000, 2, "s16", True))))
    z = np.zeros(64000, np.float32)
    N.check(lib.pf_stream_add_samples(b, z.ctypes.data_as(C.POINTER(C.c_float)), 32000))      # b: 16000 + 32000, two calls
    N.check(lib.pf_stream_add_pcm(a, raw.ctypes.data, 64000, C.byref(N.pcm_desc(16000, 2, "s16", True))))   # a: the same as PCM
    assert _speech_length(lib, a) == _speech_length(lib, b)
    e = _unowned_stream(lib)
    N.check(lib.pf_stream_add_samples(e, z.ctypes.data_as(C.POINTER(C.c_float)), 64000))
    assert _speech_length(lib, c) == _speech_length(lib, e) > _speech_length(lib, d) > 0
    for h in (a, b, c, d, e):
        lib.pf_stream_free(h)


def test_invalid_arguments_answer_statuses(lib):
    out = C.c_int64()
    good = N.pcm_desc(48000, 2, "s16")
    INV = N.PF_ERR_INVALID_ARG

    def num(desc, n=10, fs=16000):
        return lib.pf_pcm_num_samples(C.byref(desc), fs, n, C.byref(out))
    assert num(good) == 0
    assert num(N.pcm_desc(48000, 3, "s16")) == INV and num(N.pcm_desc(48000, 0, "s16")) == INV      # channels: 1 or 2
    assert num(N.pcm_desc(0, 1, "s16")) == INV and num(N.pcm_desc(-8000, 1, "s16")) == INV          # rate
    assert num(N.pcm_desc(48000, 1, 0)) == INV and num(N.pcm_desc(48000, 1, 9)) == INV              # format
    assert num(good, n=1 << 31) == INV and num(good, n=-1) == INV and num(good, n=(1 << 31) - 1) == 0
    assert num(good, fs=0) == INV
    short = N.pcm_desc(48000, 2, "s16"); short.struct_size = 16
    assert num(short) == INV
    assert lib.pf_pcm_num_samples(None, 16000, 1, C.byref(out)) == INV
    assert lib.pf_pcm_num_samples(C.byref(good), 16000, 1, None) == INV
    # null handles answer as their float counterparts do
    assert lib.pf_op_pcm_convert(None, None, 0, C.byref(good), None, 0, C.byref(out)) == lib.pf_stage_audio(None, None, None, 0) == INV
    assert lib.pf_stage_pcm(None, None, None, C.byref(good), 1, 0) == INV
    assert lib.pf_recognize_pcm(None, None, None, C.byref(good), 1, 0, None, 0, None) == lib.pf_recognize(None, None, None, 0, None, 0, None)
    assert lib.pf_stream_add_pcm(None, None, 0, C.byref(good)) == lib.pf_stream_add_samples(None, None, 0) == INV
    # a stream without a device checks its arguments too
    h = _unowned_stream(lib)
    one = np.zeros(8, np.uint8)
    assert lib.pf_stream_add_pcm(h, None, 4, C.byref(good)) == INV                                  # null data with values
    assert lib.pf_stream_add_pcm(h, None, 0, C.byref(good)) == lib.pf_stream_add_samples(h, None, 0) == N.PF_ERR_NULL_SAMPLES
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 4, None) == INV
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 4, C.byref(N.pcm_desc(48000, 3, "s16"))) == INV
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 4, C.byref(N.pcm_desc(0, 1, "s16"))) == INV
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 4, C.byref(N.pcm_desc(8000, 1, 77))) == INV
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 1 << 31, C.byref(good)) == INV
    assert _speech_length(lib, h) == 0                                                               # nothing was added
    lib.pf_stream_dispose(h)
    assert lib.pf_stream_add_pcm(h, one.ctypes.data, 4, C.byref(good)) == N.PF_ERR_DISPOSED
    lib.pf_stream_free(h)
    # the Python helper refuses an array of the wrong dtype instead of reinterpreting it
    with pytest.raises(TypeError):
        N.pcm_bytes(np.zeros(4, np.float64), "s16")
    assert N.pcm_bytes(np.zeros(6, "<i2"), "s16")[1] == 6 and N.pcm_bytes(b"\0" * 7, "s24")[1] == 2


def test_examples_intake_option():
    cfg = ex.parse_args(["-type", "offline", "-intake", "device", "-files", "a.wav"])
    assert cfg["intake"] == "device" and cfg["files"] == ["a.wav"]
    assert ex.parse_args(["-type", "offline", "-intake", "HOST"])["intake"] == "host"
    assert "intake" not in ex.parse_args(["-type", "offline"])          # default: today's host path
    with pytest.raises(ValueError, match="intake"):
        ex.parse_args(["-type", "offline", "-intake", "gpu"])
    with pytest.raises(ValueError, match="intake"):
        ex.parse_args(["-type", "offline", "-intake"])
    with pytest.raises(ValueError, match="Unknown parameters"):
        ex.parse_args(["-type", "offline", "-intakes", "device"])
