"""Shared by tests/test_pcm_cpu.py and tests/test_gpu_pcm.py: RIFF/WAVE blobs of every sample format the intake decodes,
seeded payloads with the corner values, and the expected samples — oracle.audio.decode_wav + resample (the restatement of
AliParaformerAsr.Examples/Utils/AudioHelper.cs pinned by tests/test_harness_cpu.py), nothing else."""
import struct

import numpy as np

from oracle import audio as oa

RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
# name -> (wFormatTag, bits per value)
FORMATS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "f64": (3, 64), "alaw": (6, 8),
           "mulaw": (7, 8)}


def payload(fmt, n, seed=0, nan=False):
    """n seeded finite values of `fmt` as bytes: full scale, zero and — float32 — denormals / — float64 — values that narrow
    to float32 denormals among them (nan=True: float32 NaN payloads too, for the bit copy at the native rate only)."""
    rng = np.random.default_rng([seed, n, sorted(FORMATS).index(fmt)])
    if fmt in ("u8", "alaw", "mulaw"):
        x = rng.integers(0, 256, n).astype(np.uint8)
        x[: min(n, 4)] = np.array([0, 255, 128, 127], np.uint8)[: min(n, 4)]
        return x.tobytes()
    if fmt == "s16":
        x = rng.integers(-32768, 32768, n).astype("<i2")
        x[: min(n, 4)] = np.array([-32768, 32767, 0, 1], "<i2")[: min(n, 4)]
        return x.tobytes()
    if fmt == "s24":
        x = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int64)
        x[: min(n, 4)] = np.array([-(1 << 23), (1 << 23) - 1, 0, -1])[: min(n, 4)]
        return b"".join(struct.pack("<i", int(v))[:3] for v in x)
    if fmt == "s32":
        x = rng.integers(-(1 << 31), 1 << 31, n).astype("<i4")
        x[: min(n, 5)] = np.array([-(1 << 31), (1 << 31) - 1, 0, 1, 16777217], "<i4")[: min(n, 5)]   # 2^24 + 1: rounds in int -> float
        return x.tobytes()
    if fmt == "f32":
        x = rng.uniform(-1, 1, n).astype("<f4")
        special = np.array([1.0, -1.0, 0.0, -0.0, 1e-45, -1e-40, 1.17549421e-38, 3.0e-39], "<f4")
        idx = rng.permutation(n)[: min(n, special.size)]
        x[idx] = special[: idx.size]
        if nan and n:
            bits = x.view("<u4")
            bits[rng.permutation(n)[: max(1, n // 16)]] = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000], "<u4")[rng.integers(0, 4, max(1, n // 16))]
        return x.tobytes()
    x = rng.uniform(-1, 1, n).astype("<f8")
    special = np.array([1.0, -1.0, 0.0, 1e-40, -3e-42, 7.006492321624085e-46, 1.0 + 2.0 ** -24, 0.1], "<f8")   # f32 denormals, a half-way case
    idx = rng.permutation(n)[: min(n, special.size)]
    x[idx] = special[: idx.size]
    return x.tobytes()


def wav_blob(sr, ch, fmt, data, extensible=False, odd_chunk=False, data_size=None, junk=5):
    tag, bits = FORMATS[fmt]
    align = ch * bits // 8
    if extensible:
        fmt_body = struct.pack("<HHIIHH", 0xFFFE, ch, sr, sr * align, align, bits) + struct.pack("<HHI", 22, bits, 3) + \
            struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    else:
        fmt_body = struct.pack("<HHIIHH", tag, ch, sr, sr * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body
    if odd_chunk:
        body += b"LIST" + struct.pack("<I", junk) + b"abcde" * (junk // 5) + b"x" * (junk % 5) + b"\x00" * (junk & 1)   # odd size: a pad byte follows
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def expected(data, sr, ch, fmt, downmix_always=False, fs=16000):
    """What the intake must produce for raw values `data`: decode_wav of the same values in a wav file, then GetFileSample's
    rule (resample + down-mix only off the native rate), or with the flag the same down-mix at the native rate too."""
    blob = wav_blob(sr, ch, fmt, data)
    if not downmix_always and fs == 16000:
        return oa.get_file_sample(blob)[0]
    x, gsr, gch, _dur = oa.decode_wav(blob)
    assert (gsr, gch) == (sr, ch)
    if sr != fs:
        return oa.resample(x, sr, fs, ch)
    if ch == 2:
        n = x.size // 2
        return ((x[0:2 * n:2] + x[1:2 * n:2]) * np.float32(0.5)).astype(np.float32)
    return x


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
