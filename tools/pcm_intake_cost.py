"""What the PCM intake costs and saves: 32 x 30 s through ONE recognizer with ONE caller (the flagship model of bench.py,
`CreateOfflineStream` + add + `GetResults` + texts per batch), legs alternated in one process, medians and the spread of the
repeated legs (p10 / p90 over all timed batches of a leg).

    python tools/pcm_intake_cost.py [--batch 32] [--seconds 30] [--steps 10] [--blocks 3] [--layers E,D]

  (a) 16 kHz mono:   float   AddSamples(float32)                     — the parent's via_recognizer one-caller figure, re-measured
                     pcm16   AddPcm(s16)                              — half the upload, converted on the device
  (b) 48 kHz stereo s16 wav files (page cache):
                     host    pf_host_wav_read (decode + Resample on the host, one call into a sized buffer) + AddSamples
                     device  pf_host_wav_info + payload read + AddPcm — what `examples.py -intake device` does
                     devmem  AddPcm of the payload already in memory  — PCM off a socket
  The four audio forms hold the same utterances; every leg must give the ids of its float counterpart.
  (c) the kernel alone: run under `rocprofv3 --kernel-trace --stats -- python tools/pcm_intake_cost.py --kernel-only`, which
      converts the (b) batch with pf_stage_pcm a few times; the line printed gives the byte floor: raw bytes read + float
      bytes written over the 8.0 TB/s HBM3E peak."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aliparaformerasr_amd import _native as N                     # noqa: E402
from aliparaformerasr_amd import weights as W                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seconds", type=int, default=30)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layers", default="", help="E,D: a smaller model (the audio path does not depend on it)")
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
B, HBM_PEAK = args.batch, 8.0e12
lib = N.load()


def i16(x):
    return np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype("<i2")


def wav16(path, pcm, sr, ch):
    import struct
    body = pcm.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, sr, sr * 2 * ch, 2 * ch, 16) + b"data" + struct.pack("<I", len(body)) + body)


kw = {}
if args.layers:
    e, d = (int(v) for v in args.layers.split(","))
    kw = dict(enc_layers=e, dec_layers=d)
cfg = W.paraformer_large_config(**kw)
weights = W.synth_weights(cfg, 42)
tmp = tempfile.TemporaryDirectory(prefix="pf_pcm_cost_")
# the 48 kHz stereo recordings, and what a 16 kHz mono caller would hold of the same utterances: the host conversion of them
t48 = np.arange(args.seconds * 48000) / 48000.0
pcm48, files = [], []
for u in range(B):
    rng = np.random.default_rng(1234 + u)
    x = 0.1 * rng.standard_normal(t48.size)
    for _ in range(3):
        x = x + rng.uniform(0.05, 0.2) * np.sin(2 * np.pi * rng.uniform(100.0, 4000.0) * t48 + rng.uniform(0, 2 * np.pi))
    x = np.clip(x, -0.999, 0.999)
    p = i16(np.stack([x, 0.8 * x], 1).reshape(-1))
    pcm48.append(p)
    files.append(os.path.join(tmp.name, "u%02d.wav" % u))
    wav16(files[-1], p, 48000, 2)
n16 = args.seconds * 16000
desc48, desc16 = N.pcm_desc(48000, 2, "s16"), N.pcm_desc(16000, 1, "s16")


def host_read(path, buf):
    n = C.c_int64()
    N.check(lib.pf_host_wav_read(path.encode(), buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, n, None, None, None))
    return n.value


bufs = [np.zeros(n16 + 8, np.float32) for _ in range(B)]
flt48 = []
for u in range(B):
    assert host_read(files[u], bufs[u]) == n16
    flt48.append(bufs[u][:n16].copy())
pcm16 = [i16(a) for a in flt48]                                   # (a): the same utterances as a 16 kHz mono caller holds them
flt16 = [(p.astype(np.float32) / np.float32(32768.0)).astype(np.float32) for p in pcm16]

if args.kernel_only:
    from aliparaformerasr_amd.engine import Engine
    eng = Engine(weights=W.pack_pfw(cfg, weights), cmvn=W.synth_cmvn(), device=0)
    for _ in range(5):
        eng.stage_pcm(pcm48, desc48)
        eng.stage_pcm(pcm16, desc16)
    raw48, raw16, out = sum(p.nbytes for p in pcm48), sum(p.nbytes for p in pcm16), B * n16 * 4
    print(json.dumps({"kernel": "pcm_to_samples_kernel", "batch": B, "seconds": args.seconds,
                      "s16_48k_stereo": {"bytes_read": raw48, "bytes_written": out, "floor_us_at_8TBs": round((raw48 + out) / HBM_PEAK * 1e6, 2)},
                      "s16_16k_mono": {"bytes_read": raw16, "bytes_written": out, "floor_us_at_8TBs": round((raw16 + out) / HBM_PEAK * 1e6, 2)}}))
    eng.close()
    sys.exit(0)

paths = W.synth_model_dir(tmp.name, cfg, weights, W.synth_cmvn())
rh = C.c_void_p()
N.check(lib.pf_recognizer_create(paths["model"].encode(), paths["config"].encode(), paths["mvn"].encode(), paths["tokens"].encode(),
                                 b"", b"", 1, 1, 0, C.byref(rh)))


def add_float(h, u):
    N.check(lib.pf_stream_add_samples(h, flt16[u].ctypes.data_as(C.POINTER(C.c_float)), n16))


def add_pcm16(h, u):
    N.check(lib.pf_stream_add_pcm(h, pcm16[u].ctypes.data, n16, C.byref(desc16)))


def add_host48(h, u):
    n = host_read(files[u], bufs[u])
    N.check(lib.pf_stream_add_samples(h, bufs[u].ctypes.data_as(C.POINTER(C.c_float)), n))


def add_device48(h, u):
    d = N.PfPcmDesc(); off = C.c_int64(); nb = C.c_int64()
    N.check(lib.pf_host_wav_info(files[u].encode(), C.byref(d), C.byref(off), C.byref(nb), None))
    with open(files[u], "rb") as f:
        f.seek(off.value)
        raw = np.frombuffer(f.read(nb.value), np.uint8)
    N.check(lib.pf_stream_add_pcm(h, raw.ctypes.data, raw.size // 2, C.byref(d)))


def add_devmem48(h, u):
    N.check(lib.pf_stream_add_pcm(h, pcm48[u].ctypes.data, pcm48[u].size, C.byref(desc48)))


LEGS = {"a_float": add_float, "a_pcm16": add_pcm16, "b_host": add_host48, "b_device": add_device48, "b_devmem": add_devmem48}


def one_batch(add):
    t0 = time.perf_counter()
    hs = (C.c_void_p * B)()
    for u in range(B):
        h = C.c_void_p()
        N.check(lib.pf_recognizer_create_stream(rh, C.byref(h)))
        hs[u] = h
        add(h, u)
    ta = time.perf_counter()
    N.check(lib.pf_recognizer_get_results(rh, hs, B))
    ids = []
    for u in range(B):
        txt = C.c_char_p(); tl = C.c_int32()
        N.check(lib.pf_result_text(rh, u, C.byref(txt), tl))
        p = C.POINTER(C.c_int64)(); n = C.c_int32()
        N.check(lib.pf_stream_tokens(C.c_void_p(hs[u]), C.byref(p), n))
        ids.append(np.frombuffer(C.string_at(p, n.value * 8), dtype=np.int64))
        lib.pf_stream_free(C.c_void_p(hs[u]))
    t1 = time.perf_counter()
    return (t1 - t0) * 1e3, (ta - t0) * 1e3, ids


ref = {}
for name, add in LEGS.items():
    for _ in range(args.warmup):
        _ms, _add, ids = one_batch(add)
    ref[name] = ids
for a_, b_ in (("a_pcm16", "a_float"), ("b_host", "b_device"), ("b_devmem", "b_device")):
    assert all(np.array_equal(x, y) for x, y in zip(ref[a_], ref[b_])), (a_, b_)
times = {k: [] for k in LEGS}
adds = {k: [] for k in LEGS}
for _ in range(args.blocks):
    for name, add in LEGS.items():
        one_batch(add)                                             # (first batch after a switch of legs is not timed)
        for _s in range(args.steps):
            ms, add_ms, _ids = one_batch(add)
            times[name].append(ms)
            adds[name].append(add_ms)
out = {"batch": B, "seconds": args.seconds, "batches_per_leg": args.steps * args.blocks, "model_layers": args.layers or "full"}
for k in LEGS:
    t = sorted(times[k])
    out[k] = {"median_ms": round(statistics.median(t), 3), "p10_ms": round(t[len(t) // 10], 3), "p90_ms": round(t[(len(t) * 9) // 10], 3),
              "add_median_ms": round(statistics.median(adds[k]), 3)}
print(json.dumps(out))
lib.pf_recognizer_free(rh)
