"""What the speaker embedding costs, one GPU job, the released model's dimensions with synthetic weights:

  spk                    device time of the profile class `spk` (15 launches per forward) and the wall clock of
                         Engine.op_spk_embed per call (which includes the copy of the rows to the device and of the embeddings
                         back); median with p10 / p90 over --steps calls after --warmup
  three workloads        32 x 30 s at the default windows (32 x 39 windows of 150 frames), one hour of segments (4800 windows of
                         150 frames, embedded 1024 windows per forward, about what the recogniser's 2 GiB budget allows), a single window
  floors                 computed here: the padded multiply-adds of every product (output positions padded to 64 per window and
                         frequency, channels to 32, K to 16) at the dense f16 peak of --peak-tflops, and the bytes every launch
                         reads and writes once (activations, appended channels, the weight image once per launch) at --hbm-tbs
The affinity of the hour (4800 x 4800 cosines, one launch) is timed on its own.

    python tools/spk_cost.py [--steps 5] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aliparaformerasr_amd import engine as E                      # noqa: E402
from aliparaformerasr_amd import weights as W                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--peak-tflops", type=float, default=2500.0)
ap.add_argument("--hbm-tbs", type=float, default=8.0)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


def up(x, m):
    return (x + m - 1) // m * m


cfg = W.campplus_config()
model = E.load_spk_model(W.pack_pfw(cfg, W.synth_spk_weights(cfg, seed=6)))
m, g, bn, I, Em = (cfg[k] for k in ("m_channels", "growth", "bn_channels", "init_channels", "embedding"))
F0 = cfg["n_mels"]


def floors(n_windows, T):
    """(MFMA ms, traffic ms) of n_windows windows of T frames"""
    Tp = (T + 1) // 2
    flops = bytes_ = 0.0
    F = F0
    convs = [(1, F0, 9)] + [(m, F0 // 2, 9 * m), (m, F0 // 2, 10 * m), (m, F0 // 2, 9 * m), (m, F0 // 2, 9 * m)] + \
            [(m, F0 // 4, 9 * m), (m, F0 // 4, 10 * m), (m, F0 // 4, 9 * m), (m, F0 // 4, 9 * m)] + [(m, F0 // 8, 9 * m)]
    for cin, Fo, K in convs:
        flops += 2.0 * up(Fo * T, 64) * up(m, 32) * up(K, 16)
        bytes_ += 2.0 * Fo * T * m * 2                              # one read of the input (at least), one write of the output
    flops += 2.0 * up(Tp, 64) * up(I, 32) * 5 * up(m * F0 // 8, 16)
    C = I
    for n, _ in zip(cfg["blocks"], cfg["dilations"]):
        for l in range(n):
            flops += 2.0 * up(Tp, 64) * (up(bn, 32) * up(C, 16) + up(g, 32) * 3 * up(bn, 16))
            bytes_ += Tp * (C + g) * 2
            C += g
        flops += 2.0 * up(Tp, 64) * up(C // 2, 32) * up(C, 16)
        bytes_ += Tp * (C + C // 2) * 2
        C //= 2
    flops += 2.0 * 64 * up(Em, 32) * up(2 * C, 16)
    flops *= n_windows
    bytes_ = bytes_ * n_windows + 15.0 * model.image_bytes / 15     # the image once per forward, spread over its launches
    return flops / (args.peak_tflops * 1e12) * 1e3, bytes_ / (args.hbm_tbs * 1e12) * 1e3


pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
eng = E.Engine(weights=W.pack_pfw(pcfg, W.synth_weights(pcfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
eng.set_spk_model(model)
rng = np.random.default_rng(0)
out = {"model": {k: cfg[k] for k in cfg if k != "kind"}, "image_bytes": model.image_bytes, "peak_tflops": args.peak_tflops,
       "hbm_tbs": args.hbm_tbs, "workloads": {}}
emb_hour = None
for name, n_windows, chunk in (("32x30s", 32 * 39, 32 * 39), ("one_hour", 4800, 1024), ("one_window", 1, 1)):
    rows = [(6.0 + 2.0 * rng.standard_normal((150, F0))).astype(np.float32) for _ in range(min(n_windows, chunk))]
    calls = [(c0, min(chunk, n_windows - c0)) for c0 in range(0, n_windows, chunk)]
    dev, wall = [], []
    for it in range(args.warmup + args.steps):
        eng.profile(True)
        eng.profile_reset()
        t0 = time.perf_counter()
        embs = [eng.op_spk_embed(rows[:n]) for _, n in calls]
        t1 = time.perf_counter()
        ms, launches, _ = eng.profile_get("spk")
        eng.profile(False)
        assert launches == 15 * len(calls)
        if it >= args.warmup:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    if name == "one_hour":
        emb_hour = np.concatenate(embs)
    mf, tr = floors(n_windows, 150)
    out["workloads"][name] = {"windows": n_windows, "frames_per_window": 150, "forwards": len(calls), "spk_ms": stats(dev), "wall_ms": stats(wall),
                              "floor_mfma_ms": mf, "floor_traffic_ms": tr, "spk_over_larger_floor": statistics.median(dev) / max(mf, tr)}
    print(name, json.dumps(out["workloads"][name]), flush=True)
aff_dev, aff_wall = [], []
for it in range(args.warmup + args.steps):
    eng.profile(True)
    eng.profile_reset()
    t0 = time.perf_counter()
    eng.op_spk_affinity([emb_hour])
    t1 = time.perf_counter()
    aff_dev.append(eng.profile_get("spk")[0])
    aff_wall.append((t1 - t0) * 1e3)
    eng.profile(False)
n = emb_hour.shape[0]
out["affinity_one_hour"] = {"windows": n, "spk_ms": stats(aff_dev[args.warmup:]), "wall_ms": stats(aff_wall[args.warmup:]),
                            "floor_fp32_ms": 6.0 * Em * n * n / 157e12 * 1e3, "floor_traffic_ms": 4.0 * n * n / (args.hbm_tbs * 1e12) * 1e3}
print("affinity", json.dumps(out["affinity_one_hour"]), flush=True)
out["not_measured"] = ["a real model file", "the recogniser's path end to end on an hour of audio (segmentation, staging and clustering on the host)",
                       "windows of other lengths than 150 frames", "the cost of the LDS bank conflicts of the tiles' row strides",
                       "several engines at once"]
eng.set_spk_model(None)
eng.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
