"""What the speaker clustering costs on the device and on the host, one GPU job:

  device   the two launches of Engine.op_spk_cluster alone (profile class `spk`, event times), median with p10 / p90 over
           --steps calls after --warmup, and the call's wall clock (which includes the copy of the cosines TO the device, a copy
           the recogniser's path does not make);
  host     the wall clock of pf_host_spk_cluster on the same cosines on one core (--host-steps calls; one above 5000 windows);
  shapes   32 streams of 39 windows (32 x 30 s), one stream of 4800 windows (an hour), one of 8192 (the cap);
  data     `all_merge`: random embeddings, num_speakers = 1, so every window merges (n - 1 merges; §4.6m's host figure);
           `clustered`: embeddings around eight centres at the default threshold (the walk stops with eight clusters left).
Every device result is compared with the host's before it is timed.

    python tools/spk_cluster_cost.py [--steps 5] [--warmup 2] [--host-steps 3] [--out FILE]"""
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
ap.add_argument("--host-steps", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


def cosines(n, centres, rng):
    e = rng.standard_normal((n, 192))
    if centres:
        e = rng.standard_normal((centres, 192))[rng.integers(0, centres, n)] + 0.4 * e
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return (e @ e.T).astype(np.float32)


pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
eng = E.Engine(weights=W.pack_pfw(pcfg, W.synth_weights(pcfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
rng = np.random.default_rng(0)
out = {"shapes": {}}
for shape, streams, n in (("32x39", 32, 39), ("1x4800", 1, 4800), ("1x8192", 1, 8192)):
    for data, centres, cfg in (("all_merge", 0, dict(num_speakers=1)), ("clustered", 8, {})):
        S = [cosines(n, centres, rng) for _ in range(streams)]
        host_ms, host = [], None
        for _ in range(1 if n > 5000 else args.host_steps):
            t0 = time.perf_counter()
            host = [E.host_spk_cluster(s, cfg) for s in S]
            host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms, wall_ms = [], []
        for it in range(args.warmup + args.steps):
            eng.profile(True)
            eng.profile_reset()
            t0 = time.perf_counter()
            got = eng.op_spk_cluster(S, cfg, want_trace=False)
            t1 = time.perf_counter()
            ms, launches, _ = eng.profile_get("spk")
            eng.profile(False)
            assert launches == 2
            assert all(g[0].tolist() == h[0].tolist() and g[1] == h[1] for g, h in zip(got, host))
            if it >= args.warmup:
                dev_ms.append(ms)
                wall_ms.append((t1 - t0) * 1e3)
        r = {"streams": streams, "windows": n, "speakers": [h[1] for h in host][:4], "device_spk_ms": stats(dev_ms),
             "device_call_wall_ms": stats(wall_ms), "host_ms": stats(host_ms),
             "host_over_device": statistics.median(host_ms) / statistics.median(dev_ms)}
        out["shapes"]["%s/%s" % (shape, data)] = r
        print(shape, data, json.dumps(r), flush=True)
out["not_measured"] = ["the recogniser's path end to end on an hour of audio (GetResults with and without the switch)",
                       "op_spk_embed + affinity + clustering in one timed sequence: the op's wall clock above uploads the cosines, which the "
                       "recogniser's path never does, so it is an upper bound of what replaces the 92 MB copy back and the host walk",
                       "the two launches one by one", "real embeddings", "several engines at once"]
eng.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
