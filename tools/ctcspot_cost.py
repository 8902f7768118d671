"""What phrase spotting (Engine.set_spotter, csrc/k_ctcspot.hip) costs on the SenseVoice bench workload (sensevoice-small
64 x 10 s, audio staged, one step in flight), in ONE process, legs alternating block by block, medians with quartiles:

  plain    no phrase list: the forward as the parent commit runs it (nothing of this feature is launched or allocated)
  spot16   16 phrases of 4 tokens
  spot256  256 phrases of 4 tokens

plus the device time of the `ctc_spot` class per leg and the number of hits.  The phrases are windows of the utterances' greedy
labelings and random ids, half each, so some of them do occur.

    python tools/ctcspot_cost.py [--steps 20] [--blocks 3] [--threshold 0.5]

`--legs none` never touches the spotting API and times `plain` only, so the same file also runs on the parent commit: the
baseline is that run, never this code against itself."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aliparaformerasr_amd import _native as N                     # noqa: E402
from aliparaformerasr_amd import weights as W                     # noqa: E402
from aliparaformerasr_amd.engine import Engine                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="all")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seconds", type=int, default=10)
ap.add_argument("--threshold", type=float, default=0.5)
args = ap.parse_args()
B = args.batch

cfg = W.sensevoice_small_config(use_itn=True)
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
audio = [W.synth_audio(args.seconds * 16000, u) for u in range(B)]
eng.set_decode(N.PF_DECODE_CTC)
r = eng.recognize(audio)
greedy = [[int(v) for v in r.ctc.ids[b, : r.ctc.n[b]]] for b in range(B)]
eng.set_decode(0)
eng.stage_audio(audio)
rng = np.random.default_rng(1)


def phrases(n):
    out = []
    for i in range(n):
        g = greedy[i % B]
        if i % 2 == 0 and len(g) >= 4:
            s = int(rng.integers(0, len(g) - 3))
            out.append(g[s: s + 4])
        else:
            out.append([int(v) for v in rng.integers(1, eng.vocab, size=4)])
    return out


lists = {"plain": None, "spot16": phrases(16), "spot256": phrases(256)}
legs = ["plain"] + (["spot16", "spot256"] if args.legs == "all" else [])


def set_leg(leg):
    if args.legs == "all":
        eng.set_spotter(lists[leg], math.log(args.threshold), 8)


def step():
    t0 = time.perf_counter()
    eng.run_staged()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


for leg in legs:
    set_leg(leg)
    for _ in range(args.warmup):
        step()
times = {leg: [] for leg in legs}
for _ in range(args.blocks):
    for leg in legs:
        set_leg(leg)
        step()
        times[leg] += [step() for _ in range(args.steps)]
out = {"model": "sensevoice", "batch": B, "seconds": args.seconds, "steps_per_leg": args.steps * args.blocks,
       "threshold": args.threshold, "legs": {}}
for leg in legs:
    q = statistics.quantiles(times[leg], n=4)
    rec = {"median_ms": round(q[1], 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4)}
    if lists[leg]:
        set_leg(leg)
        eng.profile_reset()                                       # event-timed, one untimed step
        eng.profile_select("ctc_spot")
        eng.profile(True)
        step()
        eng.profile(False)
        ms, n, _ = eng.profile_get("ctc_spot")
        rec["ctc_spot_kernel_ms"] = round(ms, 4)
        res = eng.recognize(audio)
        rec["hits"] = int(res.spot.n_hits.sum())
        rec["L"] = res.L
        eng.stage_audio(audio)
    out["legs"][leg] = rec
print(json.dumps(out))
eng.close()
