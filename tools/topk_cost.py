"""What PF_DECODE_TOPK costs: a step of the two bench workloads (paraformer-large 32 x 30 s, sensevoice-small 64 x 10 s;
audio staged, one step in flight) timed in ONE process with the flag clear, with K = 4 and with K = 8, alternating
blocks, medians; the device time of the `topk` and `argmax` classes; and the host n-best for N = 10 over the batch.

    python tools/topk_cost.py [--model paraformer|sensevoice] [--legs 0,4,8] [--steps 20] [--blocks 3]

`--legs 0` alone never touches the top-k API, so the same file also times a build that predates it: run it twice on the
parent commit (the spread) and once here for the flag-clear comparison of DESIGN.md "Top-k and n-best"."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aliparaformerasr_amd import weights as W                     # noqa: E402
from aliparaformerasr_amd.engine import Engine                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="paraformer", choices=("paraformer", "sensevoice"))
ap.add_argument("--legs", default="0,4,8", help="K per leg; 0 = flag clear")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--nbest", type=int, default=10)
args = ap.parse_args()
legs = [int(k) for k in args.legs.split(",")]
sv = args.model == "sensevoice"
B, seconds = (64, 10) if sv else (32, 30)

cfg = W.sensevoice_small_config(use_itn=True) if sv else W.paraformer_large_config()
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
eng.stage_audio([W.synth_audio(seconds * 16000, u) for u in range(B)])


def set_leg(k):
    if legs == [0]:
        return
    from aliparaformerasr_amd import _native as N
    eng.set_decode(N.PF_DECODE_TOPK if k else 0)
    if k:
        eng.set_topk(k)


def step():
    t0 = time.perf_counter()
    eng.run_staged()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


for k in legs:
    set_leg(k)
    for _ in range(args.warmup):
        step()
times = {k: [] for k in legs}
for _ in range(args.blocks):
    for k in legs:
        set_leg(k)
        step()
        times[k] += [step() for _ in range(args.steps)]
out = {"model": args.model, "batch": B, "seconds": seconds, "steps_per_leg": args.steps * args.blocks}
for k in legs:
    t = sorted(times[k])
    out["k_%d" % k] = {"median_ms": round(statistics.median(t), 4), "p10_ms": round(t[len(t) // 10], 4),
                       "p90_ms": round(t[(len(t) * 9) // 10], 4)}
# device time of the kernels the flag touches (event-timed, one untimed step per class and leg)
for k in legs:
    set_leg(k)
    for cls in ("argmax", "topk"):
        eng.profile_reset()
        eng.profile_select(cls)
        eng.profile(True)
        eng.run_staged()
        eng.sync()
        eng.profile(False)
        ms, n, _ = eng.profile_get(cls)
        if n:
            out["k_%d" % k][cls + "_kernel_ms"] = round(ms, 4)
r = eng.fetch()
out["L"] = r.L
if getattr(r, "topk", None) is not None and not sv:
    # the host side of an n-best request: pf_host_nbest for every utterance of the batch
    t0 = time.perf_counter()
    got = 0
    for b in range(B):
        ranks, _ = eng.host_nbest(r.topk.val[b], r.topk.n[b], min(r.L, int(r.token_num[b])), args.nbest)
        got += len(ranks)
    out["host_nbest_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 4)
    out["host_nbest_hypotheses"] = got
print(json.dumps(out))
eng.close()
