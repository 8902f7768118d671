"""What PF_DECODE_ALIGN costs on the SenseVoice bench workload (sensevoice-small 64 x 10 s, audio staged, one step in
flight), in ONE process, legs alternating, medians with p10 / p90:

  scores       PF_DECODE_SCORES alone
  align_h1     PF_DECODE_ALIGN with the greedy labeling of every utterance as its target (H = 1 job per utterance)
  beam         PF_DECODE_CTC_BEAM alone at W:K (default 16:4), N = W
  beam_align   the same with PF_DECODE_ALIGN: the N hypotheses aligned (H = N)

plus the device time of the `ctc_align` class per leg, and the host twin (pf_host_ctc_align, one thread) over the same rows and
targets, compared job by job with what the device returned.

    python tools/ctcalign_cost.py [--beam 16:4] [--steps 20] [--blocks 3]

`--legs none` never touches the alignment API and times `scores` and `beam` only, so the same file also runs on a build that
predates the flag (the parent's step times)."""
import argparse
import json
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
ap.add_argument("--beam", default="16:4")
ap.add_argument("--legs", default="all")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seconds", type=int, default=10)
args = ap.parse_args()
Wd, K = (int(x) for x in args.beam.split(":"))
B = args.batch
ALIGN = getattr(N, "PF_DECODE_ALIGN", 0) if args.legs == "all" else 0

cfg = W.sensevoice_small_config(use_itn=True)
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
audio = [W.synth_audio(args.seconds * 16000, u) for u in range(B)]

# the greedy labelings, once
eng.set_decode(N.PF_DECODE_CTC)
r = eng.recognize(audio)
greedy = [[int(v) for v in r.ctc.ids[b, : r.ctc.n[b]]] for b in range(B)]
eng.stage_audio(audio)
legs = ["scores", "beam"] + (["align_h1", "beam_align"] if ALIGN else [])


def set_leg(leg):
    eng.set_decode({"scores": N.PF_DECODE_SCORES, "align_h1": ALIGN, "beam": N.PF_DECODE_CTC_BEAM,
                    "beam_align": N.PF_DECODE_CTC_BEAM | ALIGN}[leg])
    if leg.startswith("beam"):
        eng.set_topk(K)
        eng.set_ctc_beam(Wd, Wd)


def step(leg):
    t0 = time.perf_counter()
    if leg == "align_h1":
        eng.set_align_targets(greedy)                             # consumed by the forward: part of the step
    eng.run_staged()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


for leg in legs:
    set_leg(leg)
    for _ in range(args.warmup):
        step(leg)
times = {leg: [] for leg in legs}
for _ in range(args.blocks):
    for leg in legs:
        set_leg(leg)
        step(leg)
        times[leg] += [step(leg) for _ in range(args.steps)]
out = {"model": "sensevoice", "batch": B, "seconds": args.seconds, "steps_per_leg": args.steps * args.blocks, "beam": args.beam,
       "longest_greedy_labeling": max(len(g) for g in greedy), "legs": {}}
for leg in legs:
    t = sorted(times[leg])
    rec = {"median_ms": round(statistics.median(t), 4), "p10_ms": round(t[len(t) // 10], 4), "p90_ms": round(t[(len(t) * 9) // 10], 4)}
    set_leg(leg)
    for cls in [c for c in ("ctc_beam", "ctc_align") if (c == "ctc_beam" and leg.startswith("beam")) or (c == "ctc_align" and "align" in leg)]:
        eng.profile_reset()                                       # event-timed, one untimed step per class
        eng.profile_select(cls)
        eng.profile(True)
        step(leg)
        eng.profile(False)
        ms, n, _ = eng.profile_get(cls)
        if n:
            rec[cls + "_kernel_ms"] = round(ms, 4)
    out["legs"][leg] = rec

# the host twin over the same rows: one forward with the log-probs, job by job on this thread
if ALIGN:
    rows = [4 + eng.frontend(a).shape[0] for a in audio]
    for leg in ("align_h1", "beam_align"):
        set_leg(leg)
        if leg == "align_h1":
            eng.set_align_targets(greedy)
        r = eng.recognize(audio, want_logits=True)
        al = r.align
        jobs = []
        for b in range(B):
            if leg == "align_h1":
                jobs.append((b, 0, greedy[b]))
            else:
                jobs += [(b, i, list(ids)) for i, (ids, _) in enumerate(r.beam.hyps(b))]
        t0 = time.perf_counter()
        host = [eng.host_ctc_align(r.logits[b, : rows[b]], y) for b, _, y in jobs]
        host_ms = (time.perf_counter() - t0) * 1e3
        same, worst = 0, 0.0
        for (b, h, y), g in zip(jobs, host):
            U = len(y)
            same += (g.path_score[0, 0].tobytes() == al.path_score[b, h].tobytes() and int(g.ok[0, 0]) == int(al.ok[b, h])
                     and (g.first[0, 0] == al.first[b, h, :U]).all() and (g.last[0, 0] == al.last[b, h, :U]).all()
                     and g.tok_score[0, 0].tobytes() == al.tok_score[b, h, :U].tobytes())
            ref = float(g.loglik[0, 0])
            if np.isfinite(ref):
                worst = max(worst, abs(float(al.loglik[b, h]) - ref) / (16 * rows[b] * 2.0 ** -53 * max(1.0, abs(ref))))
        out["legs"][leg].update({"host_twin_ms_per_batch": round(host_ms, 3), "L": r.L, "jobs": len(jobs),
                                 "jobs_identical_to_the_twin": int(same), "worst_loglik_difference_in_tolerances": round(worst, 4),
                                 "longest_target": max(len(y) for _, _, y in jobs)})
        del r
print(json.dumps(out))
eng.close()
