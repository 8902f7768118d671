"""What the decode flags cost: the SenseVoice step of bench.py (sensevoice-small, 64 x 10 s, audio staged, one step in
flight) timed in ONE process with flags 0 and with flags 3 (PF_DECODE_SCORES | PF_DECODE_CTC), alternating blocks, medians.

    python tools/ctc_decode_cost.py [--flags 0,3] [--steps 30] [--blocks 3] [--batch 64] [--seconds 10]

`--flags 0` alone never touches the decode API, so the same file also times a build that predates it (the flags-0
against-parent comparison of DESIGN.md "CTC decoding")."""
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
ap.add_argument("--flags", default="0,3")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seconds", type=int, default=10)
args = ap.parse_args()
flag_list = [int(f) for f in args.flags.split(",")]

cfg = W.sensevoice_small_config(use_itn=True)
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
eng.stage_audio([W.synth_audio(args.seconds * 16000, u) for u in range(args.batch)])


def set_flags(f):
    if flag_list != [0]:
        eng.set_decode(f)


def step():
    t0 = time.perf_counter()
    eng.run_staged()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


for f in flag_list:
    set_flags(f)
    for _ in range(args.warmup):
        step()
times = {f: [] for f in flag_list}
for _ in range(args.blocks):
    for f in flag_list:
        set_flags(f)
        step()
        times[f] += [step() for _ in range(args.steps)]
out = {"batch": args.batch, "seconds": args.seconds, "steps_per_flag": args.steps * args.blocks}
for f in flag_list:
    t = sorted(times[f])
    out["flags_%d" % f] = {"median_ms": round(statistics.median(t), 4), "p10_ms": round(t[len(t) // 10], 4),
                           "p90_ms": round(t[(len(t) * 9) // 10], 4)}
# device time of the two kernels the flags touch (event-timed, one untimed step per class and flag)
for f in flag_list:
    set_flags(f)
    for cls in ("argmax", "ctc_collapse"):
        eng.profile_reset()
        eng.profile_select(cls)
        eng.profile(True)
        eng.run_staged()
        eng.sync()
        eng.profile(False)
        ms, n, _ = eng.profile_get(cls)
        if n:
            out["flags_%d" % f][cls + "_kernel_ms"] = round(ms, 4)
r = eng.fetch()
out["L"] = r.L
if r.ctc is not None:
    out["ctc_tokens_max"] = int(r.ctc.n.max())
print(json.dumps(out))
eng.close()
