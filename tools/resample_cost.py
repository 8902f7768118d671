"""What the band-limited resampler costs next to the linear rule: 32 x 30 s through Engine.stage_pcm (upload + the intake launch),
the two rules alternated in one process on the same inputs; medians with p10 / p90 of the launch time between the engine's own
events (Engine.profile) and of the whole staging call on the host clock.

    python tools/resample_cost.py [--batch 32] [--seconds 30] [--steps 20] [--out profiles/resample_cost.json]
    rocprofv3 --kernel-trace --stats -- python tools/resample_cost.py --kernel-only     (kernel times alone, no counters)

Cases: 48 kHz stereo s16, 44.1 kHz mono s16, 8 kHz mono s16.  Beside each: the byte floor (raw bytes read + float bytes
written over the 8.0 TB/s HBM3E peak) and the host twin on one core (ONE utterance timed, scaled to the batch)."""
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
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seconds", type=int, default=30)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
ap.add_argument("--kernel-only", action="store_true")
args = ap.parse_args()
B, HBM_PEAK = args.batch, 8.0e12
CASES = (("48k_stereo_s16", 48000, 2), ("44k1_mono_s16", 44100, 1), ("8k_mono_s16", 8000, 1))

cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)          # the intake does not depend on the model
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
rng = np.random.default_rng(7)


def pct(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))])


report = dict(batch=B, seconds=args.seconds, steps=args.steps, cases={})
for name, sr, ch in CASES:
    datas = [rng.integers(-20000, 20000, args.seconds * sr * ch).astype("<i2") for _ in range(B)]
    descs = {rule: [N.pcm_desc(sr, ch, "s16", sinc=rule == "sinc")] * B for rule in ("linear", "sinc")}
    n_out = eng.pcm_num_samples(descs["sinc"][0], datas[0].size)
    raw_bytes, out_bytes = sum(d.nbytes for d in datas), 4 * n_out * B
    legs = {rule: dict(kernel_us=[], stage_ms=[]) for rule in descs}
    cls = dict(linear="pcm_to_samples", sinc="resample_sinc")
    eng.profile(not args.kernel_only)
    for step in range(args.warmup + args.steps):
        for rule in ("linear", "sinc"):                                        # alternated
            eng.profile_reset()
            t0 = time.perf_counter()
            eng.stage_pcm(datas, descs[rule])
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                legs[rule]["stage_ms"].append(dt * 1e3)
                if not args.kernel_only:
                    legs[rule]["kernel_us"].append(eng.profile_get(cls[rule])[0] * 1e3)
    eng.profile(False)
    t0 = time.perf_counter()
    N.host_pcm_convert(datas[0], descs["sinc"][0])
    host_s = (time.perf_counter() - t0) * B
    case = dict(raw_mb=raw_bytes / 1e6, out_mb=out_bytes / 1e6, byte_floor_us=(raw_bytes + out_bytes) / HBM_PEAK * 1e6,
                host_twin_one_core_s=host_s, outputs=n_out * B)
    for rule, leg in legs.items():
        case[rule] = {k: pct(v) for k, v in leg.items() if v}
    report["cases"][name] = case
    print(name, json.dumps(case))
eng.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
