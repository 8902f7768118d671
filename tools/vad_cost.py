"""What the voice-activity segmentation costs for ONE long utterance (default 600 s), in one process:

  vad / fbank   device time of the profile classes `vad` (the two detector launches) and `fbank` (the one batched launch)
                per Engine.vad_segment call: median with p10 / p90 over --steps calls after --warmup
  levels_1h     the segment kernel alone on an hour of levels (360 000 frames, Engine.op_vad_segments; wall clock with the
                upload and the read-back)
  get_results   wall clock of OfflineRecognizer.GetResults of that stream with SetVad on, the stream's audio already on the
                device (a 2 + 2 layer synthetic paraformer: the forwards are NOT the cost of a real model)

Audio: 0.001 N(0, 1) with a 0.3 N(0, 1) burst of 2 - 9 s every 12 s.

    python tools/vad_cost.py [--seconds 600] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from aliparaformerasr_amd import weights as W                     # noqa: E402
from aliparaformerasr_amd.engine import Engine                    # noqa: E402
from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer   # noqa: E402
from oracle import frontend as fe                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=int, default=600)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


rng = np.random.default_rng(1)
audio = (0.001 * rng.standard_normal(16000 * args.seconds)).astype(np.float32)
for k, t0 in enumerate(range(1, args.seconds - 10, 12)):
    n = 16000 * (2 + (3 * k) % 8)
    audio[16000 * t0: 16000 * t0 + n] = np.clip(0.3 * rng.standard_normal(n), -0.999, 0.999).astype(np.float32)

cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=300)
w = W.synth_weights(cfg, seed=77)
cmvn = W.synth_cmvn()
eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=cmvn, device=0)
eng.profile(True)
vad_ms, fb_ms, wall_ms, segs = [], [], [], None
for it in range(args.warmup + args.steps):
    eng.profile_reset()
    t = time.perf_counter()
    segs = eng.vad_segment([audio])[0]
    dt = (time.perf_counter() - t) * 1e3
    v, vn, _ = eng.profile_get("vad")
    f, fn, _ = eng.profile_get("fbank")
    assert vn == 2 and fn == 1, (vn, fn)
    if it >= args.warmup:
        vad_ms.append(v); fb_ms.append(f); wall_ms.append(dt)
eng.profile(False)
hour = np.where((np.arange(360000) // 700) % 2 == 1, 20000, 0).astype(np.int32)
h_ms = []
for it in range(args.warmup + args.steps):
    t = time.perf_counter()
    hs = eng.op_vad_segments([hour])[0]
    if it >= args.warmup:
        h_ms.append((time.perf_counter() - t) * 1e3)
eng.close()

d = tempfile.mkdtemp()
W.save_pfw(os.path.join(d, "model.pfw"), cfg, w)
open(os.path.join(d, "am.mvn"), "w").write(fe.format_mvn_text(*cmvn))
open(os.path.join(d, "asr.yaml"), "w").write("model: paraformer\nfrontend_conf:\n  dither: 0\n")
open(os.path.join(d, "tokens.txt"), "w", encoding="utf-8").write("\n".join("t%d" % i for i in range(300)) + "\n")
rec = OfflineRecognizer(os.path.join(d, "model.pfw"), os.path.join(d, "asr.yaml"), os.path.join(d, "am.mvn"), os.path.join(d, "tokens.txt"))
rec.SetVad(True)
g_ms, n_seg, n_batch = [], 0, 0
for it in range(args.warmup + args.steps):
    s = rec.CreateOfflineStream()
    s.AddSamples(audio)
    t = time.perf_counter()
    rec.GetResults([s])
    if it >= args.warmup:
        g_ms.append((time.perf_counter() - t) * 1e3)
    sg = s.Segments
    n_seg, n_batch = len(sg), 1 + max(g.Batch for g in sg)
rec.Dispose()
out = dict(seconds=args.seconds, frames=int((audio.size + 80) // 160), segments=int(len(segs)), vad_ms=stats(vad_ms), fbank_ms=stats(fb_ms),
           vad_segment_wall_ms=stats(wall_ms), levels_1h_wall_ms=stats(h_ms), levels_1h_segments=int(len(hs)),
           get_results_ms=stats(g_ms), get_results_segments=n_seg, get_results_batches=n_batch)
line = json.dumps(out)
print(line)
if args.out:
    open(args.out, "w").write(line + "\n")
