"""What the FSMN-VAD model score costs, one GPU job, the released model's dimensions with synthetic weights:

  vadnet / vad / fbank   device time of the profile classes per Engine.vad_segment call with the model attached: `vadnet`
                         (the 1 + n_layers launches), `vad` (the segment kernel) and `fbank` (the one batched launch);
                         median with p10 / p90 over --steps calls after --warmup
  two workloads          32 x 30 s of audio, and 4 x 1 h of ROWS (Engine.op_vad_model_levels on caller rows: an hour of samples
                         per stream is 230 MB of float32 to upload, which is not what is being measured; here the wall clock
                         includes the upload of the rows and the read-back of the levels, the class time does not)
  host twin              pf_host_vad_model_levels on one core over --host-frames frames, scaled to the workload, for scale
  floors                 computed here: the MFMA time of the padded products at the dense f16 peak of --peak-tflops, and the
                         time to write and re-read the p rows (fp32 [rows, ldp] per layer) at --hbm-tbs

    python tools/vadnet_cost.py [--steps 10] [--warmup 3] [--hours 4] [--out FILE]"""
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--hours", type=int, default=4)
ap.add_argument("--host-frames", type=int, default=3000)
ap.add_argument("--peak-tflops", type=float, default=2500.0)
ap.add_argument("--hbm-tbs", type=float, default=8.0)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


def up(x, m):
    return (x + m - 1) // m * m


vcfg = W.fsmn_vad_config()
vw = W.synth_vad_weights(vcfg, seed=6)
model = E.load_vad_model(W.pack_pfw(vcfg, vw))
I, A, L, P, O, NL = (vcfg[k] for k in ("input_dim", "affine_dim", "linear_dim", "proj_dim", "output_dim", "n_layers"))
prods = [(A, I), (L, A)] + [(P, L), (L, P)] * NL + [(A, L), (O, A)]
flops_row = sum(2.0 * up(n, 32) * up(k, 16) for n, k in prods)          # the padded products, per frame
p_bytes_row = 2.0 * 4 * up(P, 32) * NL                                     # every p row is written once and read once (halo aside)

cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
eng = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
eng.set_vad_model(model)
vc = E.vad_model_config()
out = dict(model=dict(vcfg, sil_ids=list(vcfg["sil_ids"])), image_bytes=model.image_bytes, flops_per_frame_padded=flops_row,
           p_bytes_per_frame=p_bytes_row, peak_tflops=args.peak_tflops, hbm_tbs=args.hbm_tbs)

# ---- 32 x 30 s of audio through vad_segment
rng = np.random.default_rng(1)
audio = []
for u in range(32):
    a = (0.001 * rng.standard_normal(16000 * 30)).astype(np.float32)
    for t0 in range(1, 25, 8):
        n = 16000 * (2 + (u + t0) % 4)
        a[16000 * t0: 16000 * t0 + n] = np.clip(0.3 * rng.standard_normal(n), -0.999, 0.999).astype(np.float32)
    audio.append(a)
frames = 32 * 3000
eng.profile(True)
net, vad, fb, wall = [], [], [], []
for it in range(args.warmup + args.steps):
    eng.profile_reset()
    t = time.perf_counter()
    eng.vad_segment(audio, vc)
    dt = (time.perf_counter() - t) * 1e3
    n_ms, n_n, _ = eng.profile_get("vadnet")
    v_ms, v_n, _ = eng.profile_get("vad")
    f_ms, f_n, _ = eng.profile_get("fbank")
    assert (n_n, v_n, f_n) == (1 + NL, 1, 1), (n_n, v_n, f_n)
    if it >= args.warmup:
        net.append(n_ms); vad.append(v_ms); fb.append(f_ms); wall.append(dt)
out["b32_30s"] = dict(frames=frames, vadnet_ms=stats(net), vad_ms=stats(vad), fbank_ms=stats(fb), vad_segment_wall_ms=stats(wall),
                      floor_mfma_ms=frames * flops_row / (args.peak_tflops * 1e12) * 1e3,
                      floor_p_traffic_ms=frames * p_bytes_row / (args.hbm_tbs * 1e12) * 1e3)

# ---- hours of rows through the op (the launches are the same; the rows are the caller's)
rows = [(rng.standard_normal((360000, 80)) * 3 - 4).astype(np.float32) for _ in range(args.hours)]
frames = 360000 * args.hours
net, wall = [], []
for it in range(max(args.warmup // 2, 1) + max(args.steps // 2, 3)):
    eng.profile_reset()
    t = time.perf_counter()
    lev = eng.op_vad_model_levels(rows)
    dt = (time.perf_counter() - t) * 1e3
    n_ms, n_n, _ = eng.profile_get("vadnet")
    assert n_n == 1 + NL
    if it >= max(args.warmup // 2, 1):
        net.append(n_ms); wall.append(dt)
eng.profile(False)
out["hours_of_rows"] = dict(streams=args.hours, frames=frames, vadnet_ms=stats(net), op_wall_ms=stats(wall),
                            floor_mfma_ms=frames * flops_row / (args.peak_tflops * 1e12) * 1e3,
                            floor_p_traffic_ms=frames * p_bytes_row / (args.hbm_tbs * 1e12) * 1e3)
eng.set_vad_model(None)
eng.close()

# ---- the host twin on one core
x = rows[0][: args.host_frames]
t = time.perf_counter()
host = E.host_vad_model_levels(model, x)
host_ms = (time.perf_counter() - t) * 1e3
out["host_twin"] = dict(frames=int(x.shape[0]), ms=host_ms, ms_per_hour_of_audio=host_ms * 360000 / x.shape[0],
                        max_level_difference_to_device=int(np.abs(host.astype(np.int64) - lev[0][: x.shape[0]]).max()))
model.close()
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(line + "\n")
