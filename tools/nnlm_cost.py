"""What a rescoring forward costs on the device, one GPU job: 32 utterances x 8 hypotheses x about 100 tokens
at the released dimensions (V 8404, E 128, D 512, FFN 2048, 16 layers) with synthetic weights.  Per repeat the `nnlm` class
time (event time of the 2 + 2 n_layers launches) and the wall clock of pf_engine_nnlm_score (upload, forward, copy back);
medians with min / max.  Beside them the two floors: the padded products at the dense f16 peak and the weight + activation
traffic at 8 TB/s.  Writes profiles/nnlm_cost.json.  Not measured here: real weights, where the time goes inside a launch.

    python tools/nnlm_cost.py [--repeats 20] [--warmup 3] [--layers 16]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aliparaformerasr_amd import engine as E          # noqa: E402
from aliparaformerasr_amd import weights as W         # noqa: E402

PEAK_F16_TFLOPS, PEAK_TBPS = 2500.0, 8.0               # MI355X: dense f16 MFMA, HBM


def main(argv):
    opt = lambda k, d: int(argv[argv.index(k) + 1]) if k in argv else d
    repeats, warmup, layers = opt("--repeats", 20), opt("--warmup", 3), opt("--layers", 16)
    cfg = W.transformer_lm_config(n_layers=layers)
    model = E.load_nnlm_model(W.pack_pfw(cfg, W.synth_nnlm_weights(cfg, seed=1)))
    pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = E.Engine(weights=W.pack_pfw(pcfg, W.synth_weights(pcfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    eng.set_nnlm(model)
    rng = np.random.default_rng(0)
    hyps = [rng.integers(0, cfg["vocab"], size=int(n)).astype(np.int32) for n in rng.integers(90, 111, size=32 * 8)]
    rows = sum(len(h) + 1 for h in hyps)
    wall, cls = [], []
    eng.profile(True)
    for i in range(warmup + repeats):
        eng.profile_reset()
        t0 = time.perf_counter()
        eng.nnlm_score(hyps, want_logp=False)
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e3)
            cls.append(eng.profile_get("nnlm")[0])
    launches = eng.profile_get("nnlm")[1]
    eng.profile(False)
    V, Ed, D, F = (cfg[k] for k in ("vocab", "embed", "d_model", "ffn"))
    rows_pad, v_pad = (rows + 31) // 32 * 32, (V + 31) // 32 * 32
    flops = 2.0 * rows_pad * (D * Ed + layers * (4 * D * D + 2 * D * F) + v_pad * D)
    # every workgroup streams the weights it multiplies: rows_pad / 32 tiles x the f16 weights; activations x fp32, qkv / ctx f16
    wbytes = 2.0 * (D * Ed + layers * (4 * D * D + 2 * D * F) + v_pad * D)
    traffic_once = wbytes + rows * layers * (2 * 4 * D + 2 * 2 * 3 * D + 2 * 2 * D)
    traffic_tiles = wbytes * (rows_pad // 32) + (traffic_once - wbytes)
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    out = dict(workload="32 x 8 hypotheses of 90 .. 110 tokens, V %d, E %d, D %d, FFN %d, %d layers, synthetic weights" % (V, Ed, D, F, layers),
               rows=rows, launches=launches, repeats=repeats, nnlm_class_ms=stat(cls), call_wall_ms=stat(wall),
               floor_products_ms=flops / (PEAK_F16_TFLOPS * 1e12) * 1e3,
               floor_traffic_weights_once_ms=traffic_once / (PEAK_TBPS * 1e12) * 1e3,
               traffic_weights_per_tile_from_l2_ms_at_hbm_rate=traffic_tiles / (PEAK_TBPS * 1e12) * 1e3,
               not_measured="real weights; where the time goes inside a launch")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.environ.get("NNLM_COST_OUT", os.path.join(ROOT, "profiles", "nnlm_cost.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.set_nnlm(None)
    model.close()
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
