"""What a streaming punctuation call costs, one GPU job: the realtime model's dimensions as remembered
(d_model 256, 8 heads, FFN 1024, kernel 11, --layers 3) with synthetic weights, the embedding table at --vocab = 272727 rows.

  punc_stream            device time of the profile class `punc_stream` (ONE launch per call) and the wall clock of
                         pf_op_punc_stream_step per call; median with p10 / p90 over --steps calls after --warmup
  the calls              1, 16 and 64 streams x 3 new words on contexts of 50 and of 190 words, and one stream x 64 words on an
                         empty context; without restarts, so that every call does the same work (a sentence end would make the
                         rows behind it run again); every call starts from a copy of the same seeded states

The wall clock is the stand-alone entry's: it uploads and downloads every stream's whole state block (about 0.8 MB each at three
layers), which a recogniser that keeps the states on the device does not.

    python tools/punc_stream_cost.py [--steps 30] [--warmup 5] [--out FILE]"""
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
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--vocab", type=int, default=272727)
ap.add_argument("--layers", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


pcfg = W.ct_transformer_config(vocab=args.vocab, n_layers=args.layers)
pcfg.update(causal=1, sanm_shift=(pcfg["kernel"] - 1) // 2)
model = E.load_punc_model(W.pack_pfw(pcfg, W.synth_punc_weights(pcfg, seed=6)))
cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
eng = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
eng.set_punc_model(model)
rng = np.random.default_rng(1)
NR = E.PUNC_STREAM_NO_RESTARTS
out = dict(model={k: pcfg[k] for k in ("vocab", "d_model", "heads", "ffn", "kernel", "n_layers", "n_punc")}, image_bytes=model.image_bytes,
           weight_bytes_per_pass=model.image_bytes - 2 * args.vocab * pcfg["d_model"] - 4 * 512 * pcfg["d_model"],
           state_bytes=int(E.punc_stream_state(model).size), calls={})
for B, context, n_new in ((1, 50, 3), (16, 50, 3), (64, 50, 3), (1, 190, 3), (16, 190, 3), (64, 190, 3), (1, 0, 64)):
    seeded = E.punc_stream_state(model, B=B)
    if context:
        eng.op_punc_stream_step(seeded, [rng.integers(0, args.vocab, context).astype(np.int32) for _ in range(B)], flags=NR)
    new = [rng.integers(0, args.vocab, n_new).astype(np.int32) for _ in range(B)]
    eng.profile(True)
    dev, wall = [], []
    for it in range(args.warmup + args.steps):
        st = seeded.copy()
        eng.profile_reset()
        t = time.perf_counter()
        eng.op_punc_stream_step(st, new, flags=NR, want_logits=False)
        dt = (time.perf_counter() - t) * 1e3
        ms, n, _ = eng.profile_get("punc_stream")
        assert n == 1, n
        if it >= args.warmup:
            dev.append(ms); wall.append(dt)
    eng.profile(False)
    out["calls"]["b%d_ctx%d_new%d" % (B, context, n_new)] = dict(streams=B, context=context, new_words=n_new, punc_stream_ms=stats(dev),
                                                              op_wall_ms=stats(wall))
eng.set_punc_model(None)
eng.close()
model.close()
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(line + "\n")
