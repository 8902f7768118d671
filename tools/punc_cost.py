"""What punctuation costs, one GPU job, the released model's dimensions with synthetic weights, the embedding
table at its released size of --vocab = 272727 rows (140 MB in f16 on the device):

  punc                   device time of the profile class `punc` (2 + 2 n_layers launches per round) and the wall clock of
                         Engine.punctuate per call; median with p10 / p90 over --steps calls after --warmup
  two workloads          32 texts of 100 words (5 rounds, windows of 20 .. 100 words with a random network's cuts), and one
                         text of 20 000 words (1000 rounds of ONE window each: the loop is sequential in the cuts)
  floors                 computed here from the windows the loop actually ran: the MFMA time of the padded products (rows padded
                         to 64, keys to 32, queries to 64, classes to 32) at the dense f16 peak of --peak-tflops, and the time to
                         write and read x, q | k | v and ctx once per layer plus one read of the weight image per launch at
                         --hbm-tbs

    python tools/punc_cost.py [--steps 10] [--warmup 3] [--out FILE]"""
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
ap.add_argument("--vocab", type=int, default=272727)
ap.add_argument("--long-words", type=int, default=20000)
ap.add_argument("--peak-tflops", type=float, default=2500.0)
ap.add_argument("--hbm-tbs", type=float, default=8.0)
ap.add_argument("--out", default="")
args = ap.parse_args()


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


def up(x, m):
    return (x + m - 1) // m * m


pcfg = W.ct_transformer_config(vocab=args.vocab)
model = E.load_punc_model(W.pack_pfw(pcfg, W.synth_punc_weights(pcfg, seed=6)))
D, F, NL, P = (pcfg[k] for k in ("d_model", "ffn", "n_layers", "n_punc"))
weight_bytes = model.image_bytes - 2 * args.vocab * D                      # what a forward streams: everything but the embedding table


def floors(rounds):
    """rounds: per round the list of window lengths.  (MFMA ms, traffic ms)"""
    flops = bytes_ = 0.0
    for wins in rounds:
        rows = up(sum(wins), 64)
        flops += rows * (NL * (2.0 * 3 * D * D + 2.0 * D * D + 4.0 * D * F) + 2.0 * D * up(P, 32))
        flops += NL * sum(4.0 * up(t, 64) * up(t, 32) * D for t in wins)
        bytes_ += sum(wins) * NL * (2 * 4 * D + 2 * 2 * 3 * D + 2 * 2 * D) + weight_bytes
    return flops / (args.peak_tflops * 1e12) * 1e3, bytes_ / (args.hbm_tbs * 1e12) * 1e3


def windows_of(ids_list):
    """the windows the device loop runs, round by round (replayed from the device's own marks with the host cut rule)"""
    state = [dict(ids=a, k=0, cache=np.zeros(0, np.int32)) for a in ids_list]
    rounds = []
    while True:
        act = [s for s in state if 20 * s["k"] < len(s["ids"])]
        if not act:
            return rounds
        wins = [np.concatenate([s["cache"], s["ids"][20 * s["k"]: 20 * s["k"] + 20]]) for s in act]
        last = [20 * (s["k"] + 1) >= len(s["ids"]) for s in act]
        _, cut = eng.op_punc_window(wins, last)
        rounds.append([len(w) for w in wins])
        for s, w, c in zip(act, wins, cut):
            s["cache"] = w[c + 1:]
            s["k"] += 1


cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
eng = E.Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
eng.set_punc_model(model)
rng = np.random.default_rng(1)
out = dict(model={k: pcfg[k] for k in ("vocab", "d_model", "heads", "ffn", "kernel", "n_layers", "n_punc")}, image_bytes=model.image_bytes,
           weight_bytes_per_launch_set=weight_bytes, peak_tflops=args.peak_tflops, hbm_tbs=args.hbm_tbs)
for name, texts, steps, warm in (("b32_100_words", [rng.integers(0, args.vocab, 100).astype(np.int32) for _ in range(32)], args.steps, args.warmup),
                                 ("one_text_long", [rng.integers(0, args.vocab, args.long_words).astype(np.int32)], args.steps, 1)):
    rounds = windows_of(texts)
    eng.profile(True)
    dev, wall = [], []
    for it in range(warm + steps):
        eng.profile_reset()
        t = time.perf_counter()
        _, n_rounds = eng.punctuate(texts)
        dt = (time.perf_counter() - t) * 1e3
        ms, n, _ = eng.profile_get("punc")
        assert n_rounds == len(rounds) and n == n_rounds * (2 + 2 * NL), (n_rounds, len(rounds), n)
        if it >= warm:
            dev.append(ms); wall.append(dt)
    eng.profile(False)
    f_mfma, f_bytes = floors(rounds)
    out[name] = dict(texts=len(texts), words=int(sum(len(t) for t in texts)), rounds=len(rounds), launches=len(rounds) * (2 + 2 * NL),
                     window_rows=int(sum(sum(r) for r in rounds)), longest_window=int(max(max(r) for r in rounds)),
                     punc_ms=stats(dev), punctuate_wall_ms=stats(wall), floor_mfma_ms=f_mfma, floor_traffic_ms=f_bytes)
eng.set_punc_model(None)
eng.close()
model.close()
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(line + "\n")
