"""What the n-best search costs on the paraformer bench workload (paraformer-large 32 x 30 s, audio staged, one step in flight),
in ONE process: a step with PF_DECODE_TOPK alone (today's -nbest path on the device) and with the search behind it — plain, with
hot words, with a small and with a large synthetic language model — alternating blocks, medians with p10 - p90; the device time
of the `nbest_search` class; and on the host, one thread, over the same fetched lists: pf_host_nbest for N = 10 (what today's
-nbest path adds after the step) and the twin pf_host_nbest_search, compared hypothesis by hypothesis with what the device kept.

    python tools/nbest_search_cost.py [--settings 16:4,64:8] [--steps 20] [--blocks 3] [--nbest 10] [--class-samples 5]

`--settings` lists W:K pairs; N = min(--nbest, W).  The hot-word set: 100 words of 2 .. 6 ids drawn from the plain search's
hypotheses of the batch, boost 2.  The models: synthetic 3-gram models made from those hypotheses and padded with random n-grams,
`lm_small` whose image fits in the L2 and `lm_large` of at least --lm-large-mb (256) MB; alpha 0.5, beta 0.5, no end-of-sentence
step.  Weights and audio are synthetic: the numbers say what the kernel costs at these shapes, not what a real model or a real
language model does to the lists (profiles/nbest_search_cost.json)."""
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
from aliparaformerasr_amd.engine import Engine, LanguageModel, host_nbest, host_nbest_search   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--settings", default="16:4,64:8")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--nbest", type=int, default=10)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seconds", type=int, default=30)
ap.add_argument("--class-samples", type=int, default=5)
ap.add_argument("--boost", type=float, default=2.0)
ap.add_argument("--lm-large-mb", type=int, default=256)
args = ap.parse_args()
settings = [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]
B = args.batch

cfg = W.paraformer_large_config()
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
audio = [W.synth_audio(args.seconds * 16000, u) for u in range(B)]
eng.stage_audio(audio)
V = cfg["vocab"]


def n_of(w):
    return min(args.nbest, w)


# the plain search's hypotheses of the batch: what the hot words and the models are made from
eng.set_decode(N.PF_DECODE_TOPK)
eng.set_topk(settings[0][1])
eng.set_nbest_search(settings[0][0], n_of(settings[0][0]))
r = eng.recognize(audio)
hyp = []
for b in range(B):
    nf = min(r.L, int(r.token_num[b]))
    for i in range(int(r.search.n_hyp[b])):
        y = [int(r.topk.ids[b, l, r.search.ranks[b, i, l]]) for l in range(nf)]
        hyp.append([c for c in y if c >= 1])
rng = np.random.default_rng(7)
pool = [y for y in hyp if len(y) >= 2]
hot = []
while len(hot) < 100:
    y = pool[int(rng.integers(len(pool)))]
    ln = int(min(rng.integers(2, 7), len(y)))
    at = int(rng.integers(0, len(y) - ln + 1))
    hot.append(tuple(y[at: at + ln]))


def synth_lm(n_random, seed):
    """every id a unigram; the 2- and 3-grams of the batch's hypotheses; n_random random 3-grams whose contexts are drawn from the
    first 2048 ids (and the 2-grams that are those contexts)"""
    g = np.random.default_rng(seed)
    uni = np.arange(1, V, dtype=np.int64)
    bi = {(y[p], y[p + 1]) for y in hyp for p in range(len(y) - 1)}
    tri = {(y[p], y[p + 1], y[p + 2]) for y in hyp for p in range(len(y) - 2)}
    hi = min(2048, V)
    rnd = np.unique(g.integers(1, hi, n_random) * V * V + g.integers(1, hi, n_random) * V + g.integers(1, V, n_random))
    t3 = np.unique(np.concatenate([rnd, np.asarray([a * V * V + b * V + c for a, b, c in tri], np.int64)]))
    t2 = np.unique(np.concatenate([t3 // V, np.asarray([a * V + b for a, b in bi], np.int64)]))
    ids = np.concatenate([uni, np.stack([t2 // V, t2 % V], -1).ravel(), np.stack([t3 // (V * V), t3 // V % V, t3 % V], -1).ravel()])
    n = len(uni) + len(t2) + len(t3)
    return LanguageModel.from_arrays(3, [len(uni), len(t2), len(t3)], ids, g.uniform(-6.0, -0.2, n).astype(np.float32),
                                     g.uniform(-1.0, 0.0, n).astype(np.float32), V, bos=1, eos=2)


lms = {"lm_small": synth_lm(40000, 1), "lm_large": synth_lm(int(args.lm_large_mb * 1024 * 1024 / 13.0), 2)}
ALPHA, BETA = 0.5, 0.5

legs = [("topk", 0, K) for K in sorted({k for _, k in settings})]
legs += [(name, w, k) for w, k in settings for name in ("search", "hot", "lm_small", "lm_large")]


def set_leg(leg):
    """everything a leg installs (table, image) is uploaded here, outside every timed step"""
    name, w, k = leg
    eng.set_decode(N.PF_DECODE_TOPK)
    eng.set_topk(k)
    if name == "topk":
        eng.set_nbest_search(0)
        return
    eng.set_nbest_search(w, n_of(w))
    eng.set_nbest_hotwords(hot if name == "hot" else [], args.boost if name == "hot" else 0.0)
    eng.set_nbest_lm(lms.get(name), ALPHA, BETA, 0)


def leg_name(leg):
    return "topk_k%d" % leg[2] if leg[0] == "topk" else "%s_w%d_k%d" % leg


def class_ms(cls):
    eng.profile_reset()
    eng.profile_select(cls)
    eng.profile(True)
    eng.run_staged()
    eng.sync()
    eng.profile(False)
    ms, n, _ = eng.profile_get(cls)
    return ms if n else None


def step():
    t0 = time.perf_counter()
    eng.run_staged()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


def spread(v, key=""):
    v = sorted(v)
    return {key + "median_ms": round(statistics.median(v), 4), key + "p10_ms": round(v[len(v) // 10], 4),
            key + "p90_ms": round(v[(len(v) * 9) // 10], 4)}


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
kernel = {}
for _ in range(max(args.class_samples, 1)):
    for leg in legs:
        set_leg(leg)
        for cls in ("topk",) + (("nbest_search",) if leg[0] != "topk" else ()):
            ms = class_ms(cls)
            if ms is not None:
                kernel.setdefault((leg, cls), []).append(ms)
out = {"model": "paraformer-large", "batch": B, "seconds": args.seconds, "steps_per_leg": args.steps * args.blocks, "nbest": args.nbest,
       "alpha": ALPHA, "beta": BETA, "boost": args.boost, "hot_words": len(hot), "legs": {}}
for leg in legs:
    rec = spread(times[leg])
    for (lg, cls), v in kernel.items():
        if lg == leg:
            rec.update(spread(v, cls + "_kernel_"))
    if leg[0].startswith("lm_"):
        lm = lms[leg[0]]
        rec.update({"order": lm.order, "states": lm.states, "arcs": lm.arcs, "image_bytes": lm.image_bytes})
    out["legs"][leg_name(leg)] = rec

# the host side over the same lists, one thread: today's enumeration, and the twin of every search leg against the device
for w, k in settings:
    nb = n_of(w)
    set_leg(("topk", 0, k))
    r = eng.recognize(audio)
    nf = [min(r.L, int(t)) for t in r.token_num]
    t0 = time.perf_counter()
    for b in range(B):
        host_nbest(r.topk.val[b], r.topk.n[b], nf[b], nb)
    out["legs"]["topk_k%d" % k].update({"L": r.L, "token_num_min_max": [int(min(nf)), int(max(nf))],
                                        "host_nbest_n%d_ms_per_batch" % nb: round((time.perf_counter() - t0) * 1e3, 3)})
    base = None
    for name in ("search", "hot", "lm_small", "lm_large"):
        set_leg((name, w, k))
        rd = eng.recognize(audio)
        fuse = dict(lm=lms.get(name), alpha=ALPHA, beta=BETA, hotwords=hot if name == "hot" else (), boost=args.boost if name == "hot" else 0.0)
        t0 = time.perf_counter()
        host = [host_nbest_search(r.topk.ids[b], r.topk.val[b], r.topk.n[b], int(r.token_num[b]), w, nb, **fuse) for b in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = sum(host[b].hyps(0) == rd.search.hyps(b) for b in range(B))
        if name == "search":
            base = rd
        changed = sum(rd.search.ranks[b].tolist() != base.search.ranks[b].tolist() for b in range(B))
        out["legs"]["%s_w%d_k%d" % (name, w, k)].update({
            "n": nb, "host_twin_ms_per_batch": round(host_ms, 3), "utterances_bit_identical_to_the_twin": int(same),
            "utterances_whose_list_differs_from_the_plain_search": int(changed), "matched_tokens_in_the_lists": int(rd.search.matched.sum())})
print(json.dumps(out))
eng.close()
