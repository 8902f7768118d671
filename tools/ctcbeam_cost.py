"""What PF_DECODE_CTC_BEAM costs on the SenseVoice bench workload (sensevoice-small 64 x 10 s, audio staged, one step in
flight), in ONE process: a step with PF_DECODE_TOPK alone and with the beam search behind it, alternating blocks, medians;
the device time of the `ctc_beam` class; and the host twin (pf_host_ctc_beam, one thread) over the same fetched lists and
blank column, compared hypothesis by hypothesis with what the device kept.

    python tools/ctcbeam_cost.py [--settings 16:4,64:8] [--steps 20] [--blocks 3] [--nbest 0] [--class-samples 1] [--hotwords] [--lm]

`--settings` lists W:K pairs (N = W unless --nbest is given).  `--settings none` never touches the beam API and times the
TOPK-alone legs only, so the same file also runs on a build that predates the flag (the parent's step time).
`--class-samples M` event-times a class M times per leg (legs alternating) and reports median / p10 / p90.
`--hotwords` adds per setting a leg with a hot-word set installed (Engine.set_ctc_hotwords: 100 hot words of 2 .. 6 ids drawn
from the unbiased hypotheses of the batch, boost 2): the biased step and `ctc_beam` class beside the unbiased ones in the same
alternation, and the biased host twin (pf_host_ctc_beam_hot) over the same lists (profiles/ctcbeam_hot_cost.json, DESIGN
§4.6f).  Without it nothing of the hot-word API is touched, so the file also runs on a build that predates it.
`--lm` adds per setting two legs with a language model installed (Engine.set_ctc_lm, alpha 0.5, beta 0.5, PF_LM_EOS): two
synthetic 3-gram models made from the unbiased hypotheses of the batch and padded with random n-grams, `lm_small` whose image
fits in the L2 and `lm_large` of at least --lm-large-mb (256) MB; the fused step and `ctc_beam` class beside the unfused ones in
the same alternation, and the fused host twin (pf_host_ctc_beam_lm) over the same lists (profiles/ctcbeam_lm_cost.json, DESIGN
§4.6i).  Without it nothing of the LM API is touched."""
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
ap.add_argument("--settings", default="16:4,64:8")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--nbest", type=int, default=0)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seconds", type=int, default=10)
ap.add_argument("--class-samples", type=int, default=1)
ap.add_argument("--hotwords", action="store_true")
ap.add_argument("--boost", type=float, default=2.0)
ap.add_argument("--lm", action="store_true")
ap.add_argument("--lm-large-mb", type=int, default=256)
args = ap.parse_args()
settings = [] if args.settings == "none" else [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]
B = args.batch

cfg = W.sensevoice_small_config(use_itn=True)
eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 42)), cmvn=W.synth_cmvn(), device=0)
audio = [W.synth_audio(args.seconds * 16000, u) for u in range(B)]
eng.stage_audio(audio)

# legs: ("topk", K), ("beam", W, K) and, with --hotwords, ("hot", W, K)
legs = []
for K in sorted({k for _, k in settings} or {4, 8}):
    legs.append(("topk", K))
legs += [("beam", w, k) for w, k in settings]
hot_sets = {}
if args.hotwords:
    legs += [("hot", w, k) for w, k in settings]
    for w, k in settings:                           # 100 hot words of 2 .. 6 ids out of the unbiased hypotheses of the batch
        eng.set_decode(N.PF_DECODE_CTC_BEAM)
        eng.set_topk(k)
        eng.set_ctc_beam(w, args.nbest or w)
        r = eng.recognize(audio)
        rng = np.random.default_rng(1000 * w + k)
        pool = [h[0] for b in range(B) for h in r.beam.hyps(b) if len(h[0]) >= 2]
        words = []
        while len(words) < 100:
            y = pool[int(rng.integers(len(pool)))]
            ln = int(min(rng.integers(2, 7), len(y)))
            at = int(rng.integers(0, len(y) - ln + 1))
            words.append(tuple(int(c) for c in y[at: at + ln]))
        hot_sets[(w, k)] = words


lms = {}
if args.lm:
    from aliparaformerasr_amd.engine import LanguageModel         # noqa: E402
    legs += [(name, w, k) for w, k in settings for name in ("lm_small", "lm_large")]
    V = cfg["vocab"]
    eng.set_decode(N.PF_DECODE_CTC_BEAM)
    eng.set_topk(settings[0][1])
    eng.set_ctc_beam(settings[0][0], args.nbest or settings[0][0])
    r = eng.recognize(audio)
    hyp = [h[0] for b in range(B) for h in r.beam.hyps(b)]

    def synth_lm(n_random, seed):
        """every id a unigram; the 2- and 3-grams of the batch's unbiased hypotheses; n_random random 3-grams whose contexts are
        drawn from the first 2048 ids (and the 2-grams that are those contexts)"""
        rng = np.random.default_rng(seed)
        uni = np.arange(1, V, dtype=np.int64)
        bi = {(y[p], y[p + 1]) for y in hyp for p in range(len(y) - 1)}
        tri = {(y[p], y[p + 1], y[p + 2]) for y in hyp for p in range(len(y) - 2)}
        ctx_hi = min(2048, V)
        rnd = np.unique(rng.integers(1, ctx_hi, n_random) * V * V + rng.integers(1, ctx_hi, n_random) * V + rng.integers(1, V, n_random))
        t3 = np.unique(np.concatenate([rnd, np.asarray([a * V * V + b * V + c for a, b, c in tri], np.int64)]))
        t2 = np.unique(np.concatenate([t3 // V, np.asarray([a * V + b for a, b in bi], np.int64)]))
        ids = np.concatenate([uni, np.stack([t2 // V, t2 % V], -1).ravel(), np.stack([t3 // (V * V), t3 // V % V, t3 % V], -1).ravel()])
        n = len(uni) + len(t2) + len(t3)
        logp = rng.uniform(-6.0, -0.2, n).astype(np.float32)
        bo = rng.uniform(-1.0, 0.0, n).astype(np.float32)
        return LanguageModel.from_arrays(3, [len(uni), len(t2), len(t3)], ids, logp, bo, V, bos=1, eos=2)
    lms["lm_small"] = synth_lm(40000, 1)                                        # about 2.4 MB: inside one XCD's 4 MB of L2
    lms["lm_large"] = synth_lm(int(args.lm_large_mb * 1024 * 1024 / 13.0), 2)      # 12 bytes an arc and 16 per context: ends above the mark


def set_leg(leg):
    if leg[0] == "topk":
        eng.set_decode(N.PF_DECODE_TOPK)
        eng.set_topk(leg[1])
    else:
        eng.set_decode(N.PF_DECODE_CTC_BEAM)
        eng.set_topk(leg[2])
        eng.set_ctc_beam(leg[1], args.nbest or leg[1])
        if args.hotwords:                           # the table is built and uploaded here, outside every timed step
            eng.set_ctc_hotwords(hot_sets[leg[1:]] if leg[0] == "hot" else [], args.boost if leg[0] == "hot" else 0.0)
        if args.lm:                                 # the image is uploaded once per model (one buffer: a change of model uploads again,
            eng.set_ctc_lm(lms.get(leg[0]), 0.5, 0.5, N.PF_LM_EOS)      # here, outside every timed step)


def leg_name(leg):
    return "topk_k%d" % leg[1] if leg[0] == "topk" else "%s_w%d_k%d" % (leg[0], leg[1], leg[2])


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
out = {"model": "sensevoice", "batch": B, "seconds": args.seconds, "steps_per_leg": args.steps * args.blocks, "legs": {}}
kernel = {}                                         # (leg, class) -> event-timed samples, one untimed step each, legs alternating
for _ in range(max(args.class_samples, 1)):
    for leg in legs:
        set_leg(leg)
        for cls in ("topk",) + (("ctc_beam",) if leg[0] != "topk" else ()):
            ms = class_ms(cls)
            if ms is not None:
                kernel.setdefault((leg, cls), []).append(ms)
for leg in legs:
    t = sorted(times[leg])
    rec = {"median_ms": round(statistics.median(t), 4), "p10_ms": round(t[len(t) // 10], 4), "p90_ms": round(t[(len(t) * 9) // 10], 4)}
    for (lg, cls), v in kernel.items():
        if lg != leg:
            continue
        v = sorted(v)
        rec[cls + "_kernel_ms"] = round(statistics.median(v), 4)
        if len(v) > 1:
            rec[cls + "_kernel_p10_ms"] = round(v[len(v) // 10], 4)
            rec[cls + "_kernel_p90_ms"] = round(v[(len(v) * 9) // 10], 4)
    out["legs"][leg_name(leg)] = rec

# the host twin over the same lists: one forward with the log-probs (for the blank column), utterance by utterance on this thread
for w, k in settings:
    eng.set_decode(N.PF_DECODE_CTC_BEAM)
    eng.set_topk(k)
    nb = args.nbest or w
    eng.set_ctc_beam(w, nb)
    if args.hotwords:
        eng.set_ctc_hotwords([], 0.0)
    if args.lm:
        eng.set_ctc_lm(None)
    r = eng.recognize(audio, want_logits=True)
    rows = [4 + eng.frontend(a).shape[0] for a in audio]
    lb = np.ascontiguousarray(r.logits[:, :, 0])
    del r.logits
    t0 = time.perf_counter()
    host = [eng.host_ctc_beam(lb[b, :rows[b]], r.topk.ids[b, :rows[b]], r.topk.val[b, :rows[b]], r.topk.n[b, :rows[b]], w, nb)
            for b in range(B)]
    host_ms = (time.perf_counter() - t0) * 1e3
    same_ids = sum(host[b].hyps(0) == r.beam.hyps(b) or [h[0] for h in host[b].hyps(0)] == [h[0] for h in r.beam.hyps(b)] for b in range(B))
    worst = 0.0
    for b in range(B):
        for (_, a), (_, c) in zip(host[b].hyps(0), r.beam.hyps(b)):
            worst = max(worst, abs(a - c) / (16 * rows[b] * 2.0 ** -53 * max(1.0, abs(c))))
    out["legs"]["beam_w%d_k%d" % (w, k)].update({
        "host_twin_ms_per_batch": round(host_ms, 3), "L": r.L, "utterances_with_identical_lists": int(same_ids),
        "worst_score_difference_in_tolerances": round(worst, 4), "hypotheses": int(r.beam.n_hyp.sum()),
        "longest_hypothesis": int(r.beam.len.max())})
    for name, lm in lms.items():                    # the fused twin over the same lists, against what the device kept with the model
        eng.set_ctc_lm(lm, 0.5, 0.5, N.PF_LM_EOS)
        rl = eng.recognize(audio)
        t0 = time.perf_counter()
        host = [eng.host_ctc_beam_lm(lb[b, :rows[b]], r.topk.ids[b, :rows[b]], r.topk.val[b, :rows[b]], r.topk.n[b, :rows[b]], w, lm, 0.5,
                                     0.5, N.PF_LM_EOS, n_best=nb) for b in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = changed = 0
        for b in range(B):
            dev = rl.beam.hyps(b)
            same += [h[0] for h in host[b].hyps(0)] == [h[0] for h in dev] and \
                (host[b].lm_sum[0].view(np.uint64) == rl.beam.lm_sum[b].view(np.uint64)).all()
            changed += [h[0] for h in dev] != [h[0] for h in r.beam.hyps(b)]
        out["legs"]["%s_w%d_k%d" % (name, w, k)].update({
            "alpha": 0.5, "beta": 0.5, "eos": True, "order": lm.order, "states": lm.states, "arcs": lm.arcs, "image_bytes": lm.image_bytes,
            "host_twin_ms_per_batch": round(host_ms, 3), "utterances_with_identical_lists_and_lm_sum": int(same),
            "utterances_whose_list_changed": int(changed)})
        eng.set_ctc_lm(None)
    if not args.hotwords:
        continue
    # the biased twin over the same lists, against what the device kept with the set installed
    hot = hot_sets[(w, k)]
    eng.set_ctc_hotwords(hot, args.boost)
    rh = eng.recognize(audio)
    t0 = time.perf_counter()
    host = [eng.host_ctc_beam_hot(lb[b, :rows[b]], r.topk.ids[b, :rows[b]], r.topk.val[b, :rows[b]], r.topk.n[b, :rows[b]], w, hot,
                                  args.boost, nb) for b in range(B)]
    host_ms = (time.perf_counter() - t0) * 1e3
    same = changed = 0
    worst = 0.0
    for b in range(B):
        dev = rh.beam.hyps(b)
        same += [h[0] for h in host[b].hyps(0)] == [h[0] for h in dev] and (host[b].matched[0] == rh.beam.matched[b]).all()
        changed += [h[0] for h in dev] != [h[0] for h in r.beam.hyps(b)]
        for (_, a), (_, c) in zip(host[b].hyps(0), dev):
            worst = max(worst, abs(a - c) / ((16 * rows[b] + 4) * 2.0 ** -53 * max(1.0, abs(c))))
    out["legs"]["hot_w%d_k%d" % (w, k)].update({
        "boost": args.boost, "hot_words": len(hot), "host_twin_ms_per_batch": round(host_ms, 3),
        "utterances_with_identical_lists_and_matched": int(same), "utterances_whose_list_changed": int(changed),
        "worst_score_difference_in_tolerances": round(worst, 4), "matched_tokens_in_the_lists": int(rh.beam.matched.sum())})
print(json.dumps(out))
eng.close()
