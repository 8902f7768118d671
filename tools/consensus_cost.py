"""What the consensus step costs on the device, one GPU job: 32 lists of N hypotheses of 90 .. 110 tokens over
a small alphabet, N = 8 and N = 64.  Per repeat the `consensus` class time (event time of the two launches) and the wall clock
of pf_engine_consensus (upload, launches, copy back); medians with min / max.  Beside them pf_host_consensus over the same
input on one core, and the cell updates the distance tables and the alignments need.  Writes profiles/consensus_cost.json.
Not measured here: where the time goes inside a launch.

    python tools/consensus_cost.py [--repeats 20] [--warmup 3] [--host-lists 32]"""
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


def main(argv):
    opt = lambda k, d: int(argv[argv.index(k) + 1]) if k in argv else d
    repeats, warmup, host_lists = opt("--repeats", 20), opt("--warmup", 3), opt("--host-lists", 32)
    pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = E.Engine(weights=W.pack_pfw(pcfg, W.synth_weights(pcfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    out = dict(workload="32 lists of N hypotheses of 90 .. 110 tokens, alphabet of 40 ids, posterior weights", repeats=repeats, cases=[],
               not_measured="where the time goes inside a launch")
    for n_hyp in (8, 64):
        rng = np.random.default_rng(n_hyp)
        lists = [[rng.integers(0, 40, size=int(n)).astype(np.int32) for n in rng.integers(90, 111, size=n_hyp)] for _ in range(32)]
        weights = [rng.dirichlet(np.ones(n_hyp)) for _ in range(32)]
        cells_dist = sum(len(a) * len(b) for l in lists for i, a in enumerate(l) for b in l[i + 1:])
        wall, cls = [], []
        eng.profile(True)
        for i in range(warmup + repeats):
            eng.profile_reset()
            t0 = time.perf_counter()
            got = eng.consensus(lists, weights, want_D=False)
            t1 = time.perf_counter()
            if i >= warmup:
                wall.append((t1 - t0) * 1e3)
                cls.append(eng.profile_get("consensus")[0])
        launches = eng.profile_get("consensus")[1]
        eng.profile(False)
        cells_align = sum(len(l[g.winner]) * len(b) for l, g in zip(lists, got) for b in l)
        t0 = time.perf_counter()
        host = [E.host_consensus(l, p=w, want_D=False) for l, w in zip(lists[:host_lists], weights[:host_lists])]
        host_ms = (time.perf_counter() - t0) * 1e3 * 32 / host_lists
        assert all(h.winner == g.winner and h.risk.tobytes() == g.risk.tobytes() and h.conf.tobytes() == g.conf.tobytes()
                   for h, g in zip(host, got))
        cls_ms = stat(cls)
        out["cases"].append(dict(N=n_hyp, launches=launches, cells_dist=cells_dist, cells_align=cells_align, consensus_class_ms=cls_ms,
                                 call_wall_ms=stat(wall), host_one_core_ms=host_ms,
                                 cell_updates_per_s=(cells_dist + cells_align) / (cls_ms["median"] * 1e-3)))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.environ.get("CONSENSUS_COST_OUT", os.path.join(ROOT, "profiles", "consensus_cost.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
