"""What OnlineRecognizer.SetDeviceFrontend costs per chunk: paraformer-large geometry (synthetic weights), 1 and 32 concurrent
streams fed one 0.6 s chunk per call.  Three recognizers from the same files run the same schedule: SetTokenInfo alone ("host":
fbank per stream in AddSamples, the chunk assembly on the host in GetResults), SetTokenInfo and SetDeviceFrontend ("dev"), and
SetTokenInfo alone again ("host2"), whose difference to the first is the spread of this measurement.  Every chunk is ONE alternated
triple (the order rotates every chunk).  Two windows are clocked, because the fbank moves from the second to the first with the
mode on: (a) GetResults (it ends in a device synchronise) and (b) the AddSamples calls that feed it.  Prints medians and
quartiles; --out FILE also writes them there."""
import os, sys, time, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
from oracle import frontend as fe

d = tempfile.mkdtemp()
cfg = W.paraformer_large_config()
w = W.synth_weights(cfg, 42)
w["predictor.out.bias"] = np.asarray([0.8], np.float32)
W.save_pfw(os.path.join(d, "model.pfw"), cfg, w)
sh, sc = W.synth_cmvn()
open(os.path.join(d, "am.mvn"), "w").write(fe.format_mvn_text(sh, sc))
open(os.path.join(d, "asr.yaml"), "w").write("model: paraformer\nfrontend_conf:\n  dither: 0\n")
open(os.path.join(d, "tokens.txt"), "w").write("\n".join("t%d" % i for i in range(cfg["vocab"])) + "\n")
arms = ["host", "dev", "host2"]
recs = {}
for a in arms:
    recs[a] = OnlineRecognizer(os.path.join(d, "model.pfw"), "", os.path.join(d, "asr.yaml"), os.path.join(d, "am.mvn"), os.path.join(d, "tokens.txt"))
    recs[a].SetTokenInfo(True)
recs["dev"].SetDeviceFrontend(True)
SEC, WARM = 36, 4
lines = []
for n in (1, 32):
    audio = [W.synth_audio(16000 * SEC, u) for u in range(n)]
    streams = {a: [recs[a].CreateOnlineStream() for _ in range(n)] for a in arms}
    t = {a: dict(get=[], add=[], both=[]) for a in arms}
    for k, off in enumerate(range(0, 16000 * SEC, 9600)):
        order = arms[k % 3:] + arms[:k % 3]
        for a in order:
            t0 = time.perf_counter()
            for s, x in zip(streams[a], audio):
                s.AddSamples(x[off: off + 9600])
            t1 = time.perf_counter()
            recs[a].GetResults(streams[a])
            t2 = time.perf_counter()
            if k >= WARM:
                t[a]["add"].append((t1 - t0) * 1e3); t[a]["get"].append((t2 - t1) * 1e3); t[a]["both"].append((t2 - t0) * 1e3)
    same = all(x.Tokens == y.Tokens for x, y in zip(streams["host"], streams["dev"]))
    lines.append("streams %2d, %d timed chunks per arm, tokens per stream %d, ids of dev == host: %s" % (n, len(t["host"]["get"]), len(streams["host"][0].Tokens), same))
    med = {}
    for win, name in (("get", "(a) GetResults"), ("add", "(b) AddSamples"), ("both", "(a) + (b)")):
        for a in arms:
            v = t[a][win]
            med[a, win] = float(np.median(v))
            lines.append("  %-15s %-5s median %.3f ms   quartiles %.3f .. %.3f ms" % (name, a, med[a, win], np.percentile(v, 25), np.percentile(v, 75)))
    lines.append("  (a) + (b): spread of the host arm (|host - host2| medians) %.3f ms;  dev - host: %+.3f ms" %
                 (abs(med["host", "both"] - med["host2", "both"]), med["dev", "both"] - med["host", "both"]))
    del streams
for r in recs.values():
    r.Dispose()
print("\n".join(lines), flush=True)
if "--out" in sys.argv[1:]:
    open(sys.argv[sys.argv.index("--out") + 1], "w").write("\n".join(lines) + "\n")
