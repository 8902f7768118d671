"""What OnlineRecognizer.SetTokenInfo costs per GetResults: paraformer-large geometry (synthetic weights), 1 and 32 concurrent
streams fed one 0.6 s chunk per call.  Three recognizers from the same files run the same schedule: the mode off (the path as it
is without the feature), the mode on, and the mode off again, whose difference to the first is the spread of this measurement.
Every chunk is ONE alternated triple (the order rotates every chunk); only GetResults is inside the clock (it ends in a device
synchronise), AddSamples (the fbank call) is outside.  Prints medians; --out FILE also writes them there."""
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
arms = ["off", "on", "off2"]
recs = {}
for a in arms:
    recs[a] = OnlineRecognizer(os.path.join(d, "model.pfw"), "", os.path.join(d, "asr.yaml"), os.path.join(d, "am.mvn"), os.path.join(d, "tokens.txt"))
recs["on"].SetTokenInfo(True)
SEC, WARM = 36, 4
lines = []
for n in (1, 32):
    audio = [W.synth_audio(16000 * SEC, u) for u in range(n)]
    streams = {a: [recs[a].CreateOnlineStream() for _ in range(n)] for a in arms}
    t = {a: [] for a in arms}
    for k, off in enumerate(range(0, 16000 * SEC, 9600)):
        order = arms[k % 3:] + arms[:k % 3]
        for a in order:
            for s, x in zip(streams[a], audio):
                s.AddSamples(x[off: off + 9600])
            t0 = time.perf_counter()
            recs[a].GetResults(streams[a])
            if k >= WARM:
                t[a].append((time.perf_counter() - t0) * 1e3)
    same = all(x.Tokens == y.Tokens for x, y in zip(streams["off"], streams["on"]))
    med = {a: float(np.median(t[a])) for a in arms}
    q = {a: (float(np.percentile(t[a], 25)), float(np.percentile(t[a], 75))) for a in arms}
    lines.append("streams %2d, %d timed GetResults per arm, tokens per stream %d, ids of on == off: %s" % (n, len(t["off"]), len(streams["off"][0].Tokens), same))
    for a in arms:
        lines.append("  %-4s median %.3f ms   quartiles %.3f .. %.3f ms" % (a, med[a], q[a][0], q[a][1]))
    lines.append("  spread of the off arm (|off - off2| medians): %.3f ms;  on - off: %+.3f ms" % (abs(med["off"] - med["off2"]), med["on"] - med["off"]))
    del streams
for r in recs.values():
    r.Dispose()
print("\n".join(lines), flush=True)
if "--out" in sys.argv[1:]:
    open(sys.argv[sys.argv.index("--out") + 1], "w").write("\n".join(lines) + "\n")
