"""What OnlineStream.AddPcm costs per chunk against converting on the host: paraformer-large geometry (synthetic weights), 1 and 32
concurrent streams fed 0.6 s of audio per call, every recognizer with SetTokenInfo and SetDeviceFrontend.  Three arms from the same
files run the same schedule: "host" (the host twin, pf_host_pcm_stream_push, then AddSamples of what it returned), "pcm" (AddPcm of
the raw bytes: converted by csrc/k_pcm_stream.hip in front of the fbank) and "host2" (the first again: its difference to "host" is
the spread of this measurement).  Every chunk is ONE alternated triple, the order rotating every chunk.  Inputs: 8 kHz mu-law mono
and 48 kHz stereo s16, under the linear and the band-limited rule.  Clocked: the feeding calls plus GetResults (it ends in a
device synchronise), medians and quartiles.  A second, untimed pass with the engine's profile on gives the event time of the
pcm_stream launch next to its byte floor (bytes the launch must move / --hbm-gbs, 8000 by default: the MI355X's peak).
Writes profiles/online_pcm_cost.json (or --out FILE) and prints it."""
import ctypes as C, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from aliparaformerasr_amd import _native as N, weights as W
from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
from oracle import frontend as fe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv[1:] else default
OUT, HBM = arg("--out", os.path.join(ROOT, "profiles", "online_pcm_cost.json")), float(arg("--hbm-gbs", "8000"))
SEC, WARM, PROF = int(arg("--seconds", "18")), 4, 8

d = tempfile.mkdtemp()
cfg = W.paraformer_large_config()
w = W.synth_weights(cfg, 42)
w["predictor.out.bias"] = np.asarray([0.8], np.float32)
W.save_pfw(os.path.join(d, "model.pfw"), cfg, w)
sh, sc = W.synth_cmvn()
open(os.path.join(d, "am.mvn"), "w").write(fe.format_mvn_text(sh, sc))
open(os.path.join(d, "asr.yaml"), "w").write("model: paraformer\nfrontend_conf:\n  dither: 0\n")
open(os.path.join(d, "tokens.txt"), "w").write("\n".join("t%d" % i for i in range(cfg["vocab"])) + "\n")
arms = ["host", "pcm", "host2"]
recs = {}
for a in arms:
    recs[a] = OnlineRecognizer(os.path.join(d, "model.pfw"), "", os.path.join(d, "asr.yaml"), os.path.join(d, "am.mvn"), os.path.join(d, "tokens.txt"))
    recs[a].SetTokenInfo(True)
    recs[a].SetDeviceFrontend(True)


def audio(kind, u):
    """SEC seconds of the synthetic utterance u as raw bytes of the kind"""
    x = W.synth_audio(16000 * SEC, u)
    if kind == "8k_mulaw_mono":
        y = np.clip(x[::2], -1, 1)
        m = np.sign(y) * np.log1p(255 * np.abs(y)) / np.log(256.0)
        return (~(((m < 0) * 128) | np.minimum(127, (np.abs(m) * 128).astype(np.int64)))).astype(np.uint8).tobytes()   # (a coarse G.711: timing only)
    y = np.repeat(x, 3)
    return (np.stack([y, y], 1) * 32767).astype("<i2").tobytes()


KINDS = {"8k_mulaw_mono": (8000, 1, "mulaw", 1), "48k_s16_stereo": (48000, 2, "s16", 4)}      # rate, channels, format, bytes per frame


def feed(a, streams, twins, pieces, kind, rule):
    sr, ch, fmt, _b = KINDS[kind]
    for s, t, p in zip(streams, twins, pieces):
        if a == "pcm":
            s.AddPcm(p, sr, ch, fmt, resample=rule)
        else:
            s.AddSamples(t.push(p))


def launch_ms(rec):
    ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
    N.check(N.load().pf_profile_get(C.c_void_p(rec.engine_handle()), b"pcm_stream", C.byref(ms), C.byref(n), C.byref(fpl)))
    return ms.value, n.value


result = {"seconds": SEC, "hbm_gbs": HBM, "cases": []}
for kind in KINDS:
    sr, ch, fmt, fb = KINDS[kind]
    step = int(0.6 * sr) * fb
    for rule in ("linear", "sinc"):
        for n in (1, 32):
            raws = [audio(kind, u) for u in range(n)]
            streams = {a: [recs[a].CreateOnlineStream() for _ in range(n)] for a in arms}
            twins = {a: [N.HostPcmStream(N.pcm_desc(sr, ch, fmt, sinc=rule == "sinc")) for _ in range(n)] for a in arms}
            t = {a: [] for a in arms}
            offs = list(range(0, len(raws[0]) - PROF * step, step))
            for k, off in enumerate(offs):
                pieces = [r[off: off + step] for r in raws]
                for a in arms[k % 3:] + arms[:k % 3]:
                    t0 = time.perf_counter()
                    feed(a, streams[a], twins[a], pieces, kind, rule)
                    recs[a].GetResults(streams[a])
                    if k >= WARM:
                        t[a].append((time.perf_counter() - t0) * 1e3)
            same = all(x.Tokens == y.Tokens for x, y in zip(streams["host"], streams["pcm"]))
            h = C.c_void_p(recs["pcm"].engine_handle())            # the launch alone, by its events: a pass that is not clocked
            N.check(N.load().pf_profile_enable(h, 1)); N.check(N.load().pf_profile_reset(h))
            for off in range(offs[-1] + step, offs[-1] + step + PROF * step, step):
                feed("pcm", streams["pcm"], twins["pcm"], [r[off: off + step] for r in raws], kind, rule)
                recs["pcm"].GetResults(streams["pcm"])
            ms, launches = launch_ms(recs["pcm"])
            N.check(N.load().pf_profile_enable(h, 0))
            moved = n * (step + 9600 * 4 + 2 * 4096)               # raw bytes in, the row out, one tail read and one written at the most
            q = lambda v: [float(np.percentile(v, p)) for p in (25, 50, 75)]
            case = {"input": kind, "rule": rule, "streams": n, "timed_chunks": len(t["host"]), "tokens_equal": bool(same),
                    "ms_quartiles": {a: q(t[a]) for a in arms},
                    "spread_ms": abs(q(t["host"])[1] - q(t["host2"])[1]), "pcm_minus_host_ms": q(t["pcm"])[1] - q(t["host"])[1],
                    "pcm_stream_launches": launches, "pcm_stream_event_ms": ms / max(launches, 1),
                    "pcm_stream_bytes": moved, "pcm_stream_floor_ms": moved / (HBM * 1e9) * 1e3}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del streams, twins
for r in recs.values():
    r.Dispose()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
json.dump(result, open(OUT, "w"), indent=1)
