"""What streaming endpointing costs, in one process, for 1 and for 32 streams fed one 0.6 s chunk each per call:

  get_results_off / _on   wall clock of OnlineRecognizer.GetResults without and with SetEndpoint (paraformer-large geometry with
                          synthetic weights, the model of tools/bench_online.py): median with p10 / p90 over --steps calls after
                          --warmup.  Off is the parent's path: it adds no launch.
  endpoint_ms             device time of the profile class `endpoint` (the level launch and the endpoint launch) per call, from a
                          run of its own with the profiler on
  second_pass             wall clock of the ONE call in which 32 sentences close and go through the second pass (3 + 3 layer
                          online and 2 + 2 layer offline synthetic models: the forwards are NOT the cost of a real model), against
                          the same call without a second pass

  --model                 instead of the above: the same GetResults for 1 and 32 streams with the ENERGY endpoint and with the
                          FSMN-VAD model score attached (SetEndpointModel; released dimensions, synthetic weights: the cost does
                          not depend on the values), two recognizers in one process, plus the device time of the classes
                          `endpoint` and `vadnet_stream` per call (profiles/endpoint_model_cost.json)

Audio: 0.001 N(0, 1) with 0.3 N(0, 1) bursts (tests/vad_ref.py burst_audio).

    python tools/endpoint_cost.py [--steps 10] [--warmup 3] [--model] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vad_ref as V                                               # noqa: E402
from aliparaformerasr_amd import _native as N                     # noqa: E402
from aliparaformerasr_amd import weights as W                     # noqa: E402
from aliparaformerasr_amd.engine import Engine                    # noqa: E402
from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer   # noqa: E402
from aliparaformerasr_amd.online_recognizer import OnlineRecognizer     # noqa: E402
from oracle import frontend as fe                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--model", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
CHUNK = 9600


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), p10=v[int(0.1 * (len(v) - 1))], p90=v[int(round(0.9 * (len(v) - 1)))], n=len(v))


def model_dir(cfg, w, head):
    d = tempfile.mkdtemp()
    W.save_pfw(os.path.join(d, "model.pfw"), cfg, w)
    open(os.path.join(d, "am.mvn"), "w").write(fe.format_mvn_text(*W.synth_cmvn()))
    open(os.path.join(d, "asr.yaml"), "w").write(head + "frontend_conf:\n  dither: 0\n")
    open(os.path.join(d, "tokens.txt"), "w", encoding="utf-8").write("\n".join("t%d" % i for i in range(cfg["vocab"])) + "\n")
    return [os.path.join(d, f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")]


def online(cfg, seed):
    w = W.synth_weights(cfg, seed)
    w["predictor.out.bias"] = np.asarray([0.8], np.float32)
    p = model_dir(cfg, w, "model: paraformer\n")
    return OnlineRecognizer(p[0], "", p[1], p[2], p[3])


def engine_view(rec):
    """the recognizer's engine as an Engine object for the profiler calls (borrowed: never closed here)"""
    e = Engine.__new__(Engine)
    e._lib, e._h = N.load(), C.c_void_p(rec.engine_handle())
    return e


def timed_calls(rec, n, profile=None, classes=(("endpoint", 2),)):
    """n fresh streams, warmup + steps calls of one chunk each: the wall clock of GetResults alone, and the device time of the
    profile classes (name, launches expected per call), summed"""
    calls = args.warmup + args.steps
    audio = [V.burst_audio((calls + 2) * CHUNK // 16000 + 1, [(60, 200), (330, 480), (620, 700)], u) for u in range(n)]
    streams = [rec.CreateOnlineStream() for _ in range(n)]
    for s, a in zip(streams, audio):
        s.AddSamples(a[:CHUNK])                                   # the constructor's chunk of silence goes first
    rec.GetResults(streams)
    wall, cls = [], []
    for k in range(1, calls + 1):
        for s, a in zip(streams, audio):
            s.AddSamples(a[k * CHUNK: (k + 1) * CHUNK])
        if profile:
            profile.profile_reset()
        t = time.perf_counter()
        rec.GetResults(streams)
        dt = (time.perf_counter() - t) * 1e3
        if k > args.warmup:
            wall.append(dt)
            if profile:
                total = 0.0
                for name, expect in classes:
                    ms, launches, _ = profile.profile_get(name)
                    assert launches == expect, (name, launches)
                    total += ms
                cls.append(total)
    return wall, cls, sum(len(s.Sentences) for s in streams)


def model_cost():
    """the energy endpoint and the model endpoint side by side: one recognizer each (a model is attached before any stream feeds)"""
    vcfg = W.fsmn_vad_config()
    vpath = os.path.join(tempfile.mkdtemp(), "vad.pfw")
    W.save_pfw(vpath, vcfg, W.synth_vad_weights(vcfg, 6))
    from aliparaformerasr_amd.engine import endpoint_model_config
    re_, rm = online(W.paraformer_large_config(), 42), online(W.paraformer_large_config(), 42)
    re_.SetEndpoint()
    rm.SetEndpointModel(vpath)
    rm.SetEndpoint(endpoint_model_config())
    ve, vm = engine_view(re_), engine_view(rm)
    res = {}
    for n in (1, 32):
        e1, _, _ = timed_calls(re_, n)
        m1, _, _ = timed_calls(rm, n)
        e2, _, _ = timed_calls(re_, n)                            # the energy form again, behind the model runs: the spread of the box
        m2, _, _ = timed_calls(rm, n)
        ve.profile(True)
        _, ce, _ = timed_calls(re_, n, profile=ve)
        ve.profile(False)
        vm.profile(True)
        _, cm, _ = timed_calls(rm, n, profile=vm, classes=(("vadnet_stream", 1),))
        _, cb, _ = timed_calls(rm, n, profile=vm, classes=(("vadnet_stream", 1), ("endpoint", 1)))
        vm.profile(False)
        res["streams_%d" % n] = dict(get_results_energy_ms=stats(e1 + e2), get_results_model_ms=stats(m1 + m2),
                                     get_results_energy_runs_ms=[stats(e1), stats(e2)], get_results_model_runs_ms=[stats(m1), stats(m2)],
                                     endpoint_class_energy_ms=stats(ce), vadnet_stream_class_ms=stats(cm),
                                     vadnet_stream_plus_endpoint_class_ms=stats(cb))
    ve._h = vm._h = None
    re_.Dispose(); rm.Dispose()
    return res


if args.model:
    line = json.dumps(model_cost())
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    sys.exit(0)

out = {}
rec = online(W.paraformer_large_config(), 42)
view = engine_view(rec)
for n in (1, 32):
    rec.SetEndpoint(False)
    off, _, _ = timed_calls(rec, n)
    rec.SetEndpoint()
    on, _, n_sent = timed_calls(rec, n)
    view.profile(True)
    _, cls, _ = timed_calls(rec, n, profile=view)
    view.profile(False)
    rec.SetEndpoint(False)
    off2, _, _ = timed_calls(rec, n)                               # off again, behind the on runs: the spread of the box
    out["streams_%d" % n] = dict(get_results_off_ms=stats(off), get_results_on_ms=stats(on), get_results_off_again_ms=stats(off2),
                                 endpoint_ms=stats(cls), sentences=n_sent)
view._h = None
rec.Dispose()

# ---- 32 sentences close in one call and go through the second pass (small synthetic models)
rec = online(W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=300), 31)
ocfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=300)
second = OfflineRecognizer(*model_dir(ocfg, W.synth_weights(ocfg, seed=77), "model: paraformer\n"))
rec.SetEndpoint(end_silence=40)
audio = [V.burst_audio(4, [(30, 150)], u) for u in range(32)]      # the state run ends near frame 164: the close falls into chunk 4
res = {}
for name, sp in (("without", None), ("with", second)):
    rec.SetSecondPass(sp)
    ms = []
    for it in range(args.warmup + args.steps):
        streams = [rec.CreateOnlineStream() for _ in audio]
        hit = None
        for k in range(6):
            for s, a in zip(streams, audio):
                s.AddSamples(a[k * CHUNK: (k + 1) * CHUNK])
            t = time.perf_counter()
            rec.GetResults(streams)
            dt = (time.perf_counter() - t) * 1e3
            if hit is None and sum(len(s.Sentences) for s in streams) == 32:
                hit = dt
        assert hit is not None
        if it >= args.warmup:
            ms.append(hit)
    res[name] = stats(ms)
out["second_pass_32_sentences"] = dict(closing_call_without_ms=res["without"], closing_call_with_ms=res["with"])
rec.Dispose(); second.Dispose()
line = json.dumps(out)
print(line)
if args.out:
    open(args.out, "w").write(line + "\n")
