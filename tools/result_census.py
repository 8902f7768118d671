#!/usr/bin/env python3
"""Digests of everything a GetResults leaves behind, one JSON object per case on stdout.

    python tools/result_census.py [PACKAGE_DIR] [--only NAME ...]

PACKAGE_DIR: the tree to import `aliparaformerasr_amd` from (default: this one) — a built copy of another commit gives that
commit's digests for the same cases, so two builds are compared case by case (bit identity of a refactor of
Recognizer::Forward / ForwardLong, csrc/recognizer.cpp and csrc/stream_result.cpp).  Per case: one SHA-1 over every field of
every stream (Tokens, Timestamps, Scores, TokenAlternatives, Alternatives, Alignment, Segments, speaker and punctuation
fields, SpeechLength — what RemoveChunk and quirk Q8 leave) and of every result entity (Text, TextLen, Tokens, Timestamps) of
one GetResults over two unequal utterances, and beside it how many tokens, timestamps, token alternatives, alternatives and
segments each stream got; a call that raises is recorded with the exception's type and message.  The
models are the tiny synthetic ones of the GPU tests (paraformer, with the timestamp head, SeACo, SenseVoice), built from fixed
seeds in a temporary directory; nothing outside the repository is read."""
import argparse
import dataclasses
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(x):
    import numpy as np
    h = hashlib.sha1()

    def walk(v):
        if dataclasses.is_dataclass(v):
            walk(dataclasses.asdict(v))
        elif isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode())
                walk(v[k])
        elif isinstance(v, (tuple, list)):
            h.update(b"(%d" % len(v))
            for e in v:
                walk(e)
        elif isinstance(v, np.ndarray):
            h.update(str((v.dtype.str, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    walk(x)
    return h.hexdigest()


STREAM_FIELDS = ("Tokens", "Timestamps", "Scores", "TokenAlternatives", "Alternatives", "Alignment", "Segments", "SegmentSpeakers",
                 "SpeakerCentroids", "SpeakerWindows", "Punctuated", "PuncIds", "Sentences", "SpeechLength", "Hotwords")


def snapshot(streams, results):
    return {"streams": [{f: getattr(s, f) for f in STREAM_FIELDS} for s in streams],
            "results": [(r.Text, r.TextLen, r.Tokens, r.Timestamps) for r in results]}


def sizes(snap):
    """how much a case exercised, beside its digest: per stream the number of tokens / timestamps / alternatives / segments"""
    if isinstance(snap, list):
        return [sizes(x) for x in snap]
    if not isinstance(snap, dict) or "error" in snap:
        return snap["error"][1][:60] if isinstance(snap, dict) else snap
    return [[len(s["Tokens"]), len(s["Timestamps"]), len(s["TokenAlternatives"]), len(s["Alternatives"]), len(s["Segments"])] for s in snap["streams"]]


def write_arpa(path, toks, ids):
    """a bigram model over the token ids `ids` (log10 values that are exact in float32)"""
    uni = ["-2.5\t<s>\t-0.5", "-1.5\t</s>"] + ["%s\t%s\t-0.25" % (-1.0 - 0.125 * (i % 7), toks[c]) for i, c in enumerate(ids)]
    bi = ["%s\t%s %s" % (-0.5 - 0.125 * (i % 3), toks[a], toks[b]) for i, (a, b) in enumerate(zip(ids, ids[1:]))]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\nngram 1=%d\nngram 2=%d\n\n\\1-grams:\n%s\n\n\\2-grams:\n%s\n\n\\end\\\n" % (len(uni), len(bi), "\n".join(uni), "\n".join(bi)))
    return path


def build_models(tmp, np, W):
    """kind -> the four constructor paths (+ extras beside them)"""
    out = {}
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=300)
    out["paraformer"] = W.synth_model_dir(os.path.join(tmp, "paraformer"), cfg, W.synth_weights(cfg, seed=77))
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=96, timestamp_head=True)
    w = W.synth_weights(cfg, 5)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    out["timestamp"] = W.synth_model_dir(os.path.join(tmp, "timestamp"), cfg, w)
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    w = W.synth_weights(cfg, 21)
    w["predictor.out.bias"] = np.asarray([0.0], np.float32)
    w["seaco.output.bias"][111] += 2.6
    out["seaco"] = W.synth_model_dir(os.path.join(tmp, "seaco"), cfg, w)
    for name, blank in (("sensevoice", 1.0), ("sensevoice_blank", 60.0)):          # the second one answers blank at every frame
        cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=403)
        cfg["use_itn"] = True
        w = W.synth_weights(cfg, seed=9)
        b = np.array(w["ctc.bias"], np.float32)
        b[8:] -= 30
        b[0] += blank
        w["ctc.bias"] = b
        out[name] = W.synth_model_dir(os.path.join(tmp, name), cfg, w)
    for kind, p in out.items():
        toks = open(p["tokens"], encoding="utf-8").read().split("\n")
        p["toks"] = toks
        hot = [5, 6] if kind.startswith("sensevoice") else [10, 20]
        p["hotword"] = os.path.join(os.path.dirname(p["model"]), "hotword.txt")
        with open(p["hotword"], "w", encoding="utf-8") as f:
            f.write("".join(toks[c] for c in hot) + "\n")
        p["arpa"] = write_arpa(os.path.join(os.path.dirname(p["model"]), "lm.arpa"), toks, list(range(4, 16)))
    pcfg = W.ct_transformer_config(vocab=64, n_layers=1)
    W.save_pfw(os.path.join(tmp, "punc.pfw"), pcfg, W.synth_punc_weights(pcfg, seed=5))
    scfg = W.campplus_config(m_channels=8, init_channels=24, growth=8, bn_channels=12, blocks=(2, 3, 2), seg_len=5, embedding=20)
    W.save_pfw(os.path.join(tmp, "cam.pfw"), scfg, W.synth_spk_weights(scfg, seed=3))
    return out


def cases(np, W, models, tmp):
    """name -> (model kind, constructor keywords, fn(rec, new_streams) -> snapshot or list of snapshots)"""
    out = {}
    audio = [W.synth_audio(40000, 41), W.synth_audio(27000, 42)]
    sv_audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]       # (what the SenseVoice tests collapse to two tokens and more)

    def bursts(u, plan):                                   # (silence s, speech s) ... : what SetVad cuts
        parts = []
        for k, (gap, talk) in enumerate(plan):
            parts += [np.zeros(int(16000 * gap), np.float32), W.synth_audio(int(16000 * talk), 50 + 10 * u + k)]
        return np.concatenate(parts + [np.zeros(8000, np.float32)])
    long_audio = [bursts(0, [(0.5, 1.5), (1.0, 2.5), (0.8, 1.0)]), bursts(1, [(0.3, 2.0), (1.2, 1.2)])]

    def case(name, kind, **ctor):
        def reg(fn):
            out[name] = (kind, ctor, fn)
            return fn
        return reg

    def streams_of(rec, sounds=audio, hotwords=(), targets=(), twice=False, pcm=False):
        ss = []
        for i, a in enumerate(sounds):
            s = rec.CreateOfflineStream()
            if pcm:
                s.AddPcm(np.round(a * 32767).astype(np.int16), 16000)
            elif twice:                                    # a second AddSamples: the host form
                s.AddSamples(a[: len(a) // 2])
                s.AddSamples(a[len(a) // 2:])
            else:
                s.AddSamples(a)
            if i < len(hotwords):
                s.Hotwords = hotwords[i]
            if i < len(targets) and targets[i] is not None:
                s.SetAlignIds(targets[i])
            ss.append(s)
        return ss

    def get(rec, **kw):
        ss = streams_of(rec, **kw)
        return snapshot(ss, rec.GetResults(ss))

    def simple(name, kind, setup=lambda rec: None, ctor=None, **kw):
        if kind == "sensevoice":
            kw.setdefault("sounds", sv_audio)

        @case(name, kind, **(ctor or {}))
        def run(rec, setup=setup, kw=kw):
            setup(rec)
            return get(rec, **kw)

    file_hw = lambda kind: dict(hotwordFilePath=models[kind]["hotword"])
    # paraformer: the reference behaviour, Scores, top-k, the n-best list from the host and from the device search
    simple("paraformer", "paraformer")
    simple("paraformer-host-form", "paraformer", twice=True)
    simple("paraformer-pcm", "paraformer", pcm=True)
    simple("paraformer-scores", "paraformer", lambda r: r.SetDecode(scores=True))
    simple("paraformer-nbest1", "paraformer", lambda r: r.SetNBest(1, 4))
    simple("paraformer-nbest5", "paraformer", lambda r: r.SetNBest(5, 4))
    simple("paraformer-nbest5-scores", "paraformer", lambda r: (r.SetDecode(scores=True), r.SetNBest(5, 3)))
    simple("paraformer-nbest5-host-form", "paraformer", lambda r: r.SetNBest(5, 4), twice=True)
    simple("paraformer-search", "paraformer", lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8)))
    simple("paraformer-search-lm", "paraformer", lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8), r.SetNBestLm(models["paraformer"]["arpa"], 0.6, 0.2, 0)))
    simple("paraformer-search-hot-streams", "paraformer", lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8), r.SetNBestHotwordBoost(1.5)),
           hotwords=[[[10, 20], [1]], [[30]]])
    simple("paraformer-search-hot-file-lm", "paraformer",
           lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8), r.SetNBestHotwordBoost(1.5), r.SetNBestLm(models["paraformer"]["arpa"], 0.6, 0.2, 0)),
           ctor=file_hw("paraformer"))
    simple("paraformer-search-hot-null", "paraformer", lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8), r.SetNBestHotwordBoost(1.5)),
           ctor=file_hw("paraformer"), hotwords=[None, [[30]]])
    simple("paraformer-search-off-again", "paraformer", lambda r: (r.SetNBest(5, 4), r.SetNBestSearch(8), r.SetNBestSearch(0)))
    simple("paraformer-punc", "paraformer", lambda r: r.SetPuncModel(os.path.join(tmp, "punc.pfw")))

    @case("paraformer-no-samples", "paraformer")
    def no_samples(rec):
        ss = streams_of(rec) + [rec.CreateOfflineStream()]
        try:
            rec.GetResults(ss)
        except Exception as ex:                              # noqa: BLE001 — the record is the point
            return {"error": (type(ex).__name__, str(ex)), "streams": snapshot(ss, [])}
        return "no error"
    simple("timestamp", "timestamp")
    simple("timestamp-scores-nbest3", "timestamp", lambda r: (r.SetDecode(scores=True), r.SetNBest(3, 4)))
    simple("timestamp-punc", "timestamp", lambda r: r.SetPuncModel(os.path.join(tmp, "punc.pfw")))
    # SeACo: where the hot words come from
    simple("seaco-file", "seaco", ctor=file_hw("seaco"))
    simple("seaco-no-file", "seaco")
    simple("seaco-streams", "seaco", ctor=file_hw("seaco"), hotwords=[[[30, 31], [1]], [[5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]]])
    simple("seaco-host-form", "seaco", ctor=file_hw("seaco"), twice=True)

    @case("seaco-null", "seaco", **file_hw("seaco"))
    def seaco_null(rec):
        ss = streams_of(rec, hotwords=[[[30]], None])
        try:
            rec.GetResults(ss)
        except Exception as ex:                              # noqa: BLE001
            return {"error": (type(ex).__name__, str(ex)), "streams": snapshot(ss, [])}
        return "no error"
    # SenseVoice: the collapse, top-k at the peak frame, the beam search with hot words and a model, forced alignment
    sv = "sensevoice"
    simple("sv", sv)
    simple("sv-host-form", sv, twice=True)
    simple("sv-scores", sv, lambda r: r.SetDecode(scores=True))
    simple("sv-ctc", sv, lambda r: r.SetDecode(ctc=True))
    simple("sv-ctc-host-form", sv, lambda r: r.SetDecode(ctc=True), twice=True)
    simple("sv-topk", sv, lambda r: r.SetNBest(1, 4))
    simple("sv-ctc-topk", sv, lambda r: (r.SetDecode(ctc=True), r.SetNBest(1, 3)))
    simple("sv-ctc-scores-topk", sv, lambda r: (r.SetDecode(ctc=True, scores=True), r.SetNBest(1, 4)))
    simple("sv-beam", sv, lambda r: r.SetCtcBeam(4, 8, 4))
    simple("sv-ctc-beam", sv, lambda r: (r.SetDecode(ctc=True), r.SetCtcBeam(4, 8, 4)))
    simple("sv-beam-topk-scores", sv, lambda r: (r.SetDecode(scores=True), r.SetNBest(1, 4), r.SetCtcBeam(3, 0, 4)))
    simple("sv-beam-hot-streams", sv, lambda r: (r.SetCtcBeam(4, 8, 4), r.SetHotwordBoost(2.0)), hotwords=[[[5, 6], [1]], [[7]]])
    simple("sv-beam-hot-file", sv, lambda r: (r.SetCtcBeam(4, 8, 4), r.SetHotwordBoost(2.0)), ctor=file_hw(sv))
    simple("sv-beam-hot-without-beam", sv, lambda r: r.SetHotwordBoost(2.0), ctor=file_hw(sv))
    simple("sv-beam-lm", sv, lambda r: (r.SetCtcBeam(4, 8, 4), r.SetLm(models[sv]["arpa"], 0.5, 0.25, 1)))
    simple("sv-beam-hot-lm", sv, lambda r: (r.SetCtcBeam(4, 8, 4), r.SetHotwordBoost(2.0), r.SetLm(models[sv]["arpa"], 0.5, 0.25, 0)), ctor=file_hw(sv))
    simple("sv-align-mixed", sv, lambda r: r.SetAlign(True), targets=[[5, 6, 5], None])
    simple("sv-align-none", sv, lambda r: r.SetAlign(True))
    simple("sv-align-impossible", sv, lambda r: r.SetAlign(True), targets=[None, [5] * 400])
    simple("sv-align-beam", sv, lambda r: (r.SetAlign(True), r.SetCtcBeam(4, 8, 4)), targets=[None, [5, 6]])
    simple("sv-align-beam-no-target", sv, lambda r: (r.SetAlign(True), r.SetCtcBeam(4, 8, 4)))
    simple("sv-align-beam-hot-lm-ctc", sv, lambda r: (r.SetDecode(ctc=True, scores=True), r.SetAlign(True), r.SetCtcBeam(4, 8, 4), r.SetHotwordBoost(2.0),
                                                      r.SetLm(models[sv]["arpa"], 0.5, 0.25, 0)), ctor=file_hw(sv), targets=[[6, 5], [5]])

    @case("sv-beam-hot-null", sv, **file_hw(sv))
    def sv_null(rec):
        rec.SetCtcBeam(4, 8, 4)
        rec.SetHotwordBoost(2.0)
        ss = streams_of(rec, sounds=sv_audio, hotwords=[None])
        try:
            rec.GetResults(ss)
        except Exception as ex:                              # noqa: BLE001
            return {"error": (type(ex).__name__, str(ex)), "streams": snapshot(ss, [])}
        return "no error"

    for form in ("device", "host"):
        @case("sv-q8-kept-chunk-%s-form" % form, "sensevoice_blank")
        def q8(rec, form=form):
            # every frame is blank: the collapse leaves no token, RemoveChunk keeps the chunk, and the stream carries the prompt rows
            # into its second GetResults (quirk Q8)
            rec.SetDecode(ctc=True)
            ss = streams_of(rec, twice=form == "host")
            first = snapshot(ss, rec.GetResults(ss))
            return [first, snapshot(ss, rec.GetResults(ss))]
    # long audio: segmentation, stitching, speaker labels, punctuation of the stitched text
    vad = dict(max_len=300, split_search=100, min_speech=50)
    simple("vad", "paraformer", lambda r: r.SetVad(vad, sep=" | "), sounds=long_audio)
    simple("vad-scores-small-batches", "paraformer", lambda r: (r.SetDecode(scores=True), r.SetVad(vad, batch_max=2)), sounds=long_audio)
    simple("vad-timestamp", "timestamp", lambda r: r.SetVad(vad), sounds=long_audio)
    simple("vad-seaco", "seaco", lambda r: r.SetVad(vad), ctor=file_hw("seaco"), sounds=long_audio, hotwords=[[[30, 31]], []])
    simple("vad-sv-ctc", sv, lambda r: (r.SetDecode(ctc=True), r.SetVad(vad)), sounds=long_audio)
    simple("vad-spk", "paraformer", lambda r: (r.SetSpeakerModel(os.path.join(tmp, "cam.pfw"), dict(win=100, shift=50)), r.SetVad(vad)), sounds=long_audio)
    simple("vad-spk-punc", "paraformer", lambda r: (r.SetVad(vad), r.SetSpeakerModel(os.path.join(tmp, "cam.pfw")),
                                                     r.SetPuncModel(os.path.join(tmp, "punc.pfw"))), sounds=long_audio)
    simple("vad-silence", "paraformer", lambda r: r.SetVad(vad), sounds=[np.zeros(16000, np.float32), long_audio[1]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("package_dir", nargs="?", default=HERE)
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_dir))
    import numpy as np
    import aliparaformerasr_amd
    from aliparaformerasr_amd import weights as W
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    print(json.dumps({"package": os.path.dirname(os.path.abspath(aliparaformerasr_amd.__file__))}), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        models = build_models(tmp, np, W)
        for name, (kind, ctor, fn) in cases(np, W, models, tmp).items():
            if args.only and name not in args.only:
                continue
            p = models[kind]
            rec = OfflineRecognizer(p["model"], p["config"], p["mvn"], p["tokens"], **ctor)
            try:
                snap = fn(rec)
                rec_out = {"sha1": digest(snap), "sizes": sizes(snap)}
            except Exception as ex:                          # noqa: BLE001 — a case the recogniser refuses is a record too
                rec_out = {"raised": "%s: %s" % (type(ex).__name__, ex)}
            rec.Dispose()
            print(json.dumps({"case": name, **rec_out}, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
