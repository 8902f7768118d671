"""Command-line harness mirroring AliParaformerAsr.Examples (`-type offline` and `-type online`).

    python -m aliparaformerasr_amd.examples -type offline -method batch -base <dir> -model <name> \
        [-accuracy int8] [-threads 2] [-decode ctc|frames] [-intake host|device] [-nbest N [-topk K] [-beam W | -search W] [-hotboost S] [-lm FILE [-lmweight A] [-lmbonus B] [-lmeos]]] [-align FILE|beam] [-vad [key=value,...] [-vadmodel FILE] [-spk FILE [key=value,...]]] [-punc FILE] -files a.wav b.wav
    python -m aliparaformerasr_amd.examples -type online -method one -base <dir> -model <name> [-endpoint [key=value,...] [-vadmodel FILE] [-secondpass <offline name>]] [-tokentimes] [-puncstream FILE[,max_context=N]] -files a.wav

Mirrors (file:line in /root/reference/AliParaformerAsr.Examples):
  * argument handling and defaults — Program.cs:93-104, ParseArgs :197-252: the MANYSPEECH_BASE / _TYPE / _BATCH / _MODEL /
    _ACCURACY / _THREADS environment variables are the defaults (Program.cs:20-28), command-line parameters overwrite
    them; a recognizer type must come from one of the two, unknown flags are an error;
  * model-directory file selection — OfflineAliParaformerAsrRecognizer.cs:24-100: `model*` (not `_eb`)
    preferring a name containing ".<accuracy>.", else the last; last `asr*.yaml|json`, `am*.mvn`, `tokens*.txt`,
    `hotword*.txt` (the model file here is a .pfw container instead of .onnx);
  * sample loading — IsAudioByHeader + GetFileSample (:121-160, Utils/AudioHelper.cs:12-32) through the native
    pf_host_wav_read / pf_host_is_audio; default file list = every *.wav under the model directory;
  * "-method one" / "-method batch" loops, the JSON-ish result line and the timing lines — :169-249 (the timed
    window includes stream creation, AddSamples, GetResults, printing and Dispose, as upstream);
  * `-type online` (Program.cs:290-297) — OnlineAliParaformerAsrRecognizer.cs:8-279: encoder / decoder file selection
    (:43-63), at most TWO media files (:121-171), 9600-sample chunks (AudioHelper.GetFileChunkSamples :80-127) plus six
    400-sample silence chunks (:160-163), one AddSamples + GetResult + printed text per chunk (:181-194; only the "one"
    method exists upstream — the batch loop is commented out there), timing lines :272-279.
Not in the reference: `-decode ctc` (offline, SenseVoice models) prints the CTC-collapsed hypothesis with per-token
timestamps (OfflineRecognizer.SetDecode); `-decode frames`, the default, is the reference's one id per frame.
`-intake device` (offline) reads only the wav header on the host (pf_host_wav_info) and hands the payload to
OfflineStream.AddPcm raw: decode, down-mix and resample run on the device and give the samples GetFileSample gives;
`-intake host`, the default, is the path above, untouched.
`-nbest N [-topk K]` (offline, paraformer models; OfflineRecognizer.SetNBest) prints under each result line the N best
hypotheses, one `nbest[i] score:<sum of log-probs> text:<text>` line each, best first; line 0 is the result itself.
`-nbest N -beam W` (offline, SenseVoice models; OfflineRecognizer.SetCtcBeam) prints the N best labelings of a CTC prefix
beam search of width W in the same form; the score is the log of the summed alignments.
`-hotboost S` (with `-nbest N -beam W`; OfflineRecognizer.SetHotwordBoost) biases that search towards the model directory's
`hotword*.txt` by S per matched token; each `nbest[i]` line then ends in ` hot:<matched tokens> loglik_sum:<unbiased score>`.
`-search W` (with `-nbest N`, offline, paraformer models; OfflineRecognizer.SetNBestSearch) takes the N best from a beam search
of width W over the per-token alternatives on the device instead of the exact enumeration; `-hotboost`, `-lm`, `-lmweight`,
`-lmbonus` and `-lmeos` then go to that search (SetNBestHotwordBoost, SetNBestLm) and decide which prefixes survive a position;
each `nbest[i]` line ends in ` hot:<matched tokens> lm:<lm_sum> loglik_sum:<sum of log-probs>`.
`-lm FILE [-lmweight A] [-lmbonus B] [-lmeos]` (with `-nbest N -beam W`; OfflineRecognizer.SetLm) fuses the ARPA n-gram language
model FILE into that search with weight A (default 0.5), per-token bonus B (default 0) and, with `-lmeos`, the end-of-sentence
step; each `nbest[i]` line then ends in ` hot:<matched tokens> lm:<lm_sum> loglik_sum:<unfused score>`.
`-align FILE` (offline, SenseVoice models; OfflineRecognizer.SetAlign) aligns a known text to each input file: FILE holds one
line of space-separated token ids per file of `-files`, in their order (an empty line: no target; ids, not text — the
tokenizer is not part of this package), and under each result line goes
`align ok:<0|1> path:<best alignment's log-prob> loglik:<log P(ids | audio)> pairs:[begin,end],...` in milliseconds.
`-vad [key=value,...]` (offline; OfflineRecognizer.SetVad) is for long recordings: each file is cut into speech segments on
the device, the segments are recognised in batches of similar length and stitched into one result per file; under each result
line goes one `[begin-end ms] text` line per segment.  Keys: the pf_vad_config fields (floor_pct, margin_q, abs_level, window,
on_count, off_count, pad_begin, pad_end, min_speech, max_len, split_search), batch_max, frame_budget and sep.  The default
thresholds are unvalidated on real speech.  Not beside -nbest / -align.
`-vadmodel FILE` (with `-vad`; OfflineRecognizer.SetVadModel) scores the frames with an FSMN-VAD network instead of the
log-mel energy: FILE is a `.pfw` of kind fsmnvad (`python -m aliparaformerasr_amd.convert vad.onnx out.pfw --kind fsmnvad
--mvn vad.mvn`); the model's default thresholds (floor_pct=-1, abs_level=9830; unvalidated too) apply unless keys are given.
`-spk FILE [key=value,...]` (with `-vad`; OfflineRecognizer.SetSpeakerModel) says who speaks in each segment: FILE is a `.pfw` of
kind campplus (`python -m aliparaformerasr_amd.convert campplus.bin out.pfw --kind campplus`); each segment line becomes
`[begin-end ms] spkN text`.  Keys: the pf_spk_config fields (win, shift, min_frames, threshold, num_speakers, min_cluster).  The
network and the thresholds are stated, not validated on a real model.
`-punc FILE` (OfflineRecognizer.SetPuncModel) punctuates every result on the GPU with a CT-Transformer: FILE is a `.pfw` of kind
cttransformer; under each result goes a `punctuated: ...` line and one `  [begin-end ms] sentence` line per sentence (without the
times when the result has no timestamp per word).  Rules and dimensions are stated, not validated on a real model.
`-align beam` (with `-nbest N -beam W`) aligns the beam search's labelings instead: under each `nbest[i]` line goes
`align[i] loglik:<...> pairs:[begin,end],...`.
`-endpoint [key=value,...]` (online; OnlineRecognizer.SetEndpoint) finds sentence ends while the file streams: above the partial
text of a chunk goes one `[begin-end ms] text` line per sentence that closed in it, the partial text is that of the open sentence,
and after the last chunk the input is declared finished (OnlineStream.InputFinished), which decodes the tail and closes what is
open.  Keys: the pf_endpoint_config fields (rise, margin_q, abs_level, window, on_count, off_count, pad_begin, pad_end,
end_silence, min_speech, max_len); the defaults are unvalidated on real speech.
`-vadmodel FILE` (with `-endpoint`; OnlineRecognizer.SetEndpointModel) takes the detector's level from an FSMN-VAD network (a
`.pfw` of kind fsmnvad, as above) with each stream's history carried between chunks; the model's default thresholds (rise=-1,
abs_level=9830; unvalidated too) apply unless keys are given.  A sentence line can come one chunk later than with the energy level.
`-secondpass NAME` (with `-endpoint`; OnlineRecognizer.SetSecondPass) re-recognises every finished sentence with the OFFLINE model
in directory NAME under -base (its files chosen as `-type offline` chooses them): the sentence lines then carry its text.
`-tokentimes` (online; OnlineRecognizer.SetTokenInfo) prints under each result one line of `token[time_ms score]` for the tokens
the stream fired (special tokens left out); with `-endpoint` also under each `[begin-end ms]` line, for the closed sentence.  A time is the start of the 60 ms frame in which the token fired, not a word boundary.
`-puncstream FILE[,max_context=N]` (online; OnlineRecognizer.SetPuncModel) punctuates the words as they arrive with a causal
CT-Transformer on the GPU (FILE: a .pfw made by `convert --kind cttransformer --causal`): a `punctuated: ...` line under each
partial result and under each finished sentence.  `-punc` stays an offline option.  Not validated on a real model."""
from __future__ import annotations

import ctypes as C
import os
import sys
import time

import numpy as np

from . import _native as N


def get_file_sample(path: str):
    """AudioHelper.GetFileSample -> (float32 samples, duration_ms)."""
    lib = N.load()
    n = C.c_int64(); sr = C.c_int32(); ch = C.c_int32(); dur = C.c_double()
    N.check(lib.pf_host_wav_read(path.encode(), None, 0, n, sr, ch, dur))
    out = np.zeros(max(n.value, 1), np.float32)
    N.check(lib.pf_host_wav_read(path.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, n, sr, ch, dur))
    return out[: n.value], dur.value


def get_file_pcm(path: str):
    """The file as OfflineStream.AddPcm takes it -> (payload bytes, sample_rate, channels, format name, duration_ms)."""
    desc = N.PfPcmDesc(); off = C.c_int64(); nb = C.c_int64(); dur = C.c_double()
    N.check(N.load().pf_host_wav_info(path.encode(), C.byref(desc), C.byref(off), C.byref(nb), C.byref(dur)))
    with open(path, "rb") as f:
        f.seek(off.value)
        payload = f.read(nb.value)
    name = next(k for k, v in N.PCM_FORMATS.items() if v[0] == desc.format)
    bps = N.PCM_FORMATS[name][1]
    return payload[: len(payload) // bps * bps], desc.sample_rate, desc.channels, name, dur.value


def is_audio_by_header(path: str) -> bool:
    v = C.c_int32(0)
    N.check(N.load().pf_host_is_audio(path.encode(), v))
    return bool(v.value)


def select_model_files(base: str, model: str, accuracy: str):
    folder = os.path.join(base, model)
    if not os.path.isdir(folder):
        print("Error: folder does not exist - %s" % folder)
        return None
    names = sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)))
    full = lambda f: os.path.join(base, model, f)

    def last(pred):
        m = [f for f in names if pred(f)]
        return full(m[-1]) if m else ""

    cands = [f for f in names if f.startswith("model") and "_eb" not in f]
    pref = [f for f in cands if (".%s." % accuracy) in f]
    model_path = full(pref[-1]) if pref else (full(cands[-1]) if cands else "")
    eb = [f for f in names if f.startswith("model_eb")]
    ebp = [f for f in eb if (".%s." % accuracy) in f]
    return dict(
        modelFilePath=model_path,
        modelebFilePath=full(ebp[-1]) if ebp else (full(eb[-1]) if eb else ""),
        configFilePath=last(lambda f: f.startswith("asr") and (f.endswith(".yaml") or f.endswith(".json"))),
        mvnFilePath=last(lambda f: f.startswith("am") and f.endswith(".mvn")),
        tokensFilePath=last(lambda f: f.startswith("tokens") and f.endswith(".txt")),
        hotwordFilePath=last(lambda f: f.startswith("hotword") and f.endswith(".txt")),
    )


# ---- the GUI's display step for SenseVoice results (AliParaformerAsr.Examples.MauiApp/Utils/AEDEmojiHelper.cs:7-47; callers
#      RecognitionForFiles.xaml.cs:478,583: `ReplaceTagsWithEmojis(result.Text.Replace("> ", ">"))`) — SURVEY §8f row 3
_EMOJI_MAP = {
    "Laughter": "\U0001F606", "Applause": "\U0001F44F", "HAPPY": "\U0001F600", "SAD": "\U0001F622", "ANGRY": "\U0001F621",
    "NEUTRAL": "\U0001F610", "FEARFUL": "\U0001F628", "DISGUSTED": "\U0001F922", "SURPRISED": "\U0001F632", "Cry": "\U0001F62D",
    "Sneeze": "\U0001F443\U0001F927", "Cough": "\U0001F912", "Sing": "\U0001F3A4",
}


def replace_tags_with_emojis(text: str) -> str:
    """AEDEmojiHelper.ReplaceTagsWithEmojis (:7-36): every `<|word|>` tag becomes its emoji, or nothing when the tag is
    not in the table (language / event / itn tags such as <|zh|>, <|Speech|>, <|woitn|> simply disappear)."""
    import re
    return re.sub(r"<\|(\w+)\|>", lambda m: _EMOJI_MAP.get(m.group(1), ""), text)


def replace_tags_with_empty(text: str) -> str:
    """AEDEmojiHelper.ReplaceTagsWithEmpty (:38-45): `<|...|>` (shortest match, anything but a newline inside) removed."""
    import re
    return re.sub(r"<\|.*?\|>", "", text)


def display_text(text: str) -> str:
    """What the GUI shows for a result (RecognitionForFiles.xaml.cs:478): DecodeMulti separates tags with "> "."""
    return replace_tags_with_emojis(text.replace("> ", ">"))


def _result_line(r) -> str:
    toks = ",".join('"%s"' % t for t in r.Tokens)
    ts = ",".join("[%d,%d]" % (t[0], t[-1]) for t in r.Timestamps)
    return '{"text": "%s","tokens":[%s],"timestamps":[%s]}' % (r.Text, toks, ts)


def _pairs(ts) -> str:
    return ",".join("[%d,%d]" % (t[0], t[-1]) for t in ts)


def _nbest_lines(stream, align=False) -> list:
    out = []
    for i, a in enumerate(stream.Alternatives):
        if a.LmSum is not None:
            hot = ' hot:%d lm:%.6f loglik_sum:%.6f' % (a.HotwordTokens, a.LmSum, a.LogLikSum)
        else:
            hot = '' if a.LogLikSum is None else ' hot:%d loglik_sum:%.6f' % (a.HotwordTokens, a.LogLikSum)
        out.append('nbest[%d] score:%.6f text:%s%s' % (i, a.Score, a.Text, hot))
        if align and a.LogLik is not None:
            out.append('align[%d] loglik:%.6f pairs:%s' % (i, a.LogLik, _pairs(a.Timestamps)))
    return out


def _align_lines(stream) -> list:
    a = stream.Alignment
    if a is None:
        return []
    return ['align ok:%d path:%.6f loglik:%.6f pairs:%s' % (a.Ok, a.PathScore, a.LogLik, _pairs(a.Timestamps))]


VAD_KEYS = ("floor_pct", "margin_q", "abs_level", "window", "on_count", "off_count", "pad_begin", "pad_end", "min_speech", "max_len",
            "split_search")


def parse_vad_option(text: str) -> dict:
    """`key=value,...` of -vad -> {"cfg": {pf_vad_config fields}, "batch_max", "frame_budget", "sep"}"""
    out = {"cfg": {}, "batch_max": 0, "frame_budget": 0, "sep": ""}
    for item in [x for x in text.split(",") if x]:
        k, eq, v = item.partition("=")
        k = k.strip()
        if not eq:
            raise ValueError("-vad takes key=value pairs: %r" % item)
        if k == "sep":
            out["sep"] = v
            continue
        try:
            iv = int(v)
        except ValueError:
            raise ValueError("The -vad value of %s must be an integer" % k)
        if k in VAD_KEYS:
            out["cfg"][k] = iv
        elif k in ("batch_max", "frame_budget"):
            out[k] = iv
        else:
            raise ValueError("Unknown -vad key: %s" % k)
    return out


ENDPOINT_KEYS = ("rise", "margin_q", "abs_level", "window", "on_count", "off_count", "pad_begin", "pad_end", "end_silence", "min_speech",
                 "max_len")


def parse_puncstream_option(text: str) -> dict:
    """`FILE[,max_context=N]` of -puncstream -> {file, max_context}"""
    parts = text.split(",")
    out = {"file": parts[0], "max_context": 0}
    if not parts[0]:
        raise ValueError("-puncstream takes a causal .pfw file of kind cttransformer[,max_context=N]")
    for item in parts[1:]:
        k, _, v = item.partition("=")
        if k != "max_context":
            raise ValueError("Unknown -puncstream key: %s" % k)
        try:
            out["max_context"] = int(v)
        except ValueError:
            raise ValueError("The -puncstream value of max_context must be an integer")
        if not 2 <= out["max_context"] <= 256:
            raise ValueError("-puncstream max_context lies in 2 .. 256")
    return out


def parse_endpoint_option(text: str) -> dict:
    """`key=value,...` of -endpoint -> {pf_endpoint_config fields}"""
    out = {}
    for item in [x for x in text.split(",") if x]:
        k, eq, v = item.partition("=")
        k = k.strip()
        if not eq:
            raise ValueError("-endpoint takes key=value pairs: %r" % item)
        if k not in ENDPOINT_KEYS:
            raise ValueError("Unknown -endpoint key: %s" % k)
        try:
            out[k] = int(v)
        except ValueError:
            raise ValueError("The -endpoint value of %s must be an integer" % k)
    return out


SPK_KEYS = ("win", "shift", "min_frames", "threshold", "num_speakers", "min_cluster")


def parse_spk_option(text: str) -> dict:
    """`key=value,...` of -spk -> {pf_spk_config fields}"""
    out = {}
    for item in [x for x in text.split(",") if x]:
        k, eq, v = item.partition("=")
        k = k.strip()
        if not eq:
            raise ValueError("-spk takes key=value pairs: %r" % item)
        if k not in SPK_KEYS:
            raise ValueError("Unknown -spk key: %s" % k)
        try:
            out[k] = float(v) if k == "threshold" else int(v)
        except ValueError:
            raise ValueError("The -spk value of %s must be %s" % (k, "a number" if k == "threshold" else "an integer"))
        if out[k] != out[k]:
            raise ValueError("The -spk value of %s must be a number" % k)
    return out


def _segment_lines(stream, speakers=False) -> list:
    spk = stream.SegmentSpeakers if speakers else []
    return ["[%d-%d ms] %s%s" % (g.BeginMs, g.EndMs, ("spk%d " % spk[i]) if i < len(spk) and spk[i] >= 0 else "", g.Text)
            for i, g in enumerate(stream.Segments)]


def read_align_file(path: str) -> list:
    """one line of space-separated token ids per input file; an empty line means no target for that file"""
    out = []
    with open(path, encoding="utf-8") as f:
        for ln in f.read().splitlines():
            try:
                out.append([int(x) for x in ln.split()] if ln.strip() else None)
            except ValueError:
                raise ValueError("The align file holds token ids (integers), one line per input file: %r" % ln)
    return out


def _punc_lines(st):
    """-punc: the punctuated line, then one line per sentence (with its times where the result has one timestamp per word)"""
    out = ["punctuated: " + st.Punctuated]
    for z in st.Sentences:
        out.append(("  [%d-%d ms] " % tuple(z.Times) if z.Times else "  ") + z.Text)
    return out


def offline_recognizer(method="one", model="paraformer-seaco-large-zh-timestamp-onnx-offline", accuracy="int8",
                       threads=2, files=None, base=None, out=sys.stdout, decode="frames", intake="host", nbest=0, topk=4,
                       beam=0, align=None, hotboost=0.0, vad=None, lm=None, lmweight=0.5, lmbonus=0.0, lmeos=False, search=0, vadmodel=None, punc=None, spk=None):
    from .offline_recognizer import OfflineRecognizer
    base = base or os.getcwd()
    sel = select_model_files(base, model, accuracy)
    if sel is None or not sel["modelFilePath"] or not sel["tokensFilePath"]:
        print("Init models failure!", file=out)
        return None
    t0 = time.perf_counter()
    rec = OfflineRecognizer(threadsNum=threads, **sel)
    if decode == "ctc":
        rec.SetDecode(ctc=True)
    if nbest and beam:
        rec.SetCtcBeam(nbest, beam, topk)
        if hotboost:
            rec.SetHotwordBoost(hotboost)
        if lm:
            rec.SetLm(lm, lmweight, lmbonus, 1 if lmeos else 0)
    elif nbest:
        rec.SetNBest(nbest, topk)
        if search:
            rec.SetNBestSearch(search)
            if hotboost:
                rec.SetNBestHotwordBoost(hotboost)
            if lm:
                rec.SetNBestLm(lm, lmweight, lmbonus, 1 if lmeos else 0)
    if vad is not None:
        vcfg = vad["cfg"] or True
        if vadmodel:                                       # the model's default thresholds unless keys are given
            from .engine import vad_model_config
            rec.SetVadModel(vadmodel)
            vcfg = vad_model_config(**vad["cfg"])
        rec.SetVad(vcfg, vad["batch_max"], vad["frame_budget"], vad["sep"])
    if spk:
        rec.SetSpeakerModel(spk["file"], spk["cfg"] or None)
    if punc:
        rec.SetPuncModel(punc)
    targets = None
    if align:
        rec.SetAlign(True)
        if align != "beam":
            targets = dict(zip(files or [], read_align_file(align)))
    print("init_models_elapsed_milliseconds:%s" % ((time.perf_counter() - t0) * 1e3), file=out)
    if not files:
        files = []
        for d, _dirs, fs in os.walk(os.path.join(base, model)):
            files += [os.path.join(d, f) for f in sorted(fs) if f.lower().endswith(".wav")]
    samples, paths, total_ms = [], [], 0.0
    for f in files:
        if not os.path.isfile(f) or not is_audio_by_header(f):
            continue
        if intake == "device":
            pcm = get_file_pcm(f)
            s, dur = pcm[:4], pcm[4]
        else:
            s, dur = get_file_sample(f)
        paths.append(f); samples.append(s); total_ms += dur
    if not samples:
        print("No media file is read!", file=out)
        return None
    print("Automatic speech recognition in progress!", file=out)
    t0 = time.perf_counter()
    method = method or "batch"
    results = []

    def add(st, s):
        if isinstance(s, tuple):
            st.AddPcm(s[0], s[1], s[2], s[3])
        else:
            st.AddSamples(s)

    def extra_lines(st):
        return (_nbest_lines(st, align == "beam") if nbest else []) + (_align_lines(st) if targets is not None else []) + \
            (_segment_lines(st, bool(spk)) if vad is not None else []) + (_punc_lines(st) if punc else [])
    print("Recognition results:\r\n", file=out)
    try:
        if method == "one":
            for p, s in zip(paths, samples):
                st = rec.CreateOfflineStream()
                add(st, s)
                if targets is not None and targets.get(p) is not None:
                    st.SetAlignIds(targets[p])
                r = rec.GetResult(st)
                results.append(r)
                print(p, file=out); print(_result_line(r), file=out)
                for ln in extra_lines(st):
                    print(ln, file=out)
                print("", file=out)
        elif method == "batch":
            streams = []
            for p, s in zip(paths, samples):
                st = rec.CreateOfflineStream()
                add(st, s)
                if targets is not None and targets.get(p) is not None:
                    st.SetAlignIds(targets[p])
                streams.append(st)
            results = rec.GetResults(streams)
            for p, r, st in zip(paths, results, streams):
                print(p, file=out); print(_result_line(r), file=out)
                for ln in extra_lines(st):
                    print(ln, file=out)
                print("", file=out)
    except Exception as ex:          # the reference prints the message and carries on to the timing lines
        print(str(ex), file=out)
    rec.Dispose()
    elapsed = (time.perf_counter() - t0) * 1e3
    print("recognition_elapsed_milliseconds:%s" % elapsed, file=out)
    print("total_duration_milliseconds:%s" % total_ms, file=out)
    print("rtf:%s" % (elapsed / total_ms if total_ms else float("inf")), file=out)
    print("end!", file=out)
    return results


def select_online_model_files(base: str, model: str, accuracy: str):
    """OnlineAliParaformerAsrRecognizer.cs:15-84 (the containers here are .pfw instead of .onnx)."""
    folder = os.path.join(base, model)
    if not os.path.isdir(folder):
        print("Error: folder does not exist - %s" % folder)
        return None
    names = sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)))
    full = lambda f: os.path.join(base, model, f)

    def pick(cands):
        pref = [f for f in cands if (".%s." % accuracy) in f]
        return full(pref[-1]) if pref else (full(cands[-1]) if cands else "")

    def last(pred):
        m = [f for f in names if pred(f)]
        return full(m[-1]) if m else ""
    return dict(
        encoderFilePath=pick([f for f in names if f.startswith("model") or f.startswith("encoder")]),
        decoderFilePath=pick([f for f in names if f.startswith("decoder")]),
        configFilePath=last(lambda f: f.startswith("asr") and (f.endswith(".yaml") or f.endswith(".json"))),
        mvnFilePath=last(lambda f: f.startswith("am") and f.endswith(".mvn")),
        tokensFilePath=last(lambda f: f.startswith("tokens")),
    )


def get_file_chunk_samples(path: str, chunk: int = 160 * 6 * 10):
    """AudioHelper.GetFileChunkSamples (:80-127): GetFileSample's samples cut into 9600-sample pieces, the last one shorter."""
    s, dur = get_file_sample(path)
    return [s[i: i + chunk] for i in range(0, len(s), chunk)], dur


SPECIAL_TOKENS = ("</s>", "<s>", "<blank>", "<unk>")


def read_token_table(path):
    with open(path, encoding="utf-8") as f:
        return [ln.rstrip("\n") for ln in f]


def token_times_line(info, names):
    """`token[time_ms score]` for the fired, non-special tokens of OnlineStream.TokenInfo, up to the first </s> (id 2: where
    the text ends too)"""
    out = []
    for t in info:
        if t.id == 2:
            break
        name = names[t.id] if 0 <= t.id < len(names) else "<%d>" % t.id
        if t.fired and name not in SPECIAL_TOKENS:
            out.append("%s[%d %.3f]" % (name, t.time_ms, t.score))
    return " ".join(out)


def online_recognizer(method="one", model="speech_paraformer-large_asr_nat-zh-cn-16k-common-vocab8404-online-onnx",
                      accuracy="int8", threads=2, files=None, base=None, out=sys.stdout, endpoint=None, secondpass=None, vadmodel=None,
                      tokentimes=False, puncstream=None):
    from .online_recognizer import OnlineRecognizer
    base = base or os.getcwd()
    if not model:
        print("Init models failure!", file=out)
        return None
    sel = select_online_model_files(base, model, accuracy)
    if sel is None or not sel["encoderFilePath"] or not sel["tokensFilePath"]:
        print("Init models failure!", file=out)
        return None
    t0 = time.perf_counter()
    try:
        rec = OnlineRecognizer(threadsNum=threads, **sel)
    except Exception as ex:                                 # :97-100
        print("Error occurred: %s" % ex, file=out)
        print("Init models failure!", file=out)
        return None
    second = None
    if tokentimes:
        rec.SetTokenInfo(True)
        names = read_token_table(sel["tokensFilePath"])
    if puncstream:
        try:
            rec.SetPuncModel(puncstream["file"], puncstream.get("max_context", 0))
        except Exception as ex:
            print("Error occurred: %s" % ex, file=out)
            print("Init models failure!", file=out)
            return None
    if endpoint is not None:
        try:
            if vadmodel:                                    # the model's default thresholds unless keys are given
                from .engine import endpoint_model_config
                rec.SetEndpointModel(vadmodel)
                rec.SetEndpoint(endpoint_model_config(**endpoint))
            else:
                rec.SetEndpoint(**endpoint)
            if secondpass:                                  # the offline model's directory under -base, chosen as -type offline does
                from .offline_recognizer import OfflineRecognizer
                osel = select_model_files(base, secondpass, accuracy)
                if osel is None:
                    raise ValueError("no offline model in %s" % secondpass)
                second = OfflineRecognizer(threadsNum=threads, **osel)
                rec.SetSecondPass(second)
        except Exception as ex:
            print("Error occurred: %s" % ex, file=out)
            print("Init models failure!", file=out)
            return None
    print("init_models_elapsed_milliseconds:%s" % ((time.perf_counter() - t0) * 1e3), file=out)
    t0 = time.perf_counter()                                # :126: the window opens before the files are read
    if not files:
        files = []
        for d, _dirs, fs in os.walk(os.path.join(base, model)):
            files += [os.path.join(d, f) for f in sorted(fs) if f.lower().endswith(".wav")]
    samples_list, total_ms, n = [], 0.0, 0
    for f in files:
        if n >= 2:                                          # batchSize = 2 (:129, :152-155)
            break
        if not os.path.isfile(f):
            continue
        if is_audio_by_header(f):
            chunks, dur = get_file_chunk_samples(f)
            if chunks:
                chunks += [np.zeros(400, np.float32) for _ in range(6)]          # :160-163
                samples_list.append(chunks)
                total_ms += dur
        n += 1
    if not samples_list:
        print("No media file is read!", file=out)
        return None
    method = method or "batch"
    texts = []
    if method == "one":                                     # :176-194 (the only method the reference runs)
        for chunks in samples_list:
            st = rec.CreateOnlineStream()
            shown = 0

            def step():
                nonlocal shown
                r = rec.GetResult(st)
                if endpoint is not None:                    # a line per sentence that closed in this call, then the open one's text
                    sens = st.Sentences
                    for sen in sens[shown:]:
                        print("[%d-%d ms] %s" % (sen.begin_ms, sen.end_ms, sen.text), file=out)
                        if tokentimes:                      # TokenInfo was cleared at the reset: the sentence kept its own
                            print(token_times_line(sen.tokens, names), file=out)
                        if puncstream:
                            print("punctuated: " + sen.punctuated, file=out)
                    shown = len(sens)
                print(r.Text, file=out)
                if tokentimes:
                    print(token_times_line(st.TokenInfo, names), file=out)
                if puncstream:
                    print("punctuated: " + st.Punctuated, file=out)
                texts.append(r.Text)
            for c in chunks:
                st.AddSamples(c)
                step()
            if endpoint is not None or puncstream:
                st.InputFinished()
                for _ in range(3):                          # the padded tail, then the flush
                    step()
    rec.Dispose()
    if second is not None:
        second.Dispose()
    elapsed = (time.perf_counter() - t0) * 1e3
    print("elapsed_milliseconds:%s" % elapsed, file=out)
    print("total_duration:%s" % total_ms, file=out)
    print("rtf:%s" % (elapsed / total_ms if total_ms else float("inf")), file=out)
    print("Hello, World!", file=out)
    return texts


def parse_args(argv, env=None):
    # environment variables are the defaults, command-line parameters overwrite them (Program.cs:20-28, :93-104)
    env = os.environ if env is None else env
    try:
        threads = int(env.get("MANYSPEECH_THREADS", "2"))
    except ValueError:
        raise ValueError("The number of threads must be a valid integer")
    cfg = dict(modelBasePath=env.get("MANYSPEECH_BASE", ""), recognizerType=env.get("MANYSPEECH_TYPE"),
               methodType=env.get("MANYSPEECH_BATCH", "one"), modelName=env.get("MANYSPEECH_MODEL", "default-model"),
               modelAccuracy=env.get("MANYSPEECH_ACCURACY", "int8"), threads=threads, files=[])
    i = 0
    while i < len(argv):
        a = argv[i].lower()
        if a in ("-base", "-type", "-method", "-model", "-accuracy"):
            key = {"-base": "modelBasePath", "-type": "recognizerType", "-method": "methodType", "-model": "modelName",
                   "-accuracy": "modelAccuracy"}[a]
            if i + 1 < len(argv):
                i += 1
                cfg[key] = argv[i]
        elif a == "-decode":
            i += 1
            if i >= len(argv) or argv[i].lower() not in ("ctc", "frames"):
                raise ValueError("The decode type must be ctc or frames")
            cfg["decode"] = argv[i].lower()
        elif a == "-intake":
            i += 1
            if i >= len(argv) or argv[i].lower() not in ("host", "device"):
                raise ValueError("The intake type must be host or device")
            cfg["intake"] = argv[i].lower()
        elif a in ("-nbest", "-topk", "-beam", "-search"):
            lo, hi = (1, N.PF_TOPK_MAX) if a == "-topk" else (1, N.PF_NBEST_MAX)
            try:
                i += 1
                v = int(argv[i])
            except (IndexError, ValueError):
                v = 0
            if not lo <= v <= hi:
                raise ValueError("The %s value must be an integer from %d to %d" % (a[1:], lo, hi))
            cfg[a[1:]] = v
        elif a == "-hotboost":
            try:
                i += 1
                v = float(argv[i])
            except (IndexError, ValueError):
                v = -1.0
            if not (0.0 <= v < float("inf")):
                raise ValueError("The hotboost value must be a finite number >= 0")
            cfg["hotboost"] = v
        elif a == "-lm":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-lm takes an ARPA file")
            cfg["lm"] = argv[i]
        elif a in ("-lmweight", "-lmbonus"):
            try:
                i += 1
                v = float(argv[i])
            except (IndexError, ValueError):
                v = float("nan")
            if not (abs(v) < float("inf")) or (a == "-lmweight" and v < 0):
                raise ValueError("The %s value must be a finite number%s" % (a[1:], " >= 0" if a == "-lmweight" else ""))
            cfg[a[1:]] = v
        elif a == "-lmeos":
            cfg["lmeos"] = True
        elif a == "-align":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-align takes a file of token ids, or `beam`")
            cfg["align"] = argv[i]
        elif a == "-vad":
            text = ""
            if i + 1 < len(argv) and not argv[i + 1].startswith("-") and "=" in argv[i + 1]:
                i += 1
                text = argv[i]
            cfg["vad"] = parse_vad_option(text)
        elif a == "-endpoint":
            text = ""
            if i + 1 < len(argv) and not argv[i + 1].startswith("-") and "=" in argv[i + 1]:
                i += 1
                text = argv[i]
            cfg["endpoint"] = parse_endpoint_option(text)
        elif a == "-tokentimes":
            cfg["tokentimes"] = True
        elif a == "-secondpass":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-secondpass takes the offline model's directory name")
            cfg["secondpass"] = argv[i]
        elif a == "-vadmodel":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-vadmodel takes a .pfw file of kind fsmnvad")
            cfg["vadmodel"] = argv[i]
        elif a == "-spk":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-spk takes a .pfw file of kind campplus")
            cfg["spk"] = {"file": argv[i], "cfg": {}}
            if i + 1 < len(argv) and not argv[i + 1].startswith("-") and "=" in argv[i + 1]:
                i += 1
                cfg["spk"]["cfg"] = parse_spk_option(argv[i])
        elif a == "-puncstream":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-puncstream takes a causal .pfw file of kind cttransformer[,max_context=N]")
            cfg["puncstream"] = parse_puncstream_option(argv[i])
        elif a == "-punc":
            i += 1
            if i >= len(argv) or argv[i].startswith("-"):
                raise ValueError("-punc takes a .pfw file of kind cttransformer")
            cfg["punc"] = argv[i]
        elif a == "-threads":
            try:
                i += 1
                cfg["threads"] = int(argv[i])
            except (IndexError, ValueError):
                raise ValueError("The number of threads must be a valid integer")
        elif a == "-files":
            fs = []
            while i + 1 < len(argv) and not argv[i + 1].startswith("-"):
                i += 1
                fs.append(argv[i].strip('"'))
            cfg["files"] = fs
        else:
            raise ValueError("Unknown parameters: %s" % argv[i])
        i += 1
    if cfg["recognizerType"] is None:
        raise ValueError("You must specify the recognizer type (-type online/offline)")
    if "topk" in cfg and "nbest" not in cfg:
        raise ValueError("-topk goes with -nbest")
    if "beam" in cfg and "nbest" not in cfg:
        raise ValueError("-beam goes with -nbest")
    if "beam" in cfg and cfg["beam"] < cfg["nbest"]:
        raise ValueError("The beam value must not be smaller than the nbest value")
    if "search" in cfg and "nbest" not in cfg:
        raise ValueError("-search goes with -nbest")
    if "search" in cfg and "beam" in cfg:
        raise ValueError("-search (paraformer) and -beam (SenseVoice) do not go together")
    if "hotboost" in cfg and "beam" not in cfg and "search" not in cfg:
        raise ValueError("-hotboost needs -nbest N -beam W")
    if "lm" in cfg and "beam" not in cfg and "search" not in cfg:
        raise ValueError("-lm needs -nbest N -beam W")
    if any(k in cfg for k in ("lmweight", "lmbonus", "lmeos")) and "lm" not in cfg:
        raise ValueError("-lmweight, -lmbonus and -lmeos go with -lm FILE")
    if "nbest" in cfg and cfg["recognizerType"] != "offline":
        raise ValueError("-nbest is an offline option")
    if "align" in cfg and cfg["recognizerType"] != "offline":
        raise ValueError("-align is an offline option")
    if "vad" in cfg and cfg["recognizerType"] != "offline":
        raise ValueError("-vad is an offline option")
    if "vad" in cfg and ("nbest" in cfg or "align" in cfg):
        raise ValueError("-vad does not go with -nbest or -align")
    if "endpoint" in cfg and cfg["recognizerType"] != "online":
        raise ValueError("-endpoint is an online option")
    if "secondpass" in cfg and "endpoint" not in cfg:
        raise ValueError("-secondpass goes with -endpoint")
    if "punc" in cfg and cfg["recognizerType"] != "offline":
        raise ValueError("-punc is an offline option")
    if "spk" in cfg and "vad" not in cfg:
        raise ValueError("-spk goes with -vad")
    if "puncstream" in cfg and cfg.get("recognizerType") != "online":
        raise ValueError("-puncstream goes with -type online")
    if "tokentimes" in cfg and cfg.get("recognizerType") != "online":
        raise ValueError("-tokentimes goes with -type online")
    if "vadmodel" in cfg and "vad" not in cfg and "endpoint" not in cfg:
        raise ValueError("-vadmodel goes with -vad (offline) or -endpoint (online)")
    if cfg.get("align") == "beam" and "beam" not in cfg:
        raise ValueError("-align beam needs -nbest N -beam W")
    return cfg


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        cfg = parse_args(argv)
    except ValueError as ex:
        print("parameter error: %s" % ex)
        return 2
    # Program.cs:290-308
    if cfg["recognizerType"] == "online":
        online_recognizer(cfg["methodType"], cfg["modelName"], cfg["modelAccuracy"], cfg["threads"], cfg["files"],
                          cfg["modelBasePath"] or None, endpoint=cfg.get("endpoint"), secondpass=cfg.get("secondpass"),
                          vadmodel=cfg.get("vadmodel"), tokentimes=bool(cfg.get("tokentimes")), puncstream=cfg.get("puncstream"))
    elif cfg["recognizerType"] == "offline":
        offline_recognizer(cfg["methodType"], cfg["modelName"], cfg["modelAccuracy"], cfg["threads"], cfg["files"],
                           cfg["modelBasePath"] or None, decode=cfg.get("decode", "frames"), intake=cfg.get("intake", "host"),
                           nbest=cfg.get("nbest", 0), topk=cfg.get("topk", 4), beam=cfg.get("beam", 0), align=cfg.get("align"),
                           hotboost=cfg.get("hotboost", 0.0), vad=cfg.get("vad"), lm=cfg.get("lm"), lmweight=cfg.get("lmweight", 0.5),
                           lmbonus=cfg.get("lmbonus", 0.0), lmeos=cfg.get("lmeos", False), search=cfg.get("search", 0),
                           vadmodel=cfg.get("vadmodel"), punc=cfg.get("punc"), spk=cfg.get("spk"))
    else:
        print("the recognizer type must be online or offline")
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
