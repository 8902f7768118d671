"""Python face of the drop-in API: same names, argument meaning and error behaviour as the
reference's public C# classes

    OfflineRecognizer  AliParaformerAsr/OfflineRecognizer.cs:13-477
    OfflineStream      AliParaformerAsr/OfflineStream.cs:7-121
    OfflineRecognizerResultEntity  AliParaformerAsr/Model/OfflineRecognizerResultEntity.cs:9-29

All logic lives in libparaformer_hip.so (C++ host mirror + HIP engine); this file is the
ctypes stub a Python caller uses, exactly as INTEGRATION.md's P/Invoke stub is for C#.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _native as N


class ObjectDisposedException(RuntimeError):
    def __init__(self, object_name: str):
        super().__init__(f"Cannot access a disposed object.\nObject name: '{object_name}'.")
        self.ObjectName = object_name


class ArgumentNullException(ValueError):
    def __init__(self, param_name: str):
        super().__init__(f"Value cannot be null. (Parameter '{param_name}')")
        self.ParamName = param_name


class RecognizerException(Exception):
    """`throw new Exception(message, inner)` of the reference."""


def _raise(code: int):
    msg = N.load().pf_last_error()
    msg = msg.decode("utf-8", "replace") if msg else ""
    if code == N.PF_ERR_TOKENS:
        raise RecognizerException("tokens invalid")
    if code == N.PF_ERR_DISPOSED:
        raise ObjectDisposedException(msg or "OfflineRecognizer")
    if code == N.PF_ERR_NULL_SAMPLES:
        raise ArgumentNullException(msg or "source")
    if code == N.PF_ERR_RECOGNITION:
        raise RecognizerException("Offline recognition failed" if not msg.startswith("Offline recognition failed")
                                  else msg)
    raise N.PfError(code, msg)


def _ck(code: int) -> int:
    if code < 0:
        _raise(code)
    return code


@dataclass
class OfflineRecognizerResultEntity:
    Text: Optional[str] = None
    TextLen: int = 0
    Tokens: List[str] = field(default_factory=list)
    Timestamps: List[List[int]] = field(default_factory=list)


@dataclass
class Alternative:
    """One entry of OfflineStream.Alternatives: the ids of every position, Score = the sum of their log-probs, and the Text /
    Tokens DecodeMulti makes of them."""
    Ids: List[int] = field(default_factory=list)
    Score: float = 0.0
    Text: str = ""
    Tokens: List[str] = field(default_factory=list)
    # OfflineRecognizer.SetAlign beside SetCtcBeam: one [begin, end] pair in ms per id from the labeling's own forced alignment
    # (empty without), and the log of the sum over ALL of its alignments (None without)
    Timestamps: List[List[int]] = field(default_factory=list)
    LogLik: Optional[float] = None
    # OfflineRecognizer.SetHotwordBoost beside SetCtcBeam: the hot-word tokens the labeling completed (Score = LogLikSum + boost *
    # HotwordTokens) and the unbiased log of the alignments the search summed (0 / None when the search ran unbiased)
    HotwordTokens: int = 0
    LogLikSum: Optional[float] = None
    # OfflineRecognizer.SetLm beside SetCtcBeam: the weighted language-model score of the labeling, Score = (LogLikSum + boost *
    # HotwordTokens) + LmSum (None when the search ran without a model; LogLikSum is then filled with or without hot words)
    LmSum: Optional[float] = None


@dataclass
class Alignment:
    """OfflineStream.Alignment: the forced alignment of the stream's target ids (OfflineStream.SetAlignIds) to its audio.
    Ok = 0: the target does not fit the audio (more ids than frames); Timestamps / Scores are then empty."""
    Ok: int = 0
    PathScore: float = 0.0                 # float32 log-prob of the best alignment
    LogLik: float = 0.0                    # float64 log P(target | audio): the sum over all alignments
    Timestamps: List[List[int]] = field(default_factory=list)   # [begin, end] ms per id
    Scores: List[float] = field(default_factory=list)           # per id: the largest log-prob of its run


@dataclass
class Sentence:
    """OfflineStream.Sentences: one sentence of the punctuated text (OfflineRecognizer.SetPuncModel): the words [WordBegin,
    WordEnd), its text, and Times = [begin of its first word, end of its last] in ms when the result has exactly one
    Timestamps entry per word, else []."""
    WordBegin: int = 0
    WordEnd: int = 0
    Times: List[int] = field(default_factory=list)
    Text: str = ""


@dataclass
class Segment:
    """OfflineStream.Segments: one speech piece of a long stream (OfflineRecognizer.SetVad).  [BeginMs, EndMs) on the stream's
    clock; Batch / Row: where the piece ran in the call's batch plan; [TokBegin, TokEnd): its share of the stream's Tokens,
    Scores and Timestamps; Text: its own text."""
    BeginMs: int = 0
    EndMs: int = 0
    Batch: int = 0
    Row: int = 0
    TokBegin: int = 0
    TokEnd: int = 0
    Text: str = ""


@dataclass
class FrontendConfEntity:
    """Model/FrontendConfEntity.cs:6-28 (defaults included)."""
    fs: int = 16000
    window: str = "hamming"
    n_mels: int = 80
    frame_length: int = 25
    frame_shift: int = 10
    dither: float = 1.0
    lfr_m: int = 7
    lfr_n: int = 6
    snip_edges: bool = False


@dataclass
class ConfEntity:
    """Model/ConfEntity.cs: only what OfflineStream's constructor reads (frontend_conf)."""
    frontend_conf: FrontendConfEntity = field(default_factory=FrontendConfEntity)


@dataclass
class OfflineInputEntity:
    """Model/OfflineInputEntity.cs:6-11."""
    Speech: Optional[np.ndarray] = None
    SpeechLength: int = 0
    Hotwords: Optional[List[List[int]]] = field(default_factory=list)


class OfflineStream:
    Hyp: List[int] = [0, 0]                 # OfflineStream.cs:24,31 (per instance below)

    def __init__(self, mvnFilePath=None, confEntity=None, *, _lib=None, _handle=None, _recognizer=None):
        """Public form: OfflineStream(mvnFilePath, confEntity) (OfflineStream.cs:20-28) — a stream that belongs to no
        recognizer yet; the first GetResults that receives it adopts it.  CreateOfflineStream uses the private form."""
        self.Hyp = [0, 0]                   # OfflineStream.cs:24,31: never read again by the reference
        if _handle is not None:
            self._lib, self._h, self._recognizer = _lib, _handle, _recognizer
            return
        self._lib = N.load()
        self._recognizer = None
        f = (confEntity or ConfEntity()).frontend_conf
        h = C.c_void_p()
        _ck(self._lib.pf_stream_create((mvnFilePath or "").encode("utf-8"), f.fs, f.n_mels, f.lfr_m, f.lfr_n,
                                       1 if f.snip_edges else 0, float(f.dither), (f.window or "").encode("utf-8"),
                                       C.byref(h)))
        self._h = h

    def AddSamples(self, samples) -> None:
        if samples is None:
            _ck(self._lib.pf_stream_add_samples(self._h, None, 0))
            return
        x = np.ascontiguousarray(samples, dtype=np.float32)
        _ck(self._lib.pf_stream_add_samples(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0]))

    def AddPcm(self, data, sample_rate: int, channels: int = 1, format: str = "s16", downmix_always: bool = False) -> None:
        """AddSamples for audio as callers hold it: raw interleaved PCM (bytes, or a numpy array of the format's dtype —
        "u8", "s16", "s24" (bytes), "s32", "f32", "f64", "alaw", "mulaw") at any rate, mono or stereo.  Decoded, down-mixed and
        resampled to the model's rate exactly as the Examples' GetFileSample does (a stereo stream AT the model's rate stays
        interleaved unless downmix_always), on the device for the first call on a recognizer's stream."""
        if data is None:
            _ck(self._lib.pf_stream_add_pcm(self._h, None, 0, C.byref(N.pcm_desc(sample_rate, channels, format, downmix_always))))
            return
        raw, n = N.pcm_bytes(data, format)
        keep = raw if raw.size else np.zeros(1, np.uint8)
        _ck(self._lib.pf_stream_add_pcm(self._h, keep.ctypes.data, n, C.byref(N.pcm_desc(sample_rate, channels, format, downmix_always))))

    @property
    def Hotwords(self) -> Optional[List[List[int]]]:
        n = C.c_int32()
        ids = (C.c_int32 * 4096)()
        lens = (C.c_int32 * 1024)()
        _ck(self._lib.pf_stream_get_hotwords(self._h, ids, 4096, lens, 1024, n))
        if n.value < 0:
            return None
        out, off = [], 0
        for i in range(n.value):
            out.append(list(ids[off: off + lens[i]]))
            off += lens[i]
        return out

    @Hotwords.setter
    def Hotwords(self, value: Optional[List[List[int]]]) -> None:
        if value is None:
            _ck(self._lib.pf_stream_set_hotwords(self._h, None, None, -1))
            return
        flat = [v for hw in value for v in hw]
        ids = (C.c_int32 * max(len(flat), 1))(*flat)
        lens = (C.c_int32 * max(len(value), 1))(*[len(hw) for hw in value])
        _ck(self._lib.pf_stream_set_hotwords(self._h, ids, lens, len(value)))

    @property
    def Tokens(self) -> List[int]:
        p = C.POINTER(C.c_int64)()
        n = C.c_int32()
        _ck(self._lib.pf_stream_tokens(self._h, C.byref(p), n))
        return [p[i] for i in range(n.value)]

    @Tokens.setter
    def Tokens(self, value: List[int]) -> None:
        a = (C.c_int64 * max(len(value), 1))(*value)
        _ck(self._lib.pf_stream_set_tokens(self._h, a, len(value)))

    @property
    def Scores(self) -> List[float]:
        """Scores of the last GetResults, parallel to Tokens (OfflineRecognizer.SetDecode; empty without it)."""
        p = C.POINTER(C.c_float)()
        n = C.c_int32()
        _ck(self._lib.pf_stream_scores(self._h, C.byref(p), n))
        return [p[i] for i in range(n.value)]

    @property
    def TokenAlternatives(self) -> List[List[tuple]]:
        """Per entry of Tokens the K best (id, log-prob) pairs of the last GetResults, best first (OfflineRecognizer.SetNBest;
        empty without it).  Slots a position could not fill hold (-1, -inf)."""
        pi, pv = C.POINTER(C.c_int64)(), C.POINTER(C.c_float)()
        n, k = C.c_int32(), C.c_int32()
        _ck(self._lib.pf_stream_token_alternatives(self._h, C.byref(pi), C.byref(pv), n, k))
        K = k.value
        return [[(pi[t * K + j], pv[t * K + j]) for j in range(K)] for t in range(n.value)]

    @property
    def Alternatives(self) -> List["Alternative"]:
        """The n-best list of the last GetResults (paraformer, OfflineRecognizer.SetNBest with N > 1: entry 0 is the result
        itself; SenseVoice, OfflineRecognizer.SetCtcBeam: the beam search's labelings; else empty), by descending Score."""
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_alternatives(self._h, n))
        out = []
        for i in range(n.value):
            p, k, sc, txt, nt = C.POINTER(C.c_int64)(), C.c_int32(), C.c_double(), C.c_char_p(), C.c_int32()
            _ck(self._lib.pf_stream_alternative(self._h, i, C.byref(p), k, C.byref(sc), C.byref(txt), nt))
            toks = []
            for j in range(nt.value):
                t = C.c_char_p()
                _ck(self._lib.pf_stream_alternative_token(self._h, i, j, C.byref(t)))
                toks.append((t.value or b"").decode("utf-8"))
            pt, nts, ll = C.POINTER(C.c_int32)(), C.c_int32(), C.c_double()
            _ck(self._lib.pf_stream_alternative_timestamps(self._h, i, C.byref(pt), nts, C.byref(ll)))
            hm, hs = C.c_int32(), C.c_double()
            _ck(self._lib.pf_stream_alternative_hot(self._h, i, hm, hs))
            lm = C.c_double()
            _ck(self._lib.pf_stream_alternative_lm(self._h, i, lm, None))
            out.append(Alternative(Ids=[p[m] for m in range(k.value)], Score=sc.value, HotwordTokens=hm.value,
                                   LogLikSum=None if hs.value != hs.value else hs.value,
                                   LmSum=None if lm.value != lm.value else lm.value,
                                   Text=(txt.value or b"").decode("utf-8"), Tokens=toks,
                                   Timestamps=[[pt[2 * j], pt[2 * j + 1]] for j in range(nts.value)],
                                   LogLik=None if ll.value != ll.value else ll.value))
        return out

    @property
    def Segments(self) -> List["Segment"]:
        """The pieces the last GetResults cut this stream into, in time order (OfflineRecognizer.SetVad; empty without it)."""
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_segments(self._h, n))
        out = []
        for i in range(n.value):
            v = [C.c_int32() for _ in range(6)]
            txt = C.c_char_p()
            _ck(self._lib.pf_stream_segment(self._h, i, *v, C.byref(txt)))
            out.append(Segment(*[x.value for x in v], Text=(txt.value or b"").decode("utf-8")))
        return out

    @property
    def SegmentSpeakers(self) -> List[int]:
        """The speaker label of every entry of Segments (OfflineRecognizer.SetSpeakerModel with SetVad; empty without it): 0, 1, ..
        in the order of each speaker's first window, -1 when the stream has no window at all."""
        n, v = C.c_int32(), C.c_int32()
        _ck(self._lib.pf_stream_num_segments(self._h, n))
        out = []
        for i in range(n.value):
            if self._lib.pf_stream_segment_speaker(self._h, i, v) != 0:      # no speaker model was on
                return []
            out.append(v.value)
        return out

    @property
    def SpeakerCentroids(self) -> np.ndarray:
        """[speakers, E] float32: each speaker's centroid, the L2-normalised mean of its windows' L2-normalised embeddings (for
        matching against enrolled voices); [0, 0] without speaker labels."""
        k, e = C.c_int32(), C.c_int32()
        _ck(self._lib.pf_stream_num_speakers(self._h, k))
        _ck(self._lib.pf_stream_speaker_centroid(self._h, 0, None, 0, e))
        out = np.zeros((k.value, e.value), np.float32)
        for s in range(k.value):
            row = np.zeros(max(e.value, 1), np.float32)
            _ck(self._lib.pf_stream_speaker_centroid(self._h, s, row.ctypes.data_as(C.POINTER(C.c_float)), e.value, e))
            out[s] = row[: e.value]
        return out

    @property
    def SpeakerWindows(self) -> List[tuple]:
        """(begin ms, end ms, label) of every window that was embedded, in time order."""
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_spk_windows(self._h, n))
        out = []
        for i in range(n.value):
            v = [C.c_int32() for _ in range(3)]
            _ck(self._lib.pf_stream_spk_window(self._h, i, *v))
            out.append(tuple(x.value for x in v))
        return out

    def _punctuated(self):
        txt, ids, n = C.c_char_p(), C.POINTER(C.c_int32)(), C.c_int32()
        _ck(self._lib.pf_stream_punctuated(self._h, C.byref(txt), C.byref(ids), n))
        return (txt.value or b"").decode("utf-8"), [ids[i] for i in range(n.value)]

    @property
    def Punctuated(self) -> str:
        """The punctuated form of the last GetResults' Text (OfflineRecognizer.SetPuncModel; "" without it)."""
        return self._punctuated()[0]

    @property
    def PuncIds(self) -> List[int]:
        """The mark of every word of that text, as an index into the model's punc_list."""
        return self._punctuated()[1]

    @property
    def Sentences(self) -> List["Sentence"]:
        """The sentences of the punctuated text; with times when the result has one Timestamps entry per word."""
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_sentences(self._h, n))
        out = []
        for i in range(n.value):
            v = [C.c_int32() for _ in range(5)]
            txt = C.c_char_p()
            _ck(self._lib.pf_stream_sentence(self._h, i, *v, C.byref(txt)))
            wb, we, ht, b, e = (x.value for x in v)
            out.append(Sentence(WordBegin=wb, WordEnd=we, Times=[b, e] if ht else [], Text=(txt.value or b"").decode("utf-8")))
        return out

    def SetAlignIds(self, ids: Optional[List[int]]) -> None:
        """The stream's target for forced alignment (OfflineRecognizer.SetAlign): token IDS — text to ids needs the model's
        tokenizer and is the caller's.  Kept until cleared with None."""
        if ids is None:
            _ck(self._lib.pf_stream_set_align_ids(self._h, None, -1))
            return
        a = (C.c_int64 * max(len(ids), 1))(*[int(v) for v in ids])
        _ck(self._lib.pf_stream_set_align_ids(self._h, a, len(ids)))

    @property
    def Alignment(self) -> Optional["Alignment"]:
        """The alignment of the target of the last GetResults (None when nothing was aligned for this stream)."""
        pt, ps = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
        n, ok, path, ll = C.c_int32(), C.c_int32(), C.c_float(), C.c_double()
        _ck(self._lib.pf_stream_alignment(self._h, C.byref(pt), C.byref(ps), n, path, C.byref(ll), ok))
        if n.value < 0:
            return None
        k = n.value if ok.value else 0
        return Alignment(Ok=ok.value, PathScore=path.value, LogLik=ll.value,
                         Timestamps=[[pt[2 * j], pt[2 * j + 1]] for j in range(k)], Scores=[ps[j] for j in range(k)])

    @property
    def Timestamps(self) -> List[List[int]]:
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_timestamps(self._h, n))
        out = []
        for j in range(n.value):
            p = C.POINTER(C.c_int32)()
            k = C.c_int32()
            _ck(self._lib.pf_stream_timestamp(self._h, j, C.byref(p), k))
            out.append([p[m] for m in range(k.value)])
        return out

    @Timestamps.setter
    def Timestamps(self, value: List[List[int]]) -> None:
        flat = [v for t in value for v in t]
        ints = (C.c_int32 * max(len(flat), 1))(*flat)
        lens = (C.c_int32 * max(len(value), 1))(*[len(t) for t in value])
        _ck(self._lib.pf_stream_set_timestamps(self._h, ints, lens, len(value)))

    @property
    def OfflineInputEntity(self) -> OfflineInputEntity:
        n = C.c_int32()
        rc = self._lib.pf_stream_get_speech(self._h, None, 0, n)
        speech = None
        if rc == N.PF_ERR_CAPACITY:
            speech = np.empty(n.value, np.float32)
            _ck(self._lib.pf_stream_get_speech(self._h, speech.ctypes.data_as(C.POINTER(C.c_float)), speech.size, n))
        else:
            _ck(rc)
            speech = None if n.value < 0 else np.empty(0, np.float32)
        return OfflineInputEntity(Speech=speech, SpeechLength=self.SpeechLength, Hotwords=self.Hotwords)

    @OfflineInputEntity.setter
    def OfflineInputEntity(self, value: OfflineInputEntity) -> None:
        if value is None or value.Speech is None:
            _ck(self._lib.pf_stream_set_speech(self._h, None, -1, 0 if value is None else value.SpeechLength))
        else:
            x = np.ascontiguousarray(value.Speech, dtype=np.float32)
            _ck(self._lib.pf_stream_set_speech(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, value.SpeechLength))
        self.Hotwords = None if value is None else value.Hotwords

    def GetDecodeChunk(self) -> OfflineInputEntity:        # OfflineStream.cs:58-68
        return self.OfflineInputEntity

    def RemoveChunk(self) -> None:                         # OfflineStream.cs:69-79
        if len(self.Tokens) > 2:
            _ck(self._lib.pf_stream_set_speech(self._h, None, -1, 0))

    @property
    def SpeechLength(self) -> int:
        n = C.c_int32()
        _ck(self._lib.pf_stream_num_feature_floats(self._h, n))
        return n.value

    def Dispose(self) -> None:
        # the native handle stays valid: later calls raise the reference's ObjectDisposedException
        # (PF_ERR_DISPOSED "OfflineStream"), not a null-handle error
        if self._h:
            self._lib.pf_stream_dispose(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None) and getattr(self, "_borrowed", None) is None:
                self._lib.pf_stream_free(self._h)
                self._h = None
        except Exception:
            pass


class OfflineRecognizer:
    def __init__(self, modelFilePath: str, configFilePath: str, mvnFilePath: str, tokensFilePath: str,
                 modelebFilePath: str = "", hotwordFilePath: str = "", batchSize: int = 1, threadsNum: int = 1,
                 device: int = 0):
        self._lib = N.load()
        h = C.c_void_p()
        enc = lambda s: (s or "").encode("utf-8")
        _ck(self._lib.pf_recognizer_create(enc(modelFilePath), enc(configFilePath), enc(mvnFilePath),
                                           enc(tokensFilePath), enc(modelebFilePath), enc(hotwordFilePath),
                                           batchSize, threadsNum, device, C.byref(h)))
        self._h = h

    def CreateOfflineStream(self) -> OfflineStream:
        s = C.c_void_p()
        _ck(self._lib.pf_recognizer_create_stream(self._h, C.byref(s)))
        return OfflineStream(_lib=self._lib, _handle=s, _recognizer=self)

    def SetDecode(self, ctc: bool = False, scores: bool = False) -> None:
        """Decoding beyond the reference's, for every GetResults that follows (off by default).  ctc (SenseVoice): the
        streams' Tokens are the CTC-collapsed ids (repeats merged, blanks dropped, nothing read past the utterance's own
        frames), Timestamps one [begin, end] pair in milliseconds per token, Scores the token confidences (log-probs).
        scores alone: Scores is the log-prob of every position of Tokens; Tokens / Timestamps stay as they are."""
        flags = (N.PF_DECODE_CTC if ctc else 0) | (N.PF_DECODE_SCORES if scores else 0)
        _ck(self._lib.pf_recognizer_set_decode(self._h, flags))

    def SetNBest(self, N: int, K: int = 4) -> None:
        """Alternatives for every GetResults that follows (off by default; N = 0 turns them off again).  Each stream then
        carries TokenAlternatives, the K (1 .. 8) best (id, log-prob) pairs per token, and — paraformer models, N > 1 —
        Alternatives, the exact N-best (<= 64) hypotheses with their scores.  Tokens, Timestamps, Scores and the result
        text stay as they are."""
        _ck(self._lib.pf_recognizer_set_nbest(self._h, int(N), int(K)))

    def SetCtcBeam(self, N: int, W: int = 0, K: int = 4) -> None:
        """SenseVoice models: a CTC prefix beam search on the device for every GetResults that follows (off by default;
        N = 0 turns it off again).  Each stream's Alternatives then holds up to N (<= 64) labelings by descending Score —
        the float64 log of the summed alignments the search kept — found with beam width W (0 = max(16, N)) over the K
        (1 .. 8) best ids per frame.  Tokens, Timestamps, Scores and the result text stay as they are; entry 0 is the
        search's best, which need not be the result."""
        _ck(self._lib.pf_recognizer_set_ctc_beam(self._h, int(N), int(W), int(K)))

    def SetHotwordBoost(self, s: float) -> None:
        """SenseVoice models: hot-word boosting inside the beam search of SetCtcBeam (inert without it; 0 turns it off).  A
        labeling earns s per token while it spells a hot word, keeps it when the word completes and loses it when the match
        breaks.  The hot words of a GetResults call are the union of its streams' Hotwords (token ids), else the recognizer's
        hot-word file, tokenised per character as the reference does — set stream.Hotwords ids where sentencepiece pieces are
        needed.  Alternatives then come in the biased order, each with Score, HotwordTokens and LogLikSum; Text and Tokens stay
        as they are."""
        _ck(self._lib.pf_recognizer_set_hotword_boost(self._h, float(s)))

    def SetLm(self, arpaPath, alpha: float = 0.5, beta: float = 0.0, flags: int = 0) -> None:
        """SenseVoice models: an ARPA n-gram language model fused into the beam search of SetCtcBeam (inert without it; None
        or "" clears it) with weight alpha >= 0, per-token bonus beta and flags (_native.PF_LM_EOS: add the end-of-sentence
        step).  The file is read once against the token table; each engine of the pool uploads it on first use.
        Alternatives then come in the fused order, each with Score, LmSum and LogLikSum; Text and Tokens stay as they are."""
        path = None if not arpaPath else str(arpaPath).encode("utf-8")
        _ck(self._lib.pf_recognizer_set_lm(self._h, path, float(alpha), float(beta), int(flags)))

    def SetNBestSearch(self, W: int) -> None:
        """Paraformer models: the n-best list of SetNBest(N > 1, K) from a beam search of width max(W, N) over the per-token
        alternatives on the device (inert until SetNBest; 0 turns it off, which any model accepts).  On its own it lists what
        SetNBest lists; its purpose is SetNBestLm and SetNBestHotwordBoost, whose scores decide which prefixes survive a
        position.  Alternatives then come in the fused order, each with Score, LogLikSum, LmSum and HotwordTokens:
        Score == (LogLikSum + boost * HotwordTokens) + LmSum.  Text, Tokens, Timestamps, Scores and TokenAlternatives stay."""
        _ck(self._lib.pf_recognizer_set_nbest_search(self._h, int(W)))

    def SetNBestLm(self, arpaPath, alpha: float = 0.5, beta: float = 0.0, flags: int = 0) -> None:
        """Paraformer models: an ARPA n-gram language model fused into the search of SetNBestSearch (inert without it; None or
        "" clears it) with weight alpha >= 0, per-token bonus beta and flags.  A paraformer emits its own </s> as the last
        token, which the model already scores as the end of the sentence: leave _native.PF_LM_EOS clear."""
        path = None if not arpaPath else str(arpaPath).encode("utf-8")
        _ck(self._lib.pf_recognizer_set_nbest_lm(self._h, path, float(alpha), float(beta), int(flags)))

    def SetNBestHotwordBoost(self, s: float) -> None:
        """Paraformer models: hot-word boosting inside the search of SetNBestSearch (inert without it; 0 turns it off): s per
        token while a hypothesis spells a hot word, kept when the word completes.  The hot words are read where
        SetHotwordBoost reads them: the streams' Hotwords (token ids), else the recognizer's hot-word file."""
        _ck(self._lib.pf_recognizer_set_nbest_hotword_boost(self._h, float(s)))

    def SetAlign(self, on: bool = True) -> None:
        """SenseVoice models: CTC forced alignment on the device for every GetResults that follows (off by default).  A
        stream with a target (OfflineStream.SetAlignIds) gets OfflineStream.Alignment — where each id of the known text lies
        in the audio, and log P(text | audio); with SetCtcBeam every Alternative gets Timestamps of its own and LogLik.
        Tokens, Timestamps, Scores, the result text and the alternatives' order and scores stay as they are."""
        _ck(self._lib.pf_recognizer_set_align(self._h, 1 if on else 0))

    def SetVad(self, cfg=True, batch_max: int = 0, frame_budget: int = 0, sep: str = "") -> None:
        """Long-audio recognition for every GetResults that follows (off by default; SetVad(None) turns it off again): each
        stream is cut into speech segments on the device, the segments of the call are batched by length, forwarded where
        they lie and stitched into one result per stream — Text joined by sep, Tokens / Scores concatenated, Timestamps on
        the stream's clock; stream.Segments lists the pieces.  cfg: True (the stated defaults, which nobody has validated
        on real speech), a dict of pf_vad_config fields, or a PfVadConfig.  batch_max / frame_budget: 0 = 32 rows /
        96000 frames per batch.  Not available beside SetNBest, SetCtcBeam or SetAlign."""
        if cfg is None or cfg is False:
            _ck(self._lib.pf_recognizer_set_vad(self._h, None, 0, 0, None))
            return
        from .engine import vad_config
        c = cfg if isinstance(cfg, N.PfVadConfig) else vad_config(**({} if cfg is True else cfg))
        _ck(self._lib.pf_recognizer_set_vad(self._h, C.byref(c), int(batch_max), int(frame_budget), sep.encode("utf-8")))

    def SetPuncModel(self, pfwPath) -> None:
        """Punctuation for every GetResults that follows: a `.pfw` of kind "cttransformer", loaded once and attached to every
        engine of the pool; None clears.  Each stream's final Text (with SetVad: the stitched text) is punctuated on the device,
        all streams of a call in one batch: stream.Punctuated, .PuncIds, .Sentences.  Text, Tokens and Timestamps of the result
        stay what they are.  No real model file has been through this path: the rules and dimensions are stated, not validated."""
        _ck(self._lib.pf_recognizer_set_punc_model(self._h, None if pfwPath is None else str(pfwPath).encode("utf-8")))

    def SetSpeakerModel(self, pfwPath, cfg=None) -> None:
        """Speaker labels for every long-audio GetResults that follows: a `.pfw` of kind "campplus" (python -m
        aliparaformerasr_amd.convert ... --kind campplus), loaded once and attached to every engine of the pool, present and
        future; None clears.  cfg: None (the defaults), an engine.spk_config(...) or a dict of its fields.  Inert until SetVad,
        and may be set before or after it.  stream.SegmentSpeakers, .SpeakerCentroids, .SpeakerWindows; everything else of the
        result stays what it is.  No real model file has been through this path: the network, the windows and the thresholds are
        stated, not validated."""
        from .engine import _spk_cfg_ptr
        _ck(self._lib.pf_recognizer_set_spk_model(self._h, None if pfwPath is None else str(pfwPath).encode("utf-8"), _spk_cfg_ptr(cfg)))

    def SetVadModel(self, pfwPath) -> None:
        """The FSMN-VAD model score for SetVad's segmentation: a `.pfw` of kind "fsmnvad" (python -m aliparaformerasr_amd.convert
        ... --kind fsmnvad), loaded once and attached to every engine of the pool, present and future; None clears.  Inert
        until SetVad, and may be set before or after it; pass engine.vad_model_config() to SetVad for the thresholds that go
        with it (stated, not tuned: nobody has validated them on real speech)."""
        _ck(self._lib.pf_recognizer_set_vad_model(self._h, None if pfwPath is None else str(pfwPath).encode("utf-8")))

    def GetResult(self, stream: OfflineStream) -> OfflineRecognizerResultEntity:
        return self.GetResults([stream])[0]

    def GetResults(self, streams: List[OfflineStream]) -> List[OfflineRecognizerResultEntity]:
        n = len(streams)
        arr = (C.c_void_p * max(n, 1))(*[s._h for s in streams])
        _ck(self._lib.pf_recognizer_get_results(self._h, arr, n))
        out = []
        for i in range(n):
            txt = C.c_char_p()
            tl = C.c_int32()
            _ck(self._lib.pf_result_text(self._h, i, C.byref(txt), tl))
            r = OfflineRecognizerResultEntity(Text=(txt.value or b"").decode("utf-8"), TextLen=tl.value)
            nt = C.c_int32()
            _ck(self._lib.pf_result_num_tokens(self._h, i, nt))
            for j in range(nt.value):
                t = C.c_char_p()
                _ck(self._lib.pf_result_token(self._h, i, j, C.byref(t)))
                r.Tokens.append((t.value or b"").decode("utf-8"))
            nts = C.c_int32()
            _ck(self._lib.pf_result_num_timestamps(self._h, i, nts))
            for j in range(nts.value):
                p = C.POINTER(C.c_int32)()
                k = C.c_int32()
                _ck(self._lib.pf_result_timestamp(self._h, i, j, C.byref(p), k))
                r.Timestamps.append([p[m] for m in range(k.value)])
            out.append(r)
        return out

    def DisposeOfflineStream(self, offlineStream: Optional[OfflineStream]) -> None:
        if offlineStream is not None:
            offlineStream.Dispose()

    def Dispose(self) -> None:
        if self._h:
            self._lib.pf_recognizer_dispose(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pf_recognizer_free(self._h)
                self._h = None
        except Exception:
            pass
