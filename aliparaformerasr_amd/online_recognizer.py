"""ctypes mirror of the reference's streaming API (AliParaformerAsr/OnlineRecognizer.cs, OnlineStream.cs) over
libparaformer_hip.so (include/paraformer_hip.h section 7)."""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _native as N
from .offline_recognizer import _ck


class OnlineRecognizerResultEntity:
    def __init__(self, text: str):
        self.Text = text


class OnlineSentence:
    """A sentence the endpoint detector has closed (OnlineRecognizer.SetEndpoint): [begin_ms, end_ms) in the caller's audio,
    kind ("silence", "forced" or "flush"), first_pass (the online model's text at the closing chunk), text (the second pass's
    text; first_pass without one) and result: the offline stream that produced it — Tokens, Timestamps (relative to begin_ms),
    Scores, alternatives, punctuation, whatever the offline recognizer has set — or None without a second pass."""
    KINDS = {N.PF_ENDPOINT_SILENCE: "silence", N.PF_ENDPOINT_FORCED: "forced", N.PF_ENDPOINT_FLUSH: "flush"}

    def __init__(self, begin_ms, end_ms, kind, first_pass, text, result, tokens=None, punctuated="", punc_ids=None):
        self.begin_ms, self.end_ms, self.kind, self.first_pass, self.text, self.result = begin_ms, end_ms, kind, first_pass, text, result
        # OnlineRecognizer.SetPuncModel: first_pass under the marks of its words (the flush's edit applied), and the marks
        self.punctuated, self.punc_ids = punctuated, [] if punc_ids is None else punc_ids
        self.tokens = [] if tokens is None else tokens   # the stream's TokenInfo as of the closing call (OnlineRecognizer.SetTokenInfo)

    def __repr__(self):
        return "OnlineSentence(%d, %d, %r, %r)" % (self.begin_ms, self.end_ms, self.kind, self.text)


class OnlineToken(tuple):
    """(id, time_ms, score, fired) of one position of OnlineStream.Tokens; .entry: the walked entry of [carry ; chunk] that
    completed the token (0: the carry, j: chunk position j - 1, -1: not fired); .score_bits: the score's float32 bits."""

    def __new__(cls, t):
        self = super().__new__(cls, (int(t.id), int(t.time_ms), float(t.score), bool(t.flags & N.PF_ONLINE_TOKEN_FIRED)))
        self.entry, self.flags = int(t.entry), int(t.flags)
        self.score_bits = int(np.float32(t.score).view(np.uint32))
        return self

    id = property(lambda self: self[0])
    time_ms = property(lambda self: self[1])
    score = property(lambda self: self[2])
    fired = property(lambda self: self[3])


def _tokens(p, n):
    return [OnlineToken(p[i]) for i in range(n)]


class OnlineStream:
    def __init__(self, lib, handle, recognizer):
        self._lib, self._h, self._recognizer = lib, handle, recognizer

    @property
    def TokenInfo(self) -> List[OnlineToken]:
        """With OnlineRecognizer.SetTokenInfo: (id, time_ms, score, fired) for Tokens[i], index for index; [] with the mode off.
        time_ms (-1 where fired is False) is the start of the 60 ms frame in which the integrator crossed the threshold, in the
        caller's audio: not a word boundary, and not validated on real speech.  score: the log-probability of the id."""
        p, n = C.POINTER(N.PfOnlineToken)(), C.c_int32()
        _ck(self._lib.pf_online_stream_token_info(self._h, C.byref(p), n))
        return _tokens(p, n.value)

    def InputFinished(self) -> None:
        """No more audio follows: the cached samples go through the front-end (the last ones zero-padded to one chunk, so the
        online model decodes the tail too) and the GetResults that has decoded the last chunk flushes the endpoint detector.
        A later AddSamples raises."""
        _ck(self._lib.pf_online_stream_input_finished(self._h))

    @property
    def Sentences(self) -> List[OnlineSentence]:
        """The sentences closed so far (empty without SetEndpoint), in time order."""
        from .offline_recognizer import OfflineStream
        n = C.c_int32()
        _ck(self._lib.pf_online_stream_num_sentences(self._h, n))
        out = []
        for j in range(n.value):
            b, e, k, fp, tx, h = C.c_int32(), C.c_int32(), C.c_int32(), C.c_char_p(), C.c_char_p(), C.c_void_p()
            _ck(self._lib.pf_online_stream_sentence(self._h, j, b, e, k, C.byref(fp), C.byref(tx)))
            _ck(self._lib.pf_online_stream_sentence_result(self._h, j, C.byref(h)))
            res = None
            if h.value:
                res = OfflineStream(_lib=self._lib, _handle=h, _recognizer=None)
                res._borrowed = self                     # the handle belongs to this stream: never freed by the view
            tp, tn = C.POINTER(N.PfOnlineToken)(), C.c_int32()
            _ck(self._lib.pf_online_stream_sentence_tokens(self._h, j, C.byref(tp), tn))
            pt, pi, pn = C.c_char_p(), C.POINTER(C.c_int32)(), C.c_int32()
            _ck(self._lib.pf_online_stream_sentence_punctuated(self._h, j, C.byref(pt), C.byref(pi), pn))
            out.append(OnlineSentence(b.value, e.value, OnlineSentence.KINDS.get(k.value, k.value), (fp.value or b"").decode("utf-8"),
                                      (tx.value or b"").decode("utf-8"), res, _tokens(tp, tn.value),
                                      (pt.value or b"").decode("utf-8"), [pi[i] for i in range(pn.value)]))
        return out

    def _punctuated(self):
        t, ids, fl, n = C.c_char_p(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int32()
        _ck(self._lib.pf_online_stream_punctuated(self._h, C.byref(t), C.byref(ids), C.byref(fl), n))
        return (t.value or b"").decode("utf-8"), [ids[i] for i in range(n.value)], [fl[i] for i in range(n.value)]

    @property
    def Punctuated(self) -> str:
        """With OnlineRecognizer.SetPuncModel: the open text of the last GetResults under the marks of its committed words; a
        word whose last piece ends in "@@" is held back and appended raw.  "" without a model."""
        return self._punctuated()[0]

    @property
    def PuncIds(self) -> List[int]:
        """The mark of every committed word of the open text, as an index into the model's punc_list; never revised."""
        return self._punctuated()[1]

    @property
    def PuncFlags(self) -> List[int]:
        """Per committed word: bit 0 the word ended a sentence (the context restarted behind it), bit 1 a forced restart."""
        return self._punctuated()[2]

    @property
    def InSpeech(self):
        """(a sentence is open, its begin in ms or -1) as of the last GetResults."""
        a, b = C.c_int32(), C.c_int32()
        _ck(self._lib.pf_online_stream_in_speech(self._h, a, b))
        return bool(a.value), b.value

    def AddSamples(self, samples) -> None:
        if samples is None:
            _ck(self._lib.pf_online_stream_add_samples(self._h, None, 0))
            return
        x = np.ascontiguousarray(samples, dtype=np.float32)
        _ck(self._lib.pf_online_stream_add_samples(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0]))

    @property
    def Tokens(self) -> List[int]:
        p, n = C.POINTER(C.c_int64)(), C.c_int32()
        _ck(self._lib.pf_online_stream_tokens(self._h, C.byref(p), n))
        return [p[i] for i in range(n.value)]

    def Dispose(self) -> None:
        if self._h:
            self._lib.pf_online_stream_dispose(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pf_online_stream_free(self._h)
                self._h = None
        except Exception:
            pass


class OnlineRecognizer:
    def __init__(self, encoderFilePath: str, decoderFilePath: str, configFilePath: str, mvnFilePath: str,
                 tokensFilePath: str, threadsNum: int = 1, device: int = 0):
        self._lib = N.load()
        h = C.c_void_p()
        enc = lambda s: (s or "").encode("utf-8")
        _ck(self._lib.pf_online_recognizer_create(enc(encoderFilePath), enc(decoderFilePath), enc(configFilePath),
                                                  enc(mvnFilePath), enc(tokensFilePath), threadsNum, device, C.byref(h)))
        self._h = h

    def CreateOnlineStream(self) -> OnlineStream:
        s = C.c_void_p()
        _ck(self._lib.pf_online_create_stream(self._h, C.byref(s)))
        return OnlineStream(self._lib, s, self)

    def SetTokenInfo(self, on=True) -> None:
        """Token times and scores (pf_online_recognizer_set_token_info; off by default): every chunk step then stays on the
        device from the encoder to the ids, the carried CIF runs as a kernel, and every stream fills TokenInfo (closed sentences:
        OnlineSentence.tokens).  Tokens and Text are what they are with the mode off.  Refused once a live stream of this
        recognizer has decoded a chunk."""
        _ck(self._lib.pf_online_recognizer_set_token_info(self._h, 1 if on else 0))

    def SetPuncModel(self, pfwPath, maxContext: int = 0) -> None:
        """Streaming punctuation (pf_online_recognizer_set_punc_model; off by default): a causal `.pfw` of kind "cttransformer"
        (convert --kind cttransformer --causal); None detaches and frees.  Every GetResults then marks the newly committed words
        of all its streams in one launch on the GPU: stream.Punctuated / PuncIds / PuncFlags, sentence.punctuated / punc_ids.
        Text and Tokens are what they are without it.  maxContext: the words a context holds before a forced restart (2 .. 256;
        0: 200).  Refused while a live stream holds punctuation state.  Not validated on a real model."""
        _ck(self._lib.pf_online_recognizer_set_punc_model(self._h, None if pfwPath is None else str(pfwPath).encode("utf-8"), int(maxContext)))

    def SetEndpointModel(self, pfwPath) -> None:
        """The FSMN-VAD model score as the endpoint detector's level (pf_online_recognizer_set_endpoint_model): a `.pfw` of kind
        "fsmnvad"; None goes back to the energy level.  Inert until SetEndpoint; pass engine.endpoint_model_config()'s thresholds
        there (stated, not tuned).  An event can fall one call later than with the energy level.  Refused once a live stream has
        fed the detector."""
        _ck(self._lib.pf_online_recognizer_set_endpoint_model(self._h, None if pfwPath is None else str(pfwPath).encode("utf-8")))

    def SetEndpoint(self, enabled=True, **keys) -> None:
        """Endpoint detection for every GetResults that follows (off by default; SetEndpoint(False) turns it off again and
        leaves every path as it is without it): a causal voice-activity detector on the device closes sentences —
        stream.Sentences, stream.InSpeech — and resets the stream's decoder context at each; GetResults keeps returning the text
        of the open sentence.  keys: pf_endpoint_config fields (rise, margin_q, abs_level, window, on_count, off_count, pad_begin,
        pad_end, end_silence, min_speech, max_len).  The defaults are stated, not tuned: nobody has measured them on real speech."""
        if enabled is None or enabled is False:
            _ck(self._lib.pf_online_recognizer_set_endpoint(self._h, None))
            return
        from .engine import endpoint_config
        c = enabled if isinstance(enabled, N.PfEndpointConfig) else endpoint_config(**keys)
        _ck(self._lib.pf_online_recognizer_set_endpoint(self._h, C.byref(c)))

    def SetSecondPass(self, offline) -> None:
        """The OfflineRecognizer that re-recognises every finished sentence (None: none): the sentences that close in one
        GetResults go through ONE GetResults of it, one plain stream each.  Refused for a recognizer with SetVad on."""
        _ck(self._lib.pf_online_recognizer_set_second_pass(self._h, None if offline is None else offline._h))
        self._second = offline                           # keeps it alive

    def GetResult(self, stream: OnlineStream) -> OnlineRecognizerResultEntity:
        return self.GetResults([stream])[0]

    def GetResults(self, streams: List[OnlineStream]) -> List[OnlineRecognizerResultEntity]:
        n = len(streams)
        arr = (C.c_void_p * max(n, 1))(*[s._h for s in streams])
        _ck(self._lib.pf_online_get_results(self._h, arr, n))
        out = []
        for i in range(n):
            t = C.c_char_p()
            _ck(self._lib.pf_online_result_text(self._h, i, C.byref(t)))
            out.append(OnlineRecognizerResultEntity((t.value or b"").decode("utf-8")))
        return out

    def engine_handle(self):
        return self._lib.pf_online_recognizer_engine(self._h)

    def Dispose(self) -> None:
        if self._h:
            self._lib.pf_online_recognizer_dispose(self._h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pf_online_recognizer_free(self._h)
                self._h = None
        except Exception:
            pass
