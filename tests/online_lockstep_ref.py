"""The streaming glue with the device in the loop: what OnlineRecognizer / OnlineStream (csrc/online.cpp) must compute, id for id.

LockstepRecognizer / LockstepStream subclass oracle.online.OnlineRecognizer / OnlineStream and keep the oracle's glue as it is:
chunks of 9600 samples behind a chunk of silence, the first frame repeated, the one-frame LFR splice, the ten-frame feature cache,
the sentinel for every exact 0, stack_states' layer-0 quirk, dynamic_mask, CIF with its carry, stream 0's len_time for every
stream, all L ids appended to every stream of the work set.  With an `engine` they take from the library under test every piece
the glue does not own, so that each float is bit for bit what online.cpp sees:
  fbank               Engine.fbank (pf_fbank: Engine::fbank_host, the call OnlineStreamM::InputSpeech makes)
  position encoding   pf_host_online_posenc (numpy's sin / cos differ from libm's by up to 2e-6: tests/test_online_cpu.py)
  the two graphs      Engine.online_encoder and Engine.online_decoder(..., want_logits=False) of an engine of its own, built
                      from the same files as the recognizer; the ids are the device's
CMVN and the sqrt(512) scale stay in numpy (single float32 / double operations; tests/test_online_lockstep_cpu.py holds them to a
scalar loop).  Without an engine the same object runs on the oracle alone: numpy fbank, numpy position encoding, the oracle's
graphs and argmax.

Each borrowed piece is held to a reference of its own elsewhere: the fbank conformance suite, tests/test_online_cpu.py, the seam
tests of tests/test_gpu_online.py.  What this object DEFINES is the ASSEMBLY: which stream's state goes into which row of which
call, and what comes back to whom.  An exact comparison of ids against it is therefore not circular: a recognizer that hands
stream b the caches of stream b', drops a carry or forgets a splice frame feeds the same kernels other numbers and gets other ids
(tests/test_online_lockstep_cpu.py shows that for the ten wrong assemblies of MUTATIONS, on the oracle alone).

Beyond the oracle the stream has input_finished() (OnlineStreamM::InputFinished: everything cached goes out in chunks, the last
zero-padded to 9600 samples, the first chunk ever being the constructor's silence) and reset() (OnlineStreamM::ResetDecoder).
`endpoint=` (a tests/endpoint_ref.py config) is for runs WITHOUT a device only: it closes sentences by the definition of
endpoint_ref on the levels of the caller's rows, as OnlineRecognizerM::ForwardEndpoint does, so that the CPU proof can reset where
the library would; on the device the test resets where the library's Sentences grow.

`mutate=` plants ONE wrong assembly (keys of MUTATIONS); the places are marked `# mutation`.

SCHEDULES are the event lists both new test files play: ("new", u) ("add", u, samples) ("fin", u) ("get", (u, ...)) and
("drain", (u, ...), n): GetResults until no stream's tokens change, which must take n calls.
"""
import ctypes as C
import math

import numpy as np

from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import model as om
from oracle import online as oo

F32 = np.float32
CHUNK = 160 * oo.CHUNK_FRAMES                                         # 9600 samples
VOCAB = 300

MUTATIONS = {
    "a": "FSMN caches taken from the neighbouring stream of the work set",
    "b": "layer l's cache built from the stream's layer-l state instead of layer 0",
    "c": "the CIF carry (alpha and hidden) not kept between calls",
    "d": "start_idx not advanced",
    "e": "the LFR splice frame not kept (first frame repeated every chunk)",
    "f": "the feature cache not carried (zeros every chunk)",
    "g": "results written back by position in `streams` instead of by position in the work set",
    "h": "only lens[b] ids appended instead of all L",
    "i": "the sentinel substitution skipped",
    "j": "input_finished dropping the zero-padded tail chunk",
}


def tokens():
    """the token table of tests/test_gpu_online.py"""
    toks = ["<blank>", "<s>", "</s>", "<unk>"]
    cjk = [chr(0x4E00 + 37 * i) for i in range(120)]
    bpe = []
    for i in range(VOCAB - 4 - len(cjk)):
        w = "w%d" % i
        bpe.append(w + "@@" if i % 3 == 0 else ("▁" + w if i % 3 == 1 else w))
    return toks + cjk + bpe


DENSE, SPARSE = 0.8, -1.5                                            # predictor.out.bias: tokens per chunk (below)


def model(bias=DENSE):
    """DENSE: the model of tests/test_gpu_online.py (3 + 3 layers, vocab 300, seed 31, predictor.out.bias = 0.8: 6 to 8 tokens per
    chunk of audio, 4 for a chunk of silence, never none).  SPARSE: the same weights with the bias at -1.5: 1 to 3 tokens per chunk
    of audio and NONE for a chunk of silence, so a stream that starts or ends beside running ones sits in the decoder's batch with
    no token."""
    cfg = W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=VOCAB)
    w = W.synth_weights(cfg, seed=31)
    w["predictor.out.bias"] = np.asarray([bias], F32)
    return cfg, w


def zero_cmvn(silence_row, posenc):
    """An am.mvn under which the sentinel matters.  The only exact zeros of an ordinary stream are the ten rows of a fresh feature
    cache, and a row that is one constant leaves the encoder's first LayerNorm as its beta whatever the constant: 0 or the sentinel
    give the same bytes (measured on the oracle: 0.0 apart).  Here column k is shifted and scaled so that the constructor's chunk
    of silence (fbank row `silence_row`, every frame) lands exactly on minus the position encoding of row k % 5 of the decode
    window, wherever a float32 scale does that (about three columns in four): the first chunk of every stream then holds exact
    zeros inside ordinary rows, some eighty per row.  `posenc(x, start_idx)` is the position encoding in use (numpy's or libm's).
    Returns (shift, scale), the planted (row, column) pairs."""
    shift, scale = (np.array(v, F32) for v in W.synth_cmvn())
    pe = posenc(np.zeros((10, 560), F32), 0)
    root = math.pow(512, 0.5)
    planted = []
    for k in range(560):
        t = k % 5                                                     # chunk rows 10 .. 14: inside dynamic_mask's window
        c, tgt = F32(silence_row[k % 80]), F32(-pe[t, k])
        sh = F32(F32(1.0) - c)
        r = F32(c + sh)                                               # 1, or one ulp beside it
        s0 = F32(float(tgt) / root / float(r))
        for s in (s0, np.nextafter(s0, F32(10)), np.nextafter(s0, F32(-10))):
            if F32(float(F32(r * s)) * root) == tgt:                  # ApplyCmvn, the scale: then + pe gives +0
                shift[k], scale[k] = sh, s
                planted.append((t, k))
                break
    assert len(planted) >= 300
    return (shift, scale), planted


def cmvn_scale(x, shift, scale):
    """ApplyCmvn and the sqrt(512) scale as OnlineStream.get_decode_chunk has them"""
    x = fe.apply_cmvn(x, shift, scale)
    return (x.astype(np.float64) * math.pow(512, 0.5)).astype(F32)


def reset(o, nd=None):
    """OnlineStreamM::ResetDecoder on an oracle stream (oracle/online.py OnlineStream.__init__): what a closed sentence resets.
    The token list starts EMPTY, not with the two zeros of a new stream; the splice frame and the queued speech stay."""
    o.tokens = []
    o.states = [np.zeros((512, 10), F32) for _ in range(len(o.states) if nd is None else nd)]
    o.cif_hidden = [np.zeros(512, F32)]
    o.cif_alpha = [F32(0.0)]
    o.cache_feats = np.zeros((10, 560), F32)
    o.start_idx = 0


class LockstepStream(oo.OnlineStream):
    def __init__(self, rec):
        super().__init__(rec)
        self.chunks_in = 0
        self.finished = False
        self.ep_rows, self.ep_state, self.ep_flushed, self.sentences = [], None, False, []   # runs without a device only

    def _input_speech(self, samples, n_caller=None):
        if n_caller is None:                                          # from add_samples: the first chunk ever is the silence
            n_caller = 0 if self.chunks_in == 0 else len(samples)
        self.chunks_in += 1
        before = self.speech.shape[0]
        super()._input_speech(samples)
        if n_caller > 0 and self.rec.endpoint is not None:            # the detector's share: the caller's rows (never the first
            rows = min((n_caller + 159) // 160, self.speech.shape[0] - before)   # chunk, so no repeated frame is among them)
            self.ep_rows.append(self.speech[before: before + rows])

    def input_finished(self):
        """OnlineStreamM::InputFinished"""
        self.finished = True
        while len(self.cache_samples):
            take, self.cache_samples = self.cache_samples[:CHUNK], self.cache_samples[CHUNK:]
            n_caller = 0 if self.chunks_in == 0 else len(take)
            if self.rec.mutate == "j" and len(take) < CHUNK:          # mutation
                self.chunks_in += 1
                continue
            s = np.zeros(CHUNK, F32)
            s[: len(take)] = take
            self._input_speech(s, n_caller)

    def reset(self):
        reset(self)

    def get_decode_chunk(self):
        """oracle.online.OnlineStream.get_decode_chunk with the position encoding taken from the recognizer (unmutated and
        without an engine: that function bit for bit, asserted in tests/test_online_lockstep_cpu.py)"""
        m = self.rec.mutate
        if oo.CHUNK_FRAMES > self.speech.shape[0]:
            return None
        head = self.splice if self.splice is not None else self.speech[:1]
        pad = np.concatenate([head, self.speech[: oo.CHUNK_FRAMES]])
        if m != "e":                                                  # mutation
            self.splice = pad[-1:].copy()
        x = oo.apply_lfr(pad)
        x = cmvn_scale(x, self.rec.shift, self.rec.scale)
        x = self.rec.position_encode(x, self.start_idx)
        chunk = np.concatenate([self.cache_feats, x])
        if m != "d":                                                  # mutation
            self.start_idx += x.shape[0]
        if m != "f":                                                  # mutation
            self.cache_feats = chunk[-10:].copy()
        self.speech = self.speech[oo.CHUNK_FRAMES:]
        return chunk


class LockstepRecognizer(oo.OnlineRecognizer):
    def __init__(self, cfg, weights, cmvn, toks, engine=None, quant="fp32", mutate=None, endpoint=None, fbank_cache=None):
        assert mutate is None or mutate in MUTATIONS
        assert engine is None or endpoint is None
        super().__init__(cfg, weights, cmvn, toks, quant=quant)
        self.engine, self.mutate, self.endpoint = engine, mutate, endpoint
        self.nd = cfg["dec_layers"]
        self.fbank_cache = fbank_cache                                # a dict shared between runs on the same audio, or None
        self.calls = []                                               # per get_results: (work set size, L, lens)

    # ---- the pieces the glue does not own
    def fbank(self, samples):
        if self.engine is not None:
            return self.engine.fbank(samples)
        if self.fbank_cache is None:
            return super().fbank(samples)
        key = np.asarray(samples, F32).tobytes()
        if key not in self.fbank_cache:
            self.fbank_cache[key] = super().fbank(samples)
        return self.fbank_cache[key]

    def position_encode(self, x, start_idx):
        if self.engine is None:
            return oo.position_encode(x, start_idx)
        from aliparaformerasr_amd import _native as N
        out = np.ascontiguousarray(x, dtype=F32).copy()
        N.check(N.load().pf_host_online_posenc(out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0], out.shape[1], start_idx))
        return out

    def encoder(self, speech):
        return self.engine.online_encoder(speech) if self.engine is not None else self.graphs.encoder(speech)

    def decoder(self, enc, emb, lens, cin):
        if self.engine is not None:
            _, ids, cout = self.engine.online_decoder(enc, emb, lens, cin, want_logits=False)
            return ids, cout
        logits, cout = self.graphs.decoder(enc, emb, lens, cin)
        return om.argmax_last(logits), cout

    # ---- the assembly
    def create_stream(self):
        return LockstepStream(self)

    def get_results(self, streams):
        """oracle.online.OnlineRecognizer.get_results (OnlineRecognizerM::Forward), then the sentences with endpoint="""
        m = self.mutate
        work, chunks = [], []
        for s in streams:
            c = s.get_decode_chunk()
            if c is not None:
                work.append(s)
                chunks.append(c)
        call = (len(work), 0, ())
        if work:
            B, nd = len(work), self.nd
            speech = np.stack(chunks).astype(F32)
            if m != "i":                                              # mutation
                speech = np.where(speech == 0, oo.SENTINEL, speech).astype(F32)
            src = work[1:] + work[:1] if m == "a" else work          # mutation
            cin = [np.stack([s.states[l if m == "b" else 0] for s in src]) for l in range(nd)]   # the layer-0 quirk; mutation
            enc, alphas = self.encoder(speech)
            fired = []
            for b, s in enumerate(work):
                s.cif_hidden += [enc[b, t] for t in range(enc.shape[1])]
                s.cif_alpha += list(oo.dynamic_mask(alphas[b]))
            len_time = len(work[0].cif_alpha)
            for s in work:
                f, ca, ch = oo.cif(np.stack(s.cif_hidden[:len_time]), np.asarray(s.cif_alpha[:len_time], F32),
                                   self.graphs.o.cfg.cif_threshold)
                s.cif_alpha, s.cif_hidden = [ca], [ch]
                if m == "c":                                          # mutation
                    s.cif_alpha, s.cif_hidden = [F32(0.0)], [np.zeros(512, F32)]
                fired.append(f)
            L = max(f.shape[0] for f in fired)
            call = (B, L, tuple(f.shape[0] for f in fired))
            if L > 0:
                emb = np.zeros((B, L, 512), F32)
                lens = np.zeros(B, np.int32)
                for b, f in enumerate(fired):
                    emb[b, : f.shape[0]] = f
                    lens[b] = f.shape[0]
                ids, cout = self.decoder(enc, emb, lens, cin)
                dst = list(streams)[:B] if m == "g" else work        # mutation
                for b, s in enumerate(dst):
                    n = int(lens[b]) if m == "h" else L               # mutation
                    s.tokens += [int(v) for v in ids[b][:n]]
                    s.states = [cout[l][b].copy() for l in range(nd)]
        self.calls.append(call)
        if self.endpoint is not None:
            self._close_sentences(streams)
        return [oo.decode_text(self.tokens, s.tokens) for s in streams]

    def _close_sentences(self, streams):
        """OnlineRecognizerM::ForwardEndpoint without the device: the definition on the caller's rows, and the flush once a
        finished stream has nothing left to decode"""
        import endpoint_ref as R
        import vad_ref as V
        for s in streams:
            flush = (s.finished and len(s.cache_samples) == 0 and s.speech.shape[0] < oo.CHUNK_FRAMES and s.ep_state is not None)
            if s.ep_flushed or (not s.ep_rows and not flush):
                continue
            if s.ep_state is None:
                s.ep_state = R.new_state()
            lev = V.levels(np.concatenate(s.ep_rows)) if s.ep_rows else np.zeros(0, np.int32)
            events, _, _ = R.update(s.ep_state, lev, flush, 80, self.endpoint)
            s.ep_rows, s.ep_flushed = [], flush
            for _ in events:
                s.sentences.append(oo.decode_text(self.tokens, s.tokens))   # first_pass: after this chunk's ids
                s.reset()


# ------------------------------------------------------------------------------------------------ schedules
SECONDS = 3
N = 16000 * SECONDS
RAGGED = ((1, 9599, 9601, 160, 16000, 123, 9600, 2916),               # every row sums to 48000; a stream releases ONE chunk per
          (16000, 123, 1, 9599, 9601, 160, 12516),                    # AddSamples and only above 9600 cached samples, so the three
          (160, 9601, 123, 16000, 9599, 1, 9600, 2916))               # release at different calls
ENDPOINT_BURSTS = (((30, 100), (160, 230)), ((20, 90), (150, 225)), ((40, 110), (175, 240)))
ENDPOINT_KEYS = dict(end_silence=40)                                  # as test_reset_in_lockstep_with_the_oracle


class Schedule:
    def __init__(self, name, events, endpoint=False):
        self.name, self.events, self.endpoint = name, events, endpoint
        self.n_streams = 1 + max(e[1] for e in events if e[0] == "new")


def _audio(u):
    """W.synth_audio under an envelope that changes every 10 ms frame (a gain of 1 to 0.01, drawn per frame).  The plain signal is
    stationary: the frame before a chunk and the chunk's first frame are then nearly the same row, and losing the LFR splice frame
    (mutation e) moved no id in any schedule."""
    a = W.synth_audio(N, 60 + u)
    g = (10.0 ** (-2.0 * np.random.default_rng(900 + u).random(N // 160))).astype(F32)
    return (a * np.repeat(g, 160)).astype(F32)


def _pieces(step=4000):
    """today's schedule: three streams, 4000-sample pieces, stream 2 stops at 1.5 s; yields (round, [(u, piece)])"""
    audio = [_audio(u) for u in range(3)]
    for k, off in enumerate(range(0, N, step)):
        yield k, [(u, audio[u][off: off + step]) for u in range(3) if u != 2 or off < N // 2]


def schedules():
    out = []
    # 1. today's
    ev = [("new", u) for u in range(3)]
    for k, adds in _pieces():
        ev += [("add", u, p) for u, p in adds] + [("get", (0, 1, 2))]
    out.append(Schedule("pieces", ev))
    # 2. ragged pieces
    audio = [_audio(u) for u in range(3)]
    ev = [("new", u) for u in range(3)]
    offs = [0, 0, 0]
    for k in range(max(len(r) for r in RAGGED)):
        for u in range(3):
            if k < len(RAGGED[u]):
                ev.append(("add", u, audio[u][offs[u]: offs[u] + RAGGED[u][k]]))
                offs[u] += RAGGED[u][k]
        ev.append(("get", (0, 1, 2)))
    assert offs == [N, N, N]
    out.append(Schedule("ragged", ev))
    # 3. the list rotated by one every call; call 5 passes a strict subset (stream 1 keeps its chunk for later)
    ev = [("new", u) for u in range(3)]
    for k, adds in _pieces():
        ev += [("add", u, p) for u, p in adds]
        order = tuple((k + i) % 3 for i in range(3))
        ev.append(("get", tuple(u for u in order if u != 1) if k == 5 else order))
    out.append(Schedule("rotated", ev))
    # 4. stream 2 is created after the others have decoded two chunks (the silence at call 0, the first real one at call 2)
    ev = [("new", 0), ("new", 1)]
    late = _audio(2)
    for k, adds in _pieces():
        if k == 4:
            ev.append(("new", 2))
        ev += [("add", u, p) for u, p in adds if u != 2]
        if k >= 4:
            ev.append(("add", 2, late[(k - 4) * 4000: (k - 3) * 4000]))
        ev.append(("get", (0, 1, 2) if k >= 4 else (0, 1)))
    out.append(Schedule("late", ev))
    # 5. InputFinished with 9600 (stream 0: never fed, the constructor's silence is the first chunk ever), 1 and then 0 (stream 1:
    # finished twice), 9600 + 37 (stream 2) and 9600 of the caller's (stream 3) cached samples.  The cache never holds 0 after an
    # AddSamples (it starts at 9600 and a chunk leaves only above 9600), so 0 is a second InputFinished.
    # Queued at the drain: stream 0 one chunk, stream 1 none (its padded tail went at the call before), stream 2 two, stream 3
    # one -> two calls that decode and one that changes nothing.
    a = [_audio(u) for u in range(4)]
    ev = [("new", u) for u in range(4)]
    ev += [("add", 1, a[1][:1]), ("add", 2, a[2][:16000]), ("add", 3, a[3][:9600]), ("get", (0, 1, 2, 3))]
    ev += [("add", 2, a[2][16000: 16000 + 3237]), ("get", (0, 1, 2, 3))]
    ev += [("fin", 1), ("get", (0, 1, 2, 3))]
    ev += [("fin", u) for u in range(4)] + [("drain", (0, 1, 2, 3), 3)]
    out.append(Schedule("finish", ev))
    # 6. the endpoint on: two bursts per stream in 3 s, 4000-sample pieces
    import vad_ref as V
    a = [V.burst_audio(SECONDS, list(b), 40 + i) for i, b in enumerate(ENDPOINT_BURSTS)]
    ev = [("new", u) for u in range(3)]
    for off in range(0, N, 4000):
        ev += [("add", u, a[u][off: off + 4000]) for u in range(3)] + [("get", (0, 1, 2))]
    # the fifth chunk of the caller's is still cached (a chunk leaves only above 9600): InputFinished sends it, the second
    # sentence closes on it, the call after changes nothing
    ev += [("fin", u) for u in range(3)] + [("drain", (0, 1, 2), 2)]
    out.append(Schedule("endpoint", ev, endpoint=True))
    return out


class Case:
    """a schedule on a model (DENSE / SPARSE) under the ordinary or the zero_cmvn am.mvn"""

    def __init__(self, schedule, bias=DENSE, zero_cmvn=False):
        self.schedule, self.bias, self.zero_cmvn = schedule, bias, zero_cmvn
        self.name = schedule.name + ("" if bias == DENSE else "/sparse") + ("/zero-cmvn" if zero_cmvn else "")
        self.drain_calls = None                                       # the schedule's own count


def cases():
    """every schedule on the model of tests/test_gpu_online.py; `late` and `finish` also on SPARSE (a stream with NO token beside
    streams with some: the late stream's and the never-fed stream's chunk of silence); `pieces` also under zero_cmvn"""
    s = schedules()
    by = {x.name: x for x in s}
    return [Case(x) for x in s] + [Case(by["late"], SPARSE), Case(by["finish"], SPARSE), Case(by["pieces"], zero_cmvn=True)]


class RefSide:
    """a LockstepRecognizer (or the plain oracle) behind the four verbs of a schedule"""

    def __init__(self, rec):
        self.rec = rec

    def new(self):
        return self.rec.create_stream()

    def add(self, s, x):
        s.add_samples(x)

    def fin(self, s):
        s.input_finished()

    def get(self, streams):
        return self.rec.get_results(streams)

    def tokens(self, s):
        return list(s.tokens)


def play(schedule, sides, check=None, drain_calls=None):
    """Plays the events on every side; after every GetResults check(call, order, streams, results) with streams[i][u] side i's
    stream u and results[i] what side i's call returned.  A drain is governed by side 0 and must take the event's number of calls, or
    `drain_calls` (-1: any number, for the mutated runs).  Returns the number of calls."""
    streams = [dict() for _ in sides]
    k = 0

    def get(order):
        nonlocal k
        res = [sd.get([st[u] for u in order]) for sd, st in zip(sides, streams)]
        if check is not None:
            check(k, order, streams, res)
        k += 1

    for e in schedule.events:
        if e[0] == "new":
            for sd, st in zip(sides, streams):
                st[e[1]] = sd.new()
        elif e[0] == "add":
            for sd, st in zip(sides, streams):
                sd.add(st[e[1]], e[2])
        elif e[0] == "fin":
            for sd, st in zip(sides, streams):
                sd.fin(st[e[1]])
        elif e[0] == "get":
            get(e[1])
        elif e[0] == "drain":
            n = 0
            while True:
                before = [sides[0].tokens(streams[0][u]) for u in e[1]]
                get(e[1])
                n += 1
                if before == [sides[0].tokens(streams[0][u]) for u in e[1]]:
                    break
                assert n < 16, "the drain does not end"
            want = e[2] if drain_calls is None else drain_calls
            assert want == -1 or n == want, (schedule.name, "drain calls", n, want)
    return k


def history(schedule, rec, drain_calls=None):
    """every stream's token list after every call of one side: [call][u] -> tuple of ids (None before the stream exists)"""
    out = []

    def check(k, order, streams, res):
        out.append(tuple(tuple(streams[0][u].tokens) if u in streams[0] else None for u in range(schedule.n_streams)))
    play(schedule, [RefSide(rec)], check, drain_calls)
    return out
