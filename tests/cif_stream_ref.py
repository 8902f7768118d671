"""The carried CIF of one streaming chunk step, and the time rule of the streaming token info, restated in numpy.

step() is what pf_host_online_cif_step and cif_stream_kernel (csrc/k_cif_stream.hip) must compute, bit for bit: DynamicMask
inside ([lo, hi) keeps its alphas), the walk of oracle.online.cif over [carry ; Tc frames] with the walked entry of every fire
kept, the new carry written back into the stream's state block.  The block (csrc/decode_blocks.h CifStreamBlock) is held as
float32 words: hidden [D] | the integrate, one equal copy per 256 channels, padded to four cells that nobody writes.

TimedStream / TimedRecognizer put the time rule of include/paraformer_hip.h ("Streaming token times and scores") on
tests/online_lockstep_ref.py: every fbank row carries the caller-sample index of its frame start (-1: none), copies carry what
they copy, an LFR frame takes its first row's index, a token fired at chunk position p takes the first position >= p of that chunk
that has an index (none: the caller samples that went through the front-end so far), a token fired on the carry takes position
hi - 1 of the chunk before.  TimedRecognizer keeps, beside every stream's tokens, `info`: (id, time_ms, entry, fired, score bits)
per position, from its own walk of the call's encoder output (held to the oracle's fire counts) and the log-probs of its decoder.
"""
import numpy as np

import online_lockstep_ref as LR
from oracle import online as oo

F32 = np.float32
GROUP = 256
LO, HI = 5, 15                                                        # DynamicMask: chunk_size 5, lfr 10


def groups(D):
    return (D + GROUP - 1) // GROUP


def state_words(D):
    return D + (groups(D) + 3) // 4 * 4


def state_bytes(D):
    return 4 * state_words(D)


def new_state(D):
    return np.zeros(state_words(D), F32)


def walk(hiddens, alphas, threshold):
    """oracle.online.cif with the walked entry of every fire: fired [n, D], entries [n], carry_alpha, carry_hidden"""
    th = F32(threshold)
    D = hiddens.shape[1]
    integrate = F32(0.0)
    frames = np.zeros(D, F32)
    fired, entries = [], []
    with np.errstate(all="ignore"):
        for j in range(len(alphas)):
            alpha = F32(alphas[j])
            h = hiddens[j].astype(F32)
            if F32(alpha + integrate) < th:
                integrate = F32(integrate + alpha)
                frames = (frames + (alpha * h).astype(F32)).astype(F32)
            else:
                frames = (frames + (F32(th - integrate) * h).astype(F32)).astype(F32)
                fired.append(frames)
                entries.append(j)
                integrate = F32(integrate + alpha)
                integrate = F32(integrate - th)
                frames = (integrate * h).astype(F32)
        carry_h = (frames / integrate).astype(F32) if integrate > 0 else frames
    return (np.stack(fired) if fired else np.zeros((0, D), F32)), entries, integrate, carry_h


def mask(alphas, lo=LO, hi=HI):
    a = np.array(alphas, F32, copy=True)
    a[:lo] = 0
    a[hi:] = 0
    return a


def step(state, hiddens, alphas, threshold, lo=LO, hi=HI, reset=False, cap=None):
    """One chunk step on `state` (updated in place).  Returns fired [cap, D] (zero rows behind the count), fire_entry [cap] (-1
    behind the count), count."""
    Tc, D = hiddens.shape
    cap = Tc + 1 if cap is None else cap
    assert cap >= Tc + 1 and D % 4 == 0 and state.shape == (state_words(D),)
    ch = np.zeros(D, F32) if reset else state[:D].copy()
    ca = F32(0.0) if reset else state[D]
    f, ent, ia, ih = walk(np.concatenate([ch[None], hiddens.astype(F32)]), np.concatenate([[ca], mask(alphas, lo, hi)]).astype(F32), threshold)
    state[:D] = ih
    state[D: D + groups(D)] = ia
    fired = np.zeros((cap, D), F32)
    fired[: len(ent)] = f
    entry = np.full(cap, -1, np.int32)
    entry[: len(ent)] = ent
    return fired, entry, len(ent)


# ------------------------------------------------------------------------------------------------ the time rule
def time_ms(index, fs=16000):
    return int(index) * 1000 // fs


class TimedStream(LR.LockstepStream):
    def __init__(self, rec):
        super().__init__(rec)
        self.speech_idx, self.splice_idx, self.cache_idx, self.chunk_idx = [], -1, [-1] * 10, []
        self.carry_idx, self.caller_samples = -1, 0
        self.info = [(0, -1, -1, False, None), (0, -1, -1, False, None)]     # the constructor's two zeros

    def _input_speech(self, samples, n_caller=None):
        if n_caller is None:
            n_caller = 0 if self.chunks_in == 0 else len(samples)
        before, dup = self.speech.shape[0], self.first_input
        super()._input_speech(samples, n_caller)
        added = self.speech.shape[0] - before
        first = self.caller_samples if n_caller > 0 else -1
        self.caller_samples += n_caller
        t80 = added - 1 if (dup and added > 0) else added
        rows = [first + 160 * r if first >= 0 else -1 for r in range(t80)]
        self.speech_idx += ([first] if t80 < added else []) + rows    # the repeated first row carries what it copies

    def get_decode_chunk(self):
        if oo.CHUNK_FRAMES > self.speech.shape[0]:
            return None
        pidx = [self.speech_idx[0] if self.splice is None else self.splice_idx] + self.speech_idx[: oo.CHUNK_FRAMES]
        chunk = super().get_decode_chunk()
        self.splice_idx = pidx[-1]
        frames = [pidx[6 * i] for i in range(chunk.shape[0] - 10)]   # an LFR frame (lfr_n = 6) takes its first row's index
        self.chunk_idx = self.cache_idx + frames
        self.cache_idx = self.chunk_idx[-10:]
        self.speech_idx = self.speech_idx[oo.CHUNK_FRAMES:]
        return chunk

    def reset(self):
        super().reset()
        self.cache_idx, self.carry_idx, self.info = [-1] * 10, -1, []

    def index_from(self, p):
        for q in range(max(p, 0), len(self.chunk_idx)):
            if self.chunk_idx[q] >= 0:
                return self.chunk_idx[q]
        return self.caller_samples

    def position_ms(self, p):
        return time_ms(self.index_from(p))

    def times(self, entries, hi=HI):
        """the times of this chunk's fires (entry 0: the carry), then the carry's time for the next chunk"""
        out = []
        for e in entries:
            idx = (self.carry_idx if self.carry_idx >= 0 else self.caller_samples) if e == 0 else self.index_from(e - 1)
            out.append(time_ms(idx))
        self.carry_idx = self.index_from(hi - 1)
        return out


class TimedRecognizer(LR.LockstepRecognizer):
    def create_stream(self):
        return TimedStream(self)

    def encoder(self, speech):
        self._enc = super().encoder(speech)
        return self._enc

    def decoder(self, enc, emb, lens, cin):
        if self.engine is not None:
            logp, ids, cout = self.engine.online_decoder(enc, emb, lens, cin, want_logits=True)
        else:
            from oracle import model as om
            logp, cout = self.graphs.decoder(enc, emb, lens, cin)
            ids = om.argmax_last(logp)
        ids = np.asarray(ids)
        self._score_bits = np.take_along_axis(np.ascontiguousarray(logp, dtype=F32), ids[..., None].astype(np.int64), axis=-1)[..., 0].view(np.uint32)
        return ids, cout

    def get_results(self, streams):
        work, seen = [], set()
        for s in streams:                                            # who will hand out a chunk, and with which carry
            if s.speech.shape[0] >= oo.CHUNK_FRAMES and id(s) not in seen:
                work.append((s, s.cif_hidden[0].copy(), F32(s.cif_alpha[0])))
                seen.add(id(s))
        res = super().get_results(streams)
        B, L, lens = self.calls[-1]
        assert B == len(work)
        if B:
            enc, alphas = self._enc
            thr = self.graphs.o.cfg.cif_threshold
            for b, (s, ch, ca) in enumerate(work):
                _, ent, _, _ = walk(np.concatenate([ch[None], enc[b]]), np.concatenate([[ca], mask(alphas[b])]).astype(F32), thr)
                assert len(ent) == lens[b]
                tm = s.times(ent)
                if L > 0:
                    ids = s.tokens[-L:]
                    for l in range(L):
                        bits = int(self._score_bits[b, l])
                        s.info.append((ids[l], tm[l], ent[l], True, bits) if l < len(ent) else (ids[l], -1, -1, False, bits))
        return res


# ------------------------------------------------------------------------------------------------ the case table
class StepCase:
    """a stream: its first state (None: zeros) and a chain of calls (hiddens [Tc, D], alphas [Tc], reset)"""

    def __init__(self, name, D, Tc, calls, state0=None, threshold=1.0):
        self.name, self.D, self.Tc, self.calls, self.state0, self.threshold = name, D, Tc, calls, state0, threshold


CHAIN = 6


def _rand_call(r, Tc, D, scale=1.0):
    return (r.standard_normal((Tc, D)) * scale).astype(F32), r.random(Tc).astype(F32), False


def _pad(r, calls, Tc, D):
    return calls + [_rand_call(r, Tc, D) for _ in range(CHAIN - len(calls))]


def step_cases():
    """Every case is a chain of CHAIN calls (the named situation first, random calls behind it), so that cases of one shape run
    side by side as the streams of one launch."""
    out = []
    Tc, D = 20, 512
    r = np.random.default_rng(511)
    out.append(StepCase("random", D, Tc, _pad(r, [], Tc, D)))
    # sums of 0.25 / 0.5 that land on the threshold exactly: strict < fires on equality (three times in the window, nothing carried)
    dy = np.zeros(Tc, F32)
    dy[:5] = 0.5                                                      # masked away
    dy[5:15] = [0.5, 0.5, 0.25, 0.25, 0.5, 0.25, 0.25, 0.25, 0.25, 0.0]
    dy[15:] = 0.75                                                    # masked away
    hd = (r.integers(-16, 17, (Tc, D)) / 8.0).astype(F32)
    out.append(StepCase("dyadic", D, Tc, _pad(r, [(hd, dy, False), (hd[::-1].copy(), dy, False)], Tc, D)))
    # no fire: the carry is divided by the integrate
    out.append(StepCase("no-fire", D, Tc, _pad(r, [(_rand_call(r, Tc, D)[0], np.full(Tc, 0.05, F32), False)] * 2, Tc, D)))
    # an all-zero chunk on a fresh block: integrate == 0, the carry stays unscaled; then again behind a carry
    z = (_rand_call(r, Tc, D)[0], np.zeros(Tc, F32), False)
    out.append(StepCase("all-zero", D, Tc, _pad(r, [z, _rand_call(r, Tc, D), z], Tc, D)))
    # a carried integrate at and above the threshold: entry 0 fires
    for name, v in (("carry-at-threshold", 1.0), ("carry-above-threshold", 1.5)):
        s0 = new_state(D)
        s0[:D] = r.standard_normal(D).astype(F32)
        s0[D: D + groups(D)] = F32(v)
        out.append(StepCase(name, D, Tc, _pad(r, [], Tc, D), state0=s0))
    # a reset at the 4th call
    calls = _pad(r, [], Tc, D)
    calls[3] = (calls[3][0], calls[3][1], True)
    out.append(StepCase("reset-at-4", D, Tc, calls))
    # large and negative rows with alphas near 1: many fires per chunk; a threshold other than 1
    out.append(StepCase("dense", D, Tc, [((r.standard_normal((Tc, D)) * 30).astype(F32), (0.7 + 0.3 * r.random(Tc)).astype(F32), False)
                                         for _ in range(CHAIN)]))
    out.append(StepCase("threshold-0.9", D, Tc, _pad(r, [], Tc, D), threshold=0.9))
    # one-hot rows: a fired frame shows which entries it was built from
    for k in range(3):
        rr = np.random.default_rng(520 + k)
        calls = []
        for _ in range(CHAIN):
            h = np.zeros((Tc, 8), F32)
            h[np.arange(Tc), rr.integers(0, 8, Tc)] = 1
            calls.append((h, rr.random(Tc).astype(F32), False))
        out.append(StepCase("one-hot-%d" % k, 8, Tc, calls))
    # the shapes at which the kernel takes another path: a second tile of rows (Tc > 20), a chunk shorter than hi, a last channel
    # group that is not full (D = 260: one float4 in the second group)
    for Tc2, D2 in ((23, 12), (7, 260), (41, 516)):
        for k in range(3):
            rr = np.random.default_rng([530 + k, Tc2])
            out.append(StepCase("Tc%d-D%d-%d" % (Tc2, D2, k), D2, Tc2, [_rand_call(rr, Tc2, D2) for _ in range(CHAIN)]))
    return out


def run_case(case, step_fn=step):
    """the chain on one state: [(fired, fire_entry, count, state words after)] per call"""
    st = new_state(case.D) if case.state0 is None else case.state0.copy()
    out = []
    for h, a, rs in case.calls:
        f, e, n = step_fn(st, h, a, case.threshold, reset=rs)
        out.append((f, e, n, st.copy()))
    return out


# ------------------------------------------------------------------------------------------------ the library's two forms
def _ptr(x, t):
    import ctypes as C
    return x.ctypes.data_as(C.POINTER(t))


def host_step(state, hiddens, alphas, threshold, lo=LO, hi=HI, reset=False, cap=None, rc=False):
    """pf_host_online_cif_step with step()'s interface (rc=True: the return code alone, nothing else touched)"""
    import ctypes as C
    from aliparaformerasr_amd import _native as N
    Tc, D = hiddens.shape
    cap = Tc + 1 if cap is None else cap
    h, a = np.ascontiguousarray(hiddens, dtype=F32), np.ascontiguousarray(alphas, dtype=F32)
    fired, entry, n = np.full((max(cap, 1), D), 7, F32), np.full(max(cap, 1), 7, np.int32), C.c_int32(-7)
    code = N.load().pf_host_online_cif_step(state.ctypes.data_as(C.c_void_p), _ptr(h, C.c_float), _ptr(a, C.c_float), Tc, D, float(threshold),
                                             lo, hi, int(reset), _ptr(fired, C.c_float), _ptr(entry, C.c_int32), cap, n)
    if rc:
        return code
    N.check(code)
    return fired[:cap], entry[:cap], n.value


def op_step(engine, states, hiddens, alphas, threshold, resets, lo=LO, hi=HI, cap=None):
    """pf_op_online_cif_step: states [B, words] (updated in place), hiddens [B, Tc, D], alphas [B, Tc], resets [B] ->
    fired [B, cap, D], fire_entry [B, cap], counts [B]"""
    import ctypes as C
    from aliparaformerasr_amd import _native as N
    B, Tc, D = hiddens.shape
    cap = Tc + 1 if cap is None else cap
    assert states.dtype == F32 and states.flags.c_contiguous and states.shape == (B, state_words(D))
    h, a = np.ascontiguousarray(hiddens, dtype=F32), np.ascontiguousarray(alphas, dtype=F32)
    rs = np.ascontiguousarray(resets, dtype=np.int32)
    fired, entry, n = np.full((B, cap, D), 7, F32), np.full((B, cap), 7, np.int32), np.full(B, -7, np.int32)
    N.check(N.load().pf_op_online_cif_step(engine._h, states.ctypes.data_as(C.c_void_p), _ptr(h, C.c_float), _ptr(a, C.c_float),
                                           _ptr(rs, C.c_int32), B, Tc, D, float(threshold), lo, hi, _ptr(fired, C.c_float),
                                           _ptr(entry, C.c_int32), cap, _ptr(n, C.c_int32)))
    return fired, entry, n
