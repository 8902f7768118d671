"""numpy-facing wrapper of the pf_engine C ABI (device engine + stand-alone device ops)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class CtcResult:
    """The CTC collapse of a batch (PF_DECODE_CTC): n [B] token counts; ids (int64), first / last (frame indices in the
    row, prompt rows included) and score (the run's largest frame log-prob), each [B, max(n)]; slots past n[b] hold
    -1 / -1 / -1 / 0."""

    def __init__(self, n, ids, first, last, score):
        self.n, self.ids, self.first, self.last, self.score = n, ids, first, last, score

    def tokens(self, b):
        """[(id, first, last, score)] of utterance b."""
        k = int(self.n[b])
        return list(zip(self.ids[b, :k].tolist(), self.first[b, :k].tolist(), self.last[b, :k].tolist(),
                        self.score[b, :k].tolist()))


class TopkResult:
    """The K best entries of every position (PF_DECODE_TOPK): ids [B, L, K] int64, val [B, L, K] float32 log-probs,
    n [B, L] ranked entries; slots past n hold -1 / -inf.  Order: larger value first, of equal values the larger id."""

    def __init__(self, ids, val, n):
        self.ids, self.val, self.n = ids, val, n
        self.K = ids.shape[-1]


def host_nbest(val, n, n_free, n_best, ids=None):
    """The exact n-best list of one utterance from its top-k lists val [L, K], n [L] (pf_host_nbest): (ranks [m, L] int32,
    scores [m] float64) with m <= n_best, by descending score, ties to the lexicographically smaller rank vector;
    positions l >= n_free keep rank 0.  ids [L, K] (optional): the hypotheses' ids [m, L] are returned as a third item."""
    v = _f32(val)
    nn = np.ascontiguousarray(n, dtype=np.int32)
    L, K = v.shape
    ranks = np.zeros((n_best, L), np.int32)
    scores = np.zeros(n_best, np.float64)
    got = C.c_int32()
    N.check(N.load().pf_host_nbest(None, _fp(v), _i32p(nn), L, K, int(n_free), int(n_best), _i32p(ranks),
                                   scores.ctypes.data_as(C.POINTER(C.c_double)), got))
    ranks, scores = ranks[: got.value].copy(), scores[: got.value].copy()
    if ids is None:
        return ranks, scores
    y = np.asarray(ids)
    return ranks, scores, y[np.arange(L)[None, :], ranks]


class CtcBeamResult:
    """The labelings a CTC prefix beam search kept (PF_DECODE_CTC_BEAM): n_hyp [B]; ids [B, N, cap] int64 (-1 past a
    hypothesis' length), len [B, N], score [B, N] float64 (the log of the summed alignments; -inf past n_hyp[b])."""

    def __init__(self, n_hyp, ids, len_, score, matched=None, loglik_sum=None, lm_sum=None):
        self.n_hyp, self.ids, self.len, self.score = n_hyp, ids, len_, score
        # language model (host_ctc_beam_lm / op_ctc_beam_lm), else None: lm_sum [B, N] float64, the weighted LM score of a
        # labeling; score == (loglik_sum + boost * matched) + lm_sum
        self.lm_sum = lm_sum
        self.N = score.shape[-1]
        # hot words (Engine.set_ctc_hotwords / host_ctc_beam_hot / op_ctc_beam_hot), else None: matched [B, N] int32, the
        # hot-word tokens a labeling completed; loglik_sum [B, N] float64 = score - boost * matched, the unbiased log of the sum
        self.matched, self.loglik_sum = matched, loglik_sum

    def hyps(self, b=0):
        """[(ids tuple, score)] of utterance b, best first."""
        return [(tuple(self.ids[b, i, : int(self.len[b, i])].tolist()), float(self.score[b, i])) for i in range(int(self.n_hyp[b]))]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def host_ctc_beam(blank_lp, ids, val, n, W, n_best=None, blank=0, cap=None, blank_stride=1) -> CtcBeamResult:
    """The beam search of ONE utterance in host code (pf_host_ctc_beam, the twin of the device kernel): blank_lp
    [T * blank_stride], ids / val [T, K], n [T] -> CtcBeamResult with B = 1."""
    y = np.ascontiguousarray(ids, dtype=np.int64)
    v = _f32(val)
    nn = np.ascontiguousarray(n, dtype=np.int32)
    lb = _f32(blank_lp).reshape(-1)
    T, K = y.shape
    n_best = W if n_best is None else n_best
    cap = max(T, 1) if cap is None else cap
    oi = np.zeros((1, max(n_best, 0), cap), np.int64)
    ol = np.zeros((1, max(n_best, 0)), np.int32)
    sc = np.zeros((1, max(n_best, 0)), np.float64)
    nh = np.zeros(1, np.int32)
    N.check(N.load().pf_host_ctc_beam(_fp(lb), int(blank_stride), _i64p(y), _fp(v), _i32p(nn), T, K, int(blank), int(W), int(n_best),
                                      _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh)))
    return CtcBeamResult(nh, oi, ol, sc)


def _hot_arrays(hotwords):
    """A hot-word set (sequences of ids) as the C entry points take it: flat int32 ids, int32 lengths."""
    ids = np.ascontiguousarray([c for w in hotwords for c in w], dtype=np.int32).reshape(-1)
    lens = np.ascontiguousarray([len(w) for w in hotwords], dtype=np.int32).reshape(-1)
    return ids, lens


class HotwordGraph:
    """The automaton of a hot-word set (pf_host_hotword_graph): S states, A columns, tok_col [V], table [S, A], depth [S]."""

    def __init__(self, hotwords, V):
        ids, lens = _hot_arrays(hotwords)
        lib = N.load()
        s, a = C.c_int32(), C.c_int32()
        N.check(lib.pf_host_hotword_graph(_i32p(ids), _i32p(lens), len(lens), int(V), s, a, None, None, 0, None, 0))
        self.S, self.A = s.value, a.value
        self.tok_col = np.zeros(int(V), np.int32)
        self.table = np.zeros((self.S, self.A), np.int32)
        self.depth = np.zeros(self.S, np.int32)
        N.check(lib.pf_host_hotword_graph(_i32p(ids), _i32p(lens), len(lens), int(V), s, a, _i32p(self.tok_col), _i32p(self.table),
                                          self.table.size, _i32p(self.depth), self.S))

    def step(self, state, token):
        """(next state, completed length) from `state` on `token`."""
        col = int(self.tok_col[token]) if 0 <= token < self.tok_col.shape[0] else -1
        if col < 0:
            return 0, 0
        e = int(self.table[state, col])
        return e & 0xFFFF, (e >> 16) & 0xFF


def host_ctc_beam_hot(blank_lp, ids, val, n, W, hotwords, boost, n_best=None, blank=0, cap=None, blank_stride=1) -> CtcBeamResult:
    """host_ctc_beam with a hot-word set (sequences of ids in [1, V)) and a boost >= 0 (pf_host_ctc_beam_hot): the biased
    search of ONE utterance in host code -> CtcBeamResult with B = 1, matched and loglik_sum filled."""
    y = np.ascontiguousarray(ids, dtype=np.int64)
    v = _f32(val)
    nn = np.ascontiguousarray(n, dtype=np.int32)
    lb = _f32(blank_lp).reshape(-1)
    T, K = y.shape
    n_best = W if n_best is None else n_best
    cap = max(T, 1) if cap is None else cap
    hi, hl = _hot_arrays(hotwords)
    oi = np.zeros((1, max(n_best, 0), cap), np.int64)
    ol = np.zeros((1, max(n_best, 0)), np.int32)
    sc = np.zeros((1, max(n_best, 0)), np.float64)
    om = np.zeros((1, max(n_best, 0)), np.int32)
    oll = np.zeros((1, max(n_best, 0)), np.float64)
    nh = np.zeros(1, np.int32)
    N.check(N.load().pf_host_ctc_beam_hot(_fp(lb), int(blank_stride), _i64p(y), _fp(v), _i32p(nn), T, K, int(blank), int(W), int(n_best),
                                          _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh), _i32p(hi), _i32p(hl), len(hl), float(boost),
                                          _i32p(om), _dp(oll)))
    return CtcBeamResult(nh, oi, ol, sc, om, oll)


class LanguageModel:
    """A back-off n-gram language model compiled into the flat image the beam search walks (pf_host_lm_build /
    pf_host_lm_from_arpa; see "CTC language model" in the header).  ngrams: {tuple of ids: (logp, backoff or None)} with
    natural-log float32 weights; or LanguageModel.from_arrays / from_arpa.  Release with close() (an engine that uploaded it
    keeps its own reference)."""

    def __init__(self, order, ngrams, V, bos=-1, eos=-1, unk=-1, oov=-10.0, transparent=(), _handle=None):
        self._lib = N.load()
        self.dropped = 0
        self._h = _handle
        if _handle is None:
            by_k = [[w for w in ngrams if len(w) == k] for k in range(1, int(order) + 1)]
            if sum(len(x) for x in by_k) != len(ngrams):
                raise ValueError("an n-gram of order 0 or above the model's order")
            flat = [w for x in by_k for w in x]
            self._h = self._build(order, [len(x) for x in by_k], [c for w in flat for c in w], [ngrams[w][0] for w in flat],
                                  [np.nan if ngrams[w][1] is None else ngrams[w][1] for w in flat], V, bos, eos, unk, oov, transparent)
        o, s, a, b = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        N.check(self._lib.pf_host_lm_info(self._h, o, s, a, b))
        self.order, self.states, self.arcs, self.image_bytes = o.value, s.value, a.value, b.value

    @staticmethod
    def _build(order, counts, ids, logp, backoff, V, bos, eos, unk, oov, transparent):
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        logp = np.ascontiguousarray(logp, dtype=np.float32).reshape(-1)
        bo = np.ascontiguousarray(backoff, dtype=np.float32).reshape(-1)
        tr = np.ascontiguousarray(list(transparent), dtype=np.int32).reshape(-1)
        h = C.c_void_p()
        N.check(N.load().pf_host_lm_build(int(order), _i64p(counts), _i32p(ids), _fp(logp), _fp(bo), int(V), int(bos), int(eos), int(unk),
                                          float(oov), _i32p(tr), len(tr), C.byref(h)))
        return h

    @classmethod
    def from_arrays(cls, order, counts, ids, logp, backoff, V, bos=-1, eos=-1, unk=-1, oov=-10.0, transparent=()):
        """The builder's own argument form: counts [order], then per listed n-gram (all 1-grams first) its ids flattened, logp
        and backoff (NaN: none)."""
        return cls(0, {}, 0, _handle=cls._build(order, counts, ids, logp, backoff, V, bos, eos, unk, oov, transparent))

    @classmethod
    def from_arpa(cls, path, tokens, oov=-10.0):
        """ARPA text against a token table (list of str): words map to ids by exact equality; .dropped counts the n-grams left
        out because a word is not in the table."""
        arr = (C.c_char_p * len(tokens))(*[t.encode("utf-8") for t in tokens])
        h, d = C.c_void_p(), C.c_int64()
        N.check(N.load().pf_host_lm_from_arpa(str(path).encode("utf-8"), arr, len(tokens), float(oov), d, C.byref(h)))
        lm = cls(0, {}, 0, _handle=h)
        lm.dropped = d.value
        return lm

    def score(self, ids, alpha=1.0, beta=0.0, flags=0):
        """The plain walk over ids (pf_host_lm_score): (g, state, g_pos [n] float64, state_pos [n] int32)."""
        y = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        g, st = C.c_double(), C.c_int32()
        gp, sp = np.zeros(len(y), np.float64), np.zeros(len(y), np.int32)
        N.check(self._lib.pf_host_lm_score(self._h, _i32p(y), len(y), float(alpha), float(beta), int(flags), g, st, _dp(gp), _i32p(sp)))
        return g.value, st.value, gp, sp

    def close(self):
        if self._h is not None:
            self._lib.pf_lm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_ctc_beam_lm(blank_lp, ids, val, n, W, lm, alpha, beta, flags=0, hotwords=(), boost=0.0, n_best=None, blank=0, cap=None,
                     blank_stride=1) -> CtcBeamResult:
    """host_ctc_beam_hot with a LanguageModel fused in (pf_host_ctc_beam_lm): ONE utterance in host code -> CtcBeamResult with
    B = 1, matched, loglik_sum and lm_sum filled.  An empty hot-word set is allowed."""
    y = np.ascontiguousarray(ids, dtype=np.int64)
    v = _f32(val)
    nn = np.ascontiguousarray(n, dtype=np.int32)
    lb = _f32(blank_lp).reshape(-1)
    T, K = y.shape
    n_best = W if n_best is None else n_best
    cap = max(T, 1) if cap is None else cap
    hi, hl = _hot_arrays(hotwords)
    nb = max(n_best, 0)
    oi, ol, sc = np.zeros((1, nb, cap), np.int64), np.zeros((1, nb), np.int32), np.zeros((1, nb), np.float64)
    om, oll, olm = np.zeros((1, nb), np.int32), np.zeros((1, nb), np.float64), np.zeros((1, nb), np.float64)
    nh = np.zeros(1, np.int32)
    N.check(N.load().pf_host_ctc_beam_lm(_fp(lb), int(blank_stride), _i64p(y), _fp(v), _i32p(nn), T, K, int(blank), int(W), int(n_best),
                                         _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh), _i32p(hi), _i32p(hl), len(hl), float(boost),
                                         _i32p(om), _dp(oll), lm._h, float(alpha), float(beta), int(flags), _dp(olm)))
    return CtcBeamResult(nh, oi, ol, sc, om, oll, olm)


class NbestSearchResult:
    """The hypotheses the n-best search over a paraformer's top-k lists kept (Engine.set_nbest_search / host_nbest_search /
    op_nbest_search): n_hyp [B]; ranks [B, N, L] int32 (-1 past n_hyp[b]); score, loglik_sum [B, N] float64 (-inf), lm_sum
    [B, N] float64 (0), matched [B, N] int32 (0): score == (loglik_sum + boost * matched) + lm_sum bit for bit."""

    def __init__(self, n_hyp, ranks, score, loglik_sum, lm_sum, matched):
        self.n_hyp, self.ranks, self.score, self.loglik_sum, self.lm_sum, self.matched = n_hyp, ranks, score, loglik_sum, lm_sum, matched
        self.N = score.shape[-1]

    def hyps(self, b=0):
        """[(ranks tuple, score, loglik_sum, lm_sum, matched)] of utterance b, best first."""
        return [(tuple(self.ranks[b, i].tolist()), float(self.score[b, i]), float(self.loglik_sum[b, i]), float(self.lm_sum[b, i]),
                 int(self.matched[b, i])) for i in range(int(self.n_hyp[b]))]


def _nbest_search_out(B, n_best, L, out):
    if out is not None:
        return out
    nb = max(n_best, 0)
    return (np.zeros((B, nb, L), np.int32), np.zeros((B, nb), np.float64), np.zeros((B, nb), np.float64), np.zeros((B, nb), np.float64),
            np.zeros((B, nb), np.int32), np.zeros(B, np.int32))


def host_nbest_search(ids, val, n, token_num, W, n_best=None, lm=None, alpha=0.0, beta=0.0, flags=0, hotwords=(), boost=0.0,
                      out=None) -> NbestSearchResult:
    """The n-best search of ONE utterance in host code (pf_host_nbest_search, the twin of the device kernel): ids / val [L, K],
    n [L], token_num -> NbestSearchResult with B = 1.  lm: a LanguageModel or None; hotwords: sequences of ids."""
    y = np.ascontiguousarray(ids, dtype=np.int64)
    v = _f32(val)
    nn = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
    L, K = y.shape
    n_best = W if n_best is None else n_best
    hi, hl = _hot_arrays(hotwords)
    rk, sc, ll, g, m, nh = _nbest_search_out(1, n_best, L, out)
    N.check(N.load().pf_host_nbest_search(_i64p(y), _fp(v), _i32p(nn), L, K, int(token_num), int(W), int(n_best), _i32p(hi), _i32p(hl),
                                          len(hl), float(boost), None if lm is None else lm._h, float(alpha), float(beta), int(flags),
                                          _i32p(rk), _dp(sc), _dp(ll), _dp(g), _i32p(m), _i32p(nh)))
    return NbestSearchResult(nh, rk, sc, ll, g, m)


class AlignResult:
    """CTC forced alignments (PF_DECODE_ALIGN), H jobs per utterance: path_score [B, H] float32 (the Viterbi score), loglik
    [B, H] float64 (the log of the summed alignments), ok [B, H], len [B, H] (the target's length; -1: a skipped job), first /
    last [B, H, cap] int32 frame indices (-1 past len and when not ok), tok_score [B, H, cap] float32."""

    def __init__(self, path_score, loglik, ok, len_, first, last, tok_score):
        self.path_score, self.loglik, self.ok, self.len = path_score, loglik, ok, len_
        self.first, self.last, self.tok_score = first, last, tok_score
        self.H = ok.shape[-1]


def host_ctc_align(lp, y, V=None) -> AlignResult:
    """The alignment of ONE utterance and ONE target in host code (pf_host_ctc_align, the twin of the device kernel):
    lp [T, ld] log-prob rows (V <= ld entries read per row), y [U] ids in [1, V) -> AlignResult with B = H = 1."""
    x = _f32(lp)
    T, ld = x.shape
    yy = np.ascontiguousarray(y, dtype=np.int64).reshape(-1)
    U = yy.shape[0]
    ps, ll, ok = C.c_float(), C.c_double(), C.c_int32()
    cap = max(U, 1)
    first, last, tok = np.zeros((1, 1, cap), np.int32), np.zeros((1, 1, cap), np.int32), np.zeros((1, 1, cap), np.float32)
    N.check(N.load().pf_host_ctc_align(_fp(x), ld, T, int(ld if V is None else V), _i64p(yy), U, ps, ll, ok, _i32p(first), _i32p(last),
                                       _fp(tok)))
    return AlignResult(np.array([[ps.value]], np.float32), np.array([[ll.value]], np.float64), np.array([[ok.value]], np.int32),
                       np.array([[U]], np.int32), first[:, :, :U], last[:, :, :U], tok[:, :, :U])


def vad_config(**kw) -> "N.PfVadConfig":
    """pf_vad_config with the stated defaults (pf_vad_default), fields overridden by keyword."""
    c = N.PfVadConfig()
    N.check(N.load().pf_vad_default(C.byref(c)))
    for k, v in kw.items():
        assert hasattr(c, k) and k not in ("struct_size", "reserved"), k
        setattr(c, k, int(v))
    return c


def _vad_cfg_ptr(cfg):
    if cfg is None:
        return None
    return C.byref(cfg if isinstance(cfg, N.PfVadConfig) else vad_config(**cfg))


def host_vad_levels(rows) -> np.ndarray:
    """Step 1 of the voice-activity segmentation in host code (pf_host_vad_levels): rows [T, n_mels] -> levels [T] int32."""
    x = _f32(rows)
    T, m = x.shape
    out = np.zeros(T, np.int32)
    N.check(N.load().pf_host_vad_levels(_fp(x), T, m, _i32p(out)))
    return out


def host_vad_segments(levels, n_mels=80, cfg=None, lfr_n=6, cap=None) -> np.ndarray:
    """Steps 2-6 for ONE utterance in host code (pf_host_vad_segments): levels [T] int32 -> segments [n, 2] frame pairs.
    cfg: None (the defaults), a PfVadConfig or a dict of its fields."""
    e = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
    lib, n = N.load(), C.c_int32()
    if cap is None:
        rc = lib.pf_host_vad_segments(_i32p(e), e.size, int(n_mels), int(lfr_n), _vad_cfg_ptr(cfg), None, 0, n)
        if rc != N.PF_ERR_CAPACITY:
            N.check(rc)
        cap = n.value
    seg = np.zeros((max(cap, 1), 2), np.int32)
    N.check(lib.pf_host_vad_segments(_i32p(e), e.size, int(n_mels), int(lfr_n), _vad_cfg_ptr(cfg), _i32p(seg), int(cap), n))
    return seg[: n.value].copy()


def endpoint_config(**kw) -> "N.PfEndpointConfig":
    """pf_endpoint_config with the stated defaults (pf_endpoint_default), fields overridden by keyword."""
    c = N.PfEndpointConfig()
    N.check(N.load().pf_endpoint_default(C.byref(c)))
    for k, v in kw.items():
        assert hasattr(c, k) and k not in ("struct_size", "reserved"), k
        setattr(c, k, int(v))
    return c


def _endpoint_cfg_ptr(cfg):
    if cfg is None:
        return None
    return C.byref(cfg if isinstance(cfg, N.PfEndpointConfig) else endpoint_config(**cfg))


def endpoint_state() -> np.ndarray:
    """A fresh stream's state block of the streaming endpoint detector: PF_ENDPOINT_STATE_INTS zeros."""
    return np.zeros(N.PF_ENDPOINT_STATE_INTS, np.int32)


def host_endpoint_update(state, levels, flush=False, n_mels=80, cfg=None, lfr_n=6, cap=None):
    """The streaming endpoint detector for ONE stream in host code (pf_host_endpoint_update): `levels` (int32, any count, may be
    empty) and then the flush.  state [PF_ENDPOINT_STATE_INTS] int32 is updated in place.  Returns (events [n, 3] = (begin, end,
    kind) frames, in_speech, open_begin).  cap: the capacity handed over (default: what always suffices); too small raises
    PfError(PF_ERR_CAPACITY) whose .n is the count and .events the first cap events."""
    assert isinstance(state, np.ndarray) and state.dtype == np.int32 and state.shape == (N.PF_ENDPOINT_STATE_INTS,) and state.flags.c_contiguous
    e = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
    cap = e.size + 1 if cap is None else cap                     # a frame gives at most one event, the flush one more
    ev = np.full((max(cap, 1), 3), -7, np.int32)
    n, ins, ob =C.c_int32(), C.c_int32(), C.c_int32()
    rc = N.load().pf_host_endpoint_update(_i32p(state), _i32p(e), e.size, int(bool(flush)), int(n_mels), int(lfr_n), _endpoint_cfg_ptr(cfg),
                                          _i32p(ev), int(cap), n, ins, ob)
    if rc < 0:
        try:
            N.check(rc)
        except N.PfError as ex:
            ex.n, ex.events = n.value, ev[: min(n.value, cap)].copy()
            raise
    return ev[: n.value].copy(), ins.value, ob.value


def vad_model_config(**kw) -> "N.PfVadConfig":
    """pf_vad_config with the defaults that go with the model score (pf_vad_model_config: floor_pct = -1, abs_level = 9830,
    stated and not tuned), fields overridden by keyword."""
    c = N.PfVadConfig()
    N.check(N.load().pf_vad_model_config(C.byref(c)))
    for k, v in kw.items():
        assert hasattr(c, k) and k not in ("struct_size", "reserved"), k
        setattr(c, k, int(v))
    return c


VAD_MODEL_DIMS = ("input_dim", "affine_dim", "linear_dim", "proj_dim", "output_dim", "n_layers", "lorder", "lstride", "lfr_m")


class VadModel:
    """An FSMN-VAD model: a `.pfw` of kind "fsmnvad" loaded and validated on the host (pf_vad_model_load /
    pf_vad_model_from_memory; see "Voice-activity segmentation, model score" in the header).  Release with close() (an engine
    that attached it keeps its own reference)."""

    def __init__(self, handle):
        self._lib = N.load()
        self._h = handle
        d, ns, ib = np.zeros(9, np.int32), C.c_int32(), C.c_int64()
        N.check(self._lib.pf_vad_model_info(self._h, _i32p(d), ns, ib))
        self.dims = dict(zip(VAD_MODEL_DIMS, d.tolist()))
        self.image_bytes = ib.value
        sil, n = np.zeros(max(ns.value, 1), np.int32), C.c_int32()
        N.check(self._lib.pf_vad_model_sil_ids(self._h, _i32p(sil), ns.value, n))
        self.sil_ids = sil[: n.value].tolist()

    def tensor(self, name: str) -> np.ndarray:
        """A tensor as loaded, flat float32 (pf_vad_model_tensor)."""
        n = C.c_int64()
        N.check(self._lib.pf_vad_model_tensor(self._h, name.encode("utf-8"), None, 0, n))
        out = np.zeros(max(n.value, 1), np.float32)
        N.check(self._lib.pf_vad_model_tensor(self._h, name.encode("utf-8"), _fp(out), n.value, n))
        return out[: n.value]

    def close(self):
        if self._h is not None:
            self._lib.pf_vad_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_vad_model(source) -> VadModel:
    """A `.pfw` of kind "fsmnvad" from a path or from bytes -> VadModel."""
    h = C.c_void_p()
    if isinstance(source, (bytes, bytearray, memoryview)):
        buf = bytes(source)
        N.check(N.load().pf_vad_model_from_memory(C.cast(C.c_char_p(buf), C.c_void_p), len(buf), C.byref(h)))
    else:
        N.check(N.load().pf_vad_model_load(str(source).encode("utf-8"), C.byref(h)))
    return VadModel(h)


def host_vad_model_logits(model: VadModel, rows) -> np.ndarray:
    """The network for ONE utterance in host code, float64 (pf_host_vad_model_logits): rows [T, n_mels] -> [T, output_dim]."""
    x = _f32(rows)
    T, m = x.shape
    out = np.zeros((T, model.dims["output_dim"]), np.float64)
    N.check(N.load().pf_host_vad_model_logits(model._h, _fp(x), T, m, _dp(out)))
    return out


def host_vad_model_levels(model: VadModel, rows) -> np.ndarray:
    """The model score of ONE utterance in host code (pf_host_vad_model_levels): rows [T, n_mels] -> levels [T] int32."""
    x = _f32(rows)
    T, m = x.shape
    out = np.zeros(T, np.int32)
    N.check(N.load().pf_host_vad_model_levels(model._h, _fp(x), T, m, _i32p(out)))
    return out


def endpoint_model_config(**kw) -> "N.PfEndpointConfig":
    """pf_endpoint_config with the defaults that go with the streaming model score (pf_endpoint_model_config: rise = -1,
    abs_level = 9830, stated and not tuned), fields overridden by keyword."""
    c = N.PfEndpointConfig()
    N.check(N.load().pf_endpoint_model_config(C.byref(c)))
    for k, v in kw.items():
        assert hasattr(c, k) and k not in ("struct_size", "reserved"), k
        setattr(c, k, int(v))
    return c


def vad_model_stream_state(model: VadModel, B=None, host=False) -> np.ndarray:
    """Fresh (all-zero) state blocks of the streaming model score: uint8 [state_bytes], or [B, state_bytes] when B is given.
    host=False: the device form's (pf_vad_model_stream_state_bytes); True: the host twin's own."""
    n = C.c_int64()
    fn = N.load().pf_host_vad_model_stream_state_bytes if host else N.load().pf_vad_model_stream_state_bytes
    N.check(fn(model._h, C.byref(n)))
    return np.zeros(n.value if B is None else (B, n.value), np.uint8)


def host_vad_model_stream(model: VadModel, state, rows, flush=False, cap=None, n_mels=None):
    """The streaming model score for ONE stream in host code, float64 (pf_host_vad_model_stream): `rows` [n_new, n_mels] (may be
    empty) and then the flush.  state (vad_model_stream_state(model, host=True)) is updated in place.  Returns (levels [n_out]
    int32, logits [n_out, output_dim] float64)."""
    assert isinstance(state, np.ndarray) and state.dtype == np.uint8 and state.ndim == 1 and state.flags.c_contiguous
    m = model.dims["input_dim"] // model.dims["lfr_m"] if n_mels is None else n_mels
    x = _f32(np.asarray(rows, np.float32).reshape(-1, m))
    cap = x.shape[0] + model.dims["lfr_m"] if cap is None else cap
    lev = np.zeros(max(cap, 1), np.int32)
    z = np.zeros((max(cap, 1), model.dims["output_dim"]), np.float64)
    n = C.c_int32()
    N.check(N.load().pf_host_vad_model_stream(model._h, state.ctypes.data_as(C.c_void_p), _fp(x), x.shape[0], int(bool(flush)), m,
                                              _i32p(lev), _dp(z), int(cap), C.byref(n)))
    return lev[: n.value].copy(), z[: n.value].copy()


SPK_MODEL_DIMS = ("n_mels", "m_channels", "init_channels", "growth", "bn_channels", "blocks0", "blocks1", "blocks2", "dilation0",
                  "dilation1", "dilation2", "seg_len", "embedding", "frame_width", "launches")


def spk_config(**kw) -> "N.PfSpkConfig":
    """pf_spk_config with the defaults (pf_spk_default), fields overridden by keyword."""
    c = N.PfSpkConfig()
    N.check(N.load().pf_spk_default(C.byref(c)))
    for k, v in kw.items():
        assert hasattr(c, k) and k not in ("struct_size", "reserved"), k
        setattr(c, k, float(v) if k == "threshold" else int(v))
    return c


def _spk_cfg_ptr(cfg):
    if cfg is None:
        return None
    return C.byref(cfg if isinstance(cfg, N.PfSpkConfig) else spk_config(**cfg))


class SpkModel:
    """A CAM++ speaker model: a `.pfw` of kind "campplus" loaded and validated on the host (pf_spk_model_load /
    pf_spk_model_from_memory; see "Speaker labels" in the header).  Release with close() (an engine that attached it keeps its
    own reference)."""

    def __init__(self, handle):
        self._lib = N.load()
        self._h = handle
        d, ib = np.zeros(16, np.int32), C.c_int64()
        N.check(self._lib.pf_spk_model_info(self._h, _i32p(d), ib))
        self.dims = dict(zip(SPK_MODEL_DIMS, d.tolist()))
        self.image_bytes = ib.value

    def close(self):
        if self._h is not None:
            self._lib.pf_spk_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_spk_model(source) -> SpkModel:
    """A `.pfw` of kind "campplus" from a path or from bytes -> SpkModel."""
    h = C.c_void_p()
    if isinstance(source, (bytes, bytearray, memoryview)):
        buf = bytes(source)
        N.check(N.load().pf_spk_model_from_memory(C.cast(C.c_char_p(buf), C.c_void_p), len(buf), C.byref(h)))
    else:
        N.check(N.load().pf_spk_model_load(str(source).encode("utf-8"), C.byref(h)))
    return SpkModel(h)


def host_spk_windows(segs, cfg=None):
    """The window plan of ONE stream (pf_host_spk_windows): segs [n, 2] frame pairs -> (windows [N, 3] int32 of (segment,
    begin, end), the shift used)."""
    s = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 2)
    lib, n, sh = N.load(), C.c_int32(), C.c_int32()
    rc = lib.pf_host_spk_windows(_i32p(s), s.shape[0], _spk_cfg_ptr(cfg), None, 0, n, sh)
    if rc != N.PF_ERR_CAPACITY:
        N.check(rc)
    win = np.zeros((max(n.value, 1), 3), np.int32)
    N.check(lib.pf_host_spk_windows(_i32p(s), s.shape[0], _spk_cfg_ptr(cfg), _i32p(win), n.value, n, sh))
    return win[: n.value].copy(), sh.value


def host_spk_cluster(S, cfg=None):
    """Average-linkage clustering of ONE stream's cosines (pf_host_spk_cluster): S [N, N] fp32 -> (labels [N] int32, speakers)."""
    a = _f32(S)
    a = a.reshape(a.shape[0], a.shape[0]) if a.size else a.reshape(0, 0)
    labels, k = np.zeros(max(a.shape[0], 1), np.int32), C.c_int32()
    N.check(N.load().pf_host_spk_cluster(_fp(a), a.shape[0], _spk_cfg_ptr(cfg), _i32p(labels), k))
    return labels[: a.shape[0]].copy(), k.value


def host_spk_segment_labels(segs, win_seg, win_label) -> np.ndarray:
    """The label of every segment from its windows' (pf_host_spk_segment_labels)."""
    s = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 2)
    ws, wl = np.ascontiguousarray(win_seg, dtype=np.int32).reshape(-1), np.ascontiguousarray(win_label, dtype=np.int32).reshape(-1)
    assert ws.size == wl.size
    out = np.zeros(max(s.shape[0], 1), np.int32)
    N.check(N.load().pf_host_spk_segment_labels(_i32p(s), s.shape[0], _i32p(ws), _i32p(wl), ws.size, _i32p(out)))
    return out[: s.shape[0]].copy()


def host_spk_centroids(emb, labels, K) -> np.ndarray:
    """Each speaker's centroid [K, E] (pf_host_spk_centroids)."""
    e = _f32(emb)
    l = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert e.ndim == 2 and e.shape[0] == l.size
    out = np.zeros((max(int(K), 1), e.shape[1]), np.float32)
    N.check(N.load().pf_host_spk_centroids(_fp(e), _i32p(l), l.size, e.shape[1], int(K), _fp(out)))
    return out[: int(K)].copy()


PUNC_MODEL_DIMS = ("vocab", "d_model", "heads", "ffn", "kernel", "n_layers", "n_punc", "sentence_end_id", "unk_word",
                   "id_unk", "id_none", "id_comma", "id_period", "id_question", "id_pause")


class PuncModel:
    """A CT-Transformer punctuation model: a `.pfw` of kind "cttransformer" loaded and validated on the host
    (pf_punc_model_load / pf_punc_model_from_memory; see "Punctuation" in the header).  Release with close() (an engine that
    attached it keeps its own reference)."""

    def __init__(self, handle):
        self._lib = N.load()
        self._h = handle
        d, ib = np.zeros(16, np.int32), C.c_int64()
        N.check(self._lib.pf_punc_model_info(self._h, _i32p(d), ib))
        self.dims = dict(zip(PUNC_MODEL_DIMS, d.tolist()))
        self.image_bytes = ib.value
        c = C.c_int32()
        N.check(self._lib.pf_punc_model_causal(self._h, C.byref(c)))
        self.causal = bool(c.value)                     # the streaming form (header key causal = 1)

    def close(self):
        if self._h is not None:
            self._lib.pf_punc_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_punc_model(source) -> PuncModel:
    """A `.pfw` of kind "cttransformer" from a path or from bytes -> PuncModel."""
    h = C.c_void_p()
    if isinstance(source, (bytes, bytearray, memoryview)):
        buf = bytes(source)
        N.check(N.load().pf_punc_model_from_memory(C.cast(C.c_char_p(buf), C.c_void_p), len(buf), C.byref(h)))
    else:
        N.check(N.load().pf_punc_model_load(str(source).encode("utf-8"), C.byref(h)))
    return PuncModel(h)


PUNC_STREAM_MAX_CONTEXT = 256
PUNC_STREAM_DEFAULT_CONTEXT = 200
PUNC_STREAM_NO_RESTARTS = 1


def punc_stream_state(model: PuncModel, B=None, host=False) -> np.ndarray:
    """A fresh streaming punctuation state: zeros uint8 [state_bytes] (B given: [B, state_bytes]).  host=False: the device
    form's (pf_punc_stream_state_bytes); True: the host twin's own."""
    nb = C.c_int64()
    fn = N.load().pf_host_punc_stream_state_bytes if host else N.load().pf_punc_stream_state_bytes
    N.check(fn(model._h, C.byref(nb)))
    return np.zeros(nb.value if B is None else (B, nb.value), np.uint8)


def host_punc_stream_step(model: PuncModel, state, ids, flush=False, max_context=PUNC_STREAM_DEFAULT_CONTEXT, flags=0,
                          want_logits=True):
    """One call of ONE stream in host code, float64 (pf_host_punc_stream_step): the new word ids in order, then the flush.
    state (punc_stream_state(model, host=True)) is updated in place.  Returns (marks [n] int32, mark_flags [n] int32, logits
    [n, n_punc] float64 or None, flush_mark)."""
    a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    assert isinstance(state, np.ndarray) and state.dtype == np.uint8 and state.flags.c_contiguous
    P = model.dims["n_punc"]
    mk, mf = np.full(max(a.size, 1), -77777, np.int32), np.full(max(a.size, 1), -77777, np.int32)
    z = np.zeros((max(a.size, 1), P), np.float64) if want_logits else None
    fm = C.c_int32(-77777)
    N.check(N.load().pf_host_punc_stream_step(model._h, state.ctypes.data_as(C.c_void_p), _i32p(a), a.size, int(bool(flush)),
                                              int(max_context), int(flags), _i32p(mk), _i32p(mf), _dp(z) if want_logits else None,
                                              C.byref(fm)))
    return mk[: a.size].copy(), mf[: a.size].copy(), (z[: a.size].copy() if want_logits else None), fm.value


def host_online_committed_words(model: PuncModel, tokens, ids, before=None):
    """The committed words of a streaming partial text (pf_host_online_committed_words): tokens = the token table, ids = the
    stream's Tokens.  Returns (the committed words, the held-back word or None).  before: the committed words of the last call;
    they must be a prefix of this call's (PF_ERR_RECOGNITION otherwise)."""
    tk = (C.c_char_p * max(len(tokens), 1))(*[t.encode("utf-8") for t in tokens])
    a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    ln, nc, nw = C.c_int64(), C.c_int32(), C.c_int32()
    bf = None if before is None else "\n".join(before).encode("utf-8")
    fn = N.load().pf_host_online_committed_words
    N.check(fn(model._h, tk, len(tokens), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, bf, None, 0, ln, nc, nw))
    buf = C.create_string_buffer(max(ln.value, 1))
    N.check(fn(model._h, tk, len(tokens), a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, bf, buf, ln.value, ln, nc, nw))
    words = buf.raw[: ln.value].decode("utf-8").split("\n") if nw.value else []
    return words[: nc.value], (words[nc.value] if nw.value > nc.value else None)


def host_punc_words(model: PuncModel, text: str):
    """The words of a text (pf_host_punc_words): (ids int32 [n], the words as strings)."""
    raw = text.encode("utf-8")
    n = C.c_int32()
    N.check(N.load().pf_host_punc_words(model._h, raw, None, None, None, 0, n))
    ids, b, e = (np.zeros(max(n.value, 1), np.int32) for _ in range(3))
    N.check(N.load().pf_host_punc_words(model._h, raw, _i32p(ids), _i32p(b), _i32p(e), n.value, n))
    return ids[: n.value].copy(), [raw[b[i]: e[i]].decode("utf-8") for i in range(n.value)]


def host_punc_logits(model: PuncModel, ids) -> np.ndarray:
    """The network on ONE window in host code, float64 (pf_host_punc_logits): ids [T] -> [T, n_punc]."""
    a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    out = np.zeros((a.size, model.dims["n_punc"]), np.float64)
    N.check(N.load().pf_host_punc_logits(model._h, _i32p(a), a.size, _dp(out)))
    return out


def host_punc_cut(model: PuncModel, p, last: bool):
    """The cut rule and the last-window edits on one window's p (pf_host_punc_cut): (cut, the edited p)."""
    a = np.array(p, dtype=np.int32).reshape(-1)
    cut = C.c_int32()
    N.check(N.load().pf_host_punc_cut(model._h, _i32p(a), a.size, 1 if last else 0, cut))
    return cut.value, a


def host_punc_ids(model: PuncModel, ids):
    """The text loop over the ids of one text in host code (pf_host_punc_ids): (punc_ids [n], [(window length, cut)])."""
    a = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    out = np.zeros(max(a.size, 1), np.int32)
    cap = a.size // 20 + 2
    wl, wc, nw = np.zeros(cap, np.int32), np.zeros(cap, np.int32), C.c_int32()
    N.check(N.load().pf_host_punc_ids(model._h, _i32p(a), a.size, _i32p(out), _i32p(wl), _i32p(wc), cap, nw))
    return out[: a.size].copy(), list(zip(wl[: nw.value].tolist(), wc[: nw.value].tolist()))


def host_punc_assemble(model: PuncModel, text: str, punc_ids):
    """The output text and its sentences (pf_host_punc_assemble): (text, [one past the last word of each sentence])."""
    raw = text.encode("utf-8")
    p = np.ascontiguousarray(punc_ids, dtype=np.int32).reshape(-1)
    cap = len(raw) + 17 * p.size + 16
    buf, ln, ns = C.create_string_buffer(cap), C.c_int64(), C.c_int32()
    se = np.zeros(max(p.size, 1), np.int32)
    N.check(N.load().pf_host_punc_assemble(model._h, raw, _i32p(p), p.size, buf, cap, ln, _i32p(se), se.size, ns))
    return buf.raw[: ln.value].decode("utf-8"), se[: ns.value].tolist()


def host_punc_text(model: PuncModel, text: str):
    """Words, loop and assembly on the host (pf_host_punc_text): (the punctuated text, punc_ids [n_words])."""
    raw = text.encode("utf-8")
    cap = 18 * len(raw) + 16
    buf, ln, nw = C.create_string_buffer(cap), C.c_int64(), C.c_int32()
    p = np.zeros(len(raw) + 1, np.int32)
    N.check(N.load().pf_host_punc_text(model._h, raw, buf, cap, ln, _i32p(p), p.size, nw))
    return buf.raw[: ln.value].decode("utf-8"), p[: nw.value].copy()


def host_long_plan(lens, batch_max=0, frame_budget=0):
    """The batch plan of long-audio recognition (pf_host_long_plan): ([(batch, row)] per segment, number of batches)."""
    ln = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
    b, r, nb = np.zeros(max(ln.size, 1), np.int32), np.zeros(max(ln.size, 1), np.int32), C.c_int32()
    N.check(N.load().pf_host_long_plan(_i32p(ln), ln.size, int(batch_max), int(frame_budget), _i32p(b), _i32p(r), nb))
    return list(zip(b[: ln.size].tolist(), r[: ln.size].tolist())), nb.value


class BatchResult:
    def __init__(self, token_ids, token_num, L, V, logits=None, cif_peak=None, scores=None, ctc=None, topk=None, beam=None,
                 align=None, search=None):
        self.search = search            # NbestSearchResult (PF_DECODE_TOPK with Engine.set_nbest_search) or None
        self.align = align              # AlignResult (Engine.set_decode(PF_DECODE_ALIGN) with targets or CTC_BEAM) or None
        self.token_ids = token_ids      # [B, L] int64
        self.token_num = token_num      # [B] int32
        self.L = L
        self.V = V
        self.logits = logits            # [B, L, V] float32 log-probs or None
        self.cif_peak = cif_peak        # [B, 3*Tmax] float32 us_cif_peak (timestamp models) or None
        self.scores = scores            # [B, L] float32 log-prob of token_ids (Engine.set_decode) or None
        self.ctc = ctc                  # CtcResult (Engine.set_decode(PF_DECODE_CTC)) or None
        self.topk = topk                # TopkResult (Engine.set_decode(PF_DECODE_TOPK)) or None
        self.beam = beam                # CtcBeamResult (Engine.set_decode(PF_DECODE_CTC_BEAM)) or None


def _build_config(weights, weights_path, weights_device_ptr, weights_bytes, cmvn, mvn_path, device, dither, snip_edges,
                  lfr_m, lfr_n, n_mels, fs, window, use_itn, frame_length_ms, frame_shift_ms, dither_seed, math_mode):
    """pf_engine_config + the Python objects whose memory it points into."""
    cfg = N.PfEngineConfig()
    cfg.struct_size = C.sizeof(N.PfEngineConfig)
    cfg.device = device
    keep = []
    if weights_path is not None:
        cfg.weights_path = weights_path.encode()
    elif weights_device_ptr is not None:
        cfg.weights_device = C.c_void_p(weights_device_ptr)
        cfg.weights_bytes = weights_bytes
    elif weights is not None:
        buf = (C.c_char * len(weights)).from_buffer_copy(weights) if not isinstance(weights, np.ndarray) else None
        if buf is None:
            arr = np.ascontiguousarray(weights, dtype=np.uint8)
            keep.append(arr)
            cfg.weights_host = arr.ctypes.data_as(C.c_void_p)
            cfg.weights_bytes = arr.nbytes
        else:
            keep.append(buf)
            cfg.weights_host = C.cast(buf, C.c_void_p)
            cfg.weights_bytes = len(weights)
    if mvn_path is not None:
        cfg.mvn_path = mvn_path.encode()
    elif cmvn is not None:
        sh, sc = _f32(cmvn[0]), _f32(cmvn[1])
        keep += [sh, sc]
        cfg.cmvn_shift, cfg.cmvn_scale, cfg.cmvn_dim = _fp(sh), _fp(sc), sh.shape[0]
    cfg.fs, cfg.n_mels, cfg.lfr_m, cfg.lfr_n = fs, n_mels, lfr_m, lfr_n
    cfg.snip_edges = 1 if snip_edges else 0
    cfg.dither = dither
    cfg.window = window.encode()
    cfg.use_itn = 1 if use_itn else 0
    cfg.frame_length_ms, cfg.frame_shift_ms = frame_length_ms, frame_shift_ms
    cfg.dither_seed, cfg.math_mode = dither_seed, math_mode
    return cfg, keep


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _fetch_decode(lib, h, B, L, flags):
    """scores / CTC result of the calling thread's last forward (before the pf_fetch that takes the ids)."""
    scores = ctc = None
    if flags & N.PF_DECODE_SCORES:
        scores = np.zeros((B, L), np.float32)
        N.check(lib.pf_fetch_scores(h, _fp(scores), scores.size, None))
    if flags & N.PF_DECODE_CTC:
        n, n_max = np.zeros(B, np.int32), C.c_int32()
        N.check(lib.pf_fetch_ctc(h, None, None, None, None, 0, _i32p(n), n_max))
        cap = max(n_max.value, 1)
        ids = np.zeros((B, cap), np.int64)
        first, last = np.zeros((B, cap), np.int32), np.zeros((B, cap), np.int32)
        score = np.zeros((B, cap), np.float32)
        N.check(lib.pf_fetch_ctc(h, ids.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(first), _i32p(last), _fp(score), cap,
                                 None, None))
        k = n_max.value
        ctc = CtcResult(n, ids[:, :k].copy(), first[:, :k].copy(), last[:, :k].copy(), score[:, :k].copy())
    return scores, ctc


def _fetch_topk(lib, h, B, L):
    k = C.c_int32()
    N.check(lib.pf_fetch_topk(h, None, None, None, 0, None, k))
    K = k.value
    ids = np.zeros((B, L, K), np.int64)
    val = np.zeros((B, L, K), np.float32)
    n = np.zeros((B, L), np.int32)
    N.check(lib.pf_fetch_topk(h, ids.ctypes.data_as(C.POINTER(C.c_int64)), _fp(val), _i32p(n), B * L, None, None))
    return TopkResult(ids, val, n)


def _fetch_ctc_beam(lib, h, B, n_best, hot=False, lm=False):
    nh = np.zeros(B, np.int32)
    mx = C.c_int32()
    N.check(lib.pf_fetch_ctc_beam(h, None, None, None, 0, _i32p(nh), mx))
    cap = max(mx.value, 1)
    ids = np.zeros((B, n_best, cap), np.int64)
    ln = np.zeros((B, n_best), np.int32)
    sc = np.zeros((B, n_best), np.float64)
    N.check(lib.pf_fetch_ctc_beam(h, _i64p(ids), _i32p(ln), _dp(sc), cap, None, None))
    if not hot and not lm:
        return CtcBeamResult(nh, ids, ln, sc)
    m, ll, g = np.zeros((B, n_best), np.int32), np.zeros((B, n_best), np.float64), None
    if hot:
        N.check(lib.pf_fetch_ctc_beam_hot(h, _i32p(m), _dp(ll)))
    if lm:
        g = np.zeros((B, n_best), np.float64)
        N.check(lib.pf_fetch_ctc_beam_lm(h, _dp(g), _dp(ll)))
    return CtcBeamResult(nh, ids, ln, sc, m, ll, g)


def _fetch_nbest_search(lib, h, B):
    ll, nn = C.c_int32(), C.c_int32()
    N.check(lib.pf_fetch_nbest_search(h, None, None, None, None, None, None, ll, nn))
    rk, sc, lg, g, m, nh = _nbest_search_out(B, nn.value, ll.value, None)
    N.check(lib.pf_fetch_nbest_search(h, _i32p(rk), _dp(sc), _dp(lg), _dp(g), _i32p(m), _i32p(nh), None, None))
    return NbestSearchResult(nh, rk, sc, lg, g, m)


def _fetch_align(lib, h, B):
    hh, mx = C.c_int32(), C.c_int32()
    N.check(lib.pf_fetch_align(h, None, None, None, None, None, None, None, 0, hh, mx))
    H, cap = hh.value, max(mx.value, 1)
    ps, ll = np.zeros((B, H), np.float32), np.zeros((B, H), np.float64)
    ok, ln = np.zeros((B, H), np.int32), np.zeros((B, H), np.int32)
    first, last, tok = np.zeros((B, H, cap), np.int32), np.zeros((B, H, cap), np.int32), np.zeros((B, H, cap), np.float32)
    if H:
        N.check(lib.pf_fetch_align(h, _fp(ps), _dp(ll), _i32p(ok), _i32p(ln), _i32p(first), _i32p(last), _fp(tok), cap, None, None))
    return AlignResult(ps, ll, ok, ln, first, last, tok)


def _collect_result(lib, fetch_fn, call, B, want_logits, decode=None):
    """The learn-L-then-fetch protocol shared by pf_engine and pf_group handles.  decode = (engine handle, flags):
    also the decoding extras of an engine with Engine.set_decode flags."""
    out = N.PfBatchOut()
    out.struct_size = C.sizeof(N.PfBatchOut)
    N.check(call(out))                       # first pass: learn L, V (no buffers)
    L, V, P = out.L, out.V, out.cif_peak_len
    peak = None
    if P > 0:
        peak = np.zeros((B, P), np.float32)
        out.cif_peak = _fp(peak)
        out.cif_peak_cap = peak.size
    ids = np.zeros((B, max(L, 1)), np.int64)
    tn = np.zeros(B, np.int32)
    out.token_ids = ids.ctypes.data_as(C.POINTER(C.c_int64))
    out.token_num = tn.ctypes.data_as(C.POINTER(C.c_int32))
    out.l_cap = max(L, 1)
    logits = None
    if want_logits:
        logits = np.zeros((B, L, V), np.float32)
        out.logits = _fp(logits)
        out.logits_cap = logits.size
    scores = ctc = None
    if decode is not None and decode[1]:
        scores, ctc = _fetch_decode(lib, decode[0], B, L, decode[1])
    topk = None
    if decode is not None and decode[1] & N.PF_DECODE_TOPK:
        topk = _fetch_topk(lib, decode[0], B, L)
    beam = None
    if decode is not None and decode[1] & N.PF_DECODE_CTC_BEAM:
        beam = _fetch_ctc_beam(lib, decode[0], B, decode[2], len(decode) > 3 and decode[3], len(decode) > 4 and decode[4])
    align = None
    if decode is not None and decode[1] & N.PF_DECODE_ALIGN:
        align = _fetch_align(lib, decode[0], B)
    search = None
    if decode is not None and decode[1] & N.PF_DECODE_TOPK and len(decode) > 5 and decode[5]:
        search = _fetch_nbest_search(lib, decode[0], B)
    N.check(fetch_fn(C.byref(out)))
    return BatchResult(ids[:, :L].copy(), tn, L, V, logits, peak, scores, ctc, topk, beam, align, search)


class Engine:
    """Device engine = OfflineModel + WavFrontend replacement (see include/paraformer_hip.h)."""

    def __init__(self, weights=None, weights_path=None, weights_device_ptr=None, weights_bytes=0,
                 cmvn=None, mvn_path=None, device=0, dither=0.0, snip_edges=False, lfr_m=7, lfr_n=6,
                 n_mels=80, fs=16000, window="hamming", use_itn=False, frame_length_ms=0, frame_shift_ms=0,
                 dither_seed=0, math_mode=0):
        self._lib = N.load()
        cfg, self._keep = _build_config(weights, weights_path, weights_device_ptr, weights_bytes, cmvn, mvn_path, device,
                                        dither, snip_edges, lfr_m, lfr_n, n_mels, fs, window, use_itn, frame_length_ms,
                                        frame_shift_ms, dither_seed, math_mode)
        h = C.c_void_p()
        N.check(self._lib.pf_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        kind, vocab, feat, ts = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        N.check(self._lib.pf_engine_info(self._h, kind, vocab, feat, ts))
        self.kind, self.vocab, self.feat_dim = kind.value, vocab.value, feat.value
        # the front-end geometry the library settled on (a value <= 0 selects its default)
        self.n_mels, self.lfr_m, self.lfr_n = (n_mels if n_mels > 0 else 80, lfr_m if lfr_m > 0 else 7,
                                               lfr_n if lfr_n > 0 else 6)
        self._decode = 0
        self._beam_n = 16
        self._hot = False
        self._lm = None
        self._vad_model = None
        self._punc_model = None
        self._spk_model = None
        self._search_w = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pf_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- front-end ----------------------------------------------------------
    def num_frames(self, n_samples: int) -> int:
        t = C.c_int32()
        N.check(self._lib.pf_frontend_num_frames(self._h, n_samples, t))
        return t.value

    def fbank(self, samples) -> np.ndarray:
        x = _f32(samples)
        m = self.n_mels
        cap = (x.shape[0] // 160 + 2) * m
        out = np.zeros(cap, np.float32)
        t = C.c_int32()
        N.check(self._lib.pf_fbank(self._h, _fp(x), x.shape[0], _fp(out), cap, t))
        return out[: t.value * m].reshape(t.value, m).copy()

    def frontend(self, samples) -> np.ndarray:
        x = _f32(samples)
        t = self.num_frames(x.shape[0])
        w = self.feat_dim
        out = np.zeros(max(t, 1) * w, np.float32)
        tt = C.c_int32()
        N.check(self._lib.pf_frontend(self._h, _fp(x), x.shape[0], _fp(out), out.shape[0], tt))
        return out[: tt.value * w].reshape(tt.value, w).copy()

    # ---- forward ------------------------------------------------------------
    def _collect(self, call, B, want_logits):
        return _collect_result(self._lib, lambda o: self._lib.pf_fetch(self._h, o), call, B, want_logits,
                               (self._h, self._decode, self._beam_n, self._hot, self._lm is not None, self._search_w > 0))

    def set_decode(self, flags: int):
        """Decoding extras of the forwards that follow (_native.PF_DECODE_SCORES | PF_DECODE_CTC; 0 = off, the reference
        behaviour): BatchResult.scores, and for a SenseVoice model BatchResult.ctc."""
        N.check(self._lib.pf_engine_set_decode(self._h, int(flags)))
        f = int(flags) | (N.PF_DECODE_TOPK if int(flags) & N.PF_DECODE_CTC_BEAM else 0)
        self._decode = f | (N.PF_DECODE_SCORES if f & (N.PF_DECODE_CTC | N.PF_DECODE_TOPK | N.PF_DECODE_ALIGN) else 0)

    def set_align_targets(self, targets):
        """Targets of the NEXT forward under PF_DECODE_ALIGN (consumed by it): one sequence of token ids per utterance, None
        for "no target for this row"; an empty list clears pending targets.  Ids, not text: the tokenizer is the caller's."""
        B = len(targets)
        ln = np.array([-1 if t is None else len(t) for t in targets], np.int32).reshape(B)
        cap = max(int(ln.max()) if B else 0, 1)
        ids = np.zeros((B, cap), np.int64)
        for b, t in enumerate(targets):
            if t is not None:
                ids[b, : len(t)] = np.asarray(t, dtype=np.int64)
        N.check(self._lib.pf_engine_set_align_targets(self._h, _i64p(ids), _i32p(ln), B, cap))

    host_ctc_align = staticmethod(host_ctc_align)

    def op_ctc_align(self, lp, tgt, tlen, lens, V=None, out=None) -> AlignResult:
        """The pipeline's alignment kernel on caller data: lp [B, T, ld] (V <= ld entries read per row), tgt [B, H, cap] int32,
        tlen [B, H] (-1 skips a job), lens [B].  out = (path_score, loglik, ok, first, last, tok_score): write into these."""
        x = _f32(lp)
        B, T, ld = x.shape
        y = np.ascontiguousarray(tgt, dtype=np.int32)
        tl = np.ascontiguousarray(tlen, dtype=np.int32)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        _, H, cap = y.shape
        if out is None:
            out = (np.zeros((B, H), np.float32), np.zeros((B, H), np.float64), np.zeros((B, H), np.int32),
                   np.zeros((B, H, cap), np.int32), np.zeros((B, H, cap), np.int32), np.zeros((B, H, cap), np.float32))
        ps, ll, ok, first, last, tok = out
        N.check(self._lib.pf_op_ctc_align(self._h, _fp(x), B, T, int(ld if V is None else V), ld, _i32p(y), _i32p(tl), _i32p(ln), H,
                                          cap, _fp(ps), _dp(ll), _i32p(ok), _i32p(first), _i32p(last), _fp(tok)))
        return AlignResult(ps, ll, ok, tl.copy(), first, last, tok)

    def set_ctc_beam(self, W: int = 16, n_best: int = 16):
        """Beam width W and list length n_best (1 <= n_best <= W <= 64, default 16 / 16) of PF_DECODE_CTC_BEAM for the
        forwards that follow."""
        N.check(self._lib.pf_engine_set_ctc_beam(self._h, int(W), int(n_best)))
        self._beam_n = int(n_best)

    host_ctc_beam = staticmethod(host_ctc_beam)
    host_ctc_beam_hot = staticmethod(host_ctc_beam_hot)
    host_ctc_beam_lm = staticmethod(host_ctc_beam_lm)

    def set_ctc_hotwords(self, hotwords, boost: float):
        """The hot-word set (sequences of token ids in [1, V)) and the boost per matched token (>= 0) of the forwards that
        follow (pf_engine_set_ctc_hotwords; SenseVoice only).  An empty set or boost 0 clears it.  With a set installed
        PF_DECODE_CTC_BEAM runs the biased search: BatchResult.beam comes in the biased order with matched and loglik_sum."""
        hi, hl = _hot_arrays(hotwords)
        N.check(self._lib.pf_engine_set_ctc_hotwords(self._h, _i32p(hi), _i32p(hl), len(hl), float(boost)))
        self._hot = float(np.float32(boost)) > 0 and any(len(w) > 0 for w in hotwords)

    def set_ctc_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, flags: int = 0):
        """The LanguageModel of the forwards that follow with its weight alpha >= 0, the per-token bonus beta and flags
        (_native.PF_LM_EOS) (pf_engine_set_ctc_lm; SenseVoice only); None clears it.  With a model installed PF_DECODE_CTC_BEAM
        runs the fused search: BatchResult.beam comes in the fused order with lm_sum and loglik_sum (matched 0 without hot words)."""
        N.check(self._lib.pf_engine_set_ctc_lm(self._h, None if lm is None else lm._h, float(alpha), float(beta), int(flags)))
        self._lm = lm

    host_nbest_search = staticmethod(host_nbest_search)

    def set_nbest_search(self, W: int = 16, n_best: int = None):
        """The n-best search of the forwards that follow (pf_engine_set_nbest_search; paraformer only): beam width W and list
        length n_best (1 <= n_best <= W <= 64; n_best None: W); W = 0 turns it off.  With it installed a forward with
        PF_DECODE_TOPK runs the search behind the top-k launch: BatchResult.search."""
        N.check(self._lib.pf_engine_set_nbest_search(self._h, int(W), int(W if n_best is None else n_best)))
        self._search_w = int(W)

    def set_nbest_lm(self, lm, alpha: float = 0.5, beta: float = 0.0, flags: int = 0):
        """The LanguageModel of the n-best search with its weight alpha >= 0, the per-token bonus beta and flags
        (pf_engine_set_nbest_lm; paraformer only); None clears it.  Inert until a search is installed."""
        N.check(self._lib.pf_engine_set_nbest_lm(self._h, None if lm is None else lm._h, float(alpha), float(beta), int(flags)))
        self._nbest_lm = lm                      # (keeps the handle alive while installed)

    def set_nbest_hotwords(self, hotwords, boost: float):
        """The hot-word set (sequences of token ids in [1, V)) and the boost per matched token (>= 0) of the n-best search
        (pf_engine_set_nbest_hotwords; paraformer only).  An empty set or boost 0 clears it.  Inert until a search is installed."""
        hi, hl = _hot_arrays(hotwords)
        N.check(self._lib.pf_engine_set_nbest_hotwords(self._h, _i32p(hi), _i32p(hl), len(hl), float(boost)))

    def op_nbest_search(self, ids, val, n, token_num, W, n_best=None, lm=None, alpha=0.0, beta=0.0, flags=0, hotwords=(), boost=0.0,
                        out=None) -> NbestSearchResult:
        """The search kernel alone on caller lists: ids / val [B, L, K], n [B, L], token_num [B].  out = (ranks [B, N, L] int32,
        score, loglik_sum, lm_sum [B, N] float64, matched [B, N] int32, n_hyp [B] int32): write into these arrays."""
        y = np.ascontiguousarray(ids, dtype=np.int64)
        v = _f32(val)
        nn = np.ascontiguousarray(n, dtype=np.int32)
        tn = np.ascontiguousarray(token_num, dtype=np.int32).reshape(-1)
        B, L, K = y.shape
        n_best = W if n_best is None else n_best
        hi, hl = _hot_arrays(hotwords)
        rk, sc, ll, g, m, nh = _nbest_search_out(B, n_best, L, out)
        N.check(self._lib.pf_op_nbest_search(self._h, _i64p(y), _fp(v), _i32p(nn), _i32p(tn), B, L, K, int(W), int(n_best), _i32p(hi),
                                             _i32p(hl), len(hl), float(boost), None if lm is None else lm._h, float(alpha), float(beta),
                                             int(flags), _i32p(rk), _dp(sc), _dp(ll), _dp(g), _i32p(m), _i32p(nh)))
        return NbestSearchResult(nh, rk, sc, ll, g, m)

    def op_ctc_beam_hot(self, blank_lp, ids, val, n, lens, W, hotwords, boost, n_best=None, blank=0, cap=None, out=None) -> CtcBeamResult:
        """op_ctc_beam with a hot-word set and a boost: the biased form of the kernel on caller data.  out = (ids, len, score,
        n_hyp, matched [B, N] int32, loglik_sum [B, N] float64): write into these arrays."""
        y = np.ascontiguousarray(ids, dtype=np.int64)
        v = _f32(val)
        nn = np.ascontiguousarray(n, dtype=np.int32)
        lb = _f32(blank_lp)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        B, T, K = y.shape
        n_best = W if n_best is None else n_best
        cap = max(T, 1) if cap is None else cap
        hi, hl = _hot_arrays(hotwords)
        if out is None:
            out = (np.zeros((B, max(n_best, 0), cap), np.int64), np.zeros((B, max(n_best, 0)), np.int32),
                   np.zeros((B, max(n_best, 0)), np.float64), np.zeros(B, np.int32), np.zeros((B, max(n_best, 0)), np.int32),
                   np.zeros((B, max(n_best, 0)), np.float64))
        oi, ol, sc, nh, om, oll = out
        N.check(self._lib.pf_op_ctc_beam_hot(self._h, _fp(lb), _i64p(y), _fp(v), _i32p(nn), _i32p(ln), B, T, K, int(blank), int(W),
                                             int(n_best), _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh), _i32p(hi), _i32p(hl),
                                             len(hl), float(boost), _i32p(om), _dp(oll)))
        return CtcBeamResult(nh, oi, ol, sc, om, oll)

    def op_ctc_beam_lm(self, blank_lp, ids, val, n, lens, W, lm, alpha, beta, flags=0, hotwords=(), boost=0.0, n_best=None, blank=0,
                       cap=None, out=None) -> CtcBeamResult:
        """op_ctc_beam_hot with a LanguageModel fused in: the kLm forms of the kernel on caller data.  out = (ids, len, score,
        n_hyp, matched [B, N] int32, loglik_sum [B, N] float64, lm_sum [B, N] float64): write into these arrays."""
        y = np.ascontiguousarray(ids, dtype=np.int64)
        v = _f32(val)
        nn = np.ascontiguousarray(n, dtype=np.int32)
        lb = _f32(blank_lp)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        B, T, K = y.shape
        n_best = W if n_best is None else n_best
        cap = max(T, 1) if cap is None else cap
        hi, hl = _hot_arrays(hotwords)
        nb = max(n_best, 0)
        if out is None:
            out = (np.zeros((B, nb, cap), np.int64), np.zeros((B, nb), np.int32), np.zeros((B, nb), np.float64), np.zeros(B, np.int32),
                   np.zeros((B, nb), np.int32), np.zeros((B, nb), np.float64), np.zeros((B, nb), np.float64))
        oi, ol, sc, nh, om, oll, olm = out
        N.check(self._lib.pf_op_ctc_beam_lm(self._h, _fp(lb), _i64p(y), _fp(v), _i32p(nn), _i32p(ln), B, T, K, int(blank), int(W),
                                            int(n_best), _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh), _i32p(hi), _i32p(hl), len(hl),
                                            float(boost), _i32p(om), _dp(oll), lm._h, float(alpha), float(beta), int(flags), _dp(olm)))
        return CtcBeamResult(nh, oi, ol, sc, om, oll, olm)

    def op_lm_score(self, lm, ids, lens, alpha=1.0, beta=0.0, out=None):
        """lm_walk_kernel on caller data (pf_op_lm_score): ids [B, L] int32, lens [B] -> (g [B, L] float64, state [B, L] int32)
        after every token p < lens[b]; positions past a length keep what `out` = (g, state) held."""
        y = np.ascontiguousarray(ids, dtype=np.int32)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        B, L = y.shape
        if out is None:
            out = (np.zeros((B, L), np.float64), np.zeros((B, L), np.int32))
        g, st = out
        N.check(self._lib.pf_op_lm_score(self._h, lm._h, _i32p(y), _i32p(ln), B, L, float(alpha), float(beta), _dp(g), _i32p(st)))
        return g, st

    def op_ctc_beam(self, blank_lp, ids, val, n, lens, W, n_best=None, blank=0, cap=None, out=None) -> CtcBeamResult:
        """The pipeline's beam search kernel on caller data: blank_lp [B, T], ids / val [B, T, K], n [B, T], lens [B].
        out = (ids [B, N, cap] int64, len [B, N] int32, score [B, N] float64, n_hyp [B] int32): write into these arrays."""
        y = np.ascontiguousarray(ids, dtype=np.int64)
        v = _f32(val)
        nn = np.ascontiguousarray(n, dtype=np.int32)
        lb = _f32(blank_lp)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        B, T, K = y.shape
        n_best = W if n_best is None else n_best
        cap = max(T, 1) if cap is None else cap
        if out is None:
            out = (np.zeros((B, max(n_best, 0), cap), np.int64), np.zeros((B, max(n_best, 0)), np.int32),
                   np.zeros((B, max(n_best, 0)), np.float64), np.zeros(B, np.int32))
        oi, ol, sc, nh = out
        N.check(self._lib.pf_op_ctc_beam(self._h, _fp(lb), _i64p(y), _fp(v), _i32p(nn), _i32p(ln), B, T, K, int(blank), int(W),
                                         int(n_best), _i64p(oi), _i32p(ol), _dp(sc), cap, _i32p(nh)))
        return CtcBeamResult(nh, oi, ol, sc)

    def set_topk(self, k: int):
        """K of PF_DECODE_TOPK (1 .. _native.PF_TOPK_MAX, default 4) for the forwards that follow."""
        N.check(self._lib.pf_engine_set_topk(self._h, int(k)))

    def fetch_topk(self, B: int) -> TopkResult:
        """The top-k lists of the calling thread's last forward of B utterances (before the fetch that takes its ids)."""
        L = C.c_int32()
        N.check(self._lib.pf_fetch_topk(self._h, None, None, None, 0, L, None))
        return _fetch_topk(self._lib, self._h, B, L.value)

    host_nbest = staticmethod(host_nbest)

    def op_topk(self, x, K=4, V=None) -> TopkResult:
        """The pipeline's top-k kernel on caller data: x [rows, ld], the first V (default ld) entries of each row."""
        a = _f32(x)
        rows, ld = a.shape
        V = ld if V is None else V
        ids = np.zeros((rows, K), np.int64)
        val = np.zeros((rows, K), np.float32)
        n = np.zeros(rows, np.int32)
        N.check(self._lib.pf_op_topk(self._h, _fp(a), rows, V, ld, K, ids.ctypes.data_as(C.POINTER(C.c_int64)), _fp(val), _i32p(n)))
        return TopkResult(ids, val, n)

    def op_ctc_collapse(self, ids, scores, lens, blank=0, cap=None) -> CtcResult:
        """The pipeline's CTC collapse kernel on caller data: ids / scores [B, T], lens [B]."""
        y = np.ascontiguousarray(ids, dtype=np.int64)
        sc = _f32(scores)
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        B, T = y.shape
        cap = T if cap is None else cap
        n = np.zeros(B, np.int32)
        io = np.zeros((B, cap), np.int64)
        fo, lo = np.zeros((B, cap), np.int32), np.zeros((B, cap), np.int32)
        so = np.zeros((B, cap), np.float32)
        i64 = C.POINTER(C.c_int64)
        N.check(self._lib.pf_op_ctc_collapse(self._h, y.ctypes.data_as(i64), _fp(sc), _i32p(ln), B, T, blank,
                                             io.ctypes.data_as(i64), _i32p(fo), _i32p(lo), _fp(so), cap, _i32p(n)))
        return CtcResult(n, io, fo, lo, so)

    # ---- PCM intake: raw interleaved values in, converted on the device (include/paraformer_hip.h "PCM intake") ----
    @staticmethod
    def _pcm_args(pcm_list, descs):
        """pcm_list: per utterance bytes or a numpy array of the format's dtype; descs: one _native.PfPcmDesc for all, or a
        list of B.  -> (data pointers, value counts, desc array, n_descs, B, keep-alive)"""
        B = len(pcm_list)
        dl = [descs] if isinstance(descs, N.PfPcmDesc) else list(descs)
        assert len(dl) in (1, B), "one desc, or one per utterance"
        raws = [N.pcm_bytes(x, dl[0 if len(dl) == 1 else b].format) for b, x in enumerate(pcm_list)]
        ptrs = (C.c_void_p * max(B, 1))(*[r.ctypes.data if r.size else None for r, _n in raws])
        ns = (C.c_int64 * max(B, 1))(*[n for _r, n in raws])
        da = (N.PfPcmDesc * len(dl))(*dl)
        return ptrs, ns, da, len(dl), B, raws

    def pcm_num_samples(self, desc, n_values: int, fs: int = 16000) -> int:
        n = C.c_int64()
        N.check(self._lib.pf_pcm_num_samples(C.byref(desc), fs, n_values, C.byref(n)))
        return n.value

    def op_pcm_convert(self, data, desc) -> np.ndarray:
        """The pipeline's PCM intake kernel on caller data -> the float32 samples it hands to the fbank."""
        raw, n = N.pcm_bytes(data, desc.format)
        n_out = C.c_int64()
        N.check(self._lib.pf_op_pcm_convert(self._h, None if raw.size == 0 else raw.ctypes.data, n, C.byref(desc), None, 0, C.byref(n_out)))
        out = np.zeros(max(n_out.value, 1), np.float32)
        N.check(self._lib.pf_op_pcm_convert(self._h, raw.ctypes.data if raw.size else out.ctypes.data, n, C.byref(desc), _fp(out),
                                            out.size, C.byref(n_out)))
        return out[: n_out.value]

    def stage_pcm(self, pcm_list, descs):
        ptrs, ns, da, nd, B, _keep = self._pcm_args(pcm_list, descs)
        N.check(self._lib.pf_stage_pcm(self._h, ptrs, ns, da, nd, B))
        self._staged_B = B

    def recognize_pcm(self, pcm_list, descs, want_logits=False, hotwords=None) -> BatchResult:
        hp, hn, _keep_hw = self._hw(hotwords)
        ptrs, ns, da, nd, B, _keep = self._pcm_args(pcm_list, descs)
        dummy = np.zeros(1, np.float32)

        def call(out):
            if want_logits:
                out.logits = _fp(dummy)
                out.logits_cap = 1
            rc = self._lib.pf_recognize_pcm(self._h, ptrs, ns, da, nd, B, hp, hn, C.byref(out))
            return 0 if (want_logits and rc == N.PF_ERR_CAPACITY) else rc
        return self._collect(call, B, want_logits)

    @staticmethod
    def _hw(hotwords):
        """SeACo hotword ids [N,10] int32 (PadList output) -> (pointer, N); None -> (NULL, 0)."""
        if hotwords is None:
            return None, 0, None
        a = np.ascontiguousarray(hotwords, dtype=np.int32).reshape(-1, 10)
        return a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0], a

    def forward_feats(self, speech, want_logits=False, hotwords=None) -> BatchResult:
        sp = _f32(speech)
        B, T, _ = sp.shape
        hp, hn, _keep = self._hw(hotwords)
        if want_logits:
            # logits must be requested at forward time: pass a 1-float dummy capacity marker
            dummy = np.zeros(1, np.float32)

            def call(out):
                out.logits = _fp(dummy)
                out.logits_cap = 1
                rc = self._lib.pf_forward_feats(self._h, _fp(sp), B, T, hp, hn, C.byref(out))
                # capacity error on the dummy buffer is expected; L and V are filled in
                return 0 if rc == N.PF_ERR_CAPACITY else rc
        else:
            def call(out):
                return self._lib.pf_forward_feats(self._h, _fp(sp), B, T, hp, hn, C.byref(out))
        return self._collect(call, B, want_logits)

    def model_proj(self, speeches, want_logits=False, hotwords=None) -> BatchResult:
        hp, hn, _keep = self._hw(hotwords)
        arrs = [_f32(s).reshape(-1) for s in speeches]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        lens = (C.c_int32 * B)(*[a.shape[0] for a in arrs])
        dummy = np.zeros(1, np.float32)

        def call(out):
            if want_logits:
                out.logits = _fp(dummy)
                out.logits_cap = 1
            rc = self._lib.pf_model_proj(self._h, ptrs, lens, B, hp, hn, C.byref(out))
            return 0 if (want_logits and rc == N.PF_ERR_CAPACITY) else rc
        return self._collect(call, B, want_logits)

    def recognize(self, samples_list, want_logits=False, hotwords=None) -> BatchResult:
        hp, hn, _keep = self._hw(hotwords)
        arrs = [_f32(s) for s in samples_list]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        ns = (C.c_int64 * B)(*[a.shape[0] for a in arrs])
        dummy = np.zeros(1, np.float32)

        def call(out):
            if want_logits:
                out.logits = _fp(dummy)
                out.logits_cap = 1
            rc = self._lib.pf_recognize(self._h, ptrs, ns, B, hp, hn, C.byref(out))
            return 0 if (want_logits and rc == N.PF_ERR_CAPACITY) else rc
        return self._collect(call, B, want_logits)

    # split form (bench): audio resident in HBM before the timed region
    def stage_audio(self, samples_list):
        arrs = [_f32(s) for s in samples_list]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        ns = (C.c_int64 * B)(*[a.shape[0] for a in arrs])
        N.check(self._lib.pf_stage_audio(self._h, ptrs, ns, B))
        self._staged_B = B

    def set_hotwords(self, hotwords):
        """SeACo hotword ids [N,10] for the following run_staged() calls."""
        hp, hn, _keep = self._hw(hotwords)
        N.check(self._lib.pf_engine_set_hotwords(self._h, hp, hn))

    def run_staged(self):
        N.check(self._lib.pf_run_staged(self._h))

    def sync(self):
        N.check(self._lib.pf_sync(self._h))

    def fetch(self) -> BatchResult:
        return self._collect(lambda out: self._lib.pf_fetch(self._h, C.byref(out)), self._staged_B, False)

    def fetch_ids_device(self, dev_ptr: int, l_cap: int) -> int:
        """The staged result's ids [B, l_cap] int64 (-1 padded) into caller-owned DEVICE memory (e.g. a torch tensor's
        data_ptr on this engine's GPU) — what a multi-GPU caller hands to the RCCL all-gather.  Returns L."""
        L = C.c_int32(0)
        N.check(self._lib.pf_fetch_ids_device(self._h, C.c_void_p(dev_ptr), l_cap, C.byref(L)))
        return L.value

    def profile(self, on: bool):
        N.check(self._lib.pf_profile_enable(self._h, 1 if on else 0))

    def profile_select(self, cls: str = ""):
        N.check(self._lib.pf_profile_select(self._h, cls.encode()))

    def profile_reset(self):
        N.check(self._lib.pf_profile_reset(self._h))

    def profile_get(self, cls: str):
        ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
        N.check(self._lib.pf_profile_get(self._h, cls.encode(), ms, n, fpl))
        return ms.value, n.value, fpl.value

    def profile_kernel(self, cls: str) -> str:
        buf = C.create_string_buffer(256)
        N.check(self._lib.pf_profile_kernel(self._h, cls.encode(), buf, 256))
        return buf.value.decode()

    def last_flops(self) -> float:
        f = C.c_double()
        N.check(self._lib.pf_last_flops(self._h, f))
        return f.value

    # ---- stand-alone ops ------------------------------------------------------
    def op_lfr_cmvn_pad(self, fbanks, sentinel=True) -> np.ndarray:
        arrs = [_f32(f).reshape(-1, self.n_mels) for f in fbanks]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        t80 = (C.c_int32 * B)(*[a.shape[0] for a in arrs])
        tmax = max([a.shape[0] // self.lfr_n for a in arrs] + [0])
        out = np.zeros((B, tmax, self.lfr_m * self.n_mels), np.float32)
        tm = C.c_int32()
        N.check(self._lib.pf_op_lfr_cmvn_pad(self._h, ptrs, t80, B, 1 if sentinel else 0, _fp(out), out.size, tm))
        assert tm.value == tmax, (tm.value, tmax)
        return out

    def op_vad_levels(self, rows) -> np.ndarray:
        """The detector's level kernel on caller rows [T, n_mels] (pf_op_vad_levels) -> [T] int32."""
        x = _f32(rows)
        T, m = x.shape
        out = np.zeros(T, np.int32)
        N.check(self._lib.pf_op_vad_levels(self._h, _fp(x), T, m, _i32p(out)))
        return out

    def set_vad_model(self, model):
        """Attaches a VadModel (pf_engine_set_vad_model): vad_segment and everything built on it then score frames with the
        network instead of the energy level; None detaches."""
        N.check(self._lib.pf_engine_set_vad_model(self._h, None if model is None else model._h))
        self._vad_model = model

    def _op_vad_model(self, rows_list, want_logits):
        arrs = [_f32(r) for r in rows_list]
        B = len(arrs)
        m = arrs[0].shape[1] if B else 1
        assert all(a.ndim == 2 and a.shape[1] == m for a in arrs)
        T = np.ascontiguousarray([a.shape[0] for a in arrs] + [0] * (B == 0), dtype=np.int32)
        total = int(T.sum())
        x = np.ascontiguousarray(np.concatenate(arrs, axis=0) if B else np.zeros((0, m), np.float32))
        O = self._vad_model.dims["output_dim"] if self._vad_model is not None else 1     # (without a model the call is refused)
        if want_logits:
            out = np.zeros((max(total, 1), O), np.float32)
            N.check(self._lib.pf_op_vad_model_logits(self._h, _fp(x), _i32p(T), B, m, _fp(out)))
        else:
            out = np.zeros(max(total, 1), np.int32)
            N.check(self._lib.pf_op_vad_model_levels(self._h, _fp(x), _i32p(T), B, m, _i32p(out)))
        off = np.concatenate([[0], np.cumsum(T[:B])]).astype(np.int64)
        return [out[off[b]: off[b + 1]].copy() for b in range(B)]

    def op_vad_model_logits(self, rows_list) -> list:
        """The attached model's launches on caller rows (pf_op_vad_model_logits): ONE call over all the utterances of rows_list
        ([T_b, n_mels] each); returns each utterance's logits [T_b, output_dim] float32."""
        return self._op_vad_model(rows_list, True)

    def op_vad_model_levels(self, rows_list) -> list:
        """As op_vad_model_logits, the levels [T_b] int32 (pf_op_vad_model_levels)."""
        return self._op_vad_model(rows_list, False)

    def op_vad_model_stream(self, states, rows_list, flush=None, want_logits=True, cap=None, ld=None):
        """The attached model's streaming launch on caller state blocks and rows (pf_op_vad_model_stream): ONE launch over all
        the streams.  states [B, state_bytes] uint8 (vad_model_stream_state), updated in place; rows_list: each stream's new rows
        [n_new_b, n_mels] (any counts, may be empty); flush: per-stream flags.  Returns (levels per stream [n_out_b] int32,
        logits per stream [n_out_b, output_dim] float32 or None)."""
        model = self._vad_model
        if model is not None:
            m = model.dims["input_dim"] // model.dims["lfr_m"]
        else:                                                       # (without a model the call is refused)
            m = np.asarray(rows_list[0]).shape[-1] if len(rows_list) else 80
        arrs = [_f32(np.asarray(r, np.float32).reshape(-1, m)) for r in rows_list]
        B = len(arrs)
        assert isinstance(states, np.ndarray) and states.dtype == np.uint8 and states.flags.c_contiguous and states.shape[0] == B
        ld = max([a.shape[0] for a in arrs] + [1]) if ld is None else ld
        x = np.full((max(B, 1), ld, m), np.float32(3e38), np.float32)   # past n_new[b]: values that would change every answer if read
        for b, a in enumerate(arrs):
            x[b, : min(a.shape[0], ld)] = a[:ld]
        n_new = np.ascontiguousarray([a.shape[0] for a in arrs] + [0] * (B == 0), dtype=np.int32)
        fl = np.zeros(max(B, 1), np.int32)
        if flush is not None:
            fl[:B] = np.asarray(flush, dtype=bool).astype(np.int32)
        O = model.dims["output_dim"] if model is not None else 1
        cap = ld + (model.dims["lfr_m"] if model is not None else 0) if cap is None else cap
        lev = np.full((max(B, 1), max(cap, 1)), -77777, np.int32)
        z = np.full((max(B, 1), max(cap, 1), O), np.float32(-7e7), np.float32) if want_logits else None
        n = np.zeros(max(B, 1), np.int32)
        N.check(self._lib.pf_op_vad_model_stream(self._h, states.ctypes.data_as(C.c_void_p), _fp(x), _i32p(n_new), _i32p(fl), B, ld, m,
                                                 _i32p(lev), _fp(z) if want_logits else None, int(cap), _i32p(n)))
        return ([lev[b, : n[b]].copy() for b in range(B)], [z[b, : n[b]].copy() for b in range(B)] if want_logits else None)

    def set_spk_model(self, model):
        """Attaches a SpkModel (pf_engine_set_spk_model); None detaches and frees what the attach and its runs allocated."""
        N.check(self._lib.pf_engine_set_spk_model(self._h, None if model is None else model._h))
        self._spk_model = model

    def op_spk_embed(self, rows_list, want_frames=False):
        """The attached speaker model's launches on caller windows (pf_op_spk_embed): ONE call over all the windows of
        rows_list ([T_b, n_mels] each) -> embeddings [B, E] float32, and with want_frames also the list of the frames
        [ceil(T_b / 2), C] in front of the pooling."""
        arrs = [_f32(r).reshape(-1, np.shape(r)[1]) for r in rows_list]
        B = len(arrs)
        m = arrs[0].shape[1] if B else 1
        assert all(a.shape[1] == m for a in arrs)
        T = np.ascontiguousarray([a.shape[0] for a in arrs] + [0] * (B == 0), dtype=np.int32)
        x = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if B and int(T.sum()) else np.zeros((1, m), np.float32)
        d = self._spk_model.dims if self._spk_model is not None else {"embedding": 1, "frame_width": 1}   # (without a model the call is refused)
        emb = np.zeros((max(B, 1), d["embedding"]), np.float32)
        Tp = (T[:B] + 1) // 2
        fr = np.zeros((max(int(Tp.sum()), 1), d["frame_width"]), np.float32) if want_frames else None
        N.check(self._lib.pf_op_spk_embed(self._h, _fp(x), _i32p(T), B, m, _fp(emb), _fp(fr) if want_frames else None))
        if not want_frames:
            return emb[:B].copy()
        off = np.concatenate([[0], np.cumsum(Tp)]).astype(np.int64)
        return emb[:B].copy(), [fr[off[b]: off[b + 1]].copy() for b in range(B)]

    def op_spk_affinity(self, emb_list) -> list:
        """The cosine block of every stream of emb_list ([n_s, E] each) in ONE launch (pf_op_spk_affinity) -> [n_s, n_s] float32."""
        arrs = [_f32(e).reshape(-1, np.shape(e)[1]) for e in emb_list]
        S = len(arrs)
        E_ = arrs[0].shape[1] if S else 1
        n = np.ascontiguousarray([a.shape[0] for a in arrs] + [0] * (S == 0), dtype=np.int32)
        x = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if S and int(n.sum()) else np.zeros((1, E_), np.float32)
        cells = [int(k) * int(k) for k in n[:S]]
        out = np.zeros(max(sum(cells), 1), np.float32)
        N.check(self._lib.pf_op_spk_affinity(self._h, _fp(x), _i32p(n), S, E_, _fp(out)))
        off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        return [out[off[s]: off[s + 1]].reshape(int(n[s]), int(n[s])).copy() for s in range(S)]

    def set_punc_model(self, model):
        """Attaches a PuncModel (pf_engine_set_punc_model); None detaches and frees what the attach and its runs allocated."""
        N.check(self._lib.pf_engine_set_punc_model(self._h, None if model is None else model._h))
        self._punc_model = model

    @staticmethod
    def _punc_batch(ids_list):
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in ids_list]
        T = np.ascontiguousarray([a.size for a in arrs] + [0] * (len(arrs) == 0), dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate(arrs + [np.zeros(1, np.int32)]))       # (never empty: a valid pointer)
        off = np.concatenate([[0], np.cumsum(T[: len(arrs)])]).astype(np.int64)
        return arrs, T, ids, off

    def punctuate(self, ids_list):
        """The text loop on the device for the texts of ids_list, given as word ids (pf_engine_punctuate): ONE call, a forward per
        round.  Returns (each text's punc_ids int32, the number of rounds)."""
        arrs, T, ids, off = self._punc_batch(ids_list)
        out, rounds = np.zeros(ids.size, np.int32), C.c_int32()
        N.check(self._lib.pf_engine_punctuate(self._h, _i32p(ids), _i32p(T), len(arrs), _i32p(out), rounds))
        return [out[off[b]: off[b + 1]].copy() for b in range(len(arrs))], rounds.value

    def punctuate_text(self, texts):
        """Words on the host, the loop on the device, the assembly on the host: for every text (punctuated text, punc_ids,
        sentences as [one past the last word])."""
        m = self._punc_model
        ids = [host_punc_words(m, t)[0] for t in texts]
        p, _ = self.punctuate(ids)
        return [host_punc_assemble(m, t, p[i]) + (p[i],) for i, t in enumerate(texts)]

    def op_punc_logits(self, ids_list, want_x0=False, out=None):
        """The attached model's launches on caller windows (pf_op_punc_logits): ONE call over all windows of ids_list; returns
        each window's logits [T_b, n_punc] float32 (and layer 0's input [T_b, d_model] with want_x0).  out: a float32 buffer of
        at least sum T * n_punc values to store into (tests look at what lies beyond)."""
        arrs, T, ids, off = self._punc_batch(ids_list)
        dims = self._punc_model.dims if self._punc_model is not None else {}       # (without a model the call is refused)
        P, D = dims.get("n_punc", 1), dims.get("d_model", 1)
        total = int(off[-1])
        z = np.zeros(max(total, 1) * P, np.float32) if out is None else out
        x0 = np.zeros((max(total, 1), D), np.float32) if want_x0 else None
        N.check(self._lib.pf_op_punc_logits(self._h, _i32p(ids), _i32p(T), len(arrs), _fp(z), None if x0 is None else _fp(x0)))
        zs = [z[off[b] * P: off[b + 1] * P].reshape(-1, P).copy() for b in range(len(arrs))]
        if want_x0:
            return zs, [x0[off[b]: off[b + 1]].copy() for b in range(len(arrs))]
        return zs

    def op_punc_stream_step(self, states, ids_list, flush=None, max_context=PUNC_STREAM_DEFAULT_CONTEXT, flags=0, want_logits=True,
                            ld=None, out=None):
        """The attached causal model's streaming launch on caller state blocks and ids (pf_op_punc_stream_step): ONE launch over
        all the streams.  states [B, state_bytes] uint8 (punc_stream_state), updated in place; ids_list: each stream's new word
        ids (any counts, may be empty); flush: per-stream flags.  Returns per stream (marks [n_b], mark_flags [n_b]), the
        logits [n_b, n_punc] float32 or None, and flush_mark [B].  out: a dict that receives the raw output arrays (marks,
        mark_flags, logits, flush_mark) with their fill values behind every stream's n_new (tests look at what lies beyond)."""
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in ids_list]
        B = len(arrs)
        assert isinstance(states, np.ndarray) and states.dtype == np.uint8 and states.flags.c_contiguous and states.shape[0] == B
        ld = max([a.size for a in arrs] + [1]) if ld is None else ld
        x = np.full((max(B, 1), ld), 2 ** 30, np.int32)              # past n_new[b]: ids that would be refused or fault if read
        for b, a in enumerate(arrs):
            x[b, : min(a.size, ld)] = a[:ld]
        n_new = np.ascontiguousarray([a.size for a in arrs] + [0] * (B == 0), dtype=np.int32)
        fl = np.zeros(max(B, 1), np.int32)
        if flush is not None:
            fl[:B] = np.asarray(flush, dtype=bool).astype(np.int32)
        P = self._punc_model.dims["n_punc"] if self._punc_model is not None else 1      # (without a model the call is refused)
        mk = np.full((max(B, 1), ld), -77777, np.int32)
        mf = np.full((max(B, 1), ld), -77777, np.int32)
        z = np.full((max(B, 1), ld, P), np.float32(-7e7), np.float32) if want_logits else None
        fm = np.full(max(B, 1), -77777, np.int32)
        N.check(self._lib.pf_op_punc_stream_step(self._h, states.ctypes.data_as(C.c_void_p), _i32p(x), _i32p(n_new), _i32p(fl), B, ld,
                                                 int(max_context), int(flags), _i32p(mk), _i32p(mf), _fp(z) if want_logits else None,
                                                 _i32p(fm)))
        if out is not None:
            out.update(marks=mk, mark_flags=mf, logits=z, flush_mark=fm, n_new=n_new)
        return ([(mk[b, : n_new[b]].copy(), mf[b, : n_new[b]].copy()) for b in range(B)],
                [z[b, : n_new[b]].copy() for b in range(B)] if want_logits else None, fm[:B].copy())

    def op_punc_window(self, ids_list, last, want_logits=False):
        """As op_punc_logits with the cut launch behind it (pf_op_punc_window): last[b] marks a text's last window; returns
        (each window's p int32 after the edits, cut int32 [B]) and the logits with want_logits."""
        arrs, T, ids, off = self._punc_batch(ids_list)
        P = self._punc_model.dims["n_punc"] if self._punc_model is not None else 1      # (without a model the call is refused)
        total = int(off[-1])
        lst = np.ascontiguousarray([1 if x else 0 for x in last] + [0] * (len(arrs) == 0), dtype=np.int32)
        assert len(last) == len(arrs)
        p, cut = np.zeros(max(total, 1), np.int32), np.zeros(max(len(arrs), 1), np.int32)
        z = np.zeros((max(total, 1), P), np.float32) if want_logits else None
        N.check(self._lib.pf_op_punc_window(self._h, _i32p(ids), _i32p(T), _i32p(lst), len(arrs), _i32p(p), _i32p(cut),
                                            None if z is None else _fp(z)))
        ps = [p[off[b]: off[b + 1]].copy() for b in range(len(arrs))]
        if want_logits:
            return ps, cut[: len(arrs)].copy(), [z[off[b]: off[b + 1]].copy() for b in range(len(arrs))]
        return ps, cut[: len(arrs)].copy()

    def op_vad_segments(self, levels_list, n_mels=80, cfg=None, cap=None, ld=None):
        """The detector's segment kernel on caller levels (pf_op_vad_segments): ONE launch over all the utterances of
        levels_list (int32 arrays of any lengths, laid out as [B, ld]); returns each utterance's segments [n, 2].  cap: the
        capacity handed over (default: what always suffices); too small raises PfError(PF_ERR_CAPACITY) whose .n is n [B]."""
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in levels_list]
        B = len(arrs)
        ld = max([a.size for a in arrs] + [1]) if ld is None else ld
        lev = np.full((max(B, 1), ld), 0x7FFFFFFF, np.int32)      # past T[b]: values that would change every answer if read
        for b, a in enumerate(arrs):
            lev[b, : a.size] = a
        T = np.ascontiguousarray([a.size for a in arrs] + [0] * (B == 0), dtype=np.int32)
        cap = ld // 2 + 1 if cap is None else cap
        seg = np.full((max(B, 1), max(cap, 1), 2), -7, np.int32)
        n = np.zeros(max(B, 1), np.int32)
        rc = self._lib.pf_op_vad_segments(self._h, _i32p(lev), _i32p(T), B, ld, int(n_mels), _vad_cfg_ptr(cfg), _i32p(seg), int(cap), _i32p(n))
        if rc < 0:
            try:
                N.check(rc)
            except N.PfError as ex:
                ex.n, ex.seg = n[:B].copy(), seg[:B].copy()
                raise
        return [seg[b, : n[b]].copy() for b in range(B)]

    def op_endpoint_update(self, states, levels_list, flush=None, n_mels=80, cfg=None, cap=None, ld=None):
        """The streaming endpoint kernel on caller state blocks and levels (pf_op_endpoint_update): ONE launch over all the
        streams.  states [B, PF_ENDPOINT_STATE_INTS] int32, updated in place; levels_list: each stream's new levels (any
        lengths, may be empty); flush: per-stream flags.  Returns (events per stream [n, 3], in_speech [B], open_begin [B]).
        cap: the capacity handed over (default: what always suffices); too small raises PfError(PF_ERR_CAPACITY) whose .n is
        n_events [B] and .events the [B, cap, 3] block."""
        arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in levels_list]
        B = len(arrs)
        assert isinstance(states, np.ndarray) and states.dtype == np.int32 and states.flags.c_contiguous
        assert states.shape == (B, N.PF_ENDPOINT_STATE_INTS)
        ld = max([a.size for a in arrs] + [1]) if ld is None else ld
        lev = np.full((max(B, 1), ld), 0x7FFFFFFF, np.int32)      # past n_new[b]: values that would change every answer if read
        for b, a in enumerate(arrs):
            lev[b, : min(a.size, ld)] = a[:ld]                    # (an ld below a stream's count is for the entry point to refuse)
        n_new = np.ascontiguousarray([a.size for a in arrs] + [0] * (B == 0), dtype=np.int32)
        fl =np.zeros(max(B, 1), np.int32)
        if flush is not None:
            fl[:B] = np.asarray(flush, dtype=bool).astype(np.int32)
        cap = ld + 1 if cap is None else cap
        ev = np.full((max(B, 1), max(cap, 1), 3), -7, np.int32)
        n, ins, ob = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        rc = self._lib.pf_op_endpoint_update(self._h, _i32p(states), _i32p(lev), _i32p(n_new), _i32p(fl), B, ld, int(n_mels),
                                             _endpoint_cfg_ptr(cfg), _i32p(ev), int(cap), _i32p(n), _i32p(ins), _i32p(ob))
        if rc < 0:
            try:
                N.check(rc)
            except N.PfError as ex:
                ex.n, ex.events = n[:B].copy(), ev[:B].copy()
                raise
        return [ev[b, : n[b]].copy() for b in range(B)], ins[:B].copy(), ob[:B].copy()

    def vad_segment(self, samples_list, cfg=None, cap=None):
        """Voice-activity segmentation of whole streams on the device (pf_vad_segment): upload, the one batched fbank
        launch, the detector; returns each utterance's segments [n, 2] (10 ms frame pairs)."""
        arrs = [_f32(s) for s in samples_list]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * max(B, 1))(*[_fp(a) for a in arrs])
        ns = (C.c_int64 * max(B, 1))(*[a.shape[0] for a in arrs])
        cap = max([a.shape[0] // 320 + 2 for a in arrs] + [1]) if cap is None else cap
        seg = np.zeros((max(B, 1), max(cap, 1), 2), np.int32)
        n = np.zeros(max(B, 1), np.int32)
        N.check(self._lib.pf_vad_segment(self._h, ptrs, ns, B, _vad_cfg_ptr(cfg), _i32p(seg), int(cap), _i32p(n)))
        return [seg[b, : n[b]].copy() for b in range(B)]

    def op_fbank_batch(self, samples_list) -> list:
        """The batched fbank as run_staged launches it (pf_op_fbank_batch): one launch over all the utterances;
        returns each utterance's rows [t, n_mels]."""
        arrs = [_f32(s) for s in samples_list]
        B, m = len(arrs), self.n_mels
        ptrs = (C.POINTER(C.c_float) * B)(*[_fp(a) for a in arrs])
        ns = (C.c_int64 * B)(*[a.shape[0] for a in arrs])
        cap = sum(a.shape[0] // 160 + 2 for a in arrs) * m
        out = np.zeros(max(cap, 1), np.float32)
        t80 = np.zeros(max(B, 1), np.int32)
        N.check(self._lib.pf_op_fbank_batch(self._h, ptrs, ns, B, _fp(out), cap, _i32p(t80)))
        offs = np.concatenate([[0], np.cumsum(t80[:B], dtype=np.int64)])
        return [out[offs[b] * m: offs[b + 1] * m].reshape(int(t80[b]), m).copy() for b in range(B)]

    def op_qlinear(self, x, W, bias=None, relu=False, x_is_f16=False, details=False, f16_result=False):
        """One dynamically quantised Linear on the int8 MFMA (pf_op_qlinear).  details=True also returns the uint8
        activations, (x_scale, x_zp), the uint8 weights, w_scale and w_zp.  f16_result: through the f16-result kernel
        (QKV / FFN-up in the pipeline): y = float32 of the f16 values it stored; the call fails if the range the kernel's
        epilogue reports for the next quantiser differs from a min / max pass over its output."""
        x, W = _f32(x), _f32(W)
        rows, depth = x.shape
        cols = W.shape[0]
        y = np.zeros((rows, cols), np.float32)
        b = _f32(bias) if bias is not None else None
        xq = np.zeros((rows, depth), np.uint8)
        wq = np.zeros((cols, depth), np.uint8)
        ap = np.zeros(2, np.float32)
        ws = np.zeros(cols, np.float32)
        wz = np.zeros(cols, np.int32)
        u8 = C.POINTER(C.c_uint8)
        N.check(self._lib.pf_op_qlinear(self._h, _fp(x), _fp(W), _fp(b) if b is not None else None, rows, cols, depth,
                                        1 if relu else 0, (1 if x_is_f16 else 0) | (2 if f16_result else 0), _fp(y),
                                        xq.ctypes.data_as(u8), _fp(ap),
                                        wq.ctypes.data_as(u8), _fp(ws), wz.ctypes.data_as(C.POINTER(C.c_int32))))
        return (y, xq, (float(ap[0]), int(ap[1])), wq, ws, wz) if details else y

    def op_quantize(self, x, x_is_f16=False, ldx=None, ld=None, ln=None):
        """DynamicQuantizeLinear of x [rows, cols] (pf_op_quantize: the min / max pass and the quantise pass; ln = (gamma,
        beta): of LayerNorm(x), never stored) on a hostile host.  ldx: row stride of x on the device, ld: of the result.
        Returns (a' int8 [rows, ld] = code - 128 with the pad columns, which must be 0; rowsum int32 [rows]; (scale, zp))."""
        x = _f32(x)
        rows, cols = x.shape
        ldx, ld = ldx or cols, ld or cols
        g, b = (_f32(ln[0]), _f32(ln[1])) if ln is not None else (None, None)
        aq = np.zeros((rows, ld), np.int8)
        rs = np.zeros(rows, np.int32)
        par = np.zeros(2, np.float32)
        N.check(self._lib.pf_op_quantize(self._h, _fp(x), rows, cols, ldx, int(x_is_f16), ld, _fp(g) if g is not None else None,
                                         _fp(b) if b is not None else None, aq.ctypes.data_as(C.POINTER(C.c_int8)), _i32p(rs), _fp(par)))
        return aq, rs, (par[0], par[1])

    def _op_weight_out(self, rows, ld):
        return np.zeros((rows, ld), np.int8), np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.float32), np.zeros(rows, np.int32)

    def op_quantize_weight(self, W, ld=None):
        """quantize_weight_kernel + pack_dz on W [N, K] (pf_op_quantize_weight, hostile host).  Returns (w' int8 [N, ld] =
        code - 128, colsum, wzp = zp - 128, wscale, dz)."""
        W = _f32(W)
        rows, depth = W.shape
        w, cs, wz, ws, dz = self._op_weight_out(rows, ld or depth)
        N.check(self._lib.pf_op_quantize_weight(self._h, _fp(W), rows, depth, ld or depth, w.ctypes.data_as(C.POINTER(C.c_int8)), _i32p(cs),
                                                _i32p(wz), _fp(ws), _i32p(dz)))
        return w, cs, wz, ws, dz

    def op_import_weight(self, Q, zp, scale, ld=None):
        """import_weight_kernel + pack_dz on the stored bytes of an int8 export (pf_op_import_weight); returns as op_quantize_weight."""
        Q, zp, scale = np.ascontiguousarray(Q, np.uint8), np.ascontiguousarray(zp, np.uint8), _f32(scale)
        rows, depth = Q.shape
        w, cs, wz, ws, dz = self._op_weight_out(rows, ld or depth)
        u8 = C.POINTER(C.c_uint8)
        N.check(self._lib.pf_op_import_weight(self._h, Q.ctypes.data_as(u8), zp.ctypes.data_as(u8), _fp(scale), rows, depth, ld or depth,
                                              w.ctypes.data_as(C.POINTER(C.c_int8)), _i32p(cs), _i32p(wz), _fp(ws), _i32p(dz)))
        return w, cs, wz, ws, dz

    def op_qgemm_ex(self, a_codes, a_scale, a_zp, w_codes, w_zp, w_scale, bias=None, resid=None, add2=None, relu=False, scale_cols=0,
                    scale=1.0, out_kind=0, tile_rows=0, want_range=False, K_true=None):
        """The integer GEMM on codes and parameters as given (pf_op_qgemm_ex, hostile host).  out_kind 0 fp32 (resid aliases
        the result), 1 f16 through gemm_i8f_pp3, 2 f16 through gemm_i8_pp3's direct epilogue, 3 fp32 and f16 together.
        Returns (y32 or None, y16 widened or None, (min, max) or None)."""
        a, w = np.ascontiguousarray(a_codes, np.uint8), np.ascontiguousarray(w_codes, np.uint8)
        M, K = a.shape
        Nn = w.shape[0]
        assert w.shape[1] == K and (K_true is None or K_true == K)
        d = N.PfQgemmDesc()
        d.struct_size = C.sizeof(N.PfQgemmDesc)
        d.M, d.N, d.K = M, Nn, K
        d.relu, d.out_kind, d.tile_rows, d.want_range = int(relu), out_kind, tile_rows, int(want_range)
        d.scale_cols, d.scale, d.a_scale, d.a_zp = scale_cols, scale, float(a_scale), int(a_zp)
        wz, ws = np.ascontiguousarray(w_zp, np.int32), _f32(w_scale)
        assert wz.shape == (Nn,) and ws.shape == (Nn,)
        d.w_zp, d.w_scale = _i32p(wz), _fp(ws)
        keep = [_f32(t) if t is not None else None for t in (bias, resid, add2)]
        d.bias, d.resid, d.add2 = [_fp(t) if t is not None else None for t in keep]
        y32 = np.zeros((M, Nn), np.float32) if out_kind in (0, 3) else None
        y16 = np.zeros((M, Nn), np.float32) if out_kind != 0 else None
        rng = np.zeros(2, np.float32) if want_range else None
        u8 = C.POINTER(C.c_uint8)
        N.check(self._lib.pf_op_qgemm_ex(self._h, C.byref(d), a.ctypes.data_as(u8), w.ctypes.data_as(u8), _fp(y32) if y32 is not None else None,
                                         _fp(y16) if y16 is not None else None, _fp(rng) if rng is not None else None))
        return y32, y16, (float(rng[0]), float(rng[1])) if want_range else None

    def op_argmax(self, x) -> np.ndarray:
        a = _f32(x)
        V = a.shape[-1]
        rows = a.size // V if V else 0
        ids = np.zeros(rows, np.int64)
        N.check(self._lib.pf_op_argmax(self._h, _fp(a), rows, V, ids.ctypes.data_as(C.POINTER(C.c_int64))))
        return ids.reshape(a.shape[:-1])

    def op_gemm(self, A, W, bias=None, relu=False, f16_out=False) -> np.ndarray:
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        Nn = W.shape[0]
        out = np.zeros((M, Nn), np.float32)
        b = _f32(bias) if bias is not None else None
        N.check(self._lib.pf_op_gemm(self._h, _fp(A), _fp(W), _fp(b) if b is not None else None, M, Nn, K,
                                     2 if f16_out else (1 if relu else 0), _fp(out)))
        return out

    def op_gemm_ex(self, A, W, bias=None, resid=None, add2=None, relu=False, out_kind=0, a_blocked=False,
                   tile_rows=0, scale_cols=0, scale=1.0) -> np.ndarray:
        """The GEMM as the pipeline launches it (out_kind 0 fp32 / 1 f16 / 2 f16 blocked)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        Nn = W.shape[0]
        d = N.PfGemmDesc()
        d.struct_size = C.sizeof(N.PfGemmDesc)
        d.M, d.N, d.K = M, Nn, K
        d.relu, d.out_kind, d.a_blocked, d.tile_rows = int(relu), out_kind, int(a_blocked), tile_rows
        d.scale_cols, d.scale = scale_cols, scale
        keep = [_f32(t) if t is not None else None for t in (bias, resid, add2)]
        d.bias, d.resid, d.add2 = [_fp(t) if t is not None else None for t in keep]
        out = np.zeros((M, Nn), np.float32)
        N.check(self._lib.pf_op_gemm_ex(self._h, C.byref(d), _fp(A), _fp(W), _fp(out)))
        return out

    def op_gemm_panel(self, A, W, bias=None, f16_out=False, form=7, padded=False) -> np.ndarray:
        """A [M,512] W [N,512]^T + bias on the panel-resident kernel (form 7), gemm_f16_pp3 (1 / 2) or by the rule (0)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        Nn = W.shape[0]
        assert K == 512 and W.shape[1] == 512
        b = _f32(bias) if bias is not None else None
        out = np.zeros((M, Nn), np.float32)
        N.check(self._lib.pf_op_gemm_panel(self._h, M, Nn, int(f16_out), form, int(padded), _fp(b) if b is not None else None,
                                           _fp(A), _fp(W), _fp(out)))
        return out

    def op_gemm_rc(self, A, W, bias=None, resid=None, fsmn_v=None, fsmn_w=None, T=0, ln=None, a_blocked=False,
                   want_x=True, want_n16=True, want_n32=True, short_input=False):
        """Row-complete GEMM (N = 512) + fused epilogue; returns (x, n16, n32) (n* = None without `ln`).
        short_input: the short-input kernels of the same graph nodes (k_gemm_small.hip)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        d = N.PfGemmRcDesc()
        d.struct_size = C.sizeof(N.PfGemmRcDesc)
        d.M, d.K, d.a_blocked, d.T = M, K, int(a_blocked), T
        d.short_input = int(short_input)
        d.split_k = 0
        keep = [_f32(t) if t is not None else None for t in (bias, resid, fsmn_v, fsmn_w)]
        d.bias, d.resid, d.fsmn_v, d.fsmn_w = [_fp(t) if t is not None else None for t in keep]
        d.fsmn_k = keep[3].shape[1] if keep[3] is not None else 0
        g = b = None
        if ln is not None:
            g, b = _f32(ln[0]), _f32(ln[1])
            d.ln_gamma, d.ln_beta = _fp(g), _fp(b)
        x = np.zeros((M, 512), np.float32) if (want_x or ln is None) else None
        n16 = np.zeros((M, 512), np.float32) if (ln is not None and want_n16) else None
        n32 = np.zeros((M, 512), np.float32) if (ln is not None and want_n32) else None
        N.check(self._lib.pf_op_gemm_rc(self._h, C.byref(d), _fp(A), _fp(W), _fp(x) if x is not None else None,
                                        _fp(n16) if n16 is not None else None, _fp(n32) if n32 is not None else None))
        return x, n16, n32

    def op_qkv_attention(self, x, w, bias, B, T):
        """Fused Q | K | V projection (persistent 256 x 192 kernel: Q, K blocked, V row-major) + self-attention on that
        layout, as the encoder launches them for long inputs; x [B*T, K], w [1536, K]; returns (q, k, v, ctx) [B*T, 512]."""
        x, w = _f32(x), _f32(w)
        M, K = x.shape
        assert M == B * T and w.shape == (1536, K)
        bias = _f32(bias) if bias is not None else None
        outs = [np.zeros((M, 512), np.float32) for _ in range(4)]
        N.check(self._lib.pf_op_qkv_attention(self._h, _fp(x), _fp(w), _fp(bias) if bias is not None else None, B, T, K,
                                              *[_fp(o) for o in outs]))
        return tuple(outs)

    def op_ffn(self, x, w1, b1, w2, b2, resid) -> np.ndarray:
        x, w1, b1, w2, b2, resid = map(_f32, (x, w1, b1, w2, b2, resid))
        M, D = x.shape
        F = w1.shape[0]
        y = np.zeros((M, D), np.float32)
        N.check(self._lib.pf_op_ffn(self._h, _fp(x), _fp(w1), _fp(b1), _fp(w2), _fp(b2), _fp(resid), M, D, F, _fp(y)))
        return y

    def op_ffn_fused(self, x, w1, b1, w2, b2, resid=None, ln=None):
        """The encoder FFN block as ONE launch (k_ffn.hip): returns (x_out, n16_out or None);
        ln = (gamma, beta) of the LayerNorm that follows."""
        x, w1, b1, w2, b2 = map(_f32, (x, w1, b1, w2, b2))
        M, D = x.shape
        assert D == 512 and w1.shape == (2048, 512) and w2.shape == (512, 2048)
        resid = _f32(resid) if resid is not None else None
        g = _f32(ln[0]) if ln is not None else None
        be = _f32(ln[1]) if ln is not None else None
        xo = np.zeros((M, D), np.float32)
        no = np.zeros((M, D), np.float32) if ln is not None else None
        N.check(self._lib.pf_op_ffn_fused(self._h, _fp(x), _fp(w1), _fp(b1), _fp(w2), _fp(b2),
                                          _fp(resid) if resid is not None else None, _fp(g) if g is not None else None,
                                          _fp(be) if be is not None else None, M, _fp(xo), _fp(no) if no is not None else None))
        return xo, no

    def op_dec_ffn_fused(self, x, w1, b1, ln_hidden, w2, ln=None, splits=0, out_proj=None):
        """The decoder's FFN block (LayerNorm over the 2048 hidden columns between the products, w2 without bias) in the split
        form of the fused kernel (k_ffn.hip): returns (t, LayerNorm(t; ln) or None).  x = the block's normalised input;
        ln_hidden = (gamma, beta) [2048]; splits: 0 = the pipeline's choice for the row count, or 1 | 2 | 3 | 4 | 8.
        out_proj = (ctx, wo, bo, resid, (g1, b1)): the previous layer's cross-attention out-projection in front of the block
        in the same launch (x is ignored): returns (t, n, x_out) with x_out = resid + ctx wo^T + bo, the block's input =
        LayerNorm(x_out; g1, b1)."""
        arrs = dict(w1=_f32(w1), b1=_f32(b1), gamma_f=_f32(ln_hidden[0]), beta_f=_f32(ln_hidden[1]), w2=_f32(w2))
        if out_proj is None:
            arrs["x"] = _f32(x)
            M = arrs["x"].shape[0]
        else:
            ctx, wo, bo, resid, ln1 = out_proj
            arrs.update(ctx=_f32(ctx), wo=_f32(wo), bo=_f32(bo), resid=_f32(resid), ln1_gamma=_f32(ln1[0]), ln1_beta=_f32(ln1[1]))
            M = arrs["ctx"].shape[0]
        assert arrs["w1"].shape == (2048, 512) and arrs["w2"].shape == (512, 2048) and arrs["gamma_f"].shape == (2048,)
        if ln is not None:
            arrs["ln_gamma"], arrs["ln_beta"] = _f32(ln[0]), _f32(ln[1])
        d = N.PfDecFfnDesc()
        d.struct_size, d.M, d.splits = C.sizeof(N.PfDecFfnDesc), M, int(splits)
        for k, a in arrs.items():
            setattr(d, k, _fp(a))
        t = np.zeros((M, 512), np.float32)
        n = np.zeros((M, 512), np.float32) if ln is not None else None
        xo = np.zeros((M, 512), np.float32) if out_proj is not None else None
        N.check(self._lib.pf_op_dec_ffn_fused(self._h, C.byref(d), _fp(t), _fp(n) if n is not None else None,
                                              _fp(xo) if xo is not None else None))
        return (t, n, xo) if out_proj is not None else (t, n)

    def op_attn_ffn_fused(self, ctx, wo, bo, v, fsmn_w, T, ln2, w1, b1, w2, b2, resid=None, ln=None, qkv=None):
        """Out-projection + FSMN + norm2 + the FFN block + the next LayerNorm as the ONE launch the pipeline runs
        (k_ffn.hip, OP = 1): returns (x_out, n16_out or None); with qkv = (wqkv [1536,512], bqkv) also the next layer's
        Q | K | V projection in the same launch: returns (x_out, n16_out, q, k, v)."""
        arrs = {k: _f32(a) for k, a in dict(ctx=ctx, wo=wo, bo=bo, v=v, fsmn_w=fsmn_w, ln2_gamma=ln2[0], ln2_beta=ln2[1],
                                             w1=w1, b1=b1, w2=w2, b2=b2).items()}
        if resid is not None:
            arrs["resid"] = _f32(resid)
        if ln is not None:
            arrs["ln_gamma"], arrs["ln_beta"] = _f32(ln[0]), _f32(ln[1])
        M = arrs["ctx"].shape[0]
        d = N.PfAttnFfnDesc()
        d.struct_size, d.M, d.T = C.sizeof(N.PfAttnFfnDesc), M, T
        for k, a in arrs.items():
            setattr(d, k, _fp(a))
        xo = np.zeros((M, 512), np.float32)
        no = np.zeros((M, 512), np.float32) if ln is not None else None
        outs = []
        if qkv is not None:
            keep = (_f32(qkv[0]), _f32(qkv[1]))
            d.wqkv, d.bqkv = _fp(keep[0]), _fp(keep[1])
            outs = [np.zeros((M, 512), np.float32) for _ in range(3)]
            d.q_out, d.k_out, d.v_out = [_fp(o) for o in outs]
        N.check(self._lib.pf_op_attn_ffn_fused(self._h, C.byref(d), _fp(xo), _fp(no) if no is not None else None))
        return (xo, no, *outs) if outs else (xo, no)

    def op_fsmn_enc(self, v, w) -> np.ndarray:
        v, w = _f32(v), _f32(w)
        B, T, D = v.shape
        y = np.zeros_like(v)
        N.check(self._lib.pf_op_fsmn_enc(self._h, _fp(v), _fp(w), B, T, D, w.shape[1], _fp(y)))
        return y

    def op_linear32(self, x, W, bias=None, resid=None, relu=False) -> np.ndarray:
        """A Linear of the fp32 graph as math_mode 1 / 3 runs it (pf_op_linear32)."""
        x, W = _f32(x), _f32(W)
        M, K = x.shape
        Nn = W.shape[0]
        b = _f32(bias) if bias is not None else None
        r = _f32(resid) if resid is not None else None
        y = np.zeros((M, Nn), np.float32)
        N.check(self._lib.pf_op_linear32(self._h, _fp(x), _fp(W), _fp(b) if b is not None else None,
                                         _fp(r) if r is not None else None, M, Nn, K, 1 if relu else 0, _fp(y)))
        return y

    def op_ffn32(self, x, W1, b1, W2, b2) -> np.ndarray:
        """x + relu(x W1^T + b1) W2^T + b2 as math_mode 1 / 3 runs the FFN block (pf_op_ffn32)."""
        x, W1, b1, W2, b2 = _f32(x), _f32(W1), _f32(b1), _f32(W2), _f32(b2)
        M, D = x.shape
        F = W1.shape[0]
        y = np.zeros((M, D), np.float32)
        N.check(self._lib.pf_op_ffn32(self._h, _fp(x), _fp(W1), _fp(b1), _fp(W2), _fp(b2), M, D, F, _fp(y)))
        return y

    def op_linear32_ex(self, A, W, bias=None, resid=None, resid2=None, relu=False, scale_cols=0, scale=1.0, lda=0, ldw=0, ldc=0, ldr=0,
                       resid_aliases_out=False, flags=0) -> np.ndarray:
        """Engine::gemm32 on a hostile host with every argument selectable (pf_op_linear32_ex)."""
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        Nn = W.shape[0]
        d = N.PfLinear32Desc()
        d.struct_size = C.sizeof(N.PfLinear32Desc)
        d.M, d.N, d.K = M, Nn, K
        d.lda, d.ldw, d.ldc, d.ldr = lda, ldw, ldc, ldr
        d.resid_aliases_out, d.relu, d.scale_cols, d.scale, d.flags = int(resid_aliases_out), int(relu), scale_cols, scale, flags
        keep = [_f32(t) if t is not None else None for t in (bias, resid, resid2)]
        d.bias, d.resid, d.resid2 = [_fp(t) if t is not None else None for t in keep]
        out = np.zeros((M, Nn), np.float32)
        N.check(self._lib.pf_op_linear32_ex(self._h, C.byref(d), _fp(A), _fp(W), _fp(out)))
        return out

    def op_split_x3(self, x, Kp, ldx=0, ldo=0, swap=0) -> np.ndarray:
        """split_x3_kernel alone: the [rows, ldo] uint16 image of the pair buffer, pre-filled with 0x7E5A (pf_op_split_x3)."""
        x = _f32(x)
        rows, K = x.shape
        ldx, ldo = ldx or K, ldo or 2 * Kp
        out = np.zeros((rows, ldo), np.uint16)
        N.check(self._lib.pf_op_split_x3(self._h, _fp(x), rows, K, ldx, ldo, Kp, swap, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def op_layernorm32(self, x, gamma, beta, direct_pair=False, W=None, bias=None):
        """Engine::layernorm32 (pf_op_layernorm32): (out32 or None, (hi, lo') float16 or None, y or None)."""
        x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
        M, D = x.shape
        out32 = np.zeros((M, D), np.float32)
        pair = np.zeros((M, 2 * D), np.uint16)
        wrote = C.c_int32(0)
        Wk = _f32(W) if W is not None else None
        bk = _f32(bias) if bias is not None else None
        Nn = Wk.shape[0] if Wk is not None else 0
        y = np.zeros((M, max(Nn, 1)), np.float32)
        N.check(self._lib.pf_op_layernorm32(self._h, _fp(x), _fp(gamma), _fp(beta), M, D, int(direct_pair), _fp(out32),
                                            pair.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(wrote),
                                            _fp(Wk) if Wk is not None else None, _fp(bk) if bk is not None else None, Nn, _fp(y)))
        hl = (pair[:, :D].view(np.float16), pair[:, D:].view(np.float16)) if wrote.value else None
        return (None if wrote.value else out32), hl, (y if Wk is not None else None)

    def op_ffn32_ex(self, x, W1, b1, W2, b2, hidden_scale=1.0):
        """pf_op_ffn32 on a hostile host, the hidden optionally scaled (pf_op_ffn32_ex): (y, (hi, lo') of the hidden or None)."""
        x, W1, b1, W2, b2 = _f32(x), _f32(W1), _f32(b1), _f32(W2), _f32(b2)
        M, D = x.shape
        F = W1.shape[0]
        y = np.zeros((M, D), np.float32)
        pair = np.zeros((M, 2 * F), np.uint16)
        wrote = C.c_int32(0)
        N.check(self._lib.pf_op_ffn32_ex(self._h, _fp(x), _fp(W1), _fp(b1), _fp(W2), _fp(b2), M, D, F, hidden_scale, _fp(y),
                                         pair.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(wrote)))
        return y, ((pair[:, :F].view(np.float16), pair[:, F:].view(np.float16)) if wrote.value else None)

    def op_qkv32(self, x, W, bias, qscale) -> np.ndarray:
        """Q, K and V of the fp32 graph as three Linears on one operand (pf_op_qkv32): [M, 3 D]."""
        x, W, bias = _f32(x), _f32(W), _f32(bias)
        M, K = x.shape
        D = W.shape[0] // 3
        out = np.zeros((M, 3 * D), np.float32)
        N.check(self._lib.pf_op_qkv32(self._h, _fp(x), _fp(W), _fp(bias), M, D, K, qscale, _fp(out)))
        return out

    def op_fsmn_dec(self, tn, w, token_num, x) -> np.ndarray:
        tn, w, x = _f32(tn), _f32(w), _f32(x).copy()
        B, L, D = tn.shape
        t = np.ascontiguousarray(token_num, dtype=np.int32)
        N.check(self._lib.pf_op_fsmn_dec(self._h, _fp(tn), _fp(w), t.ctypes.data_as(C.POINTER(C.c_int32)), B, L, D,
                                         w.shape[1], _fp(x)))
        return x

    def op_fsmn_dec_ln(self, tn, taps, token_num, x, ln):
        """The fused decoder FSMN + LayerNorm kernel alone (pf_op_fsmn_dec_ln): tn, x [B, L, 512], taps [k, 512] (k = 11 | 21),
        ln = (gamma, beta); returns (x_out, xn16)."""
        tn, taps, x, g, b = _f32(tn), _f32(taps), _f32(x), _f32(ln[0]), _f32(ln[1])
        B, L, D = tn.shape
        assert D == 512 and x.shape == tn.shape and taps.shape[1] == 512
        t = np.ascontiguousarray(token_num, dtype=np.int32)
        assert t.shape == (B,)
        xo, xn = np.zeros_like(x), np.zeros_like(x)
        N.check(self._lib.pf_op_fsmn_dec_ln(self._h, _fp(tn), _fp(taps), t.ctypes.data_as(C.POINTER(C.c_int32)), B, L, taps.shape[0],
                                            _fp(x), _fp(g), _fp(b), _fp(xo), _fp(xn)))
        return xo, xn

    # ---- the row kernels alone.  Every result is the WHOLE guarded buffer of the C ABI: OP_GUARD_ROWS canary rows, the result,
    # OP_GUARD_ROWS canary rows, each row as wide as its row stride; f16 results are uint16 bit patterns.
    OP_GUARD_ROWS = 2
    OP_CANARY32 = 0x7FC5A5A5
    OP_CANARY16 = 0x7E5A

    def op_layernorm_ex(self, x, gamma, beta, want16=True, want32=True, ld16=0, ld32=0, posenc_T=0):
        """launch_layernorm on x [rows, D] (pf_op_layernorm_ex), or with posenc_T launch_posenc_ln_tab on x [B, posenc_T, D];
        returns (out16 [rows + 4, ld16] uint16 | None, out32 [rows + 4, ld32] float32 | None)."""
        x, g, b = _f32(x), _f32(gamma), _f32(beta)
        D = x.shape[-1]
        rows = x.size // D
        ld16, ld32 = ld16 or D, ld32 or D
        G = self.OP_GUARD_ROWS
        o16 = np.zeros((rows + 2 * G, ld16), np.uint16) if want16 else None
        o32 = np.zeros((rows + 2 * G, ld32), np.float32) if want32 else None
        N.check(self._lib.pf_op_layernorm_ex(self._h, _fp(x), _fp(g), _fp(b), rows, D, ld16, ld32, posenc_T,
                                             o16.ctypes.data_as(C.POINTER(C.c_uint16)) if want16 else None, _fp(o32) if want32 else None))
        return o16, o32

    def op_layernorm_f16(self, x16, gamma, beta, in_place=True) -> np.ndarray:
        """launch_layernorm_f16 on x16 [rows, D] float16 (pf_op_layernorm_f16): [rows + 4, D] uint16."""
        x = np.ascontiguousarray(x16, dtype=np.float16)
        g, b = _f32(gamma), _f32(beta)
        rows, D = x.shape
        out = np.zeros((rows + 2 * self.OP_GUARD_ROWS, D), np.uint16)
        N.check(self._lib.pf_op_layernorm_f16(self._h, x.view(np.uint16).ctypes.data_as(C.POINTER(C.c_uint16)), _fp(g), _fp(b), rows, D,
                                              1 if in_place else 0, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def op_fsmn_dec_stream(self, tn, taps, lens, cache_in, x):
        """launch_fsmn_dec_stream (pf_op_fsmn_dec_stream): tn, x [B, L, D], taps [k, D], cache_in [B, D, k - 1];
        returns (x [B L + 4, D], cache_out [B D + 4, k - 1])."""
        tn, taps, cin, x = _f32(tn), _f32(taps), _f32(cache_in), _f32(x)
        B, L, D = tn.shape
        k = taps.shape[0]
        assert x.shape == tn.shape and taps.shape == (k, D) and cin.shape == (B, D, k - 1)
        t = np.ascontiguousarray(lens, dtype=np.int32)
        assert t.shape == (B,)
        G = self.OP_GUARD_ROWS
        xo, co = np.zeros((B * L + 2 * G, D), np.float32), np.zeros((B * D + 2 * G, k - 1), np.float32)
        N.check(self._lib.pf_op_fsmn_dec_stream(self._h, _fp(tn), _fp(taps), t.ctypes.data_as(C.POINTER(C.c_int32)), _fp(cin), B, L, D, k,
                                                _fp(x), _fp(xo), _fp(co)))
        return xo, co

    def op_fsmn_enc_ex(self, v16, taps, ldv=0, col=0) -> np.ndarray:
        """launch_fsmn_enc (pf_op_fsmn_enc_ex): v16 [B, T, D] float16, taps [k, D]; on the device V is columns [col, col + D) of
        rows of ldv cells (0 = D) amid a large finite pattern; returns y [B T + 4, D] float32."""
        v = np.ascontiguousarray(v16, dtype=np.float16)
        taps = _f32(taps)
        B, T, D = v.shape
        k = taps.shape[0]
        assert taps.shape == (k, D)
        y = np.zeros((B * T + 2 * self.OP_GUARD_ROWS, D), np.float32)
        N.check(self._lib.pf_op_fsmn_enc_ex(self._h, v.view(np.uint16).ctypes.data_as(C.POINTER(C.c_uint16)), _fp(taps), B, T, D, k,
                                            ldv or D, col, _fp(y)))
        return y

    def op_fsmn_f32_ex(self, v, taps, mask=None, ldv=0, col=0, form=0) -> np.ndarray:
        """launch_fsmn_f32 / launch_fsmn_f32_ld (pf_op_fsmn_f32_ex): v [B, T, D], taps [k, D], mask [B, T] floats or None; form 0 =
        the launcher's choice, 1 = fsmn_f32_kernel<0> forced, 2 = in place (refused); returns y [B T + 4, D]."""
        v, taps = _f32(v), _f32(taps)
        B, T, D = v.shape
        k = taps.shape[0]
        assert taps.shape == (k, D)
        m = None if mask is None else _f32(mask)
        assert m is None or m.shape == (B, T)
        y = np.zeros((B * T + 2 * self.OP_GUARD_ROWS, D), np.float32)
        N.check(self._lib.pf_op_fsmn_f32_ex(self._h, _fp(v), _fp(taps), None if m is None else _fp(m), B, T, D, k, ldv or D, col, form,
                                            _fp(y)))
        return y

    def op_fsmn_dec_ex(self, tn, taps, token_num, x, hostile=0) -> np.ndarray:
        """launch_fsmn_dec (pf_op_fsmn_dec_ex): tn, x [B, L, D], taps [k, D] (any k); the masked rows of tn hold a large finite
        pattern (hostile 0), NaN (1) or Inf (2) on the device; returns x [B L + 4, D]."""
        tn, taps, x = _f32(tn), _f32(taps), _f32(x)
        B, L, D = tn.shape
        k = taps.shape[0]
        assert x.shape == tn.shape and taps.shape == (k, D)
        t = np.ascontiguousarray(token_num, dtype=np.int32)
        assert t.shape == (B,)
        xo = np.zeros((B * L + 2 * self.OP_GUARD_ROWS, D), np.float32)
        N.check(self._lib.pf_op_fsmn_dec_ex(self._h, _fp(tn), _fp(taps), t.ctypes.data_as(C.POINTER(C.c_int32)), B, L, D, k, hostile,
                                            _fp(x), _fp(xo)))
        return xo

    def op_embed_gather(self, table, ids, want16=True):
        """launch_embed_gather (pf_op_embed_gather): (out32 [rows + 4, D], out16 [rows + 4, D] uint16 | None)."""
        table = _f32(table)
        vocab, D = table.shape
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        G = self.OP_GUARD_ROWS
        o32 = np.zeros((i.size + 2 * G, D), np.float32)
        o16 = np.zeros((i.size + 2 * G, D), np.uint16) if want16 else None
        N.check(self._lib.pf_op_embed_gather(self._h, _fp(table), i.ctypes.data_as(C.POINTER(C.c_int32)), i.size, D, vocab, _fp(o32),
                                             o16.ctypes.data_as(C.POINTER(C.c_uint16)) if want16 else None))
        return o32, o16

    def op_add_to_f16(self, a, b) -> np.ndarray:
        """launch_add_to_f16 (pf_op_add_to_f16): [rows + 4, D] uint16."""
        a, b = _f32(a), _f32(b)
        rows, D = a.shape
        assert b.shape == a.shape
        out = np.zeros((rows + 2 * self.OP_GUARD_ROWS, D), np.uint16)
        N.check(self._lib.pf_op_add_to_f16(self._h, _fp(a), _fp(b), rows, D, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def op_seaco_merge(self, dha, dha_ids, V, nobias, copy_logits, logits, ids):
        """launch_seaco_merge (pf_op_seaco_merge): dha [rows, ld_dha], logits [rows, ld_logits] (both wider than V), dha_ids / ids
        [rows] int64; returns (logits [rows + 4, ld_logits], ids [rows + 4] uint64: the guards hold the canary twice)."""
        dha, logits = _f32(dha), _f32(logits)
        rows = dha.shape[0]
        di, ii = np.ascontiguousarray(dha_ids, dtype=np.int64), np.ascontiguousarray(ids, dtype=np.int64)
        assert logits.shape[0] == rows and di.shape == (rows,) and ii.shape == (rows,)
        G = self.OP_GUARD_ROWS
        lo, io = np.zeros((rows + 2 * G, logits.shape[1]), np.float32), np.zeros(rows + 2 * G, np.int64)
        p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        N.check(self._lib.pf_op_seaco_merge(self._h, _fp(dha), dha.shape[1], p64(di), rows, V, nobias, 1 if copy_logits else 0, _fp(logits),
                                            logits.shape[1], p64(ii), _fp(lo), p64(io)))
        return lo, io.view(np.uint64)

    def short_input_max_rows(self) -> int:
        """rows up to which the encoder takes its short-input kernels (pf_op_short_input_max_rows)."""
        v = C.c_int32(0)
        N.check(self._lib.pf_op_short_input_max_rows(self._h, C.byref(v)))
        return int(v.value)

    def op_dec_mid(self, a, w1, b1, ln_hidden, w2, n2, taps, token_num, x, n3, wq, bq, splits=0, form=0):
        """The middle of a decoder layer (pf_op_dec_mid): form 0 = the split block without its finishing pass + the fused
        middle kernel (k_decmid.hip), 1 = finishing pass with norm2 | fused FSMN + norm3 | q GEMM, 2 = the same with the FSMN
        and the LayerNorm as two launches.  a [B L, 512], x [B, L, 512], taps [11, 512], n2 / n3 / ln_hidden = (gamma, beta).
        Returns dict(x, q, tn, xn16, ran): tn / xn16 are None in form 0; ran False = form 0 declined (x, q are None)."""
        x = _f32(x)
        B, L, D = x.shape
        arrs = dict(a=_f32(a), w1=_f32(w1), b1=_f32(b1), gamma_f=_f32(ln_hidden[0]), beta_f=_f32(ln_hidden[1]), w2=_f32(w2),
                    n2_gamma=_f32(n2[0]), n2_beta=_f32(n2[1]), taps=_f32(taps), x=x, n3_gamma=_f32(n3[0]), n3_beta=_f32(n3[1]),
                    wq=_f32(wq), bq=_f32(bq))
        assert arrs["a"].shape == (B * L, 512) and arrs["taps"].shape == (11, 512) and arrs["wq"].shape == (512, 512)
        t = np.ascontiguousarray(token_num, dtype=np.int32)
        assert t.shape == (B,)
        d = N.PfDecMidDesc()
        d.struct_size, d.B, d.L, d.splits, d.form = C.sizeof(N.PfDecMidDesc), B, L, int(splits), int(form)
        for k, v in arrs.items():
            setattr(d, k, _fp(v))
        d.token_num = t.ctypes.data_as(C.POINTER(C.c_int32))
        xo, q = np.zeros((B * L, 512), np.float32), np.zeros((B * L, 512), np.float32)
        tn = np.zeros((B * L, 512), np.float32) if form else None
        xn = np.zeros((B * L, 512), np.float32) if form else None
        ran = C.c_int32(0)
        N.check(self._lib.pf_op_dec_mid(self._h, C.byref(d), _fp(xo), _fp(q), _fp(tn) if form else None, _fp(xn) if form else None,
                                        C.byref(ran)))
        if not ran.value:
            return dict(x=None, q=None, tn=None, xn16=None, ran=False)
        return dict(x=xo, q=q, tn=tn, xn16=xn, ran=True)

    def op_lstm(self, xg, whh, ndir, form) -> np.ndarray:
        """The heads' LSTM recurrence on gate inputs xg [B, T3, ndir * 4D], whh [ndir, 4D, D] (pf_op_lstm): form 0 = as the f16
        timestamp head chooses, 1 = per-step launches, 2 = f16 ring, 3 = pair-operand ring, 4 = fp32 per step."""
        xg, whh = _f32(xg), _f32(whh)
        B, T3, G = xg.shape
        D = whh.shape[2]
        assert whh.shape == (ndir, 4 * D, D) and G == ndir * 4 * D, (xg.shape, whh.shape, ndir)
        hout = np.zeros((B, T3, ndir * D), np.float32)
        N.check(self._lib.pf_op_lstm(self._h, _fp(xg), _fp(whh), B, T3, D, ndir, form, _fp(hout)))
        return hout

    def op_us_peak(self, hout, w, b0, smooth, noise, token_num, thr):
        """launch_us_alpha + launch_us_peak as the timestamp heads run them (pf_op_us_peak): (alphas_raw, alphas, peak) [B, T3]."""
        hout, w = _f32(hout), _f32(w).reshape(-1)
        B, T3, Wd = hout.shape
        assert w.size == Wd
        b = np.asarray([b0], np.float32).reshape(1)
        t = np.ascontiguousarray(token_num, dtype=np.int32)
        assert t.shape == (B,)
        outs = [np.zeros((B, T3), np.float32) for _ in range(3)]
        N.check(self._lib.pf_op_us_peak(self._h, _fp(hout), _fp(w), _fp(b), float(smooth), float(noise),
                                        t.ctypes.data_as(C.POINTER(C.c_int32)), float(thr), B, T3, Wd, *[_fp(o) for o in outs]))
        return tuple(outs)

    def op_logsoftmax_argmax(self, x, store=True):
        a = _f32(x)
        V = a.shape[-1]
        rows = a.size // V
        ids = np.zeros(rows, np.int64)
        y = np.zeros_like(a) if store else None
        N.check(self._lib.pf_op_logsoftmax_argmax(self._h, _fp(a), rows, V, _fp(y) if store else None,
                                                  ids.ctypes.data_as(C.POINTER(C.c_int64))))
        return (y, ids.reshape(a.shape[:-1])) if store else ids.reshape(a.shape[:-1])

    # ---- streaming seams (include/paraformer_hip.h section 7) ----------------------
    def online_encoder(self, speech):
        sp = _f32(speech)
        B, Tc, _ = sp.shape
        enc = np.zeros((B, Tc, 512), np.float32)
        al = np.zeros((B, Tc), np.float32)
        N.check(self._lib.pf_online_encoder(self._h, _fp(sp), B, Tc, _fp(enc), _fp(al)))
        return enc, al

    def online_decoder(self, enc, embeds, embeds_len, caches, want_logits=True):
        enc, emb = _f32(enc), _f32(embeds)
        B, Tc, _ = enc.shape
        L = emb.shape[1]
        ln = np.ascontiguousarray(embeds_len, dtype=np.int32)
        cin = _f32(np.stack(caches))                       # [n_layers, B, 512, 10]
        cout = np.zeros_like(cin)
        ids = np.zeros((B, L), np.int64)
        logits = np.zeros((B, L, self.vocab), np.float32) if want_logits else None
        N.check(self._lib.pf_online_decoder(self._h, _fp(enc), B, Tc, _fp(emb), L, ln.ctypes.data_as(C.POINTER(C.c_int32)),
                                            _fp(cin), cin.shape[0], _fp(logits) if want_logits else None,
                                            ids.ctypes.data_as(C.POINTER(C.c_int64)), _fp(cout)))
        return logits, ids, [cout[i] for i in range(cout.shape[0])]

    def op_layernorm(self, x, gamma, beta) -> np.ndarray:
        x, g, b = _f32(x), _f32(gamma), _f32(beta)
        D = x.shape[-1]
        y = np.zeros_like(x)
        N.check(self._lib.pf_op_layernorm(self._h, _fp(x), _fp(g), _fp(b), x.size // D, D, _fp(y)))
        return y

    def op_attention(self, q, k, v, heads=4) -> np.ndarray:
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, Lq, _ = q.shape
        Lk = k.shape[1]
        o = np.zeros_like(q)
        N.check(self._lib.pf_op_attention(self._h, _fp(q), _fp(k), _fp(v), B, Lq, Lk, heads, _fp(o)))
        return o

    def op_attention_ex(self, q, k, v, heads=4, kind=0, layout=0, shared_kv=False, o_ld=0, form=0, ldkv=0, kv_off=0,
                        want_range=False) -> dict:
        """The attention kernels launched as the pipeline launches them (pf_op_attention_ex in the header).  Returns
        out [B, Lq, Dm] fp32; raw = the WHOLE output buffer as 16-bit (kinds 0 / 2) or 32-bit (kind 1) words,
        [B*Lq + 256, o_ld] (kind 2: [.., 2*o_ld] = hi | lo'), canary PF_ATTN_CANARY where nothing was stored;
        range = the 256 {min, max} pairs or None; ran = False when the kind-2 launcher declined."""
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, Lq, Dm = q.shape
        Lk = k.shape[1]
        assert Dm == heads * 128 and k.shape == v.shape and k.shape[0] == (1 if shared_kv else B)
        ld = o_ld or Dm
        rows = B * Lq + 256
        raw = np.zeros((rows, 2 * ld if kind == 2 else ld), np.uint32 if kind == 1 else np.uint16)
        out = np.zeros_like(q)
        rng = np.zeros((256, 2), np.float32) if want_range else None
        ran = C.c_int32(0)
        d = N.PfAttnDesc(C.sizeof(N.PfAttnDesc), kind, layout, 1 if shared_kv else 0, o_ld, form, ldkv, kv_off)
        N.check(self._lib.pf_op_attention_ex(self._h, _fp(q), _fp(k), _fp(v), B, Lq, Lk, heads, C.byref(d), _fp(out),
                                             raw.ctypes.data, raw.nbytes, _fp(rng) if want_range else None, C.byref(ran)))
        return {"out": out, "raw": raw, "range": rng, "ran": bool(ran.value)}

    def op_fsmn(self, v, w, mask=None) -> np.ndarray:
        v, w = _f32(v), _f32(w)
        B, T, D = v.shape
        y = np.zeros_like(v)
        m = _f32(mask) if mask is not None else None
        N.check(self._lib.pf_op_fsmn(self._h, _fp(v), _fp(w), _fp(m) if m is not None else None, B, T, D,
                                     w.shape[1], _fp(y)))
        return y

    def op_cif(self, H, alphas, threshold=1.0, Lcap=None):
        H, a = _f32(H), _f32(alphas)
        B, T, D = H.shape
        if Lcap is None:
            Lcap = int(np.ceil(a.sum(axis=1).max())) + 2
        E = np.zeros((B, Lcap, D), np.float32)
        fc, tn, L = np.zeros(B, np.int32), np.zeros(B, np.int32), C.c_int32()
        N.check(self._lib.pf_op_cif(self._h, _fp(H), _fp(a), B, T, D, threshold, Lcap, _fp(E),
                                    fc.ctypes.data_as(C.POINTER(C.c_int32)), tn.ctypes.data_as(C.POINTER(C.c_int32)), L))
        return E[:, : L.value].copy(), fc, tn

    def op_cif_alphas(self, H) -> np.ndarray:
        """The predictor's alpha stage as the pipeline runs it, on the loaded predictor weights (pf_op_cif_alphas):
        H [B, T, d_model] -> alphas [B, T+1], the tail weight last."""
        H = _f32(H)
        B, T, _ = H.shape
        a = np.zeros((B, T + 1), np.float32)
        N.check(self._lib.pf_op_cif_alphas(self._h, _fp(H), B, T, _fp(a)))
        return a

    def op_encoder(self, speech) -> np.ndarray:
        sp = _f32(speech)
        B, T, _ = sp.shape
        H = np.zeros((B, T, 512), np.float32)
        N.check(self._lib.pf_op_encoder(self._h, _fp(sp), B, T, _fp(H)))
        return H


class EngineGroup:
    """pf_group: one engine per listed device inside this process, utterance shards, RCCL weight broadcast and
    hypothesis gather (include/paraformer_hip.h section 4b).  `devices` may repeat a device."""

    def __init__(self, devices, weights=None, weights_path=None, cmvn=None, mvn_path=None, dither=0.0, snip_edges=False,
                 lfr_m=7, lfr_n=6, n_mels=80, fs=16000, window="hamming", use_itn=False, dither_seed=0, math_mode=0):
        self._lib = N.load()
        cfg, self._keep = _build_config(weights, weights_path, None, 0, cmvn, mvn_path, 0, dither, snip_edges, lfr_m,
                                        lfr_n, n_mels, fs, window, use_itn, 0, 0, dither_seed, math_mode)
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        N.check(self._lib.pf_group_create(C.byref(cfg), devs, len(devices), C.byref(h)))
        self._h = h
        n, r = C.c_int32(), C.c_int32()
        N.check(self._lib.pf_group_info(self._h, n, r))
        self.size, self.uses_rccl = n.value, bool(r.value)

    def recognize(self, samples_list, want_logits=False, hotwords=None) -> BatchResult:
        hp, hn, _keep = Engine._hw(hotwords)
        arrs = [_f32(s) for s in samples_list]
        B = len(arrs)
        ptrs = (C.POINTER(C.c_float) * max(B, 1))(*[_fp(a) for a in arrs])
        ns = (C.c_int64 * max(B, 1))(*[a.shape[0] for a in arrs])
        dummy = np.zeros(1, np.float32)

        def call(out):
            if want_logits:
                out.logits = _fp(dummy)
                out.logits_cap = 1
            rc = self._lib.pf_group_recognize(self._h, ptrs, ns, B, hp, hn, C.byref(out))
            return 0 if (want_logits and rc == N.PF_ERR_CAPACITY) else rc
        return _collect_result(self._lib, lambda o: self._lib.pf_group_fetch(self._h, o), call, B, want_logits)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pf_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
