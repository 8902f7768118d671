"""GPU: CTC forced alignment on the device (csrc/k_ctcalign.hip, Engine.set_decode(PF_DECODE_ALIGN),
OfflineRecognizer.SetAlign) — the kernel against the definition (tests/ctcalign_ref.py) over the smallest shapes at which it
can go wrong, the engine in all four math modes against the definition fed the engine's own rows, the beam's hypotheses,
refusals, the recognizer mirror, two caller threads, the CLI.

Comparison rule: path_score, ok, first, last and tok_score identical (float32 bit for bit); loglik within
16 * T * 2^-53 * max(1, |s|) (ctcalign_ref.loglik_tol), non-finite values identical."""
import io
import math
import threading
import wave

import numpy as np
import pytest

import ctcalign_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe

pytestmark = pytest.mark.gpu
SCORES, CTC, TOPK, BEAM, ALIGN = N.PF_DECODE_SCORES, N.PF_DECODE_CTC, N.PF_DECODE_TOPK, N.PF_DECODE_CTC_BEAM, N.PF_DECODE_ALIGN
SV_VOCAB = 403
POISON_ID = 1 << 30


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def any_engine():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    eng = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield eng
    eng.close()


def _check_job(tag, got, b, h, ref, T, cap):
    """job (b, h) of an AlignResult against a ctcalign_ref.Alignment (None: a skipped job)"""
    ps, ll, ok = got.path_score[b, h], float(got.loglik[b, h]), int(got.ok[b, h])
    first, last, tok = got.first[b, h], got.last[b, h], got.tok_score[b, h]
    if ref is None:
        assert ps == -np.inf and ll == -np.inf and ok == 0, (tag, ps, ll, ok)
        assert (first == -1).all() and (last == -1).all() and (_bits(tok) == 0).all(), tag
        return 0.0
    U = len(ref.first)
    assert ok == ref.ok, (tag, ok, ref.ok)
    assert _bits(ps) == _bits(ref.path_score) or (np.isnan(ps) and np.isnan(ref.path_score)), (tag, ps, ref.path_score)
    np.testing.assert_array_equal(first[:U], ref.first, err_msg=tag)
    np.testing.assert_array_equal(last[:U], ref.last, err_msg=tag)
    np.testing.assert_array_equal(_bits(tok[:U]), _bits(ref.tok_score), err_msg=tag)
    assert (first[U:cap] == -1).all() and (last[U:cap] == -1).all() and (_bits(tok[U:cap]) == 0).all(), tag   # no canary left
    if math.isfinite(ref.loglik):
        tol = R.loglik_tol(T, ref.loglik)
        assert abs(ll - ref.loglik) <= tol, (tag, ll, ref.loglik, abs(ll - ref.loglik), tol)
        return abs(ll - ref.loglik) / tol
    assert ll == ref.loglik or (math.isnan(ll) and math.isnan(ref.loglik)), (tag, ll, ref.loglik)
    return 0.0


def _run_kernel(eng, lp, targets, pad=0, cap=None, lens=None):
    """lp [T, V], targets: H entries (a list of ids, or None for a skipped job).  B = 3 utterances over the same rows with
    lengths (T, 1, 0); rows at and beyond each length, the columns beyond V and the target slots beyond tlen are poisoned;
    the outputs start as canaries.  Every job is compared with the definition."""
    T, V = lp.shape
    H = len(targets)
    ld = V + pad
    lens = np.array([T, min(T, 1), 0] if lens is None else lens, np.int32)
    B = len(lens)
    cap = max([len(t) for t in targets if t is not None] + [1]) if cap is None else cap
    x = np.full((B, max(T, 1), ld), np.nan, np.float32)
    for b in range(B):
        x[b, : lens[b], :V] = lp[: lens[b]]
    x[:, :, V:] = np.inf                                                          # never read: beyond V in a row
    x = x[:, :T]
    tgt = np.full((B, H, cap), POISON_ID, np.int32)
    tlen = np.full((B, H), -1, np.int32)
    for h, t in enumerate(targets):
        if t is not None:
            tgt[:, h, : len(t)] = np.asarray(t, np.int32)
            tlen[:, h] = len(t)
    out = (np.full((B, H), 12345.0, np.float32), np.full((B, H), 12345.0, np.float64), np.full((B, H), -77, np.int32),
           np.full((B, H, cap), -77, np.int32), np.full((B, H, cap), -77, np.int32), np.full((B, H, cap), 12345.0, np.float32))
    got = eng.op_ctc_align(x, tgt, tlen, lens, V=V, out=out)
    worst = 0.0
    for b in range(B):
        for h, t in enumerate(targets):
            ref = None if t is None else R.align(lp[: lens[b]], t)
            worst = max(worst, _check_job("T=%d b=%d h=%d U=%s ld=%d" % (T, b, h, None if t is None else len(t), ld),
                                          got, b, h, ref, max(int(lens[b]), 1), cap))
    return got, worst


# ---- 1: the kernel against the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 130])
def test_kernel_equals_reference(any_engine, T):
    """U in {0, 1, 7, 8}: S = 15 and 17 lie on either side of a back-pointer word; T on either side of a backtrace stretch
    (16 frames) and of 64; H = 1 and H = 3 with one skipped job; ld = V and ld = V + 37."""
    rng = np.random.default_rng(100 + T)
    V = 11
    worst = 0.0
    for U in (0, 1, 7, 8):
        lp, y = R.random_case(rng, T, V, U)
        _, y2 = R.random_case(rng, 1, V, max(U - 1, 0))
        for pad in (0, 37):
            worst = max(worst, _run_kernel(any_engine, lp, [y], pad)[1])
            worst = max(worst, _run_kernel(any_engine, lp, [y, None, y2], pad, cap=U + 3)[1])
    print("  T=%d: worst loglik difference %.3g of the tolerance" % (T, worst))


@pytest.mark.parametrize("U,T", [(127, 300), (128, 300), (300, 620)], ids=["S255", "S257", "S601"])
def test_kernel_states_across_the_thread_count(any_engine, U, T):
    """S = 255 / 257 on either side of the 256 threads (one / two states per thread); U = 300: four states per thread,
    38 back-pointer words per frame"""
    rng = np.random.default_rng(U)
    lp, y = R.random_case(rng, T, 50, U)
    assert R.min_frames(y) <= T
    got, worst = _run_kernel(any_engine, lp, [y], 37, lens=[T, T - 7])
    assert got.ok[0, 0] == 1 and (got.first[0, 0] >= 0).all()
    print("  U=%d T=%d: worst loglik difference %.3g of the tolerance" % (U, T, worst))
    if U == 128:                                      # the same job under a launch sized for longer targets
        _run_kernel(any_engine, lp, [y, y[:5]], 0, cap=1023, lens=[T])


def test_kernel_ties_minimal_frames_and_undefined_jobs(any_engine):
    rng = np.random.default_rng(7)
    multi = 0
    for k in range(12):                                # integer-valued rows: exact ties, the larger state wins
        lp, y = R.tie_case(rng, int(rng.integers(2, 41)), 3, int(rng.integers(1, 9)))
        _run_kernel(any_engine, lp, [y, y[:1]])
        multi += 1
    assert multi == 12
    # the fewest frames a target with repeats fits in, and one fewer
    y = [3, 3, 5, 5, 5, 2, 3]
    need = R.min_frames(y)
    assert need == len(y) + 3
    lp, _ = R.random_case(rng, need, 7, 0)
    got, _ = _run_kernel(any_engine, lp, [y], lens=[need, need - 1])
    assert got.ok[:, 0].tolist() == [1, 0] and got.path_score[1, 0] == -np.inf and got.loglik[1, 0] == -np.inf
    one = [4] * 9                                      # one repeated id: a blank between every pair
    lp, _ = R.random_case(rng, 2 * 9 - 1, 7, 0)
    got, _ = _run_kernel(any_engine, lp, [one], lens=[17, 16])
    assert got.ok[:, 0].tolist() == [1, 0]
    assert got.first[0, 0].tolist() == got.last[0, 0].tolist() == list(range(0, 17, 2))
    # U > T, T = 0 with U > 0 and with U = 0, a NaN row, -inf entries
    lp, y = R.random_case(rng, 6, 7, 0)[0], [1, 2, 3]
    got, _ = _run_kernel(any_engine, lp, [y, [], y + y + y], lens=[6, 2, 0])
    assert got.ok.tolist() == [[1, 1, 0], [0, 1, 0], [0, 1, 0]] and got.path_score[2, 1] == 0 and got.loglik[2, 1] == 0
    nan = lp.copy()
    nan[3] = np.nan
    got, _ = _run_kernel(any_engine, nan, [y, []], lens=[6, 3])
    assert got.ok.tolist() == [[0, 0], [1, 1]] and np.isnan(got.path_score[0]).all()
    ninf = lp.copy()
    ninf[:, y[1]] = -np.inf                            # the second token can never be emitted
    ninf[2, 0] = -np.inf
    got, _ = _run_kernel(any_engine, ninf, [y, y[:1], []], lens=[6])
    assert got.ok[0].tolist() == [0, 1, 0]
    # a target longer than cap or than PF_ALIGN_MAX_TOKENS, an id outside the row: not ok, nothing read out of bounds
    x = np.ascontiguousarray(lp[None])
    tgt = np.array([[[1, 2, 3], [1, 7, 2], [1, 2, -1]]], np.int32)
    r = any_engine.op_ctc_align(x, tgt, np.array([[4, 3, 3]], np.int32), np.array([6], np.int32))
    assert r.ok.tolist() == [[0, 0, 0]] and (r.first == -1).all() and (r.tok_score == 0).all()
    r = any_engine.op_ctc_align(x, tgt, np.array([[N.PF_ALIGN_MAX_TOKENS + 1, 3, 2]], np.int32), np.array([6], np.int32))
    assert r.ok.tolist() == [[0, 0, 1]]
    for bad in (dict(V=0), dict(V=8)):                 # V outside 1 .. ld
        with pytest.raises(N.PfError) as ei:
            any_engine.op_ctc_align(x, tgt, np.array([[1, 1, 1]], np.int32), np.array([6], np.int32), **bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG


# ---- 2: the engine, the tiny SenseVoice model of tests/test_gpu_topk.py, every math mode -------------------------------------
def _sv_model(sv_embed):
    cfg = W.sensevoice_small_config(enc_layers=3, tp_layers=2, vocab=SV_VOCAB)
    w = W.synth_weights(cfg, seed=9)
    w["embed.weight"] = sv_embed.astype(np.float32)
    b = np.array(w["ctc.bias"], np.float32)
    b[8:] -= 30
    b[0] += 1.0
    w["ctc.bias"] = b
    return cfg, w


def _audio():
    return [W.synth_audio(n, 40 + u) for u, n in enumerate((48000, 20000, 33000))]


def _seq_sum(v):
    s = np.float32(v[0])
    for x in v[1:]:
        s = np.float32(s + np.float32(x))
    return s


def _same_extras(r1, r0):
    np.testing.assert_array_equal(r1.token_ids, r0.token_ids)
    np.testing.assert_array_equal(_bits(r1.scores), _bits(r0.scores))
    for name in ("n", "ids", "first", "last"):
        np.testing.assert_array_equal(getattr(r1.ctc, name), getattr(r0.ctc, name))
    np.testing.assert_array_equal(_bits(r1.ctc.score), _bits(r0.ctc.score))
    np.testing.assert_array_equal(r1.topk.ids, r0.topk.ids)
    np.testing.assert_array_equal(_bits(r1.topk.val), _bits(r0.topk.val))
    np.testing.assert_array_equal(r1.topk.n, r0.topk.n)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_engine_alignment_is_the_reference_of_its_own_rows(sv_embed, mode):
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
    e0.set_decode(CTC | TOPK)
    e1.set_decode(CTC | TOPK | ALIGN)
    e0.set_topk(2)
    e1.set_topk(2)
    r0 = e0.recognize(audio, want_logits=True)
    ra = e1.recognize(audio, want_logits=True)                                   # no targets, no beam: H = 0, nothing launched
    assert r0.align is None and ra.align is not None and ra.align.H == 0
    _same_extras(ra, r0)
    rows = [4 + e1.frontend(a).shape[0] for a in audio]                          # n_b: the prompt rows and the utterance's frames
    assert max(rows) == ra.L and min(rows) < ra.L
    greedy = [[int(v) for v in r0.ctc.ids[b, : r0.ctc.n[b]]] for b in range(3)]
    assert max(len(g) for g in greedy) >= 2                                       # (short or empty labelings are targets too)
    # the greedy labeling as the target: its best alignment is the arg-max path itself
    e1.set_align_targets(greedy)
    r1 = e1.recognize(audio, want_logits=True)
    _same_extras(r1, r0)
    np.testing.assert_array_equal(_bits(r1.logits), _bits(r0.logits))
    al = r1.align
    assert al.H == 1 and al.len[:, 0].tolist() == [len(g) for g in greedy]
    for b, nb in enumerate(rows):
        lp = r1.logits[b, :nb]
        cap = al.first.shape[2]
        d = _check_job("mode %d utterance %d" % (mode, b), al, b, 0, R.align(lp, greedy[b]), nb, cap)
        print("  mode %d utterance %d: n_b=%d U=%d path %.9g loglik %.17g (%.3g of the tolerance)"
              % (mode, b, nb, len(greedy[b]), al.path_score[b, 0], al.loglik[b, 0], d))
        # no frame's two best log-probs are equal (seeds 40 .. 42 give none; with a tie another seed would be needed)
        assert (r1.topk.n[b, :nb] == 2).all() and (r1.topk.val[b, :nb, 0] != r1.topk.val[b, :nb, 1]).all()
        U = len(greedy[b])
        assert al.ok[b, 0] == 1
        np.testing.assert_array_equal(al.first[b, 0, :U], r1.ctc.first[b, :U])
        np.testing.assert_array_equal(al.last[b, 0, :U], r1.ctc.last[b, :U])
        np.testing.assert_array_equal(_bits(al.tok_score[b, 0, :U]), _bits(r1.ctc.score[b, :U]))
        assert _bits(al.path_score[b, 0]) == _bits(_seq_sum(r1.scores[b, :nb]))
        assert al.loglik[b, 0] >= float(al.path_score[b, 0]) - 1e-3
    # the targets were consumed; a row without a target is skipped; other targets than the greedy one
    r2 = e1.recognize(audio)
    assert r2.align.H == 0
    other = [[7, 6, 5, 5], None, [5]]
    e1.set_align_targets(other)
    r3 = e1.recognize(audio, want_logits=True)
    assert r3.align.H == 1 and r3.align.len[:, 0].tolist() == [len(other[0]), -1, 1]
    for b, nb in enumerate(rows):
        ref = None if other[b] is None else R.align(r3.logits[b, :nb], other[b])
        _check_job("mode %d other %d" % (mode, b), r3.align, b, 0, ref, nb, r3.align.first.shape[2])
    # the flag cleared: nothing extra comes back
    e1.set_decode(0)
    r = e1.recognize(audio)
    assert r.align is None and r.scores is None
    np.testing.assert_array_equal(r.token_ids, r0.token_ids)
    e0.close(); e1.close()


def test_engine_beam_hypotheses_are_aligned(sv_embed):
    from aliparaformerasr_amd.engine import Engine
    import ctcbeam_ref as RB
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    e0 = Engine(weights=blob, cmvn=cmvn, device=0)
    e1 = Engine(weights=blob, cmvn=cmvn, device=0)
    Wd, NB = 8, 5
    e0.set_decode(BEAM | CTC)
    e1.set_decode(BEAM | CTC | ALIGN)
    e0.set_ctc_beam(Wd, NB)
    e1.set_ctc_beam(Wd, NB)
    r0 = e0.recognize(audio, want_logits=True)
    rows = [4 + e1.frontend(a).shape[0] for a in audio]
    for with_target in (False, True):
        own = [[5, 6], None, [7]]
        if with_target:
            e1.set_align_targets(own)
        r1 = e1.recognize(audio, want_logits=True)
        _same_extras(r1, r0)                                                      # bit-identical with and without the flag
        assert [r1.beam.hyps(b) for b in range(3)] == [r0.beam.hyps(b) for b in range(3)]
        al, hc = r1.align, int(with_target)
        assert al.H == hc + NB
        cap = al.first.shape[2]
        for b, nb in enumerate(rows):
            lp = r1.logits[b, :nb]
            if with_target:
                _check_job("own %d" % b, al, b, 0, None if own[b] is None else R.align(lp, own[b]), nb, cap)
            hyps = r1.beam.hyps(b)
            assert len(hyps) >= 2
            for i in range(NB):
                if i >= len(hyps):
                    assert al.len[b, hc + i] == -1
                    _check_job("past n_hyp", al, b, hc + i, None, nb, cap)
                    continue
                ids, score = hyps[i]
                assert al.len[b, hc + i] == len(ids)
                _check_job("hyp %d of %d" % (i, b), al, b, hc + i, R.align(lp, list(ids)), nb, cap)
                assert al.ok[b, hc + i] == 1
                ll = float(al.loglik[b, hc + i])
                assert ll >= score - RB.tol(nb, score), (ll, score)               # the search sums a subset of the alignments
                f, l = al.first[b, hc + i, : len(ids)], al.last[b, hc + i, : len(ids)]
                assert (f <= l).all() and (f[1:] > l[:-1]).all() and (f >= 0).all() and (l < nb).all()
    e0.close(); e1.close()


def test_status_codes_and_refusals(sv_embed):
    import ctypes as C
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pf = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        pf.set_decode(ALIGN)                                                      # no CTC head on a paraformer
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    pf.close()
    cfg = W.seaco_paraformer_config(enc_layers=2, dec_layers=2, vocab=120, seaco_layers=2, seaco_nobias=111)
    sc = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, 21)), cmvn=W.synth_cmvn(), device=0)
    with pytest.raises(N.PfError) as ei:
        sc.set_decode(ALIGN)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    sc.close()
    cfg, w = _sv_model(sv_embed)
    eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    lib, h = eng._lib, eng._h
    for bit in (4, 64):
        assert lib.pf_engine_set_decode(h, bit) == N.PF_ERR_INVALID_ARG
        assert lib.pf_engine_set_decode(h, ALIGN | bit) == N.PF_ERR_INVALID_ARG
    audio = _audio()
    hh, mx = C.c_int32(), C.c_int32()
    with pytest.raises(N.PfError) as ei:
        eng.set_align_targets([[5], [6], [7]])                                    # the flag is not set
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    eng.set_decode(SCORES)
    eng.recognize(audio)
    assert lib.pf_fetch_align(h, None, None, None, None, None, None, None, 0, hh, mx) == N.PF_ERR_INVALID_ARG   # ran without the flag
    eng.set_decode(ALIGN)
    for bad in ([[0], [5], [5]], [[5], [SV_VOCAB], [5]], [[5], [5], [-3]]):       # an id outside [1, V)
        with pytest.raises(N.PfError) as ei:
            eng.set_align_targets(bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        eng.set_align_targets([[5] * (N.PF_ALIGN_MAX_TOKENS + 1), [5], [5]])      # an over-long target
    assert ei.value.code == N.PF_ERR_CAPACITY
    eng.set_align_targets([[5] * N.PF_ALIGN_MAX_TOKENS, None, [5]])               # the longest one is accepted: more tokens than frames
    r = eng.recognize(audio)
    assert r.align.ok[:, 0].tolist() == [0, 0, 1] and r.align.len[:, 0].tolist() == [N.PF_ALIGN_MAX_TOKENS, -1, 1]
    assert r.scores is not None and r.topk is None                                # implies SCORES, not TOPK
    eng.set_align_targets([[5], [6]])                                             # a batch of another size: refused, targets dropped
    with pytest.raises(N.PfError) as ei:
        eng.recognize(audio)
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    assert eng.recognize(audio).align.H == 0
    # the fetch protocol: sizes first, the capacity error reports them
    eng.set_align_targets([[5, 6, 7], [6], None])
    r = eng.recognize(audio)
    assert lib.pf_fetch_align(h, None, None, None, None, None, None, None, 0, hh, mx) == N.PF_OK and (hh.value, mx.value) == (1, 3)
    first = np.full((3, 1, 2), -7, np.int32)
    h2, mx2 = C.c_int32(), C.c_int32()
    assert lib.pf_fetch_align(h, None, None, None, None, first.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 2, h2, mx2) == N.PF_ERR_CAPACITY
    assert (h2.value, mx2.value) == (1, 3) and (first == -7).all()
    first = np.full((3, 1, 4), -7, np.int32)
    assert lib.pf_fetch_align(h, None, None, None, None, first.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 4, None, None) == N.PF_OK
    np.testing.assert_array_equal(first[:, :, :3], r.align.first)
    assert (first[:, :, 3] == -1).all()
    eng.close()


# ---- 3: the recognizer mirror ---------------------------------------------------------------------------------------------------
def _sv_dir(tmp_path, sv_embed):
    cfg, w = _sv_model(sv_embed)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, w)
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("model: SenseVoiceSmall\nuse_itn: true\nfrontend_conf:\n  dither: 0\n")
    toks = ["<blank>", "<s>", "</s>", "<unk>"] + ["<|tag%d|>" % i for i in range(20)] + [chr(0x4E00 + i) for i in range(SV_VOCAB - 24)]
    (tmp_path / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    return [str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")], toks


def _get(rec, audio, targets=None):
    streams = []
    for i, a in enumerate(audio):
        s = rec.CreateOfflineStream()
        s.AddSamples(a)
        if targets is not None and targets[i] is not None:
            s.SetAlignIds(targets[i])
        streams.append(s)
    return streams, rec.GetResults(streams)


def _pairs_ok(ts, n, dur_ms):
    """n [begin, end] pairs, multiples of the 60 ms frame, monotone and inside the audio"""
    assert len(ts) == n
    flat = [v for p in ts for v in p]
    assert all(len(p) == 2 and p[0] <= p[1] for p in ts) and flat == sorted(flat)
    assert all(v % 60 == 0 and 0 <= v <= dur_ms + 60 for v in flat), (ts, dur_ms)


def test_recognizer_alignment_and_alternative_times(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, toks = _sv_dir(tmp_path, sv_embed)
    audio = [W.synth_audio(32000, 5), W.synth_audio(20000, 6)]
    dur = [2000, 1250]
    plain, ctc, rec = (OfflineRecognizer(*paths) for _ in range(3))
    ctc.SetDecode(ctc=True)
    sc, _ = _get(ctc, audio)                                                     # the greedy labelings and their times
    s0, res0 = _get(plain, audio)
    rec.SetAlign(True)
    # a mixed batch: one stream has a target (its greedy labeling, the longer of the two), the other has none
    k = 0 if len(sc[0].Tokens) >= len(sc[1].Tokens) else 1
    own = [None, None]
    own[k] = sc[k].Tokens
    s1, res1 = _get(rec, audio, own)
    for b in range(2):
        assert s1[b].Tokens == s0[b].Tokens and s1[b].Timestamps == s0[b].Timestamps and s1[b].Scores == s0[b].Scores == []
        assert (res1[b].Text, res1[b].Tokens, res1[b].Timestamps) == (res0[b].Text, res0[b].Tokens, res0[b].Timestamps)
        assert s1[b].Alternatives == []
    al = s1[k].Alignment
    assert s1[1 - k].Alignment is None and s0[k].Alignment is None
    assert al.Ok == 1 and al.Timestamps == sc[k].Timestamps and len(sc[k].Tokens) >= 2    # the arg-max path is the best alignment
    assert _bits(np.array(al.Scores, np.float32)).tolist() == _bits(np.array(sc[k].Scores, np.float32)).tolist()
    assert al.LogLik >= al.PathScore - 1e-3
    _pairs_ok(al.Timestamps, len(sc[k].Tokens), dur[k])
    # the target stays with the stream object only; an impossible one is reported, not raised
    s2, _ = _get(rec, audio, [None, [5] * 400])
    assert s2[0].Alignment is None and s2[1].Alignment.Ok == 0 and s2[1].Alignment.Timestamps == []
    st = rec.CreateOfflineStream()
    for bad in ([0], [SV_VOCAB], [-1]):
        with pytest.raises(N.PfError) as ei:
            st.SetAlignIds(bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as ei:
        st.SetAlignIds([5] * (N.PF_ALIGN_MAX_TOKENS + 1))
    assert ei.value.code == N.PF_ERR_CAPACITY
    # with the beam search: every alternative carries the times of its own alignment and its log-likelihood
    beam = OfflineRecognizer(*paths)
    beam.SetCtcBeam(4, 8, 4)
    sb, _ = _get(beam, audio)
    rec.SetCtcBeam(4, 8, 4)
    s3, res3 = _get(rec, audio, own)
    from oracle import glue
    for b in range(2):
        assert (res3[b].Text, res3[b].Timestamps) == (res0[b].Text, res0[b].Timestamps)
        a0, a1 = sb[b].Alternatives, s3[b].Alternatives
        assert len(a1) >= 2 and [(a.Ids, a.Score) for a in a1] == [(a.Ids, a.Score) for a in a0]     # order and scores untouched
        assert all(a.Timestamps == [] and a.LogLik is None for a in a0)
        for a in a1:
            _pairs_ok(a.Timestamps, len(a.Ids), dur[b])
            assert a.LogLik >= a.Score - R.loglik_tol(64, a.Score)                # fewer than 64 frames here
            text, _tlen, tk, _ = glue.decode_multi_one(toks, a.Ids, a.Timestamps)
            assert (a.Text, a.Tokens) == (text, tk)
    assert s3[k].Alignment.Timestamps == al.Timestamps and s3[1 - k].Alignment is None
    # off again
    rec.SetAlign(False)
    s4, _ = _get(rec, audio, own)
    assert s4[k].Alignment is None and all(a.Timestamps == [] and a.LogLik is None for a in s4[0].Alternatives + s4[1].Alternatives)
    for r in (plain, ctc, rec, beam):
        r.Dispose()


def test_recognizer_refuses_paraformer(tmp_path):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    W.save_pfw(str(tmp_path / "model.pfw"), cfg, W.synth_weights(cfg, seed=3))
    (tmp_path / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    (tmp_path / "asr.yaml").write_text("frontend_conf:\n  dither: 0\n")
    (tmp_path / "tokens.txt").write_text("\n".join(["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(61)]) + "\n", encoding="utf-8")
    rec = OfflineRecognizer(*[str(tmp_path / f) for f in ("model.pfw", "asr.yaml", "am.mvn", "tokens.txt")])
    with pytest.raises(N.PfError) as ei:
        rec.SetAlign(True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.SetAlign(False)                                                           # turning it off is always accepted
    rec.Dispose()


def test_two_threads_on_one_recognizer(tmp_path, sv_embed):
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    paths, _ = _sv_dir(tmp_path, sv_embed)
    rec = OfflineRecognizer(*paths)
    rec.SetAlign(True)
    rec.SetCtcBeam(3, 8, 4)
    batches = [[W.synth_audio(32000, 5), W.synth_audio(20000, 6)], [W.synth_audio(26000, 91)]]
    targets = [[[5, 6], None], [[7, 6, 5]]]

    def snapshot(streams, res):
        out = []
        for s, r in zip(streams, res):
            a = s.Alignment
            out.append((r.Text, None if a is None else (a.Ok, a.PathScore, a.LogLik, a.Timestamps, a.Scores),
                        [(x.Ids, x.Score, x.Timestamps, x.LogLik) for x in s.Alternatives]))
        return out
    want = [snapshot(*_get(rec, b, t)) for b, t in zip(batches, targets)]
    assert want[0][0][1] is not None and want[0][1][1] is None and want[1][0][1] is not None and want[0][0][1] != want[1][0][1]
    errors = []

    def worker(i):
        try:
            for _ in range(4):
                assert snapshot(*_get(rec, batches[i], targets[i])) == want[i]
        except Exception as ex:                          # noqa: BLE001 — reported by the main thread
            errors.append((i, repr(ex)))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    rec.Dispose()


def test_cli_prints_the_pairs(tmp_path, sv_embed):
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "m"
    d.mkdir()
    _sv_dir(d, sv_embed)
    pcm = (np.clip(W.synth_audio(32000, 40), -1, 1) * 32767).astype("<i2")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    (tmp_path / "ids.txt").write_text("5 6 7\n")
    for method in ("one", "batch"):
        out = io.StringIO()
        res = ex.offline_recognizer(method=method, model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out,
                                    align=str(tmp_path / "ids.txt"))
        lines = out.getvalue().splitlines()
        al = [ln for ln in lines if ln.startswith("align ")]
        assert len(res) == 1 and len(al) == 1, out.getvalue()
        assert lines[lines.index(al[0]) - 1].startswith('{"text": "%s"' % res[0].Text)          # under the usual result line
        assert al[0].startswith("align ok:1 path:-") and al[0].count("[") == 3 and " loglik:-" in al[0]
        out = io.StringIO()
        ex.offline_recognizer(method=method, model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=3, topk=4, beam=8,
                              align="beam")
        lines = out.getvalue().splitlines()
        nb = [i for i, ln in enumerate(lines) if ln.startswith("nbest[")]
        assert len(nb) == 3, out.getvalue()
        for k, i in enumerate(nb):                                                # the pairs under each hypothesis
            assert lines[i + 1].startswith("align[%d] loglik:-" % k) and " pairs:" in lines[i + 1]
    out = io.StringIO()
    ex.offline_recognizer(method="one", model="m", base=str(tmp_path), files=[str(d / "a.wav")], out=out, nbest=3, topk=4, beam=8)
    assert "align" not in out.getvalue()                                          # without -align nothing changes


# ---- 4: the decoders share one forward: together they leave what each leaves alone --------------------------------------------
def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_beam(r1, r0, hot):
    for name in ("n_hyp", "ids", "len"):
        np.testing.assert_array_equal(getattr(r1.beam, name), getattr(r0.beam, name), err_msg=name)
    np.testing.assert_array_equal(_bits64(r1.beam.score), _bits64(r0.beam.score))
    if hot:
        np.testing.assert_array_equal(r1.beam.matched, r0.beam.matched)
        np.testing.assert_array_equal(_bits64(r1.beam.loglik_sum), _bits64(r0.beam.loglik_sum))
    else:
        assert r1.beam.matched is None and r0.beam.matched is None and r1.beam.loglik_sum is None and r0.beam.loglik_sum is None


def _same_align(r1, r0):
    a1, a0 = r1.align, r0.align
    assert a1.H == a0.H
    for name in ("ok", "len", "first", "last"):
        np.testing.assert_array_equal(getattr(a1, name), getattr(a0, name), err_msg=name)
    np.testing.assert_array_equal(_bits(a1.path_score), _bits(a0.path_score))
    np.testing.assert_array_equal(_bits(a1.tok_score), _bits(a0.tok_score))
    np.testing.assert_array_equal(_bits64(a1.loglik), _bits64(a0.loglik))


def test_every_flag_at_once_equals_each_flag_alone(sv_embed):
    """One engine with CTC | TOPK | CTC_BEAM | ALIGN (W = 8, N = 4, targets of lengths [-1, n, 0]) against engines that have
    only the flags a field needs: ids, scores, the collapse, the top-k lists, the beam (plain, then with a hot-word set:
    matched / loglik_sum too) and every alignment field, bit for bit."""
    from aliparaformerasr_amd.engine import Engine
    cfg, w = _sv_model(sv_embed)
    blob, cmvn, audio = W.pack_pfw(cfg, w), W.synth_cmvn(), _audio()
    Wd, NB, K = 8, 4, 4

    def run(flags, targets=None, hot=None):
        e = Engine(weights=blob, cmvn=cmvn, device=0)
        e.set_decode(flags)
        e.set_topk(K)
        e.set_ctc_beam(Wd, NB)
        if hot is not None:
            e.set_ctc_hotwords(hot, 1.5)
        if targets is not None:
            e.set_align_targets(targets)
        r = e.recognize(audio)
        e.close()
        return r
    r_plain, r_sc, r_ctc, r_topk = run(0), run(SCORES), run(CTC), run(TOPK)
    n = int(r_ctc.ctc.n[1])
    assert n >= 1
    targets = [None, [int(v) for v in r_ctc.ctc.ids[1, :n]], []]
    r_beam = run(BEAM)
    hyps = r_beam.beam.hyps(0)
    assert len(hyps) >= 2 and len(hyps[1][0]) >= 1
    hotset = [list(hyps[1][0][:3]), list(r_beam.beam.hyps(1)[0][0][:2]) or [5]]
    for hot in (None, hotset):
        if hot is not None:
            r_beam = run(BEAM, hot=hot)
            assert int(r_beam.beam.matched.max()) >= 1                            # the set does bias this search
        r_al = run(BEAM | ALIGN, targets, hot)
        r_all = run(CTC | TOPK | BEAM | ALIGN, targets, hot)
        np.testing.assert_array_equal(r_all.token_ids, r_plain.token_ids)
        np.testing.assert_array_equal(_bits(r_all.scores), _bits(r_sc.scores))
        for name in ("n", "ids", "first", "last"):
            np.testing.assert_array_equal(getattr(r_all.ctc, name), getattr(r_ctc.ctc, name), err_msg=name)
        np.testing.assert_array_equal(_bits(r_all.ctc.score), _bits(r_ctc.ctc.score))
        np.testing.assert_array_equal(r_all.topk.ids, r_topk.topk.ids)
        np.testing.assert_array_equal(_bits(r_all.topk.val), _bits(r_topk.topk.val))
        np.testing.assert_array_equal(r_all.topk.n, r_topk.topk.n)
        _same_beam(r_all, r_beam, hot is not None)
        _same_beam(r_al, r_beam, hot is not None)
        assert r_all.align.H == 1 + NB and r_all.align.len[:, 0].tolist() == [-1, n, 0]
        _same_align(r_all, r_al)
