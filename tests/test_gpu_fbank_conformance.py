"""GPU: the kaldi fbank kernel (fbank_kernel in csrc/k_frontend.hip, the first thing every utterance of every model meets)
and the LFR / CMVN / padding kernels behind it, at every accepted mode and edge.  All with dither 0.

a) float64 conformance — tests/fbank_ref.py restates the published steps with every intermediate in float64; for every
   frame and bin with E > 4 FLT_EPSILON

       |got - log E| <= K 2^-24 sqrt(max(max_m E[t, m], R0[t]) / E[t, m])

   (a float32 transform leaves an amplitude error proportional to the frame's largest amplitude, so a bin's relative error
   grows as sqrt(E_max / E_bin); R0 = sum raw^2 covers the float32 mean removal of a large DC offset); quieter bins must be
   within the same allowance of the floor, or exactly at it.  Four windows x two framings x eight signal families x the
   lengths around every frame-count and reflection edge, and n_mels 40 and 128.
   K is not tuned on the device: a float32 restatement of the oracle (torch.fft.rfft on float32) run on this suite's own
   inputs on a CPU reaches a worst ratio of 19.64 (16 of it is the rounding of a float32 logarithm between 16 and 32 at
   the loudest bin), and K = 4 x 19.64 = 78.6 (fbank_ref.MEASURED_F32, fbank_ref.K; tests/test_fbank_ref_cpu.py re-measures).
   The kernel's own worst ratio on an MI355X: see DEVICE_WORST below (information, not the source of K).
b) exact answers — silence, exact constants (their DC removal leaves exact zeros) and impulse-free frames sit AT the floor.
c) bit-exact self-consistency, no tolerance — the reflect path against interior frames of a mirrored signal; snip_edges
   against not; every utterance of a batch (pf_op_fbank_batch: the ballot search for B <= 64, the binary search above,
   zero-frame utterances sharing a frame offset, audio offsets rounded up to 4) against the same utterance alone; a batch
   of more than twice the resident grid's frames, so that every wave walks its loop and prefetches; repeatability.
d) pf_op_lfr_cmvn_pad bit-exact at four (lfr_m, lfr_n, n_mels) geometries and the frame counts around lfr_n; pad_sentinel
   (which has no entry point of its own) through Engine.model_proj against forward_feats of numpy's PadSequence.

DEVICE_WORST (MI355X, this suite): 71.2 (hamming, n_mels 80: square wave, n = 400; n_mels 40: 71.2; n_mels 128: 68.8; the
other windows and framings 64.4 .. 68.7; the persistent-loop utterance 66.5).  Nearly all of it is the kernel's logf: the
compiler's v_log_f32 sequence is good to about 2 ulp of a result near 25, i.e. about 64 of these units, and sits about half
an ulp low on average; the transform, the power and the mel sums in the kernel's own order cost at most 6 units (a numpy
float32 walk through the same butterflies).
The reference's mel weights are oracle.frontend.mel_banks(libm_log=True), a correctly rounded logf in the mel scale, which
is what the engine's host code computes.  Against the oracle's default weights (numpy's float32 log, up to 2 ulp off: 69 of
501 weights moved by up to 1.4e-5; kept as the default because the committed golden files were written with them) the same
device output measures 160 (n_mels 128: 323): at this resolution they are another filter bank.
"""
import numpy as np
import pytest
import torch

import fbank_ref as FR
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe

pytestmark = pytest.mark.gpu

HAM, HAM_SNIP = ("hamming", False, 80, 7, 6), ("hamming", True, 80, 7, 6)
MEL40, MEL128 = ("hamming", False, 40, 14, 6), ("hamming", False, 128, 1, 1)        # lfr_m * n_mels = the CMVN's width
A_CONFIGS = [(w, s, 80, 7, 6) for w in FR.WINDOWS for s in (False, True)] + [MEL40, MEL128]


@pytest.fixture(scope="module")
def engines():
    """one 1-layer synthetic engine per (window, snip_edges, n_mels, lfr_m, lfr_n) that a test asks for, closed at the end"""
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    blob = W.pack_pfw(cfg, W.synth_weights(cfg, seed=5))
    made = {}

    def get(key):
        if key not in made:
            window, snip, n_mels, lfr_m, lfr_n = key
            made[key] = Engine(weights=blob, cmvn=W.synth_cmvn(lfr_m * n_mels), device=0, dither=0.0, window=window,
                               snip_edges=snip, n_mels=n_mels, lfr_m=lfr_m, lfr_n=lfr_n)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _same(a, b, what):
    """bit for bit (array_equal alone would let -0.0 pass for 0.0 and fail NaN against the same NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, diff.sum(), diff.size, np.argwhere(diff)[0])


def _at_floor(got, what):
    got = np.asarray(got)
    assert np.isfinite(got).all(), what
    assert got.size == 0 or (got.min() == got.max() and abs(float(got.flat[0]) - FR.LOG_FLOOR) <= 1e-6), \
        (what, float(got.min()), float(got.max()), FR.LOG_FLOOR)


# ------------------------------------------------------------------------------------------ a) float64 conformance
@pytest.mark.parametrize("key", A_CONFIGS, ids=lambda k: "%s-%s-%d" % (k[0], "snip" if k[1] else "nosnip", k[2]))
def test_float64_conformance(engines, key):
    window, snip, n_mels = key[:3]
    eng = engines(key)
    worst, where = 0.0, None
    for name, n in FR.cases(snip):
        E, R0 = FR.reference(name, n, window, snip, n_mels)
        got = eng.fbank(FR.signal(name, n))
        assert got.shape == (fe.num_frames(n, snip), n_mels) == E.shape, (name, n, got.shape)
        r = FR.ratio(got, E, R0)
        if r.size and r.max() > worst:
            worst, where = float(r.max()), (name, n) + tuple(int(i) for i in np.unravel_index(r.argmax(), r.shape))
    print("fbank %s snip_edges=%s n_mels=%d: worst |got - log E| / bound = %.2f at %s (K = %.1f)" % (window, snip, n_mels, worst, where, FR.K))
    assert worst <= FR.K, (worst, where)


@pytest.mark.parametrize("key", [HAM, HAM_SNIP, MEL128], ids=["nosnip", "snip", "mels128"])
def test_frame_counts_and_zero_frame_lengths(engines, key):
    window, snip, n_mels = key[:3]
    eng = engines(key)
    for n in (0, 1, 79, 80, 81, 159, 160, 239, 240, 399, 400, 401, 559, 560, 561, 719, 720):
        got = eng.fbank(FR.signal("synth", n))
        assert got.shape == (fe.num_frames(n, snip), n_mels), (n, got.shape)
        assert np.isfinite(got).all()


def test_filters_without_a_bin_sit_at_the_floor(engines):
    """n_mels = 128: the lowest filters are narrower than one FFT bin (31.25 Hz) and hold none: E == 0 exactly"""
    E, _ = FR.reference("white", 16000, "hamming", False, 128)
    empty = (fe.mel_banks(128, 16000, libm_log=True) == 0).all(axis=1)
    assert empty.any() and not empty.all() and (E[:, empty] == 0).all()
    got = engines(MEL128).fbank(FR.signal("white", 16000))
    _at_floor(got[:, empty], "empty filters")
    assert (got[:, ~empty] > 0).all()


# ------------------------------------------------------------------------------------------ b) exact answers
@pytest.mark.parametrize("key", [(w, s, 80, 7, 6) for w in FR.WINDOWS for s in (False, True)],
                         ids=lambda k: "%s-%s" % (k[0], "snip" if k[1] else "nosnip"))
def test_silence_and_exact_constants_sit_at_the_floor(engines, key):
    """0.25 and -0.5 scale to +-2^13 / 2^14: the frame sum and its mean are exact in float32, the DC removal leaves exact
    zeros — a mean over another count, or a reflected index outside the utterance, leaves energy"""
    eng, snip = engines(key), key[1]
    for n in FR.LENGTHS[snip]:
        for c in (0.0, 0.25, -0.5):
            got = eng.fbank(np.full(n, c, np.float32))
            assert got.shape == (fe.num_frames(n, snip), 80)
            _at_floor(got, (key, n, c))


@pytest.mark.parametrize("key", [HAM, HAM_SNIP], ids=["nosnip", "snip"])
def test_frames_without_an_impulse_sit_at_the_floor(engines, key):
    eng, snip = engines(key), key[1]
    for n in (16000, 560, 401):
        E, R0 = FR.reference("impulses", n, "hamming", snip)
        got = eng.fbank(FR.signal("impulses", n))
        empty = R0 == 0
        assert n != 16000 or 0 < empty.sum() < empty.size
        _at_floor(got[empty], ("impulse-free frames", n))
        assert (got[~empty].max(axis=1) > 0).all()


# ------------------------------------------------------------------------------------------ c) self-consistency
@pytest.mark.parametrize("n", [80, 160, 320, 800])
def test_reflected_edge_frames_equal_interior_frames_of_the_mirrored_signal(engines, n):
    """x on the reflect path against y = ... | x reversed | x | x reversed | ... (the mirror extension written out, two shifts
    = 320 samples of it on either side), where the same frames are interior.  n = 80: every index of the one frame bounces,
    some twice; 160: one frame that reflects at both ends; 320, 800: single reflection at either end."""
    eng = engines(HAM)
    x = FR.signal("synth", n)
    period = np.concatenate([x, x[::-1]])                     # the mirror extension has period 2 n
    pad = 320                                                 # two shifts: frame f of x is frame f + 2 of y
    y = period[np.arange(-pad, n + pad) % (2 * n)]
    t = fe.num_frames(n, False)
    iy = FR.frame_index(n + 2 * pad, False)[2:2 + t]
    assert (iy[:, 0] == 160 * np.arange(t) + 200).all() and iy[-1, -1] < n + 2 * pad      # interior in y
    np.testing.assert_array_equal(x[FR.frame_index(n, False)], y[iy])                      # the definition agrees
    gx, gy = eng.fbank(x), eng.fbank(y)
    assert gx.shape == (t, 80) and gy.shape == (t + 4, 80)
    _same(gx, gy[2:2 + t], "reflect path vs interior path, n = %d" % n)


def test_snip_edges_frames_equal_the_centred_frames_120_samples_later(engines):
    x = FR.signal("synth", 16000)
    a = engines(HAM_SNIP).fbank(x)                            # frame f starts at 160 f
    b = engines(HAM).fbank(x[120:])                           # frame f starts at 160 f - 120 of x[120:] = 160 f of x
    assert a.shape[0] == 98 and b.shape[0] == 99
    # interior in b: 160 f - 120 >= 0 and 160 f + 280 <= 15880, so f = 1 .. 97 (all of them interior in a)
    _same(a[1:98], b[1:98], "snip_edges vs not, frames interior in both")


def _ragged_batch(B, snip, seed):
    """lengths of B utterances: ragged, mostly not divisible by 4; zero-frame utterances first, last, in the middle and
    twice in a row (empty ones and short ones); one utterance of exactly one frame"""
    rng = np.random.default_rng([B, int(snip), seed])
    zero_max, one = (399, 401) if snip else (79, 201)
    n = rng.integers(zero_max + 1, 4000, B)
    n[rng.integers(0, B, max(1, B // 3))] |= 1
    if B == 2:
        n[seed % 2] = 37
        n[1 - seed % 2] = one
    else:
        n[0], n[B - 1], n[B // 2], n[B // 2 + 1], n[1] = 0, zero_max, 0, 37, one
    return [int(v) for v in n]


def _utterances(lengths, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lengths):
        x = (0.2 * rng.standard_normal(n) + 0.05 * (i % 5)).astype(np.float32)     # distinct per utterance, some with DC
        out.append(x)
    return out


@pytest.mark.parametrize("snip", [False, True], ids=["nosnip", "snip"])
@pytest.mark.parametrize("B", [2, 7, 64, 65, 130])
def test_batch_rows_equal_each_utterance_alone(engines, B, snip):
    eng = engines(HAM_SNIP if snip else HAM)
    for seed in ((0, 1) if B == 2 else (0,)):
        lengths = _ragged_batch(B, snip, seed)
        audio = _utterances(lengths, 100 + B)
        got = eng.op_fbank_batch(audio)
        assert len(got) == B
        counts = [g.shape[0] for g in got]
        assert counts == [fe.num_frames(n, snip) for n in lengths]
        assert counts.count(0) >= (1 if B == 2 else 4) and counts.count(1) >= 1
        for b in range(B):
            _same(got[b], eng.fbank(audio[b]), "B = %d, utterance %d of %d samples" % (B, b, lengths[b]))


def test_batch_of_nothing(engines):
    eng = engines(HAM)
    assert eng.op_fbank_batch([]) == []
    got = eng.op_fbank_batch([np.zeros(0, np.float32), np.zeros(79, np.float32)])
    assert [g.shape for g in got] == [(0, 80), (0, 80)]


def test_persistent_loop_rows_equal_each_utterance_alone(engines):
    """more than twice the frames the resident grid holds (4 frames x at most 8 workgroups x CU count): every wave walks
    gf, gf + stride, ... and prefetches; about 40 ragged utterances, one of them empty"""
    eng = engines(HAM)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = 2 * 4 * 8 * cus + 37
    rng = np.random.default_rng(9)
    B = 40
    frames = rng.integers(need // B - 60, need // B + 60, B)
    frames[7] = 0
    frames[B - 1] += max(0, need - int(frames.sum()))
    lengths = [int(f * 160 + rng.integers(-79, 80)) if f else 0 for f in frames]
    assert [fe.num_frames(n, False) for n in lengths] == [int(f) for f in frames] and sum(frames) >= need
    tone = FR.signal("synth", 16000)
    audio = [np.resize(np.roll(tone, 131 * b), n) * np.float32(1 + 0.01 * b) for b, n in enumerate(lengths)]
    got = eng.op_fbank_batch(audio)
    assert [g.shape[0] for g in got] == [int(f) for f in frames]
    for b in range(B):
        _same(got[b], eng.fbank(audio[b]), "utterance %d" % b)
    b = 3                                                     # one of them against the definition
    E, R0 = FR.fbank64(audio[b], "hamming", False)
    worst = float(FR.ratio(got[b], E, R0).max())
    print("persistent loop: %d frames on %d CUs, utterance %d worst ratio %.2f (K = %.1f)" % (sum(frames), cus, b, worst, FR.K))
    assert worst <= FR.K


def test_repeatability(engines):
    eng = engines(HAM)
    x = FR.signal("synth", 16000)
    _same(eng.fbank(x), eng.fbank(x), "fbank twice")
    audio = _utterances(_ragged_batch(7, False, 0), 3)
    a, b = eng.op_fbank_batch(audio), eng.op_fbank_batch(audio)
    for u, v in zip(a, b):
        _same(u, v, "op_fbank_batch twice")


# ------------------------------------------------------------------------------------------ d) LFR, CMVN, padding
@pytest.mark.parametrize("lfr_m,lfr_n,n_mels", [(7, 6, 80), (1, 1, 80), (5, 3, 80), (14, 6, 40)])
def test_lfr_cmvn_pad_bit_exact_at_other_geometries(engines, lfr_m, lfr_n, n_mels):
    eng = engines(("hamming", False, n_mels, lfr_m, lfr_n))
    width = lfr_m * n_mels
    shift, scale = W.synth_cmvn(width)
    rng = np.random.default_rng([lfr_m, lfr_n, n_mels])
    t80s = [0, lfr_n - 1, lfr_n, lfr_n + 1, 301, 2 * lfr_n + lfr_m]
    fbs = [rng.standard_normal((t, n_mels)).astype(np.float32) for t in t80s]
    row, slot, col = 3, lfr_m // 2, 5                          # LFR row 3 of the long one: make one CMVN result an exact 0
    frame = row * lfr_n + slot - (lfr_m - 1) // 2
    fbs[4][frame, col] = -shift[slot * n_mels + col]
    feats = [fe.apply_cmvn(fe.apply_lfr(f, lfr_m, lfr_n, n_mels), shift, scale) if f.shape[0] >= lfr_n
             else np.zeros((0, width), np.float32) for f in fbs]
    assert [f.shape[0] for f in feats] == [t // lfr_n for t in t80s] and feats[4][row, slot * n_mels + col] == 0
    exp = fe.pad_sequence(feats).reshape(len(fbs), -1, width)
    got = eng.op_lfr_cmvn_pad(fbs, sentinel=True)
    _same(got, exp, "lfr_cmvn_pad with the sentinel")
    assert got[4, row, slot * n_mels + col] == fe.PAD_SENTINEL and (got[0] == fe.PAD_SENTINEL).all()
    exp0 = exp.copy()
    exp0[exp0 == fe.PAD_SENTINEL] = 0
    _same(eng.op_lfr_cmvn_pad(fbs, sentinel=False), exp0, "lfr_cmvn_pad without the sentinel")
    # nothing but utterances too short for one LFR row: an empty result, no launch
    assert eng.op_lfr_cmvn_pad([f for f in fbs[:2]], sentinel=True).shape == (2, 0, width)


def test_pad_sentinel_replaces_padding_and_genuine_zeros(engines):
    """pad_sentinel_kernel is reached through pf_model_proj only: ragged feature buffers in, the model's logits out.  Against
    pf_forward_feats of numpy's PadSequence of the same buffers the logits must be bit-identical; the same batch with the
    zeros left in place is far away, so the comparison does see the replacement."""
    eng = engines(HAM)
    shift, scale = W.synth_cmvn()
    conf = fe.FrontendConf(dither=0.0)
    feats = [fe.wav_frontend(W.synth_audio(n, 20 + i), conf, shift, scale).copy() for i, n in enumerate((16000, 9000, 12345))]
    assert [f.shape[0] for f in feats] == [16, 9, 12]
    feats[0][5, 7] = 0.0                                       # genuine zeros: in the longest utterance, in a padded one,
    feats[1][0, 0] = 0.0                                       # and in the last valid row
    feats[2][11, 559] = 0.0
    padded = fe.pad_sequence(feats).reshape(3, 16, 560)
    assert (padded == fe.PAD_SENTINEL).sum() == 3 + (7 + 4) * 560
    a = eng.model_proj(feats, want_logits=True)
    b = eng.forward_feats(padded, want_logits=True)
    assert a.L == b.L and a.L > 0
    np.testing.assert_array_equal(a.token_num, b.token_num)
    np.testing.assert_array_equal(a.token_ids, b.token_ids)
    _same(a.logits, b.logits, "model_proj vs forward_feats of PadSequence")
    zeros_left = padded.copy()
    zeros_left[zeros_left == fe.PAD_SENTINEL] = 0
    c = eng.forward_feats(zeros_left, want_logits=True)
    assert c.L != a.L or np.abs(c.logits - a.logits).max() > 1e-2
