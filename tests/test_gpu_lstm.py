"""GPU: every form in which the engine runs the (Bi)LSTM recurrence of its heads, and the timestamp head's tail, as operators
(pf_op_lstm, pf_op_us_peak: the functions the heads call, not copies) against tests/lstm_ref.py.

  form 0  what Engine::timestamp_head chooses: the ring when it fits, else T3 step launches as a cached, replayed hipGraph (B > 64)
  form 1  lstm_step_kernel, plain launches (the hot-word embedder)
  form 2  lstm_ring_kernel<false>: one persistent launch, h exchanged between 64 workgroups through a four-slot poison ring
  form 3  lstm_ring_kernel<true>: the same ring with (hi, lo') pair operands (math_mode 3)
  form 4  launch_gemm_f32 + lstm_cell_f32_kernel per step (math_mode 1, and the fallback of mode 3)

No bound below is a constant: each is computed from the reference alone, as a multiple of the distance between a float32 and a
float64 evaluation of the same model on the same input (what fp32 evaluation order — and, for f16 operands, the re-rounding
flips it causes — costs); the device's measured error stands beside it.  Every comparison takes all elements; the operators
NaN-fill their outputs first, so an element that was never written fails every test here.

Inputs: xg ~ N(0, 1), W_hh ~ N(0, 1) / sqrt(D) per direction (as synth_weights), and the same at gain 3, where the recurrent term
dominates the gates and a stale or misrouted h cannot hide behind xg."""
import functools

import numpy as np
import pytest

import lstm_ref as LR
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu
D = 512
GAINS = (1, 3)
MODE_OF_FORM = {0: 0, 1: 0, 2: 0, 3: 3, 4: 1}
STALE = np.arange(8, 16)                               # one producer workgroup's granule: hidden units 8 .. 15


@pytest.fixture(scope="module")
def engines():
    """one tiny engine per math mode (created on first use), as _tiny_engine of test_gpu_fp32_mode.py"""
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    blob, cmvn = W.pack_pfw(cfg, W.synth_weights(cfg, seed=1)), W.synth_cmvn()
    made = {}

    def get(form):
        mode = MODE_OF_FORM[form]
        if mode not in made:
            made[mode] = Engine(weights=blob, cmvn=cmvn, device=0, math_mode=mode)
        return made[mode]
    yield get
    for e in made.values():
        e.close()


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _inputs(B, T3, ndir, gain, variant=0):
    rng = np.random.default_rng([B, T3, ndir, gain, variant])
    xg = rng.standard_normal((B, T3, ndir * 4 * D), dtype=np.float32)
    whh = (np.float32(gain) * rng.standard_normal((ndir, 4 * D, D), dtype=np.float32) / np.float32(np.sqrt(D))).astype(np.float32)
    return _frozen(xg), _frozen(whh)


@functools.lru_cache(maxsize=None)
def _ref(B, T3, ndir, gain, variant, operands):
    """(float64 reference, distance of the float32 rerun from it) of one input; computed once, shared, read-only"""
    xg, whh = _inputs(B, T3, ndir, gain, variant)
    ref = LR.lstm_ref(xg, whh, ndir, np.float64, operands)
    rerun = float(np.abs(LR.lstm_ref(xg, whh, ndir, np.float32, operands) - ref).max())
    return _frozen(ref), rerun


def _check_f16(eng, form, B, T3, ndir, gain, variant=0):
    """forms 0, 1, 2 against lstm_ref(float64, "f16").  Bound: 4 x the float32 rerun's distance on this input — that distance
    already holds the f16 re-rounding flips that dominate; the kernel's __expf, its K-split summation order and its tanhf add
    terms of fp32-rounding size.

    The rerun's distance is floored at the size of ONE flip, 2^-11 max|W_hh|: an h operand that lands on the neighbouring f16
    (one ulp, at most 2^-11 below 1) moves a gate by at most that times the largest weight, and the cell's slope is at most 1.
    Why: whether the float32 rerun contains a flip at all is chance on a small input.  B = 1, T3 = 6, gain 3 re-rounds 2560
    operands; the rerun happened to flip none (distance 1.7e-7, pure fp32 rounding, bound 6.7e-7) while the device flipped
    one and measured 5.8e-5 — a single flip's size (ulp 2.4e-4 x weight 0.4 x slope), not an error of the kernel.  The floor
    is 1.0e-4 at gain 1 and 3.0e-4 at gain 3; the stale-h perturbation still lies 10 x above every bound."""
    xg, whh = _inputs(B, T3, ndir, gain, variant)
    ref, rerun = _ref(B, T3, ndir, gain, variant, "f16")
    flip = 2.0 ** -11 * float(np.abs(whh.astype(np.float16).astype(np.float64)).max())
    bound = 4.0 * max(rerun, flip)
    stale = float(np.abs(LR.lstm_ref(xg, whh, ndir, np.float64, "f16", hook=LR.stale_units(STALE)) - ref).max())
    got = eng.op_lstm(xg, whh, ndir, form)
    err = float(np.abs(got - ref).max())
    print("lstm form %d B %d T3 %d ndir %d gain %d: err %.3g bound %.3g (rerun %.3g, one flip %.3g) stale %.3g" %
          (form, B, T3, ndir, gain, err, bound, rerun, flip, stale))
    # the bound can see the failure it is there for: 8 of 512 units fed h from one step too early.  (T3 = 1 has no earlier step:
    # every form reads h_{-1} = 0 there and the perturbation is the identity)
    if T3 > 1:
        assert stale > 10.0 * bound, (stale, bound)
    else:
        assert stale == 0.0
    assert err < bound, (err, bound)


RING_CASES = [(B, 24, 2) for B in (1, 31, 32, 33, 40, 64)] + [(3, T3, 2) for T3 in (1, 2, 3, 4, 5, 7, 96)] + [(5, 9, 1)]
STEP_CASES = [(1, 6, 1), (4, 6, 1), (33, 6, 1), (40, 24, 2)]          # T3 = 6, ndir = 1: the hot-word embedder's shape class


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("B,T3,ndir", RING_CASES)
def test_f16_ring_against_float64(engines, B, T3, ndir, gain):
    """Tile edges (B = 31, 32, 33, 64; the ragged-tile clamp at 33 and 40) and the ring's slot arithmetic before, at and after
    its first wrap (T3 = 1 .. 5, 7), and long after (96).  measured at T3 = 24, worst B: 7.0e-5 (4 x rerun 2.9e-4) at gain 1, 9.2e-4
    (4.0e-3) at gain 3; T3 = 96: 5.5e-5 / 7.7e-4; T3 = 1 .. 3, where no operand flipped: 8.0e-8 .. 1.2e-7"""
    _check_f16(engines(2), 2, B, T3, ndir, gain)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("B,T3,ndir", STEP_CASES)
def test_f16_step_launches_against_float64(engines, B, T3, ndir, gain):
    """measured: 9.3e-6 .. 7.0e-5 (4 x rerun 3.7e-5 .. 2.9e-4) at gain 1, 5.8e-5 .. 9.2e-4 at gain 3 (B = 1: one flip against a
    rerun without any, see _check_f16)"""
    _check_f16(engines(1), 1, B, T3, ndir, gain)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("B", [65, 70])
def test_automatic_form_above_64_utterances_captures_then_replays(engines, B, gain):
    """B > 64: the ring does not fit and timestamp_head's recurrence runs as a captured graph of step launches.  The first call
    captures it, the second (same shape and buffers, other data) replays the cached one — and must return the second input's
    result.  measured: 5.5e-5 .. 8.1e-5 (4 x rerun 2.2e-4 .. 2.8e-4) at gain 1, 7.6e-4 .. 1.1e-3 (3.0e-3 .. 3.6e-3) at gain 3"""
    for variant in (0, 1):
        _check_f16(engines(0), 0, B, 24, 2, gain, variant)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("T3", [1, 5, 24])
@pytest.mark.parametrize("B", [1, 33, 40, 64])
def test_pair_ring_against_float64(engines, B, T3, gain):
    """form 3 against lstm_ref(float64, "exact").  Bound: 32 x the float32 rerun's distance — pair operands carry 22 of fp32's 24
    bits and h is re-split every step.  The bound must also separate pair operands from single f16 ones: it lies below an eighth
    of the distance between the f16-operand model and the unrounded one.  measured: 7.0e-8 .. 1.9e-7 (bound 2.6e-6 .. 9.6e-6) at
    gain 1, 7.1e-8 .. 6.4e-7 (2.6e-6 .. 3.8e-5) at gain 3 — below the float32 rerun's own distance in every case"""
    xg, whh = _inputs(B, T3, 2, gain)
    ref, rerun = _ref(B, T3, 2, gain, 0, "exact")
    bound = 32.0 * rerun
    f16_gap = float(np.abs(_ref(B, T3, 2, gain, 0, "f16")[0] - ref).max())
    got = engines(3).op_lstm(xg, whh, 2, 3)
    err = float(np.abs(got - ref).max())
    print("lstm form 3 B %d T3 %d gain %d: err %.3g bound %.3g (rerun %.3g) f16 gap %.3g" % (B, T3, gain, err, bound, rerun, f16_gap))
    if T3 > 1:
        assert bound < f16_gap / 8.0, (bound, f16_gap)
    else:
        assert f16_gap == 0.0                          # one step: the only recurrent operand is h_{-1} = 0, no rounding to tell apart
    assert err < bound, (err, bound)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("T3", [1, 24])
@pytest.mark.parametrize("B", [1, 33, 70])
def test_fp32_recurrence_against_float64(engines, B, T3, gain):
    """form 4 against lstm_ref(float64, "exact").  Bound: 8 x the float32 rerun's distance.  measured: 6.4e-8 .. 3.6e-7 (bound 6.5e-7 ..
    2.1e-6) at gain 1, 7.1e-8 .. 2.1e-6 (6.6e-7 .. 9.7e-6) at gain 3"""
    xg, whh = _inputs(B, T3, 2, gain)
    ref, rerun = _ref(B, T3, 2, gain, 0, "exact")
    bound = 8.0 * rerun
    got = engines(4).op_lstm(xg, whh, 2, 4)
    err = float(np.abs(got - ref).max())
    print("lstm form 4 B %d T3 %d gain %d: err %.3g bound %.3g (rerun %.3g)" % (B, T3, gain, err, bound, rerun))
    assert err < bound, (err, bound)


@pytest.mark.parametrize("form", [2, 3])
def test_rings_decline_65_utterances_and_the_engine_stays_usable(engines, form):
    eng = engines(form)
    xg, whh = _inputs(65, 24, 2, 1)
    with pytest.raises(N.PfError) as ei:
        eng.op_lstm(xg, whh, 2, form)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED, ei.value
    xg, whh = _inputs(3, 5, 2, 1)
    ref, rerun = _ref(3, 5, 2, 1, 0, "f16" if form == 2 else "exact")
    got = eng.op_lstm(xg, whh, 2, form)
    assert np.abs(got - ref).max() < (4.0 if form == 2 else 32.0) * rerun


# ---- exact-answer checks: bit equality -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [2, 3])
def test_ring_is_deterministic(engines, form):
    """A race in the exchange shows here before it shows anywhere else."""
    xg, whh = _inputs(40, 24, 2, 3)
    a = engines(form).op_lstm(xg, whh, 2, form)
    b = engines(form).op_lstm(xg, whh, 2, form)
    assert not np.isnan(a).any()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_rows_do_not_depend_on_the_batch(engines, form):
    """An utterance is one MFMA column: nothing may leak between columns or between the two tiles of a B = 40 run."""
    xg, whh = _inputs(40, 24, 2, 3)
    full = engines(form).op_lstm(xg, whh, 2, form)
    assert not np.isnan(full).any()
    for b in (0, 31, 32, 39):
        one = engines(form).op_lstm(xg[b:b + 1], whh, 2, form)
        assert np.array_equal(one[0], full[b]), b


@pytest.mark.parametrize("form", [1, 2, 3, 4])
def test_directions_are_symmetric(engines, form):
    """whh[1] = whh[0] and direction 1's gate inputs the time reversal of direction 0's: the reverse hidden sequence is the
    forward one read backwards, bit for bit."""
    xg0, whh0 = _inputs(33, 7, 2, 3)
    xg = xg0.copy()
    xg[:, :, 4 * D:] = xg[:, ::-1, :4 * D]
    whh = np.stack([whh0[0], whh0[0]])
    h = engines(form).op_lstm(xg, whh, 2, form)
    assert not np.isnan(h).any()
    assert np.array_equal(h[:, ::-1, D:], h[:, :, :D])


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("B,T3,ndir", [(40, 24, 2), (33, 5, 2), (64, 7, 2), (5, 9, 1)])
def test_ring_equals_step_launches(engines, B, T3, ndir, gain):
    """Forms 1 and 2 issue the same MFMA sequence per wave, the same reduction tree and the same cell expression
    (the compiled cell arithmetic of the two kernels is the same instruction sequence, down to the contracted multiply-add of the
    cell state and the single rounding of h to f16): bit-identical on the device, 0 of up to 983040 elements differ."""
    xg, whh = _inputs(B, T3, ndir, gain)
    ring = engines(2).op_lstm(xg, whh, ndir, 2)
    step = engines(1).op_lstm(xg, whh, ndir, 1)
    print("ring vs step B %d T3 %d gain %d: max |diff| %.3g, %d of %d elements differ" %
          (B, T3, gain, np.abs(ring - step).max(), int((ring != step).sum()), ring.size))
    assert np.array_equal(ring, step)


# ---- the tail: us_alpha_kernel, us_peak_kernel -------------------------------------------------------------------------------------

SMOOTH, NOISE, B0 = 0.25, 0.01, 0.3                    # cif_smooth2, cif_noise2 and predictor.out2.bias of synth_weights
THR = np.float32(np.float32(1.0) - np.float32(1e-4))   # cif_threshold - 1e-4 as the heads pass it


@functools.lru_cache(maxsize=None)
def _tail_inputs(rows, Wd, seed=0):
    rng = np.random.default_rng([rows, Wd, seed])
    hout = rng.uniform(-1.0, 1.0, (rows, Wd)).astype(np.float32)
    w = (rng.standard_normal(Wd, dtype=np.float32) * np.float32(4.0 / np.sqrt(Wd))).astype(np.float32)   # predictor.out2.weight's scale
    return _frozen(hout), _frozen(w)


@functools.lru_cache(maxsize=None)
def _alpha_ref(Wd):
    hout, w = _tail_inputs(257, Wd, seed=1)
    ref = LR.us_alpha_ref(hout, w, B0, SMOOTH, NOISE)
    rerun = float(np.abs(LR.us_alpha_ref(hout, w, B0, SMOOTH, NOISE, np.float32) - ref).max())
    return _frozen(ref), rerun


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("Wd", [1024, 512, 4])
def test_us_alpha_against_float64(engines, rows, Wd):
    """alphas_raw against us_alpha_ref in float64.  Bound: 4 x the float32 rerun's distance, taken once per width on the 257-row
    input whose first `rows` rows every case runs (one element gives no estimate of a maximum).  rows = 1, 3, 5: a block of four
    waves with idle ones; 257: more than one block.  measured: 3.6e-8 (bound 2.4e-7) at W = 1024, 3.4e-8 (2.2e-7) at 512,
    2.2e-8 (7.8e-8) at 4"""
    hout, w = _tail_inputs(257, Wd, seed=1)
    ref, rerun = _alpha_ref(Wd)
    assert ref[0] > 0 and (ref == 0).any() == (Wd != 4)      # the relu clips some frames (not at W = 4); the first row is never all zero
    raw, _, _ = engines(0).op_us_peak(hout[None, :rows], w, B0, SMOOTH, NOISE, [1], THR)
    err = float(np.abs(raw[0] - ref[:rows]).max())
    print("us_alpha rows %d W %d: err %.3g bound %.3g (rerun %.3g)" % (rows, Wd, err, 4.0 * rerun, rerun))
    assert err < 4.0 * rerun, (err, rerun)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T3", [1, 63, 64, 65, 300])
def test_us_peak_is_bit_equal_to_the_float32_model(engines, T3, B):
    """alphas and peak against us_peak_ref fed the device's own alphas_raw: bit equality.  token_num holds 0, 1 and values above
    the raw sum (the renormalisation scales up and fires land in consecutive frames)."""
    # the seed is picked here, on the CPU: the first whose rows all carry weight (an all-zero row divides by zero on both sides
    # and proves nothing; at T3 = 1 a row is one frame, which the relu clips once in sixteen)
    for seed in range(1, 100):
        hout, w = _tail_inputs(B * T3, 1024, seed)
        if (LR.us_alpha_ref(hout, w, B0, SMOOTH, NOISE).reshape(B, T3).sum(axis=1) > 0.01).all():
            break
    token_num = np.asarray([int(0.8 * T3) + 1, 0, 1, int(0.3 * T3) + 2, 3][:B], np.int32)
    raw, alphas, peak = engines(0).op_us_peak(hout.reshape(B, T3, 1024), w, B0, SMOOTH, NOISE, token_num, THR)
    assert (raw.sum(axis=1) > 0).all() and not np.isnan(raw).any()
    assert token_num[0] > raw[0].sum()
    # the one condition of bit equality: the float64 sum of a row rounds to the same float32 sequentially and in the kernel's
    # lane-strided + xor-tree order (the orders differ by ~1e-16 relative: only a sum on a float32 rounding boundary can fail
    # this, and then another seed is the answer)
    seq, tree = LR.us_sums(raw)
    assert np.array_equal(seq, tree), "pick another seed"
    want_a, want_p = LR.us_peak_ref(raw, token_num, THR)
    fires = want_p[0] >= THR
    assert T3 == 1 or (fires[1:] & fires[:-1]).any()
    assert np.array_equal(alphas, want_a)
    assert np.array_equal(peak, want_p)
