"""GPU: voice-activity segmentation on the device (csrc/k_vad.hip; Engine.op_vad_levels / op_vad_segments / vad_segment)
against the definition in numpy (tests/vad_ref.py).  Every value is an integer, so every comparison is exact.

Shapes: the level kernel serves 8 rows per workgroup (T = 0, 1, 63, 64, 65, 1025: none, one, around a workgroup multiple,
many) in its 16-byte-load form (n_mels % 4 == 0) and its 4-byte form; the segment kernel walks 64-frame chunks with a
256-frame history (T around the window, around 1024, 4097, and 70001 = 1094 chunks), several utterances per launch."""
import numpy as np
import pytest

import vad_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


def _pairs(a):
    return [tuple(p) for p in np.asarray(a).tolist()]


def _check(eng, levels_list, c, n_mels=80, tag=""):
    got = eng.op_vad_segments(levels_list, n_mels, c)
    for b, e in enumerate(levels_list):
        assert _pairs(got[b]) == R.segments(e, n_mels, c), (tag, b, len(e), c)
    return got


# ---- step 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 63, 64, 65, 1025])
def test_levels_equal_the_definition(eng, T):
    x = R.special_rows(T, 80, seed=T)
    np.testing.assert_array_equal(eng.op_vad_levels(x), R.levels(x))
    for m in (3, 128):                                             # the 4-byte form; more than one round of 16-byte loads
        x = R.special_rows(min(T, 70), m, seed=T + m)
        np.testing.assert_array_equal(eng.op_vad_levels(x), R.levels(x))


# ---- steps 2-6 ------------------------------------------------------------------------------------------------------
def test_three_utterances_of_different_length_in_one_call(eng):
    rng = np.random.default_rng(1)
    lv = [R.telegraph(rng, T, mean_run=120, jitter=50) for T in (1500, 333, 2801)]
    got = _check(eng, lv, R.config())
    assert sum(len(g) for g in got) >= 6


EXTREME = [dict(window=1, on_count=1, off_count=1, pad_begin=0, pad_end=0, split_search=0, min_speech=12, max_len=24),
           dict(window=256, on_count=256, off_count=1, pad_begin=1024, pad_end=1024, min_speech=12, max_len=1048, split_search=1024),
           dict(window=256, on_count=1, off_count=256, floor_pct=100, abs_level=9000, margin_q=-300),
           dict(floor_pct=-1, abs_level=10000, window=64, on_count=33, off_count=32, pad_begin=0, pad_end=1024, min_speech=12,
                max_len=40, split_search=16),
           dict(floor_pct=0, margin_q=0, window=65, on_count=40, off_count=30, pad_begin=64, pad_end=63, max_len=101, split_search=1,
                min_speech=50)]


@pytest.mark.parametrize("over", [{}] + EXTREME, ids=lambda o: "default" if not o else "-".join("%s%d" % (k[:2], v) for k, v in list(o.items())[:4]))
def test_every_length_edge_in_one_launch(eng, over):
    """T around the window (19, 20, 21), around a chunk multiple (1023 .. 1025), 4097 and 70001, empty and one frame: ten
    utterances, one launch."""
    rng = np.random.default_rng(2)
    lv = [R.telegraph(rng, T, mean_run=int(rng.choice([8, 90, 700])), jitter=int(rng.choice([0, 30]))) if T else np.zeros(0, np.int32)
          for T in (0, 1, 19, 20, 21, 1023, 1024, 1025, 4097, 70001)]
    got = _check(eng, lv, R.config(**over))
    assert len(got[0]) == 0 and len(got[-1]) > 10


def test_known_answers(eng):
    for tag, e, over, want in R.known_answers():
        if over.get("min_speech", 50) < 12:                        # below 2 * lfr_n of this engine's front-end
            with pytest.raises(N.PfError) as ei:
                eng.op_vad_segments([e], 80, over)
            assert ei.value.code == N.PF_ERR_INVALID_ARG
            continue
        assert _pairs(eng.op_vad_segments([e], 80, over)[0]) == want, tag


def test_run_ending_at_T_and_all_speech(eng):
    c = R.config(floor_pct=-1, abs_level=100)
    lv = [R.lv((R.Q, 100), (R.S, 200)), R.lv((R.S, 64)), R.lv((R.S, 128)), R.lv((R.Q, 64), (R.S, 64)), R.lv((R.S, 49)), R.lv((R.S, 50)), R.lv((R.Q, 3000), (R.S, 20))]
    got = _check(eng, lv, c)
    assert _pairs(got[0]) == [(84, 300)] and _pairs(got[1]) == [(0, 64)] and _pairs(got[4]) == [] and _pairs(got[5]) == [(0, 50)]


def test_long_run_with_tied_minima(eng):
    """A constant level over a long run: every cut is a tie over the whole search window and goes to its largest frame; a
    window of ties whose minimum is not the level at its edge; levels at the ends of the int32 range."""
    c = R.config(floor_pct=-1, abs_level=100)
    flat = R.lv((R.Q, 40), (R.S, 10000), (R.Q, 40))
    got = _check(eng, [flat], c)
    assert _pairs(got[0])[:2] == [(24, 3024), (3024, 6024)]
    dips = flat.copy()
    dips[2600:2700:7] = 150                                         # equal minima, the last one wins
    dips[5900] = 150
    dips[5950] = 101
    wide = np.where(flat > 0, np.int32(2**31 - 1), np.int32(-2**31)).astype(np.int32)
    wide[3000:3005] = 2**31 - 2
    _check(eng, [dips, wide, flat], c)
    _check(eng, [dips], R.config(floor_pct=-1, abs_level=100, max_len=700, split_search=64, min_speech=300))
    _check(eng, [wide], R.config())                                 # the percentile over the extreme keys


def test_capacity_too_small_reports_the_counts(eng):
    rng = np.random.default_rng(4)
    lv = [R.telegraph(rng, 3000, mean_run=150), R.lv((R.Q, 100), (R.S, 200), (R.Q, 100))]
    want = [R.segments(e, 80, R.config()) for e in lv]
    assert len(want[0]) > 2 and len(want[1]) == 1
    with pytest.raises(N.PfError) as ei:
        eng.op_vad_segments(lv, 80, None, cap=2)
    assert ei.value.code == N.PF_ERR_CAPACITY
    assert ei.value.n.tolist() == [len(w) for w in want]
    assert _pairs(ei.value.seg[0]) == want[0][:2] and _pairs(ei.value.seg[1][:1]) == want[1]
    assert (ei.value.seg[1][1:] == -7).all()                       # nothing is written past a row's own count
    got = eng.op_vad_segments(lv, 80, None, cap=len(want[0]))      # exactly enough
    assert [_pairs(g) for g in got] == want


def test_fuzz_random_configurations(eng):
    rng = np.random.default_rng(77)
    for it in range(12):
        c = R.random_config(rng, 6)
        lv = [R.telegraph(rng, int(rng.integers(1, 3001)), mean_run=int(rng.choice([3, 15, 60, 400])), jitter=int(rng.choice([0, 3, 4000])))
              for _ in range(6)]
        _check(eng, lv, c, n_mels=int(rng.choice([80, 1, 128])), tag=it)


def test_refusals(eng):
    e = R.lv((R.Q, 100), (R.S, 200), (R.Q, 100))
    for over in (dict(window=0), dict(on_count=10, off_count=10), dict(pad_end=1025), dict(max_len=599), dict(floor_pct=101)):
        with pytest.raises(N.PfError) as ei:
            eng.op_vad_segments([e], 80, over)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, over
        with pytest.raises(N.PfError) as ei:
            eng.vad_segment([np.zeros(16000, np.float32)], over)
        assert ei.value.code == N.PF_ERR_INVALID_ARG, over


# ---- end to end -----------------------------------------------------------------------------------------------------
BURSTS = [(200, 500), (800, 1000), (1400, 1800)]


def test_end_to_end_equals_the_definition_on_the_engines_rows(eng):
    """20 s with three bursts and 7 s with one, one call: pf_vad_segment == the definition applied to the rows the batched fbank
    returns for the same samples; one segment per burst [f0, f1), begin within 4 frames of f0 - 16, end within 4 of f1 + 19."""
    audio = [R.burst_audio(20, BURSTS, 1), R.burst_audio(7, [(100, 400)], 2)]
    rows = eng.op_fbank_batch(audio)
    assert [r.shape[0] for r in rows] == [2000, 700]
    want = [R.segments(R.levels(r), 80, R.config()) for r in rows]
    eng.profile(True)
    eng.profile_reset()
    got = eng.vad_segment(audio)
    vad_ms, vad_n, _ = eng.profile_get("vad")
    _fb_ms, fb_n, _ = eng.profile_get("fbank")
    eng.profile(False)
    assert [_pairs(g) for g in got] == want
    assert vad_n == 2 and fb_n == 1 and vad_ms > 0                  # one batched fbank launch, the two detector launches
    for segs, bursts in zip(want, (BURSTS, [(100, 400)])):
        assert len(segs) == len(bursts), segs
        for (b, e), (f0, f1) in zip(segs, bursts):
            assert abs(b - (f0 - 16)) <= 4 and abs(e - (f1 + 19)) <= 4, (segs, bursts)
    # a configuration that splits, a silent stream, an empty one and one below a frame, in one call
    c = dict(max_len=300, split_search=100, min_speech=50)
    audio2 = [audio[0], (0.001 * np.random.default_rng(3).standard_normal(48000)).astype(np.float32), np.zeros(0, np.float32),
              np.zeros(50, np.float32)]
    rows2 = eng.op_fbank_batch(audio2)
    got2 = eng.vad_segment(audio2, c)
    assert [_pairs(g) for g in got2] == [R.segments(R.levels(r), 80, R.config(**c)) for r in rows2]
    assert len(got2[0]) > 3 and len(got2[1]) == len(got2[2]) == len(got2[3]) == 0
    with pytest.raises(N.PfError) as ei:
        eng.vad_segment(audio, cap=1)
    assert ei.value.code == N.PF_ERR_CAPACITY


def test_snip_edges_front_end_is_unsupported():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0, snip_edges=True)
    try:
        with pytest.raises(N.PfError) as ei:
            e.vad_segment([np.zeros(16000, np.float32)])
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    finally:
        e.close()
