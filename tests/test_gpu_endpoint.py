"""GPU: the streaming endpoint kernel (csrc/k_endpoint.hip; Engine.op_endpoint_update) against the definition in numpy
(tests/endpoint_ref.py).  Every value is an integer, so every comparison is exact — the events, the status and the state block
after every launch.

Shapes: the kernel walks a stream's new frames in 64-frame chunks and carries everything else in the state block, so what can
go wrong sits at the chunk and launch boundaries: n_new of 0, 1, 59, 60, 63, 64, 65, 128 and 257 per launch (none, one, around a
chunk, two chunks, four chunks and a frame), a different one per stream in the same launch, state carried over 27 launches
(about 2 000 frames per stream).  No long audio: nothing in the kernel depends on the stream's age."""
import numpy as np
import pytest

import endpoint_ref as R
import vad_ref as V
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from aliparaformerasr_amd.engine import host_endpoint_update

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 59, 60, 63, 64, 65, 128, 257)
S, Q, lv = V.S, V.Q, V.lv


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=3)), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()


def _triples(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


def _walk(eng, signals, plan, c, n_mels=80, flush_at=None, form=lambda k: "device", tag=""):
    """Feeds stream b its next plan[k][b] frames in launch k (flush_at: {stream: launch}) — to the definition one stream at a
    time, to the device all streams in ONE launch (form(k) == "host": the host twin instead, on the same state blocks) — and
    compares events, status and state blocks after every launch.  Returns every stream's events."""
    B = len(signals)
    flush_at = flush_at or {}
    ref = np.zeros((B, R.STATE_INTS), np.int32)
    dev = np.zeros((B, R.STATE_INTS), np.int32)
    pos, out = [0] * B, [[] for _ in range(B)]
    for k, sizes in enumerate(plan):
        pieces = [signals[b][pos[b]: pos[b] + sizes[b]] for b in range(B)]
        flush = [flush_at.get(b) == k for b in range(B)]
        want = [R.update(ref[b], pieces[b], flush[b], n_mels, c) for b in range(B)]
        if form(k) == "device":
            ev, ins, ob = eng.op_endpoint_update(dev, pieces, flush, n_mels, c)
        else:
            got = [host_endpoint_update(dev[b], pieces[b], flush[b], n_mels, c) for b in range(B)]
            ev, ins, ob = [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]
        for b in range(B):
            assert (_triples(ev[b]), int(ins[b]), int(ob[b])) == want[b], (tag, "launch", k, "stream", b, sizes[b], form(k))
            pos[b] += len(pieces[b])
            out[b] += want[b][0]
        np.testing.assert_array_equal(dev, ref, err_msg=str((tag, "launch", k, form(k))))
    return out


def _ten_streams(seed):
    rng = np.random.default_rng(seed)
    signals = [V.telegraph(rng, 2200, mean_run=int(rng.choice([15, 60, 120])), jitter=int(rng.choice([0, 50, 4000]))) for _ in range(10)]
    plan = [[SIZES[(b + k) % 9] for b in range(9)] + [100 if k <= 13 else 0] for k in range(27)]
    return signals, plan, {9: 13, 0: 26, 4: 26}                     # stream 9 is flushed midway and then gets nothing


CONFIGS = [("defaults", {}),
           ("short sentences", dict(max_len=150, end_silence=20, min_speech=20, pad_begin=10)),
           ("absolute level", dict(rise=-1, abs_level=9000, max_len=3000)),
           ("window 1", dict(window=1, on_count=1, off_count=1, pad_begin=0, pad_end=0, end_silence=1, min_speech=12, max_len=24)),
           ("window 256", dict(window=256, on_count=40, off_count=217, pad_begin=1024, pad_end=5, end_silence=70, max_len=1025)),
           ("window 256, slow to switch off", dict(window=256, on_count=1, off_count=256, rise=0, margin_q=20, pad_begin=1024, max_len=1100)),
           ("end_silence == pad_end", dict(end_silence=30, pad_end=30, max_len=400)),
           ("chunk-sized", dict(window=64, on_count=33, off_count=32, pad_begin=64, pad_end=63, end_silence=64, min_speech=64, max_len=128,
                                rise=50, margin_q=0))]


@pytest.mark.parametrize("tag,over", CONFIGS, ids=[t for t, _ in CONFIGS])
def test_ten_streams_over_27_launches(eng, tag, over):
    c = R.config(**over)
    assert R.valid(c)
    signals, plan, flush_at = _ten_streams(len(tag))
    out = _walk(eng, signals, plan, c, flush_at=flush_at, tag=tag)
    assert sum(len(o) for o in out) >= 4, (tag, [len(o) for o in out])        # (the signals do give events under this configuration)


@pytest.mark.parametrize("first", ["device", "host"])
def test_streams_alternate_between_the_host_twin_and_the_device(eng, first):
    other = "host" if first == "device" else "device"
    for over in ({}, dict(max_len=150, end_silence=20, min_speech=20, pad_begin=10, rise=7)):
        signals, plan, flush_at = _ten_streams(5)
        out = _walk(eng, signals, plan, R.config(**over), flush_at=flush_at, form=lambda k: first if k % 2 == 0 else other, tag=first)
        assert sum(len(o) for o in out) >= 10


def test_events_and_forced_cuts_on_launch_boundaries(eng):
    # "one burst" closes at t = 393, the forced cut of max_len = 200 falls on t = 283 and t = 483 (tests/test_endpoint_cpu.py)
    burst, long_run = lv((Q, 100), (S, 200), (Q, 100)), lv((Q, 100), (S, 400), (Q, 100))
    for cut in (393, 394):                                           # the event on the first / on the last frame of a launch
        out = _walk(eng, [burst], [[cut], [400 - cut]], R.config(), tag="close %d" % cut)
        assert out == [[(84, 319, R.SILENCE)]]
    for cuts in ((283, 200, 117), (284, 200, 116), (284, 199, 117), (64, 219, 1, 199, 1, 116)):
        out = _walk(eng, [long_run], [[n] for n in cuts], R.config(max_len=200), tag="forced %s" % (cuts,))
        assert out == [[(84, 284, R.FORCED), (284, 484, R.FORCED)]]
    # the opening frame, the closing frame and the flush each alone in a launch
    out = _walk(eng, [burst[:350]], [[114], [1], [199], [36], [0]], R.config(end_silence=36), flush_at={0: 4}, tag="single frames")
    assert out == [[(84, 319, R.SILENCE)]]
    out = _walk(eng, [burst[:300]], [[300], [0]], R.config(), flush_at={0: 1}, tag="bare flush")
    assert out == [[(84, 300, R.FLUSH)]]


def test_too_small_a_capacity(eng):
    e = lv((Q, 100), (S, 100), (Q, 80), (S, 100), (Q, 100))         # two sentences
    ref = np.zeros((3, R.STATE_INTS), np.int32)
    want = [R.update(ref[b], x, False, 80, R.config()) for b, x in enumerate((e, e[:250], e))]
    assert [len(w[0]) for w in want] == [2, 0, 2]
    for cap in (0, 1):
        st = np.zeros((3, R.STATE_INTS), np.int32)
        with pytest.raises(N.PfError) as ei:
            eng.op_endpoint_update(st, [e, e[:250], e], cap=cap)
        assert ei.value.code == N.PF_ERR_CAPACITY and ei.value.n.tolist() == [2, 0, 2]      # the counts are filled in
        for b in (0, 2):
            assert _triples(ei.value.events[b, :cap]) == want[b][0][:cap]
        assert (ei.value.events[:, cap:] == -7).all() and (ei.value.events[1] == -7).all()
        np.testing.assert_array_equal(st, ref)                      # the state blocks have advanced
    st = np.zeros((3, R.STATE_INTS), np.int32)
    ev, ins, ob = eng.op_endpoint_update(st, [e, e[:250], e], cap=2)  # exactly enough
    assert [_triples(x) for x in ev] == [w[0] for w in want] and ins.tolist() == [0, 1, 0] and ob.tolist() == [-1, 84, -1]


def test_int32_extreme_levels(eng):
    rng = np.random.default_rng(11)
    x = rng.integers(-(1 << 31), 1 << 31, (4, 700)).astype(np.int32)
    x[:, :3] = [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1]
    x[1, 200:500] = (1 << 31) - 1
    x[2, 100:600] = -(1 << 31)
    n = 0
    for rise in (0, 1, 1 << 20):
        for margin_q in (0, -300, (1 << 31) - 1, -(1 << 31)):
            c = R.config(rise=rise, margin_q=margin_q, window=3, on_count=2, off_count=2, pad_begin=1, pad_end=0, end_silence=2,
                         min_speech=12, max_len=64)
            out = _walk(eng, list(x), [[65] * 4, [257] * 4, [1] * 4, [377] * 4], c, n_mels=128, tag="rise %d margin %d" % (rise, margin_q))
            n += sum(len(o) for o in out)
    assert n > 20


@pytest.mark.parametrize("B", [1, 70])
def test_batch_sizes(eng, B):
    rng = np.random.default_rng(B)
    signals = [V.telegraph(rng, 700, mean_run=int(rng.choice([15, 60])), jitter=50) for _ in range(B)]
    plan = [[int(n) for n in rng.choice([0, 1, 63, 64, 65, 200], B)] for _ in range(5)]
    out = _walk(eng, signals, plan, R.config(max_len=150, end_silence=20, min_speech=20, pad_begin=10), tag="B %d" % B)
    assert sum(len(o) for o in out) >= B


def test_contracts(eng):
    e = lv((Q, 100), (S, 200), (Q, 100))
    st = np.zeros((2, R.STATE_INTS), np.int32)
    assert eng.op_endpoint_update(np.zeros((0, R.STATE_INTS), np.int32), [])[0] == []
    for bad in (dict(rise=-2), dict(pad_end=81), dict(min_speech=11), dict(max_len=30)):
        with pytest.raises(N.PfError) as ei:
            eng.op_endpoint_update(st, [e, e], cfg=bad)
        assert ei.value.code == N.PF_ERR_INVALID_ARG and not st.any()
    with pytest.raises(N.PfError) as ei:                             # n_new[b] above ld
        eng.op_endpoint_update(st, [e, e], ld=399)
    assert ei.value.code == N.PF_ERR_INVALID_ARG and not st.any()
    # frames after a flush are refused for the whole call, and nothing changes; a flush without frames is a no-op
    eng.op_endpoint_update(st, [e[:150], e[:150]], flush=[True, False])
    before = st.copy()
    with pytest.raises(N.PfError) as ei:
        eng.op_endpoint_update(st, [e[150:160], e[150:160]])
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    np.testing.assert_array_equal(st, before)
    ev, ins, ob = eng.op_endpoint_update(st, [e[:0], e[:0]], flush=[True, False])
    assert [len(x) for x in ev] == [0, 0] and ins.tolist() == [0, 1] and ob.tolist() == [-1, 84]
    np.testing.assert_array_equal(st, before)
