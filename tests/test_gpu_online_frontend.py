"""GPU: online_frontend_kernel (csrc/k_frontend_stream.hip) through pf_op_online_frontend_step against the definition,
pf_host_online_frontend_step fed the engine's own fbank rows (pf_fbank) of the same chunks.  Equal: the carried rows (rows 58 and
59 of those fbank rows, by their bits), start_idx, the flags, and which cells hold the sentinel.  A speech or cache cell may differ
by 2^-23 + ulp32(host): the one operation that is not the same IEEE operation on both sides is the fp64 sin / cos; cast to float
its two results differ by at most one place of a value in [-1, 1], and the add that follows rounds once.  The number of cells
that are not bit-equal is printed (expected 0).  The engine's CMVN is online_lockstep_ref.zero_cmvn, so the stream fed a chunk of
exact zeros as its first chunk meets the sentinel inside ordinary rows."""
import numpy as np
import pytest

import online_frontend_ref as FR
import online_lockstep_ref as LR
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

F32 = np.float32
Z = "zeros"
# calls of (slot, chunk, reset): chunk = (audio, index) or Z.  Covered: a first chunk, carried chunks, a reset in the middle, a
# reset on a stream's first step, streams of one call at start_idx 10 / 0 / 0 and later 30 / 20 / 10 in interleaved slots, the zeros.
SCHEDULES = {
    1: (1, [[(0, Z, 1)], [(0, (0, 0), 0)], [(0, (0, 1), 1)], [(0, (0, 2), 0)]]),
    3: (4, [[(2, (0, 0), 0)],
            [(2, (0, 1), 0), (0, Z, 1), (3, (1, 0), 0)],
            [(2, (0, 2), 0), (0, (2, 1), 0), (3, (1, 1), 1)],
            [(2, (0, 3), 1), (0, (2, 2), 0), (3, (1, 2), 0)]]),
    "alone": (1, [[(0, (0, k), int(k == 3))] for k in range(4)]),     # the stream of slot 2 above, by itself
}


def _chunk(c):
    return np.zeros(FR.CHUNK, F32) if c == Z else LR._audio(c[0])[FR.CHUNK * c[1]: FR.CHUNK * (c[1] + 1)]


@pytest.fixture(scope="module")
def rig():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=40)
    pfw = W.pack_pfw(cfg, W.synth_weights(cfg, seed=5))
    plain = Engine(weights=pfw, cmvn=W.synth_cmvn(), device=0)
    cmvn, planted = LR.zero_cmvn(plain.fbank(np.zeros(FR.CHUNK, F32))[0], FR.posenc)
    plain.close()
    eng = Engine(weights=pfw, cmvn=cmvn, device=0)
    played = {}

    def play(key):
        """per call: device speech [B, 20, 560], host speech, device states after it, host states, the fbank rows"""
        if key not in played:
            n, calls = SCHEDULES[key]
            dev, host, out = FR.new_states(n), FR.new_states(n), []
            for call in calls:
                slots, resets = [c[0] for c in call], [c[2] for c in call]
                x = np.stack([_chunk(c[1]) for c in call])
                got = FR.op_step(eng, dev, slots, x, resets)
                rows = [eng.fbank(xb) for xb in x]
                want = np.stack([FR.host_step(host[s], r, cmvn, rs) for s, r, rs in zip(slots, rows, resets)])
                out.append((got, want, dev.copy(), host.copy(), rows))
            played[key] = out
        return played[key]
    yield play, planted
    eng.close()


def _close(dev, host, where):
    dev, host = dev.ravel(), host.ravel()
    sent = host.view(np.uint32) == FR.SENTINEL_BITS
    assert np.array_equal(dev.view(np.uint32) == FR.SENTINEL_BITS, sent), where
    bound = F32(2.0 ** -23) + np.spacing(np.abs(host))
    worst = np.abs(dev.astype(np.float64) - host.astype(np.float64)) - bound
    assert (worst <= 0).all(), (where, float(worst.max()))
    return int((dev.view(np.uint32) != host.view(np.uint32)).sum())


@pytest.mark.parametrize("B", (1, 3))
def test_the_op_against_the_host_statement(rig, B):
    play, planted = rig
    unequal = cells = zeros = 0
    for k, (got, want, dev, host, rows) in enumerate(play(B)):
        call = SCHEDULES[B][1][k]
        unequal += _close(got, want, (B, k, "speech"))
        cells += got.size
        for b, (slot, chunk, _) in enumerate(call):
            carry, cache, start, flags = FR.fields(dev[slot])
            h_carry, h_cache, h_start, h_flags = FR.fields(host[slot])
            assert np.array_equal(carry.view(np.uint32), rows[b][58:].view(np.uint32)), (B, k, slot)      # launch_fbank's bits
            assert np.array_equal(carry.view(np.uint32), h_carry.view(np.uint32))
            assert list(start) == list(h_start) and flags == h_flags == 1, (B, k, slot)
            unequal += _close(cache, h_cache, (B, k, slot, "cache"))
            if chunk == Z:
                hit = {(t, c) for t, c in zip(*np.nonzero(got[b, 10:].view(np.uint32) == FR.SENTINEL_BITS))}
                assert hit >= set(planted)
                zeros += len(hit)
        assert np.array_equal(dev[:, 5770:5772], host[:, 5770:5772]) and np.array_equal(dev[:, 5773:], host[:, 5773:])   # padding cells
        untouched = [s for s in range(dev.shape[0]) if s not in [c[0] for j in range(k + 1) for c in SCHEDULES[B][1][j]]]
        assert not dev[untouched].any()
    print("B = %d: %d of %d speech and cache cells are not bit-equal to the host statement" % (B, unequal, cells))
    assert zeros >= 300
    starts = [int(FR.fields(s)[2][0]) for s in play(B)[-1][2]]
    assert starts == ([20] if B == 1 else [30, 0, 10, 20])


def test_a_stream_alone_and_among_two_others_gives_the_same_bytes(rig):
    play, _ = rig
    for k, (among, alone) in enumerate(zip(play(3), play("alone"))):
        assert np.array_equal(among[0][0].view(np.uint32), alone[0][0].view(np.uint32)), k     # the stream is row 0 of both calls
        assert np.array_equal(among[2][2], alone[2][0]), k
