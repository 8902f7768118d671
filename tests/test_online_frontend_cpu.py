"""pf_host_online_frontend_step (csrc/online.cpp online_frontend_step): the streaming front-end behind the fbank on one stream's
block, against the glue it restates in closed form — LockstepStream.get_decode_chunk of tests/online_lockstep_ref.py fed the same
rows the way _input_speech queues them (the first frame repeated once), plus the sentinel rule, with the position term taken from
the library as that module takes it.  Bit-equal speech and state over five chunks with a reset after the third."""
import types

import numpy as np
import pytest

import online_frontend_ref as FR
import online_lockstep_ref as LR
from aliparaformerasr_amd import weights as W
from oracle import online as oo

F32 = np.float32


@pytest.mark.parametrize("zero_cmvn", (False, True))
def test_the_host_step_is_get_decode_chunk_and_the_sentinel(zero_cmvn):
    rng = np.random.default_rng(7)
    chunks = [(rng.standard_normal((60, 80)) * 3 + 5).astype(F32) for _ in range(5)]
    chunks[0][:] = chunks[0][0]                                       # the constructor's chunk: one row, every frame
    cmvn, planted = W.synth_cmvn(), []
    if zero_cmvn:
        cmvn, planted = LR.zero_cmvn(chunks[0][0], FR.posenc)
    shift, scale = (np.asarray(v, F32) for v in cmvn)
    rec = types.SimpleNamespace(mutate=None, endpoint=None, shift=shift, scale=scale, position_encode=FR.posenc,
                                graphs=types.SimpleNamespace(o=types.SimpleNamespace(cfg=types.SimpleNamespace(dec_layers=1))))
    ref = LR.LockstepStream(rec)
    block = FR.new_states(1)[0]
    for k, rows in enumerate(chunks):
        ref.speech = np.concatenate([ref.speech, rows[:1], rows] if k == 0 else [ref.speech, rows])   # oo.OnlineStream._input_speech
        if k == 3:
            ref.reset()
        want = ref.get_decode_chunk()
        want = np.where(want == 0, oo.SENTINEL, want).astype(F32)
        got = FR.host_step(block, rows, (shift, scale), reset=(k == 3))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        carry, cache, start, flags = FR.fields(block)
        assert np.array_equal(carry.view(np.uint32), rows[58:].view(np.uint32)), k
        assert np.array_equal(cache.view(np.uint32), ref.cache_feats.view(np.uint32)), k
        assert list(start) == [ref.start_idx] * 10 and flags == 1, k
        if k == 0:                                                    # exact zeros meet the sentinel where they were planted
            hit = {(t, c) for t, c in zip(*np.nonzero(got[10:].view(np.uint32) == FR.SENTINEL_BITS))}
            assert hit >= set(planted) and (len(hit) >= 300) == zero_cmvn
            assert (got[:10].view(np.uint32) == FR.SENTINEL_BITS).all()    # the fresh cache
    assert ref.start_idx == 20 and ref.speech.shape[0] == 1            # reset at chunk 3; one row waits for the next chunk
