"""CPU: the streaming FSMN-VAD model score off the device — the host twin (pf_host_vad_model_stream) against the whole-stream
host twins (pf_host_vad_model_logits / _levels) as float64 bits under every chunking, the release schedule
(tests/vadnet_stream_ref.py), the state and error rules, pf_endpoint_model_config and the online `-vadmodel` option."""
import ctypes as C

import numpy as np
import pytest

import vadnet_ref as R
import vadnet_stream_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import engine as E
from aliparaformerasr_amd import weights as W

MODELS = {"small": (R.small_model, R.LENGTHS_SMALL), "released": (R.released_model, R.LENGTHS_RELEASED)}


def test_symbols_are_exported_and_declared():
    lib = N.load()
    for name in ("pf_endpoint_model_config", "pf_vad_model_stream_state_bytes", "pf_host_vad_model_stream_state_bytes",
                 "pf_host_vad_model_stream", "pf_op_vad_model_stream", "pf_online_recognizer_set_endpoint_model"):
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.pf_vad_model_stream_state_bytes(None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_online_recognizer_set_endpoint_model(None, None) < 0
    assert lib.pf_op_vad_model_stream(None, None, None, None, None, 0, 0, 80, None, None, 0, None) < 0


@pytest.fixture(scope="module", params=["small", "released"])
def model(request):
    make, lengths = MODELS[request.param]
    cfg, w = make()
    m = E.load_vad_model(W.pack_pfw(cfg, w))
    yield request.param, cfg, w, m, lengths
    m.close()


def _stream(m, x, chunks, flush_at_end=True, flush_alone=False):
    """x in `chunks`, the flush with the last chunk (or in a call of its own): (levels, logits, released count per call)"""
    st = E.vad_model_stream_state(m, host=True)
    lev, z, cnt, at = [], [], [], 0
    for k, c in enumerate(chunks):
        last = k == len(chunks) - 1
        e, g = E.host_vad_model_stream(m, st, x[at: at + c], flush=flush_at_end and last and not flush_alone)
        at += c
        lev.append(e); z.append(g); cnt.append(len(e))
    if flush_at_end and flush_alone:
        e, g = E.host_vad_model_stream(m, st, x[:0], flush=True)
        lev.append(e); z.append(g); cnt.append(len(e))
    return np.concatenate(lev), np.concatenate(z), cnt, st


def test_chunk_invariance_as_float64_bits(model):
    name, cfg, w, m, lengths = model
    O = cfg["output_dim"]
    for T in lengths:
        x = R.fbank_like(T, cfg["n_mels"], 17 * T + 3)
        want_z, want_e = E.host_vad_model_logits(m, x), E.host_vad_model_levels(m, x)
        plans = [[T], [1] * T if T <= 5 else S.chunkings(T, 5 * T)] + [S.chunkings(T, 100 + s) for s in range(2)]
        for k, chunks in enumerate(plans):
            assert sum(chunks) == T
            e, z, cnt, _ = _stream(m, x, chunks, flush_alone=bool(k & 1))
            assert z.shape == (T, O) and e.shape == (T,)
            np.testing.assert_array_equal(z.view(np.uint64), want_z.view(np.uint64), err_msg=str((name, T, chunks)))
            np.testing.assert_array_equal(e, want_e)
    # T = 1 and 2 flushed at once: the lower and the upper clamp act on the same window
    for T in (1, 2):
        x = R.fbank_like(T, cfg["n_mels"], 900 + T)
        e, z, cnt, _ = _stream(m, x, [T])
        assert cnt == [T]
        np.testing.assert_array_equal(z.view(np.uint64), E.host_vad_model_logits(m, x).view(np.uint64))
        np.testing.assert_allclose(z, R.logits(cfg, w, x), rtol=0, atol=1e-9)


def test_every_chunk_size_of_the_issue_is_drawn(model):
    name, cfg, w, m, lengths = model
    x = R.fbank_like(sum(S.CHUNKS), cfg["n_mels"], 77)
    want = E.host_vad_model_logits(m, x)
    for order in (S.CHUNKS, S.CHUNKS[::-1]):
        e, z, cnt, _ = _stream(m, x, list(order))
        np.testing.assert_array_equal(z.view(np.uint64), want.view(np.uint64))
        assert cnt == S.counts(cfg, list(order), flush_at=len(order) - 1)


def test_released_counts_follow_the_schedule(model):
    name, cfg, w, m, lengths = model
    r = S.right(cfg)
    assert r == cfg["lfr_m"] - 1 - (cfg["lfr_m"] - 1) // 2 == 2
    x = R.fbank_like(140, cfg["n_mels"], 5)
    for chunks in ([1, 1, 1, 1, 0, 2, 64, 65, 5], [0, 0, 140], [2, 0, 3, 135], S.chunkings(140, 3)):
        e, z, cnt, _ = _stream(m, x, chunks, flush_alone=True)
        assert cnt == S.counts(cfg, chunks + [0], flush_at=len(chunks)), chunks
        assert cnt[-1] == min(r, 140) and sum(cnt) == 140
        # and the reference stream hands out the same levels at the same calls
        ref, at, got_at = S.Stream(cfg, w), 0, 0
        for k, c in enumerate(chunks + [0]):
            le, lz, first = ref.feed(x[at: at + c], flush=k == len(chunks))
            at += c
            assert len(le) == cnt[k] and first == got_at
            np.testing.assert_allclose(z[got_at: got_at + cnt[k]], lz, rtol=0, atol=1e-9)
            got_at += cnt[k]
    # before the flush: max(0, n - right)
    st = E.vad_model_stream_state(m, host=True)
    seen = 0
    for n_new in (1, 1, 1, 3):
        e, _ = E.host_vad_model_stream(m, st, x[seen: seen + n_new])
        seen += n_new
        assert len(e) == S.released(cfg, seen, False) - S.released(cfg, seen - n_new, False)


def test_state_and_error_rules(model):
    name, cfg, w, m, lengths = model
    lib = N.load()
    x = R.fbank_like(30, cfg["n_mels"], 8)
    nb, nh = C.c_int64(), C.c_int64()
    N.check(lib.pf_vad_model_stream_state_bytes(m._h, nb))
    N.check(lib.pf_host_vad_model_stream_state_bytes(m._h, nh))
    reach = (cfg["lorder"] - 1) * cfg["lstride"]
    ldp = (cfg["proj_dim"] + 31) // 32 * 32
    assert nb.value == (4 * (cfg["n_layers"] * reach * ldp + (cfg["lfr_m"] - 1) * cfg["n_mels"] + 2) + 15) // 16 * 16
    assert nh.value >= 8 * cfg["n_layers"] * reach * cfg["proj_dim"] + 4 * (cfg["lfr_m"] - 1) * cfg["n_mels"] + 8
    if name == "released":
        assert 39000 < nb.value < 41000                              # "about 40 KB per stream"
    st = E.vad_model_stream_state(m, host=True)
    assert st.size == nh.value and not st.any()
    E.host_vad_model_stream(m, st, x[:10])
    before = st.copy()
    e, z = E.host_vad_model_stream(m, st, x[:0])                     # n_new = 0 without a flush: no byte changes
    assert len(e) == 0 and (st == before).all()
    with pytest.raises(N.PfError) as ei:                             # too small a capacity: nothing changed
        E.host_vad_model_stream(m, st, x[10:20], cap=3)
    assert ei.value.code == N.PF_ERR_CAPACITY and (st == before).all()
    e, _ = E.host_vad_model_stream(m, st, x[10:20], flush=True)
    assert len(e) == 20 - 8
    flushed = st.copy()
    e, _ = E.host_vad_model_stream(m, st, x[:0], flush=True)         # a second flush without frames is a no-op
    assert len(e) == 0 and (st == flushed).all()
    with pytest.raises(N.PfError) as ei:                             # frames after a flush
        E.host_vad_model_stream(m, st, x[20:21])
    assert ei.value.code == N.PF_ERR_INVALID_ARG and (st == flushed).all()
    # a count beyond PF_ENDPOINT_MAX_STREAM_FRAMES: count | flushed are the block's last 8 bytes
    st = E.vad_model_stream_state(m, host=True)
    st[-8:].view(np.int32)[0] = N.PF_ENDPOINT_MAX_STREAM_FRAMES - 3
    before = st.copy()
    with pytest.raises(N.PfError) as ei:
        E.host_vad_model_stream(m, st, x[:4])
    assert ei.value.code == N.PF_ERR_CAPACITY and (st == before).all()
    with pytest.raises(N.PfError) as ei:                             # the wrong front-end width
        E.host_vad_model_stream(m, E.vad_model_stream_state(m, host=True), np.zeros((2, cfg["n_mels"] + 1), np.float32), n_mels=cfg["n_mels"] + 1)
    assert ei.value.code == N.PF_ERR_INVALID_ARG


def test_endpoint_model_config():
    c, d = E.endpoint_model_config(), E.endpoint_config()
    assert (c.rise, c.abs_level) == (-1, 9830)
    for k in ("struct_size", "margin_q", "window", "on_count", "off_count", "pad_begin", "pad_end", "end_silence", "min_speech", "max_len"):
        assert getattr(c, k) == getattr(d, k), k
    v = E.vad_model_config()
    assert c.abs_level == v.abs_level                                 # the rule pf_vad_model_config states
    assert E.endpoint_model_config(end_silence=40).end_silence == 40
    assert N.load().pf_endpoint_model_config(None) == N.PF_ERR_INVALID_ARG


def test_cli_vadmodel_with_endpoint():
    from aliparaformerasr_amd.examples import parse_args
    on = ["-type", "online", "-model", "m", "-files", "a.wav"]
    cfg = parse_args(on + ["-endpoint", "-vadmodel", "vad.pfw"])
    assert cfg["vadmodel"] == "vad.pfw" and cfg["endpoint"] == {}
    cfg = parse_args(on + ["-vadmodel", "v.pfw", "-endpoint", "end_silence=40", "-secondpass", "off"])
    assert cfg["vadmodel"] == "v.pfw" and cfg["endpoint"] == {"end_silence": 40} and cfg["secondpass"] == "off"
    with pytest.raises(ValueError, match="-vadmodel goes with -vad"):
        parse_args(on + ["-vadmodel", "vad.pfw"])
    with pytest.raises(ValueError, match="-vadmodel goes with -vad"):
        parse_args(["-type", "offline", "-model", "m", "-files", "a.wav", "-vadmodel", "vad.pfw"])
    with pytest.raises(ValueError, match="-vadmodel takes"):
        parse_args(on + ["-endpoint", "-vadmodel"])
    assert "vadmodel" not in parse_args(on + ["-endpoint"])
    off = parse_args(["-type", "offline", "-model", "m", "-files", "a.wav", "-vad", "-vadmodel", "vad.pfw"])
    assert off["vadmodel"] == "vad.pfw" and "endpoint" not in off
