"""CPU: the carried CIF of a streaming chunk step and the time rule of the streaming token info.

  * tests/cif_stream_ref.py restates the step in numpy; over chained calls its fired rows and its carry are
    oracle.online.cif's after dynamic_mask, bit for bit.
  * pf_host_online_cif_step (csrc/online.cpp, built on online_cif) equals the restatement bit for bit in fired rows, fire
    entries, count and state bytes on the case table of cif_stream_ref.step_cases: random chunks, dyadic alphas whose sums land on
    the threshold exactly (strict <: equality fires), a chunk without a fire (the carry is divided), an all-zero chunk
    (integrate == 0: the carry stays unscaled), a carry at and above the threshold (entry 0 fires), a reset inside a chain, and
    the shapes at which the device kernel takes another path.  tests/test_gpu_cif_stream.py holds the kernel to the same table.
  * the time rule, on the restated stream's provenance alone (no model runs): the anchor 600 k + 60 p - 1220 ms for whole
    9600-sample pieces wherever that is not negative, and what the rule says where it is; InputFinished with 0, 1, 9600 and
    9600 + 37 cached samples; after a reset the cached positions 5 .. 9 take position 10's time.
"""
import ctypes as C

import numpy as np
import pytest

import cif_stream_ref as CR
import online_lockstep_ref as LR
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import online as oo

F32 = np.float32
CASES = CR.step_cases()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def test_state_block_size():
    for D in (4, 8, 256, 260, 512, 1024, 1028):
        n = C.c_int64()
        N.check(N.load().pf_host_online_cif_state_bytes(D, n))
        assert n.value == CR.state_bytes(D) and n.value % 16 == 0
    assert CR.state_bytes(512) == 2048 + 16


def test_restatement_is_the_oracles_cif_behind_dynamic_mask():
    r = np.random.default_rng(7)
    D, Tc = 512, 20
    st = CR.new_state(D)
    hid, al = [np.zeros(D, F32)], [F32(0.0)]                          # the oracle stream's cache, as OnlineStream keeps it
    fires = 0
    for k in range(6):
        h = r.standard_normal((Tc, D)).astype(F32)
        a = r.random(Tc).astype(F32)
        hid += list(h)
        al += list(oo.dynamic_mask(a))
        f, ca, ch = oo.cif(np.stack(hid), np.asarray(al, F32), 1.0)
        hid, al = [ch], [ca]
        fired, entry, n = CR.step(st, h, a, 1.0)
        assert n == f.shape[0] and (_bits(fired[:n]) == _bits(f)).all() and not fired[n:].any()
        assert (_bits(st[:D]) == _bits(ch)).all() and _bits(st[D])[()] == _bits(ca)[()] and _bits(st[D + 1])[()] == _bits(ca)[()]
        assert (entry[:n] > 5).all() and (entry[:n] <= 15).all() and (np.diff(entry[:n]) > 0).all() and (entry[n:] == -1).all()
        fires += n
    assert fires > 20


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_step_equals_the_restatement(case):
    want = CR.run_case(case)
    got = CR.run_case(case, CR.host_step)
    for k, (w, g) in enumerate(zip(want, got)):
        assert g[2] == w[2], (case.name, k)
        assert (g[1] == w[1]).all(), (case.name, k)
        assert (_bits(g[0]) == _bits(w[0])).all(), (case.name, k)
        assert (_bits(g[3]) == _bits(w[3])).all(), (case.name, k)


def test_the_cases_are_what_their_names_say():
    by = {c.name: CR.run_case(c) for c in CASES}
    assert by["dyadic"][0][2] == 3 and list(by["dyadic"][0][1][:3]) == [7, 10, 14]       # equality fired; nothing is carried
    D = 512
    assert by["dyadic"][0][3][D] == 0 and not by["dyadic"][0][3][:D].any()
    c = [x for x in CASES if x.name == "no-fire"][0]
    assert by["no-fire"][0][2] == 0 and by["no-fire"][0][3][D] > 0
    a = CR.mask(c.calls[0][1])
    undivided = np.zeros(D, F32)
    for t in range(20):
        undivided = (undivided + (a[t] * c.calls[0][0][t]).astype(F32)).astype(F32)
    assert (_bits(by["no-fire"][0][3][:D]) == _bits(undivided / by["no-fire"][0][3][D])).all()          # the carry is divided
    assert by["all-zero"][0][2] == 0 and not by["all-zero"][0][3].any()                                  # integrate == 0: unscaled
    assert by["all-zero"][2][3][D] > 0
    assert by["carry-at-threshold"][0][1][0] == 0 and by["carry-above-threshold"][0][1][0] == 0          # entry 0 fired
    assert by["dense"][0][2] >= 7


def test_a_reset_inside_a_chain_equals_two_streams():
    c = [x for x in CASES if x.name == "reset-at-4"][0]
    whole = CR.run_case(c, CR.host_step)
    plain = [(h, a, False) for h, a, _ in c.calls]
    first = CR.run_case(CR.StepCase("a", c.D, c.Tc, plain[:3]), CR.host_step)
    second = CR.run_case(CR.StepCase("b", c.D, c.Tc, plain[3:]), CR.host_step)
    for w, g in zip(whole, first + second):
        assert w[2] == g[2] and (w[1] == g[1]).all() and (_bits(w[0]) == _bits(g[0])).all() and (_bits(w[3]) == _bits(g[3])).all()
    assert sum(w[2] for w in whole) > 10


def test_capacity_and_argument_errors():
    D, Tc = 8, 20
    r = np.random.default_rng(3)
    h, a = r.standard_normal((Tc, D)).astype(F32), r.random(Tc).astype(F32)
    st = CR.new_state(D)
    f, e, n = CR.host_step(st, h, a, 1.0, cap=Tc + 1)                                     # cap == Tc + 1 is enough
    assert f.shape == (Tc + 1, D) and n >= 3
    before = st.copy()
    assert CR.host_step(st, h, a, 1.0, cap=Tc, rc=True) == N.PF_ERR_INVALID_ARG          # cap == Tc is refused
    assert CR.host_step(st, h[:, :6], a, 1.0, rc=True) == N.PF_ERR_INVALID_ARG           # D % 4 != 0
    assert (_bits(st) == _bits(before)).all()
    lib = N.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    fired, ent, cnt = np.zeros((Tc + 1, D), F32), np.zeros(Tc + 1, np.int32), C.c_int32()
    args = [st.ctypes.data_as(C.c_void_p), h.ctypes.data_as(fp), a.ctypes.data_as(fp), Tc, D, 1.0, 5, 15, 0, fired.ctypes.data_as(fp),
            ent.ctypes.data_as(ip), Tc + 1, cnt]
    for i in (0, 1, 2, 9, 10, 12):                                                        # every pointer
        bad = list(args)
        bad[i] = None
        assert lib.pf_host_online_cif_step(*bad) == N.PF_ERR_INVALID_ARG, i
    bad = list(args)
    bad[3] = 0                                                                            # Tc <= 0
    assert lib.pf_host_online_cif_step(*bad) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_online_cif_state_bytes(6, C.c_int64()) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_online_cif_state_bytes(8, None) == N.PF_ERR_INVALID_ARG
    assert (_bits(st) == _bits(before)).all()
    # the device op refuses the same before it touches an engine's memory: a null engine is an error of its own
    assert lib.pf_op_online_cif_step(None, *args[:3], None, 1, Tc, D, 1.0, 5, 15, args[9], args[10], Tc + 1, args[10]) < 0


# ------------------------------------------------------------------------------------------------ the time rule
@pytest.fixture(scope="module")
def timed():
    cfg, w = LR.model()
    return CR.TimedRecognizer(cfg, w, W.synth_cmvn(), LR.tokens(), quant="fp32", fbank_cache={})


def _anchor(k, p):
    return 600 * k + 60 * p - 1220


def test_anchor_for_whole_chunks(timed):
    s = timed.create_stream()
    audio = W.synth_audio(9600 * 6, 5)
    seen = 0
    for k in range(6):
        s.add_samples(audio[9600 * k: 9600 * (k + 1)])               # releases chunk k (chunk 0: the constructor's silence)
        assert s.get_decode_chunk() is not None and len(s.chunk_idx) == 20
        for p in range(20):
            t = _anchor(k, p)
            if t >= 0:                                                # the frame has an index, and the index IS the anchor
                assert s.chunk_idx[p] >= 0 and s.position_ms(p) == t, (k, p)
                seen += 1
            else:                                                     # no index (silence, or a copy of silence): the rule's fallback
                assert s.chunk_idx[p] == -1, (k, p)
                nxt = [q for q in range(p, 20) if _anchor(k, q) >= 0]
                assert s.position_ms(p) == (_anchor(k, nxt[0]) if nxt else CR.time_ms(s.caller_samples)), (k, p)
        assert s.get_decode_chunk() is None
    assert seen == 9 + 19 + 3 * 20                                    # chunk 1: p >= 11; chunk 2: p >= 1; then every position
    # the carry: position 14 of the chunk before
    s2 = timed.create_stream()
    s2.add_samples(audio[:9600]); s2.get_decode_chunk(); s2.times([])
    s2.add_samples(audio[9600:19200]); s2.get_decode_chunk()
    assert s2.times([6, 15]) == [_anchor(1, 11), _anchor(1, 14)]     # p = 5 has no index: the first one that has is p = 11
    s2.add_samples(audio[19200:28800]); s2.get_decode_chunk()
    assert s2.times([0, 6]) == [_anchor(1, 14), _anchor(2, 5)]


FEEDS = {0: (1,), 1: (1,), 9600: (9600,), 9600 + 37: (16000, 3237)}  # a stream releases ONE chunk per AddSamples, above 9600 cached


@pytest.mark.parametrize("cached", sorted(FEEDS))
def test_input_finished(timed, cached):
    """`cached` caller samples in the stream's cache at InputFinished (0: a second InputFinished, as in the lockstep schedule)"""
    s = timed.create_stream()
    audio = W.synth_audio(9600 * 3, 6)
    off = 0
    for n in FEEDS[cached]:
        s.add_samples(audio[off: off + n])
        off += n
    if cached == 0:
        s.input_finished()
    assert len(s.cache_samples) == cached
    s.input_finished()
    assert s.caller_samples == off
    chunks = []
    while s.get_decode_chunk() is not None:
        chunks.append(list(s.chunk_idx))
    assert len(chunks) == 1 + -(-off // 9600)                         # the silence, then ceil(total / 9600) chunks, the last zero-padded
    for k, idx in enumerate(chunks):
        for p in range(20):
            t = _anchor(k, p)
            assert (idx[p] == 16 * t) if t >= 0 else (idx[p] == -1), (k, p)   # padded rows keep the frame grid of their chunk


def test_after_a_reset_the_cached_positions_take_position_tens_time(timed):
    s = timed.create_stream()
    audio = W.synth_audio(9600 * 4, 7)
    for k in range(3):
        s.add_samples(audio[9600 * k: 9600 * (k + 1)])
        s.get_decode_chunk()
    s.times([])
    s.reset()
    assert s.info == [] and s.carry_idx == -1
    s.add_samples(audio[9600 * 3:])
    s.get_decode_chunk()
    assert s.chunk_idx[:10] == [-1] * 10 and s.chunk_idx[10] == 16 * _anchor(3, 10)
    assert [s.position_ms(p) for p in range(5, 11)] == [_anchor(3, 10)] * 6
    assert s.times([0]) == [CR.time_ms(s.caller_samples)]             # (a carry cannot fire behind a reset; the rule still answers)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_tokentimes_option():
    from collections import namedtuple
    from aliparaformerasr_amd import examples as ex
    assert "tokentimes" not in ex.parse_args(["-type", "online", "-files", "a.wav"])
    assert ex.parse_args(["-type", "online", "-tokentimes", "-files", "a.wav"])["tokentimes"] is True
    with pytest.raises(ValueError):
        ex.parse_args(["-type", "offline", "-tokentimes", "-files", "a.wav"])
    T = namedtuple("T", "id time_ms score fired")
    names = ["<blank>", "<s>", "</s>", "<unk>", "a", "b@@"]
    info = [T(0, -1, 0.0, False), T(0, -1, 0.0, False), T(4, 40, -0.25, True), T(3, 100, -1.0, True), T(5, -1, -2.0, False),
            T(5, 160, -0.5, True), T(2, 220, -0.125, True), T(4, 280, -0.1, True)]
    assert ex.token_times_line(info, names) == "a[40 -0.250] b@@[160 -0.500]"
