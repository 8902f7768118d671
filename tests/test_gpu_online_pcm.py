"""GPU: the streaming PCM intake.  pcm_stream_kernel (csrc/k_pcm_stream.hip) through pf_op_online_pcm_step against the host twin
(pf_host_pcm_stream_*, itself held to the one-shot conversion by tests/test_online_pcm_cpu.py), bit for bit over consecutive steps
on one state block; stream independence; OnlineStream.AddPcm against AddSamples of the twin's output on the synthetic streaming
model, with the device front-end and without."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.offline_recognizer import RecognizerException
from pcm_ref import bits_equal, payload
from test_gpu_online_token_info import rigs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FS, ROW = 16000, 9600
BPV = {"s16": 2, "s24": 3, "f32": 4, "mulaw": 1}
STEPS = (1, 255, 256, 257, 1023, 1024, 1025, 9600)                        # n_out per step: around the pass and the tile


def fed(desc, data, cfg=None):
    """a converter for the op that holds all of data, its input ended"""
    ps = N.HostPcmStream(desc, FS, cfg)
    ps.append(data, finish=True)
    return ps


def run_steps(eng, ps, whole, steps, states, slot, where):
    """steps the converter until `whole` is out, each step against the twin's samples and the +0 pad of the row"""
    done, k = 0, 0
    while done < whole.size:
        out, nw = N.op_online_pcm_step(eng, states, [slot], [ps], [steps[k % len(steps)]])
        n = int(nw[0])
        assert n == min(steps[k % len(steps)], whole.size - done), where
        assert bits_equal(out[0, :n], whole[done:done + n]), (where, k, done)
        assert not out[0, n:].view(np.uint32).any(), (where, k)
        done, k = done + n, k + 1
    return k


@pytest.mark.parametrize("sinc", (False, True), ids=("linear", "sinc"))
@pytest.mark.parametrize("sr,fmt,ch", [(8000, "mulaw", 1), (11025, "s16", 2), (44100, "s24", 1), (48000, "s16", 2), (96000, "f32", 2),
                                       (16000, "f32", 2)])
def test_steps_equal_the_host_twin(rigs, sr, fmt, ch, sinc):
    eng = rigs().eng
    desc = N.pcm_desc(sr, ch, fmt, sinc=sinc)
    n_mono = int(sum(STEPS) * sr / FS) + 6 * 50 + 3                       # every step size once, a short finishing step behind them
    data = payload(fmt, ch * n_mono + (ch - 1), seed=sr // 100 + ch)      # stereo: an unpaired trailing value
    whole = N.host_pcm_convert(data, desc)
    states = np.full((3, N.pcm_stream_state_bytes()), 0x5A, np.uint8)     # a new stream reads nothing of its block
    k = run_steps(eng, fed(desc, data), whole, STEPS, states, 1, (sr, fmt, ch, sinc))
    assert k >= len(STEPS) and not (states[0] != 0x5A).any() and not (states[2] != 0x5A).any()


@pytest.mark.parametrize("sinc", (False, True), ids=("linear", "sinc"))
@pytest.mark.parametrize("sr", (8000, 96000))
def test_short_inputs_finish_as_the_one_shot(rigs, sr, sinc):
    """n_mono in {0, 1, 2, H - 1, H, H + 1} of the rate's own half-window (26 at 8 kHz, 154 at 96 kHz, where the whole sequence
    lies inside one window), and 6 k + 3, the half-to-even length at 96 kHz"""
    eng = rigs().eng
    H = R.shape(sr, FS)[2]
    desc = N.pcm_desc(sr, 1, "s16", sinc=sinc)
    for n_mono in (0, 1, 2, H - 1, H, H + 1, 6 * 50 + 3):
        data = payload("s16", n_mono, seed=n_mono)
        whole = N.host_pcm_convert(data, desc)
        states = np.zeros((1, N.pcm_stream_state_bytes()), np.uint8)
        run_steps(eng, fed(desc, data), whole, (7, ROW), states, 0, (sr, sinc, n_mono))
        if not whole.size:                                                # nothing to emit: the finishing step is a row of +0
            out, nw = N.op_online_pcm_step(eng, states, [0], [fed(desc, data)], [ROW])
            assert nw[0] == 0 and not out.view(np.uint32).any(), (sr, sinc, n_mono)


def test_open_stream_steps_read_the_carried_tail(rigs):
    """bytes arrive in small pieces while the stream is open: every window lies mostly in the tail the last step left"""
    eng = rigs().eng
    for sr, zeros in ((8000, 24), (11025, 32), (48000, 24)):              # zeros = 32 at 11.025 kHz: the 179 KB bank
        cfg = N.resample_config(zeros, None, None)
        desc = N.pcm_desc(sr, 1, "s16", sinc=True)
        data = payload("s16", 5000, seed=sr)
        twin, ps = N.HostPcmStream(desc, FS, cfg), N.HostPcmStream(desc, FS, cfg)
        states, flips = np.zeros((2, N.pcm_stream_state_bytes()), np.uint8), 0
        eng.set_resample(zeros=zeros)
        try:
            for a in range(0, len(data), 74):                             # 37 frames a piece
                want = twin.push(data[a:a + 74])
                ps.append(data[a:a + 74])
                out, nw = N.op_online_pcm_step(eng, states, [1], [ps], [ROW])
                assert nw[0] == want.size and bits_equal(out[0, :want.size], want), (sr, a)
                flips += 1
            want = twin.finish()
            ps.append(b"", finish=True)
            out, nw = N.op_online_pcm_step(eng, states, [1], [ps], [ROW])
            assert nw[0] == want.size and bits_equal(out[0, :want.size], want), sr
        finally:
            eng.set_resample()
        assert flips >= 3


def test_streams_are_independent_and_a_nan_poisons_its_windows_only(rigs):
    eng = rigs().eng
    specs = [(8000, "mulaw", 1, True, 1025), (44100, "s16", 2, True, 257), (48000, "s24", 2, False, 1024), (96000, "f32", 1, True, 255),
             (16000, "f32", 1, False, 9600)]
    slots = [9, 2, 7, 0, 4]
    datas = [payload(f, c * int(3000 * sr / FS), seed=i) for i, (sr, f, c, _s, _n) in enumerate(specs)]
    x = np.frombuffer(datas[3], "<f4").copy()
    x[1500] = np.nan                                                      # 96 kHz f32 mono: frame 1500
    datas[3] = x.tobytes()
    descs = [N.pcm_desc(sr, c, f, sinc=s) for sr, f, c, s, _n in specs]
    n_out = [n for *_r, n in specs]

    def two_steps(order):
        states = np.zeros((10, N.pcm_stream_state_bytes()), np.uint8)
        ps = [fed(descs[i], datas[i]) for i in order]
        a = N.op_online_pcm_step(eng, states, [slots[i] for i in order], ps, [n_out[i] for i in order])[0]
        b = N.op_online_pcm_step(eng, states, [slots[i] for i in order], ps, [n_out[i] for i in order])[0]
        return {i: np.concatenate([a[k], b[k]]) for k, i in enumerate(order)}

    together = two_steps([0, 1, 2, 3, 4])
    for other in (two_steps([4, 3, 2, 1, 0]), two_steps([0, 1, 2, 3, 4]), *(two_steps([i]) for i in range(5))):
        for i, y in other.items():
            assert np.array_equal(y.view(np.uint32), together[i].view(np.uint32)), i
    _L, _M, H, _c = R.shape(96000, FS)
    y = np.concatenate([together[3][:255], together[3][ROW:ROW + 255]])   # outputs 0 .. 509: the NaN's window crosses the two steps
    i = np.arange(510)
    hit = (6 * i - H + 1 <= 1500) & (1500 <= 6 * i + H)
    assert hit[:255].any() and hit[255:].any() and np.array_equal(np.isnan(y), hit)
    assert all(not np.isnan(together[k]).any() for k in (0, 1, 2, 4))


def _recognizers(rig, device):
    from test_gpu_online_token_info import _recognizer
    recs = [_recognizer(rig.d, True), _recognizer(rig.d, True)]
    for r in recs:
        if device:
            r.SetDeviceFrontend(True)
        else:
            r.SetEndpoint()
    return recs


def _same(a, b, where):
    assert a.Tokens == b.Tokens, where
    assert [tuple(t) + (t.score_bits,) for t in a.TokenInfo] == [tuple(t) + (t.score_bits,) for t in b.TokenInfo], where


def _census(rec):
    """launches so far of the PCM intake, the fbank and the streaming front-end on the recognizer's engine"""
    lib, h, out = N.load(), C.c_void_p(rec.engine_handle()), []
    for cls in (b"pcm_stream", b"fbank", b"online_frontend"):
        ms, n, fpl = C.c_double(), C.c_int64(), C.c_double()
        N.check(lib.pf_profile_get(h, cls, C.byref(ms), C.byref(n), C.byref(fpl)))
        out.append(n.value)
    return np.array(out)


@pytest.mark.parametrize("device", (True, False), ids=("device_frontend", "host_frontend"))
def test_add_pcm_equals_add_samples_of_the_twin(rigs, device):
    """Both recognizers take the same mixed calls; ref sees AddSamples only.  With the device front-end the launch census of every
    call: ref's is the parent's (one fbank and one front-end launch when a chunk was taken, never the PCM intake's), and pcm's is
    that plus ONE pcm_stream launch for all its PCM-fed streams."""
    rig = rigs()
    pcm, ref = _recognizers(rig, device)
    try:
        for r in (pcm, ref):
            N.check(N.load().pf_profile_enable(C.c_void_p(r.engine_handle()), 1))
            N.check(N.load().pf_profile_reset(C.c_void_p(r.engine_handle())))
        seen = [_census(pcm), _census(ref)]

        def calls(ps, rs):
            texts = [[e.Text for e in pcm.GetResults(ps)], [e.Text for e in ref.GetResults(rs)]]
            now = [_census(pcm), _census(ref)]
            if device:
                dp, dr = now[0] - seen[0], now[1] - seen[1]
                assert now[1][0] == 0 and dr[1] == dr[2] and dr[1] in (0, 1), dr
                assert dp[1] == dp[2] == dr[1] and dp[0] in (0, dp[1]), (dp, dr)
            seen[:] = now
            return texts
        kinds = [(8000, "mulaw", 1, "sinc"), (48000, "s16", 2, "linear")]
        datas = [payload(f, c * int(2.2 * sr), seed=sr) for sr, f, c, _r in kinds]
        twins = [N.HostPcmStream(N.pcm_desc(sr, c, f, sinc=r == "sinc"), FS) for sr, f, c, r in kinds]
        sp, sr_ = [pcm.CreateOnlineStream() for _ in kinds], [ref.CreateOnlineStream() for _ in kinds]
        extra_p, extra_r = pcm.CreateOnlineStream(), ref.CreateOnlineStream()     # an AddSamples-fed stream in the same calls
        noise = np.random.default_rng(3).uniform(-0.3, 0.3, 2 * FS).astype(np.float32)
        pos, rng, call = [0, 0], np.random.default_rng(11), 0
        while any(p < len(d) for p, d in zip(pos, datas)):
            for u, (srate, f, c, r) in enumerate(kinds):
                n = int(rng.integers(1, srate * BPV[f] * c // 3))                 # uneven pieces, cut anywhere
                piece = datas[u][pos[u]:pos[u] + n]
                pos[u] += n
                sp[u].AddPcm(piece, srate, c, f, resample=r)
                sr_[u].AddSamples(twins[u].push(piece))
            for s in (extra_p, extra_r):
                s.AddSamples(noise[call * 5000:(call + 1) * 5000])
            got, want = calls(sp + [extra_p], sr_ + [extra_r])
            assert got == want, call
            for u in range(len(kinds)):
                _same(sp[u], sr_[u], (device, call, u))
            _same(extra_p, extra_r, (device, call, "samples"))
            call += 1
        for u in range(len(kinds)):
            sr_[u].AddSamples(twins[u].finish())
            sp[u].InputFinished()
            sr_[u].InputFinished()
        for drain in range(8):
            got, want = calls(sp, sr_)
            assert got == want, drain
            for u in range(len(kinds)):
                _same(sp[u], sr_[u], (device, "drain", drain, u))
        assert all(len(s.Tokens) > 0 for s in sp)
        if device:
            assert seen[0][1] >= seen[0][0] >= 3
    finally:
        pcm.Dispose()
        ref.Dispose()


def test_refusals(rigs):
    rec = _recognizers(rigs(), True)[0]
    try:
        s = rec.CreateOnlineStream()
        s.AddPcm(b"\0\0", 8000)
        for bad in (lambda: s.AddSamples(np.zeros(4, np.float32)), lambda: s.AddPcm(b"\0\0", 8000, format="f32"),
                    lambda: s.AddPcm(b"\0\0", 8000, 2)):
            with pytest.raises(N.PfError) as e:
                bad()
            assert e.value.code == N.PF_ERR_INVALID_ARG
        s.InputFinished()
        t = rec.CreateOnlineStream()
        t.AddSamples(np.zeros(4, np.float32))
        for bad in (lambda: s.AddPcm(b"\0\0", 8000), lambda: t.AddPcm(b"\0\0", 8000)):
            with pytest.raises(N.PfError) as e:
                bad()
            assert e.value.code == N.PF_ERR_INVALID_ARG
        for bad, code in ((lambda: t2.AddPcm(b"", 8000, 3), N.PF_ERR_INVALID_ARG), (lambda: t2.AddPcm(b"", 16001, resample="sinc"), N.PF_ERR_UNSUPPORTED)):
            t2 = rec.CreateOnlineStream()
            with pytest.raises(N.PfError) as e:
                bad()
            assert e.value.code == code
        # a step that fails (the resampler's shape changed under the stream) fails the stream: no later step reads a stale tail
        f = rec.CreateOnlineStream()
        f.AddPcm(bytes(2 * 6000), 8000, resample="sinc")
        rec.SetResample(zeros=16)
        for bad in (lambda: rec.GetResults([f]), lambda: f.AddPcm(b"\0\0", 8000, resample="sinc"), lambda: rec.GetResults([f])):
            with pytest.raises(RecognizerException):
                bad()
    finally:
        rec.Dispose()
