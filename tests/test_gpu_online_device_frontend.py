"""GPU: OnlineRecognizer.SetDeviceFrontend end to end.  Every non-endpoint case of online_lockstep_ref.cases on two recognizers, one
with SetTokenInfo alone and one with the device front-end as well: after EVERY GetResults every stream's Tokens, Text and TokenInfo
(scores by their bits) are equal.  A new stream in a disposed stream's slot; the refusals; the command line."""
import gc
import io

import numpy as np
import pytest

import online_frontend_ref as FR
import online_lockstep_ref as LR
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from test_gpu_online_token_info import YAML, LibSide, _write

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = [c for c in LR.cases() if not c.schedule.endpoint]


def _recognizer(d, frontend):
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    rec = OnlineRecognizer(str(d / "model.pfw"), "", str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))
    rec.SetTokenInfo(True)
    if frontend:
        rec.SetDeviceFrontend(True)
    return rec


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    made = {}

    def get(bias=LR.DENSE, zero_cmvn=False):
        key = (bias, zero_cmvn)
        if key not in made:
            from aliparaformerasr_amd.engine import Engine
            cfg, w = LR.model(bias)
            cmvn = W.synth_cmvn()
            if zero_cmvn:
                eng = Engine(weights=W.pack_pfw(cfg, w), cmvn=cmvn, device=0)
                cmvn, _ = LR.zero_cmvn(eng.fbank(np.zeros(LR.CHUNK, F32))[0], FR.posenc)
                eng.close()
            d = _write(tmp_path_factory.mktemp("devfe"), cfg, w, cmvn)
            made[key] = (d, _recognizer(d, True), _recognizer(d, False))
        return made[key]
    yield get
    for _, a, b in made.values():
        a.Dispose()
        b.Dispose()


def _info(s):
    return [(t.id, t.time_ms, t.entry, t.fired, t.flags, t.score_bits) for t in s.TokenInfo]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lockstep_with_the_host_front_end(pairs, case):
    _, dev, host = pairs(case.bias, case.zero_cmvn)
    n = dict(ids=0, fired=0)

    def check(k, order, streams, res):
        d, h = streams
        for u in sorted(d):
            assert d[u].Tokens == h[u].Tokens, (case.name, k, u)
            assert _info(d[u]) == _info(h[u]), (case.name, k, u)
            n["ids"] += len(d[u].Tokens)
            n["fired"] += sum(t.fired for t in d[u].TokenInfo)
        assert [r.Text for r in res[0]] == [r.Text for r in res[1]], (case.name, k)
    LR.play(case.schedule, [LibSide(dev), LibSide(host)], check, drain_calls=-1)
    assert n["ids"] > 50 and n["fired"] > 5, n
    gc.collect()                                                      # the streams go: their slots are reused by the next case


def test_a_new_stream_in_a_disposed_streams_slot_starts_from_a_first_chunk(pairs):
    _, dev, host = pairs()
    audio = [LR._audio(u) for u in range(2)]
    for rnd in range(2):                                              # round 1 takes the slot round 0 left, with its carry and cache
        st = [r.CreateOnlineStream() for r in (dev, host)]
        for k in range(3):
            for s in st:
                s.AddSamples(audio[rnd][9600 * k: 9600 * (k + 1)])
            dev.GetResults(st[:1])
            host.GetResults(st[1:])
            assert st[0].Tokens == st[1].Tokens and _info(st[0]) == _info(st[1]), (rnd, k)
        assert len(st[0].Tokens) > 10
        for s in st:
            s.Dispose()
        del st, s
        gc.collect()


REFUSALS = ("token_info_off", "endpoint_on", "stream_took_audio", "snip_edges", "geometry", "then_endpoint_and_token_info_off")


@pytest.mark.parametrize("why", REFUSALS)
def test_refusals(pairs, tmp_path, why):
    """the refusals of SetDeviceFrontend.  chunk_length() is the constant 60 of this build (OnlineModel.cs:29), so that condition
    cannot be reached from outside; `geometry` stands for it and for a front-end that is not 80 mels with LFR 7 / 6 (here LFR 7 /
    5); the last case is what the mode refuses while it is on"""
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    d = pairs()[0]
    conf = d / "asr.yaml"
    if why in ("snip_edges", "geometry"):
        conf = tmp_path / "asr.yaml"
        conf.write_text(YAML.replace("snip_edges: false", "snip_edges: true") if why == "snip_edges" else YAML.replace("lfr_n: 6", "lfr_n: 5"))
    rec = OnlineRecognizer(str(d / "model.pfw"), "", str(conf), str(d / "am.mvn"), str(d / "tokens.txt"))
    calls = [lambda: rec.SetDeviceFrontend(True)]
    if why != "token_info_off":
        rec.SetTokenInfo(True)
    if why == "endpoint_on":
        rec.SetEndpoint(**LR.ENDPOINT_KEYS)
    if why == "stream_took_audio":
        s = rec.CreateOnlineStream()
        s.AddSamples(np.zeros(1, F32))
    if why == "then_endpoint_and_token_info_off":
        rec.SetDeviceFrontend(True)
        calls = [lambda: rec.SetEndpoint(**LR.ENDPOINT_KEYS), lambda: rec.SetTokenInfo(False)]
    for call in calls:
        with pytest.raises(N.PfError) as ei:
            call()
        assert ei.value.code == N.PF_ERR_UNSUPPORTED
    rec.Dispose()


def test_cli_devicefrontend(pairs):
    """`-type online -tokentimes -devicefrontend` prints what the run without -devicefrontend prints"""
    import wave
    from aliparaformerasr_amd import examples as ex
    d = pairs()[0]
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes((np.clip(W.synth_audio(24000, 3), -1, 1) * 32767).astype("<i2").tobytes())
    out = [io.StringIO(), io.StringIO()]
    texts = [ex.online_recognizer("one", d.name, "int8", 2, None, str(d.parent), out=o, tokentimes=True, devicefrontend=bool(k))
             for k, o in enumerate(out)]
    lines = [[ln for ln in o.getvalue().splitlines() if "elapsed" not in ln and "rtf" not in ln] for o in out]
    assert texts[0] == texts[1] and any(texts[0]) and lines[0] == lines[1] and "[" in out[1].getvalue()
    assert ex.main(["-type", "online", "-devicefrontend"]) == 2          # goes with -tokentimes
