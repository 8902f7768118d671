"""GPU: OnlineRecognizer.SetTokenInfo — the device-resident chunk step (Engine::online_step: the carried CIF as a kernel, the
FSMN caches in per-stream slots) and the token info it brings.

  * lockstep: every case of online_lockstep_ref.cases with the mode on.  After EVERY GetResults every stream's Tokens and Text are
    the restated stream's (tests/cif_stream_ref.py TimedRecognizer: online_lockstep_ref around a second engine), exactly, and a
    second recognizer with the mode off, fed the same schedule, has the same Tokens.  That includes the endpoint case, the SPARSE
    model (streams that fire nothing, calls in which nobody fires) and the zero-CMVN case.
  * info, in the same runs: len(TokenInfo) == len(Tokens) with equal ids; the fired flags and the fire entries are the restated
    CIF's; time_ms is the restated time rule; score has the bits of the second engine's online_decoder(..., want_logits=True)
    log-probs at the chosen ids (tests/test_gpu_online_lockstep.py's premise test is what allows that comparison).
  * sentences: every closed sentence's tokens are the stream's token info as of the closing call; TokenInfo is empty after it.
  * slots: a stream disposed mid-run and a new stream in its slot; growth from 1 to 9 streams and past the first 64 slots.
  * refusals: SetTokenInfo once a stream has decoded; TokenInfo == [] with the mode off; a stream twice in one call.
  * the endpoint model attached behind streams that already hold their slots; the command line.
"""
import gc

import numpy as np
import pytest

import cif_stream_ref as CR
import online_lockstep_ref as LR
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import online as oo

pytestmark = pytest.mark.gpu

F32 = np.float32
YAML = ("model: paraformer\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n"
        "  snip_edges: false\n")


def _write(d, cfg, w, cmvn):
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*cmvn))
    (d / "asr.yaml").write_text(YAML)
    (d / "tokens.txt").write_text("\n".join(LR.tokens()) + "\n", encoding="utf-8")
    return d


def _engine(d):
    from aliparaformerasr_amd.engine import Engine
    return Engine(weights_path=str(d / "model.pfw"), mvn_path=str(d / "am.mvn"), device=0, dither=0.0, snip_edges=False,
                  lfr_m=7, lfr_n=6, n_mels=80, fs=16000, window="hamming")


def _recognizer(d, token_info):
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    rec = OnlineRecognizer(str(d / "model.pfw"), "", str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))
    if token_info:
        rec.SetTokenInfo(True)
    return rec


class Rig:
    """a recognizer with the mode on, one with the mode off, and the restatement around a THIRD engine, all from one directory"""

    def __init__(self, d, cfg, w):
        self.d = d
        self.rec, self.off = _recognizer(d, True), _recognizer(d, False)
        self.eng = _engine(d)
        cmvn = fe.parse_mvn_text((d / "am.mvn").read_text())
        self.ref = CR.TimedRecognizer(cfg, w, cmvn, LR.tokens(), engine=self.eng, quant="fp16")

    def close(self):
        self.rec.Dispose()
        self.off.Dispose()
        self.eng.close()


@pytest.fixture(scope="module")
def rigs(tmp_path_factory):
    made = {}

    def get(bias=LR.DENSE, zero_cmvn=False):
        key = (bias, zero_cmvn)
        if key not in made:
            cfg, w = LR.model(bias)
            cmvn = W.synth_cmvn()
            if zero_cmvn:
                base = get(bias)
                silence = base.eng.fbank(np.zeros(LR.CHUNK, F32))
                cmvn, _ = LR.zero_cmvn(silence[0], base.ref.position_encode)
            made[key] = Rig(_write(tmp_path_factory.mktemp("tokeninfo"), cfg, w, cmvn), cfg, w)
        return made[key]
    yield get
    for r in made.values():
        r.close()


class LibSide:
    def __init__(self, rec):
        self.rec = rec

    def new(self):
        return self.rec.CreateOnlineStream()

    def add(self, s, x):
        s.AddSamples(x)

    def fin(self, s):
        s.InputFinished()

    def get(self, streams):
        return self.rec.GetResults(streams)

    def tokens(self, s):
        return s.Tokens


def _same_info(got, want, where):
    """a stream's TokenInfo (or a sentence's tokens) against the restated stream's info"""
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.id, g.time_ms, g.entry, g.fired) == w[:4], (where, i, tuple(g), g.entry, w)
        assert g.flags == (3 if w[3] else 0), (where, i)
        assert g.score_bits == (0 if w[4] is None else w[4]), (where, i)


CASES = LR.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lockstep_and_info(rigs, case):
    rig = rigs(case.bias, case.zero_cmvn)
    toks = LR.tokens()
    seen = {}
    n = dict(ids=0, fired=0, padding=0, sentences=0, timed_late=0, empty_calls=0)
    if case.schedule.endpoint:
        rig.rec.SetEndpoint(**LR.ENDPOINT_KEYS)
        rig.off.SetEndpoint(**LR.ENDPOINT_KEYS)

    def check(k, order, streams, res):
        lib, ref, off = streams
        for u in order:                                               # sentences closed in this call: what they kept, then the reset
            if not case.schedule.endpoint:
                continue
            sen, sen_off = lib[u].Sentences, off[u].Sentences
            assert len(sen) == len(sen_off), (case.name, k, u)
            for j in range(seen.get(u, 0), len(sen)):
                assert sen[j].first_pass == oo.decode_text(toks, ref[u].tokens) == sen_off[j].first_pass, (case.name, k, u, j)
                _same_info(sen[j].tokens, ref[u].info, (case.name, k, u, "sentence", j))
                assert sen_off[j].tokens == []
                assert lib[u].TokenInfo == [] and lib[u].Tokens == []                  # cleared at the reset
                ref[u].reset()
                n["sentences"] += 1
            seen[u] = len(sen)
        for u in sorted(lib):                                         # every stream, also one this call did not pass
            assert lib[u].Tokens == ref[u].tokens, (case.name, k, u)
            assert off[u].Tokens == ref[u].tokens, (case.name, k, u)
            _same_info(lib[u].TokenInfo, ref[u].info, (case.name, k, u))
            assert off[u].TokenInfo == []
            n["ids"] += len(ref[u].tokens)
            n["fired"] += sum(1 for w in ref[u].info if w[3])
            n["padding"] += sum(1 for w in ref[u].info[2:] if not w[3])
            n["timed_late"] += sum(1 for w in ref[u].info if w[3] and w[1] > 600)
        n["empty_calls"] += rig.ref.calls[-1][0] > 0 and rig.ref.calls[-1][1] == 0
        for i, u in enumerate(order):
            assert res[0][i].Text == oo.decode_text(toks, ref[u].tokens) == res[2][i].Text, (case.name, k, u)
    try:
        LR.play(case.schedule, [LibSide(rig.rec), LR.RefSide(rig.ref), LibSide(rig.off)], check, drain_calls=case.drain_calls)
    finally:
        if case.schedule.endpoint:
            rig.rec.SetEndpoint(False)
            rig.off.SetEndpoint(False)
    # not vacuous (counted over the calls; SPARSE fires 1 to 3 tokens per chunk of audio and `finish` is 2 s of it at most)
    few = case.bias == LR.SPARSE
    assert n["ids"] > 50 and n["fired"] > (5 if few else 20) and n["timed_late"] > (0 if few else 5), n
    if case.schedule.endpoint:
        assert n["sentences"] == 6, n
    if case.bias == LR.SPARSE:
        assert n["padding"] > 0 and n["empty_calls"] > 0, n          # streams with fewer tokens than the batch; calls where nobody fires
    gc.collect()                                                      # the streams go: their slots are reused by the next case


def _feed(recs, streams, u, x):
    for r in range(len(recs)):
        streams[r][u].AddSamples(x)


def test_a_new_stream_in_a_disposed_streams_slot(rigs):
    rig = rigs()
    recs = [rig.rec, rig.off]
    audio = [LR._audio(u) for u in range(3)]
    st = [{u: r.CreateOnlineStream() for u in (0, 1)} for r in recs]
    fired = 0

    def step(k, order):
        nonlocal fired
        for u in order:
            src = audio[2 if u == 2 else u]
            _feed(recs, st, u, src[9600 * k[u]: 9600 * (k[u] + 1)])
            k[u] += 1
        res = [r.GetResults([s[u] for u in order]) for r, s in zip(recs, st)]
        for u in order:
            assert st[0][u].Tokens == st[1][u].Tokens, (k, u)
            assert [t.id for t in st[0][u].TokenInfo] == st[0][u].Tokens
            fired += sum(t.fired for t in st[0][u].TokenInfo)
        assert [x.Text for x in res[0]] == [x.Text for x in res[1]]
    k = {0: 0, 1: 0, 2: 0}
    for _ in range(3):
        step(k, (0, 1))
    for s in st:                                                      # stream 1 goes mid-run, with a carry and caches in its slot
        s[1].Dispose()
        del s[1]
    gc.collect()
    for r, s in zip(recs, st):
        s[2] = r.CreateOnlineStream()                                 # takes the slot stream 1 had
    for _ in range(3):                                                # the mode-off side's new stream carries a fresh host state:
        step(k, (0, 2))                                               # equal ids mean the slot started from zeros
    assert fired > 30


@pytest.mark.parametrize("n_streams", (9, 70))
def test_growing_keeps_the_first_streams_ids(rigs, n_streams):
    """one stream, then n_streams (70: past the first allocation of 64 slots, the buffer is reallocated and copied on the device)"""
    rig = rigs()
    recs = [rig.rec, rig.off]
    a0 = LR._audio(0)
    st = [{0: r.CreateOnlineStream()} for r in recs]
    for k in range(2):
        _feed(recs, st, 0, a0[9600 * k: 9600 * (k + 1)])
        for r, s in zip(recs, st):
            r.GetResults([s[0]])
    assert len(st[0][0].Tokens) > 8 and st[0][0].Tokens == st[1][0].Tokens
    others = [LR._audio(1)[:9600], LR._audio(2)[:9600]]
    for r, s in zip(recs, st):
        for u in range(1, n_streams):
            s[u] = r.CreateOnlineStream()
    for k in range(2, 4):
        _feed(recs, st, 0, a0[9600 * k: 9600 * (k + 1)])
        for u in range(1, n_streams):
            _feed(recs, st, u, others[u % 2] if k == 2 else others[(u + 1) % 2])
        for r, s in zip(recs, st):
            r.GetResults([s[u] for u in range(n_streams)])
        for u in range(n_streams):
            assert st[0][u].Tokens == st[1][u].Tokens, (k, u)
    assert len(st[0][0].Tokens) > 20
    assert sum(t.fired for t in st[0][n_streams - 1].TokenInfo) >= 6
    st.clear()
    gc.collect()


def test_refusals(rigs):
    from aliparaformerasr_amd import _native as N
    rig = rigs()
    rec = _recognizer(rig.d, False)
    rec.SetTokenInfo(False)                                           # a no-op on a fresh recognizer
    s = rec.CreateOnlineStream()
    s.AddSamples(LR._audio(0)[:9600])
    rec.SetTokenInfo(True)                                            # nothing decoded yet: allowed, also with a live stream
    rec.SetTokenInfo(False)
    rec.GetResults([s])
    assert len(s.Tokens) > 2 and s.TokenInfo == []                    # the mode is off
    with pytest.raises(N.PfError) as ei:
        rec.SetTokenInfo(True)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    del s
    gc.collect()
    rec.SetTokenInfo(True)                                            # the stream is gone
    s = rec.CreateOnlineStream()
    assert [tuple(t) for t in s.TokenInfo] == [(0, -1, 0.0, False)] * 2 == [(t, -1, 0.0, False) for t in s.Tokens]
    s.AddSamples(LR._audio(0)[:9600])
    rec.GetResults([s])
    assert len(s.TokenInfo) == len(s.Tokens) > 2
    with pytest.raises(N.PfError) as ei:
        rec.SetTokenInfo(False)
    assert ei.value.code == N.PF_ERR_UNSUPPORTED
    del s
    rec.Dispose()


def test_cli_tokentimes(tmp_path):
    """`-type online -tokentimes`: the texts of the run without the flag, and under each a `token[time_ms score]` line"""
    import io
    import re
    import wave
    from aliparaformerasr_amd import examples as ex
    d = tmp_path / "toy-online"
    d.mkdir()
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=2, vocab=150)
    w = W.synth_weights(cfg, 45)
    w["predictor.out.bias"] = np.asarray([0.8], F32)
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*W.synth_cmvn()))
    toks = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 5 * i) for i in range(146)] + ["<unk>"]
    (d / "tokens.txt").write_text("\n".join(toks) + "\n", encoding="utf-8")
    (d / "asr.yaml").write_text("model: paraformer\nfrontend_conf:\n  dither: 0.0\n")
    with wave.open(str(d / "a.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes((np.clip(W.synth_audio(24000, 3), -1, 1) * 32767).astype("<i2").tobytes())
    plain, timed = io.StringIO(), io.StringIO()
    want = ex.online_recognizer("one", "toy-online", "int8", 2, None, str(tmp_path), out=plain)
    got = ex.online_recognizer("one", "toy-online", "int8", 2, None, str(tmp_path), out=timed, tokentimes=True)
    assert got == want and any(got)
    lines = timed.getvalue().splitlines()
    item = r"\S+\[\d+ -?\d+\.\d{3}\]"
    line = re.compile("^%s( %s)*$" % (item, item))
    n_lines = 0
    for i, ln in enumerate(lines):
        if i and lines[i - 1] in got and line.match(ln):
            n_lines += 1
            times = [int(x) for x in re.findall(r"\[(\d+) ", ln)]
            assert times == sorted(times)
    assert n_lines >= 3
    assert "[" not in plain.getvalue().replace("Init", "")


def test_a_stream_twice_in_one_call_is_refused_before_a_chunk_is_taken(rigs):
    from aliparaformerasr_amd import _native as N
    rig = rigs()
    a = LR._audio(0)
    s, t = rig.rec.CreateOnlineStream(), rig.rec.CreateOnlineStream()
    for k in range(2):
        s.AddSamples(a[9600 * k: 9600 * (k + 1)])
        t.AddSamples(a[9600 * k: 9600 * (k + 1)])
    rig.rec.GetResults([s, t])
    before = s.Tokens
    with pytest.raises(N.PfError) as ei:
        rig.rec.GetResults([s, t, s])
    assert ei.value.code == N.PF_ERR_INVALID_ARG
    assert s.Tokens == before and t.Tokens == before                  # nobody's chunk was taken ...
    rig.rec.GetResults([s, t])                                        # ... it is decoded now
    assert len(s.Tokens) > len(before) and s.Tokens == t.Tokens
    o = rig.off.CreateOnlineStream()                                  # the mode-off path takes the list as the reference does
    o.AddSamples(a[:9600])
    rig.off.GetResults([o, o])
    del s, t, o
    gc.collect()


def test_endpoint_model_attached_behind_streams_that_hold_slots(rigs, tmp_path):
    """SetTokenInfo, decode, SetEndpointModel, SetEndpoint: the streams hold their slots before the network's state buffer exists.
    Their sentences, tokens and token info are those of a recognizer that had the model from the start.  The pool is used and
    given back first (a run with the model up to the flush), so that the buffer the late attach allocates is not fresh memory."""
    import vad_ref as V
    import vadnet_ref as R
    from aliparaformerasr_amd import engine as E
    rig = rigs()
    audio = [V.burst_audio(LR.SECONDS, list(b), 40 + i) for i, b in enumerate(LR.ENDPOINT_BURSTS)]
    rows = np.concatenate([rig.eng.fbank(audio[0][off: off + LR.CHUNK]) for off in range(0, LR.N, LR.CHUNK)])
    cfg, w = R.energy_model(rows)
    path = str(tmp_path / "vad.pfw")
    W.save_pfw(path, cfg, w)
    ep = E.endpoint_model_config(**LR.ENDPOINT_KEYS)

    def feed(rec, streams, start):
        hist = []
        for off in range(start, LR.N, 4000):
            for s, a in zip(streams, audio):
                s.AddSamples(a[off: off + 4000])
            rec.GetResults(streams)
            hist.append([([(x.begin_ms, x.end_ms, x.kind, x.first_pass, [tuple(t) + (t.entry,) for t in x.tokens]) for x in s.Sentences],
                          s.Tokens, [tuple(t) + (t.entry,) for t in s.TokenInfo]) for s in streams])
        for s in streams:
            s.InputFinished()
        for _ in range(3):
            rec.GetResults(streams)
            hist.append([([(x.begin_ms, x.end_ms, x.kind, x.first_pass) for x in s.Sentences], s.Tokens) for s in streams])
        return hist
    ra, rb = _recognizer(rig.d, True), _recognizer(rig.d, True)
    rb.SetEndpointModel(path)                                         # the model from the start
    ra.SetEndpointModel(path)                                         # the pool, used up to the flush and given back
    ra.SetEndpoint(ep)
    used = [ra.CreateOnlineStream() for _ in audio]
    assert sum(len(x[0]) for x in feed(ra, used, 0)[-1]) >= 3
    del used
    gc.collect()
    ra.SetEndpoint(False)
    ra.SetEndpointModel(None)
    sa, sb = [ra.CreateOnlineStream() for _ in audio], [rb.CreateOnlineStream() for _ in audio]
    for rec, streams in ((ra, sa), (rb, sb)):                         # the constructor's silence is decoded: every stream holds a slot
        for s, a in zip(streams, audio):
            s.AddSamples(a[:1])
        rec.GetResults(streams)
        assert all(len(s.Tokens) > 2 for s in streams)
    ra.SetEndpointModel(path)                                         # accepted: no live stream has fed the detector
    ra.SetEndpoint(ep)
    rb.SetEndpoint(ep)
    ha, hb = feed(ra, sa, 1), feed(rb, sb, 1)
    assert ha == hb
    assert all(len(x[0]) >= 1 for x in ha[-1]) and sum(len(x[0]) for x in ha[-1]) >= 3
    del sa, sb
    gc.collect()
    ra.Dispose()
    rb.Dispose()
