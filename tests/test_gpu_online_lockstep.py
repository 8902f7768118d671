"""GPU: the streaming recognizer held to an exact answer, and stream isolation at its two device seams.

  * premise: online_encoder / online_decoder return the same bytes twice on one engine, and on two engines built from the same
    files, the second after an unrelated larger call.  Only then can a second engine stand in for the recognizer's own.
  * lockstep: OnlineRecognizer against tests/online_lockstep_ref.py (the oracle's glue around a second engine's fbank, libm's
    position encoding and the two graphs): after EVERY GetResults of every case every stream's Tokens are the restated stream's
    ids as lists, and every Text is decode_text of them.  No tolerance and no share of ids excused.  The cases
    (online_lockstep_ref.cases): today's 4000-sample pieces; ragged pieces (work sets of 0 to 3 streams); the list rotated every
    call and once a strict subset; a stream created late; InputFinished with 0, 1, 9600 and 9600 + 37 cached samples and the
    drain; the endpoint on (every first_pass is the restated text before the reset, exact equality goes on after it); `late` and
    `finish` again with a predictor bias at which a chunk of silence fires no token; `pieces` again under an am.mvn that puts
    exact zeros inside ordinary rows, so that the sentinel matters.  tests/test_online_lockstep_cpu.py shows on the oracle alone
    that ten wrong assemblies each change an id in these cases.  A second recognizer replays the ragged pieces to the same ids.
  * isolation: the seams run in fp16 with no whole-tensor quantiser, so a stream's output rows are a function of its own inputs
    and position.  Another stream's chunk (encoder) or its rows, embeddings, length and caches (decoder) are replaced: every other
    stream's outputs must be the same bytes.

Trial against deliberately wrong builds (scratch copies of csrc/online.cpp, not kept): with the FSMN caches taken from the
neighbouring stream of the work set the lockstep fails first at (pieces, call 4, stream 0); with layer l's cache built from
layer l's state at (pieces, call 2, stream 0) -- the calls tests/test_online_lockstep_cpu.py's table names.

Wall time on an MI355X: this file 3.6 s (tests/test_gpu_online.py at the parent commit: 3.0 s).
"""
import numpy as np
import pytest

import online_lockstep_ref as LR
import rows_ref as R
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import online as oo

pytestmark = pytest.mark.gpu

F32 = np.float32
YAML = ("model: paraformer\nfrontend_conf:\n  fs: 16000\n  window: hamming\n  n_mels: 80\n  dither: 0\n  lfr_m: 7\n  lfr_n: 6\n"
        "  snip_edges: false\n")


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _write(d, cfg, w, cmvn):
    W.save_pfw(str(d / "model.pfw"), cfg, w)
    (d / "am.mvn").write_text(fe.format_mvn_text(*cmvn))
    (d / "asr.yaml").write_text(YAML)
    (d / "tokens.txt").write_text("\n".join(LR.tokens()) + "\n", encoding="utf-8")
    return d


def _engine(d):
    """an engine from the files and the yaml's values, as OnlineRecognizerM's constructor builds its own"""
    from aliparaformerasr_amd.engine import Engine
    return Engine(weights_path=str(d / "model.pfw"), mvn_path=str(d / "am.mvn"), device=0, dither=0.0, snip_edges=False,
                  lfr_m=7, lfr_n=6, n_mels=80, fs=16000, window="hamming")


def _recognizer(d):
    from aliparaformerasr_amd.online_recognizer import OnlineRecognizer
    return OnlineRecognizer(str(d / "model.pfw"), "", str(d / "asr.yaml"), str(d / "am.mvn"), str(d / "tokens.txt"))


class Rig:
    """a recognizer and the restatement around a SECOND engine, both from one directory of files"""

    def __init__(self, d, cfg, w):
        self.d = d
        self.rec = _recognizer(d)
        self.eng = _engine(d)
        cmvn = fe.parse_mvn_text((d / "am.mvn").read_text())
        self.ref = LR.LockstepRecognizer(cfg, w, cmvn, LR.tokens(), engine=self.eng, quant="fp16")

    def close(self):
        self.rec.Dispose()
        self.eng.close()


@pytest.fixture(scope="module")
def rigs(tmp_path_factory):
    """one rig per (model, am.mvn) that the cases name, built when first asked for"""
    made = {}

    def get(bias=LR.DENSE, zero_cmvn=False):
        key = (bias, zero_cmvn)
        if key not in made:
            cfg, w = LR.model(bias)
            cmvn = W.synth_cmvn()
            if zero_cmvn:                                             # from the DEVICE's rows of silence and libm's encoding
                base = get(bias)
                silence = base.eng.fbank(np.zeros(LR.CHUNK, F32))
                assert silence.shape == (60, 80) and (_bits(silence) == _bits(silence[0])).all()
                cmvn, planted = LR.zero_cmvn(silence[0], base.ref.position_encode)
            made[key] = Rig(_write(tmp_path_factory.mktemp("lockstep"), cfg, w, cmvn), cfg, w)
        return made[key]
    yield get
    for r in made.values():
        r.close()


# ------------------------------------------------------------------------------------------------ premise
def _seam_inputs(B, nl, Tc=20):
    r = np.random.default_rng([41, B])
    speech = (r.standard_normal((B, Tc, 560)) * 4).astype(F32)
    speech[B - 1, : Tc // 2] = oo.SENTINEL
    L = (4, 7, 10)[B - 1]
    lens = np.asarray([L, 3, 0][:B], np.int32)
    emb = r.standard_normal((B, L, 512)).astype(F32)
    for b in range(B):
        emb[b, lens[b]:] = 0
    caches = [r.standard_normal((B, 512, 10)).astype(F32) for _ in range(nl)]
    return speech, emb, lens, caches


def _seams(eng, speech, emb, lens, caches):
    enc, al = eng.online_encoder(speech)
    logp, ids, cout = eng.online_decoder(enc, emb, lens, caches)
    _, ids2, cout2 = eng.online_decoder(enc, emb, lens, caches, want_logits=False)
    return [_bits(enc), _bits(al), _bits(logp), ids, ids2] + [_bits(c) for c in cout] + [_bits(c) for c in cout2]


def test_premise_same_bytes_twice_and_on_two_engines(rigs):
    rig = rigs()
    nl = 3
    first = {}
    for B in (1, 2, 3):
        x = _seam_inputs(B, nl)
        first[B] = _seams(rig.eng, *x)
        for a, b in zip(first[B], _seams(rig.eng, *x)):
            assert (a == b).all(), B
    other = _engine(rig.d)
    big = (np.random.default_rng(42).standard_normal((8, 20, 560)) * 9).astype(F32)     # leftovers of another shape and scale
    enc8, _ = other.online_encoder(big)
    other.online_decoder(enc8, np.ones((8, 13, 512), F32), np.full(8, 13, np.int32), [np.ones((8, 512, 10), F32)] * nl)
    for B in (3, 1, 2):
        for a, b in zip(first[B], _seams(other, *_seam_inputs(B, nl))):
            assert (a == b).all(), B
    other.close()


# ------------------------------------------------------------------------------------------------ lockstep
class LibSide:
    """an OnlineRecognizer behind the four verbs of a schedule"""

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


CASES = LR.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lockstep(rigs, case):
    rig = rigs(case.bias, case.zero_cmvn)
    toks = LR.tokens()
    seen = {}
    n_checked = [0, 0]
    if case.schedule.endpoint:
        rig.rec.SetEndpoint(**LR.ENDPOINT_KEYS)

    def check(k, order, streams, res):
        lib, ref = streams
        for i, u in enumerate(order):                                 # sentences closed in this call: first_pass, then the reset
            if not case.schedule.endpoint:
                continue
            sen = lib[u].Sentences
            for j in range(seen.get(u, 0), len(sen)):
                assert sen[j].first_pass == oo.decode_text(toks, ref[u].tokens), (case.name, k, u, j)
                assert sen[j].text == sen[j].first_pass and sen[j].result is None
                ref[u].reset()
                n_checked[1] += 1
            seen[u] = len(sen)
        for u in sorted(lib):                                         # every stream, also one this call did not pass
            assert lib[u].Tokens == ref[u].tokens, (case.name, k, u)
            n_checked[0] += len(ref[u].tokens)
        for i, u in enumerate(order):
            assert res[0][i].Text == oo.decode_text(toks, ref[u].tokens), (case.name, k, u)
    try:
        LR.play(case.schedule, [LibSide(rig.rec), LR.RefSide(rig.ref)], check, drain_calls=case.drain_calls)
    finally:
        if case.schedule.endpoint:
            rig.rec.SetEndpoint(False)
    assert n_checked[0] > 50
    if case.schedule.endpoint:
        assert n_checked[1] == 6                                      # two sentences on each of the three streams


def test_a_second_recognizer_replays_the_ragged_pieces(rigs):
    rig = rigs()
    rec2 = _recognizer(rig.d)
    sched = [c.schedule for c in CASES if c.name == "ragged"][0]
    n = [0]

    def check(k, order, streams, res):
        for u in streams[0]:
            assert streams[0][u].Tokens == streams[1][u].Tokens, (k, u)
            n[0] = max(n[0], len(streams[0][u].Tokens))
        assert [r.Text for r in res[0]] == [r.Text for r in res[1]], k
    LR.play(sched, [LibSide(rig.rec), LibSide(rec2)], check)
    assert n[0] > 20
    rec2.Dispose()


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize("Tc,big", ((5, False), (8, False), (20, False), (20, True)))
def test_encoder_rows_depend_on_their_own_stream_only(rigs, Tc, big):
    eng = rigs().eng
    small_max = eng.short_input_max_rows()
    B = small_max // Tc + 1 if big else 3
    assert B * Tc > small_max if big else B * Tc <= small_max
    r = np.random.default_rng([43, Tc, B])
    speech = (r.standard_normal((B, Tc, 560)) * 4).astype(F32)
    speech[1, : Tc // 2] = oo.SENTINEL
    enc, al = eng.online_encoder(speech)
    for j in (0, 1, B - 1):
        sp = speech.copy()
        sp[j] = (r.standard_normal((Tc, 560)) * 40).astype(F32)      # ten times the scale ...
        sp[j, : (Tc + 1) // 2] = oo.SENTINEL                          # ... behind a first half of sentinel rows
        e2, a2 = eng.online_encoder(sp)
        for b in range(B):
            same = (_bits(e2[b]) == _bits(enc[b])).all() and (_bits(a2[b]) == _bits(al[b])).all()
            assert same == (b != j), (j, b)


def _dec_variants(L, n):
    return sorted({0, L, max(n - 1, 0), min(n + 1, L)} - {n})


@pytest.mark.parametrize("L,lens", R.DEC_CASES)
def test_decoder_rows_depend_on_their_own_stream_only(rigs, L, lens):
    eng = rigs().eng
    nl = 3
    r = np.random.default_rng([44, L])
    enc = r.standard_normal((3, 20, 512)).astype(F32)
    emb, ln, caches = R.online_decoder_inputs(L, lens, nl)
    logp, ids, cout = eng.online_decoder(enc, emb, ln, caches)
    for j in range(3):
        for n in _dec_variants(L, lens[j]):
            enc2, emb2, ln2 = enc.copy(), emb.copy(), ln.copy()
            enc2[j] = (r.standard_normal((20, 512)) * 3).astype(F32)
            emb2[j] = 0
            emb2[j, :n] = (r.standard_normal((n, 512)) * 3).astype(F32)
            ln2[j] = n
            caches2 = [c.copy() for c in caches]
            for c in caches2:
                c[j] = (r.standard_normal((512, 10)) * 3).astype(F32)
            lp2, ids2, cout2 = eng.online_decoder(enc2, emb2, ln2, caches2)
            _, ids3, cout3 = eng.online_decoder(enc2, emb2, ln2, caches2, want_logits=False)
            for b in range(3):
                if b == j:
                    continue
                assert (ids2[b] == ids[b]).all() and (ids3[b] == ids[b]).all(), (j, n, b)
                assert (_bits(lp2[b]) == _bits(logp[b])).all(), (j, n, b)
                for l in range(nl):
                    assert (_bits(cout2[l][b]) == _bits(cout[l][b])).all() and (_bits(cout3[l][b]) == _bits(cout[l][b])).all(), (j, n, b, l)
            assert (_bits(lp2[j]) != _bits(logp[j])).any(), (j, n)    # (its caches may both be all +0: L >= 10, nothing valid late)
