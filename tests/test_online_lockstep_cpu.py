"""CPU: exact id equality against tests/online_lockstep_ref.py is a sharp enough instrument (no device: quant="fp32", numpy fbank,
numpy position encoding, the oracle's graphs).

Ids are all a recognizer shows per call.  For every case that tests/test_gpu_online_lockstep.py plays, the unmutated restatement
and each of its ten wrong assemblies (online_lockstep_ref.MUTATIONS) run on the oracle alone; a mutation counts as detected in a
case when some stream's token list differs after some call.  EVERY mutation must be detected somewhere; the table (printed,
`pytest -s`) at the chosen inputs, first differing call per case, `.` = not detected there:

      pieces ragged rotated late finish endpoint late/sparse finish/sparse pieces/zero-cmvn
    a    4      3      4      4     3      .        9            .              4
    b    2      1      2      2     3      2        7            3              2
    c    2      1      2      2     1      2        2            1              2
    d    2      1      2      4     1      4        9            4              4
    e    7      4      7      7     4      .        7            .              .
    f    2      1      2      2     1      2        2            1              2
    g    .      1      7      6     0      .        6            1              .
    h    2      1      2      4     3      2        4            3              .
    i    .      .      .      .     .      .        .            .              0
    j    .      .      .      .     2      .        .            2              .

What was changed from the inputs of tests/test_gpu_online.py, and why (the model itself is that test's, DENSE):
  * the audio is W.synth_audio under a per-frame envelope: on the stationary signal the frame before a chunk and the chunk's first
    frame are nearly one row, and (e), the lost LFR splice frame, moved no id in any schedule;
  * (i), the skipped sentinel, cannot show on an ordinary stream at all: its only exact zeros are the rows of a fresh feature cache,
    and a constant row leaves the encoder's first LayerNorm as beta whatever the constant (test_sentinel_is_invisible_on_constant_rows).
    online_lockstep_ref.zero_cmvn is an am.mvn that lands the chunk of silence exactly on minus the position encoding in some
    eighty columns of each of five rows, so exact zeros stand inside ordinary rows; `pieces` is played under it as well;
  * with predictor.out.bias = 0.8 every chunk fires 4 to 8 tokens, so no stream is ever in a decoder batch without one.  `late` and
    `finish` are played on SPARSE as well (the same weights, bias -1.5): a chunk of silence then fires none beside streams that fire.
"""
import math

import numpy as np
import pytest

import endpoint_ref as R
import online_lockstep_ref as LR
from aliparaformerasr_amd import weights as W
from oracle import frontend as fe
from oracle import online as oo

F32 = np.float32


@pytest.fixture(scope="module")
def world():
    """the models, the cases and ONE unmutated run of each, shared and left unchanged"""
    fb = {}                                                           # fbank rows per chunk of samples, shared by all runs
    models = {b: LR.model(b) for b in (LR.DENSE, LR.SPARSE)}
    silence = fe.kaldi_fbank(np.zeros(LR.CHUNK, F32), fe.FrontendConf(dither=0.0, snip_edges=False))
    assert (silence == silence[0]).all()
    zc, planted = LR.zero_cmvn(silence[0], oo.position_encode)

    def make(case, mutate=None):
        cfg, w = models[case.bias]
        return LR.LockstepRecognizer(cfg, w, zc if case.zero_cmvn else W.synth_cmvn(), LR.tokens(), mutate=mutate, fbank_cache=fb,
                                     endpoint=R.config(**LR.ENDPOINT_KEYS) if case.schedule.endpoint else None)
    cases = LR.cases()
    base = {}
    for c in cases:
        rec = make(c)
        base[c.name] = (LR.history(c.schedule, rec, drain_calls=c.drain_calls), rec.calls)
    return dict(make=make, cases=cases, base=base, models=models, planted=planted, zero_cmvn=zc)


def _first_difference(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return k
    return None if len(a) == len(b) else min(len(a), len(b))


def test_every_mutation_changes_some_token_list(world):
    table = {}
    for m in LR.MUTATIONS:
        row = []
        for c in world["cases"]:
            h = LR.history(c.schedule, world["make"](c, m), drain_calls=-1)
            row.append(_first_difference(h, world["base"][c.name][0]))
        table[m] = row
    names = [c.name for c in world["cases"]]
    print("\nfirst call at which a stream's token list differs ('.': the case does not detect the mutation)")
    print("   " + " ".join("%-*s" % (max(len(n), 3), n) for n in names))
    for m, row in table.items():
        print("%s  " % m + " ".join("%-*s" % (max(len(n), 3), "." if v is None else v) for n, v in zip(names, row))
              + "   " + LR.MUTATIONS[m])
    for m, row in table.items():
        caught = [n for n, v in zip(names, row) if v is not None]
        assert caught, "mutation %s (%s) changes no token list in any case" % (m, LR.MUTATIONS[m])
    # the six schedules on the model of tests/test_gpu_online.py alone catch all but the sentinel
    for m, row in table.items():
        assert m == "i" or any(v is not None for v in row[:6]), m


def test_the_unmutated_restatement_is_the_oracle(world):
    """without an engine and without a mutation the restated glue gives oracle.online's ids call by call (the schedules that need
    neither input_finished nor reset, which the oracle does not have)"""
    for c in world["cases"]:
        if c.schedule.name in ("finish", "endpoint"):
            continue
        cfg, w = world["models"][c.bias]
        orc = oo.OnlineRecognizer(cfg, w, world["zero_cmvn"] if c.zero_cmvn else W.synth_cmvn(), LR.tokens(), quant="fp32")
        assert LR.history(c.schedule, orc) == world["base"][c.name][0], c.name


def test_ragged_counts_and_work_sets(world):
    calls = {n: c for n, (_, c) in world["base"].items()}
    dense = [x for n in ("pieces", "ragged", "rotated", "late", "finish", "endpoint") for x in calls[n]]
    assert any(L > 0 and len(set(lens)) > 1 for _, L, lens in dense)                 # two streams differ in lens
    sparse = calls["late/sparse"] + calls["finish/sparse"]
    assert any(L > 0 and 0 in lens for _, L, lens in sparse)                         # one stream has none, the decoder runs
    assert any(B > 0 and L == 0 for B, L, _ in sparse)                               # nobody has one: no decoder call at all
    assert {B for B, _, _ in calls["ragged"]} == {0, 1, 2, 3}                       # work sets of every size, and no work
    assert {B for B, _, _ in calls["finish"]} >= {0, 1, 3}
    # every case decodes something on every stream (a closed sentence empties the list again)
    for c in world["cases"]:
        hist = world["base"][c.name][0]
        for u in range(c.schedule.n_streams):
            assert max(len(snap[u]) for snap in hist if snap[u] is not None) > 2, (c.name, u)


def test_endpoint_case_closes_sentences(world):
    """on the oracle the sentences close by the definition (tests/endpoint_ref.py); on the device the library closes them"""
    c = [x for x in world["cases"] if x.schedule.endpoint][0]
    rec = world["make"](c)
    closed = []

    def check(k, order, streams, res):
        closed.append([len(streams[0][u].sentences) for u in order])
    LR.play(c.schedule, [LR.RefSide(rec)], check)
    assert closed[-1] == [2, 2, 2] and closed[0] == [0, 0, 0]


def test_sentinel_is_invisible_on_constant_rows(world):
    """why (i) needs zero_cmvn: whole rows of 0 and whole rows of the sentinel are the same bytes behind the encoder"""
    g = world["make"](world["cases"][0]).graphs
    sp = (np.random.default_rng(0).standard_normal((1, 20, 560)) * 4).astype(F32)
    a, b = sp.copy(), sp.copy()
    a[0, :10], b[0, :10] = 0, oo.SENTINEL
    (ea, aa), (eb, ab) = g.encoder(a), g.encoder(b)
    assert (ea.view(np.uint32) == eb.view(np.uint32)).all() and (aa.view(np.uint32) == ab.view(np.uint32)).all()
    # under zero_cmvn the first chunk of a stream has exact zeros inside ordinary rows, where the planted pairs say
    c = [x for x in world["cases"] if x.zero_cmvn][0]
    s = world["make"](c).create_stream()
    s.add_samples(np.zeros(1, F32))
    chunk = s.get_decode_chunk()
    zeros = set((int(t), int(k)) for t, k in zip(*np.nonzero(chunk[10:] == 0)))
    assert zeros >= set(world["planted"]) and len(world["planted"]) >= 300      # (a slow cosine column cancels in two rows)
    assert ((chunk[10:15] == 0).sum(axis=1) >= 60).all() and not (chunk[10:] == 0).all(axis=1).any()
    assert (chunk[:10] == 0).all()


def test_input_finished_queues_every_cached_sample(world):
    """the restated input_finished leaves cache_samples empty and queues ceil(n / 9600) chunks, the last zero-padded"""
    rec = world["make"](world["cases"][0])
    rng = np.random.default_rng(8)
    for fed in ((), (1,), (9600,), (16000, 3237), (9600, 9600, 9600), (123, 30000)):
        s = rec.create_stream()
        for n in fed:
            s.add_samples((0.1 * rng.standard_normal(n)).astype(F32))
        n, chunks, frames = len(s.cache_samples), s.chunks_in, s.speech.shape[0]
        assert n >= 1                                                # a chunk leaves only ABOVE 9600 cached samples
        first = chunks == 0
        s.input_finished()
        assert len(s.cache_samples) == 0 and s.finished
        assert s.chunks_in - chunks == math.ceil(n / LR.CHUNK)
        assert s.speech.shape[0] - frames == 60 * math.ceil(n / LR.CHUNK) + (1 if first else 0)
        before = s.speech.shape[0]
        s.input_finished()                                            # nothing is left: nothing happens
        assert s.speech.shape[0] == before
    # the zero-padded tail: 37 samples of a tone and then silence -> the last rows are the rows of silence
    s = rec.create_stream()
    s.add_samples(np.zeros(1, F32))
    s.cache_samples = np.sin(np.arange(37, dtype=F32))
    s.input_finished()
    silence = rec.fbank(np.zeros(LR.CHUNK, F32))[0]
    assert (s.speech[-50:] == silence).all() and not (s.speech[-60] == silence).all()


def test_cmvn_and_scale_equal_a_scalar_loop():
    """ApplyCmvn and the sqrt(512) scale of OnlineStreamM::GetDecodeChunk, one float32 / double operation at a time"""
    shift, scale = W.synth_cmvn()
    x = (np.random.default_rng(9).standard_normal((3, 560)) * 7 - 5).astype(F32)
    x[1, :7] = [0.0, -0.0, 1e-30, -15.942385, 3e4, -3e4, 1.0]
    got = LR.cmvn_scale(x, shift, scale)
    root = math.pow(512.0, 0.5)
    want = np.zeros_like(x)
    for i in range(x.shape[0]):
        for k in range(560):
            s = F32(F32(x[i, k]) + F32(shift[k]))                     # const volatile float s = x + sh
            v = F32(s * F32(scale[k]))                                # x = s * sc
            want[i, k] = F32(float(v) * root)                         # (float)((double)v * root)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
