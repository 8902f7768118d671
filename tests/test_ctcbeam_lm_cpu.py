"""CPU: n-gram LM shallow fusion inside the CTC prefix beam search — the definition (tests/ctcbeam_lm_ref.py) against brute-force
enumeration scored log(sum of alignments) + g, the builder and scorer (pf_host_lm_build / pf_host_lm_score, csrc/lm.cpp) against
the plain-text step at every position, the ARPA reader against the reference's, the host twin (pf_host_ctc_beam_lm) against the
definition over the committed inputs with the condition those inputs must meet (a decision gap of 1000 tolerances over fused
keys and final scores), alpha = beta = 0 = no change, one case worked by hand, refusals, limits and symbols, and all of the host
code once more in a stand-alone program under ASan + UBSan."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctcbeam_bias_ref as BR
import ctcbeam_lm_ref as LR
import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import LanguageModel, host_ctc_beam, host_ctc_beam_hot, host_ctc_beam_lm

EOS = LR.PF_LM_EOS


def native(model):
    """The library's model of a reference Model."""
    return LanguageModel(model.order, model.ngrams, model.V, model.bos, model.eos, model.unk, model.oov, sorted(model.transparent))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


# ---- the definition against brute force -------------------------------------------------------------------------------------------
def small_models(V):
    """Orders 1, 2 and 3, with and without bos / eos / unk, a transparent id, an id missing from the unigrams."""
    rng = np.random.default_rng(V)
    w = lambda: np.float32(rng.uniform(-3, -0.2))                                      # noqa: E731
    uni = {(c,): (w(), w()) for c in range(1, V)}
    bi = {(a, b): (w(), w() if (a + b) % 2 else None) for a in range(1, V) for b in range(1, V) if (a * 3 + b) % 4}
    tri = {(a, b, c): (w(), None) for a in range(1, V) for b in range(1, V) for c in range(1, V) if (a + 2 * b + c) % 3 == 0}
    less = {k: v for k, v in uni.items() if k != (V - 1,)}
    bi_less = {k: v for k, v in bi.items() if V - 1 not in k}
    return [LR.Model(1, uni, V), LR.Model(2, {**uni, **bi}, V, bos=1, eos=2), LR.Model(3, {**uni, **bi, **tri}, V, bos=2, eos=1),
            LR.Model(2, {**less, **bi_less}, V, oov=-4.0), LR.Model(2, {**less, **bi_less}, V, unk=1, eos=2),
            LR.Model(3, {**uni, **tri}, V, transparent=(1,), eos=2)]


@pytest.mark.parametrize("T,V", [(5, 3), (3, 4)])
def test_definition_against_brute_force(T, V):
    logp = R.random_rows(900 + T, T, V)
    brute = R.brute_force(logp.astype(np.float64))
    lb, ids, val, n = R.case_inputs(logp, V)                                            # K = V: every id is listed
    for model in small_models(V):
        for alpha, beta, flags in ((0.7, 0.0, 0), (0.4, 0.5, EOS), (1.0, -0.25, 0)):
            ref = LR.beam_search(lb, ids, val, n, 64, model, alpha, beta, flags)
            assert len(ref.beam) == len(brute) <= 64
            want = sorted(((ll + model.score(y, alpha, beta, flags)[0], y) for y, ll in brute.items()), key=lambda x: -x[0])
            assert [h[0] for h in ref.beam] == [y for _, y in want]
            for h, (sc, y) in zip(ref.beam, want):
                assert abs(h[1] - sc) < 1e-9 and abs(h[3] - brute[y]) < 1e-9
                assert h[4] == model.score(y, alpha, beta, flags)[0] and h[1] == h[3] + h[4]


# ---- builder and scorer against the plain-text step --------------------------------------------------------------------------------
def random_model(seed, order, V=9, n_per=40, **kw):
    """A pruned model: random n-grams of every order, so prefix contexts are missing; some contexts listed without a back-off."""
    rng = np.random.default_rng(seed)
    grams = {(c,): (np.float32(rng.uniform(-4, -0.3)), np.float32(rng.uniform(-1, 0)) if c % 3 else None) for c in range(1, V) if c != 5}
    for k in range(2, order + 1):
        for x in range(n_per):
            w = tuple(int(c) for c in rng.integers(1, V, k))
            if 5 in w:
                continue
            grams[w] = (np.float32(rng.uniform(-3, -0.1)), np.float32(rng.uniform(-0.8, 0)) if x % 3 else None)
    return LR.Model(order, grams, V, **kw)


@pytest.mark.parametrize("order", [1, 2, 3, 5, 8])
def test_builder_and_scorer_equal_the_plain_text_step(order):
    for seed, kw in enumerate(({}, dict(bos=1, eos=2), dict(unk=3, eos=2, bos=4), dict(transparent=(2, 7), oov=-3.5))):
        model = random_model(100 * order + seed, order, **kw)
        lm = native(model)
        assert lm.order == order and lm.image_bytes % 16 == 0
        rng = np.random.default_rng(seed)
        for trial in range(6):
            y = [int(c) for c in rng.integers(1, 4 if trial % 2 else model.V + 2, 50)]   # a small alphabet makes long matches frequent
            for alpha, beta, flags in ((1.0, 0.0, 0), (0.37, 0.8, EOS), (0.0, 0.0, EOS)):
                g, _st, gp, _sp = lm.score(y, alpha, beta, flags)
                want, pos = model.score(y, alpha, beta, flags)
                assert bits(gp) == bits(pos) and bits([g]) == bits([want])
        assert lm.score([], 0.5, 0.5)[0] == 0.0
        lm.close()


def test_arc_list_edges():
    """Arc lists of 1 .. 9 and 4097 entries over V = 25 055, probed at every arc, between two arcs, below the first and above
    the last, in a bigram and in a trigram context."""
    model, probes = LR.edge_model()
    lm = native(model)
    assert lm.arcs == sum(len(w) > 1 for w in model.logp) and lm.order == 3
    for y in probes:
        _g, _s, gp, _sp = lm.score(y, 0.9, 0.1)
        assert bits(gp) == bits(model.score(y, 0.9, 0.1)[1]), y
    lm.close()


# ---- ARPA ---------------------------------------------------------------------------------------------------------------------------
TOKENS = ["<blank>", "<s>", "</s>", "<unk>", "a", "b", "c", "<|zh|>", "d", "a"]
ARPA = """preamble text

\\data\\
ngram 1=7
ngram 2=5
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.25 </s>
-2.5\t<unk>  -0.1
-0.75 a\t-0.30103
-1.5   b -0.2
-3 zzz -0.4
-1.0 c

\\2-grams:
-0.5 <s> a -0.25
-0.6\ta\tb
-0.7 b </s>
-0.8 zzz a -0.1
-0.9 c a -0.2

\\3-grams:
-0.1 <s> a b
-0.2 a zzz b

\\end\\
"""


def test_arpa_reader(tmp_path):
    p = tmp_path / "lm.arpa"
    p.write_text(ARPA)
    order, grams, dropped, bos, eos, unk, transparent = LR.read_arpa(p, TOKENS)
    assert (order, dropped, bos, eos, unk, transparent) == (3, 3, 1, 2, 3, [7])
    assert grams[(1,)][0] == np.float32(-99 * LR.LN10) and grams[(2,)][1] is None
    model = LR.Model(order, grams, len(TOKENS), bos, eos, unk, -12.0, transparent)
    lm = LanguageModel.from_arpa(p, TOKENS, oov=-12.0)
    assert lm.dropped == 3 and lm.order == 3
    rng = np.random.default_rng(3)
    for _ in range(20):
        y = [int(c) for c in rng.integers(1, len(TOKENS), 12)]
        for flags in (0, EOS):
            g, _s, gp, _sp = lm.score(y, 0.6, 0.2, flags)
            want, pos = model.score(y, 0.6, 0.2, flags)
            assert bits(gp) == bits(pos) and bits([g]) == bits([want])
    lm.close()
    for bad, where in ((ARPA.replace("ngram 2=5", "ngram 2=6"), ":24:"), (ARPA.replace("\\end\\\n", ""), "truncated"),
                       (ARPA.replace("-0.6\ta\tb", "-0.6\ta"), ":19:"), (ARPA.replace("-1.0 c", "x c"), ":15:"),
                       (ARPA.replace("-0.7 b </s>\n", "-0.7 b </s>\n-0.6 a b\n").replace("ngram 2=5", "ngram 2=6"), "duplicate")):
        q = tmp_path / "bad.arpa"
        q.write_text(bad)
        with pytest.raises(N.PfError) as e:
            LanguageModel.from_arpa(q, TOKENS)
        assert e.value.code == N.PF_ERR_INVALID_ARG and where in e.value.message, e.value.message
        if where != "duplicate":                   # (a dict cannot hold one: the reference leaves that refusal to the builder)
            with pytest.raises(ValueError):
                LR.read_arpa(q, TOKENS)
    with pytest.raises(N.PfError) as e:
        LanguageModel.from_arpa(tmp_path / "none.arpa", TOKENS)
    assert e.value.code == N.PF_ERR_IO


# ---- the host twin against the definition -------------------------------------------------------------------------------------------
def _hyps(res):
    return [(tuple(res.ids[0, i, : int(res.len[0, i])].tolist()), float(res.score[0, i]), int(res.matched[0, i]),
             float(res.loglik_sum[0, i]), float(res.lm_sum[0, i])) for i in range(int(res.n_hyp[0]))]


def same(got, want, T):
    """The comparison rule of the reference: lists identical and in order, lm_sum and matched bit-equal, score and loglik_sum
    within the bound."""
    assert [h[0] for h in got] == [h[0] for h in want]
    for g, w in zip(got, want):
        assert g[2] == w[2] and bits([g[4]]) == bits([w[4]])
        tol = LR.tol(T, w[1], w[3], w[4])
        assert abs(g[1] - w[1]) <= tol and abs(g[3] - w[3]) <= tol, (g, w, tol)


def check_gap(case, ref):
    """The condition on a committed input: every decision over fused keys and final scores is 1000 bounds wide; exact ties only
    on the mirrored inputs."""
    if not ref.beam:
        return
    worst = max(max(abs(h[1]), abs(h[3]), abs(h[4])) for h in ref.beam)
    gap = ref.gap_pos if case[6] == "mirror" else ref.gap
    assert gap >= 1000 * LR.tol(case[2], worst), (case, gap, LR.tol(case[2], worst))


_models = {}


def case_native(case):
    if case not in _models:
        _models[case] = native(LR.case_lm(case))
    return _models[case]


@pytest.mark.parametrize("flags", [0, EOS])
@pytest.mark.parametrize("with_hot", [False, True])
@pytest.mark.parametrize("alpha,beta", LR.WEIGHTS)
@pytest.mark.parametrize("case", R.CPU_CASES, ids=[c[0] for c in R.CPU_CASES])
def test_host_twin_equals_definition(case, alpha, beta, with_hot, flags):
    lb, ids, val, n = R.case_arrays(case)
    T, W = case[2], case[5]
    ref = LR.case_reference(case, alpha, beta, flags, with_hot)
    check_gap(case, ref)
    hot = BR.case_hotwords(case) if with_hot else ()
    got = host_ctc_beam_lm(lb, ids, val, n, W, case_native(case), alpha, beta, flags, hot, BR.RECIPE_BOOST if with_hot else 0.0)
    assert got.n_hyp[0] == len(ref.beam)
    same(_hyps(got), ref.beam, T)
    for h in _hyps(got):                           # the identity, bit for bit
        assert h[1] == (h[3] + np.float64(np.float32(BR.RECIPE_BOOST if with_hot else 0.0)) * h[2]) + h[4]


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_gpu_inputs_meet_the_gap_condition(case):
    for alpha, beta in LR.WEIGHTS:
        for with_hot in (False, True):
            check_gap(case, LR.case_reference(case, alpha, beta, EOS if with_hot else 0, with_hot))


@pytest.mark.parametrize("case", R.CPU_CASES, ids=[c[0] for c in R.CPU_CASES])
def test_zero_weights_are_the_unfused_twin(case):
    lb, ids, val, n = R.case_arrays(case)
    W = case[5]
    lm = case_native(case)
    plain = host_ctc_beam(lb, ids, val, n, W)
    got = host_ctc_beam_lm(lb, ids, val, n, W, lm, 0.0, 0.0, EOS)
    assert (got.ids == plain.ids).all() and (got.len == plain.len).all() and bits(got.score) == bits(plain.score)
    assert bits(got.loglik_sum) == bits(plain.score) and not got.lm_sum.any() and not got.matched.any()
    hot = BR.case_hotwords(case)
    biased = host_ctc_beam_hot(lb, ids, val, n, W, hot, 2.0)
    got = host_ctc_beam_lm(lb, ids, val, n, W, lm, 0.0, 0.0, 0, hot, 2.0)
    assert (got.ids == biased.ids).all() and bits(got.score) == bits(biased.score) and (got.matched == biased.matched).all()
    assert bits(got.loglik_sum) == bits(biased.loglik_sum)


def test_worked_by_hand():
    """T = 2, V = 3, W = 2.  Frames (log-probs): blank ln .5 / ln .5, id 1 ln .3 / ln .2, id 2 ln .2 / ln .3.  Bigram LM, natural
    logs: p(1) = -1, p(2) = -2, bo(1) = -0.5, p(1 2) = -0.25; alpha = 1, beta = 0.5.
    g(1) = -1 + .5 = -.5;  g(2) = -2 + .5 = -1.5;  g(1 2) = -.5 - .25 + .5 = -.25;  g(1 1) = -.5 + (-.5 - 1) + .5 = -1.5.
    Frame 0: () .5, (1) .3, (2) .2; keys ln .5 = -.693, ln .3 - .5 = -1.704, ln .2 - 1.5 = -3.109: () and (1) stay.
    Frame 1: () .25; (1) .15 + .06 + .1 = .31 (stay by blank, by repeat, extension of ()); (2) from () .15; (1 2) .3 * .3 = .09;
    (1 1) needs a blank between: only from pb of (1) = 0 at frame 0 -> dropped.  Keys: () -1.386; (1) ln .31 - .5 = -1.671;
    (2) ln .15 - 1.5 = -3.397; (1 2) ln .09 - .25 = -2.658: the beam is (), (1).  With W = 3 the prefix (2) survives frame 0 and
    reaches .1 + .06 + .15 = .31 — key -2.671, still behind (1 2) at -2.658, which the unfused search (.31 against .09) drops."""
    lp = np.log(np.array([[0.5, 0.3, 0.2], [0.5, 0.2, 0.3]])).astype(np.float32)
    lb, ids, val, n = R.case_inputs(lp, 3)
    grams = {(1,): (-1.0, -0.5), (2,): (-2.0, None), (1, 2): (-0.25, None)}
    model = LR.Model(2, grams, 3)
    assert model.score((1, 2), 1.0, 0.5)[1] == [-0.5, -0.25] and model.score((1, 1), 1.0, 0.5)[0] == -1.5
    lm = native(model)
    for W, want in ((2, [(), (1,)]), (3, [(), (1,), (1, 2)])):
        ref = LR.beam_search(lb, ids, val, n, W, model, 1.0, 0.5)
        got = host_ctc_beam_lm(lb, ids, val, n, W, lm, 1.0, 0.5)
        assert [h[0] for h in ref.beam] == want == [h[0] for h in _hyps(got)]
    assert abs(ref.beam[1][1] - (math.log(0.31) - 0.5)) < 1e-6 and abs(ref.beam[2][1] - (math.log(0.09) - 0.25)) < 1e-6
    assert ref.beam[2][4] == -0.25 and _hyps(got)[2][4] == -0.25
    assert {h[0] for h in R.beam_search(lb, ids, val, n, 3).beam} == {(1,), (), (2,)}     # the unfused search keeps (2)
    lm.close()


# ---- refusals, limits, symbols ------------------------------------------------------------------------------------------------------
def test_refusals_and_limits():
    uni = {(1,): (-1.0, -0.5), (2,): (-2.0, None)}

    def refused(code, *a, **kw):
        with pytest.raises(N.PfError) as e:
            LanguageModel(*a, **kw)
        assert e.value.code == code, e.value.message
    refused(N.PF_ERR_INVALID_ARG, 0, {}, 3)
    refused(N.PF_ERR_INVALID_ARG, N.PF_LM_ORDER_MAX + 1, uni, 3)
    refused(N.PF_ERR_INVALID_ARG, 1, {(3,): (-1.0, None)}, 3)                          # an id outside [1, V)
    refused(N.PF_ERR_INVALID_ARG, 1, {(0,): (-1.0, None)}, 3)
    refused(N.PF_ERR_INVALID_ARG, 1, {(1,): (-np.inf, None)}, 3)
    refused(N.PF_ERR_INVALID_ARG, 2, {(1,): (-1.0, np.inf)}, 3)
    refused(N.PF_ERR_INVALID_ARG, 1, uni, 3, oov=np.nan)
    refused(N.PF_ERR_INVALID_ARG, 1, uni, 3, bos=3)
    refused(N.PF_ERR_INVALID_ARG, 1, {(1,): (-1.0, None)}, 3, unk=2)                   # an unk that is no listed unigram
    refused(N.PF_ERR_INVALID_ARG, 1, uni, 3, transparent=(3,))
    for order, ids in ((1, [1, 2, 1]), (2, [1, 2, 1, 2, 1, 2])):                       # a duplicate n-gram, at both kinds of order
        counts = [3] if order == 1 else [2, 2]
        with pytest.raises(N.PfError) as e:
            LanguageModel.from_arrays(order, counts, ids, [-1.0] * sum(counts), [np.nan] * sum(counts), 3)
        assert e.value.code == N.PF_ERR_INVALID_ARG and "duplicate" in e.value.message
    with pytest.raises(N.PfError) as e:                                                # more n-grams than any image could hold
        LanguageModel.from_arrays(1, [N.PF_LM_IMAGE_BYTES_MAX], [1], [-1.0], [np.nan], 3)
    assert e.value.code == N.PF_ERR_CAPACITY
    lm = LanguageModel(1, uni, 3)
    lb, ids, val, n = R.case_arrays(R.CPU_CASES[0])
    for a, b, f in ((-1.0, 0.0, 0), (np.inf, 0.0, 0), (np.nan, 0.0, 0), (1.0, np.inf, 0), (1.0, 0.0, 2)):
        with pytest.raises(N.PfError) as e:
            lm.score([1], a, b, f)
        assert e.value.code == N.PF_ERR_INVALID_ARG
        with pytest.raises(N.PfError) as e:
            host_ctc_beam_lm(lb, ids, val, n, 3, lm, a, b, f)
        assert e.value.code == N.PF_ERR_INVALID_ARG
    with pytest.raises(N.PfError) as e:
        host_ctc_beam_lm(lb, ids, val, n, 3, lm, 1.0, 0.0, cap=1)
    assert e.value.code == N.PF_ERR_CAPACITY
    assert lm.order == 1 and lm.states == 1 and lm.arcs == 0
    lm.close()
    lm.close()                                                                         # a second close is harmless


def test_exported_symbols():
    lib = N.load()
    for name in ("pf_host_lm_build", "pf_host_lm_from_arpa", "pf_host_lm_info", "pf_host_lm_score", "pf_lm_free", "pf_host_ctc_beam_lm",
                 "pf_op_ctc_beam_lm", "pf_op_lm_score"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    assert (N.PF_LM_ORDER_MAX, N.PF_LM_IMAGE_BYTES_MAX, N.PF_LM_EOS) == (8, 1 << 30, 1)
    lib.pf_lm_free(None)


def test_cli_arguments():
    from aliparaformerasr_amd import examples as ex
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16", "-lm", "lm.arpa", "-lmweight", "0.7", "-lmbonus", "-0.5", "-lmeos"])
    assert (cfg["lm"], cfg["lmweight"], cfg["lmbonus"], cfg["lmeos"]) == ("lm.arpa", 0.7, -0.5, True)
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16", "-lm", "lm.arpa", "-hotboost", "2"])
    assert cfg["lm"] == "lm.arpa" and "lmweight" not in cfg and "lmeos" not in cfg and cfg["hotboost"] == 2.0
    assert "lm" not in ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16"])
    base = ["-type", "offline", "-nbest", "2", "-beam", "4"]
    for argv in (["-type", "offline", "-lm", "x.arpa"], ["-type", "offline", "-nbest", "2", "-lm", "x.arpa"], base + ["-lm"],
                 base + ["-lm", "-lmeos"], base + ["-lmweight", "0.5"], base + ["-lmeos"], base + ["-lm", "x", "-lmweight", "-1"],
                 base + ["-lm", "x", "-lmweight", "nan"], base + ["-lm", "x", "-lmbonus", "inf"], base + ["-lm", "x", "-lmbonus"]):
        with pytest.raises(ValueError):
            ex.parse_args(argv)


def test_the_large_model_meets_the_gap_condition():
    """The formula model of tests/test_gpu_ctcbeam_lm.py's 32 MB case, on the input it is run with."""
    case = [c for c in R.GPU_CASES if c[0] == "t65"][0]
    lb, ids, val, n = R.case_arrays(case)
    model = LR.big_model()
    for alpha, beta, flags in ((0.5, 0.0, 0), (0.3, 1.0, EOS)):
        check_gap(case, LR.beam_search(lb, ids, val, n, case[5], model, alpha, beta, flags))


def test_arpa_round_trip(tmp_path):
    """write_arpa then the library's reader: the model the text holds, scored alike by reference and library."""
    m = random_model(11, 3, bos=1, eos=2)
    toks = ["<blank>", "<s>", "</s>"] + ["w%d" % c for c in range(3, m.V)]
    LR.write_arpa(tmp_path / "m.arpa", 3, m.ngrams, toks)
    order, grams, dropped, bos, eos, unk, tr = LR.read_arpa(tmp_path / "m.arpa", toks)
    assert (order, dropped, bos, eos, unk, tr) == (3, 0, 1, 2, -1, []) and set(grams) == set(m.ngrams)
    back = LR.Model(order, grams, len(toks), bos, eos, unk, -10.0, tr)
    lm = LanguageModel.from_arpa(tmp_path / "m.arpa", toks)
    y = [int(c) for c in np.random.default_rng(1).integers(1, m.V, 60)]
    assert bits(lm.score(y, 0.5, 0.1, EOS)[2]) == bits(back.score(y, 0.5, 0.1, EOS)[1])
    lm.close()


# ---- the host code once more, under sanitizers ----------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_host_code_under_sanitizers(tmp_path):
    """csrc/lm.cpp (builder, ARPA reader, scorer) and the fused twin of csrc/hostutil.cpp in a stand-alone program
    (tests/native/ctcbeam_lm_sanitize.cpp) built with AddressSanitizer + UBSan on the host code: no report, and the library's
    own answers bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "ctcbeam_lm_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "ctcbeam_lm_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    u32 = lambda a: " ".join(map(str, np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).tolist()))    # noqa: E731
    ints = lambda a: " ".join(map(str, a))                                                                         # noqa: E731

    def model_cmd(m, order=None, extra=()):
        order = m.order if order is None else order
        by_k = [[w for w in m.ngrams if len(w) == k] for k in range(1, order + 1)]
        out = ["M %d %d %d %d %d %s %d %s" % (order, m.V, m.bos, m.eos, m.unk, u32([m.oov]), len(m.transparent), ints(sorted(m.transparent))),
               ints(len(x) + (len(extra) if k == 0 else 0) for k, x in enumerate(by_k))]
        for k, x in enumerate(by_k):
            for w in list(x) + (list(extra) if k == 0 else []):
                v = m.ngrams[w]
                out.append("%s %s %s" % (ints(w), u32([v[0]]), u32([np.nan if v[1] is None else v[1]])))
        return " ".join(out)

    def beam_cmd(arr, W, cap, hot, boost, alpha, beta, flags):
        lb, ids, val, n = arr
        T, K = ids.shape
        return "B %d %d %d %d %d %d %s %s %s %d %s %s %s %s %s %s" % (
            T, K, W, W, cap, len(hot), u32([boost]), u32([alpha]), u32([beta]), flags, u32(lb), ints(ids.ravel().tolist()), u32(val),
            ints(n.tolist()), ints(len(w) for w in hot), ints(c for w in hot for c in w))
    cmds, want = [], []
    for case in R.CPU_CASES[::3]:
        m = LR.case_lm(case)
        lm = case_native(case)
        cmds.append(model_cmd(m))
        want.append("M %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes))
        arr = R.case_arrays(case)
        for hot, boost, flags in (((), 0.0, 0), (BR.case_hotwords(case), 2.0, EOS)):
            cmds.append(beam_cmd(arr, case[5], max(case[2], 1), hot, boost, 0.3, 1.0, flags))
            res = host_ctc_beam_lm(*arr, case[5], lm, 0.3, 1.0, flags, hot, boost)
            txt = "B %d" % int(res.n_hyp[0])
            for i in range(int(res.n_hyp[0])):
                L = int(res.len[0, i])
                txt += " %d %s %d %d %d %d" % (L, ints(res.ids[0, i, :L].tolist()), int(res.matched[0, i]), bits(res.score[0, i: i + 1])[0],
                                               bits(res.loglik_sum[0, i: i + 1])[0], bits(res.lm_sum[0, i: i + 1])[0])
            want.append(" ".join(txt.split()))
    for order in (1, 3, 8):                                                            # pruned models, the scorer at every position
        m = random_model(7 + order, order, bos=1, eos=2, transparent=(7,))
        lm = native(m)
        cmds.append(model_cmd(m))
        want.append("M %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes))
        y = [int(c) for c in np.random.default_rng(order).integers(1, m.V + 3, 40)]
        cmds.append("S %s %s %d %d %s" % (u32([0.37]), u32([0.8]), EOS, len(y), ints(y)))
        g, st, gp, sp = lm.score(y, 0.37, 0.8, EOS)
        want.append(" ".join(("S %d %d " % (bits([g])[0], st) + " ".join("%d %d" % (a, b) for a, b in zip(bits(gp), sp.tolist()))).split()))
        lm.close()
    edge, probes = LR.edge_model()                                                     # the 4097-arc lists, first / last / missing
    lm = native(edge)
    cmds.append(model_cmd(edge))
    want.append("M %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes))
    for y in probes[-6:] + probes[-4103:-4100]:
        cmds.append("S %s %s 0 %d %s" % (u32([1.0]), u32([0.0]), len(y), ints(y)))
        g, st, gp, sp = lm.score(y, 1.0, 0.0)
        want.append(" ".join(("S %d %d " % (bits([g])[0], st) + " ".join("%d %d" % (a, b) for a, b in zip(bits(gp), sp.tolist()))).split()))
    lm.close()
    arpa, toks = tmp_path / "lm.arpa", tmp_path / "tokens.txt"
    arpa.write_text(ARPA)
    toks.write_text("\n".join(TOKENS) + "\n")
    lm = LanguageModel.from_arpa(arpa, TOKENS, oov=-12.0)
    cmds.append("A %s %s %s" % (arpa, toks, u32([-12.0])))
    want.append("A %d %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes, lm.dropped))
    lm.close()
    bad = tmp_path / "bad.arpa"
    bad.write_text(ARPA.replace("\\end\\\n", ""))
    cmds.append("A %s %s %s" % (bad, toks, u32([-12.0])))
    want.append("error %d" % N.PF_ERR_INVALID_ARG)
    m = random_model(3, 2)
    cmds.append(model_cmd(m, extra=[(1,)]))                                            # a duplicate unigram
    want.append("error %d" % N.PF_ERR_INVALID_ARG)
    cmds.append(model_cmd(m).replace("M 2 9", "M 2 4", 1))                             # ids outside [1, V)
    want.append("error %d" % N.PF_ERR_INVALID_ARG)
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(cmds) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % len(cmds)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, cmds[i][:60], g[:200], w[:200])
