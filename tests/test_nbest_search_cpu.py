"""CPU: the n-best search over paraformer's top-k lists with hot-word and LM shallow fusion — the definition
(tests/nbest_search_ref.py) against brute-force enumeration, the host twin (pf_host_nbest_search) against the definition bit for
bit over that table and over pruned searches, the twin against pf_host_nbest where nothing is fused, the score identity, one case
worked by hand, the inputs that have no hypothesis, refusals, symbols, the CLI, and the twin once more in a stand-alone program
under ASan + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nbest_search_ref as S
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import LanguageModel, host_nbest, host_nbest_search

EOS = S.PF_LM_EOS


def native(model):
    """The library's model of a reference Model (None stays None)."""
    if model is None:
        return None
    return LanguageModel(model.order, model.ngrams, model.V, model.bos, model.eos, model.unk, model.oov, sorted(model.transparent))


def keys(hyps):
    return [h.key() for h in hyps]


def table():
    """(L, K, variant, ids, val, n, V, n_free, form) over every shape, input variant, n_free and fusion form."""
    for L, K in S.TABLE_SHAPES:
        for variant in S.TABLE_VARIANTS:
            ids, val, n, V = S.table_lists(L, K, variant)
            for n_free in range(L + 1):
                for form in S.fusion_forms(ids, n, n_free, V):
                    yield L, K, variant, ids, val, n, V, n_free, form


# ---- the definition against brute force: W = K ** n_free prunes nothing ---------------------------------------------------------------
def test_definition_against_brute_force():
    seen_completed = seen_pending = seen_neginf = seen_tie = 0
    for L, K, variant, ids, val, n, V, n_free, (name, model, a, b, fl, hot, boost) in table():
        W = K ** n_free
        assert 1 <= W <= 64
        ref = S.search(ids, val, n, n_free, W, None, model, a, b, fl, hot, boost)
        brute = S.brute_force(ids, val, n, n_free, None, model, a, b, fl, hot, boost)
        assert len(ref) == len(brute) == int(np.prod(n[:n_free])), (L, K, variant, n_free, name)
        assert S.grouped(ref) == S.grouped(brute), (L, K, variant, n_free, name)
        if hot and boost > 0 and n_free >= 2:
            ys = [tuple(int(ids[l, h.ranks[l]]) for l in range(n_free)) for h in ref]
            seen_completed += any(y[-2:] == tuple(hot[0]) for y in ys)         # a word completed at the last free position
            seen_pending += any(S.BR.walk(y, hot)[1] > 0 for y in ys)         # a pending partial match at the end
        seen_neginf += any(h.loglik_sum == -np.inf for h in ref)
        seen_tie += len({S.bits(h.score) for h in ref}) < len(ref)
    assert seen_completed and seen_pending and seen_neginf and seen_tie


# ---- the twin against the definition, bit for bit -----------------------------------------------------------------------------------
def test_twin_against_definition_over_the_table():
    for L, K, variant, ids, val, n, V, n_free, (name, model, a, b, fl, hot, boost) in table():
        lm = native(model)
        for W in sorted({K ** n_free, 1, 2, 4}):
            for Nb in sorted({W, 1}):
                ref = S.search(ids, val, n, n_free, W, Nb, model, a, b, fl, hot, boost)
                got = host_nbest_search(ids, val, n, n_free, W, Nb, lm, a, b, fl, hot, boost)
                assert keys(S.as_hyps(got)) == keys(ref), (L, K, variant, n_free, name, W, Nb)
                # the slots past n_hyp hold the fill values
                k = int(got.n_hyp[0])
                assert (got.ranks[0, k:] == -1).all() and (got.score[0, k:] == -np.inf).all() and (got.loglik_sum[0, k:] == -np.inf).all()
                assert (got.lm_sum[0, k:] == 0).all() and (got.matched[0, k:] == 0).all()
        if lm is not None:
            lm.close()


PRUNE_V = 14


def prune_case(L, K, seed=0):
    rng = np.random.default_rng(77 + 100 * L + K + seed)
    ids, val, n = S.log_softmax_lists(rng, L, K, PRUNE_V)
    hot = [(int(ids[0, 0]), int(ids[min(1, L - 1), min(1, K - 1)])), (int(ids[L - 1, 0]), 3, 5), (int(ids[L // 2, K - 1]),), (2, 4, 6, 8)]
    hot = [tuple(max(c, 1) for c in w) for w in hot]                    # (id 0 may be listed, but is no hot-word id)
    return ids, val, n, hot


@pytest.mark.parametrize("L", [1, 2, 40])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_twin_against_definition_when_the_beam_prunes(L, K):
    ids, val, n, hot = prune_case(L, K)
    model = S.small_model(PRUNE_V, 3, bos=1, eos=2, missing=(PRUNE_V - 1,))
    lm = native(model)
    for W in (1, 2, 4, 16, 64):
        for form, (m, l, a, b, fl, h, s) in enumerate(((None, None, 0, 0, 0, (), 0.0), (None, None, 0, 0, 0, hot, 2.0),
                                                      (model, lm, 0.5, 0.25, 0, (), 0.0), (model, lm, 0.3, 1.0, EOS, hot, 1.5))):
            if L == 40 and W in (2, 16) and form in (1, 2):
                continue                                                # (the long input: every form at W = 1, 4, 64, both fused at all)
            for tn in sorted({L, max(L - 3, 0)}):
                ref = S.search(ids, val, n, tn, W, None, m, a, b, fl, h, s)
                got = host_nbest_search(ids, val, n, tn, W, None, l, a, b, fl, h, s)
                assert keys(S.as_hyps(got)) == keys(ref), (L, K, W, form, tn)
    lm.close()


# ---- nothing fused: pf_host_nbest's list ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,K,Nb,W,seed", [(3, 4, 10, 10, 1), (12, 4, 10, 16, 2), (12, 8, 10, 64, 3), (30, 4, 16, 16, 4), (6, 2, 10, 33, 5)])
def test_twin_against_host_nbest(L, K, Nb, W, seed):
    ids, val, n = S.log_softmax_lists(np.random.default_rng(seed), L, K, 40)
    lm = native(S.small_model(40, 2))
    for n_free in (L, L - 2):
        ranks, sc = host_nbest(val, n, n_free, Nb + 1)                  # one more: the first hypothesis left out must not tie either
        total = int(np.prod(n[:n_free].astype(np.int64)))
        assert len(sc) == min(Nb + 1, total)
        assert len(set(np.asarray(sc, np.float64).view(np.int64).tolist())) == len(sc), "choose another seed: scores tie"
        k = min(Nb, total)
        for model in (None, lm):                                        # no model, and a model with alpha = beta = 0
            got = host_nbest_search(ids, val, n, n_free, W, Nb, model, 0.0, 0.0)
            assert int(got.n_hyp[0]) == k
            assert got.ranks[0, :k].tolist() == np.asarray(ranks)[:k].tolist()
            assert got.score[0, :k].view(np.int64).tolist() == np.asarray(sc[:k], np.float64).view(np.int64).tolist()
            assert got.loglik_sum[0].view(np.int64).tolist() == got.score[0].view(np.int64).tolist()
            assert (got.lm_sum[0] == 0).all() and not np.signbit(got.lm_sum[0]).any() and (got.matched[0] == 0).all()
    lm.close()


# ---- the identity, and one case by hand ---------------------------------------------------------------------------------------------
def test_score_identity_bit_for_bit():
    ids, val, n, hot = prune_case(40, 8)
    model = S.small_model(PRUNE_V, 3, bos=1, eos=2)
    lm = native(model)
    for boost, a, b, fl in ((1.7, 0.37, 0.8, EOS), (0.0, 0.5, 0.0, 0), (2.5, 0.0, 0.0, 0)):
        got = host_nbest_search(ids, val, n, 37, 64, None, lm, a, b, fl, hot, boost)
        s = float(np.float32(boost))
        assert int(got.n_hyp[0]) == 64
        for i in range(64):
            want = (got.loglik_sum[0, i] + s * int(got.matched[0, i])) + got.lm_sum[0, i]
            assert S.bits(want) == S.bits(got.score[0, i])
        assert (got.matched[0] > 0).any() == (boost > 0)
    lm.close()


def test_one_case_by_hand():
    """L = 2, K = 2, W = N = 2; ids [[3, 5], [4, 6]], val [[-0.5, -1.0], [-0.25, -2.0]]; hot word (5, 6) with boost 2; a unigram
    model logp(3) = logp(4) = -1, logp(5) = logp(6) = -0.5, alpha = 0.5, beta = 0.25.  Every number is a dyadic fraction: exact.
      position 0   index 0 (c = 3): a = -0.5,  g = 0.5 * -1 + 0.25 = -0.25, m + d = 0      key = -0.75
                   index 1 (c = 5): a = -1.0,  g = 0.5 * -0.5 + 0.25 = 0,  m + d = 0 + 1   key = (-1 + 2) + 0 = 1
                   beam: [ranks (1), ranks (0)]
      position 1   index 0 = (1) + 4: a = -1.25, g = 0 - 0.5 + 0.25 = -0.25, the match breaks     key = -1.5
                   index 1 = (1) + 6: a = -3.0,  g = 0 - 0.25 + 0.25 = 0,  m = 2 (completed)      key = (-3 + 4) + 0 = 1
                   index 2 = (0) + 4: a = -0.75, g = -0.25 - 0.5 + 0.25 = -0.5                    key = -1.25
                   index 3 = (0) + 6: a = -2.5,  g = -0.25 - 0.25 + 0.25 = -0.25                  key = -2.75
                   beam: [(1, 1), (0, 0)] — the acoustic second best (1, 0) is pruned, the acoustic best comes second
      finish       (1, 1): score (-3 + 2 * 2) + 0 = 1;  (0, 0): score -0.75 + -0.5 = -1.25"""
    ids = np.array([[3, 5], [4, 6]], np.int64)
    val = np.array([[-0.5, -1.0], [-0.25, -2.0]], np.float32)
    n = np.array([2, 2], np.int32)
    grams = {(3,): (-1.0, None), (4,): (-1.0, None), (5,): (-0.5, None), (6,): (-0.5, None)}
    model = S.LR.Model(1, grams, 7)
    lm = native(model)
    want = [((1, 1), 1.0, -3.0, 0.0, 2), ((0, 0), -1.25, -0.75, -0.5, 0)]
    ref = S.search(ids, val, n, 2, 2, None, model, 0.5, 0.25, 0, [(5, 6)], 2.0)
    got = host_nbest_search(ids, val, n, 2, 2, None, lm, 0.5, 0.25, 0, [(5, 6)], 2.0)
    assert [(h.ranks, h.score, h.loglik_sum, h.lm_sum, h.matched) for h in ref] == want
    assert got.hyps(0) == want
    # without the fusion the acoustic order: (0, 0) -0.75, (1, 0) -1.25
    assert host_nbest_search(ids, val, n, 2, 2).hyps(0) == [((0, 0), -0.75, -0.75, 0.0, 0), ((1, 0), -1.25, -1.25, 0.0, 0)]
    lm.close()


# ---- no hypotheses, refusals, symbols, the CLI ---------------------------------------------------------------------------------------
def test_inputs_without_a_hypothesis_fill_every_slot():
    ids, val, n, _ = prune_case(5, 4)
    bad = []
    z = n.copy(); z[3] = 0                                              # noqa: E702
    bad.append((ids, val, z, 2))                                        # an empty position, in the tail
    for x in (np.nan, np.inf):
        v = val.copy(); v[4, 3] = x                                     # noqa: E702
        bad.append((ids, v, n, 2))                                      # a listed NaN / +inf, in the tail and not at rank 0
    bad.append((ids[:0], val[:0], n[:0], 0))                            # L = 0
    for i, v, nn, tn in bad:
        assert S.search(i, v, nn, tn, 4) == []
        got = host_nbest_search(i, v, nn, tn, 4, 3)
        assert int(got.n_hyp[0]) == 0 and (got.ranks == -1).all() and (got.score == -np.inf).all() and (got.loglik_sum == -np.inf).all()
        assert (got.lm_sum == 0).all() and (got.matched == 0).all()
    v = val.copy(); v[4, 3] = np.nan; z = n.copy(); z[4] = 3            # noqa: E702
    assert int(host_nbest_search(ids, v, z, 5, 4).n_hyp[0]) == 4        # a NaN past n[l] is not listed: never read
    assert keys(S.as_hyps(host_nbest_search(ids, v, z, 99, 4))) == keys(S.search(ids, v, z, 5, 4))    # token_num > L; < 0 below
    assert keys(S.as_hyps(host_nbest_search(ids, v, z, -3, 4))) == keys(S.search(ids, v, z, 0, 4))


def test_refusals():
    ids, val, n, hot = prune_case(3, 4)
    lm = native(S.small_model(PRUNE_V, 2))

    def refused(*a, **k):
        with pytest.raises(N.PfError) as e:
            host_nbest_search(*a, **k)
        assert e.value.code == N.PF_ERR_INVALID_ARG
    refused(ids, val, n, 3, 65)
    refused(ids, val, n, 3, 4, 5)
    refused(ids, val, n, 3, 4, 0)
    refused(ids, val, n, 3, 0, 0)
    refused(np.zeros((3, 9), np.int64), np.zeros((3, 9), np.float32), n, 3, 4)
    z = n.copy(); z[1] = 5                                              # noqa: E702
    refused(ids, val, z, 3, 4)
    z[1] = -1
    refused(ids, val, z, 3, 4)
    for boost in (-1.0, np.inf, np.nan):
        refused(ids, val, n, 3, 4, hotwords=hot, boost=boost)
    refused(ids, val, n, 3, 4, hotwords=[(0, 3)], boost=1.0)           # a hot-word id outside [1, 2^24)
    for a, b, f in ((-1.0, 0.0, 0), (np.inf, 0.0, 0), (np.nan, 0.0, 0), (1.0, np.inf, 0), (1.0, 0.0, 2)):
        refused(ids, val, n, 3, 4, lm=lm, alpha=a, beta=b, flags=f)
    host_nbest_search(ids, val, n, 3, 4, alpha=-1.0)                    # without a model the weights are not read
    lm.close()


def test_exported_symbols():
    lib = N.load()
    for name in ("pf_engine_set_nbest_search", "pf_engine_set_nbest_lm", "pf_engine_set_nbest_hotwords", "pf_fetch_nbest_search",
                 "pf_host_nbest_search", "pf_op_nbest_search", "pf_recognizer_set_nbest_search", "pf_recognizer_set_nbest_lm",
                 "pf_recognizer_set_nbest_hotword_boost"):
        assert hasattr(lib, name) and name in N.SIGNATURES
    from aliparaformerasr_amd.offline_recognizer import OfflineRecognizer
    for name in ("SetNBestSearch", "SetNBestLm", "SetNBestHotwordBoost"):
        assert hasattr(OfflineRecognizer, name)


def test_cli_arguments():
    from aliparaformerasr_amd import examples as ex
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-search", "16", "-lm", "lm.arpa", "-lmweight", "0.7", "-lmbonus", "-0.5", "-lmeos",
                         "-hotboost", "2"])
    assert (cfg["search"], cfg["lm"], cfg["lmweight"], cfg["lmbonus"], cfg["lmeos"], cfg["hotboost"]) == (16, "lm.arpa", 0.7, -0.5, True, 2.0)
    assert ex.parse_args(["-type", "offline", "-nbest", "4", "-search", "64"])["search"] == 64
    assert "search" not in ex.parse_args(["-type", "offline", "-nbest", "4"])
    base = ["-type", "offline", "-nbest", "2"]
    for argv in (["-type", "offline", "-search", "4"], base + ["-search"], base + ["-search", "0"], base + ["-search", "65"],
                 base + ["-search", "x"], base + ["-search", "4", "-beam", "4"], ["-type", "online", "-nbest", "2", "-search", "4"],
                 base + ["-search", "4", "-lmweight", "0.5"], base + ["-search", "4", "-lm", "x", "-lmweight", "-1"],
                 base + ["-lm", "x.arpa"], base + ["-hotboost", "2"]):            # the last two: without -search, as before
        with pytest.raises(ValueError):
            ex.parse_args(argv)


# ---- the twin once more, under sanitizers -------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_twin_under_sanitizers(tmp_path):
    """csrc/hostutil.cpp's search (with csrc/lm.cpp's builder) in a stand-alone program (tests/native/nbest_search_sanitize.cpp)
    built with AddressSanitizer + UBSan on the host code, run over the case table: no report, and the library's own answers bit
    for bit, fills included."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "nbest_search_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "nbest_search_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), os.path.join(cs, "lm.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    u32 = lambda a: " ".join(map(str, np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).tolist()))    # noqa: E731
    ints = lambda a: " ".join(map(str, a))                                                                         # noqa: E731
    b64 = lambda a: np.asarray(a, np.float64).view(np.uint64).tolist()                                             # noqa: E731

    def model_cmd(m):
        by_k = [sorted(w for w in m.ngrams if len(w) == k) for k in range(1, m.order + 1)]
        out = ["M %d %d %d %d %d %s %d %s" % (m.order, m.V, m.bos, m.eos, m.unk, u32([m.oov]), len(m.transparent), ints(sorted(m.transparent))),
               ints(len(x) for x in by_k)]
        for x in by_k:
            for w in x:
                v = m.ngrams[w]
                out.append("%s %s %s" % (ints(w), u32([v[0]]), u32([np.nan if v[1] is None else v[1]])))
        return " ".join(out)

    def search_cmd(ids, val, n, tn, W, Nb, hot, boost, a, b_, fl, use_lm):
        L, K = ids.shape
        return "N %d %d %d %d %d %d %s %s %s %d %d %s %s %s %s %s" % (
            L, K, tn, W, Nb, len(hot), u32([boost]), u32([a]), u32([b_]), fl, use_lm, ints(ids.ravel().tolist()), u32(val), ints(n.tolist()),
            ints(len(w) for w in hot), ints(c for w in hot for c in w))

    def answer(got, Nb, L):
        txt = "N %d" % int(got.n_hyp[0])
        for i in range(Nb):
            txt += " %s %d %d %d %d" % (ints(got.ranks[0, i].tolist()), int(got.matched[0, i]), b64(got.score[0, i: i + 1])[0],
                                        b64(got.loglik_sum[0, i: i + 1])[0], b64(got.lm_sum[0, i: i + 1])[0])
        return " ".join(txt.split())
    cmds, want = [], []
    for L, K, variant, ids, val, n, V, n_free, (name, model, a, b_, fl, hot, boost) in table():
        if (L + n_free) % 2:                                            # every other n_free: half the table
            continue
        lm = native(model)
        if model is not None:
            cmds.append(model_cmd(model))
            want.append("M %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes))
        for W, Nb in ((K ** n_free, K ** n_free), (2, 1)):
            cmds.append(search_cmd(ids, val, n, n_free, W, Nb, hot, boost, a, b_, fl, int(model is not None)))
            want.append(answer(host_nbest_search(ids, val, n, n_free, W, Nb, lm, a, b_, fl, hot, boost), Nb, L))
        if lm is not None:
            lm.close()
    ids, val, n, hot = prune_case(40, 8)                                 # the widest search, and an input without a hypothesis
    model = S.small_model(PRUNE_V, 3, bos=1, eos=2)
    lm = native(model)
    cmds.append(model_cmd(model))
    want.append("M %d %d %d %d" % (lm.order, lm.states, lm.arcs, lm.image_bytes))
    cmds.append(search_cmd(ids, val, n, 38, 64, 64, hot, 1.5, 0.3, 1.0, EOS, 1))
    want.append(answer(host_nbest_search(ids, val, n, 38, 64, 64, lm, 0.3, 1.0, EOS, hot, 1.5), 64, 40))
    z = n.copy(); z[7] = 0                                              # noqa: E702
    cmds.append(search_cmd(ids, val, z, 38, 8, 8, hot, 1.5, 0.3, 1.0, 0, 1))
    want.append(answer(host_nbest_search(ids, val, z, 38, 8, 8, lm, 0.3, 1.0, 0, hot, 1.5), 8, 40))
    cmds.append(search_cmd(ids, val, n, 38, 8, 9, (), 0.0, 0.0, 0.0, 0, 0))      # N > W
    want.append("error %d" % N.PF_ERR_INVALID_ARG)
    lm.close()
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(cmds) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % len(cmds)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, cmds[i][:120], g[:200], w[:200])
