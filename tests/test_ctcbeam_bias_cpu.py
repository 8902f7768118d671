"""CPU: hot-word boosting inside the CTC prefix beam search — the definition (tests/ctcbeam_bias_ref.py) against brute-force
enumeration with the plain-text bonus, the automaton (pf_host_hotword_graph, csrc/hostutil.cpp) against the plain-text walk,
the host twin (pf_host_ctc_beam_hot) against the definition over the committed inputs, the condition those inputs must meet
(a decision gap of 1000 tolerances over biased keys and final scores), no bias = no change, one case worked by hand, refusals,
symbols, the CLI argument, and the twin and the graph builder once more in a stand-alone program under ASan + UBSan."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctcbeam_bias_ref as BR
import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import HotwordGraph, host_ctc_beam, host_ctc_beam_hot

NEW = ("pf_host_hotword_graph", "pf_engine_set_ctc_hotwords", "pf_fetch_ctc_beam_hot", "pf_host_ctc_beam_hot", "pf_op_ctc_beam_hot",
       "pf_recognizer_set_hotword_boost", "pf_stream_alternative_hot")
BOOSTS = (2.0, float(np.float32(0.7)))


def _hyps(res, b=0):
    """[(ids, score, matched, loglik_sum)] of a CtcBeamResult"""
    return [(tuple(res.ids[b, i, : int(res.len[b, i])].tolist()), float(res.score[b, i]), int(res.matched[b, i]),
             float(res.loglik_sum[b, i])) for i in range(int(res.n_hyp[b]))]


def _same(got, want, T):
    """lists, their order and matched identical; score and loglik_sum within (16 T + 4) 2^-53 max(1, |s|)"""
    assert [h[0] for h in got] == [h[0] for h in want]
    assert [h[2] for h in got] == [h[2] for h in want]
    for g, w in zip(got, want):
        assert abs(g[1] - w[1]) <= BR.tol(T, w[1]), (g, w, abs(g[1] - w[1]), BR.tol(T, w[1]))
        assert abs(g[3] - w[3]) <= BR.tol(T, w[3]), (g, w)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,V", [(4, 3), (5, 3), (3, 4), (4, 4)])
def test_definition_equals_brute_force_with_the_plain_text_bonus(T, V):
    """K covers every non-blank id and W = 64 prunes nothing: the search lists every labeling, ordered by the log of its
    summed alignments plus s times the tokens the plain-text walk says it matched."""
    hot = [(1, 2), (2,)] if V == 3 else [(1, 2, 3), (3, 1), (2, 2)]
    s = 1.5
    for seed in range(6):
        x = R.random_rows(seed, T, V).astype(np.float64)
        want = sorted(((y, lp + s * BR.walk(y, hot)[0], BR.walk(y, hot)[0]) for y, lp in R.brute_force(x).items()),
                      key=lambda h: -h[1])
        ids, _, n = R.topk_lists(x.astype(np.float32), V)
        val = np.take_along_axis(x, np.maximum(ids, 0), 1)                      # the float64 rows themselves
        res = BR.beam_search(x[:, 0], ids, val, n, 64, hot, s)
        assert len(res.beam) == len(want) < 64
        assert [h[0] for h in res.beam] == [h[0] for h in want], (seed, T, V)
        for got, w in zip(res.beam, want):
            assert abs(got[1] - w[1]) <= 1e-14 and got[2] == w[2], (got, w)
            assert got[1] == got[3] + s * got[2]                                   # one product, one addition


# ---- 2. the automaton -------------------------------------------------------------------------------------------------------
SETS = {
    "overlapping": [(1, 2, 3), (3, 4, 5), (2, 3, 4)],
    "nested_abcd_bc": [(1, 2, 3, 4), (2, 3)],
    "prefix_ab_abc": [(1, 2), (1, 2, 3)],
    "aa": [(1, 1)],
    "aaa_aa_suffix": [(1, 1, 1), (2, 1, 1)],
    "duplicates": [(1, 2), (1, 2), (2, 1), (1, 2)],
    "empty_entry": [(), (2, 1), ()],
    "single_ids": [(3,), (1, 3, 1)],
    "chain": [(1, 2, 1, 2, 1), (2, 1, 2), (1, 1)],
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_automaton_equals_the_plain_text_walk(name):
    hot = SETS[name]
    V = 6
    g = HotwordGraph(hot, V)
    words = BR.clean_set(hot)
    assert g.A == len({c for w in words for c in w})
    assert g.S == 1 + len({w[:k] for w in words for k in range(1, len(w) + 1)})       # trie nodes, root included
    assert g.depth[0] == 0 and (g.tok_col >= -1).all() and (g.tok_col < g.A).all()
    for seed in range(8):
        rng = np.random.default_rng(1000 + seed)
        hi = 3 if seed % 2 else V                                                  # a small alphabet makes matches frequent
        y = [int(c) for c in rng.integers(1, hi, 60)]
        want = BR.walk_positions(y, hot)
        state, m = 0, 0
        for p, c in enumerate(y):
            state, done = g.step(state, c)
            m += done
            assert 0 <= state < g.S and (done == 0 or state == 0)
            assert (m, int(g.depth[state])) == want[p], (name, seed, p, y[: p + 1])
    assert (g.table >= 0).all()
    # the depth of the next state rides in the top byte of an entry
    nxt = g.table & 0xFFFF
    assert ((g.table >> 24) == g.depth[nxt]).all()


def _graph_rc(hot, V):
    ids = np.asarray([c for w in hot for c in w], np.int32)
    lens = np.asarray([len(w) for w in hot], np.int32)
    s, a = C.c_int32(-1), C.c_int32(-1)
    i32 = C.POINTER(C.c_int32)
    rc = N.load().pf_host_hotword_graph(ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), len(lens), V, s, a, None, None, 0, None, 0)
    return rc, s.value, a.value


def test_automaton_limits():
    # 64-id words over 11 ids until one more would pass 4096 states: accepted, and that one more word is refused
    alphabet = 12
    many, seen = [], set()
    rng = np.random.default_rng(5)
    while 1 + len(seen) <= N.PF_HOTWORD_STATES_MAX:
        w = tuple(int(c) for c in rng.integers(1, alphabet, 64))
        many.append(w)
        seen |= {w[:k] for k in range(1, 65)}
    assert _graph_rc(many, alphabet)[0] == N.PF_ERR_CAPACITY
    kept = {w[:k] for w in many[:-1] for k in range(1, 65)}
    assert _graph_rc(many[:-1], alphabet) == (N.PF_OK, 1 + len(kept), 11) and 1 + len(kept) <= N.PF_HOTWORD_STATES_MAX
    # exactly 4096: the last word leaves an earlier one where the missing states say
    p = 64 - (N.PF_HOTWORD_STATES_MAX - 1 - len(kept))
    free = [c for c in range(1, alphabet) if many[0][:p] + (c,) not in kept]
    last = many[0][:p] + (free[0],) + tuple([free[0]] * (63 - p))
    assert 0 < p < 64 and len(last) == 64
    assert _graph_rc(many[:-1] + [last], alphabet) == (N.PF_OK, N.PF_HOTWORD_STATES_MAX, 11)
    # a hot word of 65 ids; 64 is fine
    assert _graph_rc([tuple([1] * 65)], 4)[0] == N.PF_ERR_CAPACITY
    assert _graph_rc([tuple([1] * 64)], 4) == (N.PF_OK, 65, 1)
    # a table over 16 MB: 33 words of 64 distinct ids each: 2113 states x 2112 columns x 4 bytes
    big = [tuple(range(1 + 64 * k, 1 + 64 * (k + 1))) for k in range(33)]
    assert 2113 * 2112 * 4 > N.PF_HOTWORD_TABLE_BYTES_MAX
    assert _graph_rc(big, 3000)[0] == N.PF_ERR_CAPACITY
    assert _graph_rc(big[:31], 3000) == (N.PF_OK, 1985, 1984)
    # ids outside [1, V)
    for bad in ([(0,)], [(1, -1)], [(1, 2), (4,)]):
        assert _graph_rc(bad, 4)[0] == N.PF_ERR_INVALID_ARG
    assert _graph_rc([(3,)], 4) == (N.PF_OK, 2, 1)
    # nothing left: the root alone
    assert _graph_rc([(), ()], 4) == (N.PF_OK, 1, 0)
    assert _graph_rc([], 4) == (N.PF_OK, 1, 0)
    # buffers too small
    g = HotwordGraph([(1, 2), (2, 3)], 5)
    i32 = C.POINTER(C.c_int32)
    ids, lens = np.asarray([1, 2, 2, 3], np.int32), np.asarray([2, 2], np.int32)
    s, a = C.c_int32(), C.c_int32()
    tab, dep = np.zeros(g.S * g.A, np.int32), np.zeros(g.S, np.int32)
    lib = N.load()
    assert lib.pf_host_hotword_graph(ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), 2, 5, s, a, None, tab.ctypes.data_as(i32),
                                     g.S * g.A - 1, None, 0) == N.PF_ERR_CAPACITY and (s.value, a.value) == (g.S, g.A)
    assert lib.pf_host_hotword_graph(ids.ctypes.data_as(i32), lens.ctypes.data_as(i32), 2, 5, s, a, None, None, 0,
                                     dep.ctypes.data_as(i32), g.S - 1) == N.PF_ERR_CAPACITY


# ---- 3. the host twin ---------------------------------------------------------------------------------------------------------
def test_recipe_changes_the_lists():
    """The recipe's hot words matter: on every committed input the biased list differs from the unbiased one."""
    for case in list(dict.fromkeys(R.CPU_CASES + R.GPU_CASES)):
        plain = [h[0] for h in R.case_reference(case).beam]
        biased = [h[0] for h in BR.case_reference(case).beam]
        assert plain != biased, case


@pytest.mark.parametrize("boost", BOOSTS, ids=["s2", "s0p7"])
@pytest.mark.parametrize("case", R.CPU_CASES, ids=[c[0] for c in R.CPU_CASES])
def test_host_twin_equals_definition(case, boost):
    lb, ids, val, n = R.case_arrays(case)
    T, W = case[2], case[5]
    hot = BR.case_hotwords(case)
    ref = BR.case_reference(case, boost)
    # the condition on the input: every decision, over biased keys and final scores, is 1000 tolerances wide (the mirrored
    # inputs tie exactly by construction and rely on the tie rule)
    if case[6] != "mirror" and ref.beam:
        worst = max(abs(h[1]) for h in ref.beam)
        print(case[0], boost, "gap / tol =", ref.gap / BR.tol(T, worst))
        assert ref.gap >= 1000 * BR.tol(T, worst), (case, boost, ref.gap, BR.tol(T, worst))
    got = host_ctc_beam_hot(lb, ids, val, n, W, hot, boost)
    assert got.n_hyp[0] == len(ref.beam)
    _same(_hyps(got), ref.beam, T)
    s = float(np.float32(boost))
    for h in _hyps(got):
        assert h[1] == h[3] + s * h[2]                                             # one product, one addition
        assert h[2] == BR.walk(h[0], hot)[0]
    for i in range(W):                                                             # every slot is written
        k = int(got.len[0, i])
        assert (got.ids[0, i, k:] == -1).all()
        if i >= got.n_hyp[0]:
            assert k == 0 and got.score[0, i] == -np.inf and got.matched[0, i] == 0 and got.loglik_sum[0, i] == -np.inf
    nb = max(1, W // 2)                                                            # N < W is a prefix of the re-ordered list
    _same(_hyps(host_ctc_beam_hot(lb, ids, val, n, W, hot, boost, nb)), ref.beam[:nb], T)


# ---- 4. no bias means no change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CPU_CASES, ids=[c[0] for c in R.CPU_CASES])
def test_no_bias_is_the_unbiased_twin_bit_for_bit(case):
    lb, ids, val, n = R.case_arrays(case)
    W = case[5]
    plain = host_ctc_beam(lb, ids, val, n, W)
    for hot, boost in ((BR.case_hotwords(case), 0.0), ([], 2.0), ([(), ()], 2.0)):
        got = host_ctc_beam_hot(lb, ids, val, n, W, hot, boost)
        assert (got.n_hyp == plain.n_hyp).all() and (got.ids == plain.ids).all() and (got.len == plain.len).all()
        assert (got.score.view(np.uint64) == plain.score.view(np.uint64)).all()
        assert (got.matched == 0).all() and (got.loglik_sum.view(np.uint64) == plain.score.view(np.uint64)).all()
        ref = BR.case_reference(case, boost, hot)
        unb = R.case_reference(case)
        assert [(h[0], h[1]) for h in ref.beam] == list(unb.beam)                   # and so says the definition


# ---- 5. one case by hand ----------------------------------------------------------------------------------------------------
def test_hand_derived_case():
    """T = 3, blank 0, the listed ids and their probabilities:
         t0: blank .1 | 1: .5   2: .4
         t1: blank .2 | 1: .5   3: .3
         t2: blank .4 | 1: .3   3: .3
    W = 64 prunes nothing, so a score is the log of the summed listed alignments:
      (1,)   = 1bb + 11b + 111 + b1b + b11 + bb1 = .04 + .1 + .075 + .02 + .015 + .006 = .256     the unbiased best
      (1,3)  = 13b + 133 + 1b3 + 113 + b13       = .06 + .045 + .03 + .075 + .015      = .225
      (2,1)  = 21b + 211 + 2b1                   = .08 + .06 + .024                    = .164
      (2,3)  = 23b + 233 + 2b3                   = .048 + .036 + .024                  = .108
    With the hot word (2, 3) and s = 0.5, (2,3) completes it (m = 2): ln .108 + 2 * 0.5 = -1.2256 > ln .256 = -1.3626, and no
    other labeling of three frames that holds 2 3 does better ((2,3,1) = .036); (2,) only has it pending, which the finish
    revokes.  So the best becomes (2, 3) with matched 2 and loglik_sum ln .108."""
    lb = np.log(np.asarray([.1, .2, .4])).astype(np.float32)
    ids = np.asarray([[1, 2], [1, 3], [1, 3]], np.int64)
    val = np.log(np.asarray([[.5, .4], [.5, .3], [.3, .3]])).astype(np.float32)
    n = np.asarray([2, 2, 2], np.int32)
    plain = R.beam_search(lb, ids, val, n, 64).beam
    assert [h[0] for h in plain[:4]] == [(1,), (1, 3), (2, 1), (2, 3)]
    for h, p in zip(plain[:4], (.256, .225, .164, .108)):
        assert abs(h[1] - math.log(p)) < 1e-6
    hot, s = [(2, 3)], 0.5
    for best in (BR.beam_search(lb, ids, val, n, 64, hot, s).beam[0], _hyps(host_ctc_beam_hot(lb, ids, val, n, 64, hot, s))[0]):
        assert best[0] == (2, 3) and best[2] == 2
        assert abs(best[3] - math.log(.108)) < 1e-6 and abs(best[1] - (math.log(.108) + 1.0)) < 1e-6
    second = BR.beam_search(lb, ids, val, n, 64, hot, s).beam[1]
    assert second[0] == (1,) and second[2] == 0
    assert host_ctc_beam(lb, ids, val, n, 64).hyps(0)[0][0] == (1,)
    # (2,) holds the word pending only: nothing stays of it
    two = [h for h in BR.beam_search(lb, ids, val, n, 64, hot, s).beam if h[0] == (2,)][0]
    assert two[2] == 0 and two[1] == two[3]


# ---- 6. refusals, symbols, the CLI, sanitizers ------------------------------------------------------------------------------
def test_argument_refusals():
    lib = N.load()
    case = R.CPU_CASES[0]
    lb, ids, val, n = R.case_arrays(case)
    T, K = case[2], case[4]
    oi, ol, sc, nh = np.zeros((64, T), np.int64), np.zeros(64, np.int32), np.zeros(64, np.float64), C.c_int32()
    om, oll = np.zeros(64, np.int32), np.zeros(64, np.float64)
    f, i64, i32, d = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    a = [lb.ctypes.data_as(f), 1, ids.ctypes.data_as(i64), val.ctypes.data_as(f), n.ctypes.data_as(i32)]
    o = [oi.ctypes.data_as(i64), ol.ctypes.data_as(i32), sc.ctypes.data_as(d)]

    def call(hot=((1, 2),), boost=1.0, W=3, Nq=3, cap=T, m=om.ctypes.data_as(i32), ll=oll.ctypes.data_as(d)):
        hi = np.asarray([c for w in hot for c in w], np.int32)
        hl = np.asarray([len(w) for w in hot], np.int32)
        return lib.pf_host_ctc_beam_hot(*a, T, K, 0, W, Nq, *o, cap, nh, hi.ctypes.data_as(i32), hl.ctypes.data_as(i32), len(hl),
                                        boost, m, ll)
    assert call() == N.PF_OK and nh.value == 3
    for kw in (dict(boost=-1.0), dict(boost=float("nan")), dict(boost=float("inf")), dict(hot=((0,),)), dict(hot=((1, -3),)),
               dict(hot=((1 << 24,),)), dict(m=None), dict(ll=None), dict(W=2, Nq=3), dict(W=65, Nq=1)):
        assert call(**kw) == N.PF_ERR_INVALID_ARG, kw
    assert call(hot=(tuple([1] * 65),)) == N.PF_ERR_CAPACITY
    assert call(cap=0) == N.PF_ERR_CAPACITY
    # null handles
    assert lib.pf_engine_set_ctc_hotwords(None, None, None, 0, 0.0) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_ctc_beam_hot(None, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_recognizer_set_hotword_boost(None, 1.0) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_alternative_hot(None, 0, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_hotword_graph(None, None, 0, 4, None, None, None, None, 0, None, 0) == N.PF_ERR_INVALID_ARG


def test_new_symbols_are_exported_and_declared():
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.pf_version() == 6                      # additions only: the ABI number stays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "paraformer_hip.h")).read()
    for name in NEW:
        assert "int %s(" % name in header, name
    assert "#define PF_HOTWORD_STATES_MAX 4096\n" in header and "#define PF_HOTWORD_LEN_MAX 64\n" in header
    assert (N.PF_HOTWORD_STATES_MAX, N.PF_HOTWORD_LEN_MAX, N.PF_HOTWORD_TABLE_BYTES_MAX) == (4096, 64, 16 << 20)
    cs = open(os.path.join(root, "csharp", "ParaformerHip.cs"), encoding="utf-8-sig").read()
    for name in NEW:
        assert name in cs, name
    rec = open(os.path.join(root, "csharp", "OfflineRecognizerHip.cs"), encoding="utf-8-sig").read()
    assert "SetHotwordBoost" in rec and "HotwordTokens" in rec and "LogLikSum" in rec


def test_cli_arguments():
    from aliparaformerasr_amd import examples as ex
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16", "-hotboost", "1.5"])
    assert (cfg["nbest"], cfg["beam"], cfg["hotboost"]) == (4, 16, 1.5)
    assert "hotboost" not in ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16"])
    for argv in (["-type", "offline", "-hotboost", "1"], ["-type", "offline", "-nbest", "2", "-hotboost", "1"],
                 ["-type", "offline", "-nbest", "2", "-beam", "4", "-hotboost", "-1"],
                 ["-type", "offline", "-nbest", "2", "-beam", "4", "-hotboost", "x"],
                 ["-type", "offline", "-nbest", "2", "-beam", "4", "-hotboost", "inf"],
                 ["-type", "offline", "-nbest", "2", "-beam", "4", "-hotboost"]):
        with pytest.raises(ValueError):
            ex.parse_args(argv)


@pytest.mark.timeout(300)
def test_twin_and_graph_builder_under_sanitizers(tmp_path):
    """csrc/hostutil.cpp's graph builder and biased search in a stand-alone program (tests/native/ctcbeam_bias_sanitize.cpp)
    built with AddressSanitizer + UBSan on the host code, over the committed inputs, the sets of the automaton test, a set at
    the state limit and refused ones: no report, and the library's own answers bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "ctcbeam_bias_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "ctcbeam_bias_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    u32 = lambda a: " ".join(map(str, np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()))  # noqa: E731
    ints = lambda a: " ".join(map(str, a))                                                                     # noqa: E731

    def line(case_arrays, W, Nq, cap, hot, boost):
        lb, ids, val, n = case_arrays
        T, K = ids.shape
        return "%d %d %d %d %d %d %s %s %s %s %s %s %s" % (
            T, K, W, Nq, cap, len(hot), u32([boost]), u32(lb), ints(ids.ravel().tolist()), u32(val), ints(n.tolist()),
            ints(len(w) for w in hot), ints(c for w in hot for c in w))
    lines, want = [], []
    for case in R.CPU_CASES:
        arr = R.case_arrays(case)
        for hot, boost in ((BR.case_hotwords(case), 2.0), (BR.case_hotwords(case), 0.0), ([()], 1.0)):
            lines.append(line(arr, case[5], case[5], max(case[2], 1), hot, boost))
            want.append(host_ctc_beam_hot(*arr, case[5], hot, boost))
    arr = R.case_arrays(R.CPU_CASES[3])
    for name in sorted(SETS):
        lines.append(line(arr, 8, 8, 30, SETS[name], 1.25))
        want.append(host_ctc_beam_hot(*arr, 8, SETS[name], 1.25, 8))
    rng = np.random.default_rng(5)                                                # the state limit, over the case's 11 ids
    many, seen = [], set()
    while True:
        w = tuple(int(c) for c in rng.integers(1, 12, 64))
        if 1 + len(seen | {w[:k] for k in range(1, 65)}) > N.PF_HOTWORD_STATES_MAX:
            break
        many.append(w)
        seen |= {w[:k] for k in range(1, 65)}
    lines.append(line(arr, 8, 8, 30, many, 1.0))
    want.append(host_ctc_beam_hot(*arr, 8, many, 1.0, 8))
    n_ok = len(lines)
    lines.append(line(arr, 8, 8, 30, many + [w], 1.0))                            # one word too many: capacity
    lines.append(line(arr, 8, 8, 30, [tuple([2] * 65)], 1.0))                     # a word of 65 ids
    lines.append(line(arr, 8, 8, 30, [(0, 1)], 1.0))                              # id 0
    lines.append(line(arr, 8, 8, 30, [(1, 2)], -1.0))                             # a negative boost
    lines.append(line(arr, 8, 8, 1, [(1, 2)], 1.0))                               # cap too small
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % len(lines)
    for txt, res in zip(got[:n_ok], want):
        f = [int(x) for x in txt.split()]
        assert f[2] == int(res.n_hyp[0]), txt[:80]
        p = 3
        for i in range(f[2]):
            L = f[p]
            assert L == int(res.len[0, i]) and f[p + 1: p + 1 + L] == res.ids[0, i, :L].tolist()
            assert f[p + 1 + L] == int(res.matched[0, i])
            assert f[p + 2 + L] == int(res.score[0, i: i + 1].view(np.uint64)[0])
            assert f[p + 3 + L] == int(res.loglik_sum[0, i: i + 1].view(np.uint64)[0])
            p += 4 + L
        assert p == len(f)
    assert f[0] <= N.PF_HOTWORD_STATES_MAX and f[0] > N.PF_HOTWORD_STATES_MAX - 64   # the last accepted case sits at the limit
    assert got[n_ok: n_ok + 5] == ["error %d" % N.PF_ERR_CAPACITY] * 2 + ["error %d" % N.PF_ERR_INVALID_ARG] * 2 + \
        ["error %d" % N.PF_ERR_CAPACITY]
