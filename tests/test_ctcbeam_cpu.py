"""CPU: the CTC prefix beam search — the definition (tests/ctcbeam_ref.py) against brute-force enumeration of all alignments,
the host twin (pf_host_ctc_beam, csrc/hostutil.cpp) against the definition over the committed inputs, the condition those
inputs must meet (a decision gap of 1000 tolerances), refusals, symbols, the CLI arguments, and the twin once more in a
stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctcbeam_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import host_ctc_beam

NEW = ("pf_engine_set_ctc_beam", "pf_fetch_ctc_beam", "pf_host_ctc_beam", "pf_op_ctc_beam", "pf_recognizer_set_ctc_beam")
ALL_CASES = list(dict.fromkeys(R.CPU_CASES + R.GPU_CASES))


def _same(got, ref, T, n_best=None):
    """token lists and their order identical; scores within 16 * T * 2^-53 * max(1, |s|)"""
    want = ref.beam if n_best is None else ref.beam[:n_best]
    assert [h[0] for h in got] == [h[0] for h in want]
    for (_, a), (_, b) in zip(got, want):
        assert abs(a - b) <= R.tol(T, b), (a, b, abs(a - b), R.tol(T, b))


# ---- the definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,V", [(4, 3), (5, 3), (3, 4)])
def test_reference_equals_brute_force(T, V):
    """K covers every non-blank id and W = 64 prunes nothing: every labeling's score is the log of its summed alignments."""
    for seed in range(3):
        x = R.random_rows(seed, T, V).astype(np.float64)
        want = R.brute_force(x)
        ids, _, n = R.topk_lists(x.astype(np.float32), V)
        val = np.take_along_axis(x, np.maximum(ids, 0), 1)                      # the float64 rows themselves
        res = R.beam_search(x[:, 0], ids, val, n, 64)
        assert len(res.beam) == len(want) < 64
        for prefix, s in res.beam:
            assert abs(s - want[prefix]) <= 1e-14, (prefix, s, want[prefix])
            assert abs(s - R.ctc_loglik(x, prefix)) <= 1e-14


def test_parent_identity_differs_on_the_committed_seeds():
    """The inputs that tell sequence identity from node identity: the faulty variant keeps another list on each."""
    for case in R.CPU_CASES[: len(R.PARENT_SEEDS)]:
        lb, ids, val, n = R.case_arrays(case)
        good = R.case_reference(case)
        bad = R.beam_search(lb, ids, val, n, case[5], identity="parent")
        assert [h[0] for h in good.beam] != [h[0] for h in bad.beam] or any(abs(a[1] - b[1]) > 1e-9 for a, b in zip(good.beam, bad.beam))
        assert len({h[0] for h in good.beam}) == len(good.beam)                 # the definition never lists a prefix twice


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] + "_" + str(i) for i, c in enumerate(ALL_CASES)])
def test_committed_inputs_have_a_decision_gap(case):
    """A condition on the inputs, not a measurement: every decision the search takes on a committed input is 1000 tolerances
    wide (for its first frame and its first half too: the GPU tests run those lengths).  Mirrored inputs tie exactly
    where the mirror says so; their other gaps meet the same condition."""
    for T in (None, 1, max(case[2] // 2, 1)):
        ref = R.case_reference(case, T)
        frames = case[2] if T is None else T
        worst = min(s for _, s in ref.beam)
        gap = ref.gap_pos if case[6] == "mirror" else ref.gap
        assert gap >= 1000 * R.tol(frames, worst), (case, T, gap, R.tol(frames, worst))
    if case[6] == "mirror":
        assert R.case_reference(case).gap == 0                                  # the tie is there, and exact


# ---- the host twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CPU_CASES, ids=[c[0] for c in R.CPU_CASES])
def test_host_twin_equals_reference(case):
    lb, ids, val, n = R.case_arrays(case)
    T, W = case[2], case[5]
    ref = R.case_reference(case)
    got = host_ctc_beam(lb, ids, val, n, W)
    assert got.n_hyp[0] == len(ref.beam)
    _same(got.hyps(0), ref, T)
    # slots past a hypothesis and past n_hyp hold the fill values
    for i in range(W):
        k = int(got.len[0, i])
        assert (got.ids[0, i, k:] == -1).all()
        if i >= got.n_hyp[0]:
            assert k == 0 and got.score[0, i] == -np.inf
    # N < W is a prefix of the list; a strided blank column reads the same values
    nb = max(1, W // 2)
    _same(host_ctc_beam(lb, ids, val, n, W, nb).hyps(0), ref, T, nb)
    wide = np.full((T, 3), np.nan, np.float32)
    wide[:, 0] = lb
    _same(host_ctc_beam(wide, ids, val, n, W, blank_stride=3).hyps(0), ref, T)


def test_host_twin_case_table_covers_the_issue():
    assert {c[5] for c in R.CPU_CASES} >= {1, 2, 3, 16, 64} and {c[4] for c in R.CPU_CASES} >= {1, 4, 8}
    inside = outside = 0
    for case in R.CPU_CASES:
        _, ids, _, n = R.case_arrays(case)
        has = [(ids[t, : n[t]] == 0).any() for t in range(case[2])]
        inside += any(has)
        outside += not all(has)
    assert inside and outside
    assert any((R.case_arrays(c)[3] < c[4]).any() for c in R.CPU_CASES if c[6] == "ragged")


def test_host_twin_empty_frame_nan_blank_and_no_frames():
    case = R.CPU_CASES[4]
    lb, ids, val, n = R.case_arrays(case)
    T, K, W = case[2], case[4], case[5]
    hole = n.copy()
    hole[T // 2] = 0
    assert R.beam_search(lb, ids, val, hole, W).n_hyp == 0
    got = host_ctc_beam(lb, ids, val, hole, W)
    assert got.n_hyp[0] == 0 and (got.ids == -1).all() and (got.len == 0).all() and (got.score == -np.inf).all()
    nan = lb.copy()
    nan[T - 1] = np.nan
    assert R.beam_search(nan, ids, val, n, W).n_hyp == 0
    assert host_ctc_beam(nan, ids, val, n, W).n_hyp[0] == 0
    # T = 0: the beam is what it starts as — the empty labeling with probability 1
    ref = R.beam_search(lb[:0], ids[:0], val[:0], n[:0], W)
    assert ref.beam == [((), 0.0)]
    got = host_ctc_beam(lb[:0], np.zeros((0, K), np.int64), np.zeros((0, K), np.float32), n[:0], W)
    assert got.n_hyp[0] == 1 and got.len[0, 0] == 0 and got.score[0, 0] == 0.0 and (got.ids == -1).all()


def test_mirrored_ties_go_to_the_smaller_candidate_index():
    """Columns 1 = 2 and 3 = 4 bit for bit: candidates that differ by the mirror total the same to the bit wherever both are
    alive, so the search decides exact ties (the definition reports a decision gap of 0), and the twin decides them alike.
    (After a tie at the beam's edge dropped one of the two, their descendants no longer mirror each other.)"""
    cases = [c for c in R.CPU_CASES if c[6] == "mirror"]
    assert len(cases) >= 3
    for case in cases:
        lb, ids, val, n = R.case_arrays(case)
        ref = R.case_reference(case)
        assert ref.gap == 0
        _same(host_ctc_beam(lb, ids, val, n, case[5]).hyps(0), ref, case[2])
    # one frame, nothing pruned: the mirrored labelings are neighbours with one score, the larger id first (the list's order)
    lb, ids, val, n = R.case_arrays(cases[-1])                                   # K = 8 lists all of V = 6
    got = host_ctc_beam(lb[:1], ids[:1], val[:1], n[:1], 8).hyps(0)
    assert len(got) == 6
    tied = [(a, b) for a, b in zip(got, got[1:]) if a[1] == b[1]]
    assert len(tied) == 2 and all(a[0][0] > b[0][0] and {a[0][0], b[0][0]} in ({1, 2}, {3, 4}) for a, b in tied)


def test_argument_refusals():
    lib = N.load()
    case = R.CPU_CASES[0]
    lb, ids, val, n = R.case_arrays(case)
    T, K = case[2], case[4]
    oi, ol, sc, nh = np.zeros((64, T), np.int64), np.zeros(64, np.int32), np.zeros(64, np.float64), C.c_int32()
    f, i64, i32, d = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    a = [lb.ctypes.data_as(f), 1, ids.ctypes.data_as(i64), val.ctypes.data_as(f), n.ctypes.data_as(i32)]
    o = [oi.ctypes.data_as(i64), ol.ctypes.data_as(i32), sc.ctypes.data_as(d)]

    def call(T=T, K=K, W=3, Nq=3, cap=T, args=a, outs=o, nhyp=nh):
        return lib.pf_host_ctc_beam(*args, T, K, 0, W, Nq, *outs, cap, nhyp)
    assert call() == N.PF_OK and nh.value == 3
    for kw in (dict(W=0, Nq=0), dict(W=65, Nq=1), dict(W=2, Nq=3), dict(Nq=0), dict(K=0), dict(K=9), dict(T=-1), dict(cap=-1),
               dict(args=[a[0], 0] + a[2:]), dict(args=[None] + a[1:]), dict(outs=[None] + o[1:]), dict(nhyp=None)):
        assert call(**kw) == N.PF_ERR_INVALID_ARG, kw
    bad_n = n.copy()
    bad_n[3] = K + 1
    assert call(args=a[:4] + [bad_n.ctypes.data_as(i32)]) == N.PF_ERR_INVALID_ARG
    assert call(cap=0) == N.PF_ERR_CAPACITY                                     # the hypotheses have tokens
    # null handles
    assert lib.pf_engine_set_ctc_beam(None, 16, 16) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_ctc_beam(None, None, None, None, 0, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_recognizer_set_ctc_beam(None, 4, 8, 4) == N.PF_ERR_INVALID_ARG


def test_new_symbols_are_exported_and_declared():
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert N.PF_DECODE_CTC_BEAM == 16
    assert lib.pf_version() == 6                      # additions only: the ABI number stays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "paraformer_hip.h")).read()
    assert "#define PF_DECODE_CTC_BEAM 16\n" in header
    cs = open(os.path.join(root, "csharp", "ParaformerHip.cs"), encoding="utf-8-sig").read()
    assert "PF_DECODE_CTC_BEAM = 16" in cs
    assert "SetCtcBeam" in open(os.path.join(root, "csharp", "OfflineRecognizerHip.cs"), encoding="utf-8-sig").read()


def test_cli_arguments():
    from aliparaformerasr_amd import examples as ex
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16", "-topk", "8"])
    assert (cfg["nbest"], cfg["beam"], cfg["topk"]) == (4, 16, 8)
    assert "beam" not in ex.parse_args(["-type", "offline", "-nbest", "4"])
    for argv in (["-type", "offline", "-beam", "8"], ["-type", "offline", "-nbest", "9", "-beam", "8"],
                 ["-type", "offline", "-nbest", "2", "-beam", "65"], ["-type", "offline", "-nbest", "2", "-beam", "x"],
                 ["-type", "online", "-nbest", "2", "-beam", "4"]):
        with pytest.raises(ValueError):
            ex.parse_args(argv)


# ---- the twin under sanitizers ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_host_ctc_beam_under_sanitizers(tmp_path):
    """csrc/hostutil.cpp's beam search in a stand-alone program (tests/native/ctcbeam_sanitize.cpp) built with
    AddressSanitizer + UBSan on the host code, over the committed inputs (plus refused ones): no report, the same lists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "ctcbeam_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "ctcbeam_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    u32 = lambda a: " ".join(map(str, np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()))  # noqa: E731
    lines, want = [], []
    for case in R.CPU_CASES:
        lb, ids, val, n = R.case_arrays(case)
        T, K, W = case[2], case[4], case[5]
        lines.append("%d %d %d %d %d %s %s %s %s" % (T, K, W, W, max(T, 1), u32(lb), " ".join(map(str, ids.ravel().tolist())), u32(val),
                                                     " ".join(map(str, n.tolist()))))
        want.append((T, R.case_reference(case)))
    lb, ids, val, n = R.case_arrays(R.CPU_CASES[0])
    lines.append("0 3 4 2 1")                                                    # no frames
    want.append((0, R.beam_search(lb[:0], ids[:0], val[:0], n[:0], 4, 2)))
    tail = "%s %s %s %s" % (u32(lb), " ".join(map(str, ids.ravel().tolist())), u32(val), " ".join(map(str, n.tolist())))
    lines.append("12 3 2 3 12 " + tail)                                          # N > W
    lines.append("12 3 3 3 1 " + tail)                                           # cap too small
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % len(lines)
    assert got[-3:-1] == ["error %d" % N.PF_ERR_INVALID_ARG, "error %d" % N.PF_ERR_CAPACITY]
    for (T, ref), line in zip(want, got):
        f = line.split()
        hyps, at = [], 1
        for _ in range(int(f[0])):
            k = int(f[at])
            ids_ = tuple(int(x) for x in f[at + 1: at + 1 + k])
            hyps.append((ids_, float(np.uint64(int(f[at + 1 + k])).view(np.float64))))
            at += k + 2
        assert at == len(f)
        _same(hyps, ref, T, len(ref.hyps))
