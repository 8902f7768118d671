"""CPU: top-k alternatives and the n-best list without a device — the numpy reference of the selection order pinned by
hand cases, pf_host_nbest against brute-force enumeration (through the library, and as a stand-alone program under
AddressSanitizer + UBSan), the new C ABI symbols, the `-nbest` / `-topk` options of the examples harness."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import examples as ex
from aliparaformerasr_amd.engine import host_nbest
from topk_ref import hyp_score, nbest_brute, topk_ref, topk_row

NEW = ("pf_engine_set_topk", "pf_fetch_topk", "pf_op_topk", "pf_host_nbest", "pf_recognizer_set_nbest",
       "pf_stream_token_alternatives", "pf_stream_num_alternatives", "pf_stream_alternative", "pf_stream_alternative_token")
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _f(*v):
    return np.asarray(v, np.float32)


# ---- the reference, pinned by hand --------------------------------------------------------------------------------------
def test_reference_all_equal_row_gives_descending_indices():
    ids, val, n = topk_row(np.full(9, -1.5, np.float32), 4)
    assert ids.tolist() == [8, 7, 6, 5] and val.tolist() == [-1.5] * 4 and n == 4
    ids, val, n = topk_row(np.full(3, 0.25, np.float32), 3)
    assert ids.tolist() == [2, 1, 0] and n == 3


def test_reference_plain_order_and_ties():
    #            0     1     2     3     4     5
    ids, val, n = topk_row(_f(-3.0, -1.0, -2.0, -1.0, -9.0, -2.0), 5)
    assert ids.tolist() == [3, 1, 5, 2, 0] and val.tolist() == [-1.0, -1.0, -2.0, -2.0, -3.0] and n == 5


def test_reference_signed_zeros_tie():
    # -0.0 == +0.0: the larger index first, each slot keeps its own bit pattern
    ids, val, n = topk_row(_f(0.0, -0.0, -1.0, 0.0, -0.0), 4)
    assert ids.tolist() == [4, 3, 1, 0] and n == 4
    assert np.signbit(val).tolist() == [True, False, True, False]


def test_reference_minus_inf_entries_are_ranked():
    ids, val, n = topk_row(_f(-INF, -2.0, -INF, -INF), 4)
    assert ids.tolist() == [1, 3, 2, 0] and n == 4 and val.tolist() == [-2.0, -np.inf, -np.inf, -np.inf]
    ids, val, n = topk_row(_f(-INF, -INF, -INF), 1)              # the arg-max of a row of -inf only: the last index
    assert ids.tolist() == [2] and n == 1


def test_reference_nan_is_never_ranked():
    ids, val, n = topk_row(_f(NAN, -1.0, NAN, -0.5, NAN), 4)
    assert ids.tolist() == [3, 1, -1, -1] and n == 2
    assert val[:2].tolist() == [-0.5, -1.0] and np.isneginf(val[2:]).all()
    ids, val, n = topk_row(_f(NAN, NAN), 3)
    assert ids.tolist() == [-1, -1, -1] and n == 0 and np.isneginf(val).all()
    ids, val, n = topk_row(_f(INF, NAN, INF), 2)
    assert ids.tolist() == [2, 0] and n == 2


def test_reference_row_shorter_than_k_and_slack():
    ids, val, n = topk_row(_f(-2.0, -1.0), 4)
    assert ids.tolist() == [1, 0, -1, -1] and n == 2 and np.isneginf(val[2:]).all()
    x = np.asarray([[-1.0, -2.0, 5.0, NAN], [-4.0, -3.0, INF, INF]], np.float32)       # ld 4, V 2: the slack is not read
    ids, val, n = topk_ref(x, 3, V=2)
    assert ids.tolist() == [[0, 1, -1], [1, 0, -1]] and n.tolist() == [2, 2] and ids.dtype == np.int64 and n.dtype == np.int32


def test_reference_score_is_a_sequential_float64_sum():
    val = np.asarray([[-0.1], [-1e-9], [-3.0]], np.float32)
    want = ((0.0 + float(np.float32(-0.1))) + float(np.float32(-1e-9))) + -3.0
    assert hyp_score(val, (0, 0, 0)) == want
    ranks, scores = nbest_brute(np.asarray([[-1.0, -2.0], [-1.0, -2.0]], np.float32), [2, 2], 2, 10)
    assert ranks == [(0, 0), (0, 1), (1, 0), (1, 1)] and scores == [-2.0, -3.0, -3.0, -4.0]    # the tie: (0, 1) before (1, 0)
    assert nbest_brute(np.zeros((2, 2), np.float32), [2, 0], 2, 4) == ([], [])


# ---- pf_host_nbest against brute force -----------------------------------------------------------------------------------
def _cases():
    """L 1..5 x K 1..4 x n_free 0..L, ragged n[l], values from a small pool (score ties by construction) and from a
    continuous draw, N below and above the number of hypotheses."""
    rng = np.random.default_rng(7)
    pool = _f(-0.0, 0.0, -0.25, -0.5, -0.5, -1.0, -3.0, -np.inf)
    out = []
    for L in range(1, 6):
        for K in range(1, 5):
            for n_free in range(L + 1):
                for style in range(3):
                    n = rng.integers(1, K + 1, size=L).astype(np.int32)
                    if style == 2:
                        n[:] = K
                    if style == 0:
                        v = rng.choice(pool, size=(L, K))
                    else:
                        v = -rng.random((L, K), dtype=np.float32) * 4
                    v = -np.sort(-v.astype(np.float32), axis=1)                 # rows descending, as the kernel leaves them
                    for l in range(L):
                        v[l, n[l]:] = -np.inf
                    total = int(np.prod([n[l] for l in range(n_free)])) if n_free else 1
                    for Nq in sorted({1, min(max(total // 2, 1), 64), min(total, 64), min(total + 3, 64), 64}):
                        out.append((v, n, n_free, Nq))
    return out


def test_host_nbest_equals_brute_force():
    cases = _cases()
    assert len(cases) > 500
    tied = 0
    for v, n, n_free, Nq in cases:
        ranks, scores = host_nbest(v, n, n_free, Nq)
        want_r, want_s = nbest_brute(v, n, n_free, Nq)
        assert ranks.dtype == np.int32 and scores.dtype == np.float64
        assert [tuple(r) for r in ranks.tolist()] == want_r, (v, n, n_free, Nq)
        assert scores.view(np.uint64).tolist() == np.asarray(want_s, np.float64).view(np.uint64).tolist()
        assert not ranks[0].any()                                               # hypothesis 0: all-zero ranks
        assert (ranks[:, n_free:] == 0).all()
        tied += len(set(want_s)) < len(want_s)
    assert tied > 50                                                            # the tie rule was exercised


def test_host_nbest_ids_and_refusals():
    v = np.asarray([[-0.1, -2.0, -3.0], [-0.5, -0.6, -np.inf]], np.float32)
    n = np.asarray([3, 2], np.int32)
    ids = np.asarray([[5, 6, 7], [8, 9, -1]], np.int64)
    ranks, scores, hyp = host_nbest(v, n, 2, 64, ids=ids)
    assert ranks.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [2, 1]]
    assert hyp.tolist() == [[5, 8], [5, 9], [6, 8], [6, 9], [7, 8], [7, 9]]
    assert host_nbest(v, n, 1, 64)[0].tolist() == [[0, 0], [1, 0], [2, 0]]       # the second position is past n_free
    assert host_nbest(v, n, 0, 64)[0].tolist() == [[0, 0]]
    assert len(host_nbest(v, np.asarray([3, 0], np.int32), 2, 8)[0]) == 0        # a position with no ranked entry
    lib = N.load()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    r, s, got = np.zeros((4, 2), np.int32), np.zeros(4, np.float64), C.c_int32()
    d = s.ctypes.data_as(C.POINTER(C.c_double))

    def call(val, nn, L, K, n_free, Nq):
        return lib.pf_host_nbest(None, val.ctypes.data_as(f32), nn.ctypes.data_as(i32), L, K, n_free, Nq, r.ctypes.data_as(i32), d, got)
    assert call(v, n, 2, 3, 2, 4) == N.PF_OK and got.value == 4
    for bad in ((2, 3, 3, 4), (2, 3, -1, 4), (2, 3, 2, 0), (2, 3, 2, 65), (2, 9, 2, 4), (0, 3, 0, 4), (2, 0, 2, 4)):
        assert call(v, n, *bad) == N.PF_ERR_INVALID_ARG, bad
    assert call(v, np.asarray([4, 2], np.int32), 2, 3, 2, 4) == N.PF_ERR_INVALID_ARG               # n[l] > K
    vn = v.copy(); vn[1, 1] = np.nan
    assert call(vn, n, 2, 3, 2, 4) == N.PF_ERR_INVALID_ARG
    vn[1, 1] = np.inf
    assert call(vn, n, 2, 3, 2, 4) == N.PF_ERR_INVALID_ARG
    assert lib.pf_host_nbest(None, None, n.ctypes.data_as(i32), 2, 3, 2, 4, r.ctypes.data_as(i32), d, got) == N.PF_ERR_INVALID_ARG


@pytest.mark.timeout(300)
def test_host_nbest_under_sanitizers(tmp_path):
    """csrc/hostutil.cpp's enumerator in a stand-alone program (tests/native/nbest_sanitize.cpp) built with AddressSanitizer +
    UBSan on the host code, over the cases of the brute-force test (plus refused ones): no report, the same lists."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "nbest_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "nbest_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    cases = _cases()
    bad = [(cases[0][0], cases[0][1], 0, 0), (cases[0][0], cases[0][1], 0, 65)]
    lines = []
    for v, n, n_free, Nq in cases + bad:
        L, K = v.shape
        lines.append("%d %d %d %d %s %s" % (L, K, n_free, Nq, " ".join(map(str, n.tolist())),
                                            " ".join(map(str, np.ascontiguousarray(v).view(np.uint32).ravel().tolist()))))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % (len(cases) + 2) and got[-3:-1] == ["error %d" % N.PF_ERR_INVALID_ARG] * 2
    for (v, n, n_free, Nq), line in zip(cases, got):
        want_r, want_s = nbest_brute(v, n, n_free, Nq)
        f = [int(t) for t in line.split()]
        L = v.shape[0]
        assert f[0] == len(want_r)
        for i in range(f[0]):
            rec = f[1 + i * (L + 1): 1 + (i + 1) * (L + 1)]
            assert tuple(rec[:L]) == want_r[i]
            assert rec[L] == int(np.float64(want_s[i]).view(np.uint64))


# ---- symbols, null handles, CLI ------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert N.PF_DECODE_TOPK not in (0, N.PF_DECODE_SCORES, N.PF_DECODE_CTC) and N.PF_DECODE_TOPK & (N.PF_DECODE_TOPK - 1) == 0
    assert (N.PF_TOPK_MAX, N.PF_NBEST_MAX) == (8, 64)
    assert lib.pf_version() == 6                      # additions only: the ABI number stays
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "paraformer_hip.h")).read()
    assert "#define PF_DECODE_TOPK %d\n" % N.PF_DECODE_TOPK in header
    for name in NEW:
        assert "int %s(" % name in header, name


def test_null_handles_are_refused():
    lib = N.load()
    n, k = C.c_int32(), C.c_int32()
    pi, pv, pc, sc = C.POINTER(C.c_int64)(), C.POINTER(C.c_float)(), C.c_char_p(), C.c_double()
    assert lib.pf_engine_set_topk(None, 4) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_topk(None, None, None, None, 0, n, k) == N.PF_ERR_INVALID_ARG
    assert lib.pf_op_topk(None, None, 1, 1, 1, 1, None, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_recognizer_set_nbest(None, 4, 4) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_token_alternatives(None, C.byref(pi), C.byref(pv), n, k) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_num_alternatives(None, n) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_alternative(None, 0, C.byref(pi), n, C.byref(sc), C.byref(pc), k) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_alternative_token(None, 0, 0, C.byref(pc)) == N.PF_ERR_INVALID_ARG


def test_examples_nbest_options():
    cfg = ex.parse_args(["-type", "offline", "-nbest", "5", "-files", "a.wav"])
    assert cfg["nbest"] == 5 and "topk" not in cfg and cfg["files"] == ["a.wav"]
    cfg = ex.parse_args(["-type", "offline", "-topk", "8", "-nbest", "64"])
    assert (cfg["nbest"], cfg["topk"]) == (64, 8)
    assert "nbest" not in ex.parse_args(["-type", "offline"])                   # default: no alternatives
    for bad in (["-nbest"], ["-nbest", "0"], ["-nbest", "65"], ["-nbest", "x"], ["-nbest", "3", "-topk", "9"],
                ["-nbest", "3", "-topk", "0"], ["-nbest", "3", "-topk"]):
        with pytest.raises(ValueError, match="nbest|topk"):
            ex.parse_args(["-type", "offline"] + bad)
    with pytest.raises(ValueError, match="-topk goes with -nbest"):
        ex.parse_args(["-type", "offline", "-topk", "4"])
    with pytest.raises(ValueError, match="offline"):
        ex.parse_args(["-type", "online", "-nbest", "4"])
    with pytest.raises(ValueError, match="Unknown parameters"):
        ex.parse_args(["-type", "offline", "-n-best", "4"])
