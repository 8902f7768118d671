"""CPU: CTC forced alignment (PF_DECODE_ALIGN) — the definition (tests/ctcalign_ref.py) against brute-force enumeration of
every alignment, the host twin (pf_host_ctc_align, csrc/hostutil.cpp) against the definition over a case table, refusals,
symbols, the CLI's argument checks, and the twin as a stand-alone program under AddressSanitizer + UBSan.

Comparison rule: path_score, ok, first, last and tok_score identical (float32 bit for bit); loglik within
16 * T * 2^-53 * max(1, |s|) (ctcalign_ref.loglik_tol), non-finite values identical."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctcalign_ref as R
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd.engine import host_ctc_align

NEW = ("pf_engine_set_align_targets", "pf_fetch_align", "pf_host_ctc_align", "pf_op_ctc_align", "pf_recognizer_set_align",
       "pf_stream_set_align_ids", "pf_stream_alignment", "pf_stream_alternative_timestamps")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(tag, got, ref, T):
    """(ok, path_score, loglik, first, last, tok_score) of the twin against a ctcalign_ref.Alignment"""
    ok, ps, ll, first, last, tok = got
    assert ok == ref.ok, (tag, ok, ref.ok)
    assert _bits(ps) == _bits(ref.path_score) or (np.isnan(ps) and np.isnan(ref.path_score)), (tag, ps, ref.path_score)
    np.testing.assert_array_equal(first, ref.first, err_msg=tag)
    np.testing.assert_array_equal(last, ref.last, err_msg=tag)
    np.testing.assert_array_equal(_bits(tok), _bits(ref.tok_score), err_msg=tag)
    if math.isfinite(ref.loglik):
        assert abs(ll - ref.loglik) <= R.loglik_tol(T, ref.loglik), (tag, ll, ref.loglik)
        return abs(ll - ref.loglik) / R.loglik_tol(T, ref.loglik)
    assert ll == ref.loglik or (math.isnan(ll) and math.isnan(ref.loglik)), (tag, ll, ref.loglik)
    return 0.0


def _twin(lp, y, V=None):
    r = host_ctc_align(lp, y, V)
    return int(r.ok[0, 0]), r.path_score[0, 0], float(r.loglik[0, 0]), r.first[0, 0], r.last[0, 0], r.tok_score[0, 0]


def _case_table():
    """(tag, lp [T, V], y): U in {0, 1, 2, 7, 8}; one repeated id; T at the minimum (U + adjacent repeats) and one below;
    T = 0; a NaN row; -inf entries; integer-valued tie inputs"""
    rng = np.random.default_rng(11)
    out = []
    for U in (0, 1, 2, 7, 8):
        for T in (1, 2, 9, 40):
            lp, y = R.random_case(rng, T, 6, U)
            out.append(("random U=%d T=%d" % (U, T), lp, y))
    for U in (1, 2, 7, 8):
        y = [3] * U
        for T in (2 * U - 1, 2 * U - 2, 2 * U + 5):
            out.append(("repeated U=%d T=%d" % (U, T), R.random_case(rng, max(T, 1), 6, 0)[0][:T], y))
    for y in ([1, 1, 2], [2, 3, 3, 3, 1, 1, 4], [5, 4, 3, 2, 1], [1, 2, 1, 2, 2]):
        need = R.min_frames(y)
        for T in (need, need - 1):
            out.append(("minimal %s T=%d" % (y, T), R.random_case(rng, T, 6, 0)[0], y))
    for U in (0, 1, 3):
        out.append(("no frames U=%d" % U, np.zeros((0, 6), np.float32), [1, 2, 3][:U]))
    lp, y = R.random_case(rng, 8, 6, 0)[0], [1, 2, 3]
    nan = lp.copy()
    nan[4] = np.nan
    out.append(("nan row", nan, y))
    out.append(("nan row, no tokens", nan, []))
    ninf = lp.copy()
    ninf[:, 2] = -np.inf
    out.append(("-inf column of a token", ninf, y))
    ninf = lp.copy()
    ninf[3, 0] = -np.inf
    ninf[5, 1:] = -np.inf
    out.append(("-inf entries on some paths", ninf, y))
    out.append(("-inf blank, no tokens", ninf, []))
    for k in range(40):
        lp, y = R.tie_case(rng, int(rng.integers(1, 30)), int(rng.integers(2, 4)), int(rng.integers(0, 9)))
        out.append(("ties %d" % k, lp, y))
    return out


CASES = _case_table()


# ---- the definition ------------------------------------------------------------------------------------------------------------
def test_reference_equals_brute_force():
    """Score bits always; the path where brute force finds one optimum; on integer-valued inputs (exact ties) the optimal path
    that is largest when read from the last frame backwards."""
    unique, multi = R.check_against_brute()
    print("  %d random inputs with one optimum, %d tie inputs with several" % (unique, multi))
    assert unique >= 200 and multi >= 50


def test_reference_properties():
    rng = np.random.default_rng(5)
    lp, y = R.random_case(rng, 30, 8, 6)
    r = R.align(lp, y)
    assert r.ok == 1 and r.loglik >= float(r.path_score) - 1e-4                   # a sum is no smaller than its largest term
    assert (r.first <= r.last).all() and (r.first[1:] > r.last[:-1]).all() and r.first[0] >= 0 and r.last[-1] < 30
    for u, c in enumerate(y):                                                     # the token score is the run's maximum
        assert r.tok_score[u] == lp[r.first[u]: r.last[u] + 1, c].max()
    s = np.float32(lp[0, 0 if r.path[0] % 2 == 0 else y[r.path[0] // 2]])        # the score is the path's sequential sum
    for t in range(1, 30):
        s = np.float32(s + lp[t, 0 if r.path[t] % 2 == 0 else y[r.path[t] // 2]])
    assert _bits(s) == _bits(r.path_score)
    assert R.ROUNDINGS_PER_FRAME == 16 and R.loglik_tol(10, -50.0) == 16 * 10 * 2.0 ** -53 * 50
    assert R.min_frames([1, 1, 2, 2, 2]) == 8 and R.min_frames([]) == 0
    e = R.align(np.zeros((0, 4), np.float32), [])
    assert e.ok == 1 and e.path_score == 0 and e.loglik == 0
    assert R.align(np.zeros((0, 4), np.float32), [1]).ok == 0


# ---- the host twin ---------------------------------------------------------------------------------------------------------------
def test_host_twin_equals_reference():
    worst = 0.0
    oks = set()
    for tag, lp, y in CASES:
        ref = R.align(lp, y)
        oks.add((tag.split()[0], ref.ok))
        worst = max(worst, _same(tag, _twin(lp, y), ref, max(lp.shape[0], 1)))
    print("  %d cases, worst loglik difference %.3g of the tolerance" % (len(CASES), worst))
    for kind in ("repeated", "minimal", "no"):                                    # both outcomes are in the table
        assert (kind, 0) in oks and (kind, 1) in oks, kind
    assert ("nan", 0) in oks and ("-inf", 0) in oks and ("-inf", 1) in oks
    # a row stride: nothing beyond V in a row is read
    rng = np.random.default_rng(2)
    lp, y = R.random_case(rng, 12, 7, 4)
    wide = np.full((12, 20), np.inf, np.float32)
    wide[:, :7] = lp
    _same("ld = 20", _twin(wide, y, V=7), R.align(lp, y), 12)


def test_argument_refusals():
    lib = N.load()
    lp = np.zeros((4, 5), np.float32)
    y = np.array([1, 2], np.int64)
    first, last, tok = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.float32)
    ps, ll, ok = C.c_float(), C.c_double(), C.c_int32()
    f, i64, i32 = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def call(lp_=lp.ctypes.data_as(f), ld=5, T=4, V=5, y_=y, U=2, ps_=ps, ll_=C.byref(ll), ok_=ok, first_=first.ctypes.data_as(i32)):
        return lib.pf_host_ctc_align(lp_, ld, T, V, y_.ctypes.data_as(i64), U, ps_, ll_, ok_, first_, last.ctypes.data_as(i32),
                                     tok.ctypes.data_as(f))
    assert call() == N.PF_OK and ok.value == 1
    for kw in (dict(lp_=None), dict(ld=4), dict(T=-1), dict(V=0), dict(U=-1), dict(ps_=None), dict(ll_=None), dict(ok_=None),
               dict(first_=None), dict(y_=np.array([1, 5], np.int64)), dict(y_=np.array([0, 1], np.int64)),
               dict(y_=np.array([1, -2], np.int64))):
        assert call(**kw) == N.PF_ERR_INVALID_ARG, kw
    long = np.ones(N.PF_ALIGN_MAX_TOKENS + 1, np.int64)
    assert call(y_=long, U=long.shape[0]) == N.PF_ERR_CAPACITY
    # null handles
    assert lib.pf_engine_set_align_targets(None, None, None, 0, 0) == N.PF_ERR_INVALID_ARG
    assert lib.pf_fetch_align(None, None, None, None, None, None, None, None, 0, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_recognizer_set_align(None, 1) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_set_align_ids(None, None, -1) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_alignment(None, None, None, None, None, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_stream_alternative_timestamps(None, 0, None, None, None) == N.PF_ERR_INVALID_ARG
    assert lib.pf_op_ctc_align(None, None, 0, 0, 1, 1, None, None, None, 0, 1, None, None, None, None, None, None) == N.PF_ERR_INVALID_ARG


def test_new_symbols_are_exported_and_declared():
    lib = N.load()
    for name in NEW:
        assert name in N.SIGNATURES, name
        assert hasattr(lib, name), name
    assert N.PF_DECODE_ALIGN == 32 and N.PF_ALIGN_MAX_TOKENS == 1023
    assert lib.pf_version() == 6                      # additions only: the ABI number stays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "paraformer_hip.h")).read()
    assert "#define PF_DECODE_ALIGN 32\n" in header and "#define PF_ALIGN_MAX_TOKENS 1023\n" in header
    cs = open(os.path.join(root, "csharp", "ParaformerHip.cs"), encoding="utf-8-sig").read()
    assert "PF_DECODE_ALIGN = 32" in cs
    rec = open(os.path.join(root, "csharp", "OfflineRecognizerHip.cs"), encoding="utf-8-sig").read()
    assert "SetAlign" in rec and "SetAlignIds" in rec
    mk = open(os.path.join(root, "aliparaformerasr_amd", "csrc", "Makefile")).read()
    assert "k_ctcalign.hip" in mk


def test_cli_arguments(tmp_path):
    from aliparaformerasr_amd import examples as ex
    cfg = ex.parse_args(["-type", "offline", "-align", "ids.txt", "-files", "a.wav"])
    assert cfg["align"] == "ids.txt"
    cfg = ex.parse_args(["-type", "offline", "-nbest", "4", "-beam", "16", "-align", "beam"])
    assert (cfg["nbest"], cfg["beam"], cfg["align"]) == (4, 16, "beam")
    assert "align" not in ex.parse_args(["-type", "offline", "-nbest", "4"])
    for argv in (["-type", "offline", "-align"], ["-type", "offline", "-align", "-files"], ["-type", "offline", "-align", "beam"],
                 ["-type", "offline", "-nbest", "2", "-align", "beam"], ["-type", "online", "-align", "ids.txt"]):
        with pytest.raises(ValueError):
            ex.parse_args(argv)
    p = tmp_path / "ids.txt"
    p.write_text("5 6 7\n\n12\n")
    assert ex.read_align_file(str(p)) == [[5, 6, 7], None, [12]]
    p.write_text("5 six\n")
    with pytest.raises(ValueError):
        ex.read_align_file(str(p))


# ---- the twin under sanitizers ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_host_ctc_align_under_sanitizers(tmp_path):
    """csrc/hostutil.cpp's alignment in a stand-alone program (tests/native/ctcalign_sanitize.cpp) built with
    AddressSanitizer + UBSan on the host code, over the case table (plus refused inputs): no report, the same results."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    exe = str(tmp_path / "ctcalign_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "ctcalign_sanitize.cpp"),
                        os.path.join(cs, "hostutil.cpp"), "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    u32 = lambda a: " ".join(map(str, _bits(a).ravel().tolist()))  # noqa: E731
    lines = []
    for _tag, lp, y in CASES:
        T, V = lp.shape
        lines.append(("%d %d %d %d %s %s" % (T, V, V, len(y), u32(lp), " ".join(map(str, y)))).strip())
    lp = CASES[1][1]
    lines.append("%d %d %d 2 %s 1 %d" % (lp.shape[0], lp.shape[1], lp.shape[1], u32(lp), lp.shape[1]))        # an id = V
    lines.append("1 6 6 %d %s %s" % (N.PF_ALIGN_MAX_TOKENS + 1, u32(np.zeros(6)), " ".join(["1"] * (N.PF_ALIGN_MAX_TOKENS + 1))))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ok %d" % len(lines)
    assert got[-3:-1] == ["error %d" % N.PF_ERR_INVALID_ARG, "error %d" % N.PF_ERR_CAPACITY]
    for (tag, lp, y), line in zip(CASES, got):
        f = [int(x) for x in line.split()]
        U = len(y)
        assert len(f) == 3 + 3 * U, (tag, line)
        ps = np.array([f[1]], np.uint32).view(np.float32)[0]
        ll = float(np.array([f[2]], np.uint64).view(np.float64)[0])
        tok = np.array(f[5::3], np.uint32).view(np.float32) if U else np.zeros(0, np.float32)
        _same(tag, (f[0], ps, ll, np.array(f[3::3], np.int32), np.array(f[4::3], np.int32), tok), R.align(lp, y), max(lp.shape[0], 1))
