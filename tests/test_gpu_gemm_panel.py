"""GPU: the panel-resident K = 512 GEMM (csrc/k_gemm_panel.hip gemm_panel_kernel) — the decoder's K | V projection of all
layers and the vocabulary layer.

  test_panel_exact          small-integer inputs (every fp32 sum exact, every result an f16 integer): the same bits as numpy,
                            at every row / column edge of the kernel's geometry (128-row panels, 64-column blocks, shares of N),
                            through pf_op_gemm_panel — a hostile host: NaNs behind the last row of A and of W, a
                            sentinel-filled result in which only [M, N] may change (the op raises otherwise);
  test_panel_matches_tiled  random f16-rounded inputs: bit-equal to gemm_f16_pp3 with 128- and 256-row tiles, both result forms,
                            including the vocabulary's ragged width (both kernels accumulate every output over k ascending in
                            steps of 16 on the same MFMA and round at the same points);
  test_panel_in_engine      PF_GEMM_PANEL = 0 against 1 on two engines of the small configuration;
  test_panel_beside_another_engine   the operator beside a second, recognising engine: the quiet bits.

Measured on an MI355X: all 20 cases pass in 6 s; every comparison is bit-equal (no bound is used anywhere in this file)."""
import threading
import time

import numpy as np
import pytest

from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

PANEL = "gemm_panel_kernel<"


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=5)), cmvn=W.synth_cmvn(), device=0)
    e.profile(True)
    yield e
    e.close()


def _ints(M, N, seed):
    """|a| <= 1, |w| <= 2, |bias| <= 8: |sum| <= 1032, exact in fp32 in any order and exact as f16"""
    rng = np.random.default_rng(seed)
    A = rng.integers(-1, 2, (M, 512)).astype(np.float32)
    Wt = rng.integers(-2, 3, (N, 512)).astype(np.float32)
    b = rng.integers(-8, 9, N).astype(np.float32)
    return A, Wt, b


def _run(eng, A, Wt, b, f16_out, form, padded, want_kernel):
    eng.profile_reset()
    got = eng.op_gemm_panel(A, Wt, b, f16_out=f16_out, form=form, padded=padded)
    ran = eng.profile_kernel("gemm_op")
    assert ran.startswith(want_kernel), "ran %r, expected %s..." % (ran, want_kernel)
    return got


@pytest.mark.parametrize("N", [64, 300, 1088])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_panel_exact(eng, M, N):
    A, Wt, b = _ints(M, N, 1000 * M + N)
    want = (A.astype(np.float64) @ Wt.astype(np.float64).T + b).astype(np.float32)
    for f16_out in (True, False):
        for padded in (False, True):
            got = _run(eng, A, Wt, b if f16_out else None, f16_out, 7, padded, PANEL)
            ref = want if f16_out else want - b
            assert not np.isnan(got).any(), "M %d N %d f16 %d padded %d: a NaN from behind an operand reached the result" % (M, N, f16_out, padded)
            assert np.array_equal(got, ref), "M %d N %d f16 %d padded %d: %d cells differ, max |d| %g" % (
                M, N, f16_out, padded, int((got != ref).sum()), float(np.abs(got - ref).max()))
    got = _run(eng, A, Wt, b, False, 7, False, PANEL)         # fp32 result with the bias
    assert np.array_equal(got, want)


@pytest.mark.parametrize("M,N,f16_forms", [(300, 1088, (True, False)), (640, 2048, (True, False)), (384, 8404, (False,))])
def test_panel_matches_tiled(eng, M, N, f16_forms):
    rng = np.random.default_rng(M + N)
    A = rng.standard_normal((M, 512)).astype(np.float16).astype(np.float32)
    Wt = (rng.standard_normal((N, 512)) / 22).astype(np.float16).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    for f16_out in f16_forms:
        for padded in (True, False):
            got = _run(eng, A, Wt, b, f16_out, 7, padded, PANEL)
            assert np.isfinite(got).all()
            for form in (1, 2):
                tiled = _run(eng, A, Wt, b, f16_out, form, padded, "gemm_f16_pp3<")
                d = got != tiled
                assert not d.any(), "M %d N %d f16 %d padded %d: %d cells differ from gemm_f16_pp3 (form %d), max |d| %g" % (
                    M, N, f16_out, padded, int(d.sum()), form, float(np.abs(got - tiled).max()))


def test_panel_in_engine(monkeypatch):
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=2, dec_layers=3, vocab=300)
    w = W.synth_weights(cfg, seed=19)
    w["predictor.out.bias"] = np.asarray([-0.2], np.float32)
    cmvn = W.synth_cmvn()
    lens = [16000 * 24, 16000 * 9, 16000 * 17, 4000, 16000 * 30, 16000 * 13] * 3
    audio = [W.synth_audio(n, 300 + u) for u, n in enumerate(lens)]
    out, counts = {}, {}
    for flag in ("0", "1"):
        monkeypatch.setenv("PF_GEMM_PANEL", flag)
        e = Engine(weights=W.pack_pfw(cfg, w), cmvn=cmvn, device=0)
        e.profile(True)
        e.recognize(audio, want_logits=True)
        e.profile_reset()
        out[flag] = e.recognize(audio, want_logits=True)
        kv, vocab = e.profile_kernel("gemm_dec_kv"), e.profile_kernel("gemm_vocab")
        counts[flag] = {c: e.profile_get(c)[1] for c in ("gemm_dec_kv", "gemm_vocab", "gemm_dec_ffn", "attn_cross", "dec_mid", "argmax")}
        assert counts[flag]["gemm_dec_kv"] == 1 and counts[flag]["gemm_vocab"] == 1, counts[flag]
        e.close()
        if flag == "1":
            assert kv.startswith(PANEL) and vocab.startswith(PANEL), (kv, vocab)
        else:
            assert kv.startswith("gemm_f16_pp3") and vocab.startswith("gemm_f16_pp3"), (kv, vocab)
    a, b = out["0"], out["1"]
    assert a.L == b.L
    np.testing.assert_array_equal(a.token_num, b.token_num)
    np.testing.assert_array_equal(a.token_ids, b.token_ids)
    assert np.array_equal(a.logits, b.logits), float(np.abs(a.logits - b.logits).max())
    assert counts["0"] == counts["1"], (counts["0"], counts["1"])


@pytest.mark.timeout(300)
def test_panel_beside_another_engine(eng):
    from aliparaformerasr_amd.engine import Engine
    cfgA = W.paraformer_large_config(enc_layers=2, dec_layers=1, timestamp_head=True)
    A = Engine(weights=W.pack_pfw(cfgA, W.synth_weights(cfgA, 1)), cmvn=W.synth_cmvn(), device=0)
    audio = [W.synth_audio(30 * 16000, u) for u in range(16)]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4000, 512)).astype(np.float32)
    wk = (rng.standard_normal((2048, 512)) / 22).astype(np.float32)
    wv = (rng.standard_normal((1236, 512)) / 22).astype(np.float32)
    ops = {
        "f16 result 4000 x 2048": lambda: eng.op_gemm_panel(x, wk, None, f16_out=True, form=7, padded=True),
        "fp32 result 4000 x 1236": lambda: eng.op_gemm_panel(x, wv, None, f16_out=False, form=7),
    }
    quiet = {name: f() for name, f in ops.items()}
    stop = []

    def disturb():
        while not stop:
            A.recognize(audio)
    th = threading.Thread(target=disturb)
    th.start()
    try:
        for name, f in ops.items():
            t0, n = time.time(), 0
            while time.time() - t0 < 1.0 or n < 4:
                y = f()
                n += 1
                assert np.array_equal(y, quiet[name]), "%s: run %d beside the busy engine differs from the quiet run by %.3g" % (
                    name, n, float(np.abs(y - quiet[name]).max()))
    finally:
        stop.append(1)
        th.join()
    A.close()
