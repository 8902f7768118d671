"""GPU: the kernels that are a layer — k_ffn.hip's decoder split forms ffn_fused_kernel<8, 0, 2, {0 | 2}, 0, {8, 4, 3, 2, 1}> with
ffn_dec_finish_kernel, its encoder forms with the out-projection in front ffn_fused_kernel<8, 0, 2, 1, {0 | 1}, 0>, k_decmid.hip
dec_mid_kernel<11>, k_norm.hip fsmn_dec_ln_kernel<11 | 21> — against the designs and the
float64 references of tests/layer_ref.py, launched through the stand-alone ops the way the pipeline launches them.  `steer`
demands the same bits up to and including t / x (and tn where it is exposed), the outputs behind the last LayerNorm and the
whole `normal` design the derived bound; every case asserts the kernel that ran (Engine.profile_kernel), is called twice and
must return the same bits.  The ops are hostile hosts (engine_ops.cpp): operand and residual rows behind M - 1 hold a large
finite pattern, the masked rows of tn too (pf_op_fsmn_dec_ln) and, between the split launch and the fused middle, the workspace rows of
every masked position (pf_op_dec_mid, form 0), every output is sentinel-filled and checked for unwritten
cells and for stores outside what kernels.h declares written (rows at or beyond M; columns [512, 520) of q), the bytes behind
ffn_dec_workspace_bytes are guarded, and a masked row of x must come back with the bits it went in with.
tests/test_layer_ref_cpu.py proves the designs' exactness claims and shows that these assertions reject fourteen wrong
implementations.

Measured on an MI355X (run with -s: one line per `normal` case, the worst per kernel and output at the end): all 58 tests
pass, every `steer` case bit-equal (t and x_out of the split block at every split count and equal across the five, x of the
encoder tail with and without residual and tail, x of the decoder middle in its three forms and equal across them, tn, x of
fsmn_dec_ln), no guard violation, every kernel name as expected; the file takes 4.7 s of wall time (engine set-up 1.7 s, the
slowest test 0.24 s).  No defect was found in a kernel; what the suite corrects is a statement: q of the fused middle kernel is
NOT bit-identical to q of the three launches it replaces (identical at L = 1 only, in the 17 `steer` cases printed below; x
is, and both q agree with the reference under the same bound) — DESIGN.md 4.1k said "bit-identical" on the strength of one
end-to-end run that compared log-probs to 5e-3.
(The hosts' poison was tried once against a deliberately wrong build — the input mask of dec_mid_kernel off by one row, every access
still in bounds: 15 of the 19 decoder-middle tests failed, the hostile workspace row reaching x.)
Worst |err| / bound, bounds derived in tests/layer_ref.py and not tuned:
    behind an exact x or t (the LayerNorm's own arithmetic and one f16 rounding):
        n of the finishing pass 0.0005 (fp32)    n16 of the encoder tail 0.687    xn16 of fsmn_dec_ln_kernel<11 | 21> 0.738 / 0.735,
        of the three-launch middle 0.738    q of dec_mid_kernel<11> 0.128, of the q GEMM behind the three launches 0.128
        Q | K | V of the encoder tail 0.131
    `normal`, M = 129, every split count:  t 0.0011 (0.0001 with the out-projection), n 0.0003, x_out 0.0017
        b1 = 16 (mean^2 / var = 249): t 0.0024, its constant row 0.0068;  b1 <= 0: t 0.0007, its all-zero row = beta_F W2^T exactly
    `normal`, encoder tail at (3, 83): x 0.0006, n16 0.0003, Q | K | V 0.00007
    `normal`, decoder middle at L = 37 / 70, all three forms: x 0.0002, q 0.079
(the chained `normal` bounds are worst cases over every summation order and every f16 value that may sit on a rounding boundary:
three orders of magnitude of room is their nature, layer_ref's docstring says why; 0.69 - 0.74 for an f16 LayerNorm result is
the half f16 ulp that is most of ln_bound(half=True), as in the GEMM suite.)  T = 5 is refused by launch_ffn_fused ("T >= 8", as
kernels.h documents; asserted below).  splits = 0 runs the form ffn_dec_splits names: 8 shares at M = 65 and 129.
"""
import numpy as np
import pytest

import layer_ref as LR
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

WORST = {}
SPLITS = (1, 2, 3, 4, 8)
MID, FDL = "dec_mid_kernel<11>", "fsmn_dec_ln_kernel<%d>"


def dec_kernel(out_proj, splits):
    return "ffn_fused_kernel<8, 0, 2, %d, 0, %d>" % (2 if out_proj else 0, LR.SHARE_CHUNKS[splits])


def ffn_dec_splits(M):
    """k_ffn.hip's rule, restated: the form with the shortest critical path on 256 compute units"""
    tiles = -(-M // 64)
    best, bt = 1, 1e30
    for cand, nch in zip(SPLITS, (8, 4, 3, 2, 1)):
        wgs = tiles * cand
        rounds = -(-wgs // 256)
        last = (wgs - (rounds - 1) * 256) / 256.0
        t = (17.0 + 4.3 * nch) * (rounds - 1 + (0.5 + 0.5 * last if rounds > 1 else 1.0)) + 1.2 * cand
        if t < bt - 0.5:
            bt, best = t, cand
    return best


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    w = W.synth_weights(cfg, seed=5)
    e = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    e.profile(True)
    yield e
    e.close()
    print("worst |err| / bound per kernel and output:", {k: "%.3g" % v for k, v in sorted(WORST.items())})


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


_CACHE = {}


def _dec(design, M, out_proj, special=None):
    """case, reference and bounds, computed once per shape and shared"""
    key = (design, M, out_proj, special)
    if key not in _CACHE:
        c = LR.make_dec_case(design, M, out_proj=out_proj, special=special)
        ref = LR.dec_reference(c)
        _CACHE[key] = (c, ref, LR.dec_bounds(c, ref) if design == "normal" else None)
    return _CACHE[key]


def _run_dec(eng, c, splits, expect):
    kw = dict(ln=c.ln, splits=splits, out_proj=c.out_proj)
    eng.profile_reset()
    out = eng.op_dec_ffn_fused(None if c.out_proj else c.a, c.w1, c.b1, (c.gf, c.bf), c.w2, **kw)
    ran = eng.profile_kernel("gemm_op")
    assert ran == expect, "M %d splits %d: ran %r, expected %r" % (c.M, splits, ran, expect)
    again = eng.op_dec_ffn_fused(None if c.out_proj else c.a, c.w1, c.b1, (c.gf, c.bf), c.w2, **kw)
    for a, b in zip(out, again):
        assert np.array_equal(a, b, equal_nan=True), "M %d splits %d: a second call returned other bits" % (c.M, splits)
    return out


# ---- the decoder split block
@pytest.mark.parametrize("out_proj", (False, True))
@pytest.mark.parametrize("M", (1, 63, 64, 65, 129))
def test_dec_block_steer(eng, M, out_proj):
    c, ref, _ = _dec("steer", M, out_proj)
    first = None
    for splits in SPLITS:
        what = "steer M %d out-projection %d splits %d" % (M, out_proj, splits)
        out = _run_dec(eng, c, splits, dec_kernel(out_proj, splits))
        LR.assert_exact(None, ref["t"], out[0], what + " t")
        if out_proj:
            LR.assert_exact(None, ref["x_out"], out[2], what + " x_out")
        r = LR.assert_bounded(ref["n"], LR.ln_bound(ref["t"], *c.ln), out[1], what + " n")
        _note("LayerNorm behind the finishing pass", r)
        first = first or out
        for a, b in zip(out, first):
            assert np.array_equal(a, b, equal_nan=True), what + ": differs from splits 1"


@pytest.mark.parametrize("M", (65, 129))
def test_dec_block_automatic_split_count(eng, M):
    for out_proj in (False, True):
        c, ref, _ = _dec("steer", M, out_proj)
        out = _run_dec(eng, c, 0, dec_kernel(out_proj, ffn_dec_splits(M)))
        LR.assert_exact(None, ref["t"], out[0], "steer M %d automatic splits t" % M)


@pytest.mark.parametrize("splits", SPLITS)
def test_dec_block_normal(eng, splits):
    out_proj = splits in (2, 4)
    c, ref, bnd = _dec("normal", 129, out_proj)
    what = "normal M 129 out-projection %d splits %d" % (out_proj, splits)
    out = _run_dec(eng, c, splits, dec_kernel(out_proj, splits))
    k = dec_kernel(out_proj, splits)
    rt = LR.ratio(ref["t"], bnd["t"], out[0], what + " t")
    rn = LR.ratio(ref["n"], bnd["n"], out[1], what + " n")
    print("%s [%s]: |err| / bound t %.3g, n %.3g" % (what, k, rt, rn))
    _note(k + " t", rt)
    _note(k + " n", rn)
    if out_proj:
        rx = LR.assert_bounded(ref["x_out"], bnd["x_out"], out[2], what + " x_out")
        print("%s: x_out %.3g" % (what, rx))
        _note(k + " x_out", rx)


@pytest.mark.parametrize("special", ("offset", "zero"))
def test_dec_block_degenerate_rows(eng, special):
    """b1 = 16: mean / std of the hidden = 16 (the conditioning of E[h^2] - mean^2), row 0 a constant hidden row (its variance
    comes out of the subtraction as rounding noise of either sign: the clamp is the code under test).  b1 <= 0: row 0 an all-zero
    hidden row, whose answer is exactly beta_F W2^T."""
    c, ref, bnd = _dec("normal", 9, False, special)
    for splits in (1, 3, 8):
        out = _run_dec(eng, c, splits, dec_kernel(False, splits))
        what = "normal (%s) splits %d" % (special, splits)
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), what
        r0 = LR.assert_bounded(ref["t"][:1], bnd["t"][:1], out[0][:1], what + " t, row 0")
        r = LR.assert_bounded(ref["t"][1:], bnd["t"][1:], out[0][1:], what + " t")
        print("%s: |err| / bound of t %.3g (row 0: %.3g), mean^2 / var %.0f" % (what, r, r0, float(np.median(bnd["rho"][1:]))))
        _note("t, %s rows" % special, r)
        _note("t, %s row 0" % special, r0)
        if special == "zero":
            assert np.array_equal(out[0][0], ref["d"].astype(np.float32)), what + ": an all-zero hidden row must give beta_F W2^T exactly"


# ---- the encoder tail: out-projection + FSMN + norm2 in front of the block, optionally the next layer's Q | K | V behind it
def enc_kernel(tail):
    return "ffn_fused_kernel<8, 0, 2, 1, %d, 0>" % int(tail)


def _run_enc(eng, c, ref, bnd, tail, what):
    args = (c.ctx, c.wo, c.bo, c.v, c.taps, c.T, c.ln2, c.w1, c.b1, c.w2, c.b2)
    kw = dict(resid=c.resid, ln=c.ln, qkv=(c.wqkv, c.bqkv) if tail else None)
    eng.profile_reset()
    out = eng.op_attn_ffn_fused(*args, **kw)
    assert eng.profile_kernel("gemm_op") == enc_kernel(tail), (what, eng.profile_kernel("gemm_op"))
    again = eng.op_attn_ffn_fused(*args, **kw)
    for a, b in zip(out, again):
        assert np.array_equal(a, b, equal_nan=True), what + ": a second call returned other bits"
    if c.design == "steer":
        LR.assert_exact(None, ref["x"], out[0], what + " x")
        rx = 0.0
    else:
        rx = LR.ratio(ref["x"], bnd["x"], out[0], what + " x")
    rn = LR.ratio(ref["n_raw"], bnd["n16"], out[1], what + " n16")
    rq = LR.ratio(ref["qkv"], bnd["qkv"], np.concatenate(out[2:], 1), what + " Q | K | V") if tail else 0.0
    for name, r in (("x", rx), ("n16", rn), ("Q | K | V", rq)):
        _note("%s %s (%s)" % (enc_kernel(tail), name, c.design), r)
    return out, (rx, rn, rq)


@pytest.mark.parametrize("B,T", ((8, 8), (7, 9), (5, 13), (2, 64), (1, 65), (3, 83)))
def test_enc_tail_steer(eng, B, T):
    for resid in (True, False):
        c = LR.make_enc_case("steer", B, T, resid)
        ref = LR.enc_reference(c)
        bnd = LR.enc_bounds(c, ref)
        outs = [_run_enc(eng, c, ref, bnd, tail, "steer B %d T %d residual %d tail %d" % (B, T, resid, tail))[0] for tail in (False, True)]
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "the tail changed x or n16"


def test_enc_tail_normal(eng):
    for resid in (True, False):
        c = LR.make_enc_case("normal", 3, 83, resid)
        ref = LR.enc_reference(c)
        bnd = LR.enc_bounds(c, ref)
        for tail in (False, True):
            what = "normal B 3 T 83 residual %d tail %d" % (resid, tail)
            _, r = _run_enc(eng, c, ref, bnd, tail, what)
            print("%s [%s]: |err| / bound x %.3g, n16 %.3g, Q | K | V %.3g" % ((what, enc_kernel(tail)) + r))


def test_enc_tail_refuses_utterances_shorter_than_its_window(eng):
    """kernels.h documents T >= 8 for the fused FSMN memory of FfnFusedArgs; the launcher must refuse T = 5, not compute it"""
    from aliparaformerasr_amd import _native as N
    c = LR.make_enc_case("steer", 8, 8, True)
    with pytest.raises(N.PfError, match="T >= 8"):
        eng.op_attn_ffn_fused(c.ctx[:60], c.wo, c.bo, c.v[:60], c.taps, 5, c.ln2, c.w1, c.b1, c.w2, c.b2, resid=c.resid[:60], ln=c.ln)


# ---- the decoder middle
def _mid(design, L, tok):
    key = ("mid", design, L, tok)
    if key not in _CACHE:
        c = LR.make_mid_case(design, 3, L, tok)
        dref = LR.dec_reference(c.dec)
        ref = LR.mid_reference(c, dref["t"])
        bt = LR.dec_bounds(c.dec, dref)["t"] if design == "normal" else None
        _CACHE[key] = (c, ref, LR.mid_bounds(c, ref, bt))
    return _CACHE[key]


def _run_mid(eng, c, splits, form):
    d = c.dec
    args = (d.a, d.w1, d.b1, (d.gf, d.bf), d.w2, c.n2, c.taps, c.token_num, c.x, c.n3, c.wq, c.bq)
    S = splits or ffn_dec_splits(c.B * c.L)
    eng.profile_reset()
    out = eng.op_dec_mid(*args, splits=splits, form=form)
    assert out["ran"], "form %d declined B %d L %d" % (form, c.B, c.L)
    assert eng.profile_kernel("gemm_op") == dec_kernel(False, S), (form, splits, eng.profile_kernel("gemm_op"))
    if form < 2:
        assert eng.profile_kernel("gemm_op_mid") == (MID if form == 0 else FDL % 11), eng.profile_kernel("gemm_op_mid")
    again = eng.op_dec_mid(*args, splits=splits, form=form)
    for k in ("x", "q", "tn", "xn16"):
        assert (out[k] is None and again[k] is None) or np.array_equal(out[k], again[k], equal_nan=True), "form %d: a second call returned other %s" % (form, k)
    return out


MID_RUNS = [(L, tok, 0) for L, tok in LR.MID_CASES] + [(37, LR.MID_CASES[5][1], s) for s in (1, 3, 8)]


@pytest.mark.parametrize("L,tok,splits", MID_RUNS)
def test_dec_mid_steer(eng, L, tok, splits):
    c, ref, bnd = _mid("steer", L, tok)
    outs = []
    for form in (0, 1, 2):
        what = "steer L %d token_num %s splits %d form %d" % (L, tok, splits, form)
        out = _run_mid(eng, c, splits, form)
        _, rq = LR.check_mid(c, ref, bnd, out["x"], out["q"], what, exact_x=True)
        _note(("dec_mid_kernel<11>" if form == 0 else "three launches") + " q (steer)", rq)
        if form:
            valid = (np.arange(L)[None, :] < np.asarray(tok)[:, None]).reshape(-1)
            LR.assert_exact(None, ref["tn"][valid], out["tn"][valid], what + " tn")
            _note("xn16, form %d" % form, LR.assert_bounded(ref["xn_raw"], bnd["xn16"], out["xn16"], what + " xn16"))
        outs.append(out)
    assert np.array_equal(outs[0]["x"], outs[1]["x"]) and np.array_equal(outs[0]["x"], outs[2]["x"])
    assert np.array_equal(outs[1]["q"], outs[2]["q"]) and np.array_equal(outs[1]["xn16"], outs[2]["xn16"]), "forms 1 and 2 run the same arithmetic"
    print("L %d token_num %s splits %d: q of the fused kernel and of the three launches bit-identical: %s"
          % (L, tok, splits, bool(np.array_equal(outs[0]["q"], outs[1]["q"]))))


@pytest.mark.parametrize("L,tok", (LR.MID_CASES[5], LR.MID_CASES[13]))
def test_dec_mid_normal(eng, L, tok):
    c, ref, bnd = _mid("normal", L, tok)
    for form in (0, 1, 2):
        what = "normal L %d token_num %s form %d" % (L, tok, form)
        out = _run_mid(eng, c, 0, form)
        rx, rq = LR.check_mid(c, ref, bnd, out["x"], out["q"], what, exact_x=False)
        print("%s: |err| / bound x %.3g, q %.3g" % (what, rx, rq))
        name = "dec_mid_kernel<11>" if form == 0 else "three launches, form %d" % form
        _note(name + " x", rx)
        _note(name + " q", rq)


# ---- fsmn_dec_ln_kernel alone
@pytest.mark.parametrize("k", (11, 21))
@pytest.mark.parametrize("L", LR.FDL_L)
def test_fsmn_dec_ln(eng, L, k):
    for i in range(3):
        tok = tuple(int(v) for v in LR.token_nums(L, i + L))
        c = LR.make_fdl_case(3, L, k, tok)
        ref = LR.fdl_reference(c)
        what = "fsmn_dec_ln L %d k %d token_num %s" % (L, k, tok)
        eng.profile_reset()
        x, xn = eng.op_fsmn_dec_ln(c.tn, c.taps, c.token_num, c.x, c.ln)
        assert eng.profile_kernel("gemm_op") == FDL % k, eng.profile_kernel("gemm_op")
        LR.assert_exact(None, ref["x"], x.reshape(-1, 512), what + " x")
        _note(FDL % k + " xn16", LR.assert_bounded(ref["xn"], ref["bxn"], xn.reshape(-1, 512), what + " xn16"))
        x2, xn2 = eng.op_fsmn_dec_ln(c.tn, c.taps, c.token_num, c.x, c.ln)
        assert np.array_equal(x2, x, equal_nan=True) and np.array_equal(xn2, xn, equal_nan=True), what + ": a second call returned other bits"
