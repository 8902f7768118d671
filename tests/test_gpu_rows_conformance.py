"""GPU: the row kernels — csrc/k_norm.hip (layernorm_kernel<NV, POSENC>, layernorm512_kernel<2> without a pair,
layernorm_f16_kernel<NV>) and the non-CIF half of csrc/k_misc.hip (fsmn_dec_stream_kernel, embed_gather_kernel,
add_to_f16_kernel, seaco_merge_kernel) — each launcher alone through a thin stand-alone op (engine_ops.cpp: op_layernorm_ex,
op_layernorm_f16, op_fsmn_dec_stream, op_embed_gather, op_add_to_f16, op_seaco_merge) against the float64 definitions and the
derived bounds of tests/rows_ref.py.  The ops add no arithmetic; every result comes back inside its canary-filled buffer (two
guard rows at either end, guard columns where the row stride is wider than the result), so a store outside the result shows
here, not in the op.  tests/test_rows_ref_cpu.py checks the definitions against independent formulations.

What is visited: the dispatch edge of ln_dispatch (D = 512 at 4095 | 4096 | 4097 rows: the generic kernel, the two-row kernel,
the two-row kernel with its clamped second row, whose store would land in the guard row) in the three result forms; every
width class of the generic kernel down to D = 4, with the K-pad columns [560, 576) and a pad wider than a wavefront; rows whose
offset is a million times their spread and constant rows; the position-encoding form against the oracle's table at B > 1; the
f16 LayerNorm in place and out of place; the streaming FSMN at L = 1 .. 25 (at L >= 10 the whole cache comes from the new
positions) with full, ragged, empty and over-long streams, chained across four calls; every branch of the merge rule with
steered ties at V = 1 .. 8404; the gather at both clamped ends.

Measured (one run of this file with -s on an MI355X, at the commit that adds it, on top of ed968dc; the fixture prints the table when
it closes): 73 tests pass in 3 s, the largest (4095 rows, fp32, first call) 0.1 s; every guard cell canary, every pad column of an
f16 operand zero, every bit-exact comparison equal (constant rows = beta, cache_out, masked rows of x, the chained FSMN against
the single call in x and in the final cache, in place against out of place, batch against utterance alone, the merge at every
row class, the gather, f16(fl32(a + b)) on the double-rounding pairs), every repeated call the same bytes.  Worst |err| / bound,
bounds derived in tests/rows_ref.py and gemm_ref.ln_bound, not tuned:
    launch_layernorm, fp32 result     layernorm512_kernel<2>: random rows 0.002, large-offset rows 0.000 (4096 and 4097 rows)
                                      layernorm_kernel: D = 4 0.027 (large-offset 0.015), D = 512 0.002, 560 0.001, 2048 0.000
    launch_layernorm, f16 result      layernorm512_kernel<2> 0.643 (large-offset 0.615); layernorm_kernel D = 4 0.887, 512 0.662,
                                      560 0.637, 2048 0.323
    launch_posenc_ln_tab (f16)        0.654
    launch_layernorm_f16              0.952
    launch_fsmn_dec_stream, x         k = 11: 0.187, k = 21: 0.091
Every ratio above 0.5 belongs to an f16 result and sits against one term of the bound, the rounding of the result itself,
2^-11 |y|: a value just above a power of two is rounded by up to half an f16 ulp, 2^-11 of that power, so the term is reached to
within the share of |y| above it (0.95 at |y| = 1.05 2^e).  The fp32 results of the same launches show what the arithmetic in
front of that rounding uses of its bound: 0.03 at most.

Found in the kernels: no defect.  One property the definition had to learn from the kernel: a masked position enters xc and
cache_out as +0 (fsmn_dec_stream_kernel selects 0.f), where the graph's tn * mask gives -0 for a negative tn; the two are the same
number to every consumer, and csrc/kernels.h now says which one is stored."""
import functools

import numpy as np
import pytest

import rows_ref as R
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=5)), cmvn=W.synth_cmvn(), device=0)
    assert (e.OP_GUARD_ROWS, e.OP_CANARY32, e.OP_CANARY16) == (R.OP_GUARD_ROWS, R.CANARY32, R.CANARY16)
    yield e
    e.close()
    print("worst |err| / bound per kernel and output form:")
    for k, v in sorted(R.LOG.items()):
        print("    %-64s %.3f" % (k, v))


def h2f(u16):
    return np.ascontiguousarray(u16).view(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------ launch_layernorm
@functools.lru_cache(maxsize=None)
def _ln_case(rows, D):
    x, kind = R.ln_cases(rows, D, 11)
    g, b = R.ln_params(D, 11)
    return x, kind, g, b, R.ln_expect(x, kind, g, b, half=False), R.ln_expect(x, kind, g, b, half=True)


def _check_ln(eng, rows, D, form, ld16=0, ld32=0, key=None):
    x, kind, g, b, e32, e16 = _ln_case(rows, D)
    want16, want32 = form in ("f16", "both"), form in ("fp32", "both")
    o16, o32 = eng.op_layernorm_ex(x, g, b, want16, want32, ld16, ld32)
    what = "layernorm D %d rows %d %s" % (D, rows, form)
    assert (o16 is None) == (not want16) and (o32 is None) == (not want32)
    if want32:
        R.assert_guards(o32, rows, D, what + " fp32")                     # a wider ld32: the kernel leaves [D, ld32) alone
    if want16:
        R.assert_guards(o16, rows, D, what + " f16", pad=0)               # ... and zeroes [D, ld16) of the f16 operand, all of it
    for name, sub in (("random", kind == 0), ("large-offset", kind != 0)):   # noted apart (a constant row: bound 0, equality)
        if not sub.any():
            continue
        tag = "%s D = %d, %s rows" % (key, D, name)
        if want32:
            R.note(tag + ", fp32", R.assert_ln(R.body(o32, rows, D)[sub], e32[0][sub], e32[1][sub], what + " fp32"))
        if want16:
            R.note(tag + ", f16", R.assert_ln(h2f(R.body(o16, rows, D))[sub], e16[0][sub], e16[1][sub], what + " f16"))
    const = kind == 2
    if const.any():                                                       # beta, bit for bit
        if want32:
            assert np.array_equal(R.bits(R.body(o32, rows, D)[const]), R.bits(np.broadcast_to(b, (int(const.sum()), D))))
        if want16:
            assert np.array_equal(R.body(o16, rows, D)[const], np.broadcast_to(R.bits(R.f16(b)), (int(const.sum()), D)))
    p16, p32 = eng.op_layernorm_ex(x, g, b, want16, want32, ld16, ld32)   # twice: the same bytes
    assert (not want16 or np.array_equal(p16, o16)) and (not want32 or np.array_equal(R.bits(p32), R.bits(o32)))
    return o16, o32


@pytest.mark.parametrize("form", ("fp32", "f16", "both"))
@pytest.mark.parametrize("rows", (4095, 4096, 4097))
def test_layernorm_dispatch_edge(eng, rows, form):
    """4095: layernorm_kernel<2, false>; 4096: layernorm512_kernel<2>, every wave two rows; 4097: its last wave holds row 4096
    twice (the second clamped to rows - 1) and must store it once — the guard row behind it stays canary"""
    _, kind, _, _, _, _ = _ln_case(rows, 512)
    assert list(kind[-3:]) == [1, 2, 1]
    _check_ln(eng, rows, 512, form, key="layernorm512_kernel<2>" if rows >= 4096 else "layernorm_kernel")


def test_layernorm_dispatch_edge_agrees_across_the_seam(eng):
    """the two kernels on the same 4095 rows: within the sum of their bounds (their FMA contraction differs: not bitwise)"""
    x, kind, g, b, e32, _ = _ln_case(4096, 512)
    big = R.body(eng.op_layernorm_ex(x, g, b, False, True)[1], 4096)
    small = R.body(eng.op_layernorm_ex(x[:4095], g, b, False, True)[1], 4095)
    assert (np.abs(big[:4095].astype(np.float64) - small) <= 2 * e32[1][:4095]).all()


@pytest.mark.parametrize("D", (4, 512, 560, 2048))
@pytest.mark.parametrize("rows", (1, 3, 4, 5, 37))
def test_layernorm_generic_widths(eng, rows, D):
    ld16 = 576 if D == 560 else D
    o16, _ = _check_ln(eng, rows, D, "both", ld16=ld16, ld32=D + 8, key="layernorm_kernel")
    assert o16.shape[1] == ld16
    if D == 560:                                                          # a pad wider than a wavefront: every column of it is zeroed
        _check_ln(eng, rows, D, "f16", ld16=704, key="layernorm_kernel")
    _check_ln(eng, rows, D, "fp32", key="layernorm_kernel")
    _check_ln(eng, rows, D, "f16", ld16=ld16, key="layernorm_kernel")


# ------------------------------------------------------------------------------------------------ launch_posenc_ln_tab
@pytest.mark.parametrize("B,T", ((1, 1), (3, 7), (2, 83)))
def test_posenc_ln_tab(eng, B, T):
    x = R.posenc_case(B, T, 4)
    g, b = R.ln_params(560, 4)
    ref, bnd = R.posenc_expect(x, g, b)
    o16, o32 = eng.op_layernorm_ex(x, g, b, True, False, 576, 0, posenc_T=T)
    assert o32 is None
    what = "posenc_ln_tab B %d T %d" % (B, T)
    R.assert_guards(o16, B * T, 560, what, pad=0)
    R.note("layernorm_kernel<3, true> (posenc_ln_tab), f16", R.assert_ln(h2f(R.body(o16, B * T, 560)), ref, bnd, what))
    for u in range(B if B > 1 else 0):                                    # row % T: an utterance alone = its rows in the batch
        alone = eng.op_layernorm_ex(x[u: u + 1], g, b, True, False, 576, 0, posenc_T=T)[0]
        assert np.array_equal(R.body(alone, T), R.body(o16, B * T)[u * T: (u + 1) * T]), (what, u)


# ------------------------------------------------------------------------------------------------ launch_layernorm_f16
@pytest.mark.parametrize("D", (8, 1024, 2048))
@pytest.mark.parametrize("rows", (1, 4, 5, 37))
def test_layernorm_f16(eng, rows, D):
    x = R.f16(R.ln_rows(rows, D, 12))
    x[rows - 1] = np.float16(-3.140625)                                   # a constant row
    kind = np.zeros(rows, np.int32)
    kind[rows - 1] = 2
    g, b = R.ln_params(D, 12)
    ref, bnd = R.ln_expect(x.astype(np.float64), kind, g, b, half=True)
    out = eng.op_layernorm_f16(x, g, b, in_place=False)
    what = "layernorm_f16 D %d rows %d" % (D, rows)
    R.assert_guards(out, rows, D, what)
    got = h2f(R.body(out, rows))
    if rows > 1:
        R.note("layernorm_f16_kernel, f16 in and out", R.assert_ln(got[:-1], ref[:-1], bnd[:-1], what))
    assert np.array_equal(R.body(out, rows)[-1], R.bits(R.f16(b))), what + ": a constant row is f16(beta)"
    assert np.array_equal(eng.op_layernorm_f16(x, g, b, in_place=True), out), what + ": in place"
    assert np.array_equal(eng.op_layernorm_f16(x, g, b, in_place=False), out)


# ------------------------------------------------------------------------------------------------ launch_fsmn_dec_stream
def _lens(B, L):
    return (L,) if B == 1 else (L + 2, (L + 1) // 2, 0)                   # full | above L (counts as L), ragged, nobody


def _check_stream(eng, case, what):
    tn, taps, lens, cache, x = case
    B, L, D = tn.shape
    k = taps.shape[0]
    xo, co = eng.op_fsmn_dec_stream(tn, taps, lens, cache, x)
    R.assert_guards(xo, B * L, D, what + " x")
    R.assert_guards(co, B * D, k - 1, what + " cache_out")
    xr, cr, bnd = R.fsmn_stream_ref(tn, taps, lens, cache, x)
    got = R.body(xo, B * L).reshape(B, L, D)
    ratio = R.assert_ln(got.reshape(B * L, D), xr.reshape(B * L, D), bnd.reshape(B * L, D), what)
    masked = np.arange(L)[None, :] >= np.asarray(lens)[:, None]
    assert np.array_equal(R.bits(got[masked]), R.bits(x[masked])), what + ": a masked row of x changed"
    cg = R.body(co, B * D).reshape(B, D, k - 1)
    bad = np.argwhere(R.bits(cg) != R.bits(cr))
    assert not len(bad), "%s: cache_out%s holds %r, want %r" % (what, tuple(bad[0]), cg[tuple(bad[0])], cr[tuple(bad[0])])
    return ratio, got, cg


@pytest.mark.parametrize("L", (1, 4, 10, 11, 25))
@pytest.mark.parametrize("B", (1, 3))
def test_fsmn_dec_stream(eng, B, L):
    for zero in (False, True):
        case = R.fsmn_stream_case(B, L, 11, _lens(B, L), 21, zero_cache=zero)
        ratio, _, co = _check_stream(eng, case, "fsmn_dec_stream B %d L %d%s" % (B, L, " zero cache" if zero else ""))
        R.note("fsmn_dec_stream_kernel k = 11, x", ratio)
        if L >= 10 and not zero:                                          # the whole cache comes from the new positions
            assert np.array_equal(co[0], case[0][0, L - 10:].T)


def test_fsmn_dec_stream_k21(eng):
    ratio, _, _ = _check_stream(eng, R.fsmn_stream_case(3, 11, 21, _lens(3, 11), 22), "fsmn_dec_stream k 21")
    R.note("fsmn_dec_stream_kernel k = 21, x", ratio)


def test_fsmn_dec_stream_chained(eng):
    """25 tokens as chunks of 4, 1, 10 and 10 with carried caches = the single call, bit for bit: an output's K products are
    summed in the same order wherever the chunk borders fall"""
    tn, taps, _, cache, x = R.fsmn_stream_case(2, 25, 11, (25, 25), 23)
    _, whole, cwhole = _check_stream(eng, (tn, taps, np.asarray((25, 25), np.int32), cache, x), "fsmn_dec_stream whole")
    c, at = cache, 0
    for n in (4, 1, 10, 10):
        part = (np.ascontiguousarray(tn[:, at: at + n]), taps, np.asarray((n, n), np.int32), c, np.ascontiguousarray(x[:, at: at + n]))
        _, got, c = _check_stream(eng, part, "fsmn_dec_stream chunk at %d" % at)
        assert np.array_equal(R.bits(got), R.bits(whole[:, at: at + n])), "chunk of %d at %d" % (n, at)
        at += n
    assert np.array_equal(R.bits(c), R.bits(cwhole))


# ------------------------------------------------------------------------------------------------ launch_seaco_merge
@pytest.mark.parametrize("copy_logits", (False, True))
@pytest.mark.parametrize("V", (1, 255, 256, 257, 8404))
def test_seaco_merge(eng, V, copy_logits):
    for nobias in sorted({0, V // 2, V - 1, -1, V}):
        c = R.merge_case(V, nobias, 1)                                    # (what each row class must do: tests/test_rows_ref_cpu.py)
        rows, ld = c["dha"].shape
        r = np.random.default_rng([V, nobias + 9])
        logits = r.standard_normal((rows, ld)).astype(np.float32)
        ids, dha_ids = r.integers(0, V, rows), r.integers(1 << 40, 1 << 41, rows)
        lo, io = eng.op_seaco_merge(c["dha"], dha_ids, V, nobias, copy_logits, logits, ids)
        what = "seaco_merge V %d nobias %d copy %d" % (V, nobias, copy_logits)
        R.assert_guards(lo, rows, None, what + " logits")
        R.assert_guards(io, rows, None, what + " ids")
        lr, ir = R.merge_ref(c["dha"], dha_ids, V, nobias, copy_logits, logits, ids)
        got = R.body(io, rows).view(np.int64)
        bad = np.argwhere(got != ir)
        assert not len(bad), "%s: row %d (%s) %s" % (what, bad[0][0], c["cls"][bad[0][0]], "kept" if c["want"][bad[0][0]] else "was replaced")
        assert np.array_equal(R.bits(R.body(lo, rows)), R.bits(lr)), what + ": logits (pad columns and kept rows keep their bits)"


# ------------------------------------------------------------------------------------------------ embed_gather, add_to_f16
@pytest.mark.parametrize("rows", (1, 10, 130))
def test_embed_gather(eng, rows):
    vocab, D = 97, 512
    r = np.random.default_rng(rows)
    table = r.standard_normal((vocab, D)).astype(np.float32)
    edge = (0, vocab - 1, -1, vocab, -(1 << 31), (1 << 31) - 1)
    sets = [[e] for e in edge] if rows == 1 else [list(edge) + list(r.integers(-3, vocab + 3, rows - len(edge)))]
    for ids in sets:
        o32, o16 = eng.op_embed_gather(table, ids, want16=True)
        w32, w16 = R.embed_ref(table, ids)
        R.assert_guards(o32, rows, D, "embed_gather fp32")
        R.assert_guards(o16, rows, D, "embed_gather f16")
        assert np.array_equal(R.bits(R.body(o32, rows)), R.bits(w32)) and np.array_equal(R.body(o16, rows), R.bits(w16)), ids[:6]
        p32, p16 = eng.op_embed_gather(table, ids, want16=False)          # the SeACo fp32 graph's call: no f16 copy
        assert p16 is None and np.array_equal(R.bits(p32), R.bits(o32))


@pytest.mark.parametrize("rows", (1, 10, 130))
def test_add_to_f16(eng, rows):
    D = 512
    r = np.random.default_rng(rows + 50)
    a = (r.standard_normal((rows, D)) * 10.0 ** r.uniform(-3, 3, (rows, 1))).astype(np.float32)
    b = (r.standard_normal((rows, D)) * 10.0 ** r.uniform(-3, 3, (rows, 1))).astype(np.float32)
    a[0, :256], b[0, :256] = R.double_rounding_pairs(256, rows)           # f16(fl32(a + b)), not f16(a + b)
    a[-1, -4:], b[-1, -4:] = (65504, 65519, 65520, -1e9), (0, 0, 0, 0)    # the largest f16, the last value below the overflow, inf
    out = eng.op_add_to_f16(a, b)
    R.assert_guards(out, rows, D, "add_to_f16")
    with np.errstate(over="ignore"):
        want = R.add_to_f16_ref(a, b)
    assert np.array_equal(R.body(out, rows), R.bits(want))
