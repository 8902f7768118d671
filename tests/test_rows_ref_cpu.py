"""CPU: tests/rows_ref.py against independent formulations, and the discriminating power of the streaming-seam cases.

  * ln_ref against torch's float64 layer_norm; the large-offset rows really are exact in fp32 and shift-invariant; ln_bound is
    void on them as they stand and small on x - x0; an fp32 emulation of the kernels' shifted two-pass form stays inside it;
  * fsmn_stream_ref against the conv1d form of oracle/online.py (cat(cache, tn * m) -> conv1d without padding), chunked
    against whole;
  * merge_replace against a first-index arg-max (np.argmax) and against om.argmax_last on the reversed row; every steered row
    of merge_case does what its class says;
  * add_to_f16: the double-rounding pairs separate the two-step definition from a one-step rounding;
  * the seam cases of tests/test_gpu_online.py: a cache rotated by one column, a mask applied one position late and a cache
    taken before masking each move a compared quantity by at least 10 x its tolerance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import rows_ref as R
from aliparaformerasr_amd import weights as W
from oracle import model as om
from oracle import online as oo


def test_ln_ref_is_layer_norm():
    for D in (4, 512, 560, 2048):
        x = R.ln_rows(9, D, 1)
        g, b = R.ln_params(D, 1)
        want = Fn.layer_norm(torch.from_numpy(x).double(), (D,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-12).numpy()
        assert np.abs(R.ln_ref(x, g, b) - want).max() < 1e-12


def _kernel_emulation(x, g, b):
    """the shifted two-pass form of layernorm_kernel in fp32 (summation order aside)"""
    x = np.asarray(x, np.float32)
    d = (x - x[:, :1]).astype(np.float32)
    mean = (d.sum(axis=1, keepdims=True, dtype=np.float32) / np.float32(x.shape[1])).astype(np.float32)
    e = (d - mean).astype(np.float32)
    var = ((e * e).sum(axis=1, keepdims=True, dtype=np.float32) / np.float32(x.shape[1])).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(1e-12))).astype(np.float32)
    return ((e * rstd).astype(np.float32) * g + b).astype(np.float32)


def test_large_offset_rows_are_exact_and_bounded():
    for D in (512, 560, 2048):
        x, kind = R.ln_cases(7, D, 3)
        assert list(kind[-3:]) == [1, 2, 1]
        off = x[kind == 1].astype(np.float64)
        d32 = (x[kind == 1] - x[kind == 1][:, :1]).astype(np.float32)
        assert (d32.astype(np.float64) == off - off[:, :1]).all()                       # x - x0 is exact in fp32
        assert (np.abs(off) <= 2 * np.abs(off[:, :1])).all() and (2 * np.abs(off) >= np.abs(off[:, :1])).all()
        g, b = R.ln_params(D, 3)
        ref, bnd = R.ln_expect(x, kind, g, b, half=False)
        assert np.abs(R.ln_ref(off, g, b) - ref[kind == 1]).max() < 1e-6               # shift-invariant
        assert R.ln_bound(off, g, b).min() > 1.0 and bnd[kind == 1].max() < 1e-2       # void as they stand, tight on x - x0
        got = _kernel_emulation(x, g, b)
        ratio = R.assert_ln(got, ref, bnd, "emulation D %d" % D)
        assert ratio < 1.0
        assert np.array_equal(got[kind == 2], np.broadcast_to(b, got[kind == 2].shape))   # a constant row: beta, bit for bit
        # the unshifted one-pass form is what these rows catch
        naive = ((x - x.mean(axis=1, keepdims=True, dtype=np.float32)) /
                 np.sqrt(x.var(axis=1, keepdims=True, dtype=np.float32) + np.float32(1e-12)) * g + b).astype(np.float32)
        with pytest.raises(AssertionError):
            R.assert_ln(naive, ref, bnd, "naive")


def test_posenc_reference_is_the_oracles_prologue():
    x = (np.random.default_rng(2).standard_normal((2, 9, 560)) * 3).astype(np.float32)
    g, b = R.ln_params(560, 2)
    ref, bnd = R.posenc_expect(x, g, b)
    pe = om.sinusoidal_pe(9, 560)
    v = torch.from_numpy(x) * float(np.sqrt(512.0)) + pe                                 # Oracle.forward's prologue, fp32
    want = om.layer_norm(v, torch.from_numpy(g), torch.from_numpy(b)).numpy().reshape(18, 560)
    assert (np.abs(want - ref) <= bnd).all()
    assert bnd.max() < 5e-3                                                              # f16 result: within an f16 ulp of |y| < 8
    for B, T in ((3, 7), (2, 83)):                                                       # the GPU cases feel a table read one row off
        xc = R.posenc_case(B, T, 4)
        ref, bnd = R.posenc_expect(xc, g, b)
        for pos in (0, 2):
            assert (np.abs(R.posenc_expect(xc, g, b, first_pos=pos)[0] - ref) / bnd).max() > 100


def _conv_form(tn, taps, lens, cache, x):
    tn, x = torch.from_numpy(tn).double(), torch.from_numpy(x).double()
    B, L, D = tn.shape
    mask = (torch.arange(L)[None, :] < torch.as_tensor(lens, dtype=torch.int64)[:, None]).double().unsqueeze(-1)
    t = tn * mask
    xc = torch.cat([torch.from_numpy(cache).double(), t.transpose(1, 2)], dim=2)
    y = Fn.conv1d(xc, torch.from_numpy(np.ascontiguousarray(taps.T)).double().unsqueeze(1), groups=D).transpose(1, 2)
    return (x + (y + t) * mask).numpy(), xc[:, :, -(taps.shape[0] - 1):].numpy()


@pytest.mark.parametrize("L", (1, 4, 10, 11, 25))
def test_fsmn_stream_ref_is_the_conv1d_form(L):
    for k in (11, 21):
        lens = (L, max(L - 3, 0), 0, L + 2)
        tn, taps, ln, cache, x = R.fsmn_stream_case(4, L, k, lens, 5, D=64)
        xo, co, bnd = R.fsmn_stream_ref(tn, taps, ln, cache, x)
        xw, cw = _conv_form(tn, taps, np.minimum(ln, L), cache, x)
        assert np.abs(xo - xw).max() < 1e-12
        assert np.array_equal(co, cw.astype(np.float32))
        valid = np.arange(L)[None, :] < ln[:, None]
        assert (bnd[valid] > 0).all() and (bnd[~valid] == 0).all() and np.array_equal(xo[~valid], x[~valid].astype(np.float64))


def test_fsmn_stream_ref_chains():
    tn, taps, ln, cache, x = R.fsmn_stream_case(2, 25, 11, (25, 25), 6, D=64)
    xo, co, _ = R.fsmn_stream_ref(tn, taps, ln, cache, x)
    c, at, parts = cache, 0, []
    for n in (4, 1, 10, 10):
        xp, c, _ = R.fsmn_stream_ref(tn[:, at: at + n], taps, (n, n), c, x[:, at: at + n])
        parts.append(xp); at += n
    assert np.array_equal(np.concatenate(parts, axis=1), xo) and np.array_equal(c, co)


def test_merge_rule_is_the_first_index_argmax():
    r = np.random.default_rng(7)
    for V in (1, 2, 5, 257):
        x = r.integers(0, 4, (400, V + 3)).astype(np.float32)                            # many ties; three pad columns
        x[:, V:] = 9
        for nobias in (0, V // 2, V - 1):
            first = np.argmax(x[:, :V], axis=1)
            assert np.array_equal(R.merge_replace(x, V, nobias), first != nobias)
            last_of_reversed = om.argmax_last(np.ascontiguousarray(x[:, :V][:, ::-1]))   # the reference's own scan, mirrored
            assert np.array_equal(V - 1 - last_of_reversed, first)
        assert R.merge_replace(x, V, -1).all() and R.merge_replace(x, V, V).all()


@pytest.mark.parametrize("V", (1, 255, 256, 257, 8404))
def test_merge_cases_are_steered(V):
    seen = set()
    for nobias in sorted({0, V // 2, V - 1, -1, V}):
        c = R.merge_case(V, nobias, 1)
        rule = R.merge_replace(c["dha"], V, nobias)
        assert np.array_equal(rule, c["want"]), [(k, w, g) for k, w, g in zip(c["cls"], c["want"], rule) if w != g]
        assert c["ld"] > V and c["ld"] % 4 == 0
        seen |= {(k, bool(w)) for k, w, s in zip(c["cls"], c["want"], c["steered"]) if s and 0 <= nobias < V}
        dha_ids, ids = np.arange(100, 100 + len(rule)), np.arange(len(rule))
        logits = np.full_like(c["dha"], -7.0)
        lo, io = R.merge_ref(c["dha"], dha_ids, V, nobias, True, logits, ids)
        assert np.array_equal(io, np.where(rule, dha_ids, ids)) and (lo[:, V:] == -7).all() and (lo[~rule] == -7).all()
        assert np.array_equal(R.bits(lo[rule][:, :V]), R.bits(c["dha"][rule][:, :V]))
    want = {("unique", False), ("bigger_pad", False), ("nan_nobias", True)}
    if V > 1:
        want |= {("tie_before", True), ("tie_after", False), ("bigger_last", True), ("nan_elsewhere", False), ("bigger_first", True)}
    assert want <= seen, want - seen


def test_add_to_f16_is_two_roundings():
    a, b = R.double_rounding_pairs(4096, 3)
    two = R.add_to_f16_ref(a, b)
    one = (a.astype(np.float64) + b.astype(np.float64)).astype(np.float16)
    assert (np.float32(a + b) == a).all()
    assert (two != one).mean() > 0.4 and np.isfinite(two.astype(np.float32)).all()
    assert (R.bits(two) & 1 == 0).all()                                                  # the even neighbour, whatever b's sign
    t, ids = np.arange(12, dtype=np.float32).reshape(3, 4), [0, 2, -1, 3, 1]
    assert np.array_equal(R.embed_ref(t, ids)[0], t[[0, 2, 0, 2, 1]])


# ---- the streaming seams: the cases of tests/test_gpu_online.py tell the three classic cache mistakes from the right answer
@pytest.fixture(scope="module")
def graphs():
    cfg = W.paraformer_large_config(enc_layers=3, dec_layers=3, vocab=300)
    w = W.synth_weights(cfg, seed=31)                                                    # the model of tests/test_gpu_online.py
    return oo.OnlineGraphs(om.Oracle(om.ModelConfig(**cfg), w, quant="fp16"))


def test_restated_decoder_is_the_oracles(graphs):
    enc = np.random.default_rng(1).standard_normal((3, 6, 512)).astype(np.float32)
    emb, lens, caches = R.online_decoder_inputs(11, (11, 3, 0), 3)
    a, b = graphs.decoder(enc, emb, lens, caches), R.online_decoder(graphs, enc, emb, lens, caches)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("L,lens", R.DEC_CASES)
def test_seam_cases_separate_the_mutations(graphs, L, lens):
    enc = np.random.default_rng(1).standard_normal((3, 6, 512)).astype(np.float32)
    emb, ln, caches = R.online_decoder_inputs(L, lens, 3)
    ref = R.online_decoder(graphs, enc, emb, ln, caches)
    for m in R.MUTATIONS:
        if m != "rotate" and not any(n < L for n in lens):
            continue                                                                     # no masked position: the mutation is the identity
        sep = R.separation(ref, R.online_decoder(graphs, enc, emb, ln, caches, m), ln)
        print("L %d lens %s %s: %.1f tolerances" % (L, lens, m, sep))
        assert sep >= 10, (L, lens, m, sep)
