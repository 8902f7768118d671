"""GPU: the attention kernels (csrc/k_attn.hip attn_kernel<4,2> / <8,2>; csrc/k_fp32.hip attn_f32_mfma_kernel, its (hi | lo')
pair output and the one-query-per-workgroup attn_f32_kernel) against the float64 reference and the exact-answer designs of
tests/attn_ref.py, launched through pf_op_attention_ex the way the pipeline launches them: packed q | k | v rows,
interleaved K | V, the blocked Q | K matrix with utterances that start inside a 32-row block, shared K | V with one, two
or five keys, both workgroup forms, the narrow store path, the range output.  Every operand buffer is NaN except its
valid elements and every case checks that nothing outside [B, Lq, Dm] was stored, that no NaN came back and that a second
call returns the same bits.  tests/test_attn_ref_cpu.py shows that the same assertion rejects nine wrong attentions.

Measured on an MI355X (run with -s: one line per case, the worst per kind at the end), against bounds that are derived in
tests/attn_ref.py, not tuned: worst |err| / bound 0.322 for kind 0 (f16 kernel), 0.068 for kind 1 (fp32) and 0.068 for
kind 2 (pair).  form = 4 and form = 8 returned identical bits in every one of the 52 kind-0 cases.

One finding, fixed in k_fp32.hip: the pair epilogue of attn_f32_mfma_kernel was contracted to fma(oacc, inv, -hi), so lo'
was taken from the unrounded product and carried bits below the last place of the fp32 value; hi + lo' 2^-11 was then not
an fp32 number and the pair differed from the split of the fp32 kernel's result (found by uniform, layout 1, B 3, H 4,
T 65: lo' != f16((value - hi) 2^11)).  With the contraction off the pair is the split of kind 1's output bit for bit, which
test_fp32_kernels now also asserts.  hi == f16(value) holds except at exact ties, see the comment there."""
import numpy as np
import pytest

import attn_ref as R
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

WORST = {0: 0.0, 1: 0.0, 2: 0.0}


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    w = W.synth_weights(cfg, seed=5)
    e = Engine(weights=W.pack_pfw(cfg, w), cmvn=W.synth_cmvn(), device=0)
    yield e
    e.close()
    print("worst |err| / bound per kind:", {k: "%.3f" % v for k, v in WORST.items()})


def _launch(eng, c, kind, layout, shared=False, o_ld=0, form=0, want_range=False):
    Dm = c.heads * 128
    kw = dict(ldkv=4 * Dm, kv_off=2 * Dm) if layout == 2 else {}
    return eng.op_attention_ex(c.q, c.k, c.v, c.heads, kind=kind, layout=layout, shared_kv=shared, o_ld=o_ld, form=form,
                               want_range=want_range, **kw)


def _check(eng, design, kind, layout, B, H, Lq, Lk, shared=False, o_ld=0, form=0):
    c = R.make_case(design, B, H, Lq, Lk, shared)
    ref = R.case_ref(design, B, H, Lq, Lk, shared, kind=kind)
    what = "%s kind %d layout %d B %d H %d Lq %d Lk %d form %d" % (design, kind, layout, B, H, Lq, Lk, form)
    r = _launch(eng, c, kind, layout, shared, o_ld, form)
    assert r["ran"]
    ratio = R.assert_conforms(c, ref, kind, r["raw"], what)
    print("%s: |err| / bound = %.3f" % (what, ratio))
    WORST[kind] = max(WORST[kind], ratio)
    # the fp32 value the op hands back is the buffer's
    val, _ = R.unpack_raw(r["raw"], kind, B, Lq, H * 128)
    assert np.array_equal(r["out"].astype(np.float64), val)
    again = _launch(eng, c, kind, layout, shared, o_ld, form)
    assert np.array_equal(again["raw"], r["raw"]), what + ": a second call returned other bits"
    return r


# ---- the f16 kernel: (design, layout, B, H, Lq, Lk, shared, o_ld), each in both workgroup forms
def _kind0_cases():
    cases = []
    other = ("uniform", "stress", "random")
    bh = ((1, 4), (3, 4), (3, 2), (1, 2))
    for i, (Lq, Lk) in enumerate(R.CROSS_SHAPES):              # contiguous and interleaved K | V
        B, H = bh[i % 4]
        cases.append(("select", (0, 2)[i % 2], B, H, Lq, Lk, False, 0))
        cases.append((other[i % 3], (2, 0)[i % 2], B, H, Lq, Lk, False, 0))
    for i, T in enumerate(R.SELF_T):                           # packed q | k | v rows
        B, H = bh[(i + 1) % 4]
        cases.append((R.DESIGNS[i % 4], 1, B, H, T, T, False, 0))
    cases.append(("select", 1, 3, 4, 257, 257, False, 0))
    for T in R.BLOCKED_T:                                      # blocked Q | K: utterances 1, 2 start inside a 32-row block
        for design in R.DESIGNS:
            cases.append((design, 3, 3, 4, T, T, False, 0))
    for i, Lk in enumerate(R.SHARED_LK):                       # one K | V for every utterance (batch stride 0)
        cases.append(("select", (0, 2)[i % 2], 4, 4, 33, Lk, True, 0))
        cases.append(("uniform", (2, 0)[i % 2], 4, 4, 33, Lk, True, 0))
    for design in ("select", "uniform"):                       # o_rstride % 8 != 0: the narrow stores
        cases.append((design, 0, 3, 4, 33, 65, False, 516))
        cases.append((design, 1, 1, 2, 129, 129, False, 260))
    return cases


@pytest.mark.parametrize("design,layout,B,H,Lq,Lk,shared,o_ld", _kind0_cases())
def test_f16_kernel_in_both_forms(eng, design, layout, B, H, Lq, Lk, shared, o_ld):
    r4 = _check(eng, design, 0, layout, B, H, Lq, Lk, shared, o_ld, form=4)
    r8 = _check(eng, design, 0, layout, B, H, Lq, Lk, shared, o_ld, form=8)
    # a wave owns the same 32 queries and walks the same tiles in the same order in both forms
    assert np.array_equal(r4["raw"], r8["raw"]), "form 4 and form 8 differ"
    # form 0 picks one of the two
    assert np.array_equal(_launch(eng, R.make_case(design, B, H, Lq, Lk, shared), 0, layout, shared, o_ld)["raw"], r4["raw"])


@pytest.mark.parametrize("form", (4, 8))
@pytest.mark.parametrize("sign,layout,B,H,Lq,Lk,o_ld", ((1, 0, 3, 4, 300, 129, 0), (-1, 0, 3, 4, 300, 129, 0), (0, 0, 3, 4, 300, 129, 0),
                                                        (0, 1, 3, 2, 65, 65, 260)))
def test_range_output(eng, form, sign, layout, B, H, Lq, Lk, o_ld):
    """{min, max} per workgroup of the values as stored, 0 included; the consumer folds 256 pairs whatever the grid was."""
    c = R.make_case("select", B, H, Lq, Lk, False, sign)
    r = _launch(eng, c, 0, layout, o_ld=o_ld, form=form, want_range=True)
    R.assert_conforms(c, R.case_ref("select", B, H, Lq, Lk, False, sign), 0, r["raw"], "range")
    out, pairs = r["out"], r["range"]
    assert np.isfinite(pairs).all()
    want = (min(0.0, float(out.min())), max(0.0, float(out.max())))
    assert (float(pairs[:, 0].min()), float(pairs[:, 1].max())) == want
    assert (want[0] < 0) == (sign != 1) and (want[1] > 0) == (sign != -1)
    assert (pairs[:, 0] <= 0).all() and (pairs[:, 1] >= 0).all()
    grid = -(-Lq // (32 * form)) * B * H
    assert grid <= 256 and int(((pairs[:, 0] == 0) & (pairs[:, 1] == 0)).sum()) >= 256 - grid
    assert np.array_equal(r["raw"], _launch(eng, c, 0, layout, o_ld=o_ld, form=form)["raw"])      # the range costs the result nothing


# ---- the fp32 kernels: (design, layout, B, H, Lq, Lk, shared)
def _fp32_cases():
    cases = []
    shapes = ((1, 4, 1, 1), (3, 4, 33, 65), (3, 2, 129, 128), (1, 2, 257, 193), (1, 4, 97, 2), (3, 4, 160, 129),
              (1, 4, 31, 63), (3, 2, 128, 127))
    for i, (B, H, Lq, Lk) in enumerate(shapes):
        layout = i % 3
        cases.append((R.DESIGNS[i % 4], layout, B, H, Lk if layout == 1 else Lq, Lk, False))
    cases.append(("select", 2, 4, 4, 33, 5, True))
    cases.append(("uniform", 0, 4, 4, 33, 1, True))
    return cases


@pytest.mark.parametrize("kind", (1, 2))
@pytest.mark.parametrize("design,layout,B,H,Lq,Lk,shared", _fp32_cases())
def test_fp32_kernels(eng, kind, design, layout, B, H, Lq, Lk, shared):
    r = _check(eng, design, kind, layout, B, H, Lq, Lk, shared)
    if kind == 2:
        # the pair is (hi, lo') of ONE fp32 value: hi = f16(value), lo' = f16((value - hi) * 2^11)
        Dm, raw = H * 128, r["raw"]
        hi, lo = raw[:B * Lq, :Dm].view(np.float16), raw[:B * Lq, Dm:2 * Dm].view(np.float16)
        value = r["out"].reshape(B * Lq, Dm)
        hi32, near = hi.astype(np.float32), value.astype(np.float16)
        # value = hi + lo' 2^-11 is exact in fp32 (lo' is a multiple of 2^11 ulp32(x)), so lo' comes back bit for bit
        assert np.array_equal(lo, ((value - hi32) * np.float32(2048)).astype(np.float16))
        # hi = f16(value), except where lo' ROUNDED UP to half an f16 step of hi: value is then exactly midway between hi and
        # its neighbour, and round-to-nearest-even of that tie may name the neighbour (about one element in 2^13).  Nothing
        # else is let through: a differing element must be that exact tie.
        off = hi != near
        assert np.array_equal(value[off] - hi32[off], near.astype(np.float32)[off] - value[off]), "hi is not a nearest f16 of the value"
        # and the pair is the split of the fp32 kernel's own result on the same inputs, bit for bit: the same MFMA kernel
        # stores either o * inv or its (hi | lo')
        x = _launch(eng, R.make_case(design, B, H, Lq, Lk, shared), 1, layout, shared)["out"].reshape(B * Lq, Dm)
        assert np.array_equal(hi, x.astype(np.float16))
        assert np.array_equal(lo, ((x - hi32) * np.float32(2048)).astype(np.float16))


@pytest.mark.parametrize("design,B,H,Lq,Lk", (("select", 3, 4, 33, 65), ("stress", 1, 2, 129, 193)))
def test_fp32_misaligned_output_takes_the_fallback(eng, design, B, H, Lq, Lk):
    """o_ld % 4 != 0 breaks the 16-byte rule of the MFMA form: launch_attention_f32 runs attn_f32_kernel, and
    launch_attention_f32_pair reports that it does not apply and stores nothing."""
    Dm = H * 128
    _check(eng, design, 1, 0, B, H, Lq, Lk, o_ld=Dm + 2)
    c = R.make_case(design, B, H, Lq, Lk)
    r = _launch(eng, c, 2, 0, o_ld=Dm + 2)
    assert not r["ran"] and (r["raw"] == R.CANARY).all()
