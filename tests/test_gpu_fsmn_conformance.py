"""GPU: the stand-alone FSMN memory blocks of csrc/k_misc.hip — fsmn_enc_kernel<3 | 5 | 7 | 9 | 11> (launch_fsmn_enc),
fsmn_f32_win_kernel<11> (launch_fsmn_f32_ld, and launch_fsmn_f32 without a mask at k = 11), fsmn_f32_kernel<0> (launch_fsmn_f32
otherwise, and the fallback of launch_fsmn_dec) and fsmn_dec_kernel<11 | 21> (launch_fsmn_dec) — each launcher alone through a
thin stand-alone op (engine_ops.cpp: op_fsmn_enc_ex, op_fsmn_f32_ex, op_fsmn_dec_ex) against the float64 definition, the two
designs and the derived bound of tests/fsmn_ref.py.  The ops add no arithmetic: the operand lies amid a large finite pattern
(the Q | K columns beside V, 16 rows behind row B T - 1), the result comes back inside its canary-filled buffer, the masked
rows of the decoder's tn hold a large finite pattern, NaN or Inf on the device.  Every case asserts the kernel that ran
(Engine.profile_kernel), is run twice and must return the same bytes.  tests/test_fsmn_ref_cpu.py checks the definition against
three independent formulations and shows which case of this table rejects which of eleven wrong kernels.

What is visited.  T (the decoder's L) below `left`, between `left` and the 8 frames of a thread, at 8 m - 1 | 8 m | 8 m + 1;
B = 1 and 3, the rows on either side of an utterance seam large, so that a tap across it is 2^15 ulps; D = 8, 24 (a partial
workgroup) and 512, and one shape with 256 n + 1 threads per kernel; dense rows and the V third of a Q | K | V row (ldv = 3 D at
column 2 D); every tap count launch_fsmn_enc instantiates; the generic kernel at k = 3, 9, 11 (forced), 21 and under binary
and fractional masks; the decoder at k = 11, 21 and 9 (the fallback) with token_num at every value in [0, 17] inside B = 3,
at 0, L and L + 3, the masked rows of x holding -0, denormals and NaN payloads.  The generic kernel has no row stride
(launch_fsmn_f32 takes none): it runs on dense rows only.

Measured (one run of this file with -s on an MI355X, at the commit that adds it; the fixture prints the table when it closes; no
figure below was known before the bound was written down): 42 tests pass, 2.5 s for all of them after 1.7 s for the engine,
the largest (the generic kernel's cases at D = 512) 0.4 s; every guard cell canary, every dyadic case bit-equal, every masked
row of x its bits, every repeated call the same bytes.  Worst |err| / bound on the normal design, bound (k + 2) 2^-24 magnitude:
    fsmn_enc_kernel<3>  0.564   <5>  0.459   <7>  0.420   <9>  0.376   <11>  0.344
    fsmn_f32_win_kernel<11>                        0.444
    fsmn_f32_kernel<0> (k = 3 .. 21, masks)        0.597
    fsmn_f32_kernel<0> as the decoder fallback, 9  0.541
    fsmn_dec_kernel<11>  0.418   <21>  0.280
The largest ratios belong to the short windows (k = 3, and the rows at an utterance's edge), where two or three roundings of
nearly the whole magnitude stand against a bound of k + 2 of them.
The window kernel against the generic kernel (the "same roundings" comment on fsmn_f32_win_kernel): bit-equal on every normal
case of the grid, dense and at ldv = 3 D; the comment stands.

Found in the kernels:
  * the fallback of launch_fsmn_dec (k outside {11, 21}: fsmn_f32_kernel<0> with token_num and accumulate) multiplied a masked
    row of tn by 0 and stored x + 0 into a masked row of x: a NaN or Inf in a masked row of tn reached the valid rows next to
    it, and a masked -0 of x came back as +0, against the contract of its siblings.  The token_num path now skips masked input
    rows and the store of a masked output row (test_dec at k = 9 cannot pass without either: the NaN / Inf cases need the
    first, the -0 cells of every masked row the second);
  * launch_fsmn_f32 sent v == y to the generic kernel, where a thread reads rows its neighbours overwrite; it now refuses;
  * launch_fsmn_enc left the channels of a D that is no multiple of the channels per thread unwritten and loaded through
    misaligned vector pointers for an odd row stride or column offset; it now refuses both."""
import time

import numpy as np
import pytest

import fsmn_ref as F
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W

pytestmark = pytest.mark.gpu

ENC, WIN, GEN, DEC = "fsmn_enc_kernel<%d>", "fsmn_f32_win_kernel<11>", "fsmn_f32_kernel<0>", "fsmn_dec_kernel<%d>"


@pytest.fixture(scope="module")
def eng():
    from aliparaformerasr_amd.engine import Engine
    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
    e = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=5)), cmvn=W.synth_cmvn(), device=0)
    assert (e.OP_GUARD_ROWS, e.OP_CANARY32) == (F.OP_GUARD_ROWS, F.CANARY32)
    e.profile(True)
    t0 = time.perf_counter()
    yield e
    e.close()
    print("wall time of the module's tests: %.1f s" % (time.perf_counter() - t0))
    print("worst |err| / bound per kernel on the normal design:")
    for k, v in sorted(F.LOG.items()):
        print("    %-40s %.3f" % (k, v))


def _run(eng, spec):
    c = F.make_case(spec)
    eng.profile_reset()
    if spec.kind == "enc":
        buf = eng.op_fsmn_enc_ex(c.v.astype(np.float16), c.taps, spec.ldv, spec.col)
    elif spec.kind == "f32":
        buf = eng.op_fsmn_f32_ex(c.v, c.taps, c.mask, spec.ldv, spec.col, spec.form)
    else:
        buf = eng.op_fsmn_dec_ex(c.v, c.taps, c.valid, c.x, spec.hostile)
    return buf, eng.profile_kernel("gemm_op")


def _check(eng, spec, kernel, key=None):
    rows = spec.B * spec.T
    buf, ran = _run(eng, spec)
    assert ran == kernel, (spec.name, ran)
    F.assert_guards(buf, rows, spec.D, spec.name)
    got = F.body(buf, rows)
    ratio = F.check(spec, got, key=key or kernel)
    again, _ = _run(eng, spec)
    assert np.array_equal(F.bits(again), F.bits(buf)), spec.name + ": two runs, different bytes"
    return got, ratio


def _refused(code, fn, *a, **kw):
    with pytest.raises(N.PfError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


# ------------------------------------------------------------------------------------------------ fsmn_enc_kernel
@pytest.mark.parametrize("D", F.DS + (F.ODD_ENC[2],))
@pytest.mark.parametrize("k", F.KS_ENC)
def test_enc(eng, k, D):
    """every T and B of the grid, dense and as the V third of Q | K | V, dyadic bit for bit (seams included) and normal within
    the bound against float64 of the f16 operand; D = 12: the shape with 513 threads"""
    specs = F.enc_specs(k, D)
    assert len(specs) == (4 if D == F.ODD_ENC[2] else 4 * len(F.TS) * len(F.BS))
    for spec in specs:
        _check(eng, spec, ENC % k)


def test_enc_refusals(eng):
    v, r = np.zeros((1, 9, 8), np.float16), _refused
    for k in (4, 13):
        r(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_enc_ex, v, np.zeros((k, 8), np.float32))
    taps = np.zeros((11, 8), np.float32)
    r(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_enc_ex, np.zeros((1, 9, 6), np.float16), np.zeros((11, 6), np.float32))   # D % 4
    r(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_enc_ex, v, taps, 10, 0)                   # a row stride off the 8-byte load
    r(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_enc_ex, v, taps, 12, 2)                   # a column offset off it
    r(N.PF_ERR_INVALID_ARG, eng.op_fsmn_enc_ex, v, taps, 12, 8)                   # V does not fit the row
    assert eng.op_fsmn_enc_ex(v, taps, 12, 4).shape == (9 + 2 * F.OP_GUARD_ROWS, 8)


# ------------------------------------------------------------------------------------------------ the fp32 kernels
@pytest.mark.parametrize("D", F.DS + (F.ODD_ENC[2],))
def test_f32_win(eng, D):
    """what the fp32 engine launches: k = 11, no mask; dense through launch_fsmn_f32, strided through launch_fsmn_f32_ld"""
    for spec in F.win_specs(D):
        _check(eng, spec, WIN)


@pytest.mark.parametrize("D", F.DS + (F.ODD_F32[2],))
def test_f32_generic(eng, D):
    """fsmn_f32_kernel<0>: k = 11 forced, k = 3 | 9 | 21, binary and fractional masks"""
    specs = F.generic_specs(D)
    assert {s.mask for s in specs} == {None, "binary", "frac"} and {s.k for s in specs if s.mask is None} == {3, 9, 11, 21}
    for spec in specs:
        _check(eng, spec, GEN)


@pytest.mark.parametrize("D", F.DS)
def test_f32_win_has_the_roundings_of_the_generic_kernel(eng, D):
    """the comment on fsmn_f32_win_kernel: the window kernel (dense and strided) and the generic kernel on the same operand
    return the same bits, on the normal design, where a different order or contraction would show"""
    for spec in F.win_specs(D):
        if spec.design != "normal" or spec.ldv != D:
            continue
        win, _ = _run(eng, spec)
        ld3, _ = _run(eng, spec._replace(ldv=3 * D, col=2 * D))
        gen, ran = _run(eng, spec._replace(form=1))
        assert ran == GEN
        assert np.array_equal(F.bits(win), F.bits(ld3)), spec.name + ": dense and strided differ"
        assert np.array_equal(F.bits(win), F.bits(gen)), spec.name + ": window and generic kernel differ"


def test_f32_in_place_is_refused(eng):
    """launch_fsmn_f32 with y == v: refused before anything runs, with and without a mask, at k = 11 and elsewhere"""
    v = np.ones((1, 9, 8), np.float32)
    for k in (11, 5):
        for mask in (None, np.ones((1, 9), np.float32)):
            _refused(N.PF_ERR_INVALID_ARG, eng.op_fsmn_f32_ex, v, np.zeros((k, 8), np.float32), mask, 0, 0, 2)
    _refused(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_f32_ex, v, np.zeros((5, 8), np.float32), None, 24, 16)     # _ld: k = 11 only
    _refused(N.PF_ERR_UNSUPPORTED, eng.op_fsmn_f32_ex, v, np.zeros((11, 8), np.float32), np.ones((1, 9), np.float32), 24, 16)


# ------------------------------------------------------------------------------------------------ launch_fsmn_dec
@pytest.mark.parametrize("D", (8, 512, F.ODD_ENC[2]))
@pytest.mark.parametrize("k", (11, 21, 9))
def test_dec(eng, k, D):
    """k = 11 | 21: fsmn_dec_kernel; 9: the fallback.  Masked tn rows hold a large finite pattern, NaN or Inf; every valid row
    finite and equal to the reference (dyadic: bit for bit), every masked row of x (-0, denormals, NaN payloads) its bits"""
    specs = [s for s in F.dec_specs(k)] if D == F.ODD_ENC[2] else F.dec_specs(k, D)
    specs = [s for s in specs if s.D == D]
    assert specs and (D == F.ODD_ENC[2] or {s.hostile for s in specs} == {0, 1, 2})
    if D != F.ODD_ENC[2]:
        assert {s.valid[1] for s in specs if s.T == 17} >= set(range(18))
    for spec in specs:
        _check(eng, spec, (DEC % k) if k in (11, 21) else GEN, key=None if k in (11, 21) else GEN + " as the decoder fallback, k = 9")
