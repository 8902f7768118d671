"""GPU: the CIF kernels (k_misc.hip: cif_scan_kernel, cif_scan_cumsum_kernel, cif_gather_kernel, cif_gather_cumsum_kernel, and the
predictor tail cif_im2col_kernel / the fp32 im2col -> conv GEMM -> cif_alpha_kernel) on the case table of tests/cif_ref.py.

Everything goes through pf_op_cif and pf_op_cif_alphas, the launchers and the member functions the pipelines call.  Two tiers:

  bit equality   E, fire_count, token_num and L against oracle.model's cif_fire / cif_fire_cumsum, at D = 512 (random H), D = 4, D = 516
                 (the gather kernels' second trip over the channels) and the one-hot D.  Bits are compared as 32-bit words; only the
                 sign of a zero is left open (a token completed on the tail frame: the oracle adds the tail's zero hidden state, the
                 kernels skip it, so -0.0 can stand where the oracle has +0.0).
  float64 tier   the weight matrices read from the device's one-hot runs against the definition (cif_ref.check_weights,
                 float64_crossings) — no code shared with the oracle.

tests/test_cif_ref_cpu.py proves on the reference alone that the table reaches what these tests are for: the inexact family takes
cif_scan_cumsum_kernel's sequential redo (and the random family its parallel walk), the near-tie family holds fire_count != token_num
in both directions and utterances on which the two formulations disagree."""
import ctypes as C
import functools

import numpy as np
import pytest

import cif_ref as CR
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W
from oracle import model as om

pytestmark = pytest.mark.gpu
VARIANTS = ("loop", "cumsum")
ORACLE = {"loop": om.Oracle.cif_fire, "cumsum": om.Oracle.cif_fire_cumsum}
SIZES = ("d512", "d4", "d516", "onehot")
CFG = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128)
SEED = 5


@pytest.fixture(scope="module")
def engines():
    """the two engines of the suite (default cif_variant and "cumsum"), and one fp32 engine for the alpha stage, on first use"""
    from aliparaformerasr_amd.engine import Engine
    made = {}

    def get(variant="loop", math_mode=0):
        key = (variant, math_mode)
        if key not in made:
            cfg = CFG if variant == "loop" else W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=128, cif_variant=variant)
            made[key] = Engine(weights=W.pack_pfw(cfg, W.synth_weights(cfg, seed=SEED)), cmvn=W.synth_cmvn(), device=0, math_mode=math_mode)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _case(name):
    return next(c for c in CR.cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def _hidden(name, size):
    c = _case(name)
    if size == "onehot":
        return c.H
    H = CR.random_hidden(c, int(size[1:]))
    H.flags.writeable = False
    return H


def _thr(case, variant):
    return case.threshold if variant == "loop" else 1.0          # the prefix-sum export has no threshold input


@functools.lru_cache(maxsize=None)
def _want(name, variant, size):
    """the oracle's (E, fire_count, token_num); computed once, shared, read-only"""
    c = _case(name)
    out = ORACLE[variant](_hidden(name, size), c.alphas, _thr(c, variant))
    for a in out:
        a.flags.writeable = False
    return out


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.dtype == np.float32:
        differ = (got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0))
    else:
        differ = got != want
    assert not differ.any(), "%s: %d of %d words differ, first at %s" % (what, int(differ.sum()), differ.size, np.argwhere(differ)[0])


def _run(eng, name, variant, size):
    c = _case(name)
    return eng.op_cif(_hidden(name, size), c.alphas, threshold=_thr(c, variant))


# ------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_whole_table_bit_equal_to_the_oracle(engines, variant, size):
    eng = engines(variant)
    ran = 0
    for c in CR.cases():
        if size == "onehot" and c.H is None:
            continue
        E, fc, tn = _run(eng, c.name, variant, size)
        Er, fcr, tnr = _want(c.name, variant, size)
        what = "%s %s %s" % (c.name, variant, size)
        _same_bits(fc, fcr, what + " fire_count")
        _same_bits(tn, tnr, what + " token_num")
        assert E.shape[1] == Er.shape[1] == (int(fcr.max()) if fcr.size else 0), what + " L"
        _same_bits(E, Er, what + " E")
        ran += 1
    assert ran >= (20 if size == "onehot" else len(CR.cases()))


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_calls_return_equal_bytes(engines, variant):
    eng = engines(variant)
    for name in ("random_T1_1025", "inexact_T1_501_x1e-09", "near_tie_T1_500"):
        first = _run(eng, name, variant, "d512")
        again = _run(eng, name, variant, "d512")
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), name


# ------------------------------------------------------------------ float64 tier, no oracle
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_hot_weight_matrices_meet_the_definition(engines, variant):
    """rows sum to 1, columns to alpha[t], fire frames strictly increase (bounds: cif_ref's docstring); fire frames equal the
    float64 prefix's integer crossings on the random and inexact families wherever the prefix keeps its distance from the integers.
    measured on the device: the oracle's own figures, |row sum - 1| <= 1.2e-7 (loop) and 6.1e-6 (cumsum), column error 0."""
    eng = engines(variant)
    worst_row = worst_col = 0.0
    compared = skipped = 0
    for c in CR.cases():
        if c.H is None or c.threshold != 1.0:
            continue
        E, fc, _ = _run(eng, c.name, variant, "onehot")
        T = c.alphas.shape[1] - 1
        for b in range(c.alphas.shape[0]):
            Wm = CR.weight_matrix(E[b], int(fc[b]), T)
            ff, row_err, col_err = CR.check_weights(Wm, c.alphas[b], variant)
            worst_row, worst_col = max(worst_row, row_err), max(worst_col, col_err)
            if c.family in ("random", "inexact"):
                want, decidable = CR.float64_crossings(c.alphas[b], variant)
                if not decidable:
                    skipped += 1
                    continue
                assert ff == want, (c.name, b, ff, want)
                compared += 1
    print("%s: largest |row sum - 1| %.3g, largest column error %.3g u alpha; fire frames of %d utterances compared, %d skipped" %
          (variant, worst_row, worst_col, compared, skipped))
    assert compared >= 20


@pytest.mark.parametrize("variant", VARIANTS)
def test_fire_counts_of_the_long_utterances_are_the_float64_crossings(engines, variant):
    """the random family beyond the one-hot sizes (T+1 = 301, 1025, the ragged batch): fire_count against the crossings"""
    eng = engines(variant)
    compared = 0
    for c in CR.family("random"):
        _, fc, _ = _run(eng, c.name, variant, "d4")
        for b in range(c.alphas.shape[0]):
            want, decidable = CR.float64_crossings(c.alphas[b], variant)
            if decidable:
                assert int(fc[b]) == len(want), (c.name, b)
                compared += 1
    assert compared >= 0.95 * sum(c.alphas.shape[0] for c in CR.family("random"))


# ------------------------------------------------------------------ the two formulations
def test_variants_disagree_where_their_oracles_do(engines):
    """near-tie utterances on which cif_fire and cif_fire_cumsum give different fire counts: each engine gives its own oracle's
    count — so the two engines differ there, asserted directly — and fire_count != token_num occurs in both directions"""
    rows = more = less = 0
    for c in CR.family("near_tie"):
        got = {v: _run(engines(v), c.name, v, "d4") for v in VARIANTS}
        ref = {v: _want(c.name, v, "d4") for v in VARIANTS}
        for b in np.flatnonzero(ref["loop"][1] != ref["cumsum"][1]):
            for v in VARIANTS:
                assert got[v][1][b] == ref[v][1][b], (c.name, b, v)
            assert got["loop"][1][b] != got["cumsum"][1][b], (c.name, b)
            rows += 1
        for v in VARIANTS:
            more += int((got[v][1] > got[v][2]).sum())
            less += int((got[v][1] < got[v][2]).sum())
    assert rows >= 3 and more and less, (rows, more, less)


# ------------------------------------------------------------------ batches and the workspace
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_utterance_alone_equals_its_rows_in_the_batch(engines, variant):
    eng = engines(variant)
    c = _case("random_ragged")
    H = _hidden(c.name, "d512")
    E, fc, tn = eng.op_cif(H, c.alphas)
    assert fc[1] == 0 and fc.max() > 4 * max(int(fc[0]), 1)      # ragged: an empty row, a short one, a dense one
    for b in range(c.alphas.shape[0]):
        E1, fc1, tn1 = eng.op_cif(H[b:b + 1], c.alphas[b:b + 1])
        assert fc1[0] == fc[b] and tn1[0] == tn[b] and E1.shape[1] == fc[b]
        assert E1[0].tobytes() == E[b, : fc[b]].tobytes(), b
        assert not E[b, fc[b]:].view(np.uint32).any(), b                 # +0.0, every bit


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_behind_fire_count_are_zero_in_a_reused_workspace(engines, variant):
    """a dense batch first, then a sparse one of the same shape and Lcap: op_cif's workspace is reused, so what comes back in rows
    l >= fire_count[b] is what the gather kernel wrote there"""
    eng = engines(variant)
    dense = _case("random_T1_301")
    H = _hidden(dense.name, "d516")
    Ed, fcd, _ = eng.op_cif(H, dense.alphas)
    Lcap = int(fcd.max()) + 2
    Ed2, _, _ = eng.op_cif(H, dense.alphas, Lcap=Lcap)
    assert Ed2.tobytes() == Ed.tobytes() and np.count_nonzero(Ed) > 0.8 * Ed.size
    sparse = (dense.alphas * np.float32(0.05)).astype(np.float32)
    sparse[1] = 0.0
    sparse[2, :100] = dense.alphas[2, :100]
    Es, fcs, _ = eng.op_cif(H, sparse, Lcap=Lcap)
    L = Es.shape[1]
    assert L == fcs.max() and 0 < L < fcd.min() and fcs[1] == 0 and 0 < fcs[0] < L
    for b in range(3):
        assert np.count_nonzero(Es[b, : fcs[b]]) == fcs[b] * 516
        assert not Es[b, fcs[b]:].view(np.uint32).any(), (b, int(fcs[b]), L)


def _raw_cif(eng, H, a, Lcap, fill=np.nan):
    H, a = np.ascontiguousarray(H, np.float32), np.ascontiguousarray(a, np.float32)
    B, T, D = H.shape
    E = np.full((B, max(Lcap, 1), D), fill, np.float32)
    fc, tn, L = np.full(B, -7, np.int32), np.full(B, -7, np.int32), C.c_int32(-7)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = eng._lib.pf_op_cif(eng._h, H.ctypes.data_as(fp), a.ctypes.data_as(fp), B, T, D, 1.0, Lcap, E.ctypes.data_as(fp),
                            fc.ctypes.data_as(ip), tn.ctypes.data_as(ip), L)
    return rc, E, fc, tn, L.value


@pytest.mark.parametrize("variant", VARIANTS)
def test_capacity_and_invalid_shapes(engines, variant):
    eng = engines(variant)
    c = _case("random_T1_65")
    H = _hidden(c.name, "d4")
    Er, fcr, tnr = _want(c.name, variant, "d4")
    L = Er.shape[1]
    rc, E, fc, tn, Lo = _raw_cif(eng, H, c.alphas, L)                    # Lcap == L: every row is written
    assert rc == N.PF_OK and Lo == L
    _same_bits(E, Er, "Lcap == L")
    rc, E, fc, tn, Lo = _raw_cif(eng, H, c.alphas, L - 1)                # one short: refused, the counts are back, E untouched
    assert rc == N.PF_ERR_CAPACITY and Lo == L and np.isnan(E).all()
    _same_bits(fc, fcr, "fire_count"); _same_bits(tn, tnr, "token_num")
    rc, E, fc, tn, Lo = _raw_cif(eng, H, c.alphas, 0)                    # Lcap == 0: the counts only
    assert rc == N.PF_ERR_CAPACITY and Lo == L and np.isnan(E).all()
    _same_bits(fc, fcr, "fire_count"); _same_bits(tn, tnr, "token_num")
    z = _case("dyadic_zeros")
    rc, E, fc, tn, Lo = _raw_cif(eng, _hidden(z.name, "d4"), z.alphas, 0)   # nothing fires: L = 0 fits Lcap = 0
    assert rc == N.PF_OK and Lo == 0 and not fc.any() and not tn.any() and np.isnan(E).all()
    rc, *_ = _raw_cif(eng, np.zeros((1, 5, 6), np.float32), np.zeros((1, 6), np.float32), 4)
    assert rc == N.PF_ERR_INVALID_ARG                                    # D % 4 != 0
    rc, *_ = _raw_cif(eng, np.zeros((1, 0, 4), np.float32), np.zeros((1, 1), np.float32), 4)
    assert rc == N.PF_ERR_INVALID_ARG                                    # T = 0
    E, fc, tn = _run(eng, c.name, variant, "d4")                         # the engine stays usable
    _same_bits(E, Er, "after the refusals")


# ------------------------------------------------------------------ the predictor's alpha stage
@functools.lru_cache(maxsize=None)
def _alpha_ref(name, operands):
    """(float64 reference, its logits, distance of the float32 evaluation from it) on one input; computed once, read-only"""
    w = W.synth_weights(CFG, seed=SEED)
    H = CR.alpha_inputs(name, w, CFG)
    ref, z = CR.alpha_ref(H, w, CFG, np.float64, operands)
    rerun = float(np.abs(CR.alpha_ref(H, w, CFG, np.float32, operands)[0].astype(np.float64) - ref).max())
    for a in (H, ref, z):
        a.flags.writeable = False
    return H, ref, z, rerun


@pytest.mark.parametrize("name", CR.ALPHA_CASES)
@pytest.mark.parametrize("math_mode", [0, 1])
def test_alpha_stage_against_float64(engines, math_mode, name):
    """pf_op_cif_alphas (im2col -> conv GEMM with ReLU -> cif_alpha_kernel on the loaded predictor weights, the member function
    the pipeline runs) against cif_ref.alpha_ref in float64, operands rounded as the mode rounds them (f16 H and conv weight in
    math_mode 0, none in math_mode 1).  Bound: 4 x the distance of a float32 evaluation of the same reference from the float64 one on
    the same input — measured, not chosen.  T = 1, 2, 3 are shorter than the conv's 3 taps (padding from both ends); "contrast" puts
    utterances of very different size and sign side by side; "saturated" scales H by 50: where the float64 logit is beyond +20 / -110
    the alpha is exactly float32(smooth - noise) / exactly 0.0.  alphas[:, T] is the tail weight, bit for bit.
    measured, error (bound), math_mode 0: T = 1, 2, 3: 2.4e-9 (1.1e-7), 1.4e-8 (3.0e-7), 2.0e-8 (2.1e-7); (3, 9) 3.3e-8 (8.6e-7); (2, 83)
    4.7e-8 (1.3e-6); contrast 1.4e-7 (1.6e-6); saturated 3.4e-7 (1.5e-5).  math_mode 1: 1.0e-8 (4.0e-8), 2.2e-8 (2.7e-7), 8.7e-8
    (2.9e-7); 1.4e-7 (5.2e-7); 2.3e-7 (1.0e-6); 3.2e-7 (9.6e-7); 3.5e-6 (2.4e-5)."""
    eng = engines("loop", math_mode)
    H, ref, z, rerun = _alpha_ref(name, "f16" if math_mode == 0 else "exact")
    got = eng.op_cif_alphas(H)
    assert got.shape == ref.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bound = 4.0 * rerun
    print("alphas math_mode %d %s: err %.3g bound %.3g (float32 rerun %.3g)" % (math_mode, name, err, bound, rerun))
    assert np.isfinite(got).all()
    assert got[:, -1].tobytes() == np.full(H.shape[0], CFG["cif_tail"], np.float32).tobytes()
    if name == "saturated":
        hi, lo = z > CR.Z_SATURATED_HIGH, z < CR.Z_SATURATED_LOW
        assert hi.any() and lo.any()
        one = np.float32(np.float32(CFG["cif_smooth"]) - np.float32(CFG["cif_noise"]))
        assert (got[:, :-1][hi].view(np.uint32) == one.view(np.uint32)).all()
        assert not got[:, :-1][lo].view(np.uint32).any()
    assert err <= bound, (err, bound)


def test_alpha_stage_refuses_what_it_does_not_serve(engines):
    eng = engines("loop", 0)
    a = np.zeros((1, 1), np.float32)
    fp = C.POINTER(C.c_float)
    assert eng._lib.pf_op_cif_alphas(eng._h, np.zeros((1, 512), np.float32).ctypes.data_as(fp), 1, 0, a.ctypes.data_as(fp)) == N.PF_ERR_INVALID_ARG
    assert eng._lib.pf_op_cif_alphas(eng._h, None, 1, 1, a.ctypes.data_as(fp)) == N.PF_ERR_INVALID_ARG
