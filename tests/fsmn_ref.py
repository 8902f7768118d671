"""Float64 definition, case table and derived error bound for the stand-alone FSMN memory blocks of csrc/k_misc.hip:
fsmn_enc_kernel<3 | 5 | 7 | 9 | 11> (launch_fsmn_enc), fsmn_f32_win_kernel<11> (launch_fsmn_f32_ld), fsmn_f32_kernel<0>
(launch_fsmn_f32, and the fallback of launch_fsmn_dec) and fsmn_dec_kernel<11 | 21> (launch_fsmn_dec).  TEST INFRASTRUCTURE ONLY:
tests/test_gpu_fsmn_conformance.py compares the device with what stands here, tests/test_fsmn_ref_cpu.py compares what stands
here with three independent formulations and shows that check() rejects eleven wrong kernels.

One definition, fsmn(v, taps, k, valid | mask):
    y[b, t, c] = m_t (v m)[b, t, c] + m_t sum_j taps[j, c] (v m)[b, t + j - left, c],   left = (k - 1) // 2, zero outside [0, T)
m from valid[b] (a length: the decoder's token_num; a masked row is never READ, so it may hold NaN), from a float mask [B, T]
(it multiplies; fractions allowed) or absent.  Returned with the magnitude sum_j |taps| |v m| + |v m| the bound needs.  The
decoder form adds y into x on the valid rows and leaves every other cell of x with its bits.

Two designs.
  dyadic   v = i 2^-4 with |i| <= 8, or 1024 <= |i| < 2048 in the rows within `left` of an utterance seam (B > 1); taps = i 2^-6,
           1 <= |i| <= 8; x = i 2^-10, |i| <= 2^12; masks in {0, 1/4, 1/2, 1}.  Every one is an f16 value.  Bit budget: a product
           v w m m' is an integer multiple of U = 2^-14 (2^-4 2^-6 2^-2 2^-2), so is every partial sum in any order, and the sum of
           the absolute values of all terms of one result is at most 2047 2^-4 (1 + 21 * 8 * 2^-6) + 4 < 464 = 2^22.9 U < 2^24 U:
           every partial sum is exact in fp32 whatever the order and whether or not a product is contracted into an FMA.
           make_case asserts the grid and the 2^24 U budget on the case it built.  The result must equal the float64 value bit
           for bit.  A tap taken across a seam moves a result by at least 1024 2^-4 2^-6 = 1 while the result stays below 2^9,
           where fp32 counts in 2^-15: 2^15 ulps (make_case asserts >= 2^10).
  normal   v standard normal (rounded to f16 for the encoder kernel) with a common offset of 64 on every fourth row, taps
           0.1 N(0, 1) as fp32.  Bound: the kernels' arithmetic was read from the gfx950 code of k_misc.hip: every tap is one
           fused multiply-add (v_pk_fma_f32 / v_fmac_f32; no separate product rounding), the identity term one add (encoder,
           decoder) or the start value of the sum (fp32 kernels; v * 1 is exact), the decoder's `x +` one more add.  A term
           therefore meets at most k + 1 roundings in fsmn_enc_kernel, k in fsmn_f32_win_kernel and fsmn_f32_kernel<0> (a mask
           value that is a power of two multiplies exactly), k + 2 in fsmn_dec_kernel and the decoder fallback, so to first
           order |err| <= (k + 2) 2^-24 magnitude for all of them (the decoder's magnitude includes |x|).  bound_factor
           holds the k + 2; nothing here is tuned to a measurement."""
import collections
import functools

import numpy as np

import gemm_ref as G
import rows_ref as R

f16, is_f16 = G.f16, G.is_f16
body, assert_guards, bits = R.body, R.assert_guards, R.bits
OP_GUARD_ROWS, CANARY32 = R.OP_GUARD_ROWS, R.CANARY32

FS_ROWS = 8                                        # frames per thread of the window kernels (csrc/k_misc.hip)
UNIT = 2.0 ** -14
KS_ENC = (3, 5, 7, 9, 11)
TS = (1, 2, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33)      # below left, left .. FS_ROWS, 8 m - 1 | 8 m | 8 m + 1
BS = (1, 3)
DS = (8, 24, 512)
LS_DEC = (1, 3, 8, 9, 17, 25)
ODD_ENC = (3, 450, 12)                             # 3 * 57 * 3 = 513 = 2 * 256 + 1 threads of the window kernels
ODD_F32 = (1, 257, 4)                              # 257 threads of the one-row-per-thread kernel
LOG = {}


def bound_factor(k):
    return k + 2


def note(key, ratio):
    LOG[key] = max(LOG.get(key, 0.0), float(ratio))
    return ratio


# eleven wrong kernels; the first comes in both directions
MUTANTS = ("left_plus", "left_minus", "taps_reversed", "no_identity", "double_identity", "seam", "mask_input_only", "mask_output_only",
           "token_le", "skip_last_frame", "masked_x_plus_zero", "clamped_edge")


# ------------------------------------------------------------------------------------------------ the definition
def fsmn(v, taps, k, valid=None, mask=None, mutate=None):
    """-> (y, magnitude) float64 [B, T, D].  mutate: a wrong kernel (MUTANTS), for tests/test_fsmn_ref_cpu.py; "skip_last_frame"
    marks the frame it does not store with NaN"""
    v, w = np.asarray(v, np.float64), np.asarray(taps, np.float64)
    B, T, D = v.shape
    assert w.shape == (k, D) and (valid is None or mask is None)
    left = (k - 1) // 2 + {"left_plus": 1, "left_minus": -1}.get(mutate, 0)
    if mutate == "taps_reversed":
        w = w[::-1]
    if valid is not None:
        n = np.asarray(valid)[:, None]
        m = (np.arange(T)[None, :] <= n) if mutate == "token_le" else (np.arange(T)[None, :] < n)
        vin = np.where(m[..., None], v, 0.0)                              # a masked row is never read
        m = m.astype(np.float64)
    elif mask is not None:
        m = np.asarray(mask, np.float64)
        vin = v * m[..., None]
    else:
        m = np.ones((B, T))
        vin = v
    if mutate == "mask_output_only":
        vin = v
    mout = np.ones((B, T)) if mutate == "mask_input_only" else m
    ident = {"no_identity": 0.0, "double_identity": 2.0}.get(mutate, 1.0)
    y, mag = ident * vin, np.abs(vin)
    flat = vin.reshape(B * T, D)
    for j in range(k):
        src = np.arange(T) + j - left
        if mutate == "seam":                                               # the neighbouring utterance's rows
            rows = np.arange(B)[:, None] * T + src[None, :]
            ok = (rows >= 0) & (rows < B * T)
            term = np.where(ok[..., None], flat[np.clip(rows, 0, B * T - 1)], 0.0)
        elif mutate == "clamped_edge":                                     # the clamped read used, not skipped
            term = vin[:, np.clip(src, 0, T - 1)]
        else:
            ok = (src >= 0) & (src < T)
            term = np.where(ok[None, :, None], vin[:, np.clip(src, 0, T - 1)], 0.0)
        y = y + w[j] * term
        mag = mag + np.abs(w[j]) * np.abs(term)
    if valid is not None:
        y, mag = np.where(mout[..., None] > 0, y, 0.0), np.where(mout[..., None] > 0, mag, 0.0)
    else:
        y, mag = y * mout[..., None], mag * np.abs(mout[..., None])
    if mutate == "skip_last_frame" and T % FS_ROWS:
        y = y.copy()
        y[:, T - 1] = np.nan
    return y, mag


# ------------------------------------------------------------------------------------------------ the case table
Spec = collections.namedtuple("Spec", "name kind design k B T D ldv col form mask valid hostile")
Case = collections.namedtuple("Case", "spec v taps mask valid x")


def _spec(kind, design, k, B, T, D, ldv=0, col=0, form=0, mask=None, valid=None, hostile=0):
    name = "%s-%s-k%d-B%d-T%d-D%d" % (kind, design, k, B, T, D)
    if ldv not in (0, D):
        name += "-ld%d+%d" % (ldv, col)
    if form:
        name += "-form%d" % form
    if mask:
        name += "-" + mask
    if valid is not None:
        name += "-n" + ".".join(str(n) for n in valid) + "-" + ("finite", "nan", "inf")[hostile]
    return Spec(name, kind, design, k, B, T, D, ldv or D, col, form, mask, valid, hostile)


def shapes(odd=None):
    """(B, T, D) of the grid, then the shape with 256 n + 1 threads"""
    out = [(B, T, D) for D in DS for B in BS for T in TS]
    return out + ([odd] if odd else [])


def enc_specs(k, D=None):
    """fsmn_enc_kernel<k>: the grid (one D, or all with the 513-thread shape) x {dense, the V third of Q | K | V} x both designs"""
    return [_spec("enc", design, k, B, T, Dd, ldv=ld * Dd, col=(ld - 1) * Dd)
            for (B, T, Dd) in shapes(ODD_ENC) if D is None or Dd == D for ld in (1, 3) for design in ("dyadic", "normal")]


def win_specs(D=None):
    """fsmn_f32_win_kernel<11> as the launchers choose it (form 0, no mask, k = 11): dense and strided"""
    return [_spec("f32", design, 11, B, T, Dd, ldv=ld * Dd, col=(ld - 1) * Dd)
            for (B, T, Dd) in shapes(ODD_ENC) if D is None or Dd == D for ld in (1, 3) for design in ("dyadic", "normal")]


def generic_specs(D=None):
    """fsmn_f32_kernel<0>: k = 11 forced (form 1), k = 3 | 9 | 21 without a mask, k = 5 | 11 under a binary and a fractional mask"""
    out = []
    for (B, T, Dd) in shapes(ODD_F32):
        if D is not None and Dd != D:
            continue
        for design in ("dyadic", "normal"):
            out.append(_spec("f32", design, 11, B, T, Dd, form=1))
            out += [_spec("f32", design, k, B, T, Dd) for k in (3, 9, 21)]
            out += [_spec("f32", design, k, B, T, Dd, mask="binary") for k in (5, 11)]
        out += [_spec("f32", "dyadic", k, B, T, Dd, mask="frac") for k in (5, 11)]
    return out


def dec_token_sets(L):
    """[(token_num, hostile)], B = 3: four sets at every L (0, L and L + 3 among them); at L = 17 the middle utterance, between
    one above L and a full one, takes every value in [0, L]: every position of a block and of the one behind it"""
    sets = {tn: i % 3 for i, tn in enumerate(((L, 0, L + 3), (L + 3, L, L), (0, 0, 0), (L, (L + 1) // 2, 0)))}
    if L == 17:
        for n in range(L + 1):
            sets.setdefault((L + 3, n, L), n % 3)
    return list(sets.items())


def dec_specs(k, D=None):
    """launch_fsmn_dec: k = 11 | 21 the window kernel, anything else the fallback"""
    out = []
    for Dd in (8, 512):
        if D is not None and Dd != D:
            continue
        for L in LS_DEC:
            for i, (tn, hostile) in enumerate(dec_token_sets(L)):
                out.append(_spec("dec", "dyadic", k, 3, L, Dd, valid=tn, hostile=hostile))
                if i < 4:
                    out.append(_spec("dec", "normal", k, 3, L, Dd, valid=tn, hostile=(hostile + 1) % 3))
    if D is None:
        B, T, Dd = ODD_ENC
        out.append(_spec("dec", "dyadic", k, B, T, Dd, valid=(T, T // 2 + 3, T + 1), hostile=1))
    return out


def _rng(spec):
    """seeded by what the data depend on: not by the row stride or the form, so that those cases hold the same bytes"""
    import zlib
    return np.random.default_rng(zlib.crc32(repr(spec._replace(name="", ldv=0, col=0, form=0)).encode()))


X_HOSTILE = np.array([0x80000000, 0x00000001, 0x7FC12345, 0xFFC00001, 0x7149F2CA, 0x80000001], np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(spec):
    r = _rng(spec)
    k, B, T, D = spec.k, spec.B, spec.T, spec.D
    left = (k - 1) // 2
    mask = valid = x = None
    if spec.design == "dyadic":
        iv = r.integers(-8, 9, (B, T, D))
        near = np.zeros((B, T), bool)                                      # the rows within `left` of a seam between utterances
        for b in range(B):
            if b + 1 < B:
                near[b, max(T - left, 0):] = True
            if b > 0:
                near[b, :left] = True
        big = r.integers(1024, 2048, (B, T, D)) * r.choice([-1, 1], (B, T, D))
        iv = np.where(near[..., None], big, iv)
        v = iv * 2.0 ** -4
        taps = r.integers(1, 9, (k, D)) * r.choice([-1, 1], (k, D)) * 2.0 ** -6
    else:
        v = r.standard_normal((B, T, D)) + 64.0 * (np.arange(T) % 4 == 1)[None, :, None]
        v = f16(v) if spec.kind == "enc" else v.astype(np.float32).astype(np.float64)
        taps = (0.1 * r.standard_normal((k, D))).astype(np.float32).astype(np.float64)
    if spec.mask == "binary":
        lens = r.integers(0, T + 1, B)
        lens[0] = max(T - 1, 0)
        mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)
    elif spec.mask == "frac":
        mask = r.choice([0.0, 0.25, 0.5, 1.0], (B, T))
    if spec.kind == "dec":
        valid = np.asarray(spec.valid, np.int32)
        masked = np.arange(T)[None, :] >= valid[:, None]
        if spec.design == "dyadic":
            x = r.integers(-2 ** 12, 2 ** 12 + 1, (B, T, D)) * 2.0 ** -10
        else:
            x = r.standard_normal((B, T, D)).astype(np.float32).astype(np.float64)
        x = x.astype(np.float32)
        x[masked] = X_HOSTILE[(np.arange(int(masked.sum()) * D) % len(X_HOSTILE))].reshape(-1, D)   # -0, denormals, NaN payloads
        v = v.copy()                                                       # what the device buffer holds there; never read
        v[masked] = (np.nan, np.inf)[spec.hostile - 1] if spec.hostile else 2.0 ** 100 * (1 + (np.arange(D) % 7) / 8.0)
    c = Case(spec, v, taps, mask, valid, x)
    if spec.design == "dyadic":
        live = v if valid is None else np.where(np.arange(T)[None, :, None] < valid[:, None, None], v, 0.0)
        assert is_f16(live) and is_f16(taps) and (live * 16 == np.round(live * 16)).all() and (taps * 64 == np.round(taps * 64)).all()
        assert mask is None or np.isin(mask, (0.0, 0.25, 0.5, 1.0)).all()
        _, mag = fsmn(v, taps, k, valid=valid, mask=mask)
        if x is not None:
            xv = np.where(masked[..., None], 0.0, x.astype(np.float64))
            assert (xv * 1024 == np.round(xv * 1024)).all()
            mag = mag + np.abs(xv)
        assert mag.max() < 2.0 ** 24 * UNIT, (spec.name, mag.max())         # the bit budget of the module docstring
        if B > 1 and valid is None and mask is None:                       # a tap across the seam: >= 2^10 ulps somewhere
            y, _ = fsmn(v, taps, k)
            ys, _ = fsmn(v, taps, k, mutate="seam")
            ulp = np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
            assert (np.abs(ys - y) / ulp).max() >= 2.0 ** 10, spec.name
    for a in c[1:]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expect(spec):
    """(reference, bound) float64 [B T, D] of the stored result; the decoder form: x + y on the valid rows (elsewhere: 0, 0 — those
    rows are compared by their bits)"""
    c = make_case(spec)
    y, mag = fsmn(c.v, c.taps, spec.k, valid=c.valid, mask=c.mask)
    if spec.kind == "dec":
        ok = (np.arange(spec.T)[None, :] < c.valid[:, None])[..., None]
        x64 = np.where(ok, c.x.astype(np.float64), 0.0)
        y, mag = np.where(ok, x64 + y, 0.0), np.where(ok, np.abs(x64) + mag, 0.0)
    bnd = 0.0 * mag if spec.design == "dyadic" else bound_factor(spec.k) * 2.0 ** -24 * mag
    return y.reshape(-1, spec.D), bnd.reshape(-1, spec.D)


def check(spec, got, key=None):
    """the assertions of the GPU suite on `got`, the body [B T, D] float32 of a guarded result: dyadic bit for bit (as values: a
    bound of 0), normal within the bound; the decoder form besides: every valid row finite, every masked row of x its bits"""
    c = make_case(spec)
    ref, bnd = expect(spec)
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape, (spec.name, got.shape, ref.shape)
    g64 = got.astype(np.float64)
    if spec.kind == "dec":
        ok = (np.arange(spec.T)[None, :] < c.valid[:, None]).reshape(-1)
        x = c.x.reshape(-1, spec.D)
        bad = np.argwhere(bits(got[~ok]) != bits(x[~ok]))
        assert not len(bad), "%s: a masked row of x changed: masked row %d column %d holds 0x%08X, went in as 0x%08X" % (
            spec.name, bad[0][0], bad[0][1], int(bits(got[~ok])[tuple(bad[0])]), int(bits(x[~ok])[tuple(bad[0])]))
        assert np.isfinite(got[ok]).all(), spec.name + ": a valid row is not finite"
        g64, ref, bnd = g64[ok], ref[ok], bnd[ok]
    exact = bnd == 0
    if exact.any():
        G.assert_exact(None, np.where(exact, ref, 0.0), np.where(exact, g64, 0.0), spec.name)
    if (~exact).any():
        one = np.where(exact, 1.0, bnd)
        ratio = G.assert_bounded(np.where(exact, 0.0, ref), one, np.where(exact, 0.0, g64), spec.name)
        if key:
            note(key, ratio)
        return ratio
    return 0.0


# ------------------------------------------------------------------------------------------------ evaluations on the host
def evaluate(spec, mutate=None, order="forward"):
    """what a kernel would store for the case, [B T, D] float32, every operation rounded to fp32: the identity term, then the taps
    in `order` (forward | reversed | pairwise); mutate: a wrong kernel (MUTANTS).  The unmutated dyadic result does not depend on
    the order (tests/test_fsmn_ref_cpu.py)"""
    c = make_case(spec)
    k, B, T, D = spec.k, spec.B, spec.T, spec.D
    if mutate is not None:
        y, _ = fsmn(c.v, c.taps, k, valid=c.valid, mask=c.mask, mutate=None if mutate == "masked_x_plus_zero" else mutate)
        y32 = y.astype(np.float32)
    else:
        f = np.float32
        if c.valid is not None:
            m = (np.arange(T)[None, :] < c.valid[:, None]).astype(f)
            vin = np.where(m[..., None] > 0, c.v, 0.0).astype(f)
        else:
            m = np.ones((B, T), f) if c.mask is None else c.mask.astype(f)
            vin = (c.v.astype(f) * m[..., None]).astype(f)
        w = c.taps.astype(f)
        left = (k - 1) // 2
        terms = [vin]
        for j in range(k):
            src = np.arange(T) + j - left
            ok = (src >= 0) & (src < T)
            terms.append((w[j] * np.where(ok[None, :, None], vin[:, np.clip(src, 0, T - 1)], f(0))).astype(f))
        if order == "reversed":
            terms = terms[::-1]
        if order == "pairwise":
            while len(terms) > 1:
                terms = [(terms[i] + terms[i + 1]).astype(f) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            y32 = terms[0]
        else:
            y32 = terms[0]
            for t in terms[1:]:
                y32 = (y32 + t).astype(f)
        y32 = (y32 * m[..., None]).astype(f)
    if spec.kind == "dec":
        ok = np.arange(T)[None, :] < c.valid[:, None]
        if mutate == "token_le":
            ok = np.arange(T)[None, :] <= c.valid[:, None]
        if mutate == "mask_input_only":
            ok = np.ones_like(ok)
        with np.errstate(invalid="ignore", over="ignore"):
            wr = ok[..., None] & ~np.isnan(y32) if mutate == "skip_last_frame" else ok[..., None]   # the skipped frame: x as it was
            out = np.where(wr, (c.x + y32).astype(np.float32), c.x)
            if mutate == "masked_x_plus_zero":
                out = np.where(ok[..., None], out, (c.x + np.float32(0)).astype(np.float32))
        return out.reshape(-1, D)
    if mutate == "skip_last_frame":                                        # the frame it skipped keeps the canary
        y32 = np.where(np.isnan(y32), np.array([CANARY32], np.uint32).view(np.float32)[0], y32)
    return y32.reshape(-1, D)
