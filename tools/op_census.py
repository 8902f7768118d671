#!/usr/bin/env python3
"""Digests and launch counts of the stand-alone operator entry points (pf_op_*), one JSON object per case on stdout.

    python tools/op_census.py [PACKAGE_DIR] [--only NAME ...]

PACKAGE_DIR: the tree to import `aliparaformerasr_amd` from (default: this one) — a built copy of another commit gives that
commit's figures for the same cases, so two builds are compared digest by digest (bit identity of a refactor of the ops'
staging code: csrc/op_stage.h).  Per case: SHA-1 of the raw bytes of every array the op returns (None and scalars included
by their repr), and the launch count of every profile class an op times.  The inputs come from fixed seeds; the shapes are
the small awkward ones of the conformance suites (33 and 70 rows: no multiple of 32, one 32-row block crossed; K = 200: no
multiple of 64), never the workload's.  An op that raises is recorded with its error code, not its message."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("gemm_op", "gemm_op_warm", "gemm_op_mid", "attn_op", "gemm32_op", "gemm32_op_q", "gemm32_op_k", "gemm32_op_v", "gemm32_ffn1",
           "gemm32_ffn2", "gemm_ffn1", "gemm_ffn2", "gemm_dec_q")


def digest(x):
    import numpy as np
    h = hashlib.sha1()

    def walk(v):
        if isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode())
                walk(v[k])
        elif isinstance(v, (tuple, list)):
            h.update(b"(%d" % len(v))
            for e in v:
                walk(e)
        elif isinstance(v, np.ndarray):
            h.update(str((v.dtype.str, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    walk(x)
    return h.hexdigest()


def cases(np):
    """name -> (math_mode, fn(engine)); every fn draws from its own seeded generator"""
    f32 = np.float32
    out = {}

    def case(name, mode=0):
        def reg(fn):
            out[name] = (mode, fn)
            return fn
        return reg

    def rn(seed, *shape, scale=1.0):
        return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(f32)

    M, K, D, F = 70, 200, 512, 2048
    ln = lambda seed, n=D: (1 + 0.1 * rn(seed, n), 0.1 * rn(seed + 1, n))

    case("lfr_cmvn_pad")(lambda e: e.op_lfr_cmvn_pad([rn(1, 33, 80), rn(2, 70, 80), rn(3, 0, 80)]))
    case("argmax")(lambda e: e.op_argmax(rn(4, 33, 50)))
    case("logsoftmax_argmax")(lambda e: (e.op_logsoftmax_argmax(rn(5, 33, 50)), e.op_logsoftmax_argmax(rn(5, 33, 50), store=False)))
    case("layernorm")(lambda e: e.op_layernorm(rn(6, 33, D), *ln(7)))
    for f16 in (False, True):
        case("gemm-f16out%d" % f16)(lambda e, f16=f16: e.op_gemm(rn(8, M, K), rn(9, 128, K, scale=0.1), rn(10, 128), relu=not f16, f16_out=f16))
    for kind, blocked, tile in ((0, False, 0), (0, True, 128), (1, False, 256), (2, False, 0), (2, True, 0), (1, True, 128), (0, False, 256)):
        Kx = 192 if blocked or kind == 2 or tile else K
        case("gemm_ex-kind%d-ablk%d-tile%d" % (kind, blocked, tile))(
            lambda e, kind=kind, blocked=blocked, tile=tile, Kx=Kx: e.op_gemm_ex(
                rn(11, M, Kx), rn(12, 128, Kx, scale=0.1), rn(13, 128), resid=rn(14, M, 128) if kind == 0 else None,
                add2=rn(15, M, 128) if kind == 0 else None, relu=kind != 0, out_kind=kind, a_blocked=blocked, tile_rows=tile, scale_cols=64, scale=0.5))
    for form, f16, padded in ((7, False, True), (7, True, True), (0, False, True), (1, True, False), (2, False, False)):
        case("gemm_panel-form%d-f16%d-pad%d" % (form, f16, padded))(
            lambda e, form=form, f16=f16, padded=padded: e.op_gemm_panel(rn(16, M, D), rn(17, 516, D, scale=0.05), rn(18, 516), f16_out=f16, form=form, padded=padded))
    for blocked, short, Kx, fsmn in ((False, False, 512, True), (True, False, 2048, False), (False, True, 512, True), (False, True, 2048, False)):
        case("gemm_rc-ablk%d-short%d-K%d" % (blocked, short, Kx))(
            lambda e, blocked=blocked, short=short, Kx=Kx, fsmn=fsmn: e.op_gemm_rc(
                rn(19, M, Kx), rn(20, D, Kx, scale=0.05), rn(21, D), resid=rn(22, M, D), fsmn_v=rn(23, M, D) if fsmn else None,
                fsmn_w=rn(24, D, 11, scale=0.3) if fsmn else None, T=35 if fsmn else 0, ln=ln(25), a_blocked=blocked, short_input=short))
    case("ffn")(lambda e: e.op_ffn(rn(26, M, 128), rn(27, 256, 128, scale=0.1), rn(28, 256), rn(29, 128, 256, scale=0.1), rn(30, 128), rn(31, M, 128)))
    w1, b1, w2, b2 = (lambda: rn(32, F, D, scale=0.05)), (lambda: rn(33, F)), (lambda: rn(34, D, F, scale=0.03)), (lambda: rn(35, D))
    case("ffn_fused")(lambda e: e.op_ffn_fused(rn(36, M, D), w1(), b1(), w2(), b2(), resid=rn(37, M, D), ln=ln(38)))
    for tail in (False, True):
        case("attn_ffn_fused-qkv%d" % tail)(lambda e, tail=tail: e.op_attn_ffn_fused(
            rn(39, M, D), rn(40, D, D, scale=0.05), rn(41, D), rn(42, M, D), rn(43, D, 11, scale=0.3), 35, ln(44), w1(), b1(), w2(), b2(),
            resid=rn(45, M, D), ln=ln(46), qkv=(rn(47, 3 * D, D, scale=0.05), rn(48, 3 * D)) if tail else None))
    for splits, op in ((0, False), (2, True)):
        case("dec_ffn_fused-splits%d-outproj%d" % (splits, op))(lambda e, splits=splits, op=op: e.op_dec_ffn_fused(
            rn(49, M, D), w1(), b1(), ln(50, F), w2(), ln=ln(52), splits=splits,
            out_proj=(rn(53, M, D), rn(54, D, D, scale=0.05), rn(55, D), rn(56, M, D), ln(57)) if op else None))
    for form in (0, 1, 2):
        case("dec_mid-form%d" % form)(lambda e, form=form: e.op_dec_mid(
            rn(58, M, D), w1(), b1(), ln(59, F), w2(), ln(61), rn(62, 11, D, scale=0.3), [20, 35], rn(63, 2, 35, D), ln(64),
            rn(65, D, D, scale=0.05), rn(66, D), form=form))
    case("fsmn_enc")(lambda e: e.op_fsmn_enc(rn(67, 2, 35, D), rn(68, D, 11, scale=0.3)))
    case("fsmn_dec")(lambda e: e.op_fsmn_dec(rn(69, 2, 35, D), rn(70, D, 11, scale=0.3), [20, 35], rn(71, 2, 35, D)))
    for k in (11, 21):
        case("fsmn_dec_ln-k%d" % k)(lambda e, k=k: e.op_fsmn_dec_ln(rn(72, 2, 35, D), rn(73, k, D, scale=0.3), [0, 33], rn(74, 2, 35, D), ln(75)))
    case("fsmn")(lambda e: e.op_fsmn(rn(76, 2, 35, D), rn(77, D, 11, scale=0.3), mask=(np.arange(70).reshape(2, 35) % 35 < 30).astype(f32)))
    case("layernorm_ex")(lambda e: e.op_layernorm_ex(rn(78, 33, D), *ln(79), ld16=520, ld32=516))
    case("layernorm_ex-posenc")(lambda e: e.op_layernorm_ex(rn(80, 2, 17, e.feat_dim), *ln(81, e.feat_dim), want32=False, posenc_T=17))
    for inplace in (False, True):
        case("layernorm_f16-inplace%d" % inplace)(lambda e, inplace=inplace: e.op_layernorm_f16(rn(82, 33, D).astype(np.float16), *ln(83), in_place=inplace))
    case("fsmn_dec_stream")(lambda e: e.op_fsmn_dec_stream(rn(84, 2, 5, D), rn(85, 11, D, scale=0.3), [3, 5], rn(86, 2, D, 10), rn(87, 2, 5, D)))
    case("embed_gather")(lambda e: e.op_embed_gather(rn(88, 50, D), np.random.default_rng(89).integers(0, 50, 33)))
    case("add_to_f16")(lambda e: e.op_add_to_f16(rn(90, 33, D), rn(91, 33, D)))
    case("seaco_merge")(lambda e: e.op_seaco_merge(rn(92, 33, 52), np.random.default_rng(93).integers(1 << 40, 1 << 41, 33), 50, 25, 1, rn(94, 33, 56),
                                                   np.random.default_rng(95).integers(0, 50, 33)))
    for form in range(5):
        case("lstm-form%d" % form, 3 if form >= 3 else 0)(lambda e, form=form: e.op_lstm(rn(96, 2, 5, 2 * 4 * D), rn(97, 2, 4 * D, D, scale=0.05), 2, form))
    case("us_peak")(lambda e: e.op_us_peak(rn(98, 2, 9, D), rn(99, D, scale=0.05), 0.1, 1.0, 0.0, [3, 5], 1.0))
    case("attention")(lambda e: e.op_attention(rn(100, 2, 33, D), rn(101, 2, 40, D), rn(102, 2, 40, D)))
    for kind, layout in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)):
        Lk = 33 if layout in (1, 3) else 40
        case("attention_ex-kind%d-layout%d" % (kind, layout), 3 if kind else 0)(lambda e, kind=kind, layout=layout, Lk=Lk: e.op_attention_ex(
            rn(103, 2, 33, D), rn(104, 2, Lk, D), rn(105, 2, Lk, D), kind=kind, layout=layout, o_ld=520, ldkv=1040 if layout == 2 else 0,
            kv_off=8 if layout == 2 else 0, want_range=kind == 0))
    case("qkv_attention")(lambda e: e.op_qkv_attention(rn(106, 3 * 77, 560), rn(107, 1536, 560, scale=0.04), rn(108, 1536), 3, 77))
    case("cif")(lambda e: e.op_cif(rn(109, 2, 33, D), np.abs(rn(110, 2, 34, scale=0.3))))
    case("cif_alphas")(lambda e: e.op_cif_alphas(rn(111, 2, 33, D)))
    # the fp32 graph's ops, on the fp32 matrix path (math_mode 1) and as x3 products (math_mode 3)
    for mode in (1, 3):
        t = "-mode%d" % mode
        case("linear32" + t, mode)(lambda e: e.op_linear32(rn(112, M, K), rn(113, 130, K, scale=0.1), rn(114, 130), resid=rn(115, M, 130), relu=True))
        case("ffn32" + t, mode)(lambda e: e.op_ffn32(rn(116, M, 128), rn(117, 256, 128, scale=0.1), rn(118, 256), rn(119, 128, 256, scale=0.1), rn(120, 128)))
        for alias in (False, True):
            case("linear32_ex-alias%d" % alias + t, mode)(lambda e, alias=alias: e.op_linear32_ex(
                rn(121, M, K), rn(122, 130, K, scale=0.1), rn(123, 130), resid=rn(124, M, 130), ldc=136, resid_aliases_out=alias, relu=True))
        case("split_x3" + t, mode)(lambda e: e.op_split_x3(rn(126, 33, K), 256))
        for pair, W in ((False, False), (True, False), (False, True)):
            case("layernorm32-pair%d-W%d" % (pair, W) + t, mode)(lambda e, pair=pair, W=W: e.op_layernorm32(
                rn(127, M, D), *ln(128), direct_pair=pair, W=rn(130, 130, D, scale=0.05) if W else None, bias=rn(131, 130) if W else None))
        case("ffn32_ex" + t, mode)(lambda e: e.op_ffn32_ex(rn(132, M, 128), rn(133, 256, 128, scale=0.1), rn(134, 256), rn(135, 128, 256, scale=0.1), rn(136, 128),
                                                           hidden_scale=0.5))
        case("qkv32" + t, mode)(lambda e: e.op_qkv32(rn(137, M, K), rn(138, 3 * 128, K, scale=0.1), rn(139, 3 * 128), 0.25))
    # the int8 path's ops
    u8 = lambda seed, *shape: np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)
    for xf, fr in ((False, False), (True, True)):
        case("qlinear-xf16%d-f16res%d" % (xf, fr))(lambda e, xf=xf, fr=fr: e.op_qlinear(rn(140, M, K), rn(141, 128, K, scale=0.1), rn(142, 128), relu=True, x_is_f16=xf,
                                                                                       details=True, f16_result=fr))
    case("quantize")(lambda e: e.op_quantize(rn(143, 33, K), ldx=K + 4, ld=K + 8))
    case("quantize-f16")(lambda e: e.op_quantize(rn(144, 33, K), x_is_f16=True, ldx=K + 4, ld=K + 8))
    case("quantize-ln")(lambda e: e.op_quantize(rn(145, 33, K), ld=K + 8, ln=ln(146, K)))
    case("quantize_weight")(lambda e: e.op_quantize_weight(rn(147, 33, K), ld=K + 8))
    case("import_weight")(lambda e: e.op_import_weight(u8(148, 33, K), u8(149, 33), np.abs(rn(150, 33, scale=0.01)) + 1e-4, ld=K + 8))
    for kind in range(4):
        case("qgemm_ex-kind%d" % kind)(lambda e, kind=kind: e.op_qgemm_ex(
            u8(151, M, K), 0.02, 117, u8(152, 130, K), np.random.default_rng(153).integers(0, 256, 130), np.abs(rn(154, 130, scale=0.01)) + 1e-4, bias=rn(155, 130),
            resid=rn(156, M, 130) if kind == 0 else None, relu=kind == 1, out_kind=kind, want_range=kind in (1, 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("package_dir", nargs="?", default=HERE)
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_dir))
    import numpy as np
    import aliparaformerasr_amd
    from aliparaformerasr_amd import weights as W
    from aliparaformerasr_amd import _native as N
    from aliparaformerasr_amd.engine import Engine
    print(json.dumps({"package": os.path.dirname(os.path.abspath(aliparaformerasr_amd.__file__))}), flush=True)

    cfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=64)
    pfw = W.pack_pfw(cfg, W.synth_weights(cfg, seed=11))
    todo = cases(np)
    engines = {}
    for name, (mode, fn) in todo.items():
        if args.only and name not in args.only:
            continue
        if mode not in engines:
            engines[mode] = Engine(weights=pfw, cmvn=W.synth_cmvn(), device=0, math_mode=mode)
            engines[mode].profile(True)
        eng = engines[mode]
        eng.profile_reset()
        try:
            rec = {"sha1": digest(fn(eng))}
        except N.PfError as err:
            rec = {"error_code": int(err.code)}
            print("%s: %s" % (name, err), file=sys.stderr)
        rec["launches"] = {}
        for c in CLASSES:
            try:
                n = eng.profile_get(c)[1]
            except N.PfError:                                   # a class this engine never opened
                n = 0
            if n:
                rec["launches"][c] = n
        print(json.dumps({"case": name, **rec}, sort_keys=True), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
