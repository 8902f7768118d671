"""ctypes binding of libparaformer_hip.so (include/paraformer_hip.h).

The library is the product; this module only declares its entry points.  There is
no CPU fallback: if the shared object is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libparaformer_hip.so")

PF_OK = 0
PF_ERR_INVALID_ARG = -1
PF_ERR_DEVICE = -2
PF_ERR_IO = -3
PF_ERR_FORMAT = -4
PF_ERR_CAPACITY = -5
PF_ERR_UNSUPPORTED = -6
PF_ERR_DISPOSED = -7
PF_ERR_TOKENS = -8
PF_ERR_NULL_SAMPLES = -9
PF_ERR_RECOGNITION = -10

# pf_engine_set_decode / pf_recognizer_set_decode
PF_DECODE_SCORES = 1
PF_DECODE_CTC = 2
PF_DECODE_TOPK = 8
PF_DECODE_CTC_BEAM = 16
PF_HOTWORD_STATES_MAX = 4096
PF_HOTWORD_LEN_MAX = 64
PF_HOTWORD_TABLE_BYTES_MAX = 16 * 1024 * 1024
PF_LM_ORDER_MAX = 8
PF_LM_IMAGE_BYTES_MAX = 1024 * 1024 * 1024
PF_LM_EOS = 1
PF_DECODE_ALIGN = 32
PF_ALIGN_MAX_TOKENS = 1023
PF_TOPK_MAX = 8
PF_NBEST_MAX = 64

# PCM intake (pf_pcm_format, pf_pcm_desc.flags)
PF_PCM_U8, PF_PCM_S16, PF_PCM_S24, PF_PCM_S32, PF_PCM_F32, PF_PCM_F64, PF_PCM_ALAW, PF_PCM_MULAW = range(1, 9)
PF_PCM_DOWNMIX_ALWAYS = 1
# name -> (pf_pcm_format, bytes per value, numpy dtype a caller's array must have; 24-bit values travel as bytes)
PCM_FORMATS = {"u8": (PF_PCM_U8, 1, "u1"), "s16": (PF_PCM_S16, 2, "<i2"), "s24": (PF_PCM_S24, 3, "u1"),
               "s32": (PF_PCM_S32, 4, "<i4"), "f32": (PF_PCM_F32, 4, "<f4"), "f64": (PF_PCM_F64, 8, "<f8"),
               "alaw": (PF_PCM_ALAW, 1, "u1"), "mulaw": (PF_PCM_MULAW, 1, "u1")}


class PfPcmDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("format", C.c_int32), ("sample_rate", C.c_int32), ("channels", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class PfVadConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "floor_pct", "margin_q", "abs_level", "window", "on_count", "off_count",
                                         "pad_begin", "pad_end", "min_speech", "max_len", "split_search")] + \
               [("reserved", C.c_int32 * 4)]


class PfOnlineToken(C.Structure):
    """pf_online_token (paraformer_hip.h "Streaming token times and scores")"""
    _fields_ = [("id", C.c_int64), ("time_ms", C.c_int32), ("entry", C.c_int32), ("score", C.c_float), ("flags", C.c_int32)]


PF_ONLINE_TOKEN_FIRED = 1
PF_ONLINE_TOKEN_TIMED = 2


class PfEndpointConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "rise", "margin_q", "abs_level", "window", "on_count", "off_count",
                                         "pad_begin", "pad_end", "end_silence", "min_speech", "max_len")] + \
               [("reserved", C.c_int32 * 4)]


class PfSpkConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("win", C.c_int32), ("shift", C.c_int32), ("min_frames", C.c_int32), ("threshold", C.c_float),
                ("num_speakers", C.c_int32), ("min_cluster", C.c_int32), ("reserved", C.c_int32 * 5)]


PF_SPK_MAX_FRAMES = 512
PF_SPK_MAX_WINDOWS = 8192
PF_VAD_MAX_SEGMENTS = 65536
PF_VAD_MAX_FRAMES = 1 << 22
PF_ENDPOINT_STATE_INTS = 16
PF_ENDPOINT_MAX_STREAM_FRAMES = 1 << 30
PF_ENDPOINT_SILENCE, PF_ENDPOINT_FORCED, PF_ENDPOINT_FLUSH = 1, 2, 3


class PfAttnDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("layout", C.c_int32), ("shared_kv", C.c_int32),
                ("o_ld", C.c_int32), ("form", C.c_int32), ("ldkv", C.c_int32), ("kv_off", C.c_int32)]


PF_ATTN_CANARY = 0x4D2B


def pcm_desc(sample_rate, channels=1, format="s16", downmix_always=False) -> "PfPcmDesc":
    fmt = PCM_FORMATS[format][0] if isinstance(format, str) else int(format)
    return PfPcmDesc(C.sizeof(PfPcmDesc), fmt, int(sample_rate), int(channels), PF_PCM_DOWNMIX_ALWAYS if downmix_always else 0)


def pcm_bytes(data, format="s16"):
    """bytes / bytearray / memoryview, or a numpy array of the format's dtype -> (contiguous uint8 array, n_values)."""
    import numpy as np
    _code, bps, dt = PCM_FORMATS[format] if isinstance(format, str) else \
        next(v for v in PCM_FORMATS.values() if v[0] == int(format))
    if isinstance(data, np.ndarray):
        if data.dtype != np.dtype(dt):
            raise TypeError("PCM format %s takes a numpy array of dtype %s (or bytes), not %s" % (format, np.dtype(dt), data.dtype))
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        raw = np.frombuffer(data, np.uint8)
    return raw, raw.size // bps


class PfEngineConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32),
        ("weights_path", C.c_char_p), ("weights_host", C.c_void_p), ("weights_device", C.c_void_p),
        ("weights_bytes", C.c_int64),
        ("mvn_path", C.c_char_p), ("cmvn_shift", C.POINTER(C.c_float)), ("cmvn_scale", C.POINTER(C.c_float)),
        ("cmvn_dim", C.c_int32),
        ("fs", C.c_int32), ("n_mels", C.c_int32), ("lfr_m", C.c_int32), ("lfr_n", C.c_int32),
        ("snip_edges", C.c_int32), ("dither", C.c_float), ("window", C.c_char_p), ("use_itn", C.c_int32),
        ("frame_length_ms", C.c_int32), ("frame_shift_ms", C.c_int32), ("dither_seed", C.c_int32),
        ("math_mode", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


class PfGemmDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("relu", C.c_int32), ("out_kind", C.c_int32), ("a_blocked", C.c_int32), ("tile_rows", C.c_int32),
        ("scale_cols", C.c_int32), ("scale", C.c_float),
        ("bias", C.POINTER(C.c_float)), ("resid", C.POINTER(C.c_float)), ("add2", C.POINTER(C.c_float)),
    ]


class PfLinear32Desc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldw", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32),
        ("resid_aliases_out", C.c_int32), ("relu", C.c_int32), ("scale_cols", C.c_int32), ("scale", C.c_float), ("flags", C.c_int32),
        ("bias", C.POINTER(C.c_float)), ("resid", C.POINTER(C.c_float)), ("resid2", C.POINTER(C.c_float)),
    ]


class PfQgemmDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("relu", C.c_int32), ("out_kind", C.c_int32), ("tile_rows", C.c_int32), ("want_range", C.c_int32),
        ("scale_cols", C.c_int32), ("scale", C.c_float), ("a_scale", C.c_float), ("a_zp", C.c_int32),
        ("w_zp", C.POINTER(C.c_int32)), ("w_scale", C.POINTER(C.c_float)),
        ("bias", C.POINTER(C.c_float)), ("resid", C.POINTER(C.c_float)), ("add2", C.POINTER(C.c_float)),
    ]


class PfGemmRcDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("M", C.c_int32), ("K", C.c_int32), ("a_blocked", C.c_int32), ("T", C.c_int32),
        ("fsmn_k", C.c_int32),
        ("bias", C.POINTER(C.c_float)), ("resid", C.POINTER(C.c_float)), ("fsmn_v", C.POINTER(C.c_float)),
        ("fsmn_w", C.POINTER(C.c_float)), ("ln_gamma", C.POINTER(C.c_float)), ("ln_beta", C.POINTER(C.c_float)),
        ("short_input", C.c_int32), ("split_k", C.c_int32),
    ]


class PfBatchOut(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("l_cap", C.c_int32), ("logits_cap", C.c_int64), ("cif_peak_cap", C.c_int64),
        ("token_ids", C.POINTER(C.c_int64)), ("token_num", C.POINTER(C.c_int32)),
        ("logits", C.POINTER(C.c_float)), ("cif_peak", C.POINTER(C.c_float)),
        ("L", C.c_int32), ("V", C.c_int32), ("cif_peak_len", C.c_int32), ("reserved", C.c_int32),
    ]


# name -> (restype, argtypes); kept in one table so tests can check that every symbol the
# header declares is exported.
_P = C.POINTER
_vp = C.c_void_p
_f = _P(C.c_float)
_i32 = _P(C.c_int32)
_i64 = _P(C.c_int64)
_cpp = _P(C.c_char_p)
SIGNATURES = {
    "pf_version": (C.c_int, []),
    "pf_last_error": (C.c_char_p, []),
    "pf_engine_create": (C.c_int, [_P(PfEngineConfig), _P(_vp)]),
    "pf_engine_destroy": (None, [_vp]),
    "pf_engine_info": (C.c_int, [_vp, _i32, _i32, _i32, _i32]),
    "pf_frontend_num_frames": (C.c_int, [_vp, C.c_int64, _i32]),
    "pf_frontend": (C.c_int, [_vp, _f, C.c_int64, _f, C.c_int64, _i32]),
    "pf_fbank": (C.c_int, [_vp, _f, C.c_int64, _f, C.c_int64, _i32]),
    "pf_forward_feats": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, _i32, C.c_int32, _P(PfBatchOut)]),
    "pf_model_proj": (C.c_int, [_vp, _P(_f), _i32, C.c_int32, _i32, C.c_int32, _P(PfBatchOut)]),
    "pf_recognize": (C.c_int, [_vp, _P(_f), _i64, C.c_int32, _i32, C.c_int32, _P(PfBatchOut)]),
    "pf_stage_audio": (C.c_int, [_vp, _P(_f), _i64, C.c_int32]),
    "pf_pcm_num_samples": (C.c_int, [_P(PfPcmDesc), C.c_int32, C.c_int64, _i64]),
    "pf_stage_pcm": (C.c_int, [_vp, _P(_vp), _i64, _P(PfPcmDesc), C.c_int32, C.c_int32]),
    "pf_recognize_pcm": (C.c_int, [_vp, _P(_vp), _i64, _P(PfPcmDesc), C.c_int32, C.c_int32, _i32, C.c_int32, _P(PfBatchOut)]),
    "pf_op_pcm_convert": (C.c_int, [_vp, _vp, C.c_int64, _P(PfPcmDesc), _f, C.c_int64, _i64]),
    "pf_vad_default": (C.c_int, [_P(PfVadConfig)]),
    "pf_vad_segment": (C.c_int, [_vp, _P(_f), _i64, C.c_int32, _P(PfVadConfig), _i32, C.c_int32, _i32]),
    "pf_host_vad_levels": (C.c_int, [_f, C.c_int64, C.c_int32, _i32]),
    "pf_host_vad_segments": (C.c_int, [_i32, C.c_int32, C.c_int32, C.c_int32, _P(PfVadConfig), _i32, C.c_int32, _i32]),
    "pf_host_long_plan": (C.c_int, [_i32, C.c_int32, C.c_int32, C.c_int64, _i32, _i32, _i32]),
    "pf_op_vad_levels": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, _i32]),
    "pf_endpoint_default": (C.c_int, [_P(PfEndpointConfig)]),
    "pf_host_endpoint_update": (C.c_int, [_i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(PfEndpointConfig), _i32, C.c_int32,
                                          _i32, _i32, _i32]),
    "pf_op_endpoint_update": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, _P(PfEndpointConfig), _i32,
                                        C.c_int32, _i32, _i32, _i32]),
    "pf_vad_model_load": (C.c_int, [C.c_char_p, _P(_vp)]),
    "pf_vad_model_from_memory": (C.c_int, [_vp, C.c_int64, _P(_vp)]),
    "pf_vad_model_info": (C.c_int, [_vp, _i32, _i32, _i64]),
    "pf_vad_model_sil_ids": (C.c_int, [_vp, _i32, C.c_int32, _i32]),
    "pf_vad_model_tensor": (C.c_int, [_vp, C.c_char_p, _f, C.c_int64, _i64]),
    "pf_vad_model_config": (C.c_int, [_P(PfVadConfig)]),
    "pf_vad_model_free": (None, [_vp]),
    "pf_host_vad_model_logits": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, _P(C.c_double)]),
    "pf_host_vad_model_levels": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, _i32]),
    "pf_engine_set_vad_model": (C.c_int, [_vp, _vp]),
    "pf_op_vad_model_logits": (C.c_int, [_vp, _f, _i32, C.c_int32, C.c_int32, _f]),
    "pf_op_vad_model_levels": (C.c_int, [_vp, _f, _i32, C.c_int32, C.c_int32, _i32]),
    "pf_endpoint_model_config": (C.c_int, [_P(PfEndpointConfig)]),
    "pf_vad_model_stream_state_bytes": (C.c_int, [_vp, _i64]),
    "pf_host_vad_model_stream_state_bytes": (C.c_int, [_vp, _i64]),
    "pf_host_vad_model_stream": (C.c_int, [_vp, _vp, _f, C.c_int32, C.c_int32, C.c_int32, _i32, _P(C.c_double), C.c_int32, _i32]),
    "pf_op_vad_model_stream": (C.c_int, [_vp, _vp, _f, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, _i32, _f, C.c_int32, _i32]),
    "pf_punc_model_load": (C.c_int, [C.c_char_p, _P(_vp)]),
    "pf_punc_model_from_memory": (C.c_int, [_vp, C.c_int64, _P(_vp)]),
    "pf_punc_model_info": (C.c_int, [_vp, _i32, _i64]),
    "pf_punc_model_free": (None, [_vp]),
    "pf_spk_model_load": (C.c_int, [C.c_char_p, _P(_vp)]),
    "pf_spk_model_from_memory": (C.c_int, [_vp, C.c_int64, _P(_vp)]),
    "pf_spk_model_info": (C.c_int, [_vp, _i32, _i64]),
    "pf_spk_model_free": (None, [_vp]),
    "pf_spk_default": (C.c_int, [_P(PfSpkConfig)]),
    "pf_engine_set_spk_model": (C.c_int, [_vp, _vp]),
    "pf_host_spk_windows": (C.c_int, [_i32, C.c_int32, _P(PfSpkConfig), _i32, C.c_int32, _i32, _i32]),
    "pf_host_spk_cluster": (C.c_int, [_f, C.c_int32, _P(PfSpkConfig), _i32, _i32]),
    "pf_host_spk_segment_labels": (C.c_int, [_i32, C.c_int32, _i32, _i32, C.c_int32, _i32]),
    "pf_host_spk_centroids": (C.c_int, [_f, _i32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_spk_embed": (C.c_int, [_vp, _f, _i32, C.c_int32, C.c_int32, _f, _f]),
    "pf_op_spk_affinity": (C.c_int, [_vp, _f, _i32, C.c_int32, C.c_int32, _f]),
    "pf_host_punc_words": (C.c_int, [_vp, C.c_char_p, _i32, _i32, _i32, C.c_int32, _i32]),
    "pf_host_punc_logits": (C.c_int, [_vp, _i32, C.c_int32, _P(C.c_double)]),
    "pf_host_punc_cut": (C.c_int, [_vp, _i32, C.c_int32, C.c_int32, _i32]),
    "pf_host_punc_ids": (C.c_int, [_vp, _i32, C.c_int64, _i32, _i32, _i32, C.c_int32, _i32]),
    "pf_host_punc_assemble": (C.c_int, [_vp, C.c_char_p, _i32, C.c_int32, C.c_char_p, C.c_int64, _i64, _i32, C.c_int32, _i32]),
    "pf_host_punc_text": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_int64, _i64, _i32, C.c_int32, _i32]),
    "pf_engine_set_punc_model": (C.c_int, [_vp, _vp]),
    "pf_engine_punctuate": (C.c_int, [_vp, _i32, _i32, C.c_int32, _i32, _i32]),
    "pf_op_punc_logits": (C.c_int, [_vp, _i32, _i32, C.c_int32, _f, _f]),
    "pf_op_punc_window": (C.c_int, [_vp, _i32, _i32, _i32, C.c_int32, _i32, _i32, _f]),
    "pf_punc_model_causal": (C.c_int, [_vp, _i32]),
    "pf_punc_stream_state_bytes": (C.c_int, [_vp, _i64]),
    "pf_host_punc_stream_state_bytes": (C.c_int, [_vp, _i64]),
    "pf_host_punc_stream_step": (C.c_int, [_vp, _vp, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _P(C.c_double), _i32]),
    "pf_host_online_committed_words": (C.c_int, [_vp, _P(C.c_char_p), C.c_int32, _i64, C.c_int32, C.c_char_p, C.c_char_p, C.c_int64, _i64, _i32, _i32]),
    "pf_online_recognizer_set_punc_model": (C.c_int, [_vp, C.c_char_p, C.c_int32]),
    "pf_online_stream_punctuated": (C.c_int, [_vp, _cpp, _P(_i32), _P(_i32), _i32]),
    "pf_online_stream_sentence_punctuated": (C.c_int, [_vp, C.c_int32, _cpp, _P(_i32), _i32]),
    "pf_op_punc_stream_step": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _f, _i32]),
    "pf_op_vad_segments": (C.c_int, [_vp, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, _P(PfVadConfig), _i32, C.c_int32, _i32]),
    "pf_stream_add_pcm": (C.c_int, [_vp, _vp, C.c_int64, _P(PfPcmDesc)]),
    "pf_host_wav_info": (C.c_int, [C.c_char_p, _P(PfPcmDesc), _i64, _i64, C.POINTER(C.c_double)]),
    "pf_engine_set_hotwords": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int32]),
    "pf_run_staged": (C.c_int, [_vp]),
    "pf_host_wav_read": (C.c_int, [C.c_char_p, _f, C.c_int64, _i64, _i32, _i32, C.POINTER(C.c_double)]),
    "pf_host_resample": (C.c_int, [_f, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f, C.c_int64, _i64]),
    "pf_host_is_audio": (C.c_int, [C.c_char_p, _i32]),
    "pf_group_create": (C.c_int, [_P(PfEngineConfig), _i32, C.c_int32, _P(_vp)]),
    "pf_group_destroy": (None, [_vp]),
    "pf_group_info": (C.c_int, [_vp, _i32, _i32]),
    "pf_group_engine": (_vp, [_vp, C.c_int32]),
    "pf_group_recognize": (C.c_int, [_vp, _P(_f), _i64, C.c_int32, _i32, C.c_int32, _P(PfBatchOut)]),
    "pf_group_fetch": (C.c_int, [_vp, _P(PfBatchOut)]),
    "pf_sync": (C.c_int, [_vp]),
    "pf_fetch": (C.c_int, [_vp, _P(PfBatchOut)]),
    "pf_fetch_ids_device": (C.c_int, [_vp, _vp, C.c_int32, _i32]),
    "pf_engine_set_decode": (C.c_int, [_vp, C.c_int32]),
    "pf_fetch_scores": (C.c_int, [_vp, _f, C.c_int64, _i32]),
    "pf_fetch_ctc": (C.c_int, [_vp, _i64, _i32, _i32, _f, C.c_int32, _i32, _i32]),
    "pf_op_ctc_collapse": (C.c_int, [_vp, _i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, _i64, _i32, _i32, _f, C.c_int32, _i32]),
    "pf_recognizer_set_decode": (C.c_int, [_vp, C.c_int32]),
    "pf_engine_set_topk": (C.c_int, [_vp, C.c_int32]),
    "pf_fetch_topk": (C.c_int, [_vp, _i64, _f, _i32, C.c_int64, _i32, _i32]),
    "pf_op_topk": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _i64, _f, _i32]),
    "pf_host_nbest": (C.c_int, [_i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _P(C.c_double), _i32]),
    "pf_recognizer_set_nbest": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "pf_engine_set_ctc_beam": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "pf_fetch_ctc_beam": (C.c_int, [_vp, _i64, _i32, _P(C.c_double), C.c_int32, _i32, _i32]),
    "pf_host_ctc_beam": (C.c_int, [_f, C.c_int64, _i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64, _i32,
                                   _P(C.c_double), C.c_int32, _i32]),
    "pf_op_ctc_beam": (C.c_int, [_vp, _f, _i64, _f, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 _i64, _i32, _P(C.c_double), C.c_int32, _i32]),
    "pf_recognizer_set_ctc_beam": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32]),
    "pf_host_hotword_graph": (C.c_int, [_i32, _i32, C.c_int32, C.c_int32, _i32, _i32, _i32, _i32, C.c_int64, _i32, C.c_int32]),
    "pf_engine_set_ctc_hotwords": (C.c_int, [_vp, _i32, _i32, C.c_int32, C.c_float]),
    "pf_fetch_ctc_beam_hot": (C.c_int, [_vp, _i32, _P(C.c_double)]),
    "pf_host_ctc_beam_hot": (C.c_int, [_f, C.c_int64, _i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64, _i32,
                                       _P(C.c_double), C.c_int32, _i32, _i32, _i32, C.c_int32, C.c_float, _i32, _P(C.c_double)]),
    "pf_op_ctc_beam_hot": (C.c_int, [_vp, _f, _i64, _f, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     _i64, _i32, _P(C.c_double), C.c_int32, _i32, _i32, _i32, C.c_int32, C.c_float, _i32,
                                     _P(C.c_double)]),
    "pf_host_lm_build": (C.c_int, [C.c_int32, _i64, _i32, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _i32, C.c_int32,
                                   _P(_vp)]),
    "pf_host_lm_from_arpa": (C.c_int, [C.c_char_p, _cpp, C.c_int32, C.c_float, _i64, _P(_vp)]),
    "pf_host_lm_info": (C.c_int, [_vp, _i32, _i64, _i64, _i64]),
    "pf_host_lm_score": (C.c_int, [_vp, _i32, C.c_int32, C.c_float, C.c_float, C.c_int32, _P(C.c_double), _i32, _P(C.c_double), _i32]),
    "pf_lm_free": (None, [_vp]),
    "pf_engine_set_ctc_lm": (C.c_int, [_vp, _vp, C.c_float, C.c_float, C.c_int32]),
    "pf_fetch_ctc_beam_lm": (C.c_int, [_vp, _P(C.c_double), _P(C.c_double)]),
    "pf_host_ctc_beam_lm": (C.c_int, [_f, C.c_int64, _i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64, _i32,
                                      _P(C.c_double), C.c_int32, _i32, _i32, _i32, C.c_int32, C.c_float, _i32, _P(C.c_double), _vp,
                                      C.c_float, C.c_float, C.c_int32, _P(C.c_double)]),
    "pf_op_ctc_beam_lm": (C.c_int, [_vp, _f, _i64, _f, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    _i64, _i32, _P(C.c_double), C.c_int32, _i32, _i32, _i32, C.c_int32, C.c_float, _i32,
                                    _P(C.c_double), _vp, C.c_float, C.c_float, C.c_int32, _P(C.c_double)]),
    "pf_engine_set_nbest_search": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "pf_engine_set_nbest_lm": (C.c_int, [_vp, _vp, C.c_float, C.c_float, C.c_int32]),
    "pf_engine_set_nbest_hotwords": (C.c_int, [_vp, _i32, _i32, C.c_int32, C.c_float]),
    "pf_fetch_nbest_search": (C.c_int, [_vp, _i32, _P(C.c_double), _P(C.c_double), _P(C.c_double), _i32, _i32, _i32, _i32]),
    "pf_host_nbest_search": (C.c_int, [_i64, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, C.c_int32,
                                       C.c_float, _vp, C.c_float, C.c_float, C.c_int32, _i32, _P(C.c_double), _P(C.c_double),
                                       _P(C.c_double), _i32, _i32]),
    "pf_op_nbest_search": (C.c_int, [_vp, _i64, _f, _i32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _i32,
                                     C.c_int32, C.c_float, _vp, C.c_float, C.c_float, C.c_int32, _i32, _P(C.c_double), _P(C.c_double),
                                     _P(C.c_double), _i32, _i32]),
    "pf_op_lm_score": (C.c_int, [_vp, _vp, _i32, _i32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P(C.c_double), _i32]),
    "pf_recognizer_set_vad": (C.c_int, [_vp, _P(PfVadConfig), C.c_int32, C.c_int64, C.c_char_p]),
    "pf_recognizer_set_vad_model": (C.c_int, [_vp, C.c_char_p]),
    "pf_recognizer_set_punc_model": (C.c_int, [_vp, C.c_char_p]),
    "pf_recognizer_set_spk_model": (C.c_int, [_vp, C.c_char_p, _P(PfSpkConfig)]),
    "pf_stream_num_speakers": (C.c_int, [_vp, _i32]),
    "pf_stream_segment_speaker": (C.c_int, [_vp, C.c_int32, _i32]),
    "pf_stream_speaker_centroid": (C.c_int, [_vp, C.c_int32, _f, C.c_int32, _i32]),
    "pf_stream_num_spk_windows": (C.c_int, [_vp, _i32]),
    "pf_stream_spk_window": (C.c_int, [_vp, C.c_int32, _i32, _i32, _i32]),
    "pf_stream_punctuated": (C.c_int, [_vp, _cpp, _P(_i32), _i32]),
    "pf_stream_num_sentences": (C.c_int, [_vp, _i32]),
    "pf_stream_sentence": (C.c_int, [_vp, C.c_int32, _i32, _i32, _i32, _i32, _i32, _cpp]),
    "pf_stream_num_segments": (C.c_int, [_vp, _i32]),
    "pf_stream_segment": (C.c_int, [_vp, C.c_int32, _i32, _i32, _i32, _i32, _i32, _i32, _cpp]),
    "pf_recognizer_set_hotword_boost": (C.c_int, [_vp, C.c_float]),
    "pf_stream_alternative_hot": (C.c_int, [_vp, C.c_int32, _i32, _P(C.c_double)]),
    "pf_recognizer_set_lm": (C.c_int, [_vp, C.c_char_p, C.c_float, C.c_float, C.c_int32]),
    "pf_stream_alternative_lm": (C.c_int, [_vp, C.c_int32, _P(C.c_double), _P(C.c_double)]),
    "pf_recognizer_set_nbest_search": (C.c_int, [_vp, C.c_int32]),
    "pf_recognizer_set_nbest_lm": (C.c_int, [_vp, C.c_char_p, C.c_float, C.c_float, C.c_int32]),
    "pf_recognizer_set_nbest_hotword_boost": (C.c_int, [_vp, C.c_float]),
    "pf_engine_set_align_targets": (C.c_int, [_vp, _i64, _i32, C.c_int32, C.c_int32]),
    "pf_fetch_align": (C.c_int, [_vp, _f, _P(C.c_double), _i32, _i32, _i32, _i32, _f, C.c_int32, _i32, _i32]),
    "pf_host_ctc_align": (C.c_int, [_f, C.c_int64, C.c_int32, C.c_int32, _i64, C.c_int32, _f, _P(C.c_double), _i32, _i32, _i32, _f]),
    "pf_op_ctc_align": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _i32, C.c_int32, C.c_int32,
                                  _f, _P(C.c_double), _i32, _i32, _i32, _f]),
    "pf_recognizer_set_align": (C.c_int, [_vp, C.c_int32]),
    "pf_stream_set_align_ids": (C.c_int, [_vp, _i64, C.c_int32]),
    "pf_stream_alignment": (C.c_int, [_vp, _P(_i32), _P(_f), _i32, _f, _P(C.c_double), _i32]),
    "pf_stream_alternative_timestamps": (C.c_int, [_vp, C.c_int32, _P(_i32), _i32, _P(C.c_double)]),
    "pf_stream_token_alternatives": (C.c_int, [_vp, _P(_i64), _P(_f), _i32, _i32]),
    "pf_stream_num_alternatives": (C.c_int, [_vp, _i32]),
    "pf_stream_alternative": (C.c_int, [_vp, C.c_int32, _P(_i64), _i32, _P(C.c_double), _P(C.c_char_p), _i32]),
    "pf_stream_alternative_token": (C.c_int, [_vp, C.c_int32, C.c_int32, _P(C.c_char_p)]),
    "pf_stream_scores": (C.c_int, [_vp, _P(_f), _i32]),
    "pf_host_group_sim": (C.c_int, [C.c_int32, C.c_int32, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64,
                                    C.c_int32, _i32, _i32]),
    "pf_profile_enable": (C.c_int, [_vp, C.c_int32]),
    "pf_profile_reset": (C.c_int, [_vp]),
    "pf_profile_select": (C.c_int, [_vp, C.c_char_p]),
    "pf_profile_get": (C.c_int, [_vp, C.c_char_p, _P(C.c_double), _i64, _P(C.c_double)]),
    "pf_profile_kernel": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_int32]),
    "pf_last_flops": (C.c_int, [_vp, _P(C.c_double)]),
    "pf_op_lfr_cmvn_pad": (C.c_int, [_vp, _P(_f), _i32, C.c_int32, C.c_int32, _f, C.c_int64, _i32]),
    "pf_op_fbank_batch": (C.c_int, [_vp, _P(_f), _i64, C.c_int32, _f, C.c_int64, _i32]),
    "pf_op_qlinear": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f, _P(C.c_uint8), _f,
                                _P(C.c_uint8), _f, _i32]),
    "pf_op_quantize": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f, _f, _P(C.c_int8), _i32, _f]),
    "pf_op_quantize_weight": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int8), _i32, _i32, _f, _i32]),
    "pf_op_import_weight": (C.c_int, [_vp, _P(C.c_uint8), _P(C.c_uint8), _f, C.c_int32, C.c_int32, C.c_int32, _P(C.c_int8), _i32, _i32,
                                      _f, _i32]),
    "pf_op_qgemm_ex": (C.c_int, [_vp, _P(PfQgemmDesc), _P(C.c_uint8), _P(C.c_uint8), _f, _f, _f]),
    "pf_op_argmax": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, _i64]),
    "pf_op_gemm": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_gemm_ex": (C.c_int, [_vp, _P(PfGemmDesc), _f, _f, _f]),
    "pf_op_gemm_panel": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f, _f]),
    "pf_op_gemm_rc": (C.c_int, [_vp, _P(PfGemmRcDesc), _f, _f, _f, _f, _f]),
    "pf_op_ffn": (C.c_int, [_vp, _f, _f, _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_ffn_fused": (C.c_int, [_vp, _f, _f, _f, _f, _f, _f, _f, _f, C.c_int32, _f, _f]),
    "pf_op_dec_ffn_fused": (C.c_int, [_vp, C.c_void_p, _f, _f, _f]),
    "pf_op_attn_ffn_fused": (C.c_int, [_vp, _vp, _f, _f]),
    "pf_op_dec_mid": (C.c_int, [_vp, C.c_void_p, _f, _f, _f, _f, _i32]),
    "pf_op_fsmn_dec_ln": (C.c_int, [_vp, _f, _f, _i32, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f, _f, _f]),
    "pf_op_layernorm_ex": (C.c_int, [_vp, _f, _f, _f, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_uint16), _f]),
    "pf_op_layernorm_f16": (C.c_int, [_vp, _P(C.c_uint16), _f, _f, C.c_int64, C.c_int32, C.c_int32, _P(C.c_uint16)]),
    "pf_op_fsmn_dec_stream": (C.c_int, [_vp, _f, _f, _i32, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f]),
    "pf_op_fsmn_enc_ex": (C.c_int, [_vp, _P(C.c_uint16), _f] + [C.c_int32] * 6 + [_f]),
    "pf_op_fsmn_f32_ex": (C.c_int, [_vp, _f, _f, _f] + [C.c_int32] * 7 + [_f]),
    "pf_op_fsmn_dec_ex": (C.c_int, [_vp, _f, _f, _i32] + [C.c_int32] * 5 + [_f, _f]),
    "pf_op_embed_gather": (C.c_int, [_vp, _f, _i32, C.c_int32, C.c_int32, C.c_int32, _f, _P(C.c_uint16)]),
    "pf_op_add_to_f16": (C.c_int, [_vp, _f, _f, C.c_int64, C.c_int32, _P(C.c_uint16)]),
    "pf_op_seaco_merge": (C.c_int, [_vp, _f, C.c_int32, _i64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f, C.c_int32, _i64, _f, _i64]),
    "pf_op_short_input_max_rows": (C.c_int, [_vp, _i32]),
    "pf_op_fsmn_enc": (C.c_int, [_vp, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_linear32": (C.c_int, [_vp, _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_ffn32": (C.c_int, [_vp, _f, _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_linear32_ex": (C.c_int, [_vp, _P(PfLinear32Desc), _f, _f, _f]),
    "pf_op_split_x3": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(C.c_uint16)]),
    "pf_op_layernorm32": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f, _P(C.c_uint16), _i32, _f, _f, C.c_int32, _f]),
    "pf_op_ffn32_ex": (C.c_int, [_vp, _f, _f, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float, _f, _P(C.c_uint16), _i32]),
    "pf_op_qkv32": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float, _f]),
    "pf_op_fsmn_dec": (C.c_int, [_vp, _f, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_lstm": (C.c_int, [_vp, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_us_peak": (C.c_int, [_vp, _f, _f, _f, C.c_float, C.c_float, _i32, C.c_float, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f]),
    "pf_op_logsoftmax_argmax": (C.c_int, [_vp, _f, C.c_int64, C.c_int32, _f, _i64]),
    "pf_op_layernorm": (C.c_int, [_vp, _f, _f, _f, C.c_int64, C.c_int32, _f]),
    "pf_op_attention": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_fsmn": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f]),
    "pf_op_attention_ex": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P(PfAttnDesc), _f, _vp, C.c_int64, _f,
                                     _i32]),
    "pf_op_qkv_attention": (C.c_int, [_vp, _f, _f, _f, C.c_int32, C.c_int32, C.c_int32, _f, _f, _f, _f]),
    "pf_op_cif": (C.c_int, [_vp, _f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _f, _i32, _i32, _i32]),
    "pf_op_cif_alphas": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, _f]),
    "pf_op_encoder": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, _f]),
    "pf_recognizer_create": (C.c_int, [C.c_char_p] * 6 + [C.c_int32, C.c_int32, C.c_int32, _P(_vp)]),
    "pf_recognizer_dispose": (None, [_vp]),
    "pf_recognizer_free": (None, [_vp]),
    "pf_recognizer_engine": (_vp, [_vp]),
    "pf_recognizer_create_stream": (C.c_int, [_vp, _P(_vp)]),
    "pf_stream_add_samples": (C.c_int, [_vp, _f, C.c_int64]),
    "pf_stream_set_hotwords": (C.c_int, [_vp, _i32, _i32, C.c_int32]),
    "pf_stream_get_hotwords": (C.c_int, [_vp, _i32, C.c_int32, _i32, C.c_int32, _i32]),
    "pf_stream_num_feature_floats": (C.c_int, [_vp, _i32]),
    "pf_stream_dispose": (None, [_vp]),
    "pf_stream_free": (None, [_vp]),
    "pf_recognizer_num_engines": (C.c_int, [_vp]),
    "pf_recognizer_get_results": (C.c_int, [_vp, _P(_vp), C.c_int32]),
    "pf_result_text": (C.c_int, [_vp, C.c_int32, _cpp, _i32]),
    "pf_result_num_tokens": (C.c_int, [_vp, C.c_int32, _i32]),
    "pf_result_token": (C.c_int, [_vp, C.c_int32, C.c_int32, _cpp]),
    "pf_result_timestamp": (C.c_int, [_vp, C.c_int32, C.c_int32, _P(_i32), _i32]),
    "pf_result_num_timestamps": (C.c_int, [_vp, C.c_int32, _i32]),
    "pf_stream_tokens": (C.c_int, [_vp, _P(_i64), _i32]),
    "pf_stream_create": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_char_p, _P(_vp)]),
    "pf_stream_set_tokens": (C.c_int, [_vp, _i64, C.c_int32]),
    "pf_stream_num_timestamps": (C.c_int, [_vp, _i32]),
    "pf_stream_timestamp": (C.c_int, [_vp, C.c_int32, _P(_i32), _i32]),
    "pf_stream_set_timestamps": (C.c_int, [_vp, _i32, _i32, C.c_int32]),
    "pf_stream_get_speech": (C.c_int, [_vp, _f, C.c_int64, _i32]),
    "pf_stream_set_speech": (C.c_int, [_vp, _f, C.c_int32, C.c_int32]),
    "pf_online_recognizer_create": (C.c_int, [C.c_char_p] * 5 + [C.c_int32, C.c_int32, _P(_vp)]),
    "pf_online_recognizer_dispose": (None, [_vp]),
    "pf_online_recognizer_free": (None, [_vp]),
    "pf_online_recognizer_engine": (_vp, [_vp]),
    "pf_online_create_stream": (C.c_int, [_vp, _P(_vp)]),
    "pf_online_stream_add_samples": (C.c_int, [_vp, _f, C.c_int64]),
    "pf_online_get_results": (C.c_int, [_vp, _P(_vp), C.c_int32]),
    "pf_online_result_text": (C.c_int, [_vp, C.c_int32, _cpp]),
    "pf_online_recognizer_set_endpoint": (C.c_int, [_vp, _P(PfEndpointConfig)]),
    "pf_online_recognizer_set_endpoint_model": (C.c_int, [_vp, C.c_char_p]),
    "pf_online_recognizer_set_second_pass": (C.c_int, [_vp, _vp]),
    "pf_online_stream_input_finished": (C.c_int, [_vp]),
    "pf_online_stream_num_sentences": (C.c_int, [_vp, _i32]),
    "pf_online_stream_sentence": (C.c_int, [_vp, C.c_int32, _i32, _i32, _i32, _P(C.c_char_p), _P(C.c_char_p)]),
    "pf_online_stream_sentence_result": (C.c_int, [_vp, C.c_int32, _P(_vp)]),
    "pf_online_stream_in_speech": (C.c_int, [_vp, _i32, _i32]),
    "pf_online_stream_tokens": (C.c_int, [_vp, _P(_i64), _i32]),
    "pf_online_recognizer_set_token_info": (C.c_int, [_vp, C.c_int32]),
    "pf_online_stream_token_info": (C.c_int, [_vp, _P(_P(PfOnlineToken)), _i32]),
    "pf_online_stream_sentence_tokens": (C.c_int, [_vp, C.c_int32, _P(_P(PfOnlineToken)), _i32]),
    "pf_online_stream_dispose": (None, [_vp]),
    "pf_online_stream_free": (None, [_vp]),
    "pf_online_encoder": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, _f, _f]),
    "pf_online_decoder": (C.c_int, [_vp, _f, C.c_int32, C.c_int32, _f, C.c_int32, _i32, _f, C.c_int32, _f, _i64, _f]),
    "pf_host_online_lfr": (C.c_int, [_f, C.c_int32, C.c_int32, C.c_int32, _f, C.c_int64, _i32]),
    "pf_host_online_posenc": (C.c_int, [_f, C.c_int32, C.c_int32, C.c_int32]),
    "pf_host_online_dynamic_mask": (C.c_int, [_f, C.c_int32]),
    "pf_host_online_cif": (C.c_int, [_f, _f, C.c_int32, C.c_int32, C.c_float, _f, C.c_int32, _i32, _f, _f]),
    "pf_host_online_cif_state_bytes": (C.c_int, [C.c_int32, _i64]),
    "pf_host_online_cif_step": (C.c_int, [_vp, _f, _f, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, _f, _i32, C.c_int32,
                                          _i32]),
    "pf_op_online_cif_step": (C.c_int, [_vp, _vp, _f, _f, _i32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _f, _i32,
                                        C.c_int32, _i32]),
    "pf_host_online_decode": (C.c_int, [_cpp, C.c_int32, _i64, C.c_int32, C.c_char_p, C.c_int32]),
    "pf_host_timestamps": (C.c_int, [_f, C.c_int32, _i64, C.c_int32, _i32, C.c_int32]),
    "pf_host_hotword_ids": (C.c_int, [_cpp, C.c_int32, _cpp, C.c_int32, _i32, C.c_int32, _i32, C.c_int32, _i32]),
    "pf_host_decode": (C.c_int, [_cpp, C.c_int32, _i64, C.c_int32, _i32, _i32, C.c_int32, _P(_vp)]),
    "pf_decoded_text": (C.c_int, [_vp, _cpp, _i32]),
    "pf_decoded_num_tokens": (C.c_int, [_vp, _i32]),
    "pf_decoded_token": (C.c_int, [_vp, C.c_int32, _cpp]),
    "pf_decoded_num_timestamps": (C.c_int, [_vp, _i32]),
    "pf_decoded_timestamp": (C.c_int, [_vp, C.c_int32, _P(_i32), _i32]),
    "pf_decoded_free": (None, [_vp]),
}

_lib = None


class NativeLibraryMissing(ImportError):
    pass


def load() -> C.CDLL:
    """Loads libparaformer_hip.so (built in-tree by __graft_entry__.build() / csrc/Makefile).
    Raises NativeLibraryMissing when it is absent — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build it with `make -C aliparaformerasr_amd/csrc` "
            "(or __graft_entry__.build()); this package has no CPU fallback")
    try:
        # If torch is (or will be) in the process, its bundled libamdhip64 must be the one
        # HIP runtime instance: import it first so both share one runtime.
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PfAttnFfnDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("T", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("ctx", "wo", "bo", "v", "fsmn_w", "ln2_gamma", "ln2_beta", "resid",
                                                    "w1", "b1", "w2", "b2", "ln_gamma", "ln_beta",
                                                    "wqkv", "bqkv", "q_out", "k_out", "v_out")]


class PfDecFfnDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("splits", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("x", "w1", "b1", "gamma_f", "beta_f", "w2", "ln_gamma", "ln_beta",
                                                    "ctx", "wo", "bo", "resid", "ln1_gamma", "ln1_beta")]


class PfDecMidDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "B", "L", "splits", "form", "reserved")] + \
               [(n, C.POINTER(C.c_int32) if n == "token_num" else C.POINTER(C.c_float))
                for n in ("a", "w1", "b1", "gamma_f", "beta_f", "w2", "n2_gamma", "n2_beta", "taps", "token_num", "x",
                          "n3_gamma", "n3_beta", "wq", "bq")]


class PfError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


def check(code: int) -> int:
    if code < 0:
        msg = load().pf_last_error()
        raise PfError(code, msg.decode("utf-8", "replace") if msg else "")
    return code
