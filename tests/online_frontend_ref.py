"""One stream's front-end block (csrc/decode_blocks.h FrontendStreamBlock, 80 mels x 560 columns) as numpy views, and the two entry
points that step it: pf_host_online_frontend_step (the definition) and pf_op_online_frontend_step (the kernel)."""
import ctypes as C

import numpy as np

from aliparaformerasr_amd import _native as N

F32 = np.float32
CHUNK = 9600
SENTINEL_BITS = int(np.array([-23.025850929940457], F32).view(np.uint32)[0])
_FP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def posenc(x, start_idx):
    """the position term as online.cpp adds it (libm), the way online_lockstep_ref takes it with an engine"""
    out = np.ascontiguousarray(x, dtype=F32).copy()
    N.check(N.load().pf_host_online_posenc(out.ctypes.data_as(_FP), out.shape[0], out.shape[1], start_idx))
    return out


def new_states(n):
    b = C.c_int64()
    N.check(N.load().pf_host_online_frontend_state_bytes(80, 560, b))
    assert b.value == (160 + 5600 + 12 + 4) * 4                       # carry | cache | start_idx copies | flags
    return np.zeros((n, b.value // 4), np.uint32)


def fields(block):
    """(carry [2, 80], cache [10, 560], start_idx [10], flags) of one block (a row of new_states)"""
    return (block[:160].view(F32).reshape(2, 80), block[160:5760].view(F32).reshape(10, 560), block[5760:5770].view(np.int32),
            int(block[5772]))


def host_step(block, rows, cmvn, reset):
    """block updated in place; rows [60, 80]; cmvn (shift, scale) or None -> speech [20, 560]"""
    rows = np.ascontiguousarray(rows, F32)
    sh, sc = (None, None) if cmvn is None else (np.ascontiguousarray(v, F32).ctypes.data_as(_FP) for v in cmvn)
    speech = np.zeros((20, 560), F32)
    N.check(N.load().pf_host_online_frontend_step(block.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(_FP), sh, sc, int(reset),
                                                  speech.ctypes.data_as(_FP)))
    return speech


def op_step(engine, states, slots, samples, resets):
    """states [n, words] updated in place; samples [B, 9600] -> speech [B, 20, 560]"""
    slots, resets = np.asarray(slots, np.int32), np.asarray(resets, np.int32)
    samples = np.ascontiguousarray(samples, F32)
    speech = np.zeros((len(slots), 20, 560), F32)
    N.check(N.load().pf_op_online_frontend_step(engine._h, states.ctypes.data_as(C.c_void_p), states.shape[0], slots.ctypes.data_as(_IP),
                                                samples.ctypes.data_as(_FP), resets.ctypes.data_as(_IP), len(slots),
                                                speech.ctypes.data_as(_FP)))
    return speech
