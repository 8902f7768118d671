"""CPU: the one reader of the PFW1 container (csrc/pfw.cpp) in a stand-alone program (tests/native/pfw_sanitize.cpp) built with
AddressSanitizer + UBSan on the host code: the malformed containers of test_vadnet_cpu.py, test_punc_cpu.py and
test_gpu_edges.py under each of the three caller policies.  No report, and every refusal carries the caller's own status
code: the recogniser's weights PF_ERR_FORMAT, the two models PF_ERR_INVALID_ARG."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pfw_helpers as P
import vadnet_ref
from aliparaformerasr_amd import _native as N
from aliparaformerasr_amd import weights as W


def _kinds():
    """a small container of each kind; the reader looks at no tensor name, so the recogniser's holds three small tensors"""
    pcfg = W.paraformer_large_config(enc_layers=1, dec_layers=1, vocab=16)
    pw = {"encoder.after_norm.weight": np.ones(512, np.float32), "decoder.output.weight": np.zeros((16, 512), np.float32),
          "x.weight_q": np.arange(48, dtype=np.uint8).reshape(3, 16)}
    vcfg, vw = vadnet_ref.small_model()
    ccfg = W.ct_transformer_config(vocab=64, n_layers=1)
    return {"weights": (pcfg, pw), "vad": (vcfg, vw), "punc": (ccfg, W.synth_punc_weights(ccfg, seed=5))}


def _malformed(cfg, w):
    good = W.pack_pfw(cfg, w)
    hdr, base = P.split(good)
    hlen = struct.unpack_from("<Q", good, 8)[0]
    end = base + max(t["offset"] + t["nbytes"] for t in hdr["tensors"])
    assert end <= len(good)

    def far(h): h["tensors"][1]["offset"] = 1 << 40
    def big(h): h["tensors"][-1]["nbytes"] = h["tensors"][-1]["nbytes"] + 4096
    def neg(h): h["tensors"][0]["offset"] = -256
    def frac(h): h["tensors"][1]["offset"] = 256.5
    def mism(h): h["tensors"][1]["shape"] = [h["tensors"][1]["shape"][0] + 1] + h["tensors"][1]["shape"][1:]
    def negdim(h): h["tensors"][0]["shape"][0] = -h["tensors"][0]["shape"][0]
    def dtype(h): h["tensors"][1]["dtype"] = "i4"
    def noshape(h): del h["tensors"][0]["shape"]
    def noconfig(h): del h["config"]
    def config_list(h): h["config"] = [1, 2]
    def tensors_obj(h): h["tensors"] = {"a": 1}
    # a shape whose running product passes 2^63 at the third factor: refused before the multiplication, not after it wrapped
    def overflow(h): h["tensors"][0]["shape"] = [2147483647] * 4
    # 2^32 * 2^32 wraps to 0 and 0 * 4 == nbytes would "agree": each dimension is refused by the dimension bound
    def wrap(h): h["tensors"][0]["shape"] = [1 << 32, 1 << 32]; h["tensors"][0]["nbytes"] = 0
    def entry_number(h): h["tensors"].append(5)
    def entry_string(h): h["tensors"].insert(0, "x")
    def entry_list(h): h["tensors"][1] = [h["tensors"][1]]

    deep = b"[" * 10000
    bad = {"cut %d" % c: good[:c] for c in (0, 3, 4, 15, 16, 40, 16 + hlen - 1, base - 1, end - 1, len(good) // 2)}
    bad.update({"magic": b"PFW2" + good[4:], "magic X": b"XXXX" + good[4:], "hlen 2^62": good[:8] + struct.pack("<Q", 1 << 62) + good[16:],
                "hlen wraps": good[:8] + struct.pack("<Q", (1 << 64) - 8) + good[16:], "no json": good[:16] + b"{" * 10 + good[26:],
                "no json 40": good[:16] + b"{" * 40 + good[56:], "deep": good[:8] + struct.pack("<Q", len(deep)) + deep + good[16:]})
    for edit in (far, big, neg, frac, mism, negdim, dtype, noshape, noconfig, config_list, tensors_obj, overflow, wrap, entry_number,
                 entry_string, entry_list):
        bad[edit.__name__] = P.repack(cfg, w, edit)
    # the boundary itself: nothing behind the last tensor's last byte is needed
    return {"good": good, "cut at the end of the data": good[:end], "re-serialised": P.repack(cfg, w, lambda h: None)}, bad


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    out = str(tmp_path_factory.mktemp("pfw") / "pfw_sanitize")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                        "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs, os.path.join(root, "tests", "native", "pfw_sanitize.cpp"),
                        os.path.join(cs, "pfw.cpp"), "-o", out], capture_output=True, text=True)
    if b.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a compile error in the sources under test is a failure
        missing = any(t in b.stderr for t in ("libclang_rt.asan", "libclang_rt.ubsan", "cannot find -lclang_rt", "unsupported option '-fsanitize"))
        assert missing, b.stderr[-3000:]
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    return out


def _run(exe, tmp_path, blobs):
    paths = []
    for i, blob in enumerate(blobs):
        p = tmp_path / ("c%d.pfw" % i)
        p.write_bytes(blob)
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == len(blobs) and all(len(ln) == 3 for ln in lines)
    return lines


@pytest.mark.parametrize("kind", ["weights", "vad", "punc"])
def test_reader_under_sanitizers(exe, tmp_path, kind):
    cfg, w = _kinds()[kind]
    ok, bad = _malformed(cfg, w)
    refused = [str(N.PF_ERR_FORMAT), str(N.PF_ERR_INVALID_ARG), str(N.PF_ERR_INVALID_ARG)]
    for (name, _), got in zip(bad.items(), _run(exe, tmp_path, list(bad.values()))):
        assert got == refused, (name, got)
    # a sound container passes under its own policy and under the recogniser's (which takes f32 and u8 at 16-byte offsets);
    # the VAD policy refuses the punctuation model's u8 vocabulary with its own code
    col = {"weights": 0, "vad": 1, "punc": 2}[kind]
    has_u8 = any(np.asarray(a).dtype == np.uint8 for a in w.values())
    for (name, _), got in zip(ok.items(), _run(exe, tmp_path, list(ok.values()))):
        assert got[col] == "ok" and got[0] == "ok", (name, got)
        assert got[1] == (str(N.PF_ERR_INVALID_ARG) if has_u8 else "ok") and got[2] == "ok", (name, got)


def test_offset_alignment_is_the_recognisers_alone(exe, tmp_path):
    cfg, w = _kinds()["vad"]
    def odd(h):
        h["tensors"][0]["offset"] += 4
    got = _run(exe, tmp_path, [P.repack(cfg, w, odd)])[0]
    assert got == [str(N.PF_ERR_FORMAT), "ok", "ok"]


def test_the_loaders_refuse_the_two_new_cases():
    """through the library: a shape whose running product overflows, and an entry of `tensors` that is no object"""
    from aliparaformerasr_amd import engine as E
    def overflow(h): h["tensors"][0]["shape"] = [2147483647] * 4
    def entry(h): h["tensors"].append(5)
    kinds = _kinds()
    for edit in (overflow, entry):
        for kind, load in (("vad", E.load_vad_model), ("punc", E.load_punc_model)):
            with pytest.raises(N.PfError) as ei:
                load(P.repack(*kinds[kind], edit))
            assert ei.value.code == N.PF_ERR_INVALID_ARG, (kind, edit.__name__)
