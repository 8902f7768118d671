"""The result-building half of Recognizer::Forward (csrc/stream_result.cpp) on the host: no GPU."""
import os
import shutil
import subprocess

import pytest


@pytest.mark.timeout(300)
def test_stream_result_builder_under_sanitizers(tmp_path):
    """build_stream_result under AddressSanitizer + UBSan (tests/native/stream_result_sanitize.cpp): HostBatchOut blocks of exactly
    words() filled by hand through the block views, B = 2 with unequal streams, expected fields written out literally — plain and
    peak-row timestamps, Scores on and off, the CTC collapse at the prompt rows' edge (inside, across, n = 0, cap > n, no block),
    the peak-frame choice under CTC + TOPK (two matching frames, none, a NaN of equal bits), the n-best list from the host
    enumeration and from the device search (n_hyp < N, L = 0), the beam's labelings plain / hot / LM / both, own alignments
    (len = -1, no target in the batch, not ok, no block) and alignments beside the beam (H >= a_hc + N, H below it,
    a_len != b_len); no report."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "stream_result_sanitize")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    flags = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
             "-fno-omit-frame-pointer", "-std=c++17", "-I" + cs]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    b = subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if b.returncode != 0:                              # only a missing sanitizer runtime skips; the program itself must compile
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    srcs = [os.path.join(root, "tests", "native", "stream_result_sanitize.cpp"), os.path.join(cs, "stream_result.cpp"),
            os.path.join(cs, "hostutil.cpp")]
    b = subprocess.run(flags + srcs + ["-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("ok ")
