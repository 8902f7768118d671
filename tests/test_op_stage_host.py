"""The staging kit of the stand-alone ops (csrc/op_stage.h) on the host: no GPU."""
import os
import shutil
import subprocess

import pytest


@pytest.mark.timeout(300)
def test_op_stage_kit_under_sanitizers(tmp_path):
    """The host-only part of csrc/op_stage.h under AddressSanitizer + UBSan (tests/native/op_stage_sanitize.cpp), compiled as plain
    C++ (no HIP header): blocked_index is a bijection and the restated formula; the hostile patterns are finite, large and the
    restated bit formulas; the typed carve's fields are 256-aligned, in declaration order and disjoint, and a pattern written
    through each field of a heap buffer of exactly the carved size reads back; the guard rule agrees with a brute-force
    restatement on a grid of geometries (row-major and blocked) and FIRES on one unwritten cell, one cell beyond N and one
    guard-row cell, naming that cell; the two-sentinel byte rule; no report."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "op_stage_sanitize")
    cs = os.path.join(root, "aliparaformerasr_amd", "csrc")
    flags = [hipcc, "-x", "c++", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-omit-frame-pointer", "-std=c++17",
             "-Wall", "-Werror", "-I" + cs]          # host code only: plain C++, no device pass, no GPU sanitizer
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    b = subprocess.run(flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if b.returncode != 0:                              # only a missing sanitizer runtime skips; the program itself must compile
        pytest.skip("sanitizer runtime not available: " + b.stderr[-300:])
    b = subprocess.run(flags + [os.path.join(root, "tests", "native", "op_stage_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("ok ")
