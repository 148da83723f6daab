"""The rules of a batch of gathered BGZF blocks (unfazed_amd/csrc/bgzf_batch.hpp: no HIP in it) without a device: tests/bgzf_batch_main.cpp is
built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan.  It holds the slicer to cut lists written
out by hand, the slices' byte ranges to the clamp at 0 and the end of `comp`, the table check to every rule with and without the in-order
rule, and the flag decode to the lower of two refused slices and the two error texts."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_bgzf_batch_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "bgzf_batch")
    cc = _gxx(san, os.path.join(_HERE, "bgzf_batch_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "bgzf_batch ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
