"""The device's head walk and rank selection (unfazed_amd/csrc/headwalk.hpp: __host__ __device__, the bodies k_head_walk and k_head_rank run)
without a device: tests/headwalk_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer +
UBSan.  It drives the walk window by window over heap copies of exactly the stream's size (a load outside the file's bytes is the sanitizer's
finding) and the selection pass by pass, on hand-built cases and a seeded fuzz; expected values come from a plain sequential reader and
std::nth_element inside the program."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_headwalk_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "headwalk")
    cc = _gxx(san, os.path.join(_HERE, "headwalk_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "headwalk ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
