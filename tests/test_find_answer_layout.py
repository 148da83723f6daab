"""The block layout of uz_find_answer (unfazed_amd/csrc/find_answer.hpp) without a device: tests/find_answer_main.cpp is built with g++ into a
program of its own and run as a child process under AddressSanitizer + UBSan; the engine's Python statement of the layout is held to the
same plain recomputation."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, exe):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"),
                           src, "-o", exe], capture_output=True, text=True)


def test_layout_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "find_answer")
    cc = _gxx(san, os.path.join(_HERE, "find_answer_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "find answer layout ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr


def test_the_engine_states_the_same_layout():
    from unfazed_amd.engine import HipEngine
    for n in (0, 1, 2, 3, 30, 31, 32, 33):
        for nc in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257):
            for nh in (0, 1, 2, 3, 63, 64, 65):
                off, total = HipEngine.find_answer_layout(n, nc, nh)
                at = 0
                for k, b in enumerate((64, 8 * (n + 1), 8 * (n + 1), 4 * nc, nc, 4 * nh)):
                    assert off[k] == at and at % 256 == 0
                    at += -(-b // 256) * 256
                assert total == at
