"""The book of the walk slots (unfazed_amd/csrc/walk_book.hpp: which slot is held, the high-water mark of every kind of buffer, the parked
blocks) without a device: tests/walk_book_main.cpp is built with g++ into a program of its own and run as a child process, once under
ThreadSanitizer and once under AddressSanitizer + UBSan.  The program asserts the claim policy on a hand-written table, the drain signal, release
then claim, and four threads that claim, note and release 10 000 times each; the kind count is checked against the two lists at compile time."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_walk_book_under_sanitizer(san, tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "walk_book")
    cc = _gxx(san, os.path.join(_HERE, "walk_book_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "walk book ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
