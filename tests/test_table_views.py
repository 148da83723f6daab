"""The rules of a site, family and sample view (unfazed_amd/csrc/table_views.hpp: no HIP in it) without a device: tests/table_views_main.cpp
is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan.  It holds every rule of the header to
one hand-built view just inside it and one just outside (code and a part of the text): the compact site form's escape list -- an escape
first, last and out of order in its span, every refusal tests/test_site_forms_gpu.py::test_refusals makes on the device --, the three forms
of a family's columns with the het form's offsets and its cross rule, the wide-depth list in both row shapes and in the settle wording, an
empty table with every pointer null, and the row stride of a sample table.  The program prints how many cases it ran; the count is pinned
here, so that a case cannot drop out silently."""
import os
import re
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
N_CASES = 311


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_table_views_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "table_views")
    cc = _gxx(san, os.path.join(_HERE, "table_views_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
    m = re.search(r"table_views ok: (\d+) cases", run.stdout)
    assert m and int(m.group(1)) == N_CASES, run.stdout
