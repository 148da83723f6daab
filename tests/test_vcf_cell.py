"""The device's sample-cell parser (unfazed_amd/csrc/vcf_cell.hpp: __host__ __device__, the body k_vcf_cells runs) without a device:
tests/vcf_cell_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan.  It runs the
hand-built edge table (tests/vcfcases.py) and a seeded fuzz of 10^5 cells; every cell must equal the host reader's value after the pack rules
or be unsettled, every `plain` case must be settled and every `unsettled` one handed back."""
import os
import subprocess

import pytest

import vcfcases

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def case_lines():
    out = []
    for c in vcfcases.CASES:
        cells = vcfcases.record_cells(c)
        seen = set()
        for text, _, label in cells:
            key = (text, label)
            if key in seen:
                continue
            seen.add(key)
            out.append("\x1f".join([label, "1" if c.get("raises") else "0", c["fmt"] if c["fmt"] is not None else "\x1e", "\x1e" if text is None else text]))
    return out


def test_the_table_has_the_cases_the_grammar_names():
    names = {c["name"] for c in vcfcases.CASES}
    assert len(names) == len(vcfcases.CASES) >= 40
    texts = {t for c in vcfcases.CASES for t, _, _ in c["cells"]}
    for gq in ("99", "99.", "99.5", "0.000001", "1.0000001", "1e2", "-0.0", "nan", "32767.9", "32768"):
        assert "0/1:" + gq in texts, gq
    for ad in ("0,0", "32767,32767", "32768,1", "1073741824,5", "-1,5", "-5,5"):
        assert any(t.endswith(":" + ad) for t in texts), ad
    assert all(label in ("plain", "unsettled") for c in vcfcases.CASES for _, _, label in c["cells"])


def test_vcf_cell_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "vcf_cell")
    cc = _gxx(san, os.path.join(_HERE, "vcf_cell_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.txt"
    cases.write_bytes(("\n".join(case_lines()) + "\n").encode())
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "vcf cell ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
