"""The device's BED row body (unfazed_amd/csrc/bed_row.hpp: __host__ __device__, what k_bed_size / k_bed_fill run) without a device:
tests/bed_row_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan, with nothing
preloaded.  It runs the hand-built panel (tests/bedcases.py) and a seeded fuzz of 10^4 rows; every line must equal what summarize.bed_lines
prints for the equivalent records dict, byte for byte, and every row's sized length must equal its written bytes."""
import os
import subprocess

import pytest

import bedcases

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_the_panel_names_the_cases_the_rules_have():
    names = [c["name"] for c in bedcases.CASES]
    assert len(set(names)) == len(names) >= 100
    stems = {n.rsplit("/", 2)[0] for n in names}
    for ratio, pairs in ((10, [(0, 0), (1, 0), (0, 1), (10, 1), (9, 1), (1, 10), (1, 9), (1, 1), (20, 2), (19, 2)]), (1, [(1, 1)]), (0, [(0, 0), (0, 3)])):
        for nd, nm in pairs:
            assert "decision/r%d/%d_%d" % (ratio, nd, nm) in stems
    for n in (0, 1, 63, 64, 65, 129, 1025, 5000):
        assert "len/%d" % n in stems
    for n in (0, 1, 65):
        assert "rows/%d" % n in stems
    assert {"sex", "long_line", "ints", "rows/all_dropped", "names/1", "names/8", "names/254"} <= stems


def test_the_panel_means_what_its_names_say():
    by = {c["name"]: c for c in bedcases.CASES}
    line = lambda name: [b.decode() for b in bedcases.expected_rows(by[name])]
    assert line("decision/r1/1_1/v0/a0")[0].split("\t")[5:9] == ["dad1", "mom1", "1", "READBACKED\n"]
    assert line("decision/r10/9_1/v0/a0") == [""] and line("decision/r10/9_1/v0/a1")[0].split("\t")[5:] == ["dad1|mom1", "None", "10", "AMBIGUOUS_READBACKED\n"]
    assert line("decision/r10/0_0/v0/a1")[0].endswith("\tNone\tNone\t0\t\n") and line("decision/r0/0_0/v1/a1")[0].endswith("\tNone\tNone\t0\t\t-\t-\t-\t-\n")
    assert line("decision/r0/0_3/v0/a0")[0].split("\t")[5] == "mom1"
    assert line("sites/0/v1/a0")[0].split("\t")[9] == "10,9"
    assert [ln.split("\t")[5] for ln in line("sex/v0/a0")] == ["dad1", "dad1", "dad1", "mom1", "mom1"]
    assert len(line("long_line/v1/a0")[0]) > 65536
    assert all(ln == "" for ln in line("rows/all_dropped/v0/a0"))
    kept = [bool(ln) for ln in line("rows/65/v0/a0")]
    assert True in kept and False in kept and len(kept) == 65


def test_bed_row_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "bed_row")
    cc = _gxx(san, os.path.join(_HERE, "bed_row_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.bin"
    fuzz = bedcases.fuzz_cases(20240611, 10000)
    assert sum(len(c["rows"]) for c in fuzz) == 10000
    bedcases.dump(bedcases.CASES + fuzz, str(cases))
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "bed row ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
