"""The device's BCF value body (unfazed_amd/csrc/bcf_cell.hpp: __host__ __device__, the body k_bcf_cells runs) without a device:
tests/bcf_cell_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan.  It runs the
hand-built edge table (tests/bcfcases.py) and a seeded fuzz of 2 * 10^5 cells against a plain restatement of the host's reader and the pack
rules: every settled cell equal (to the restatement and to the table's hand-written values), every `unsettled` cell handed back, at least 90 %
of the fuzzed cells settled."""
import os
import re
import subprocess

import pytest

import bcfcases

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def case_lines():
    out = []
    for c in bcfcases.CASES:
        if not c["cells"]:
            out.append("\x1f".join([c["name"], bcfcases.P] + ["0:"] * 5 + ["2,65535,65535,65535"]))
            continue
        where = {key: (f, t, n) for f, (key, t, n) in enumerate(c["fields"])}
        for k, (raw, values, label) in enumerate(c["cells"]):
            fields = []
            for key in ("GT", "AD", "RO", "AO", "GQ"):
                if key not in where:
                    fields.append("0:")
                    continue
                f, t, n = where[key]
                fields.append("%d:%s" % (t | n << 4, b"".join(bcfcases.entry_bytes(t, x) for x in raw[f]).hex()))
            want = "%d,%d,%d,%d" % bcfcases.packed(values) if label == bcfcases.P else "-"
            out.append("\x1f".join(["%s[%d]" % (c["name"], k), label] + fields + [want]))
    return out


def test_the_table_has_the_cases_the_format_names():
    names = {c["name"] for c in bcfcases.CASES}
    assert len(names) == len(bcfcases.CASES) >= 35
    by = {c["name"]: c for c in bcfcases.CASES}
    gt_shapes = {(t, n) for c in bcfcases.CASES for key, t, n in c["fields"] if key == "GT"}
    assert {(bcfcases.INT8, 1), (bcfcases.INT8, 2), (bcfcases.INT8, 3), (bcfcases.INT16, 2), (bcfcases.CHAR, 3)} <= gt_shapes
    ad_shapes = {(t, n) for c in bcfcases.CASES for key, t, n in c["fields"] if key == "AD"}
    assert {t for t, _ in ad_shapes} >= {bcfcases.INT8, bcfcases.INT16, bcfcases.INT32} and {n for _, n in ad_shapes} >= {1, 2, 3}
    depths = {x for c in bcfcases.CASES for _, v, _ in c["cells"] for x in v[1:3]}
    assert {32767, 32768, -5} <= depths
    assert [lab for _, _, lab in by["depth_32767"]["cells"]] == [bcfcases.P] * 2 and by["depth_32768"]["cells"][0][2] == bcfcases.U
    assert by["depth_minus_five"]["pack_raises"] and by["depth_minus_five"]["cells"][0][2] == bcfcases.U
    gq = [v[3] for _, v, _ in by["gq_float"]["cells"]]
    assert 40000.0 in gq and any(abs(x - 99.9) < 1e-4 for x in gq)
    assert bcfcases.packed((1, -1, -1, bcfcases.F32(99.9))) == (1, 0xFFFF, 0xFFFF, 99) and bcfcases.packed((1, 5, 32768, 40000.0)) == (1, 5, 32767, 32767)
    assert bcfcases.packed((1, -1, -1, bcfcases.NAN))[3] == bcfcases.packed((1, -1, -1, -1.0))[3] == bcfcases.packed((1, -1, -1, -0.5))[3] == 0xFFFF
    assert any(n >= 15 and key not in ("GT", "AD", "RO", "AO", "GQ") for c in bcfcases.CASES for key, _, n in c["fields"])  # the long length form
    assert by["no_format_fields"]["fields"] == [] and all(lab == bcfcases.U for _, _, lab in by["gt_as_characters"]["cells"])
    assert all(label in (bcfcases.P, bcfcases.U) for c in bcfcases.CASES for _, _, label in c["cells"])


def test_bcf_cell_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "bcf_cell")
    cc = _gxx(san, os.path.join(_HERE, "bcf_cell_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.txt"
    cases.write_bytes(("\n".join(case_lines()) + "\n").encode())
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "bcf cell ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr, run.stderr
    share = re.search(r"fuzz: (\d+) of (\d+) cells settled", run.stdout)
    assert share and int(share.group(2)) >= 100000 and int(share.group(1)) >= 0.9 * int(share.group(2)), run.stdout
