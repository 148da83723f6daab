"""The device's annotated-VCF line body (unfazed_amd/csrc/vcf_row.hpp: __host__ __device__, what k_vcfout_size / k_vcfout_fill run) without a
device: tests/vcf_row_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan, with nothing
preloaded.  It runs the hand-built panel (tests/vcfrowcases.py) and a seeded fuzz of 2 000 records; every line must equal what the host
write_vcf_output prints, byte for byte, every record's sized length must equal its written bytes, and the records handed back must be the stated
ones."""
import os
import subprocess

import pytest

import vcfrowcases

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_the_panel_names_the_cases_the_rules_have():
    names = [c["name"] for c in vcfrowcases.CASES]
    assert len(set(names)) == len(names) >= 80
    want = {"gate/0_0", "gate/0_1", "gate/1_1", "gate/1p0", "gate/d_d", "gate/d", "gate/d_1", "gate/0_d", "gate/1", "gate/0", "gate/0_1_1", "gate/10_11", "gate/123_0",
            "handback/gt_1234_0", "handback/gt_empty", "handback/gt_a_b", "handback/col_few", "handback/col_many", "handback/no_format", "handback/gt_twice",
            "gtslot/0", "gtslot/mid", "gtslot/last", "gtslot/none", "pad/short1", "pad/short3", "pad/equal", "pad/longer", "pad/dot5",
            "gtcode/0", "gtcode/1", "gtcode/2", "keys/same_site_twice", "keys/homref_and_het", "keys/end_abc", "keys/end_empty", "keys/sv_and_point", "keys/dup_sample",
            "long/64k_cell", "ends/no_final_newline", "ends/crlf", "ends/empty_lines", "chunks/4096", "chunks/long_line", "chunks/all_handed_back"}
    want |= {"uet/%d" % e for e in range(-1, 7)} | {"uops/%d" % n for n in (0, 9, 10, 999999, 1000000)} | {"samples/%d" % n for n in (1, 3, 63, 64, 65, 130)}
    want |= {"records/%d" % n for n in (0, 1, 65, 257)} | {"align/%d" % a for a in range(16)}
    want |= {"edge/%s/%d" % (k, t) for k in ("tab", "colon", "gt") for t in (1023, 1024, 1025, 527, 528, 529)}
    assert want <= set(names), sorted(want - set(names))


def test_the_panel_means_what_its_names_say(tmp_path):
    by = vcfrowcases.BY_NAME
    cells = lambda name, k=0: vcfrowcases.expected_rows(by[name], tmp_path)[k].decode().rstrip("\n").split("\t")[9:]
    assert cells("gate/0_1") == ["1|0:7:2:0", "0/0:3:-1:-1"] and cells("gate/0_0") == ["0/0:7:-1:-1", "0/0:3:-1:-1"]
    assert cells("gate/10_11")[0] == "1|0:7:2:0" and cells("gate/1")[0] == "1|0:7:2:0" and cells("gate/d_1")[0] == "1|0:7:2:0" and cells("gate/0_d")[0] == "0/.:7:-1:-1"
    assert cells("gtcode/0")[0] == "0/1:7:2:3" and cells("gtcode/0_dropped")[0] == "0/1:7:-1:-1" and cells("gtcode/2")[0] == "0|1:7:3:0"
    assert cells("pad/short3")[0] == "1|0:7:.:.:.:2:0" and cells("pad/dot5") == [".:.:.:.:.:-1:-1", "1|0:.:.:.:.:2:0"] and cells("pad/longer")[0].endswith(":x:y:2:0")
    assert cells("gtslot/none") == ["7:9:-1:-1", "3:1:-1:-1"] and cells("gtslot/last")[0] == "7:9:1|0:2:0" and cells("gtslot/not_reached") == ["7:.:.:-1:-1", "3:1:0|1:3:0"]
    assert [cells("uet/%d" % e)[0].rsplit(":", 1)[1] for e in range(-1, 7)] == [str(e) for e in range(-1, 7)]
    assert cells("uops/999999")[0] == "1|0:7:999999:0"
    assert vcfrowcases.host_output(by["uops/1000000"], tmp_path)[1].split(b"\n")[-3].split(b"\t")[9] == b"1|0:7:1e+06:0"
    assert cells("keys/dup_sample") == ["1|0:7:2:0", "0/0:3:-1:-1", "1|0:2:2:0"] and cells("keys/sv_and_point", 0) == ["1|0:7:3:1", "0/1:3:-1:-1"]
    assert cells("keys/sv_and_point", 1) == ["0/1:7:-1:-1", "0|1:3:2:0"] and cells("keys/end_abc")[0] == "1|0:7:2:0" and cells("keys/end_empty")[0] == "1|0:7:2:0"
    assert [vcfrowcases.host_output(by["handback/gt_" + t], tmp_path) for t in ("empty", "a_b")] == [("raise", ValueError)] * 2
    assert vcfrowcases.host_output(by["handback/col_few"], tmp_path) == ("raise", IndexError) and vcfrowcases.host_output(by["handback/no_format"], tmp_path) == ("raise", IndexError)
    for kind in ("tab", "colon", "gt"):
        for target in (1023, 1024, 1025, 527, 528, 529):
            d = vcfrowcases.decode(by["edge/%s/%d" % (kind, target)])
            at = (int(d["line_at"][0]) & ~15) + target
            assert d["text"][at:at + 1] == {"tab": b"\t", "colon": b":", "gt": b"/"}[kind] and d["text"][at - 2:at + 3] == {"tab": b"99\t10", "colon": b"11:7\t", "gt": b"10/11"}[kind]
    assert sorted({int(vcfrowcases.decode(by["align/%d" % a])["samp_at"][0]) % 16 for a in range(16)}) == list(range(16))
    assert len(by["long/64k_cell"]["lines"][0]) > 65536 and len(by["long/64k_cells"]["lines"][0]) > 65536
    assert 38000 < len(vcfrowcases.file_bytes(by["chunks/4096"])) < 44000


def test_vcf_row_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "vcf_row")
    cc = _gxx(san, os.path.join(_HERE, "vcf_row_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.bin"
    fuzz = vcfrowcases.fuzz_cases(20240917, 2000)
    assert sum(len(c["lines"]) for c in fuzz) == 2000 and any(c["hb"] for c in fuzz)
    vcfrowcases.dump(vcfrowcases.CASES + fuzz, str(cases), tmp_path)
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "vcf row ok" in run.stdout, run.stdout + run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
