"""The BCF-record-to-line rules without a device.  The plain converter (unfazed_amd/bcf_text.py) is held to the hand-built panel's literal lines
(tests/bcfrowcases.py) and to a seeded fuzz; then the device's body (unfazed_amd/csrc/bcf_row.hpp: __host__ __device__, what k_bcfout_size /
k_bcfout_fill run): tests/bcf_row_main.cpp is built with g++ into a program of its own and run as a child process under AddressSanitizer + UBSan,
with nothing preloaded, over the panel and 2 000 fuzzed records -- every line equal to the stated one byte for byte, sized == written, samp_at, the
handed-back set equal to the stated one -- and, in the same program, the float rule against snprintf("%g")."""
import os
import subprocess

import numpy as np
import pytest

import bcfrowcases
from unfazed_amd import bcf_text

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _gxx(san, src, out):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=300)


def test_the_panel_names_the_cases_the_rules_have():
    names = [c["name"] for c in bcfrowcases.CASES]
    assert len(set(names)) == len(names) >= 150
    want = {"empty/all", "empty/id", "empty/alt", "empty/qual", "empty/filter", "empty/info", "flag/type0", "flag/len0_int", "format/none", "format/no_samples",
            "gt/haploid", "gt/diploid", "gt/triploid", "gt/phased", "gt/half_missing", "gt/empty", "gt/int8_allele126", "gt/int16_allele126", "gt/int16_allele127",
            "gt/int8_allele62", "gt/chars", "cell/strings", "cell/string_padding_unread", "chunks/after_first", "chunks/before_last", "chunks/long_record",
            "handback/first", "handback/last", "handback/adjacent", "handback/all", "handback/no_allele", "handback/dict_one_beyond", "handback/contig_one_beyond",
            "handback/fmt_key_vector", "handback/byte_1f_id", "handback/byte_7f_info", "handback/byte_1f_cell", "handback/byte_7f_cell", "handback/n_sample_differs",
            "bound/info_value_over_l_shared", "bound/fmt_array_over_l_indiv", "bound/data_end_over", "bound/escape_length_over", "bound/info_descriptor_at_end",
            "bound/fmt_descriptor_at_end", "float/0", "float/neg0", "float/1e-4", "float/below_1e-4_rounds_up", "float/999999", "float/999999.4375", "float/50",
            "float/0.1", "float/tie_even_down", "float/tie_even_up", "float/carry", "float/qual_1e6", "float/qual_999999.5", "float/qual_inf", "float/qual_nan",
            "float/reserved", "float/reserved_eov_qual"}
    want |= {"%s/%s" % (w, k) for w in ("int8", "int16", "int32") for k in ("value", "missing", "eov_first", "eov_mid")}
    want |= {"len/%s_%d" % (k, n) for k in ("str", "vec", "fmt") for n in (14, 15, 16)} | {"handback/type_%d" % t for t in (4, 6, 8, 15)}
    want |= {"samples/%d" % n for n in (0, 1, 63, 64, 65, 130)} | {"records/%d" % n for n in (0, 1, 65, 257)}
    assert want <= set(names), sorted(want - set(names))


def test_the_panel_means_what_its_names_say():
    by = bcfrowcases.BY_NAME
    rec = lambda name, k=0: by[name]["records"][k]
    # the escape is taken exactly from 15 on, and the int8 genotype bytes are the ones the names speak of
    assert rec("len/str_14")[8 + 24] == 0xE7 and rec("len/str_15")[8 + 24:8 + 27] == bytes([0xF7, 0x11, 15]) and rec("len/str_16")[8 + 24:8 + 27] == bytes([0xF7, 0x11, 16])
    assert rec("gt/int8_allele126")[-2:] == bytes([2, 0xFE]) and rec("gt/int8_allele62")[-2:] == bytes([126, 127])
    assert rec("gt/int16_allele127")[-4:] == bytes([0, 1, 1, 1])
    # a bound case differs from the record that fits by exactly one byte of one length word
    fits, over = rec("bound/info_value_fits"), rec("bound/info_value_over_l_shared")
    assert fits[8:] == over[8:] and fits[4:8] == over[4:8] and int.from_bytes(fits[:4], "little") - int.from_bytes(over[:4], "little") == 1
    fits, over = rec("bound/fmt_fits"), rec("bound/fmt_array_over_l_indiv")
    assert fits[8:] == over[8:] and fits[:4] == over[:4] and int.from_bytes(fits[4:8], "little") - int.from_bytes(over[4:8], "little") == 1
    assert by["bound/data_end_over"]["cut"] == 1 and rec("bound/data_end_over") == rec("bound/data_end_fits")
    assert len(bcfrowcases.layout(by["bound/data_end_fits"])[0]) - len(bcfrowcases.layout(by["bound/data_end_over"])[0]) == 1
    assert rec("handback/dict_one_beyond")[-4:] == bytes([0x11, len(bcfrowcases.DICT), 0x11, 1]) and bcfrowcases.DICT[12] == "" and bcfrowcases.CONTIGS[2] == ""
    assert b"\x1f" in rec("handback/byte_1f_id") and b"\x7f" in rec("handback/byte_7f_info")
    # the floats are the ones named: the largest below 1e-4, the nearest to 999999.5 below it, the ties exact
    f = lambda name: np.array([int.from_bytes(rec(name)[8 + 12:8 + 16], "little")], np.uint32).view(np.float32)[0]
    assert f("float/below_1e-4_rounds_up") == np.nextafter(np.float32(0.0001), np.float32(0)) and float(f("float/1e-4")) < 1e-4
    assert float(f("float/999999.4375")) == 999999.4375 and float(f("float/qual_999999.5")) == 999999.5
    assert float(f("float/tie_even_down")) == 125000.5 and float(f("float/tie_even_up")) == 125001.5 and 9.99999 < float(f("float/carry")) < 10
    # chunk edges: the first chunk ends behind the first record / ahead of the last
    c = by["chunks/after_first"]
    data, at = bcfrowcases.layout(c)
    assert int(at[0]) - (int(at[0]) & ~15) + len(c["records"][0]) == c["chunk"]
    c = by["chunks/before_last"]
    data, at = bcfrowcases.layout(c)
    assert len(data) - (int(at[0]) & ~15) - 1 == c["chunk"]
    assert max(len(r) for r in by["chunks/long_record"]["records"]) > by["chunks/long_record"]["chunk"]
    assert [len(by["samples/%d" % n]["lines"][0].split("\t")) - 9 for n in (1, 63, 64, 65, 130)] == [1, 63, 64, 65, 130]
    assert [by["handback/" + k]["hb"] for k in ("first", "last", "adjacent", "all")] == [[0], [2], [1, 2], [0, 1, 2]]


@pytest.mark.parametrize("case", bcfrowcases.CASES, ids=lambda c: c["name"])
def test_converter_on_the_panel(case):
    bcfrowcases.converter_holds(case, bcf_text.line)


def test_converter_on_the_fuzz():
    fuzz = bcfrowcases.fuzz_cases(20241020, 2000)
    assert sum(len(c["lines"]) for c in fuzz) == 2000 and 100 < sum(len(c["hb"]) for c in fuzz) < 500
    assert {"raise", "line"} <= {"raise" if v == bcfrowcases.RAISE else "line" for c in fuzz for v in c["conv"].values()}
    for case in fuzz:
        bcfrowcases.converter_holds(case, bcf_text.line)


def test_the_converter_does_not_import_the_engine():
    src = open(os.path.join(_ROOT, "unfazed_amd", "bcf_text.py")).read()
    assert "import" in src and "engine" not in src and "ctypes" not in src


def test_bcf_row_under_sanitizer(tmp_path):
    san = "address,undefined"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(san, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=" + san)
    exe = str(tmp_path / "bcf_row")
    cc = _gxx(san, os.path.join(_HERE, "bcf_row_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    cases = tmp_path / "cases.bin"
    fuzz = bcfrowcases.fuzz_cases(20241021, 2000)
    assert sum(len(c["lines"]) for c in fuzz) == 2000 and any(c["hb"] for c in fuzz)
    bcfrowcases.dump(bcfrowcases.CASES + fuzz, str(cases))
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "bcf row ok" in run.stdout, run.stdout + run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
