"""outfile.write_output without a device: with UZ_OUT_BGZF unset every outfile is plain text, whatever its name (what the writers did before
there was a switch); with "host" a name ending in ".gz" is written as BGZF by zlib -- one block per 65 280 bytes, the end-of-file marker --
and the driver's writers go through it."""
import gzip
import io
import contextlib
import os

import pytest

import bgzfoutcases as panel
import vcfrowcases
from unfazed_amd import outfile, summarize, unfazed

TEXT = panel.BY_NAME["text/vcf"]


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for key in ("UZ_OUT_BGZF", "UZ_OUT_BGZF_LEVEL"):
        monkeypatch.delenv(key, raising=False)


def _blocks(path, payload):
    raw = open(path, "rb").read()
    assert raw.endswith(panel.EOF_MARKER) and gzip.decompress(raw) == payload
    return panel.check_blocks(payload, raw[:-len(panel.EOF_MARKER)])


def test_unset_writes_plain_text_whatever_the_name(tmp_path, monkeypatch):
    for value in (None, "", "0", "gpu", "yes"):
        if value is None:
            monkeypatch.delenv("UZ_OUT_BGZF", raising=False)
        else:
            monkeypatch.setenv("UZ_OUT_BGZF", value)
        before = dict(outfile.OUT_STATS)
        for name in ("x.vcf.gz", "x.vcf", "x.bed.gz"):
            outfile.write_output(str(tmp_path / name), [TEXT[:500], TEXT[500:].decode()])
            assert open(str(tmp_path / name), "rb").read() == TEXT
            outfile.write_output(str(tmp_path / name), ["a\n", "b\n"])
            assert open(str(tmp_path / name), "rb").read() == b"a\nb\n"
        assert outfile.OUT_STATS == before


def test_stdout_stays_text_on_every_setting(monkeypatch):
    for value in (None, "host"):
        if value:
            monkeypatch.setenv("UZ_OUT_BGZF", value)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            outfile.write_output("/dev/stdout", ["a\tb\n", b"c\n", memoryview(b"d\n")])
        assert buf.getvalue() == "a\tb\nc\nd\n"


def test_host_writes_bgzf(tmp_path, monkeypatch):
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    before = dict(outfile.OUT_STATS)
    path = str(tmp_path / "x.vcf.gz")
    outfile.write_output(path, [TEXT[:70000], memoryview(TEXT)[70000:]])
    parts = _blocks(path, TEXT)
    k, rest = divmod(len(TEXT), panel.SLICE)
    assert [p[3] for p in parts] == [panel.SLICE] * k + [rest] and k == 4 and rest
    assert {key: outfile.OUT_STATS[key] - before[key] for key in before} == {"bgzf_device_blocks": 0, "bgzf_host_blocks": 5, "bgzf_calls": 1}
    size6 = os.path.getsize(path)
    monkeypatch.setenv("UZ_OUT_BGZF_LEVEL", "1")
    outfile.write_output(path, [TEXT])
    _blocks(path, TEXT)
    assert os.path.getsize(path) > size6
    # a name without ".gz" stays plain, and counts nothing
    before = dict(outfile.OUT_STATS)
    outfile.write_output(str(tmp_path / "x.vcf"), [TEXT])
    assert open(str(tmp_path / "x.vcf"), "rb").read() == TEXT and outfile.OUT_STATS == before


def test_host_edges(tmp_path, monkeypatch):
    monkeypatch.setenv("UZ_OUT_BGZF", "HOST")  # (the value's case does not matter, as for the other switches)
    path = str(tmp_path / "e.bed.gz")
    outfile.write_output(path, [])
    assert open(path, "rb").read() == panel.EOF_MARKER  # no bytes, no blocks: the marker is the whole file
    for name in ("edge/65280", "edge/65281", "random/65280", "tiny/1"):
        outfile.write_output(path, [panel.BY_NAME[name]])
        for _, stream, _, _ in _blocks(path, panel.BY_NAME[name]):
            assert len(stream) <= 5 + panel.SLICE


def test_the_drivers_writers_go_through_it(tmp_path, monkeypatch):
    case = next(c for c in vcfrowcases.CASES if c["records"] and not c["hb"] and c["raw_ann"] is None)
    kind, want_vcf = vcfrowcases.host_output(case, tmp_path)
    assert kind == "text"
    plain_bed = str(tmp_path / "plain.bed")
    summarize.write_bed_output(case["records"], True, True, plain_bed, 10)
    want_bed = open(plain_bed, "rb").read()
    assert want_bed.count(b"\n") > 1
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    monkeypatch.setenv("UZ_VCF_ROUTE", "host")
    before = dict(outfile.OUT_STATS)
    src, out_vcf, out_bed, out_rows = (str(tmp_path / n) for n in ("in2.vcf", "out.vcf.gz", "out.bed.gz", "rows.bed.gz"))
    with open(src, "wb") as fh:
        fh.write(vcfrowcases.file_bytes(case))
    unfazed.write_vcf_output(src, case["records"], case["amb"], False, out_vcf, 10)
    _blocks(out_vcf, want_vcf)
    summarize.write_bed_output(case["records"], True, True, out_bed, 10)
    _blocks(out_bed, want_bed)
    rows = summarize.BedRows(True, True, 10)
    rows.write(out_rows, extra_records=case["records"])
    _blocks(out_rows, want_bed)
    assert outfile.OUT_STATS["bgzf_calls"] - before["bgzf_calls"] == 3
