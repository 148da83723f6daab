"""UZ_BCF_ROUTE=host through the driver's writer (unfazed.write_vcf_output on a BCF of DNMs), no device involved: the records become text by
unfazed_amd/bcf_text.py and go through the host writer.  On the panel's files (tests/bcfrowcases.py) the output equals, byte for byte, what the
host writer makes of a text VCF that holds the same header and the panel's LITERAL lines; on a file tests/bcfio.py wrote, every sample's GT piece
and UOPS / UET equal those of the run on the text file the BCF was made from.  Not set, or any other value: the refusal, unchanged.  And
read_vars_vcf's BCF branch, a numpy selection now, against the plain double loop."""
import numpy as np
import pytest

import bcfrowcases
from unfazed_amd import session, unfazed
from unfazed_amd.model import HET, HOM_ALT

FILE_CASES = [c for c in bcfrowcases.CASES if c["file_ok"] and c["lines"]]


def test_the_switch(monkeypatch):
    monkeypatch.delenv("UZ_BCF_ROUTE", raising=False)
    assert unfazed.bcf_route() is None
    for value, want in (("device", "device"), ("Device", "device"), ("host", "host"), ("HOST", "host"), ("anything", None), ("", None), ("1", None)):
        monkeypatch.setenv("UZ_BCF_ROUTE", value)
        assert unfazed.bcf_route() == want


@pytest.mark.parametrize("value", [None, "", "anything", "on"])
def test_unset_or_unknown_still_refuses(tmp_path, monkeypatch, value):
    case = bcfrowcases.BY_NAME["gt/diploid"]
    src = str(tmp_path / "dnms.bcf")
    open(src, "wb").write(bcfrowcases.file_bytes(case))
    monkeypatch.delenv("UZ_BCF_ROUTE", raising=False)
    if value is not None:
        monkeypatch.setenv("UZ_BCF_ROUTE", value)
    before = dict(unfazed.BCF_STATS)
    with pytest.raises(SystemExit) as e:
        unfazed.write_vcf_output(src, {}, False, False, str(tmp_path / "out.vcf"), 10)
    assert e.value.code == unfazed.BCF_OUTPUT_MESSAGE and "BCF" in unfazed.BCF_OUTPUT_MESSAGE
    assert unfazed.BCF_STATS == before and not (tmp_path / "out.vcf").exists()


@pytest.mark.parametrize("case", FILE_CASES, ids=lambda c: c["name"])
def test_panel_files_on_the_host_route(case, tmp_path, monkeypatch):
    src, ref = str(tmp_path / "dnms.bcf"), str(tmp_path / "lines.vcf")
    open(src, "wb").write(bcfrowcases.file_bytes(case))
    open(ref, "wb").write(bcfrowcases.text_file_bytes(case))
    records = bcfrowcases.route_records(case)
    want = bcfrowcases.host_writer(ref, str(tmp_path / "want.vcf"), records, {"UZ_VCF_ROUTE": "host"}, monkeypatch)
    before = dict(unfazed.BCF_STATS)
    got = bcfrowcases.host_writer(src, str(tmp_path / "got.vcf"), records, {"UZ_BCF_ROUTE": "host"}, monkeypatch)
    assert got == want, case["name"]
    assert session.current_backend() is None  # (the host route makes no backend)
    grew = {k: unfazed.BCF_STATS[k] - before[k] for k in before}
    assert grew == {"bcf_device_rows": 0, "bcf_host_rows": len(case["lines"]), "bcf_calls": 0}


def test_the_panel_files_annotate_something(tmp_path, monkeypatch):
    case = bcfrowcases.BY_NAME["records/65"]
    src = str(tmp_path / "dnms.bcf")
    open(src, "wb").write(bcfrowcases.file_bytes(case))
    kind, text = bcfrowcases.host_writer(src, str(tmp_path / "got.vcf"), bcfrowcases.route_records(case), {"UZ_BCF_ROUTE": "host"}, monkeypatch)
    assert kind == "text"
    rows = [ln.split("\t") for ln in text.decode().split("\n") if ln and ln[0] != "#"]
    assert len(rows) == 65 and all(r[8] == "GT:DP:UOPS:UET" for r in rows)
    assert all(r[9].startswith("1|0:") and r[9].endswith(":0") and not r[9].endswith(":-1:0") for r in rows)  # s0 is 0/1 everywhere, dad's
    assert all(r[11].endswith(":-1:-1") for r in rows)  # the last sample is ./.
    assert text.count(b"##unfazed=") == 1 and text.decode().split("\n")[0] == "##fileformat=VCFv4.2"


def test_a_record_without_a_line_raises_with_its_index(tmp_path, monkeypatch):
    from unfazed_amd import bcf_text
    case = bcfrowcases.BY_NAME["handback/alternate"]
    data, rec_at = bcfrowcases.layout(bcfrowcases.BY_NAME["handback/byte_7f_info"])
    with pytest.raises(ValueError, match="record 7"):
        bcf_text.line(data, rec_at[0], bcfrowcases.DICT, bcfrowcases.CONTIGS, 0, index=7)
    data, rec_at = bcfrowcases.layout(case)
    assert bcf_text.lines(data, rec_at, case["dict"], case["contigs"], 0, only=[1, 3]) == [case["lines"][1], case["lines"][3]]


def test_a_bcfio_file_on_the_host_route(tmp_path, monkeypatch):
    from synth.small import SmallConfig, make_small
    from tests.bcfio import write_bcf
    from tests.filesio import dump_dataset
    from unfazed_amd.io_vcf import read_vcf
    from vcfrowcases import rec
    ds = make_small(SmallConfig(seed=77, n_dnms=10))
    paths = dump_dataset(ds, str(tmp_path))
    samples, recs, _ = read_vcf(paths["dnm_vcf"])
    bcf = str(tmp_path / "dnms.bcf")
    write_bcf(bcf, samples, recs, ds.contigs)
    records = {}
    for k, r in enumerate(recs):
        for i, g in enumerate(r.gt_types):
            if g in (HET, HOM_ALT):
                vt = r.info.get("SVTYPE") or "POINT"
                key, val = rec(samples[i], r.start, r.end, chrom=r.chrom, vartype=vt, nd=(k + i) % 3, nm=(k + 2 * i) % 2 * 2)
                records[key] = val
    assert records
    kind_t, text = bcfrowcases.host_writer(paths["dnm_vcf"], str(tmp_path / "t.vcf"), records, {"UZ_VCF_ROUTE": "host"}, monkeypatch)
    kind_b, out = bcfrowcases.host_writer(bcf, str(tmp_path / "b.vcf"), records, {"UZ_BCF_ROUTE": "host"}, monkeypatch)
    assert kind_t == kind_b == "text"
    rows = lambda b: [ln.split("\t") for ln in b.decode().split("\n") if ln and ln[0] != "#"]
    t_rows, b_rows = rows(text), rows(out)
    assert len(t_rows) == len(b_rows) == len(recs) and out.count(b"|") >= 1
    for t, b in zip(t_rows, b_rows):
        assert t[:2] == b[:2] and t[3:5] == b[3:5] and b[8] == "GT:AD:GQ:UOPS:UET" and len(t) == len(b)
        gi = t[8].split(":").index("GT")
        for ct, cb in zip(t[9:], b[9:]):
            # (the text file writes a no-call as ./. and bcfio encodes it as two missing alleles: the same piece)
            assert ct.split(":")[gi] == cb.split(":")[0] and ct.split(":")[-2:] == cb.split(":")[-2:]


def test_read_vars_vcf_selection_equals_the_plain_loop(tmp_path):
    from unfazed_amd.hostpath import SNV_TYPES
    from unfazed_amd.io_native import read_vcf_table
    case = bcfrowcases.BY_NAME["samples/65"]
    recs = [bcfrowcases.record(pos=10 * k, info=[(bcfrowcases.key("SVTYPE"), bcfrowcases.tstr("DEL"))] if k % 3 == 0 else (),
                               fmt=[bcfrowcases.fmt_ints("GT", [bcfrowcases.gt(["0/1", "0/0", "1/1", "./.", "1", "0", "1|0"][(k + s) % 7]) for s in range(5)], 1)], n_sample=5)
            for k in range(40)]
    recs += [bcfrowcases.record(chrom=1, pos=5, fmt=[bcfrowcases.fmt_ints("GT", [bcfrowcases.gt("0/0")] * 5, 1)], n_sample=5),
             bcfrowcases.record(chrom=3, pos=7, fmt=[bcfrowcases.fmt_ints("GT", [bcfrowcases.gt("1/1")] * 5, 1)], n_sample=5), bcfrowcases.record(chrom=3, pos=9, n_sample=5)]
    path = str(tmp_path / "dnms.bcf")
    open(path, "wb").write(bcfrowcases.file_bytes(dict(case, records=recs, n_samples=5, file_ok=True)))
    t = read_vcf_table(path)
    chrom_of = np.repeat(np.arange(len(t.contigs)), np.diff(t.contig_off))
    want = []
    for j in range(t.n_sites):  # the plain loop read_vars_vcf ran before
        vartype = t.info(j, "SVTYPE")
        if vartype is None:
            vartype = SNV_TYPES[0]
        for i in range(len(t.samples)):
            if int(t.gt[i, j]) in [HET, HOM_ALT]:
                want.append({"chrom": t.contigs[int(chrom_of[j])], "start": int(t.pos[j]), "end": int(t.end[j]), "kid": t.samples[i], "vartype": vartype, "bam": ""})
    got = list(unfazed.read_vars_vcf(path))
    assert got == want and len(got) > 60 and {d["vartype"] for d in got} == {"DEL", "POINT"} and {d["chrom"] for d in got} == {"chr1", "chrX"}
    assert [type(v) for v in got[0].values()] == [type(v) for v in want[0].values()]
