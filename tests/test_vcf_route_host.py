"""The annotated-VCF writer's device route where no device is involved (unfazed.write_vcf_output, vcf_annotations): a backend without vcf_rows
keeps the host writer, and the annotation table built from a panel case (tests/vcfrowcases.py), applied by the plain-Python statement of the
rules (vcfrowcases.rules_text), reproduces the host writer's text -- which holds the table builder, and the statement, on the CPU."""
import os

import pytest

import vcfrowcases
from unfazed_amd import session, unfazed


def test_a_backend_without_vcf_rows_keeps_the_host_writer(tmp_path, monkeypatch):
    from oracle_backend import OracleBackend
    case = vcfrowcases.BY_NAME["samples/65"]
    kind, want = vcfrowcases.host_output(case, tmp_path)
    assert kind == "text"
    src, dst = str(tmp_path / "in.vcf"), str(tmp_path / "routed.vcf")
    backend = OracleBackend()
    assert not hasattr(backend, "vcf_rows")
    session.set_backend(backend)
    monkeypatch.setenv("UZ_VCF_ROUTE", "device")
    before = dict(unfazed.VCF_STATS)
    try:
        assert unfazed.vcf_route() == "device"
        unfazed.write_vcf_output(src, case["records"], case["amb"], False, dst, 10)
    finally:
        session.set_backend(None)
    assert open(dst, "rb").read() == want
    after = unfazed.VCF_STATS
    assert after["vcf_host_rows"] - before["vcf_host_rows"] == 2 and after["vcf_device_rows"] == before["vcf_device_rows"] and after["vcf_calls"] == before["vcf_calls"]


def test_the_switch_and_its_default(tmp_path, monkeypatch):
    monkeypatch.delenv("UZ_VCF_ROUTE", raising=False)
    assert unfazed.vcf_route() == unfazed.VCF_ROUTE_DEFAULT == "device"
    monkeypatch.setenv("UZ_VCF_ROUTE", "Device")
    assert unfazed.vcf_route() == "device"
    monkeypatch.setenv("UZ_VCF_ROUTE", "host")
    assert unfazed.vcf_route() == "host"
    monkeypatch.setenv("UZ_VCF_ROUTE", "anything")
    assert unfazed.vcf_route() == "host"
    # the default makes no backend: a call without one (no phasing ran in this process) is the host writer's
    monkeypatch.delenv("UZ_VCF_ROUTE")
    assert session.current_backend() is None
    case = vcfrowcases.BY_NAME["gate/0_1"]
    want = vcfrowcases.host_output(case, tmp_path)
    before = dict(unfazed.VCF_STATS)
    unfazed.write_vcf_output(str(tmp_path / "in.vcf"), case["records"], case["amb"], False, str(tmp_path / "plain.vcf"), 10)
    assert ("text", open(str(tmp_path / "plain.vcf"), "rb").read()) == want and session.current_backend() is None
    assert unfazed.VCF_STATS["vcf_host_rows"] == before["vcf_host_rows"] + 1 and unfazed.VCF_STATS["vcf_calls"] == before["vcf_calls"]


@pytest.mark.parametrize("case", [c for c in vcfrowcases.CASES if c["raw_ann"] is None], ids=lambda c: c["name"])
def test_the_table_and_the_rules_give_the_host_writers_text(case, tmp_path):
    d = vcfrowcases.decode(case)
    ann = vcfrowcases.annotations(case, d)
    assert (ann[0][1:] >= ann[0][:-1]).all() and int(ann[0][-1]) == len(ann[1]) == len(ann[2]) == len(ann[3]) == len(ann[4])
    for k in range(len(d["line_at"])):  # ascending columns inside a record
        cols = ann[1][int(ann[0][k]):int(ann[0][k + 1])]
        assert (cols[1:] > cols[:-1]).all()
    assert vcfrowcases.rules_text(d, ann, set(case["hb"])) == vcfrowcases.expected_rows(case, tmp_path)


def test_the_table_keeps_a_count_the_device_does_not_print_for_the_host():
    case = vcfrowcases.BY_NAME["uops/1000000"]
    off, col, gt, uops, uet, host_rows = unfazed.vcf_annotations(vcfrowcases.sites_of(case), case["samples"], case["records"], False, False, 10)
    assert host_rows == [0] and off.tolist() == [0, 0, 1] and (col.tolist(), gt.tolist(), uops.tolist(), uet.tolist()) == ([1], [1], [5], [0])
    case = vcfrowcases.BY_NAME["keys/dup_sample"]
    off, col, gt, uops, uet, host_rows = unfazed.vcf_annotations(vcfrowcases.sites_of(case), case["samples"], case["records"], False, False, 10)
    assert host_rows == [] and off.tolist() == [0, 2, 4] and col.tolist() == [0, 2, 0, 2] and gt.tolist() == [1, 1, 2, 2]
    # a dict whose keys are not made of its records' own fields cannot be indexed by site: the caller takes the host route
    key, rec = vcfrowcases.rec("kid", 99)
    assert unfazed.vcf_annotations([("chr1", 99, 100, "POINT")], ["kid"], {"other_key": rec}, False, False, 10) is None


class _RulesBackend:
    """a stand-in for the device: vcf_rows applies the plain-Python rules to the view it is given and hands back the case's stated records, so that
    the HOST side of the device route -- the native decode, the line starts, the header, the splice of handed-back records -- runs without a device"""

    def __init__(self, case):
        self.case, self.calls = case, 0

    def vcf_rows(self, view, line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet):
        import ctypes as C
        import numpy as np
        self.calls += 1
        n = int(view.n_records)
        arr = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (n,)).copy() if n else np.zeros(0, np.uint64)
        d = {"text": C.string_at(view.text, int(view.text_bytes)), "line_at": np.asarray(line_at, np.int64), "samp_at": arr(view.samp_at), "line_end": arr(view.line_end),
             "n_samples": int(view.n_samples)}
        want = vcfrowcases.decode(self.case)
        assert d["line_at"].tolist() == want["line_at"].tolist() and d["samp_at"].tolist() == want["samp_at"].tolist() and d["line_end"].tolist() == want["line_end"].tolist()
        hb = set(self.case["hb"])
        rows = vcfrowcases.rules_text(d, (ann_off, ann_col, ann_gt, ann_uops, ann_uet), hb)
        off = np.cumsum([0] + [0 if r is None else len(r) for r in rows]).astype(np.int64)
        return b"".join(r for r in rows if r is not None), off, np.asarray([k in hb for k in range(n)], bool)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
@pytest.mark.parametrize("name", ["samples/65", "handback/gt_1234_0", "handback/gt_a_b", "handback/col_few", "handback/no_format", "uops/1000000", "ends/crlf",
                                  "ends/empty_lines", "ends/no_final_newline", "records/0", "records/257", "keys/dup_sample", "keys/end_empty"])
def test_the_host_side_of_the_device_route(name, gz, tmp_path, monkeypatch):
    import gzip
    case = vcfrowcases.BY_NAME[name]
    want = vcfrowcases.host_output(case, tmp_path)
    src, dst = str(tmp_path / ("dnms.vcf.gz" if gz else "dnms.vcf")), str(tmp_path / "routed.vcf")
    with (gzip.open if gz else open)(src, "wb") as fh:
        fh.write(vcfrowcases.file_bytes(case))
    backend = _RulesBackend(case)
    session.set_backend(backend)
    monkeypatch.setenv("UZ_VCF_ROUTE", "device")
    before = dict(unfazed.VCF_STATS)
    try:
        unfazed.write_vcf_output(src, case["records"], case["amb"], False, dst, 10)
        got = ("text", open(dst, "rb").read())
    except Exception as e:  # noqa: BLE001 -- compared with what the host raises
        got = ("raise", type(e))
    finally:
        session.set_backend(None)
    assert got == want
    grew = {k: unfazed.VCF_STATS[k] - before[k] for k in before}
    n = len(vcfrowcases.decode(case)["line_at"])
    if name == "ends/crlf":  # (a '\r': the host route, whole)
        assert backend.calls == 0 and grew == {"vcf_device_rows": 0, "vcf_host_rows": n, "vcf_calls": 0}
    elif want[0] == "text":
        host_rows = len(case["hb"])
        assert backend.calls == 1 and grew == {"vcf_device_rows": n - host_rows, "vcf_host_rows": host_rows, "vcf_calls": 1}
