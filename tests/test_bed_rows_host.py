"""The host side of the BED route without a device: summarize.BedRows orders and merges as summarize.bed_lines does, and
snv_phaser.phase_snvs_bed / UZ_BED_ROUTE=device on a backend without bed_rows (the CPU oracle) take the dict route and print the same text."""
import contextlib
import copy
import io

import pytest

import bedcases
from test_cli_golden import _argv, _inputs
from unfazed_amd import summarize


def _rec(chrom, start, end, kid="k", vartype="POINT", n_dad=2, n_mom=0, sex=False):
    row = dict(chrom=chrom, start=start, end=end, vartype=vartype, kid=kid, dad="D", mom="M", dnm=None if sex else 0)
    case = dict(names=["r%d" % k for k in range(n_dad + n_mom)],
                dnms=[dict(status=0, lists=(list(range(n_dad)), list(range(n_dad, n_dad + n_mom)), [7, 10, 9000], [8]))])
    return "_".join([chrom, str(start), str(end), kid, vartype]), bedcases.record_of(case, row)


RECORDS = [
    _rec("chr2", 5, 6), _rec("chr10", 5, 6), _rec("chr1", 100, 101), _rec("chr1", 100, 101, kid="k2"), _rec("chr1", 100, 99), _rec("chr1", 20, 21, n_dad=1, n_mom=1),
    _rec("1", 3, 4, n_dad=0, n_mom=3), _rec("chr1", 100, 101, kid="k3", n_dad=0, n_mom=0), _rec("chrY", 1, 2, sex=True), _rec("chrX", 1, 2, sex=True),
    _rec("chr1", -5, 0), _rec("chr1", 2147483647, 2147483647),
]


@pytest.mark.parametrize("verbose", [False, True])
@pytest.mark.parametrize("ambiguous", [False, True])
def test_bed_rows_orders_as_bed_lines(verbose, ambiguous):
    records = dict(RECORDS)
    assert len(records) == len(RECORDS)
    rows = summarize.BedRows(ambiguous, verbose, 10)
    rows.add_records(records)
    want = summarize.bed_lines(records, ambiguous, verbose, 10)
    assert rows.lines() == want
    assert rows.text() == "\n".join(want) + "\n"
    # ties keep the insertion order (stable): the two kids at chr1:100-101
    tied = [ln for ln in rows.lines() if ln.startswith("chr1\t100\t101\t")]
    assert [ln.split("\t")[4] for ln in tied][:2] == ["k", "k2"]


def test_a_key_that_comes_again_keeps_its_place_and_takes_the_new_content():
    first = dict(RECORDS)
    again_key, again = _rec("chr1", 100, 101, n_dad=0, n_mom=4)  # the key of RECORDS[2], another decision
    gone_key, gone = _rec("chr2", 5, 6, n_dad=1, n_mom=1)        # RECORDS[0] turns ambiguous: its line goes away
    sv_key, sv = _rec("chr1", 100, 101, vartype="DEL")           # a new key: behind everything else among its ties
    second = {again_key: again, gone_key: gone, sv_key: sv}
    merged = dict(first)
    merged.update(second)
    for verbose in (False, True):
        rows = summarize.BedRows(False, verbose, 10)
        rows.add_records(first)
        rows.add_records(second)
        assert rows.lines() == summarize.bed_lines(merged, False, verbose, 10)
    body = rows.lines()[1:]
    assert not any(ln.startswith("chr2\t") for ln in body)
    assert [ln.split("\t")[3:6] for ln in body if ln.startswith("chr1\t100\t101\t")][0] == ["POINT", "k", "M"]


def test_write_merges_extra_records_and_prints_what_write_bed_output_prints(tmp_path):
    snv, sv = dict(RECORDS[:6]), dict([_rec("chr1", 50, 900, vartype="DEL"), _rec("chr1", 100, 101, vartype="DUP", n_dad=0, n_mom=2)])
    merged = dict(snv)
    merged.update(sv)
    a, b = tmp_path / "a.bed", tmp_path / "b.bed"
    rows = summarize.BedRows(True, True, 10)
    rows.add_records(snv)
    rows.write(str(a), extra_records=sv)
    summarize.write_bed_output(merged, True, True, str(b), 10)
    assert a.read_bytes() == b.read_bytes()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rows.write("/dev/stdout")
    assert out.getvalue() == b.read_text()


def _oracle_session():
    from oracle_backend import OracleBackend
    from unfazed_amd import session
    session.set_backend(OracleBackend())
    session._READS.clear()
    session._HOSTS.clear()
    return session


def _cli(args):
    from unfazed_amd.unfazed import unfazed
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        unfazed(args)
    return buf.getvalue()


def test_the_route_switch_on_a_backend_without_bed_rows(tmp_path, monkeypatch):
    """every `bed` run of cli.json: UZ_BED_ROUTE=device prints what the default prints, and phase_snvs_bed(...).lines() equals
    bed_lines(phase_snvs(...)) on the arguments the driver passed"""
    from unfazed_amd import snv_phaser
    from unfazed_amd import unfazed as driver
    from unfazed_amd.__main__ import setup_args
    g, ds, paths = _inputs(tmp_path)
    session = _oracle_session()
    calls = []

    def spy(*a, **kw):
        calls.append((copy.deepcopy(a), dict(kw)))
        rows = snv_phaser.phase_snvs_bed(*a, **kw)
        calls[-1] += (rows,)
        return rows
    monkeypatch.setattr(driver, "phase_snvs_bed", spy)
    try:
        runs = [r for r in g["runs"] if r["output_type"] == "bed"]
        assert runs
        for run in runs:
            args = setup_args().parse_args(_argv(paths, run))
            monkeypatch.delenv("UZ_BED_ROUTE", raising=False)
            want = _cli(args)
            n = len(calls)
            monkeypatch.setenv("UZ_BED_ROUTE", "device")
            assert _cli(args) == want
            assert len(calls) == n + 1  # (the switch really took the new entry point)
            a, kw, rows = calls[-1]
            flags = dict(include_ambiguous=kw.pop("include_ambiguous"), verbose=kw.pop("verbose"))
            records = snv_phaser.phase_snvs(*a, **kw)
            assert rows.lines() == summarize.bed_lines(records, flags["include_ambiguous"], flags["verbose"], kw["evidence_min_ratio"])
        monkeypatch.setenv("UZ_BED_ROUTE", "device")
        n = len(calls)
        for run in g["runs"]:
            if run["output_type"] == "vcf":
                _cli(setup_args().parse_args(_argv(paths, run)))
        assert len(calls) == n  # annotated-VCF output keeps the dict route
    finally:
        session.set_backend(None)
        for k in [k for k in session._SITES if "@" in k]:
            del session._SITES[k]
