"""UZ_BCF_ROUTE through the command line and the driver's writer on a device: `python -m unfazed_amd -d dnms.bcf` with the annotated VCF as its
output -- refused while the switch is not set -- written with the records' text made on the device (uz_bcf_rows) and by the plain converter, the
two files equal byte for byte; every sample's GT piece, UOPS and UET those of the same run on the text VCF the BCF was made from; the counters;
a file with one handed-back record written whole; and the panel's files, held to the host writer over the panel's literal lines."""
import os
import subprocess
import sys

import pytest

import bcfrowcases
from synth.small import SmallConfig, make_small
from tests.bcfio import write_bcf
from tests.filesio import dump_dataset
from unfazed_amd import session, unfazed
from unfazed_amd.io_vcf import read_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_the_command_line_writes_the_annotated_vcf_of_a_bcf(tmp_path, hip_lib):
    ds = make_small(SmallConfig(seed=77, n_dnms=10))
    paths = dump_dataset(ds, str(tmp_path))
    kid = list(ds.pedigrees)[0]
    smp, recs, _ = read_vcf(paths["dnm_vcf"])
    dnm_bcf = str(tmp_path / "dnms.bcf")
    write_bcf(dnm_bcf, smp, recs, ds.contigs)
    base = ["-s", paths["sites"], "-p", paths["ped"], "--build", "38", "-t", "1", "-q", "--bam-pairs", "%s:%s" % (kid, paths["bams"][kid])]

    def run(dnms, **env):
        clean = {k: v for k, v in os.environ.items() if k not in ("UZ_BCF_ROUTE", "UZ_VCF_ROUTE")}
        return subprocess.run([sys.executable, "-m", "unfazed_amd", "-d", dnms] + base, cwd=ROOT, capture_output=True, text=True, env=dict(clean, **env))
    dev, host, text = run(dnm_bcf, UZ_BCF_ROUTE="device"), run(dnm_bcf, UZ_BCF_ROUTE="host"), run(paths["dnm_vcf"])
    assert dev.returncode == 0, dev.stderr[-2000:]
    assert host.returncode == 0, host.stderr[-2000:]
    assert text.returncode == 0, text.stderr[-2000:]
    assert dev.stdout == host.stdout and dev.stdout.count("|") >= 1
    rows = lambda out: [ln.split("\t") for ln in out.split("\n") if ln and ln[0] != "#"]
    d_rows, t_rows = rows(dev.stdout), rows(text.stdout)
    assert len(d_rows) == len(t_rows) == len(recs) >= 2
    for d, t in zip(d_rows, t_rows):
        assert d[:2] == t[:2] and d[3:5] == t[3:5] and len(d) == len(t) == 9 + len(smp) and d[8].endswith(":UOPS:UET")
        gd, gt = d[8].split(":").index("GT"), t[8].split(":").index("GT")
        for cd, ct in zip(d[9:], t[9:]):
            assert cd.split(":")[gd] == ct.split(":")[gt] and cd.split(":")[-2:] == ct.split(":")[-2:]
    # not set: the refusal, as before
    none = run(dnm_bcf)
    assert none.returncode != 0 and "BCF" in (none.stderr + none.stdout)


@pytest.fixture()
def routed(engine, tmp_path, monkeypatch):
    session.set_backend(engine)

    def route(case, env, chunk=None):
        src = str(tmp_path / "dnms.bcf")
        open(src, "wb").write(bcfrowcases.file_bytes(case))
        if chunk:
            monkeypatch.setenv("UZ_BCFOUT_CHUNK_BYTES", str(chunk))
        else:
            monkeypatch.delenv("UZ_BCFOUT_CHUNK_BYTES", raising=False)
        before = dict(unfazed.BCF_STATS)
        got = bcfrowcases.host_writer(src, str(tmp_path / "out.vcf"), bcfrowcases.route_records(case), env, monkeypatch)
        return got, {k: unfazed.BCF_STATS[k] - before[k] for k in before}

    yield route
    session.set_backend(None)


def _want(case, tmp_path, monkeypatch, lines=None):
    ref = str(tmp_path / "lines.vcf")
    open(ref, "wb").write(bcfrowcases.text_file_bytes(case, lines))
    return bcfrowcases.host_writer(ref, str(tmp_path / "want.vcf"), bcfrowcases.route_records(case, lines), {"UZ_VCF_ROUTE": "host"}, monkeypatch)


@pytest.mark.parametrize("case", [c for c in bcfrowcases.CASES if c["file_ok"] and c["lines"]], ids=lambda c: c["name"])
def test_panel_files_through_the_driver(routed, case, tmp_path, monkeypatch):
    want = _want(case, tmp_path, monkeypatch)
    got, grew = routed(case, {"UZ_BCF_ROUTE": "device"}, chunk=case["chunk"])
    assert got == want, case["name"]
    assert grew == {"bcf_device_rows": len(case["lines"]), "bcf_host_rows": 0, "bcf_calls": 1}


def test_a_file_with_a_handed_back_record_is_written_whole(routed, tmp_path, monkeypatch):
    base = bcfrowcases.BY_NAME["records/65"]
    recs, lines = list(base["records"]), list(base["lines"])
    g = bcfrowcases
    for k, qual, text in ((0, 1e6, "1e+06"), (31, 2.5e-7, "2.5e-07"), (64, float("inf"), "inf")):  # (first, inside, last: QUAL in exponent form)
        recs[k] = g.record(pos=10 * k, qual=g.fbits(qual), fmt=[g.fmt_ints("GT", [g.gt("0/1"), g.gt("1/1"), g.gt("./.")], 1)], n_sample=3)
        lines[k] = "chr1\t%d\t.\tA\tT\t%s\tPASS\t.\tGT\t0/1\t1/1\t./." % (10 * k + 1, text)
    case = dict(base, records=recs, lines=lines, name="one_handed_back")
    want = _want(case, tmp_path, monkeypatch, lines)
    assert want[0] == "text" and want[1].count(b"1|0") >= 60
    got, grew = routed(case, {"UZ_BCF_ROUTE": "device"}, chunk=700)
    assert got == want and grew == {"bcf_device_rows": 62, "bcf_host_rows": 3, "bcf_calls": 1}
    got, grew = routed(case, {"UZ_BCF_ROUTE": "host"})
    assert got == want and grew == {"bcf_device_rows": 0, "bcf_host_rows": 65, "bcf_calls": 0}
