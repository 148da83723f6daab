"""The annotated-VCF writer's device route through the driver (UZ_VCF_ROUTE=device: unfazed.write_vcf_output -> engine.vcf_rows): the golden
command-line runs that write a VCF, both routes on a generated file with SV records mixed in, the counters, a handed-back record written by the
per-record host code, and the panel's files (tests/vcfrowcases.py) -- the host writer's file, or the host writer's exception."""
import os
import subprocess
import sys

import pytest

import vcfrowcases
from test_cli_golden import ROOT, _argv, _check, _inputs
from unfazed_amd import session, unfazed

pytestmark = pytest.mark.gpu


def test_golden_runs_on_the_device_route(tmp_path, hip_lib):
    g, ds, paths = _inputs(tmp_path)
    runs = [r for r in g["runs"] if r["output_type"] == "vcf"]
    assert runs
    env = dict(os.environ, UZ_VCF_ROUTE="device")
    for run in runs:
        out = subprocess.run([sys.executable, "-m", "unfazed_amd"] + _argv(paths, run), cwd=ROOT, check=True, capture_output=True, text=True, env=env)
        _check(run, out.stdout, len(ds.samples))
        host = subprocess.run([sys.executable, "-m", "unfazed_amd"] + _argv(paths, run), cwd=ROOT, check=True, capture_output=True, text=True,
                              env=dict(os.environ, UZ_VCF_ROUTE="host"))
        assert out.stdout == host.stdout


@pytest.fixture()
def routed(engine, tmp_path, monkeypatch):
    """route(case) -> ("text", bytes) or ("raise", type) of the driver's writer on the device route, and the counters' growth"""
    session.set_backend(engine)

    def route(case, chunk=None):
        src, dst = str(tmp_path / "in_dev.vcf"), str(tmp_path / "out_dev.vcf")
        with open(src, "wb") as fh:
            fh.write(vcfrowcases.file_bytes(case))
        monkeypatch.setenv("UZ_VCF_ROUTE", "device")
        if chunk or case["chunk"]:
            monkeypatch.setenv("UZ_VCFOUT_CHUNK_BYTES", str(chunk or case["chunk"]))
        else:
            monkeypatch.delenv("UZ_VCFOUT_CHUNK_BYTES", raising=False)
        before = dict(unfazed.VCF_STATS)
        try:
            unfazed.write_vcf_output(src, case["records"], case["amb"], False, dst, 10)
        except Exception as e:  # noqa: BLE001 -- compared with what the host raises
            return ("raise", type(e)), {k: unfazed.VCF_STATS[k] - before[k] for k in before}
        finally:
            monkeypatch.delenv("UZ_VCF_ROUTE")
        return ("text", open(dst, "rb").read()), {k: unfazed.VCF_STATS[k] - before[k] for k in before}

    yield route
    session.set_backend(None)


def _generated(amb):
    fuzz = vcfrowcases.fuzz_cases(77, 200, per_case=200)[0]
    names = ["s%d" % i for i in range(8)]
    import random
    rng = random.Random(5)
    lines, records = [], []
    for k in range(200):
        sv = k % 5 == 0
        pos = 1000 + 20 * k
        cells = ["%s:%d:%d" % (rng.choice(vcfrowcases.GATE_FORMS), rng.randrange(60), rng.randrange(99)) for _ in names]
        lines.append(vcfrowcases.line(pos, cells, fmt="GT:DP:GQ", info="SVTYPE=%s;END=%d" % (rng.choice(["DEL", "DUP"]), pos + 400) if sv else "."))
        for i in rng.sample(range(8), 2):
            vt = lines[-1].split(b"SVTYPE=")[1][:3].decode() if sv else "POINT"
            records.append(vcfrowcases.rec(names[i], pos - 1, pos + 400 if sv else pos, vartype=vt, nd=rng.randrange(4), nm=rng.randrange(3),
                                           cd=rng.randrange(3) if sv else 0, cm=rng.randrange(3) if sv else 0))
    return dict(fuzz, name="generated", header=vcfrowcases.header(names), samples=names, lines=lines, records=dict(records), amb=amb, hb=[])


@pytest.mark.parametrize("amb", [False, True], ids=["unambiguous", "include_ambiguous"])
def test_both_routes_write_the_same_file(routed, tmp_path, amb):
    case = _generated(amb)
    want = vcfrowcases.host_output(case, tmp_path)
    assert want[0] == "text" and want[1].count(b"|") > 20
    got, grew = routed(case, chunk=8192)
    assert got == want
    assert grew == {"vcf_device_rows": 200, "vcf_host_rows": 0, "vcf_calls": 1}


def test_a_handed_back_record_is_written_by_the_host_code(routed, tmp_path):
    case = vcfrowcases.BY_NAME["handback/gt_1234_0"]  # (its genotype is outside the device's grammar and inside Python's int)
    want = vcfrowcases.host_output(case, tmp_path)
    assert want[0] == "text"
    got, grew = routed(case)
    assert got == want and grew == {"vcf_device_rows": 2, "vcf_host_rows": 1, "vcf_calls": 1}
    case = vcfrowcases.BY_NAME["uops/1000000"]  # (a count the host keeps for itself)
    got, grew = routed(case)
    assert got == vcfrowcases.host_output(case, tmp_path) and b"1e+06" in got[1] and grew == {"vcf_device_rows": 1, "vcf_host_rows": 1, "vcf_calls": 1}


@pytest.mark.parametrize("case", [c for c in vcfrowcases.CASES if c["raw_ann"] is None], ids=lambda c: c["name"])
def test_panel_files_through_the_driver(routed, case, tmp_path):
    want = vcfrowcases.host_output(case, tmp_path)
    got, grew = routed(case)
    assert got == want, case["name"]
    n = len(vcfrowcases.decode(case)["line_at"])
    if want[0] == "text":
        assert grew["vcf_device_rows"] + grew["vcf_host_rows"] == n


def test_the_default_route_is_the_device_where_the_call_has_a_backend(engine, tmp_path, monkeypatch):
    case = vcfrowcases.BY_NAME["samples/65"]
    want = vcfrowcases.host_output(case, tmp_path)
    monkeypatch.delenv("UZ_VCF_ROUTE", raising=False)
    monkeypatch.delenv("UZ_VCFOUT_CHUNK_BYTES", raising=False)
    session.set_backend(engine)
    before = dict(unfazed.VCF_STATS)
    try:
        unfazed.write_vcf_output(str(tmp_path / "in.vcf"), case["records"], case["amb"], False, str(tmp_path / "default.vcf"), 10)
    finally:
        session.set_backend(None)
    assert ("text", open(str(tmp_path / "default.vcf"), "rb").read()) == want
    assert {k: unfazed.VCF_STATS[k] - before[k] for k in before} == {"vcf_device_rows": 2, "vcf_host_rows": 0, "vcf_calls": 1}
