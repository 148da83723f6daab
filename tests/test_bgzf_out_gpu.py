"""UZ_OUT_BGZF=device through the command line: the golden runs of tests/test_cli_golden.py with --outfile out.vcf.gz / out.bed.gz.  The file must
inflate to exactly the file the same run writes with the switch unset, and carry the ISIZE and CRC-32 sequence of the host route's file."""
import gzip
import os
import subprocess
import sys

import pytest

import bgzfoutcases as panel
from test_cli_golden import ROOT, _argv, _check, _inputs
from unfazed_amd import outfile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    return _inputs(tmp_path_factory.mktemp("bgzf_out_gpu"))


@pytest.mark.parametrize("k", range(5))
def test_golden_runs_written_as_bgzf_on_the_device(golden, tmp_path, hip_lib, monkeypatch, k):
    g, ds, paths = golden
    assert len(g["runs"]) == 5
    run = g["runs"][k]
    ext = run["output_type"]
    plain, packed, by_host = str(tmp_path / ("plain." + ext + ".gz")), str(tmp_path / ("out." + ext + ".gz")), str(tmp_path / ("host." + ext + ".gz"))
    env = {key: v for key, v in os.environ.items() if key not in ("UZ_OUT_BGZF", "UZ_BCF_ROUTE")}
    env["PYTHONHASHSEED"] = "0"  # (two processes are compared byte for byte: the verbose BED lists read names in a set's order)
    cmd = [sys.executable, "-m", "unfazed_amd"] + _argv(paths, run)
    subprocess.run(cmd + ["--outfile", plain], cwd=ROOT, check=True, capture_output=True, text=True, env=env)
    want = open(plain, "rb").read()  # a ".gz" name, and plain text: today's behaviour
    _check(run, want.decode(), len(ds.samples))
    dev_env = dict(env, UZ_OUT_BGZF="device")
    if k == 3:
        dev_env["UZ_BCF_ROUTE"] = "device"
    subprocess.run(cmd + ["--outfile", packed], cwd=ROOT, check=True, capture_output=True, text=True, env=dev_env)
    got = open(packed, "rb").read()
    assert got.endswith(panel.EOF_MARKER) and gzip.decompress(got) == want
    parts = panel.check_blocks(want, got[:-len(panel.EOF_MARKER)])
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    outfile.write_output(by_host, [want])
    host = open(by_host, "rb").read()
    assert host.endswith(panel.EOF_MARKER) and gzip.decompress(host) == want
    host_parts = panel.split_blocks(host[:-len(panel.EOF_MARKER)])
    assert [(p[2], p[3]) for p in parts] == [(p[2], p[3]) for p in host_parts] and parts


def test_the_device_route_counts_its_blocks(engine, tmp_path, monkeypatch):
    from unfazed_amd import session
    session.set_backend(engine)
    try:
        monkeypatch.setenv("UZ_OUT_BGZF", "device")
        text = panel.BY_NAME["text/vcf"]
        before = dict(outfile.OUT_STATS)
        outfile.write_output(str(tmp_path / "x.vcf.gz"), [text[:1000], text[1000:].decode()])
        grown = {key: outfile.OUT_STATS[key] - before[key] for key in before}
        assert grown == {"bgzf_device_blocks": 5, "bgzf_host_blocks": 0, "bgzf_calls": 1}
        assert gzip.decompress(open(str(tmp_path / "x.vcf.gz"), "rb").read()) == text
        outfile.write_output(str(tmp_path / "x.vcf"), [text])
        assert open(str(tmp_path / "x.vcf"), "rb").read() == text
    finally:
        session.set_backend(None)
