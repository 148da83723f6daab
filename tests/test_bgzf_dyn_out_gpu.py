"""UZ_OUT_BGZF=device with UZ_OUT_BGZF_CODE=dynamic through the command line: one golden run of tests/test_cli_golden.py with --outfile
out.vcf.gz.  The file must inflate to exactly the file the same run writes with the switches unset, be smaller than the fixed code's file, and
its blocks must count as dynamic."""
import gzip
import os
import subprocess
import sys

import pytest

import bgzfoutcases as panel
from test_cli_golden import ROOT, _argv, _check, _inputs
from unfazed_amd import outfile

pytestmark = pytest.mark.gpu


def test_a_golden_run_written_with_the_dynamic_code(tmp_path_factory, tmp_path, hip_lib):
    g, ds, paths = _inputs(tmp_path_factory.mktemp("bgzf_dyn_out_gpu"))
    run = next(r for r in g["runs"] if r["output_type"] == "vcf")
    plain, fixed, packed = (str(tmp_path / n) for n in ("plain.vcf.gz", "fixed.vcf.gz", "out.vcf.gz"))
    env = {key: v for key, v in os.environ.items() if key not in ("UZ_OUT_BGZF", "UZ_OUT_BGZF_CODE", "UZ_BCF_ROUTE")}
    env["PYTHONHASHSEED"] = "0"
    cmd = [sys.executable, "-m", "unfazed_amd"] + _argv(paths, run)
    subprocess.run(cmd + ["--outfile", plain], cwd=ROOT, check=True, capture_output=True, text=True, env=env)
    want = open(plain, "rb").read()  # a ".gz" name, and plain text
    _check(run, want.decode(), len(ds.samples))
    subprocess.run(cmd + ["--outfile", fixed], cwd=ROOT, check=True, capture_output=True, text=True, env=dict(env, UZ_OUT_BGZF="device"))
    subprocess.run(cmd + ["--outfile", packed], cwd=ROOT, check=True, capture_output=True, text=True,
                   env=dict(env, UZ_OUT_BGZF="device", UZ_OUT_BGZF_CODE="Dynamic"))
    got = open(packed, "rb").read()
    assert got.endswith(panel.EOF_MARKER) and gzip.decompress(got) == want
    parts = panel.check_blocks(want, got[:-len(panel.EOF_MARKER)])
    assert parts and (parts[0][1][0] >> 1) & 3 == 2  # BTYPE 10: a block of VCF text is shorter in a code of its own
    by_fixed = open(fixed, "rb").read()
    assert gzip.decompress(by_fixed) == want and len(got) < len(by_fixed)


def test_the_device_route_counts_the_blocks_forms(engine, tmp_path, monkeypatch):
    from unfazed_amd import session
    session.set_backend(engine)
    try:
        monkeypatch.setenv("UZ_OUT_BGZF", "device")
        text = panel.BY_NAME["text/vcf"] + panel.BY_NAME["random/65280"][:-(len(panel.BY_NAME["text/vcf"]) % panel.SLICE)] + b"xyz"
        grown = []
        for code in ("dynamic", None):
            if code:
                monkeypatch.setenv("UZ_OUT_BGZF_CODE", code)
            else:
                monkeypatch.delenv("UZ_OUT_BGZF_CODE")
            stats, kinds = dict(outfile.OUT_STATS), dict(outfile.OUT_KINDS)
            outfile.write_output(str(tmp_path / "x.vcf.gz"), [text[:1000], text[1000:]])
            assert gzip.decompress(open(str(tmp_path / "x.vcf.gz"), "rb").read()) == text
            assert {key: outfile.OUT_STATS[key] - stats[key] for key in stats} == {"bgzf_device_blocks": 6, "bgzf_host_blocks": 0, "bgzf_calls": 1}
            grown.append({key: outfile.OUT_KINDS[key] - kinds[key] for key in kinds})
            assert sorted(outfile.OUT_STATS) == ["bgzf_calls", "bgzf_device_blocks", "bgzf_host_blocks"]
        # four slices of text, one that ends in bytes that do not compress, and the last three bytes
        assert grown[0]["dynamic"] >= 4 and grown[0]["fixed"] >= 1 and sum(grown[0].values()) == 6
        assert grown[1]["dynamic"] == 0 and sum(grown[1].values()) == 6
    finally:
        session.set_backend(None)
