"""UZ_OUT_BGZF_CODE without a device: the switch is read on the device route alone, so with UZ_OUT_BGZF=host, and with UZ_OUT_BGZF unset, an
outfile is what it is today, byte for byte, whatever UZ_OUT_BGZF_CODE says."""
import pytest

import bgzfoutcases as panel
from unfazed_amd import outfile

TEXT = panel.BY_NAME["text/vcf"]


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for key in ("UZ_OUT_BGZF", "UZ_OUT_BGZF_LEVEL", "UZ_OUT_BGZF_CODE"):
        monkeypatch.delenv(key, raising=False)


def _write(tmp_path, name):
    path = str(tmp_path / name)
    outfile.write_output(path, [TEXT[:500], TEXT[500:].decode()])
    return open(path, "rb").read()


def test_the_code_switch_is_read_as_stated(monkeypatch):
    assert outfile.out_code() == "fixed"
    for value, want in (("dynamic", "dynamic"), ("DYNAMIC", "dynamic"), ("Dynamic", "dynamic"), ("fixed", "fixed"), ("", "fixed"), ("1", "fixed"), ("dyn", "fixed")):
        monkeypatch.setenv("UZ_OUT_BGZF_CODE", value)
        assert outfile.out_code() == want, value


def test_the_host_route_and_the_plain_file_ignore_it(tmp_path, monkeypatch):
    plain = _write(tmp_path, "plain.vcf.gz")
    assert plain == TEXT
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    by_host = _write(tmp_path, "host.vcf.gz")
    assert by_host.endswith(panel.EOF_MARKER) and by_host != plain
    kinds, stats = dict(outfile.OUT_KINDS), dict(outfile.OUT_STATS)
    assert sorted(kinds) == ["dynamic", "fixed", "stored"] and sorted(stats) == ["bgzf_calls", "bgzf_device_blocks", "bgzf_host_blocks"]
    for value in ("dynamic", "DYNAMIC", "fixed"):
        monkeypatch.setenv("UZ_OUT_BGZF_CODE", value)
        monkeypatch.setenv("UZ_OUT_BGZF", "host")
        assert _write(tmp_path, "host2.vcf.gz") == by_host, value
        monkeypatch.delenv("UZ_OUT_BGZF")
        assert _write(tmp_path, "plain2.vcf.gz") == plain, value
    assert outfile.OUT_KINDS == kinds  # the split counts the device's blocks alone
    assert {key: outfile.OUT_STATS[key] - stats[key] for key in stats} == {"bgzf_device_blocks": 0, "bgzf_host_blocks": 15, "bgzf_calls": 3}
