"""outfile.write_output under UZ_OUT_INDEX=tbi on the host route (UZ_OUT_BGZF=host: tabix_index.build_host, no device): the .tbi beside the
file, held to the per-line model (tests/tbxmodel.py) byte for byte and to the project's own region reader; texts that cannot be indexed; the
switch unset; plain outfiles."""
import os

import pytest

import tbxcases as panel
import tbxmodel as model
from unfazed_amd import io_native, outfile, tabix_index


@pytest.fixture
def host_route(monkeypatch):
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    monkeypatch.setenv("UZ_OUT_INDEX", "TBI")  # (any case)
    before = dict(outfile.OUT_STATS)
    yield before
    for key in outfile.INDEX_KEYS:  # the counters the switch adds leave with it: other tests see the keys they always saw
        if key not in before:
            outfile.OUT_STATS.pop(key, None)


def _grown(before):
    return {key: outfile.OUT_STATS[key] - before.get(key, 0) for key in outfile.INDEX_KEYS}


def test_the_index_is_written_beside_the_file(tmp_path, host_route):
    _, _, payload, _ = panel.BY_NAME["bulk/four-contigs"]
    path = str(tmp_path / "out.vcf.gz")
    outfile.write_output(path, [payload[:1000], payload[1000:].decode()])
    assert os.path.exists(path + ".tbi")
    assert _grown(host_route) == {"index_files": 1, "index_refused": 0, "index_host_rows": 0}
    blocks = open(path, "rb").read()
    assert model.inflate(blocks) == payload
    tables, _ = model.tables(payload, "vcf", blocks[:-28])
    assert model.inflate(open(path + ".tbi", "rb").read()) == model.tbi_bytes("vcf", tables)
    assert io_native.tabix_index_path(path) == path + ".tbi"
    assert io_native.tabix_contigs(path) == ["chr1", "chr2", "chr10", "chrX"]


def held_against_the_whole_file(path, seed, regions=10):
    """test_io_csi._held_against_the_whole_file for a file of 65 280-byte blocks: random regions through the index give the records, strings and
    raw lines of the whole-file decode restricted to them.  What is read: a region of 10 kb lies in at most two 16 kb windows, whose records
    (some 13 KB of this text) lie in at most two blocks, a third for the long records the higher bins add behind the linear index's offset:
    30 blocks of the file's 77, so less than half of it"""
    import numpy as np
    names = io_native.tabix_contigs(path)
    assert names == ["chr1", "chr2", "chrX"]
    whole = io_native.read_vcf_table(path)
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(whole.pos.size, regions, replace=False))
    ref = np.searchsorted(whole.contig_off, pick, "right") - 1
    lo, hi = whole.pos[pick] - 5002, whole.pos[pick] + 5002
    t = io_native.read_vcf_table_regions(path, [names.index(whole.contigs[r]) for r in ref], lo, hi)
    keep = np.zeros(whole.pos.size, bool)
    for r, a, b in zip(ref, lo, hi):
        c0, c1 = int(whole.contig_off[r]), int(whole.contig_off[r + 1])
        keep[c0:c1] |= (whole.pos[c0:c1] < b) & (whole.end[c0:c1] > a)
    idx = np.nonzero(keep)[0]
    assert 200 < idx.size < 0.2 * whole.pos.size and t.pos.size == idx.size
    for k in ("pos", "end", "sflags", "ref_base", "alt_base"):
        assert np.array_equal(getattr(whole, k)[idx], getattr(t, k)), k
    for k in ("gt", "ref_depth", "alt_depth", "gq"):
        assert np.array_equal(getattr(whole, k)[:, idx], getattr(t, k)), k
    assert t.samples == whole.samples and [c for c in whole.contigs if c in t.contigs] == t.contigs
    for j in range(0, idx.size, 7):
        i = int(idx[j])
        assert whole.ref_str[i] == t.ref_str[j] and whole.alt_strs[i] == t.alt_strs[j] and whole.lines[i] == t.lines[j]
    assert (whole.end - whole.pos).max() > 1000  # (long records reach into windows: the higher bins are asked too)
    print("read %d of %d bytes" % (t.io_stats[0], os.path.getsize(path)))
    assert t.io_stats[0] < 0.5 * os.path.getsize(path) and t.io_stats[3] == idx.size


def test_region_decode_through_the_index_is_the_whole_files(tmp_path, host_route):
    from test_io_native import _big_vcf_text
    path = str(tmp_path / "sites.vcf.gz")
    outfile.write_output(path, [_big_vcf_text()])
    assert os.path.exists(path + ".tbi") and io_native.tabix_index_path(path) == path + ".tbi"
    held_against_the_whole_file(path, 11)


@pytest.mark.parametrize("name", [c[0] for c in panel.CASES])
def test_every_payload_by_the_host_builder(tmp_path, host_route, name, capsys):
    """the host builder against the model on the whole panel, through write_output where the text names its own preset"""
    _, preset, payload, verdict = panel.BY_NAME[name]
    blocks, _ = outfile.host_blocks(payload)
    tables, why = tabix_index.build_host(payload, tabix_index.block_sizes(blocks), preset)
    want, _ = model.tables(payload, preset, blocks)
    assert (tables is None) == (verdict is not None) and (why is None) == (verdict is None)
    if tables is not None:
        assert tabix_index.serialize(preset, tables) == model.tbi_bytes(preset, want)
    if tabix_index.preset_of(payload) != preset:
        return
    ext = ".vcf.gz" if preset == "vcf" else ".bed.gz"
    path, plain = str(tmp_path / ("out" + ext)), str(tmp_path / ("plain" + ext))
    with open(path + ".tbi", "wb") as fh:
        fh.write(b"an earlier run's")
    outfile.write_output(path, [payload])
    err = capsys.readouterr().err
    os.environ.pop("UZ_OUT_INDEX")
    outfile.write_output(plain, [payload])
    assert open(path, "rb").read() == open(plain, "rb").read() and not os.path.exists(plain + ".tbi")
    if verdict is None:
        assert model.inflate(open(path + ".tbi", "rb").read()) == model.tbi_bytes(preset, want) and err == ""
        assert _grown(host_route) == {"index_files": 1, "index_refused": 0, "index_host_rows": 0}
    else:
        assert not os.path.exists(path + ".tbi")
        assert _grown(host_route) == {"index_files": 0, "index_refused": 1, "index_host_rows": 0}
        assert err.count("\n") == 1 and why in err and path in err


def test_no_index_without_the_switch_or_for_a_plain_file(tmp_path, monkeypatch):
    _, _, payload, _ = panel.BY_NAME["lines/one-record"]
    before = dict(outfile.OUT_STATS)
    for route, index, name in (("host", None, "a.vcf.gz"), ("host", "csi", "b.vcf.gz"), ("host", "tbi", "c.vcf"), (None, "tbi", "d.vcf.gz")):
        for key, val in (("UZ_OUT_BGZF", route), ("UZ_OUT_INDEX", index)):
            monkeypatch.delenv(key, raising=False) if val is None else monkeypatch.setenv(key, val)
        outfile.write_output(str(tmp_path / name), [payload])
        assert os.path.exists(str(tmp_path / name)) and not os.path.exists(str(tmp_path / name) + ".tbi")
    assert sorted(outfile.OUT_STATS) == sorted(before)
    monkeypatch.setenv("UZ_OUT_INDEX", "tbi")
    monkeypatch.setenv("UZ_OUT_BGZF", "host")
    outfile.write_output("/dev/stdout", [payload])
    assert sorted(outfile.OUT_STATS) == sorted(before)


def test_the_bed_preset(tmp_path, host_route):
    _, _, payload, _ = panel.BY_NAME["bed/rows"]
    path = str(tmp_path / "out.bed.gz")
    outfile.write_output(path, [payload])
    got = model.parse_tbi(model.inflate(open(path + ".tbi", "rb").read()))
    assert got["header"] == (0x10000, 1, 2, 3, ord("#"), 0) and got["names"] == [b"chr1", b"chr2"]
    tables, _ = model.tables(payload, "bed", open(path, "rb").read()[:-28])
    assert model.inflate(open(path + ".tbi", "rb").read()) == model.tbi_bytes("bed", tables)
    assert got["pseudo"][0][1] == [3, 0] and 4681 in got["bins"][0] and 585 in got["bins"][0]  # start = end is one base; 16000 .. 40000 spans windows
