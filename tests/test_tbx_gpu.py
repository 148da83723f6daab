"""uz_bgzf_deflate_indexed on the device (unfazed_amd/csrc/k_tbx.hip) over the whole panel (tests/tbxcases.py), at every chunk size and code:
the blocks are uz_bgzf_deflate_coded's byte for byte; the tables, serialized, are the per-line model's on the written file, byte for byte; a
text that cannot be indexed is refused for the model's reason; and the rows the host settled are exactly the first and cut lines the payload has
-- a kernel that handed every row back, or none, fails here.  Then write_output on the device route, and one golden command-line run."""
import os
import subprocess
import sys

import pytest

import tbxcases as panel
import tbxmodel as model
from unfazed_amd import io_native, outfile, tabix_index

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in panel.CASES]
REASON = {"order": 1, "range": 2, "meta": 4, "empty": 8, "cr": 16, "pos": 32}  # unfazed_hip.h UZ_TBX_S_*


@pytest.mark.parametrize("code", ["fixed", "dynamic"])
@pytest.mark.parametrize("chunk", [65280, 130560, None])
@pytest.mark.parametrize("name", NAMES)
def test_blocks_and_tables(engine, monkeypatch, name, chunk, code):
    _, preset, payload, verdict = panel.BY_NAME[name]
    if chunk is None:
        monkeypatch.delenv("UZ_BGZF_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("UZ_BGZF_CHUNK_BYTES", str(chunk))
    want_blocks, want_n, _ = engine.bgzf_deflate(payload, code=code)
    blocks, n, _, dev = engine.bgzf_deflate(payload, code=code, index=preset)
    assert (blocks, n) == (want_blocks, want_n)
    assert model.inflate(blocks + outfile.BGZF_EOF) == payload
    assert dev["n_rows"] == len(model.lines(payload))
    # the host's rows: by the model's count, by hand where the payload was built around an edge, one per chunk at the default chunk size
    assert dev["host_rows"] == model.host_rows(payload, preset, chunk)
    if chunk is None:
        assert dev["host_rows"] == 1
    elif name in panel.HOST_ROWS:
        assert dev["host_rows"] == panel.HOST_ROWS[name][chunk]
    tables, why = tabix_index.from_device(payload, dev)
    want, model_why = model.tables(payload, preset, blocks)
    assert model_why == verdict
    if verdict is None:
        assert why is None and dev["status"] == 0
        assert tabix_index.serialize(preset, tables) == model.tbi_bytes(preset, want)
    else:
        assert tables is None and why is not None
        if verdict == "contig":
            assert dev["status"] == 0 and why == tabix_index.CONTIG_BACK
        else:
            assert dev["status"] & REASON[verdict]
        assert dev["refs"].size == dev["runs"].size == dev["linear"].size == 0 or verdict == "contig"


def test_the_empty_text(engine):
    blocks, n, _, dev = engine.bgzf_deflate(b"", index="vcf")
    assert (blocks, n) == (b"", 0) and dev["n_rows"] == dev["host_rows"] == dev["status"] == 0 and dev["refs"].size == 0
    with pytest.raises(ValueError):
        engine.bgzf_deflate(b"x", index="csi")


def test_the_device_route_writes_the_index(engine, tmp_path, monkeypatch):
    from test_io_native import _big_vcf_text
    from test_tbx_out_host import held_against_the_whole_file
    from unfazed_amd import session
    session.set_backend(engine)
    before = dict(outfile.OUT_STATS)
    try:
        monkeypatch.setenv("UZ_OUT_BGZF", "device")
        monkeypatch.setenv("UZ_OUT_INDEX", "tbi")
        monkeypatch.setenv("UZ_BGZF_CHUNK_BYTES", str(16 * 65280))  # five chunks of the 5 MB text
        path = str(tmp_path / "sites.vcf.gz")
        text = _big_vcf_text().encode()
        outfile.write_output(path, [text])
        grown = {key: outfile.OUT_STATS[key] - before.get(key, 0) for key in outfile.INDEX_KEYS}
        n_chunks = -(-len(text) // (16 * 65280))
        assert grown["index_files"] == 1 and grown["index_refused"] == 0 and n_chunks <= grown["index_host_rows"] <= 2 * n_chunks
        assert grown["index_host_rows"] == model.host_rows(text, "vcf", 16 * 65280)
        data = open(path, "rb").read()
        want, _ = model.tables(text, "vcf", data[:-28])
        assert model.inflate(open(path + ".tbi", "rb").read()) == model.tbi_bytes("vcf", want)
        held_against_the_whole_file(path, 12)
        # a text that cannot be indexed: the data file as ever, the earlier index gone
        bad = panel.BY_NAME["order/decreasing"][2]
        outfile.write_output(path, [bad])
        assert model.inflate(open(path, "rb").read()) == bad and not os.path.exists(path + ".tbi")
        assert outfile.OUT_STATS["index_refused"] - before.get("index_refused", 0) == 1
    finally:
        session.set_backend(None)
        for key in outfile.INDEX_KEYS:
            if key not in before:
                outfile.OUT_STATS.pop(key, None)


def test_a_golden_run_with_its_index(tmp_path, hip_lib):
    """the annotated VCF of tests/golden/cli.json written under UZ_OUT_BGZF=device UZ_OUT_INDEX=tbi: the .tbi is there, it is the model's, and the
    records of every region read through it are the whole file's"""
    import numpy as np
    from test_cli_golden import ROOT, _argv, _inputs
    g, ds, paths = _inputs(tmp_path)
    run = g["runs"][3]
    assert run["output_type"] == "vcf"
    out = str(tmp_path / "out.vcf.gz")
    env = dict(os.environ, UZ_OUT_BGZF="device", UZ_OUT_INDEX="tbi", UZ_BCF_ROUTE="device", PYTHONHASHSEED="0")
    done = subprocess.run([sys.executable, "-m", "unfazed_amd"] + _argv(paths, run) + ["--outfile", out], cwd=ROOT, check=True, capture_output=True, text=True, env=env)
    assert os.path.exists(out + ".tbi") and "no index written" not in done.stderr
    data = open(out, "rb").read()
    text = model.inflate(data)
    want, why = model.tables(text, "vcf", data[:-28])
    assert why is None and model.inflate(open(out + ".tbi", "rb").read()) == model.tbi_bytes("vcf", want)
    names = io_native.tabix_contigs(out)
    assert names == [nm.decode() for nm in want["names"]]
    whole = io_native.read_vcf_table(out)
    assert whole.pos.size == len(run["body"])
    for i in range(whole.pos.size):
        r = int(np.searchsorted(whole.contig_off, i, "right") - 1)
        t = io_native.read_vcf_table_regions(out, [names.index(whole.contigs[r])], np.array([whole.pos[i] - 2]), np.array([whole.pos[i] + 2]))
        c0, c1 = int(whole.contig_off[r]), int(whole.contig_off[r + 1])
        idx = [j for j in range(c0, c1) if whole.pos[j] < whole.pos[i] + 2 and whole.end[j] > whole.pos[i] - 2]
        assert i in idx and [whole.lines[j] for j in idx] == list(t.lines) and np.array_equal(whole.pos[idx], t.pos)
