"""The per-line model of the tabix index (tests/tbxmodel.py) held to the TBI writer the tests had before it, filesio.write_tbi: a Python loop over
the re-inflated file.  On every VCF payload of the panel that can be indexed and has a meta line, the model's tables over the file host_blocks
writes, in the TBI layout and parsed again, are write_tbi's: names, header integers, every bin's chunks, the linear index.  (Without a meta line
the first record's offset is 0, which write_tbi's linear index reads as "empty": those payloads are held to the model alone, elsewhere.)  The
pseudo-bin, which write_tbi does not write, is held to the rows by itself."""
import pytest

import tbxcases as panel
import tbxmodel as model
from filesio import write_tbi
from unfazed_amd import outfile

VCF = [c[0] for c in panel.CASES if c[1] == "vcf"]


@pytest.mark.parametrize("name", VCF)
def test_the_models_tables_are_write_tbis(tmp_path, name):
    _, preset, payload, verdict = panel.BY_NAME[name]
    blocks, _ = outfile.host_blocks(payload)
    tables, why = model.tables(payload, preset, blocks)
    assert why == verdict and (tables is None) == (verdict is not None)
    if tables is None or not payload.startswith(b"#"):
        return
    path = str(tmp_path / "x.vcf.gz")
    with open(path, "wb") as fh:
        fh.write(blocks + outfile.BGZF_EOF)
    mine = model.parse_tbi(model.tbi_bytes(preset, tables))
    theirs = model.parse_tbi(model.inflate(open(write_tbi(path), "rb").read()))
    for key in ("header", "names", "bins", "linear"):
        assert mine[key] == theirs[key], key
    assert theirs["pseudo"] == {} and sorted(mine["pseudo"]) == list(range(len(mine["names"])))
    # the pseudo-bin: the reference's first offset and last end, its record count
    rows = [(r, payload[r["at"]:r["at"] + r["name_len"]]) for r in model.rows(payload, preset) if r["kind"] == model.DATA]
    for t, ref in enumerate(mine["names"]):
        (v0, v1), (count, zero) = mine["pseudo"][t]
        chunks = sorted(c for cs in mine["bins"][t].values() for c in cs)
        assert (v0, v1, zero) == (chunks[0][0], max(c[1] for c in chunks), 0)
        assert count == sum(1 for _, nm in rows if nm == ref)


def test_the_panel_has_what_the_rules_have():
    verdicts = {c[3] for c in panel.CASES}
    assert verdicts == {None, "order", "contig", "range", "meta", "empty", "cr", "pos"}
    assert all(len(c[2]) <= 400_000 for c in panel.CASES)
    levels = set()
    for name in ("pos/levels", "bins/a-b-a", "linear/gaps", "bulk/four-contigs"):
        _, preset, payload, _ = panel.BY_NAME[name]
        tables, _ = model.tables(payload, preset, outfile.host_blocks(payload)[0])
        for bins in tables["bins"]:
            for b in bins:
                levels.add(sum(b >= first for first in (1, 9, 73, 585, 4681)))
        if name == "bins/a-b-a":
            assert sorted(len(v) for v in tables["bins"][0].values()) == [1, 2]
        if name == "linear/gaps":
            assert tables["linear"][0][0] == tables["linear"][0][6] and len(set(tables["linear"][0])) == 3 and len(tables["linear"][0]) == 55
    assert levels == {0, 1, 2, 3, 4, 5}
