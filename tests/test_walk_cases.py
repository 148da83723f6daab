"""The panel of tests/walkcases.py on the CPU: the plain model of the device's walk, filter and extract (tests/walkmodel.py) is held against the
host's walk of the same plan (uz_stage_walk_host), against the one-pass stage's table (BamSource.select) and against the whole-file decoder
(read_bam_table) -- and every case asserts, from the plan and the file, that the branch it aims at is reached.  tests/test_walk_cases_gpu.py then holds
the device to the model."""
import numpy as np
import pytest

import walkcases as wc
import walkmodel as wm
from unfazed_amd import io_native

CASES = wc.build_panel()


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    folder = tmp_path_factory.mktemp("walkcases")
    return {c.name: c.write(folder) for c in CASES}


def test_the_constants_are_the_sources():
    """a case is built against a constant of the kernels: a change to one breaks the case instead of un-aiming it"""
    have = wm.constants_in_sources()
    assert have == dict(WIN=wm.WIN, WIN_RECS=wm.WIN_RECS, EX_CAP=wm.EX_CAP, FCAP=wm.FCAP, RCAP=wm.RCAP, SUB_EXTENT=wm.SUB_EXTENT, LSEQ_MAX=wm.LSEQ_MAX)
    assert (wm.WIN, wm.WIN_RECS, wm.EX_CAP, wm.FCAP, wm.RCAP, wm.SUB_EXTENT, wm.LSEQ_MAX) == (16384, 512, 768, 1024, 256, 32768, 65535)
    assert (io_native.lib_path() and wm.INCOMPLETE, wm.BAD) == (1, 2)


def test_the_record_maker_and_the_writer(tmp_path):
    assert len(wc.tiny(5)) == 37 and len(wc.filler(5, 42)) == 42 and len(wc.filler(5, 9000)) == 9000
    recs = [wc.read(100 + k, 30) for k in range(50)]
    info = wc.write_bam(str(tmp_path / "a.bam"), wc.CONTIGS, recs, ends=[-(100 + 1), 400], empty_at=[-(100 + 1)], level=0)
    data, coff, at = wm.inflate_file(str(tmp_path / "a.bam"))
    names, lens, first = wm.header_of(data)
    assert names == ["c0", "c1", "c2"] and first == info["header"] and info["rec_off"][0] == first
    assert data[first:] == b"".join(recs)
    assert at.tolist() == [0, first, first + 100, first + 100, 400, info["total"], info["total"]]  # header | 100 bytes | empty | ... 400 | the rest | EOF
    got = wm.records_of(data, first)
    assert [r["pos"] for r in got] == [100 + k for k in range(50)] and got[3]["end"] == 133 and got[3]["name"] == b"q0000103"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_model_equals_the_hosts_walk(case, written, monkeypatch):
    """every descriptor field of uz_stage_walk_host's answer, the flags the model expects, and the case's shape"""
    ctx = wc.host_context(case, written[case.name], monkeypatch)
    case.shape(ctx)
    m = ctx["model"]
    assert any(m["keep_all"]) and any(d["direct"] for d in m["desc_all"])  # what the device hands over is not empty: its comparison compares something
    assert {i: f for i, f in enumerate(m["flags"]) if f} == case.flags  # exactly the tasks the case names, with the bit it names
    w = written[case.name]
    if case.raises is not None and case.raises_at == "walk":
        with pytest.raises(io_native.IoError, match=case.raises):  # the host's walk says what it says today
            wc.host_twin(case, w)
        return
    twin = wc.host_twin(case, w)
    want = wm.desc_array(m["desc_all"], twin.desc.dtype)  # (what the model walked until it raised a flag: the host reads on where the device hands back)
    if case.raises is not None:  # the host's walk keeps the record's bytes as they are; the extract of the one-pass stage refuses them
        fc, flo, fhi, fex = case.fetch_arrays()
        with pytest.raises(io_native.IoError, match=case.raises):
            io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1).select(fc, flo, fhi, 20, extra=fex)
        assert twin.desc.size > want.size
        twin.desc = twin.desc[: want.size]
    else:
        assert twin.desc.size == want.size and np.array_equal(twin.d_first, np.array(m["first_all"]))
    for f in wm.FIELDS:
        assert np.array_equal(twin.desc[f], want[f]), f


@pytest.mark.parametrize("case", [c for c in CASES if c.twin is None], ids=[c.name for c in CASES if c.twin is None])
def test_the_models_parse_equals_the_whole_file_decoder(case, written):
    wc.check_parse(written[case.name]["path"])


@pytest.mark.parametrize("case", [c for c in CASES if c.raises is None], ids=[c.name for c in CASES if c.raises is None])
def test_filter_and_extract_equal_the_one_pass_stage(case, written, monkeypatch):
    for thr in case.thr:
        wc.check_one_pass(case, written[case.name], thr, monkeypatch)


@pytest.mark.parametrize("slack", sorted(wc.sets_of(CASES), key=str), ids=lambda s: "slack_%s" % s)
def test_the_model_equals_the_hosts_walk_of_the_files_as_a_set(slack, written, monkeypatch):
    """BamSource.open_many: references shifted by the files in front, names salted per file, a refID a file's own header does not know INT32_MAX"""
    cases = wc.sets_of(CASES)[slack]
    monkeypatch.setenv("UZ_STAGE_SLACK", str(slack)) if slack is not None else monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    src, paths, (fc, flo, fhi, fex) = wc.open_set(cases, written)
    twin = src.select_kept(fc, flo, fhi, 20, small_tasks=True)
    assert twin.plan.get("files") is not None or len(paths) == 1
    m = wm.walk_plan(twin.plan, paths)
    assert not any(m["flags"])
    want = wm.desc_array(m["desc"], twin.desc.dtype)
    assert want.size == twin.desc.size and want.size > 0 and np.array_equal(twin.d_first, np.array(m["first"]))
    for f in wm.FIELDS:
        assert np.array_equal(twin.desc[f], want[f]), f
    if slack is None:
        assert (want["mtid"] == wm.INT32_MAX).sum() == 1  # the next_refID 7 of a file with three references
        same = want["h1"][(want["pos"] == 1000) & (want["l_name"] == 8)]  # the read q0001000 stands in several files
        assert same.size > 3 and np.unique(same).size == same.size  # ... under another hash in every one of them: the salts
