"""The device's record walk, mate-candidate filter and extract (k_bam_walk, k_bam_walk_many, k_tab_insert, k_walk_scan, k_desc_filter, k_bam_extract:
csrc/bamwalk_body.hpp, csrc/k_bamwalk.hip) held to the plain model of tests/walkmodel.py on the hand-built panel of tests/walkcases.py: every
descriptor field, every flag, and the table built from the bytes in HBM record by record and base by base (uz_reads_headers, uz_reads_columns).
Bit-exact throughout.  tests/test_walk_cases.py holds the model itself against the host's walk on the same files, without a device."""
import numpy as np
import pytest

import walkcases as wc
import walkmodel as wm
from unfazed_amd import io_native

pytestmark = pytest.mark.gpu

CASES = wc.build_panel()
LINK_MAX_BASES = 255 * 32  # the host's link form counts a record's staged units in one byte (io_stage.cpp WRec::n_units): the host route cannot stage a longer read


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    folder = tmp_path_factory.mktemp("walkcases_gpu")
    return {c.name: c.write(folder) for c in CASES}


def recording(engine, box):
    """engine.bam_walk, with what the device said of every walk task kept aside (a flagged batch's answer never reaches the caller of select_kept)"""
    def walk(plan):
        out = engine.bam_walk(plan)
        box.update(plan=plan, sub_flags=np.array(out[2]).copy(), token=out[4])
        return out
    return walk


def source(case, w, monkeypatch):
    wc._slack(case, monkeypatch)
    return io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_descriptors_and_flags_equal_the_model(engine, case, written, monkeypatch):
    w = written[case.name]
    src = source(case, w, monkeypatch)
    fc, flo, fhi, fex = case.fetch_arrays()
    box = {}
    if case.raises is not None and case.raises_at == "walk":  # the device flags the task, the host walks it and says what it says of the record
        try:
            with pytest.raises(io_native.IoError, match=case.raises):
                src.select_kept(fc, flo, fhi, 20, walk=recording(engine, box), merge=True)
            ctx = wc.context(case, w, box["plan"])
            case.shape(ctx)
            assert box["sub_flags"].tolist() == ctx["model"]["sub_flags"] and {i: f for i, f in enumerate(ctx["model"]["flags"]) if f} == case.flags
        finally:
            if "token" in box:
                engine.bam_walk_release(box["token"])
        return
    dev = src.select_kept(fc, flo, fhi, 20, walk=recording(engine, box), merge=True)
    try:
        ctx = wc.context(case, w, dev.plan)
        case.shape(ctx)  # the branch the case aims at is reached by THIS plan
        m = ctx["model"]
        assert box["sub_flags"].tolist() == m["sub_flags"]
        assert {i: int(f) for i, f in enumerate(dev.d_flags) if f} == case.flags == {i: f for i, f in enumerate(m["flags"]) if f}
        want = wc.filtered(m, dev.desc.dtype)
        assert dev.desc.size == want.size and (want.size > 0 or bool(case.flags))
        for f in wm.FIELDS:
            assert np.array_equal(dev.desc[f], want[f]), f
        twin = wc.host_twin(case, w)  # the list of kept records is the same whoever walked
        for f in ("qname", "mate", "cig_off", "unit_off", "seq_off", "name_off"):
            assert np.array_equal(dev.kept[f], twin.kept[f]), f
        here = (dev.kept["src"] & np.uint64(io_native.WALK_SRC_AUX)) == 0
        assert np.array_equal(dev.kept["src"][here], twin.kept["src"][here]) and (here.all() or bool(case.flags))
    finally:
        engine.bam_walk_release(dev.token)
        dev.token = None


def check_table(engine, src, paths, fetches, thr, host_route):
    """the table uz_reads_from_bam builds for the fetches == the model's extract of every kept record; names by id; the host route's headers"""
    fc, flo, fhi, fex = fetches
    twin = src.select_kept(fc, flo, fhi, thr, small_tasks=True)  # (where every kept record lies in the plan's bytes: the host's walk raises no flag)
    dev = src.select_kept(fc, flo, fhi, thr, walk=engine.bam_walk, release=engine.bam_walk_release)
    pb = wm.PlanBytes(dev.plan, paths)
    rid = engine.reads_from_bam(dev, names=True)
    rid_h = None
    try:
        n = dev.n
        assert n == twin.n and n > 0
        for f in ("qname", "mate", "cig_off", "unit_off", "seq_off"):
            assert np.array_equal(dev.kept[f], twin.kept[f]), f
        head, cols = engine.reads_headers(rid, n), engine.reads_columns(rid, n)
        assert cols["cigar"].size == dev.n_cigar_total and cols["seq4"].size == 16 * dev.n_seq_units and cols["qlow"].size == dev.n_row_units
        names = dev.qnames.take(np.arange(dev.n_qnames, dtype=np.uint32))
        for i in range(n):
            bases = int(twin.kept["seq_off"][i]) != io_native.KEPT_NO_SEQ
            x = wm.extract(pb.buf, int(twin.kept["src"][i]), thr, bases)
            assert (int(head["start"][i]), int(head["tlen"][i]), int(head["mate"][i]), int(head["qname"][i])) == \
                (x["start"], x["tlen"], int(twin.kept["mate"][i]), int(twin.kept["qname"][i])), i
            assert int(cols["fm"][i]) == x["flag"] | (x["mapq"] << 16) | (x["aux"] << 24), (i, hex(int(cols["fm"][i])))
            assert (int(cols["l_seq"][i]), int(cols["n_cigar"][i]), int(cols["cigar_off"][i])) == (x["l_seq"], x["n_cigar"], int(twin.kept["cig_off"][i])), i
            assert np.array_equal(cols["cigar"][int(cols["cigar_off"][i]): int(cols["cigar_off"][i]) + x["n_cigar"]], x["cigar"]), i
            bits, words = wm.low_bits_of(cols, i)
            assert int(cols["qoff"][i]) == int(twin.kept["unit_off"][i]) and np.array_equal(words, x["plane"]) and np.array_equal(bits, x["low"]), i
            if bases:
                assert int(cols["sq_off"][i]) == int(twin.kept["seq_off"][i]), i
                assert wm.row_of(cols, i) == x["row"], i  # every unit: the pad nibble and the rest of the last unit zero
                assert np.array_equal(wm.codes_of(cols, i), x["codes"]), i
            assert names[int(twin.kept["qname"][i])].encode() == x["name"], i
        if host_route:  # ... and the host route's table for the same fetches (uz_reads_upload_packed of the one-pass stage)
            staged = src.select(fc, flo, fhi, thr, extra=fex)
            assert int(staged.view.n_segs) == n
            rid_h = engine.upload_reads_packed(staged)
            engine.wait_reads(rid_h)
            other = engine.reads_headers(rid_h, n)
            for k in ("start", "end", "tlen", "mate", "qname"):
                assert np.array_equal(head[k], other[k]), k
            ids = np.arange(len(staged.qnames), dtype=np.uint32)
            assert names == staged.qnames.take(ids)
    finally:
        engine.free_reads(rid)
        if rid_h is not None:
            engine.free_reads(rid_h)
    return dev


TABLES = [c for c in CASES if c.raises is None]


@pytest.mark.parametrize("case", TABLES, ids=[c.name for c in TABLES])
def test_the_table_from_hbm_equals_the_model(engine, case, written, monkeypatch):
    w = written[case.name]
    src = source(case, w, monkeypatch)
    longest = wc.longest_read([w["path"]])
    for thr in case.thr:
        dev = check_table(engine, src, [w["path"]], case.fetch_arrays(), thr, host_route=longest <= LINK_MAX_BASES)
        assert int(np.count_nonzero(dev.d_flags)) == len(case.flags)  # (a flagged task's records come from the host's walk, as aux bytes: the same table)
        assert dev.n_aux > 0 or not case.flags


def test_a_kept_record_that_overruns_its_block_is_refused(engine, written, monkeypatch):
    """bases and qualities that overrun the record: the device flags the task, the host's walk keeps the record's bytes as they are, and the extract
    refuses them (the one-pass stage's extract raises: tests/test_walk_cases.py)"""
    from unfazed_amd.engine import UnfazedHipError
    case = [c for c in CASES if c.raises_at == "extract"][0]
    w = written[case.name]
    src = source(case, w, monkeypatch)
    fc, flo, fhi, fex = case.fetch_arrays()
    box = {}
    dev = src.select_kept(fc, flo, fhi, 20, walk=recording(engine, box), release=engine.bam_walk_release)
    ctx = wc.context(case, w, dev.plan)
    case.shape(ctx)
    assert box["sub_flags"].tolist() == ctx["model"]["sub_flags"] == [wm.BAD]
    with pytest.raises(UnfazedHipError, match="kept record"):
        engine.reads_from_bam(dev)
    del dev  # (gives the walked batch up)


@pytest.mark.parametrize("slack", sorted(wc.sets_of(CASES), key=str), ids=lambda s: "slack_%s" % s)
def test_the_files_as_a_set(engine, slack, written, monkeypatch):
    """k_bam_walk_many: the same files through BamSource.open_many against the model's shifted and salted form -- the record whose refID its own header
    does not know among them"""
    cases = wc.sets_of(CASES)[slack]
    monkeypatch.setenv("UZ_STAGE_SLACK", str(slack)) if slack is not None else monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    src, paths, fetches = wc.open_set(cases, written)
    fc, flo, fhi, fex = fetches
    dev = src.select_kept(fc, flo, fhi, 20, walk=engine.bam_walk, merge=True)
    try:
        assert dev.plan.get("files") is not None or len(paths) == 1
        m = wm.walk_plan(dev.plan, paths)
        assert not any(m["flags"]) and not dev.d_flags.any()
        want = wc.filtered(m, dev.desc.dtype)
        assert dev.desc.size == want.size and want.size > 0
        for f in wm.FIELDS:
            assert np.array_equal(dev.desc[f], want[f]), f
        if slack is None:
            assert (want["mtid"] == wm.INT32_MAX).sum() == 1
    finally:
        engine.bam_walk_release(dev.token)
        dev.token = None
    longest = wc.longest_read(paths)
    check_table(engine, src, paths, fetches, 20, host_route=longest <= LINK_MAX_BASES)
