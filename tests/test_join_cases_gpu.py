"""The batch-wide joins on the device (csrc/k_bamjoin.hip: 18 kernels, two radix sorts, two scans) held to the hand-built panel of
tests/joincases.py, one case per rule's edge: the kept list the kernels build in HBM against the plain oracle (tests/joinoracle.py) and against the
host's joins over the same walk, its offsets, totals, per-reference counts and spans, its names by id; the same batch joined twice; the table built
from the list; files as a set; descriptors written by hand where no file can hold the case (two names that agree in a hash), and the two errors of
uz_bam_join a caller can reach without a fault.  Bit-exact throughout.  tests/test_join_cases.py holds the panel, the oracle and the model together
on the CPU."""
import numpy as np
import pytest

import joincases as jc
import joinmodel
import joinoracle
import walkcases as wc
from unfazed_amd import io_native

pytestmark = pytest.mark.gpu

CASES = jc.build_panel()
SOUND = [c for c in CASES if not c.refused]
TABLES = [cs[0] for cs in jc.groups_of(SOUND).values()]  # one case per group also has its table built on both routes
KEPT_FIELDS = ("qname", "mate", "cig_off", "unit_off", "seq_off", "name_off")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    folder = tmp_path_factory.mktemp("joincases_gpu")
    return {c.name: c.write(folder) for c in CASES}


def joined(engine, src, fetches, all_bases):
    fc, flo, fhi, fex = fetches
    return src.select_kept(fc, flo, fhi, 20, all_bases=all_bases, join=engine, release=engine.bam_walk_release)


def fetched(engine, dev, n_ref):
    got = engine.join_fetch(dev.token, dev.n, n_ref)
    got["bases"] = got["bases"].astype(bool)
    got["n_qnames"] = dev.n_qnames
    return got


def check_against_host_and_oracle(engine, src, fetches, all_bases, want, refs_of_kept, spans_of_kept, table=False):
    """want: the oracle's answer; refs_of_kept / spans_of_kept: reference and end - pos of every kept record, from the oracle's parse"""
    fc, flo, fhi, fex = fetches
    n_ref = len(src.contigs)
    host = src.select_kept(fc, flo, fhi, 20, all_bases=all_bases, walk=engine.bam_walk, release=engine.bam_walk_release)  # the device's walk, the HOST's joins
    dev = joined(engine, src, fetches, all_bases)
    again = None
    rids = []
    try:
        assert dev.joined and dev.n == host.n == want["voff"].size
        got = fetched(engine, dev, n_ref)
        assert jc.same(got, want) == []  # the oracle: voff, qname, mate, bases, the number of names
        for f in KEPT_FIELDS:
            assert np.array_equal(got["kept"][f], host.kept[f]), f
        assert np.array_equal(got["kept"]["seq_off"] != io_native.KEPT_NO_SEQ, want["bases"])
        in_hbm = ((got["kept"]["src"] | host.kept["src"]) & np.uint64(io_native.WALK_SRC_AUX)) == 0
        assert np.array_equal(got["kept"]["src"][in_hbm], host.kept["src"][in_hbm])
        assert (dev.n, dev.n_qnames, dev.n_cigar_total, dev.n_row_units, dev.n_seq_units, dev.n_name_bytes) == \
            (host.n, host.n_qnames, host.n_cigar_total, host.n_row_units, host.n_seq_units, host.n_name_bytes)
        assert dev.n_name_bytes == sum(len(want["names"][q]) for q in want["qname"])
        contig_off = np.concatenate([[0], np.cumsum(np.bincount(refs_of_kept, minlength=n_ref))])
        max_span = np.zeros(n_ref, np.int64)
        np.maximum.at(max_span, refs_of_kept, spans_of_kept)
        assert np.array_equal(got["contig_off"], host.contig_off) and np.array_equal(got["contig_off"], contig_off)
        assert np.array_equal(got["max_span"][:n_ref], host.max_span[:n_ref]) and np.array_equal(got["max_span"][:n_ref], max_span)
        # ---- the same batch once more: byte for byte the same list
        again = joined(engine, src, fetches, all_bases)
        twice = fetched(engine, again, n_ref)
        assert again.n == dev.n and twice["kept"].tobytes() == got["kept"].tobytes() and jc.same(twice, got) == []
        assert np.array_equal(twice["contig_off"], got["contig_off"]) and np.array_equal(twice["max_span"], got["max_span"])
        # ---- names by id, from the table built from the list in HBM: forwards, backwards, with repeats
        rids.append(engine.reads_from_bam(again, names=True))
        ids = np.arange(dev.n_qnames, dtype=np.uint32)
        names = [n.decode() for n in want["names"]]
        assert len(again.qnames) == len(names) and again.qnames.take(ids) == names
        back = np.concatenate([ids[::-1], ids[::-1][:3], ids[:2]])
        assert again.qnames.take(back) == [names[int(i)] for i in back]
        if table:  # ... and the table itself against the host route's (the one-pass stage's link form, uploaded), header by header
            staged = src.select(fc, flo, fhi, 20, extra=fex, all_bases=all_bases)
            assert int(staged.view.n_segs) == dev.n
            rids.append(engine.upload_reads_packed(staged))
            engine.wait_reads(rids[1])
            a, b = engine.reads_headers(rids[1], dev.n), engine.reads_headers(rids[0], dev.n)
            for k in ("start", "end", "tlen", "mate", "qname"):
                assert np.array_equal(a[k], b[k]), k
            assert staged.qnames.take(ids) == names
    finally:
        for d in (dev, again):
            if d is not None and d.token is not None:
                engine.bam_walk_release(d.token)
                d.token = None
        for r in rids:
            engine.free_reads(r)
        del host
    return dev


@pytest.mark.parametrize("case", SOUND, ids=[c.name for c in SOUND])
def test_the_kernels_equal_the_oracle_and_the_hosts_joins(engine, case, written, monkeypatch):
    w = written[case.name]
    wc._slack(case, monkeypatch)
    src = io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)
    recs, n_ref = joinoracle.records(w["path"])
    want = joinoracle.join(recs, case.fetches, 0, n_ref, case.all_bases)
    kept = [recs[k] for k in want["rec"]]
    dev = check_against_host_and_oracle(engine, src, case.fetch_arrays(), case.all_bases, want, np.array([r["ref"] for r in kept], np.int64),
                                        np.array([r["end"] - r["pos"] for r in kept], np.int64), table=case in TABLES)
    # (the case's shape is asserted on the CPU, from the same plan: tests/test_join_cases.py; here: the route it implies was taken)
    assert (dev.join_calls > 1) == (dev.io_stats["index_mate_lookups"] > 0)


def test_a_closure_that_needs_a_65th_trip_is_refused_and_its_slot_given_back(engine, written, monkeypatch):
    """include/uz_bamwalk.h UZ_JOIN_MAX_TRIPS: the device route refuses the batch as every host route does (tests/test_join_cases.py), the walked batch's
    slot is free again, and the chain that needs exactly the cap goes through"""
    monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    by = {c.name: c for c in CASES}
    over, at = by["chain_of_%d_trips" % (joinmodel.MAX_TRIPS + 1)], by["chain_of_%d_trips" % joinmodel.MAX_TRIPS]
    assert over.refused and not at.refused
    src = io_native.BamSource(written[over.name]["path"], threads=2, insert_size_max_sample=-1)
    with pytest.raises(io_native.IoError, match=joinmodel.REFUSED):
        joined(engine, src, over.fetch_arrays(), False)
    src = io_native.BamSource(written[at.name]["path"], threads=2, insert_size_max_sample=-1)
    dev = joined(engine, src, at.fetch_arrays(), False)
    try:
        assert dev.token == 0 and dev.join_calls == joinmodel.MAX_TRIPS + 1 and dev.n == joinmodel.MAX_TRIPS + 1  # the slot the refused batch held
    finally:
        engine.bam_walk_release(dev.token)
        dev.token = None


def test_files_as_a_set(engine, tmp_path_factory, written, monkeypatch):
    """two files with byte-identical records and names, of six cases, as one source: mates inside their file, name ids per file -- and uz_reads_files
    accepts the id ranges"""
    monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    cases = [c for c in CASES if c.name in jc.SET_CASES]
    folder = tmp_path_factory.mktemp("joincases_gpu_twice")
    second = {c.name: c.write(folder) for c in cases}
    src, paths, fetches = jc.open_twice(cases, written, second)
    want = joinoracle.run_set(paths, src.file_base, src.ref_base, list(zip(*(a.tolist() for a in fetches))))
    refs, spans = [], []
    for f, p in enumerate(paths):
        recs, n_ref = joinoracle.records(p, int(src.file_base[f]), int(src.ref_base[f]))
        x = joinoracle.join(recs, list(zip(*(a.tolist() for a in fetches))), int(src.ref_base[f]), int(src.ref_base[f]) + n_ref)
        refs += [recs[k]["ref"] for k in x["rec"]]
        spans += [recs[k]["end"] - recs[k]["pos"] for k in x["rec"]]
    check_against_host_and_oracle(engine, src, fetches, False, want, np.array(refs, np.int64), np.array(spans, np.int64), table=True)
    dev = joined(engine, src, fetches, False)
    rid = engine.reads_from_bam(dev, names=True)
    try:
        rec_first, name_first = engine.reads_files(rid, src.ref_base)
        assert np.array_equal(rec_first, want["first_rec"]) and np.array_equal(name_first, want["first_name"])
    finally:
        engine.free_reads(rid)


# ---------------------------------------------------------------------------------------------------------------- descriptors written by hand
@pytest.fixture(scope="module")
def desc_level(tmp_path_factory):
    folder = tmp_path_factory.mktemp("joincases_gpu_rows")
    empty = wc.Case("empty_walk", [wc.read(1990, 30)] + wc.tail(), [], None).write(folder)
    return jc.desc_level_cases(folder), empty


def join_rows_on_the_device(engine, empty, rows, n_ref, answer=lambda need: np.zeros(need.size, np.int32)):
    """a walk with no task of its own, then uz_bam_join over rows of the host alone (one look-up task, on reference 0): every asker raises a need, the
    test answers it -> the kept list"""
    src = io_native.BamSource(empty["path"], threads=2, insert_size_max_sample=-1)
    z, zx = np.zeros(0, np.int32), np.zeros(0, np.uint16)
    sh, plan = jc.begin(src, (z, z, z, zx))
    assert plan["task"].shape[0] == 0
    token, n_desc = engine.walk(plan)
    try:
        assert n_desc == 0
        h_flags, look_tid = np.zeros(1, np.int32), np.zeros(1, np.int32)
        n_need, tot = engine.join(token, 0, h_flags, n_ref, False, rows, None, look_tid, None)
        calls = 1
        while n_need:
            assert calls <= 4
            need = engine.join_needs(token, n_need)
            assert (need["who"] < rows.size).all() and np.array_equal(need["h1"], rows["h1"][need["who"]]) and np.array_equal(need["mpos"], rows["mpos"][need["who"]])
            n_need, tot = engine.join(token, 0, h_flags, n_ref, False, None, None, look_tid, answer(need))
            calls += 1
        got = engine.join_fetch(token, int(tot[0]), n_ref)
        got["bases"] = got["bases"].astype(bool)
        got["n_qnames"] = int(tot[1])
        return got, calls
    finally:
        engine.bam_walk_release(token)


@pytest.mark.parametrize("k", range(3), ids=["equal_h1_different_h2", "equal_h1_and_h2_different_length", "all_three_equal"])
def test_names_that_agree_in_a_hash(engine, desc_level, k):
    """the mate search (k_join_round) and the name ids (k_final_names) compare h1, h2 AND the length: the same rows the model's pure function answers on
    the CPU (tests/test_join_cases.py), against the oracle's answer for the names as they are"""
    (name, rows, n_ref, want), empty = desc_level[0][k], desc_level[1]
    got, calls = join_rows_on_the_device(engine, empty, rows, n_ref)
    assert jc.same(got, want) == [] and calls == 3  # the fetched records ask, then their mates, then nobody
    assert jc.same(got, jc.join_rows(rows, n_ref)) == []


def test_join_tasks_that_do_not_exist_are_refused(engine, desc_level):
    from unfazed_amd.engine import UnfazedHipError
    (name, rows, n_ref, want), empty = desc_level[0][0], desc_level[1]
    bad = rows.copy()
    bad["task"][1] = io_native.WALK_TASK_JOIN | 1  # one look-up task: join task 1 is one too many
    with pytest.raises(UnfazedHipError, match="a descriptor of the host names a join task that does not exist"):
        join_rows_on_the_device(engine, empty, bad, n_ref)
    for wrong in (-1, 1):
        with pytest.raises(UnfazedHipError, match="an answer names a join task that does not exist"):
            join_rows_on_the_device(engine, empty, rows, n_ref, answer=lambda need: np.full(need.size, wrong, np.int32))
    got, calls = join_rows_on_the_device(engine, empty, rows, n_ref)  # the slots were given back, and the context goes on
    assert jc.same(got, want) == []
