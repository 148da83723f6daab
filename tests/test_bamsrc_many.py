"""Many BAMs as ONE source (uz_bamsrc_open_many; include/unfazed_io.h) on the host: what the set gives for its files' fetches must be what the
files give one by one, laid end to end -- the kept records and their mates (moved by the records of the files in front), the name ids (moved by
their names), contig_off / max_span at ref_base, the name bytes.  Through the one-pass stage (uz_bam_stage_plan: names compared byte for byte) and
through the descriptor route with the host's twin of the device's walk and the host's joins (select_kept(walk=None): names are hash triples).
The cases: tests/manycases.py."""
import numpy as np
import pytest

import manycases
from unfazed_amd import io_native

Q = 20


def _set_env(monkeypatch, case, host_only=True):
    for k, v in case.env.items():
        if not (host_only and k == "UZ_TEST_FLAG_EVERY"):  # (the device route's hook; here every third task is handed back by `_flagging_walk`)
            monkeypatch.setenv(k, v)


def _one_pass(src, f):
    ref = src.select(f[0], f[1], f[2], Q, extra=f[3])
    n = int(ref.view.n_segs)
    voff, qn, mt, bs = io_native.stage_kept_debug(src.lib, ref._stage.ptr, n)
    names = ref.qnames.take(np.arange(len(ref.qnames), dtype=np.uint32))
    return dict(n=n, voff=voff, qname=qn, mate=mt, bases=bs, names=names, contig_off=ref.arrays["contig_off"].copy(), max_span=ref.arrays["max_span"].copy(),
                lookups=ref.io_stats["index_mate_lookups"])


def _flagging_walk(src, f):
    """a `walk` that hands every third task back to the host (tests/test_stage_desc.py): the stage's own tasks, walked by the host's twin"""
    plain = src.select_kept(f[0], f[1], f[2], Q, extra=f[3], small_tasks=False)

    def walk(plan):
        nt = plan["task"].shape[0]
        flags = np.zeros(max(1, nt), np.int32)
        flags[:nt:3] = 1
        keep = np.ones(plain.desc.size, bool)
        for t in range(0, nt, 3):
            keep[plain.d_first[t]: plain.d_first[t + 1]] = False
        cnt = np.diff(plain.d_first).copy()
        cnt[::3] = 0
        return plain.desc[keep].copy(), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), flags[:nt], np.zeros(nt, np.int64), None
    return walk


def _desc_route(src, f, flagged=False):
    if flagged:
        return src.select_kept(f[0], f[1], f[2], Q, extra=f[3], walk=_flagging_walk(src, f), small_tasks=False, merge=True)
    return src.select_kept(f[0], f[1], f[2], Q, extra=f[3], small_tasks=True)


def _check_tables(many, singles):
    assert many.n_files == len(singles)
    assert many.contigs == [c for s in singles for c in s.contigs]
    assert many.contig_len == [c for s in singles for c in s.contig_len]
    assert np.array_equal(many.ref_base, manycases.ends([len(s.contigs) for s in singles]))
    sizes = [-(-__import__("os").path.getsize(s.path) // 65536) * 65536 for s in singles]
    assert np.array_equal(many.file_base, manycases.ends(sizes))
    assert many.salt1[0] == 0 and many.salt2[0] == 0 and len(set(many.salt1.tolist())) == many.n_files and len(set(many.salt2.tolist())) == many.n_files
    for r in range(len(many.contigs)):
        assert many.ref_file(r) == int(np.searchsorted(many.ref_base, r, side="right")) - 1
    assert many.ref_file(len(many.contigs)) == -1 and many.ref_file(-1) == -1
    assert many.tlen_head.size == 0


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache, root = {}, tmp_path_factory.mktemp("many")

    def get(name):
        if name not in cache:
            cache[name] = manycases.build(name, root)
        return cache[name]
    return get


@pytest.mark.parametrize("name", manycases.CASES)
def test_one_pass_stage_of_a_set_is_its_files_laid_end_to_end(built, name, monkeypatch):
    case = built(name)
    _set_env(monkeypatch, case)
    singles = [io_native.BamSource(p, threads=2) for p in case.paths]
    many = io_native.BamSource.open_many(case.paths, threads=2)
    _check_tables(many, singles)
    per = [_one_pass(s, f) for s, f in zip(singles, case.fetches)]
    got = _one_pass(many, manycases.joined_fetches(many, case))
    for k, p in enumerate(per):
        assert p["n"] >= case.min_kept[k] and (case.min_kept[k] > 0 or p["n"] == 0), (k, p["n"])
    rec_first, name_first = manycases.ends([p["n"] for p in per]), manycases.ends([len(p["names"]) for p in per])
    assert got["n"] == rec_first[-1] and len(got["names"]) == name_first[-1]
    assert np.array_equal(got["voff"], np.concatenate([p["voff"] + (np.uint64(many.file_base[k]) << np.uint64(16)) for k, p in enumerate(per)]))
    assert np.array_equal(got["mate"], np.concatenate([manycases.shifted(p["mate"], rec_first[k]) for k, p in enumerate(per)]))
    assert np.array_equal(got["qname"], np.concatenate([p["qname"].astype(np.int64) + name_first[k] for k, p in enumerate(per)]))
    assert np.array_equal(got["bases"], np.concatenate([p["bases"] for p in per]))
    assert got["names"] == [x for p in per for x in p["names"]]
    assert np.array_equal(got["contig_off"][: len(many.contigs) + 1], np.concatenate([[0]] + [rec_first[k] + p["contig_off"][1: len(s.contigs) + 1] for k, (p, s) in enumerate(zip(per, singles))]))
    assert np.array_equal(got["max_span"][: len(many.contigs)], np.concatenate([p["max_span"][: len(s.contigs)] for p, s in zip(per, singles)]))
    if name == "index_and_host":
        assert all(p["lookups"] > 0 for p in per) and got["lookups"] == sum(p["lookups"] for p in per)
    if name in ("copies", "same_path"):  # the same names in two files: two sets of ids, mates inside each file's own records
        assert per[0]["names"] == per[2]["names"] and per[0]["n"] == per[2]["n"] > 0
        m2 = got["mate"][rec_first[2]: rec_first[3]]
        assert (m2[m2 >= 0] >= rec_first[2]).all() and (got["qname"][rec_first[2]:] >= name_first[2]).all()
        m0 = got["mate"][: rec_first[1]]
        assert (m0 < rec_first[1]).all() and (m0 >= 0).any()
    if name == "empty_middle":
        assert rec_first[1] == rec_first[2] and name_first[1] == name_first[2]


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("name", manycases.CASES)
def test_descriptor_route_of_a_set_is_its_files_laid_end_to_end(built, name, flagged, monkeypatch):
    """the host's twin of the device's walk (the walk plan's sub-tasks) and the host's joins; flagged: every third task of the stage is handed back
    and walked by the host's own walk, its records travel as aux bytes"""
    case = built(name)
    _set_env(monkeypatch, case)
    singles = [io_native.BamSource(p, threads=2) for p in case.paths]
    many = io_native.BamSource.open_many(case.paths, threads=2)
    per = [_desc_route(s, f, flagged) for s, f in zip(singles, case.fetches)]
    got = _desc_route(many, manycases.joined_fetches(many, case), flagged)
    assert "files" in got.plan and "files" not in per[0].plan
    rec_first, name_first = manycases.ends([p.n for p in per]), manycases.ends([p.n_qnames for p in per])
    for k, p in enumerate(per):
        assert p.n >= case.min_kept[k], (k, p.n)
    assert got.n == rec_first[-1] and got.n_qnames == name_first[-1]
    assert np.array_equal(got.kept["mate"], np.concatenate([manycases.shifted(p.kept["mate"], rec_first[k]) for k, p in enumerate(per)]))
    assert np.array_equal(got.kept["qname"], np.concatenate([p.kept["qname"].astype(np.int64) + name_first[k] for k, p in enumerate(per)]))
    for col, tot in (("cig_off", "n_cigar_total"), ("unit_off", "n_row_units"), ("name_off", "n_name_bytes")):
        base = manycases.ends([getattr(p, tot) for p in per])
        assert np.array_equal(got.kept[col], np.concatenate([p.kept[col].astype(np.int64) + base[k] for k, p in enumerate(per)])), col
        assert getattr(got, tot) == base[-1]
    base = manycases.ends([p.n_seq_units for p in per])
    assert np.array_equal(got.kept["seq_off"], np.concatenate([manycases.shifted(p.kept["seq_off"], base[k], none=io_native.KEPT_NO_SEQ) for k, p in enumerate(per)]))
    # where a record lies: in the gathered blocks (file after file) or, for a record the host walked itself, in the aux bytes
    in_aux = (got.kept["src"] & np.uint64(io_native.WALK_SRC_AUX)) != 0
    want_aux = np.concatenate([(p.kept["src"] & np.uint64(io_native.WALK_SRC_AUX)) != 0 for p in per])
    if flagged:  # (every third task of the set is not every third task of each file: the same list, other records in the aux bytes)
        assert in_aux.any() and want_aux.any()
    else:
        assert np.array_equal(in_aux, want_aux)
        hbm = manycases.ends([p.plan["out_bytes"] for p in per])
        want_src = np.concatenate([p.kept["src"] + np.uint64(hbm[k]) for k, p in enumerate(per)])
        assert np.array_equal(got.kept["src"][~in_aux], want_src[~in_aux])
    assert np.array_equal(got.contig_off, np.concatenate([[0]] + [rec_first[k] + p.contig_off[1:] for k, p in enumerate(per)]))
    assert np.array_equal(got.max_span[: got.n_contigs], np.concatenate([p.max_span[: p.n_contigs] for p in per]))
    if flagged:
        return
    # the descriptors: a file's, with its references, offsets and salts
    d = got.desc
    want = np.concatenate([p.desc for p in per])
    assert d.size == want.size
    fo = np.concatenate([np.full(p.desc.size, k) for k, p in enumerate(per)]).astype(np.int64)
    assert np.array_equal(d["voff"], want["voff"] + (many.file_base[fo].astype(np.uint64) << np.uint64(16)))
    assert np.array_equal(d["h1"], want["h1"] ^ many.salt1[fo]) and np.array_equal(d["h2"], want["h2"] ^ many.salt2[fo])
    assert np.array_equal(d["mtid"], np.where(want["mtid"] >= 0, want["mtid"] + many.ref_base[fo], want["mtid"]))
    for col in ("pos", "end", "tlen", "mpos", "flag", "l_seq", "n_cigar", "mapq", "l_name", "direct"):
        assert np.array_equal(d[col], want[col]), col


def test_one_path_is_the_plain_source(built):
    case = built("copies")
    f = case.fetches[0]
    a = io_native.BamSource(case.paths[0], threads=2, insert_size_max_sample=500)
    b = io_native.BamSource.open_many(case.paths[:1], threads=2, insert_size_max_sample=500)
    assert b.n_files == 1 and a.n_files == 1 and b.contigs == a.contigs and b.contig_len == a.contig_len
    assert np.array_equal(a.tlen_head, b.tlen_head) and a.tlen_head.size > 0
    assert np.array_equal(a.file_base, b.file_base) and np.array_equal(a.ref_base, b.ref_base) and b.salt1[0] == 0 and b.salt2[0] == 0
    ra, rb = a.select(f[0], f[1], f[2], Q, extra=f[3]), b.select(f[0], f[1], f[2], Q, extra=f[3])
    assert sorted(ra.arrays) == sorted(rb.arrays) and int(ra.view.n_segs) > 0
    for k in ra.arrays:
        assert ra.arrays[k].tobytes() == rb.arrays[k].tobytes(), k
    ka, kb = a.select_kept(f[0], f[1], f[2], Q, extra=f[3]), b.select_kept(f[0], f[1], f[2], Q, extra=f[3])
    assert "files" not in kb.plan
    assert ka.kept.tobytes() == kb.kept.tobytes() and ka.desc.tobytes() == kb.desc.tobytes()
    for k in ("comp", "in_off", "out_off", "task", "span", "reach", "fetch", "blk_coff", "blk_crc"):
        assert ka.plan[k][: ka.plan["comp_bytes"] if k == "comp" else None].tobytes() == kb.plan[k][: kb.plan["comp_bytes"] if k == "comp" else None].tobytes(), k


def test_a_set_is_refused_when_a_file_is(built, tmp_path):
    case = built("copies")
    with pytest.raises(io_native.IoError):
        io_native.BamSource.open_many([case.paths[0], str(tmp_path / "missing.bam")])
    with pytest.raises(io_native.IoError):
        io_native.BamSource.open_many([])
    bad = tmp_path / "bad.bam"
    bad.write_bytes(open(case.paths[1], "rb").read())
    (tmp_path / "bad.bam.bai").write_bytes(open(case.paths[0] + ".bai", "rb").read()[:-40])  # a truncated index
    with pytest.raises(io_native.IoError):
        io_native.BamSource.open_many([case.paths[0], str(bad)])


def test_block_chains_end_with_their_file(built):
    """the gathered blocks of the set are its files' blocks, file after file: no chain takes the next file's header block for its own"""
    case = built("file_end")
    singles = [io_native.BamSource(p, threads=2) for p in case.paths]
    many = io_native.BamSource.open_many(case.paths, threads=2)
    per = [s.select_kept(f[0], f[1], f[2], Q, extra=f[3]) for s, f in zip(singles, case.fetches)]
    got = many.select_kept(*manycases.joined_fetches(many, case)[:3], Q, extra=manycases.joined_fetches(many, case)[3])
    assert np.array_equal(got.plan["blk_coff"], np.concatenate([p.plan["blk_coff"] + many.file_base[k] for k, p in enumerate(per)]))
    assert got.plan["comp"][: got.plan["comp_bytes"]].tobytes() == b"".join(p.plan["comp"][: p.plan["comp_bytes"]].tobytes() for p in per)
    size0 = __import__("os").path.getsize(case.paths[0])
    last = int(per[0].plan["blk_coff"][-1])
    assert last + 28 == size0  # file 0's chain was gathered up to the file's last block (the 28-byte end-of-file marker)
