"""Many BAMs walked and joined on the device as ONE batch (io_native.BamSource.open_many -> uz_bam_walk_many -> uz_bam_join -> uz_reads_from_walk):
  * the table of a set of files == the tables of its files laid end to end -- start / end / tlen exactly, mates moved by the records of the files in
    front, name ids by their names, the read names byte for byte -- and uz_reads_files names those starts (cases: tests/manycases.py);
  * uz_reads_files refuses a table whose files' name ids interleave;
  * uz_phase_cohort_joined on the joined table == uz_phase_cohort on the per-file tables over the same groups, vote lists included once each
    group's first name id is added, == the CPU oracle kid by kid."""
import numpy as np
import pytest

import manycases
from unfazed_amd import abi, io_native

pytestmark = pytest.mark.gpu

Q = 20


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cache, root = {}, tmp_path_factory.mktemp("many")

    def get(name):
        if name not in cache:
            cache[name] = manycases.build(name, root)
        return cache[name]
    return get


def _table(engine, src, f):
    """the device route of stage_reads and the table built from it -> (reads id, headers, names by id, the batch)"""
    kb = engine.stage_reads(src, f[0], f[1], f[2], f[3], Q, slot="test")
    assert isinstance(kb, io_native.KeptBatch) and kb.joined
    rid = engine.reads_from_bam(kb, names=True)
    names = kb.qnames.take(np.arange(len(kb.qnames), dtype=np.uint32))
    return rid, engine.reads_headers(rid, kb.n), names, kb


@pytest.mark.parametrize("name", manycases.CASES)
def test_table_of_a_set_is_its_files_tables_laid_end_to_end(engine, built, name, monkeypatch):
    case = built(name)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    singles = [io_native.BamSource(p, threads=2) for p in case.paths]
    many = io_native.BamSource.open_many(case.paths, threads=2)
    rids = []
    try:
        per = []
        for s, f in zip(singles, case.fetches):
            per.append(_table(engine, s, f))
            rids.append(per[-1][0])
        rid, got, names, kb = _table(engine, many, manycases.joined_fetches(many, case))
        rids.append(rid)
        for k, p in enumerate(per):
            assert p[3].n >= case.min_kept[k] and (case.min_kept[k] > 0 or p[3].n == 0), (k, p[3].n)
        rec_first, name_first = manycases.ends([p[3].n for p in per]), manycases.ends([len(p[2]) for p in per])
        assert kb.n == rec_first[-1] and len(names) == name_first[-1]
        for col in ("start", "end", "tlen"):
            assert np.array_equal(got[col], np.concatenate([p[1][col] for p in per])), col
        assert np.array_equal(got["mate"], np.concatenate([manycases.shifted(p[1]["mate"], rec_first[k]) for k, p in enumerate(per)]))
        assert np.array_equal(got["qname"], np.concatenate([p[1]["qname"].astype(np.int64) + name_first[k] for k, p in enumerate(per)]))
        assert names == [x for p in per for x in p[2]]
        rf, nf = engine.reads_files(rid, many.ref_base)
        assert np.array_equal(rf, rec_first) and np.array_equal(nf, name_first)
        if name == "index_and_host":
            assert kb.io_stats["index_mate_lookups"] > 0 and kb.host_tasks > 0 and all(p[3].io_stats["index_mate_lookups"] > 0 for p in per)
        if name in ("copies", "same_path"):
            assert per[0][2] == per[2][2] and per[0][3].n == per[2][3].n > 0
            m2 = got["mate"][rec_first[2]:]
            assert (m2[m2 >= 0] >= rec_first[2]).all() and (m2 >= 0).any()
    finally:
        for r in rids:
            engine.free_reads(r)


def test_interleaved_name_ranges_are_refused(engine):
    """a hand-built table of two 'files' (one contig each): as staged, each file's names are one range; with the ids reversed file 0 does not start
    at 0; with every second id swapped between the files the ranges interleave"""
    from helpers import tables
    from synth.small import SmallConfig, make_small
    from unfazed_amd.engine import UnfazedHipError
    ds = make_small(SmallConfig(seed=5, n_dnms=4, coverage_per_hap=4.0, odd_read_prob=0.0))
    _, reads = tables(ds)
    rt = list(reads.values())[0]
    assert len(rt.contigs) == 2 and rt.contig_off[1] > 0 and rt.contig_off[2] > rt.contig_off[1]
    base = np.array([0, 1, 2], np.int32)
    nq = len(rt.qnames)
    # the names numbered by first appearance, as the BAM stage numbers them; no name of this table has records on both contigs
    _, first_at, inv = np.unique(rt.qname, return_index=True, return_inverse=True)
    own = np.argsort(np.argsort(first_at))[inv].astype(rt.qname.dtype)
    assert not set(own[: rt.contig_off[1]].tolist()) & set(own[rt.contig_off[1]:].tolist()) and int(own.max()) == nq - 1

    def files_of(qname):
        rt.qname = np.ascontiguousarray(qname, own.dtype)
        rid = engine.upload_reads(rt)
        try:
            return engine.reads_files(rid, base)
        finally:
            engine.free_reads(rid)

    rf, nf = files_of(own)
    n0 = int(own[: rt.contig_off[1]].max()) + 1
    assert rf.tolist() == [0, int(rt.contig_off[1]), rt.n_segs] and nf.tolist() == [0, n0, nq]
    with pytest.raises(UnfazedHipError, match="uz_reads_files.*name ids of file 0"):
        files_of(nq - 1 - own)
    swap = own.copy()
    a, b = int(own[0]), int(own[-1])  # one name of each file changes places: both ranges now reach into each other
    assert a < n0 <= b
    swap[own == a], swap[own == b] = b, a
    with pytest.raises(UnfazedHipError, match="uz_reads_files"):
        files_of(swap)
    rt.qname = own
    rid = engine.upload_reads(rt)
    try:
        with pytest.raises(UnfazedHipError, match="ref_base"):
            engine.reads_files(rid, np.array([0, 1, 3], np.int32))
    finally:
        engine.free_reads(rid)


@pytest.fixture(scope="module")
def four(engine, tmp_path_factory):
    """four kids from files: each kid's table staged from its own BAM, the joined table staged from the four files as one, the groups over
    both, and the batch's results by uz_phase_cohort on the per-file tables and by the CPU oracle; made once"""
    from types import SimpleNamespace
    from filesio import dump_dataset, write_bai
    from helpers import tables
    from oracle_backend import OracleBackend
    from synth.small import SmallConfig, make_small
    from unfazed_amd.hostpath import concordant_cutoff
    from unfazed_amd.staging import fetch_points
    kids = ["kidA", "kidB", "kidC", "kidD"]
    ds = make_small(SmallConfig(seed=911, n_dnms=20, kids=kids, cluster_prob=0.6, odd_read_prob=0.05))
    paths = dump_dataset(ds, str(tmp_path_factory.mktemp("four")))
    for b in paths["bams"].values():
        write_bai(b)
    sites, reads = tables(ds)
    P = abi.make_params()
    engine.set_params(P)
    orc = OracleBackend()
    sid, osid = engine.upload_sites(sites), orc.upload_sites(sites)
    many = io_native.BamSource.open_many([paths["bams"][k] for k in kids], threads=2)
    groups, ogroups, cols, first, found_all = [], [], dict(contig=[], rcontig=[], start=[], end=[], vartype=[], refs=[], alts=[]), 0, []
    per_f, per_rid, per_names, per_cols = [], [], [], []
    for g, kid in enumerate(kids):
        ped = ds.pedigrees[kid]
        fam_cols = sites.family_columns(kid, ped["dad"], ped["mom"])
        rt = reads["mem://%s.bam" % kid]
        src = io_native.BamSource(paths["bams"][kid], threads=2)
        assert src.contigs == rt.contigs
        dn = [d for d in ds.dnms if d["kid"] == kid]
        refs, alts = [], []
        for d in dn:
            j = int(sites.query(d["chrom"], d["start"], d["start"] + 1)[-1])
            refs.append(sites.ref_str[j].encode()); alts.append(sites.alt_strs[j][0].encode())
        c = dict(contig=[sites.contig_index[d["chrom"]] for d in dn], rcontig=[rt.contig_index[d["chrom"]] for d in dn], start=[d["start"] for d in dn],
                 end=[d["end"] for d in dn], vartype=[0] * len(dn), refs=refs, alts=alts)
        cutoff = concordant_cutoff(rt.tlen, P.readlen, 3) + float(g)
        ofam = orc.add_family(osid, *fam_cols)
        co, ci, cf, ho, hi = orc.find(ofam, abi.dnms_view(cutoff=cutoff, **c), P, abi.FIND_SECOND_WINDOW)[:5]
        found = [dict(cand_idx=ci[co[k]: co[k + 1]], cand_flags=cf[co[k]: co[k + 1]], het_idx=hi[ho[k]: ho[k + 1]]) for k in range(len(dn))]
        f = fetch_points(c["rcontig"], c["start"], [0] * len(dn), sites.pos, ho, hi, P, allele_len=[max(len(r), len(a)) for r, a in zip(refs, alts)])
        f = (np.ascontiguousarray(f[0], np.int32), np.ascontiguousarray(f[1], np.int32), np.ascontiguousarray(f[2], np.int32), np.ascontiguousarray(f[3], np.uint16))
        rid, _, names, _ = _table(engine, src, f)
        per_f.append(f); per_rid.append(rid); per_names.append(names); per_cols.append(c)
        groups.append((engine.add_family(sid, *fam_cols), rid, first, len(dn), cutoff))
        ogroups.append((ofam, orc.upload_reads(rt), first, len(dn), cutoff))
        found_all += found
        for k in cols:
            cols[k] += c[k]
        first += len(dn)
    dv = abi.dnms_view(cutoff=0.0, **cols)
    kid0 = engine.phase_raw(groups[0][0], per_rid[0], abi.dnms_view(cutoff=groups[0][4], **per_cols[0]), P, abi.FIND_SECOND_WINDOW)  # (before any cohort call)
    want = engine.phase_cohort(groups, dv, P)
    oracle = orc.phase_cohort(ogroups, dv, P, found_all)
    case = manycases.Case([paths["bams"][k] for k in kids], per_f, {}, None)
    jrid, _, jnames, jkb = _table(engine, many, manycases.joined_fetches(many, case))
    try:
        yield SimpleNamespace(kids=kids, ds=ds, sites=sites, reads=reads, P=P, many=many, groups=groups, cols=cols, per_cols=per_cols, per_rid=per_rid,
                              per_names=per_names, dv=dv, kid0=kid0, want=want, oracle=oracle, jrid=jrid, jnames=jnames)
    finally:
        engine.free_reads(jrid)
        for r in per_rid:
            engine.free_reads(r)
        engine.free_sites(sid)


def test_joined_cohort_phase_equals_the_cohort_of_tables_and_the_oracle(engine, four):
    t = four
    kids, reads, P, many, groups, cols, dv = t.kids, t.reads, t.P, t.many, t.groups, t.cols, t.dv
    per_names, want, oracle, jrid, jnames = t.per_names, t.want, t.oracle, t.jrid, t.jnames
    engine.set_params(P)
    rec_first, name_first = engine.reads_files(jrid, many.ref_base)
    assert np.array_equal(name_first, manycases.ends([len(x) for x in per_names])) and jnames == [x for p in per_names for x in p]
    got = engine.phase_cohort_joined(jrid, groups, many.ref_base[:-1], dv, P)
    for k in ("status", "counts", "origin", "evidence"):
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[k], oracle[k]), k
    assert int((got["status"] == abi.ST_OK).sum()) >= 3
    for g, (fam, rid, f0, cnt, cutoff) in enumerate(groups):
        rt = reads["mem://%s.bam" % kids[g]]
        for d in range(f0, f0 + cnt):
            for j in (0, 1):  # read names: the table's ids = the file's + the file's first name id
                assert np.array_equal(got["lists"][d][j], want["lists"][d][j].astype(np.int64) + name_first[g]), (g, d, j)
                assert sorted(jnames[q] for q in got["lists"][d][j]) == sorted(rt.qnames[q] for q in oracle["lists"][d][j]), (g, d, j)
            for j in (2, 3):  # site positions
                assert np.array_equal(got["lists"][d][j], want["lists"][d][j]) and np.array_equal(got["lists"][d][j], oracle["lists"][d][j]), (g, d, j)
    # a DNM whose file-local contig is not one of its group's file is on no contig of the table, as in uz_phase_cohort
    bad = dict(cols)
    bad["rcontig"] = [len(many.contigs) // len(kids)] + cols["rcontig"][1:]
    dvb = abi.dnms_view(cutoff=0.0, **bad)
    a, b = engine.phase_cohort_joined(jrid, groups, many.ref_base[:-1], dvb, P, want_lists=False), engine.phase_cohort(groups, dvb, P, want_lists=False)
    for k in ("status", "counts", "origin", "evidence"):
        assert np.array_equal(a[k], b[k]), k


def test_refusals_on_the_joined_table_leave_the_context_usable(engine, four):
    """uz_phase_cohort_joined refuses what uz_phase_cohort refuses of a batch's groups (tests/test_cohort_gpu.py: a gap, an overlap, a group past
    the batch, two sites tables): UZ_E_ARG and a message, a plain uz_phase of kid 0 afterwards as before any cohort call, and the good batch on
    the joined table still what the per-file tables give"""
    from test_cohort_gpu import E_ARG, bad_covers
    t = four
    ped = t.ds.pedigrees[t.kids[2]]
    sid2 = engine.upload_sites(t.sites)
    other = engine.add_family(sid2, *t.sites.family_columns(t.kids[2], ped["dad"], ped["mom"]))
    engine.set_params(t.P)
    n = t.dv.view.n
    out = [np.zeros(4 * n, np.int32) for _ in range(4)]
    base = np.ascontiguousarray(t.many.ref_base[:-1], np.int32)
    dv0 = abi.dnms_view(cutoff=t.groups[0][4], **t.per_cols[0])
    for what, g3 in bad_covers(t.groups[1:], other).items():  # (the last three kids' groups, so that "past n" is past the batch's end)
        g = [t.groups[0]] + g3
        rc = engine.L.uz_phase_cohort_joined(engine.h, int(t.jrid), engine._groups(g), len(g), base.ctypes.data, t.dv.ref(), abi.FIND_SECOND_WINDOW,
                                             *[x.ctypes.data for x in out])
        assert rc == E_ARG, what
        assert engine.L.uz_last_error(engine.h), what
        again = engine.phase_raw(t.groups[0][0], t.per_rid[0], dv0, t.P, abi.FIND_SECOND_WINDOW)
        for k in ("status", "counts", "origin", "evidence"):
            assert np.array_equal(again[k], t.kid0[k]), (what, k)
    got = engine.phase_cohort_joined(t.jrid, t.groups, t.many.ref_base[:-1], t.dv, t.P, want_lists=False)
    for k in ("status", "counts", "origin", "evidence"):
        assert np.array_equal(got[k], t.want[k]), k
    engine.free_sites(sid2)
