"""The read stage held to hand-built reads at every rule's edge (tests/readcases.py), on the CPU: the reference's recorded answers
(tests/golden/read_edges.json, written by tests/golden/make_golden_edges.py) against the case table's hand-written expectations, the oracle,
the kernel body's CPU twin (tests/emu) and the reach rule of the staged forms."""
import contextlib
import copy
import functools
import io
import json
import os
import sys

import numpy as np
import pytest

import readcases
from helpers import RUN_DEFAULTS, norm_records, run_host, tables
from oracle import oracle as orc
from oracle_backend import OracleBackend
from unfazed_amd import abi
from unfazed_amd.hostpath import concordant_cutoff, vartype_code

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PANELS = {"point": readcases.point_panel, "sv": readcases.sv_panel}
RUN_IDS = [(p, r) for p, runs in (("point", readcases.RUNS), ("sv", readcases.SV_RUNS)) for r in runs]


@functools.lru_cache(maxsize=None)
def panel(name):
    return PANELS[name]()


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLD, "read_edges.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def panel_tables(name):
    return tables(panel(name).dataset)


def run_panel(backend, name, run, sites=None, reads=None, bams=None, sites_name=None):
    """One run of a panel through the host path with `backend` -> (records, annotated DNMs, stderr lines).  bams / sites_name: file paths
    instead of the in-memory tables (through the session)."""
    pn = panel(name)
    ds = pn.dataset
    kw = pn.runs[run]
    if name == "point" and bams is None:
        if sites is None:
            sites, reads = panel_tables(name)
        recs, dn, err = run_host(backend, ds, sites, reads, **kw)
        return recs, dn, err.splitlines()
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    from unfazed_amd.sv_phaser import phase_svs
    a = dict(RUN_DEFAULTS)
    a.update(kw)
    own = session._BACKEND
    session.set_backend(backend)
    session._READS.clear()
    session._HOSTS.clear()
    for k in [k for k in session._SITES if "@" in k]:
        del session._SITES[k]
    try:
        dn = copy.deepcopy(ds.dnms)
        if bams is None:
            if sites is None:
                sites, reads = panel_tables(name)
            sites_name = "mem://read_edges_%s" % name
            session.register_sites(sites_name, sites)
            for k, t in reads.items():
                session.register_reads(k, t)
        else:
            for d in dn:
                d["bam"] = bams[d["kid"]]
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            recs = (phase_snvs if name == "point" else phase_svs)(
                dn, list(ds.pedigrees), ds.pedigrees, sites_name, a["threads"], a["build"], a["no_extended"], a["multithread_proc_min"],
                a["quiet_mode"], a["ab_homref"], a["ab_homalt"], a["ab_het"], a["min_gt_qual"], a["min_depth"], a["search_dist"],
                a["insert_size_max_sample"], a["stdevs"], a["min_map_qual"], a["readlen"], a["split_error_margin"])
    finally:
        session.set_backend(own)
        session._READS.clear()
        session._HOSTS.clear()
    return recs, dn, err.getvalue().splitlines()


def assert_same_as_golden(name, run, got):
    """records, their order, stderr and the annotated site lists of one run against the reference's"""
    recs, dn, err = got
    g = golden()[name]
    r = g["runs"][run]
    assert r["run"] == panel(name).runs[run]
    assert list(recs.keys()) == r["record_order"]
    assert json.loads(json.dumps(norm_records(recs))) == r["records"]
    assert err == r["stderr"]
    assert len(dn) == len(g["dnms"])
    for d, w in zip(dn, g["dnms"]):
        assert (d["chrom"], d["start"], d["end"], d["kid"]) == (w["chrom"], w["start"], w["end"], w["kid"])
        assert d.get("candidate_sites") == w["candidate_sites"] and d.get("het_sites") == w["het_sites"]


def assert_same_runs(a, b):
    assert list(a[0].keys()) == list(b[0].keys()) and norm_records(a[0]) == norm_records(b[0])
    assert a[2] == b[2]
    assert [(d.get("candidate_sites"), d.get("het_sites")) for d in a[1]] == [(d.get("candidate_sites"), d.get("het_sites")) for d in b[1]]


@functools.lru_cache(maxsize=None)
def oracle_run(name, run):
    """the oracle's answers, computed once and shared (never modified by a test)"""
    return run_panel(OracleBackend(), name, run)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PANELS))
def test_panel_is_the_one_the_reference_answered(name):
    sys.path.insert(0, GOLD)
    from make_golden import dataset_digest
    pn = panel(name)
    assert dataset_digest(pn.dataset) == golden()[name]["digest"], "the case table changed: run tests/golden/make_golden_edges.py"
    assert golden()[name]["cutoff"] == {readcases.KID: readcases.CUTOFF}
    assert len(pn.cases) >= (25 if name == "point" else 6)


@pytest.mark.parametrize("name", sorted(PANELS))
def test_every_hand_written_expectation_holds_in_the_reference(name):
    """each case sits on the edge it names: the reference itself gives the outcome worked out by hand for every probe pair"""
    pn = panel(name)
    g = golden()[name]
    n = 0
    for c in pn.cases:
        for run, qname, want in c.expect:
            got = readcases.outcome(g["runs"][run]["records"].get(c.key), qname)
            assert got == want, (c.name, c.rule, run, qname, want, got)
            n += 1
    assert n >= (150 if name == "point" else 50)
    if name == "point":  # the ladders: 127 and 128 het sites, every one of them reached by the chain
        by_start = {d["start"]: d for d in g["dnms"]}
        for c in pn.cases:
            if hasattr(c, "n_het"):
                assert len(by_start[c.pos]["het_sites"]) == c.n_het
                assert len(g["runs"]["default"]["records"][c.key]["dad_sites"]) == c.n_het


@pytest.mark.parametrize("name,run", RUN_IDS)
def test_oracle_reproduces_the_reference(name, run):
    assert_same_as_golden(name, run, oracle_run(name, run))


# ---------------------------------------------------------------------------------------------------------------------------------------
def batch_views(name, run):
    """-> (params, sites view, reads view, reads Held source, DNM view, found, allele lengths) of one run of a panel, as the host would hand
    them to the read stage"""
    pn = panel(name)
    ds = pn.dataset
    sites, reads = panel_tables(name)
    rt = reads["mem://%s.bam" % readcases.KID]
    a = dict(RUN_DEFAULTS)
    a.update(pn.runs[run])
    from helpers import params_from
    P = params_from(a)
    sv = abi.sites_view(sites)
    ped = ds.pedigrees[readcases.KID]
    fv = abi.family_view(*sites.family_columns(readcases.KID, ped["dad"], ped["mom"]))
    rv = abi.reads_view(rt)
    dn = ds.dnms
    n = len(dn)
    if name == "point":
        refs = [c.ref.encode() for c in pn.cases]
        alts = [c.alt.encode() for c in pn.cases]
    else:
        refs = alts = [b""] * n
    head = rt.tlen_head[: int(a["insert_size_max_sample"]) + 1]
    cutoff = concordant_cutoff(head, P.readlen, 3)
    assert cutoff == readcases.CUTOFF
    vt = [vartype_code(d["vartype"]) for d in dn]
    dv = abi.dnms_view([0] * n, [0] * n, [d["start"] for d in dn], [d["end"] for d in dn], vt, refs, alts, cutoff)
    found = orc.find(P, sv, fv, dv, abi.FIND_SECOND_WINDOW)
    alen = np.array([max(len(r), len(x)) for r, x in zip(refs, alts)], np.int64)
    return P, sv, rv, dv, found, alen, vt, rt


def assert_same_phase(want, got, n, lists=True):
    for k in ("status", "counts", "origin", "evidence"):
        assert np.array_equal(want[k], got[k]), k
    if lists:
        vo, vv = want["vote_off"], want["vote_val"]
        for d in range(n):
            for j in range(4):
                assert np.array_equal(vv[vo[4 * d + j]: vo[4 * d + j + 1]], got["lists"][d][j]), (d, j)


@pytest.mark.parametrize("name,run", RUN_IDS)
def test_kernel_body_matches_oracle_on_every_case(name, run):
    """the kernel body's CPU twin on the whole panel (ladders included: the twin takes about a second for them), as test_emu_phase does on
    generated reads: status, counts, origin, evidence and the four vote lists of every case, and no base or quality bit asked for that the
    staged form would not hold"""
    from emu import emu
    P, sv, rv, dv, found, alen, vt, rt = batch_views(name, run)
    n = dv.view.n
    want = orc.phase(P, sv, rv, dv, found, keep_lists=True)
    got = emu.phase(P, sv, rv, dv, found)
    assert got["base_err"] == 0
    assert_same_phase(want, got, n)
    assert int((want["status"] == abi.ST_OK).sum()) == n


@pytest.mark.parametrize("name,run", [("point", "default"), ("point", "small"), ("point", "mapq20"), ("sv", "default")])
@pytest.mark.parametrize("base_lists", [False, True], ids=["units", "lists"])
def test_kernel_body_stays_inside_what_the_reach_rule_staged(name, run, base_lists):
    """The reach rule on the panel, in the manner of test_pack_select's ..._staged_units / ..._listed_bases (those run the big generator's
    M-only reads): select with ReadsSource.select for the panel's fetch points -- with unit masks, and again with base lists -- and run the twin on
    exactly what was selected: records nobody fetched without their bases, of the others only the staged units / the listed bases.  Results
    equal the oracle's on the whole table and the guard stays silent, on MNPs across unit boundaries, gaps, clips and short reads.  (A
    --no-extended batch is staged with all its bases: there is no reach to check.)"""
    from emu import emu
    from unfazed_amd import io_native
    from unfazed_amd.staging import fetch_points
    P, sv, rv, dv, found, alen, vt, rt = batch_views(name, run)
    n = dv.view.n
    N = rt.n_segs
    want = orc.phase(P, sv, rv, dv, found, keep_lists=True)
    sites, _ = panel_tables(name)
    dn = panel(name).dataset.dnms
    fc, flo, fhi, fex = fetch_points([0] * n, [d["start"] for d in dn], np.zeros(n, np.uint8), sites.pos, found[3], found[4], P,
                                     vartype=np.array(vt), end=[d["end"] for d in dn], cutoff=readcases.CUTOFF, allele_len=alen)
    src = io_native.ReadsSource(io_native.pack_reads(rv, P.min_gt_qual, with_end=True))
    part, idx = src.select(fc, flo, fhi, want_index=True, extra=fex, base_lists=base_lists)
    small = abi.small_columns(part)
    m = int(part.view.n_segs)
    # the selection is what the fetches return, closed under `mate`
    keep = np.zeros(N, bool)
    for lo, hi in zip(flo, fhi):
        keep |= (rt.start < hi) & (rt.end > lo)
    direct = keep.copy()
    for _ in range(4):
        mt = rt.mate[keep]
        keep[mt[mt >= 0]] = True
    assert np.array_equal(np.nonzero(keep)[0], idx)
    um = np.zeros(N, np.uint16)
    um[idx] = small["umask"][:m]
    no_seq = np.ones(N, bool)
    no_seq[idx] = (small["aux"][:m] & abi.AUX_NO_SEQ) != 0
    assert np.array_equal(no_seq[idx], ~direct[idx])
    bl = None
    if base_lists:
        off, pos, code = abi.base_lists(part)
        cnt = np.diff(off)
        assert (cnt > 0).sum() > (50 if name == "point" else 0)  # (the +-cutoff fetches of an SV batch list nothing: few records there)
        # codes = the source's bases at the listed positions
        rec_of = np.repeat(np.arange(m), cnt)
        row0 = rt.sq_off16[idx[rec_of]].astype(np.int64) * 16
        lut = np.full(256, 255, np.uint8)
        for k, ch in enumerate(b"ACGT"):
            lut[ch] = k
        assert np.array_equal(code, lut[rt.seq[row0 + pos.astype(np.int64)]])
        full_cnt = np.zeros(N, np.int64)
        full_cnt[idx] = cnt
        full_off = np.concatenate([[0], np.cumsum(full_cnt)]).astype(np.int64)
        full_pos = np.zeros(int(full_off[-1]), np.uint16)
        for k in np.nonzero(cnt)[0]:
            full_pos[full_off[idx[k]]: full_off[idx[k] + 1]] = pos[off[k]: off[k + 1]]
        bl = (full_off, full_pos)
    got = emu.phase(P, sv, rv, dv, found, no_seq=no_seq, umask=um, bl=bl)
    assert got["base_err"] == 0
    assert_same_phase(want, got, n)
    # ... and the guard is awake on this panel: the same rows with the DNMs' own fetches left out of the masks trip it
    if name == "point":
        sel = np.arange(fc.size) >= n  # (fetch_points lists the n DNM fetches first)
        part2, idx2 = src.select(fc[sel], flo[sel], fhi[sel], want_index=True, extra=fex[sel], base_lists=base_lists)
        small2 = abi.small_columns(part2)
        um2 = np.zeros(N, np.uint16)
        um2[idx2] = small2["umask"][: idx2.size]
        bl2 = None
        if base_lists:
            off2, pos2, _ = abi.base_lists(part2)
            c2 = np.zeros(N, np.int64)
            c2[idx2] = np.diff(off2)
            fo2 = np.concatenate([[0], np.cumsum(c2)]).astype(np.int64)
            fp2 = np.zeros(int(fo2[-1]), np.uint16)
            for k in np.nonzero(np.diff(off2))[0]:
                fp2[fo2[idx2[k]]: fo2[idx2[k] + 1]] = pos2[off2[k]: off2[k + 1]]
            bl2 = (fo2, fp2)
        got2 = emu.phase(P, sv, rv, dv, found, no_seq=no_seq, umask=np.where(no_seq, um, um2), bl=bl2)
        assert got2["base_err"] in (3, 4)


@pytest.mark.parametrize("name", sorted(PANELS))
def test_panel_written_as_files_comes_back_and_phases_the_same(name, tmp_path, monkeypatch):
    """tests/filesio.py writes every operation and record shape of the panel (H, P, N, = / X, short reads, an unmapped record with a CIGAR): the
    native BAM decoder gives back the table that ReadsTable.from_segments builds, and the product's file route (session, BAI, the host's walk),
    answered by the oracle, gives the reference's records."""
    from filesio import dump_dataset, write_bai
    from unfazed_amd import io_native
    monkeypatch.setenv("UZ_WALK", "host")
    ds = panel(name).dataset
    paths = dump_dataset(ds, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    got = io_native.read_bam_table(paths["bams"][readcases.KID], threads=2)
    want = panel_tables(name)[1]["mem://%s.bam" % readcases.KID]
    for k in ("start", "end", "flag", "mapq", "aux", "tlen", "mate", "n_cigar", "l_seq", "cigar", "seq", "qual"):
        assert np.array_equal(np.asarray(getattr(got, k)), getattr(want, k)), k
    assert [got.qnames[i] for i in got.qname] == [want.qnames[i] for i in want.qname]
    for run in panel(name).runs:
        assert_same_as_golden(name, run, run_panel(OracleBackend(), name, run, bams=paths["bams"], sites_name=paths["sites"]))
