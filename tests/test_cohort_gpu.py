"""Cohort batches (uz_phase_cohort): the DNMs of several kids -- own trio columns, own alignment
records, own insert cutoff each -- in one launch sequence give, DNM by DNM, what one uz_phase per kid gives, vote lists
(query-name ids of the kid's own table) included; and the host path, which routes multi-kid batches through it,
reproduces the reference's two-kid goldens (tests/test_golden_gpu.py runs those too)."""
import numpy as np
import pytest

from helpers import tables
from synth.small import SmallConfig, make_small
from unfazed_amd import abi, io_native
from unfazed_amd.hostpath import concordant_cutoff

pytestmark = pytest.mark.gpu


E_ARG = -1
RESULTS = ("status", "counts", "origin", "evidence")


@pytest.fixture(scope="module")
def three(engine):
    """three kids of one synth.small set staged on the context, and what one uz_phase per kid gives for each: made once, before any cohort call
    on these tables"""
    from types import SimpleNamespace
    kids = ["kidA", "kidB", "kidC"]
    ds = make_small(SmallConfig(seed=909, n_dnms=21, kids=kids, cluster_prob=0.6, odd_read_prob=0.05))
    sites, reads = tables(ds)
    P = abi.make_params()
    engine.set_params(P)
    sid = engine.upload_sites(sites)
    fams, rhs, cuts, per_kid = {}, {}, {}, {}
    for kid in kids:
        ped = ds.pedigrees[kid]
        fams[kid] = engine.add_family(sid, *sites.family_columns(kid, ped["dad"], ped["mom"]))
        rt = reads["mem://%s.bam" % kid]
        # one kid staged in the packed form, the others in the ASCII form: the merged table takes either
        rhs[kid] = engine.upload_reads(rt, min_base_qual=P.min_gt_qual if kid == "kidB" else None)
        cuts[kid] = concordant_cutoff(rt.tlen, P.readlen, 3) + (7.0 if kid == "kidC" else 0.0)  # cutoffs differ per kid

    def view(dn, kid, cutoff):
        rt = reads["mem://%s.bam" % kid]
        refs, alts = [], []
        for d in dn:
            j = int(sites.query(d["chrom"], d["start"], d["start"] + 1)[-1])
            refs.append(sites.ref_str[j].encode())
            alts.append(sites.alt_strs[j][0].encode())
        return (dict(contig=[sites.contig_index[d["chrom"]] for d in dn], rcontig=[rt.contig_index[d["chrom"]] for d in dn],
                     start=[d["start"] for d in dn], end=[d["end"] for d in dn], vartype=[0] * len(dn), refs=refs, alts=alts), cutoff)

    groups, cols, first = [], dict(contig=[], rcontig=[], start=[], end=[], vartype=[], refs=[], alts=[]), 0
    want = {}
    for kid in kids:
        dn = [d for d in ds.dnms if d["kid"] == kid]
        c, cutoff = view(dn, kid, cuts[kid])
        dv = abi.dnms_view(cutoff=cutoff, **c)
        r = engine.phase_raw(fams[kid], rhs[kid], dv, P, abi.FIND_SECOND_WINDOW)
        vo, vv = engine.votes(len(dn))
        go, gq = engine.groups(len(dn))
        want[kid] = (r, vo, vv, go, gq)
        groups.append((fams[kid], rhs[kid], first, len(dn), cutoff))
        for k in cols:
            cols[k] += c[k]
        first += len(dn)
    dv_all = abi.dnms_view(cutoff=0.0, **cols)
    yield SimpleNamespace(kids=kids, ds=ds, sites=sites, P=P, sid=sid, fams=fams, rhs=rhs, cuts=cuts, view=view, groups=groups, want=want,
                          dv_all=dv_all, n=first)
    for kid in kids:
        engine.free_reads(rhs[kid])
    engine.free_sites(sid)


def _equals_per_kid(engine, t, got):
    """the results of a cohort batch over t.groups, and the lists the context holds behind them, against one uz_phase per kid"""
    vo, vv = engine.votes(t.n)
    go, gq = engine.groups(t.n)
    for (fam, rh, f0, cnt, cutoff), kid in zip(t.groups, t.kids):
        r, wvo, wvv, wgo, wgq = t.want[kid]
        for k in RESULTS:
            assert np.array_equal(got[k][f0: f0 + cnt], r[k]), (kid, k)
        for d in range(cnt):
            for j in range(4):
                assert np.array_equal(vv[vo[4 * (f0 + d) + j]: vo[4 * (f0 + d) + j + 1]], wvv[wvo[4 * d + j]: wvo[4 * d + j + 1]]), (kid, d, j)
            for j in range(2):
                assert np.array_equal(gq[go[2 * (f0 + d) + j]: go[2 * (f0 + d) + j + 1]], wgq[wgo[2 * d + j]: wgo[2 * d + j + 1]]), (kid, d, j)


def _plain_again(engine, t, what):
    """a plain uz_phase of kid 0 is what it was before any cohort call"""
    kid = t.kids[0]
    dn = [d for d in t.ds.dnms if d["kid"] == kid]
    c, cutoff = t.view(dn, kid, t.cuts[kid])
    again = engine.phase_raw(t.fams[kid], t.rhs[kid], abi.dnms_view(cutoff=cutoff, **c), t.P, abi.FIND_SECOND_WINDOW)
    for k in RESULTS:
        assert np.array_equal(again[k], t.want[kid][0][k]), (what, k)


def test_cohort_batch_equals_per_kid_batches(engine, three):
    t = three
    for attempt in range(2):  # the second call reuses the merged table
        got = engine.phase_cohort(t.groups, t.dv_all, t.P, want_lists=False)
        _equals_per_kid(engine, t, got)
    assert sum(int((t.want[k][0]["status"] == abi.ST_OK).sum()) for k in t.kids) >= 3
    # a plain uz_phase afterwards is unaffected by the cohort state
    _plain_again(engine, t, "after a cohort batch")


def bad_covers(groups, other_fam):
    """four batches over three groups (fam, reads, first, count, cutoff) that a cohort call must refuse: the middle group moved or resized so
    that a DNM is in no group or in two, the last group reaching past the batch, the middle group's family on another sites table"""
    A, B, C = groups
    assert B[3] >= 2
    return {
        "gap": [A, (B[0], B[1], B[2] + 1, B[3] - 1, B[4]), C],
        "overlap": [A, (B[0], B[1], B[2] - 1, B[3] + 1, B[4]), C],
        "past n": [A, B, (C[0], C[1], C[2], C[3] + 1, C[4])],
        "two sites tables": [A, (other_fam, B[1], B[2], B[3], B[4]), C],
    }


def test_refusals_leave_the_context_usable(engine, three):
    """uz_phase_cohort refuses groups that do not cover the batch exactly once, reach past it or mix sites tables (UZ_E_ARG, a message), and the
    context is as usable afterwards as one that never saw the call (tests/test_find_cohort_gpu.py holds uz_find_cohort to the same)"""
    t = three
    ped = t.ds.pedigrees[t.kids[1]]
    sid2 = engine.upload_sites(t.sites)
    other = engine.add_family(sid2, *t.sites.family_columns(t.kids[1], ped["dad"], ped["mom"]))
    engine.set_params(t.P)
    out = [np.zeros(4 * t.n, np.int32) for _ in range(4)]
    for what, g in bad_covers(t.groups, other).items():
        rc = engine.L.uz_phase_cohort(engine.h, engine._groups(g), len(g), t.dv_all.ref(), abi.FIND_SECOND_WINDOW, *[x.ctypes.data for x in out])
        assert rc == E_ARG, what
        assert engine.L.uz_last_error(engine.h), what
        _plain_again(engine, t, what)
    _equals_per_kid(engine, t, engine.phase_cohort(t.groups, t.dv_all, t.P, want_lists=False))
    engine.free_sites(sid2)


def test_one_family_serving_two_groups(engine, three):
    """kid 0's DNMs as two groups over the same family and reads table, next to the other kids' groups, give what the unsplit batch gives, DNM for
    DNM -- with every family's classes stale when the split batch arrives (another min_depth), so that the one scan launch meets kid 0's family
    in two groups and classifies it once"""
    t = three
    P2 = abi.make_params(min_depth=9)
    fam, rh, first, count, cutoff = t.groups[0]
    assert first == 0 and count >= 2
    half = count // 2
    split = [(fam, rh, 0, half, cutoff), (fam, rh, half, count - half, cutoff)] + t.groups[1:]
    got = engine.phase_cohort(split, t.dv_all, P2)
    want = engine.phase_cohort(t.groups, t.dv_all, P2)
    for k in RESULTS:
        assert np.array_equal(got[k], want[k]), k
    assert int((want["status"] == abi.ST_OK).sum()) >= 3
    for d in range(t.n):
        for j in range(4):
            assert np.array_equal(got["lists"][d][j], want["lists"][d][j]), (d, j)


def test_cohort_of_two_hundred_kids_equals_the_oracle_kid_by_kid(engine):
    """The reference's published run is 603 samples in one sites file (README.md:208, unfazed.py:574-575): a cohort batch of 200
    kids x 50 DNMs -- every kid with its own genotype columns, its own alignment records and its own insert cutoff -- through
    ONE uz_phase_cohort, held DNM by DNM against the CPU oracle run kid by kid."""
    import copy
    from oracle import oracle as orc
    from synth import bigsynth
    from synth.sites_np import make_clusters, make_sites, place_dnms_full
    K, D = 200, 50
    from synth.sites_np import DnmColumns
    base = make_sites(600_000, seed=4401, contig_lens=[1.0e8])
    # all DNMs of the cohort at once, on distinct records of the shared table (their REF / ALT are the table's: get_refalt reads the
    # sites file); DNM j belongs to kid j % K
    all_dn = place_dnms_full(base, K * D, seed=5000, indel_frac=0.2)
    P = abi.make_params()
    engine.set_params(P)
    sv = abi.SitesView()
    keep = dict(contig_off=np.ascontiguousarray(base.contig_off, np.int64), pos=base.pos, sflags=base.sflags, ref_base=base.ref_base, alt_base=base.alt_base)
    sv.n_sites, sv.n_contigs = base.n, 1
    for k, a in keep.items():
        setattr(sv, k, a.ctypes.data)
    sites_h = abi.Held(sv, keep)
    sid = engine.upload_sites_view(sites_h)
    groups, want, cols, first = [], [], dict(contig=[], rcontig=[], start=[], end=[], vartype=[], refs=[], alts=[]), 0
    rids = []
    for kid in range(K):
        # the kid's trio: the base genotype columns shifted along the table (every kid sees other genotypes at a site), then its
        # own DNM records made kid het / parents hom-ref with good depth and GQ, as place_dnms_full makes them
        sel = np.arange(kid, K * D, K)
        idx = all_dn.site_idx[sel]
        sc = copy.copy(base)
        sh = 997 * kid + 13
        sc.gt = np.roll(base.gt, sh).copy()
        sc.khap = np.roll(base.khap, sh).copy()
        sc.rd = np.ascontiguousarray(np.roll(base.rd, sh, axis=1))
        sc.ad = np.ascontiguousarray(np.roll(base.ad, sh, axis=1))
        sc.gq = np.ascontiguousarray(np.roll(base.gq, sh, axis=1))
        sc.gt[idx] = 1
        sc.khap[idx] = 0
        for m in range(3):
            sc.rd[m][idx] = 30 if m else 15
            sc.ad[m][idx] = 0 if m else 15
            sc.gq[m][idx] = 99
        dn = DnmColumns(idx, all_dn.contig[sel], all_dn.start[sel], all_dn.end[sel], all_dn.kind[sel], all_dn.length[sel], all_dn.origin[sel],
                        [all_dn.refs[j] for j in sel], [all_dn.alts[j] for j in sel])
        cl = make_clusters(dn)
        cfg = bigsynth.make_cfg(seed=6000 + kid)
        cfg.n_clusters = cl.n
        rh, arrs = bigsynth.reads_cpu(cfg, sc, dn, cl, 0, cl.n, threads=4)
        cutoff = concordant_cutoff(arrs["tlen"][: min(int(rh.view.n_segs), 100000)], P.readlen, 3) + float(kid % 3)
        fam_view = abi.family_view(sc.gt, sc.rd, sc.ad, sc.gq)
        dv = abi.dnms_view(dn.contig, dn.contig, dn.start, dn.end, np.zeros(D, np.uint8), dn.refs, dn.alts, cutoff)
        found = orc.find(P, sites_h, fam_view, dv, abi.FIND_SECOND_WINDOW)
        want.append(orc.phase(P, sites_h, rh, dv, found, keep_lists=False))
        fam = engine.add_family(sid, sc.gt, sc.rd, sc.ad, sc.gq)
        packed = io_native.pack_reads(rh, int(P.min_gt_qual), lists=True, with_end=None, cigar_compact=True)
        rid = engine.upload_reads_packed(packed)
        engine.wait_reads(rid)
        rids.append(rid)
        groups.append((fam, rid, first, D, cutoff))
        cols["contig"] += dn.contig.tolist(); cols["rcontig"] += dn.contig.tolist(); cols["start"] += dn.start.tolist(); cols["end"] += dn.end.tolist()
        cols["vartype"] += [0] * D; cols["refs"] += list(dn.refs); cols["alts"] += list(dn.alts)
        first += D
    dv_all = abi.dnms_view(cutoff=0.0, **cols)
    got = engine.phase_cohort(groups, dv_all, P, want_lists=False)
    phased = 0
    for kid in range(K):
        f0 = kid * D
        for k in ("status", "counts", "origin", "evidence"):
            assert np.array_equal(got[k][f0: f0 + D], want[kid][k]), (kid, k)
        phased += int((want[kid]["status"] == abi.ST_OK).sum())
    assert phased > K * D // 10
    for rid in rids:
        engine.free_reads(rid)
    engine.free_sites(sid)
