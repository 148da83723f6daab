"""Trios made on the device from a sample table (uz_samples_upload + uz_families_from_samples: the members' 16-bit rows aliased, the packed
genotype byte written by k_family_gt_pack with the complex bit folded in, the wide depths gathered) against the same trios made on the host
(SitesTable.family_columns + uz_family_upload): the device columns byte for byte (uz_family_fetch), and everything downstream -- class
bytes, window lists, a cohort read stage, the allele-balance stage."""
import ctypes as C

import numpy as np
import pytest

from helpers import tables
from synth.small import SmallConfig, make_small
from unfazed_amd import abi
from unfazed_amd.hostpath import concordant_cutoff

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


def _cohort_table():
    """the data of test_cohort_gpu.test_cohort_batch_equals_per_kid_batches (three kids, nine samples) with four more samples in the sites
    table: a sibling of kidA, a child of kidB (kidB is then kid AND parent), that child's other parent and an unused one -- their rows are
    other samples' rows shifted along the table; plus a few depths the 16-bit columns cannot hold, in several samples"""
    kids = ["kidA", "kidB", "kidC"]
    ds = make_small(SmallConfig(seed=909, n_dnms=21, kids=kids, cluster_prob=0.6, odd_read_prob=0.05))
    sites, reads = tables(ds)
    extra = ["sibA", "grandkid", "spouseB", "spare"]
    src = [sites.samples.index(s) for s in ("kidA", "kidC", "mom1", "dad3")]
    for name in ("gt", "ref_depth", "alt_depth", "gq"):
        a = getattr(sites, name)
        more = np.stack([np.roll(a[j], 17 * (k + 1)) for k, j in enumerate(src)])
        setattr(sites, name, np.ascontiguousarray(np.concatenate([a, more])))
    sites.samples = sites.samples + extra
    n = sites.n_sites
    rng = np.random.default_rng(77)
    plain = np.nonzero(sites.sflags == 0)[0]
    deep = rng.choice(plain, 9, replace=False)
    col = {s: i for i, s in enumerate(sites.samples)}
    sites.ref_depth[col["kidA"], deep[0]] = 40000
    sites.alt_depth[col["kidA"], deep[0]] = 39000
    sites.ref_depth[col["dad1"], deep[1]] = 32768
    sites.alt_depth[col["mom1"], deep[2]] = 1 << 30
    sites.ref_depth[col["kidB"], deep[3]] = 70000
    sites.alt_depth[col["kidB"], deep[3]] = 70000
    sites.ref_depth[col["sibA"], deep[4]] = 50000
    sites.alt_depth[col["grandkid"], deep[5]] = 33000
    sites.ref_depth[col["spare"], deep[6]] = 99999  # (a sample no trio names: it is not uploaded)
    sites.ref_depth[col["mom2"], deep[7]] = 32767  # (fits: not a wide site)
    sites.alt_depth[col["kidC"], deep[8]] = 45000
    for j in deep:  # the members of such a site confident enough that the exact depths decide its class
        sites.gq[:, j] = 99.0
    assert n > 300 and (sites.sflags & 1).any()
    trios = [(k, ds.pedigrees[k]["dad"], ds.pedigrees[k]["mom"]) for k in kids]
    trios += [("sibA", "dad1", "mom1"), ("grandkid", "kidB", "spouseB")]
    return ds, sites, reads, trios


def _dnm_cols(sites, rt, dn):
    refs, alts = [], []
    for d in dn:
        j = int(sites.query(d["chrom"], d["start"], d["start"] + 1)[-1])
        refs.append(sites.ref_str[j].encode())
        alts.append(sites.alt_strs[j][0].encode())
    return dict(contig=[sites.contig_index[d["chrom"]] for d in dn], rcontig=[rt.contig_index[d["chrom"]] for d in dn], start=[d["start"] for d in dn],
                end=[d["end"] for d in dn], vartype=[0] * len(dn), refs=refs, alts=alts)


def test_device_made_families_equal_uploaded_families(engine):
    ds, sites, reads, trios = _cohort_table()
    n = sites.n_sites
    P = abi.make_params()
    engine.set_params(P)
    sid = engine.upload_sites(sites)
    # the host route, one trio at a time
    host = []
    n_wide_host = 0
    for t in trios:
        gt, rd, ad, gq = sites.family_columns(*t)
        wide = sites.wide_depths
        n_wide_host += 0 if wide is None else len(wide[0])
        host.append(engine.add_family(sid, gt, rd, ad, gq, wide=wide))
    assert n_wide_host >= 6
    # the device route: the samples the trios name, once; all trios in one call
    names = list(dict.fromkeys(s for t in trios for s in t))
    assert len(sites.samples) >= 12 and len(names) == 12 and "spare" not in names
    cols = sites.sample_columns(names)
    assert cols.wide is not None and len(cols.wide[0]) == 7
    mid = engine.upload_samples(sid, cols)
    dev = engine.families_from_samples(mid, [cols.row(t[0]) for t in trios], [cols.row(t[1]) for t in trios], [cols.row(t[2]) for t in trios])
    assert len(set(dev)) == len(trios) and not set(dev) & set(host)

    # the device columns, byte for byte; the complex bit is in gt on both routes
    for t, fh, fd in zip(trios, host, dev):
        gh, ch = engine.family_fetch(fh, n)
        gd, cd = engine.family_fetch(fd, n)
        assert np.array_equal(gh, gd), t
        assert np.array_equal(ch, cd), t
        assert np.array_equal((gd & 0x40) != 0, (sites.sflags & 1) != 0) and not (gd & 0x80).any()
        gt, rd, ad, gq = sites.family_columns(*t)
        assert np.array_equal(gd & 0x3F, gt) and np.array_equal(cd, np.concatenate([rd, ad, gq]))

    # class bytes, wide sites included: default thresholds and another pair
    P2 = abi.make_params(min_depth=20, min_gt_qual=40)
    wide_sites = cols.wide[0]
    for params in (P, P2, P):
        for t, fh, fd in zip(trios, host, dev):
            a, b = engine.classify(fh, params, n), engine.classify(fd, params, n)
            assert np.array_equal(a, b), t
            assert np.array_equal(a[wide_sites], b[wide_sites])
    one = engine.classify(host[0], P, n)
    assert not np.array_equal(one, engine.classify(host[0], P2, n))
    engine.set_params(P)
    engine.site_scan_many(dev)  # the cohort scan takes them too
    for fh, fd in zip(host, dev):
        assert np.array_equal(engine.classify(fh, P, n), engine.classify(fd, P, n))

    # window lists
    real = {"kidA": 0, "kidB": 1, "kidC": 2, "sibA": 0, "grandkid": 1}  # whose DNMs / alignment records a trio is run on
    kid_names = ["kidA", "kidB", "kidC"]
    for t, fh, fd in zip(trios, host, dev):
        kid = kid_names[real[t[0]]]
        rt = reads["mem://%s.bam" % kid]
        dn = [d for d in ds.dnms if d["kid"] == kid]
        dv = abi.dnms_view(cutoff=0.0, **_dnm_cols(sites, rt, dn))
        for mode in (abi.FIND_SECOND_WINDOW, 0):
            fa, fb = engine.find(fh, dv, P, mode), engine.find(fd, dv, P, mode)
            for x, y in zip(fa, fb):
                assert np.array_equal(x, y), (t, mode)
        assert int(fa[0][-1]) + int(fa[3][-1]) > 0

    # the cohort read stage over all five trios (the two extra trios on tables of their own: copies of kidA's and kidB's records)
    def cohort(fams):
        groups, allc, first, rids = [], dict(contig=[], rcontig=[], start=[], end=[], vartype=[], refs=[], alts=[]), 0, []
        for t, f in zip(trios, fams):
            kid = kid_names[real[t[0]]]
            rt = reads["mem://%s.bam" % kid]
            dn = [d for d in ds.dnms if d["kid"] == kid]
            rid = engine.upload_reads(rt, min_base_qual=P.min_gt_qual if kid == "kidB" else None)
            rids.append(rid)
            c = _dnm_cols(sites, rt, dn)
            groups.append((f, rid, first, len(dn), concordant_cutoff(rt.tlen, P.readlen, 3) + float(len(groups))))
            for k in allc:
                allc[k] += c[k]
            first += len(dn)
        got = engine.phase_cohort(groups, abi.dnms_view(cutoff=0.0, **allc), P, want_lists=False)
        vo, vv = engine.votes(first)
        go, gq = engine.groups(first)
        out = {k: got[k].copy() for k in ("status", "counts", "origin", "evidence")}
        out.update(vo=vo.copy(), vv=vv.copy(), go=go.copy(), gq=gq.copy())
        for rid in rids:
            engine.free_reads(rid)
        return out
    a, b = cohort(host), cohort(dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert int((a["status"] == abi.ST_OK).sum()) >= 3

    # the allele-balance stage: one DEL and one DUP over stretches of the table
    pos0 = sites.pos[int(sites.contig_off[0]): int(sites.contig_off[1])]
    lo, hi = int(pos0[len(pos0) // 5]), int(pos0[len(pos0) // 2])
    lo2, hi2 = int(pos0[len(pos0) // 2]) + 1, int(pos0[-2])
    dvc = abi.dnms_view([0, 0], [0, 0], [lo, lo2], [hi, hi2], np.asarray([1, 2], np.uint8), [b"", b""], [b"", b""], 0.0)
    votes = 0
    for t, fh, fd in zip(trios, host, dev):
        ra, rb = engine.phase_cnv(fh, dvc, P), engine.phase_cnv(fd, dvc, P)
        for k in ("cnv_counts", "origin", "evidence", "etype"):
            assert np.array_equal(ra[k], rb[k]), (t, k)
        for la, lb in zip(ra["lists"], rb["lists"]):
            assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
        votes += int(ra["cnv_counts"].sum())
    assert votes > 0

    # lifetime and arguments
    L, h = engine.L, engine.h
    assert L.uz_samples_free(h, mid) == E_STATE  # families made from it are alive
    out = (C.c_int * 4)()
    i32 = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    k, d, m = i32(0), i32(1), i32(2)
    assert L.uz_families_from_samples(h, mid, -1, k.ctypes.data, d.ctypes.data, m.ctypes.data, out) == E_ARG
    for bad in (i32(12), i32(-1)):
        assert L.uz_families_from_samples(h, mid, 1, bad.ctypes.data, d.ctypes.data, m.ctypes.data, out) == E_ARG
        assert L.uz_families_from_samples(h, mid, 1, k.ctypes.data, d.ctypes.data, bad.ctypes.data, out) == E_ARG
    assert L.uz_families_from_samples(h, mid + 1000, 1, k.ctypes.data, d.ctypes.data, m.ctypes.data, out) == E_ARG  # no such table
    assert L.uz_samples_free(h, mid + 1000) == E_ARG
    assert L.uz_families_from_samples(h, mid, 0, None, None, None, None) == 0  # no trios: nothing to do
    # a table of ANOTHER sites table: its families belong to that table, and a table nobody made families from can be freed
    sid2 = engine.upload_sites(sites)
    mid2 = engine.upload_samples(sid2, cols)
    assert mid2 != mid
    f2 = engine.families_from_samples(mid2, [cols.row("kidA")], [cols.row("dad1")], [cols.row("mom1")])
    assert np.array_equal(engine.classify(f2[0], P, n), engine.classify(host[0], P, n))
    with pytest.raises(Exception):
        engine.site_scan_many([dev[0], f2[0]])  # families of two sites tables do not mix
    mid3 = engine.upload_samples(sid2, cols)
    engine.free_samples(mid3)
    engine.free_sites(sid2)  # frees f2 and mid2 with it
    assert L.uz_samples_free(h, mid2) == E_ARG
    assert L.uz_families_from_samples(h, mid2, 1, k.ctypes.data, d.ctypes.data, m.ctypes.data, out) == E_ARG

    # a plain uz_family_upload on the same sites table afterwards is what it was
    gt, rd, ad, gq = sites.family_columns(*trios[0])
    again = engine.add_family(sid, gt, rd, ad, gq, wide=sites.wide_depths)
    assert np.array_equal(engine.classify(again, P, n), one)
    ga, ca = engine.family_fetch(again, n)
    gh, ch = engine.family_fetch(host[0], n)
    assert np.array_equal(ga, gh) and np.array_equal(ca, ch)
    # ... and more trios from the first table: the table serves a second call
    more = engine.families_from_samples(mid, [cols.row("sibA")], [cols.row("dad1")], [cols.row("mom1")])
    assert np.array_equal(engine.classify(more[0], P, n), engine.classify(host[3], P, n))
    engine.free_sites(sid)
    assert L.uz_samples_free(h, mid) == E_ARG  # (went with its sites table)


def test_empty_sites_table_and_many_trios_of_few_samples(engine):
    """a table without sites makes families without a launch; 300 trios drawn from 6 samples of a 5 000-site table (tails shorter than a
    16-site vector included) equal the packed byte computed on the host"""
    from unfazed_amd.model import SitesTable
    samples = ["s%d" % i for i in range(6)]
    P = abi.make_params()
    e = SitesTable(samples, ["1"])
    sid = engine.upload_sites(e)
    mid = engine.upload_samples(sid, e.sample_columns(samples))
    f = engine.families_from_samples(mid, [0, 3], [1, 4], [2, 5])
    assert len(f) == 2
    engine.free_sites(sid)
    rng = np.random.default_rng(3)
    for n in (5003, 16, 7):
        t = SitesTable(samples, ["1"])
        t.contig_off = np.asarray([0, n], np.int64)
        t.pos = np.cumsum(rng.integers(1, 50, n)).astype(np.int32)
        t.end = t.pos + 1
        t.sflags = (rng.random(n) < 0.2).astype(np.uint8)
        t.ref_base = np.where(t.sflags == 0, ord("A"), 0).astype(np.uint8)
        t.alt_base = np.where(t.sflags == 0, ord("C"), 0).astype(np.uint8)
        t.gt = rng.integers(0, 4, (6, n)).astype(np.uint8)
        t.ref_depth = rng.integers(-1, 80, (6, n)).astype(np.int32)
        t.alt_depth = rng.integers(-1, 80, (6, n)).astype(np.int32)
        t.gq = rng.uniform(-1, 99, (6, n))
        sid = engine.upload_sites(t)
        cols = t.sample_columns(samples)
        mid = engine.upload_samples(sid, cols)
        tr = rng.integers(0, 6, (300, 3))
        fams = engine.families_from_samples(mid, tr[:, 0], tr[:, 1], tr[:, 2])
        for q in (0, 1, 150, 299):
            g, c = engine.family_fetch(fams[q], n)
            k, d, m = (int(x) for x in tr[q])
            assert np.array_equal(g, (t.gt[k] & 3) | ((t.gt[d] & 3) << 2) | ((t.gt[m] & 3) << 4) | ((t.sflags & 1) << 6))
            assert np.array_equal(c[0], cols.ref_depth[k]) and np.array_equal(c[4], cols.alt_depth[d]) and np.array_equal(c[8], cols.gq[m])
        gtp, rd, ad, gq = t.family_columns(*(samples[int(x)] for x in tr[7]))
        up = engine.add_family(sid, gtp, rd, ad, gq)
        assert np.array_equal(engine.classify(up, P, n), engine.classify(fams[7], P, n))
        engine.free_sites(sid)
