#!/usr/bin/env python
"""A/B of the two routes of the read side of a cohort call (PhasingHost._reads_route):
  kid     every kid's BAM staged by itself -- fetch list, walk, joins, table -- then uz_phase_cohort lays the tables end to end
          (UZ_READS_ROUTE=kid: the code before the cohort route)
  cohort  the kids' BAMs presented to the BAM stage as ONE file (io_native.BamSource.open_many), walked and joined in one batch per run of
          at most UZ_COHORT_RUN_DNMS DNMs, uz_phase_cohort_joined on the table that comes out
Workload: --kids kids (default 600, sibships of three) x --snvs SNV DNMs (default 48), one synthetic BAM + BAI per kid (synth/bigsynth.py's
writer: the read pile-ups of the kid's DNMs), one sample table in memory.  ONE phase_snvs call per measurement, all kids named; timed: the
"reads" section of the host path (UZ_HOST_TRACE) and the whole call.  One process, turn by turn: --warmup calls of every setting, then
--repeat timed calls of each -- the kid route, and the cohort route at every --runs value (DNMs per run; 0 = all kids in one run).
Reported per setting: every wall time, the median, the device calls (PhasingHost.stats) and whether the records equal the kid route's.
`cohort_beats_kid`: every cohort run below every kid run, the rule a default is changed by.
    timeout -k 10 1100 python scripts/reads_route_ab.py [--kids 600] [--snvs 48] [--runs 1700,3400,6800,0] [--repeat 5] [--out profiles/reads_route_ab.json]"""
import argparse
import contextlib
import copy
import hashlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["UZ_HOST_TRACE"] = "1"  # (read when hostpath is imported)
os.environ.setdefault("UZ_HOST_CHUNKS", "0")


def make_cohort(n_kids, n_snvs, n_sites, out_dir, seed=41):
    """-> (sites table, pedigrees, DNM dicts): a sample table over synthetic sites (the generator's trio columns, one per kid / father / mother),
    every kid's DNMs on records of their own (kid het, parents hom-ref, good depth and quality) and the kid's BAM + BAI with the read pile-ups around them"""
    import numpy as np
    from synth import bigsynth
    from synth.sites_np import DnmColumns, make_clusters, make_sites, place_dnms_full
    from unfazed_amd.model import SitesTable
    lens = [100_000_000]
    base = make_sites(n_sites, seed=seed, contig_lens=lens, complex_frac=0.0, weird_frac=0.0)
    all_dn = place_dnms_full(base, n_kids * n_snvs, seed=seed + 1, indel_frac=0.0)
    n_par = 2 * ((n_kids + 2) // 3)
    names = ["k%04d" % i for i in range(n_kids)] + ["p%04d" % i for i in range(n_par)]
    t = SitesTable(names, list(base.contig_names))
    # every kid carries the generator's kid column, every father / mother its dad / mom column: the reads the writer lays down agree with them
    member = np.asarray([0] * n_kids + [1 + (i & 1) for i in range(n_par)])
    t.gt = np.ascontiguousarray(((base.gt[None, :] >> (2 * member[:, None])) & 3).astype(np.uint8))
    t.ref_depth = np.ascontiguousarray(base.rd[member].astype(np.int32))
    t.alt_depth = np.ascontiguousarray(base.ad[member].astype(np.int32))
    t.gq = np.ascontiguousarray(base.gq[member].astype(np.float64))
    t.pos = base.pos.astype(np.int32)
    t.end = t.pos + 1
    t.sflags = base.sflags.astype(np.uint8)
    t.ref_base, t.alt_base = base.ref_base.astype(np.uint8), base.alt_base.astype(np.uint8)
    t.contig_off = np.asarray(base.contig_off, np.int64)
    ped, dnms = {}, []
    for k in range(n_kids):
        kid, dad, mom = names[k], "p%04d" % (2 * (k // 3)), "p%04d" % (2 * (k // 3) + 1)
        ped[kid] = {"kid": kid, "dad": dad, "mom": mom, "sex": "2"}
        sel = np.arange(k, n_kids * n_snvs, n_kids)
        idx = all_dn.site_idx[sel]
        for row, gt, rd, ad in ((k, 1, 15, 15), (names.index(dad), 0, 30, 0), (names.index(mom), 0, 30, 0)):
            t.gt[row, idx], t.ref_depth[row, idx], t.alt_depth[row, idx], t.gq[row, idx] = gt, rd, ad, 99.0
        dn = DnmColumns(idx, all_dn.contig[sel], all_dn.start[sel], all_dn.end[sel], all_dn.kind[sel], all_dn.length[sel], all_dn.origin[sel],
                        [all_dn.refs[j] for j in sel], [all_dn.alts[j] for j in sel])
        cl = make_clusters(dn)
        cfg = bigsynth.make_cfg(seed=seed + 10 + k)
        cfg.n_clusters = cl.n
        bam = os.path.join(out_dir, kid + ".bam")
        bigsynth.write_bam(bam, cfg, base, dn, cl, contig_len=lens, level=1, threads=4)
        for j in range(n_snvs):
            dnms.append({"chrom": base.contig_names[int(dn.contig[j])], "start": int(dn.start[j]), "end": int(dn.end[j]), "kid": kid, "vartype": "POINT",
                         "bam": bam, "cram_ref": None})
    return t, ped, dnms


def digest(recs):
    return hashlib.sha256(json.dumps(recs, sort_keys=True, default=str).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kids", type=int, default=600)
    ap.add_argument("--snvs", type=int, default=48, help="SNV DNMs per kid")
    ap.add_argument("--sites", type=int, default=400_000)
    ap.add_argument("--runs", default="1700,3400,6800,0", help="UZ_COHORT_RUN_DNMS values of the cohort route; 0 = all kids in one run")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the BAMs go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_route_ab.json"))
    a = ap.parse_args()
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    tmp = a.dir or tempfile.mkdtemp(prefix="reads_route_ab_")
    os.makedirs(tmp, exist_ok=True)
    t0 = time.perf_counter()
    table, ped, dnms = make_cohort(a.kids, a.snvs, a.sites, tmp)
    print("[reads_route_ab] %d kids, %d DNMs, files in %.1f s" % (a.kids, len(dnms), time.perf_counter() - t0), file=sys.stderr, flush=True)
    session.register_sites("mem://reads_route_ab", table)
    settings = [("kid", None)] + [("cohort", int(x)) for x in a.runs.split(",") if x != ""]
    keys = ("bam_walks", "read_tables", "phase_cohort_calls")

    def one(route, limit):
        os.environ["UZ_READS_ROUTE"] = route
        if limit is None:
            os.environ.pop("UZ_COHORT_RUN_DNMS", None)
        else:
            os.environ["UZ_COHORT_RUN_DNMS"] = str(limit if limit > 0 else 1 << 30)
        session._HOSTS.clear()  # (a host of its own per call: its counters are the call's; the opened files stay)
        err = io.StringIO()
        t1 = time.perf_counter()
        with contextlib.redirect_stderr(err):
            recs = phase_snvs(copy.deepcopy(dnms), list(ped), ped, "mem://reads_route_ab", 2, "38", False, 10 ** 9, True, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8],
                              20, 10, 5000, 1000000, 3, 1, 151, 5)
        wall = time.perf_counter() - t1
        m = re.search(r"\breads ([0-9.]+) ", err.getvalue())
        stats = {}
        for h in session._HOSTS.values():
            for k in keys:
                stats[k] = stats.get(k, 0) + h.stats[k]
        return float(m.group(1)) if m else None, wall, stats, recs

    name = lambda route, limit: route if limit is None else "cohort_%s" % (limit if limit > 0 else "all")  # noqa: E731
    reads = {name(*s): [] for s in settings}
    walls = {name(*s): [] for s in settings}
    calls, shas, n_recs = {}, {}, {}
    for it in range(a.warmup + a.repeat):
        for s in settings:
            r, w, st, recs = one(*s)
            if it >= a.warmup:
                reads[name(*s)].append(r)
                walls[name(*s)].append(w)
            calls[name(*s)] = st
            if it == 0:
                shas[name(*s)] = digest({k: {f: v for f, v in rec.items()} for k, rec in recs.items()})
                n_recs[name(*s)] = len(recs)
            print("[reads_route_ab] pass %d %s: reads %.3f s, call %.3f s, %s" % (it, name(*s), r or -1.0, w, st), file=sys.stderr, flush=True)
    res = dict(what="wall time of the read side of ONE phase_snvs call over a cohort from files (one BAM + BAI per kid): the host path's `reads` section "
                    "(UZ_HOST_TRACE) and the whole call, by route of the read side (UZ_READS_ROUTE) and, for the cohort route, by DNMs per run "
                    "(UZ_COHORT_RUN_DNMS); one process, turn by turn",
               kids=a.kids, dnms=len(dnms), sites=a.sites, warmup=a.warmup, repeat=a.repeat, records=n_recs)
    for n in reads:
        res[n + "_reads_s"] = reads[n]
        res[n + "_reads_median_s"] = statistics.median(reads[n]) if reads[n] and None not in reads[n] else None
        res[n + "_call_s"] = walls[n]
        res[n + "_device_calls"] = calls[n]
        res[n + "_same_records_as_kid"] = shas[n] == shas["kid"]
    cohort = [n for n in reads if n != "kid"]
    res["cohort_beats_kid"] = {n: bool(reads[n]) and None not in reads[n] + reads["kid"] and max(reads[n]) < min(reads["kid"]) for n in cohort}
    res["nonempty"] = n_recs["kid"] > 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    return 0 if all(res[n + "_same_records_as_kid"] for n in reads) and res["nonempty"] else 1


if __name__ == "__main__":
    sys.exit(main())
