#!/usr/bin/env python
"""A/B of the two routes of the host path's site stage over a cohort batch (PhasingHost._cohort_route):
  kid     one uz_find / one uz_phase_cnv per kid -- the code before the cohort calls, reached by UZ_FIND_ROUTE=kid
  cohort  ONE uz_find_cohort / ONE uz_phase_cnv_cohort over all kids
Workload: a synthetic sample table (default 100 k sites; --kids 600 kids in sibships of three, 1 000 samples), 48 SNV DNMs per kid for
`find` as run_read_phasing calls it (lists only, the site dicts deferred) and 2 DEL / DUP per kid for `run_cnv_phasing` as phase_svs calls
it (annotate off).  Both routes run in ONE process on one table, turn by turn: --warmup calls of each, then --repeat timed calls of each;
every timed call starts from stale classes (uz_drop_derived), so the site scan of 600 families is part of both.  Reported: the median
wall time per route and stage, the device calls per route (PhasingHost.stats), and whether both routes left the same lists / records.
Exit status 1 when the cohort route's median is above the per-kid route's in either stage.
    timeout -k 10 900 python scripts/find_route_ab.py [--kids 600] [--sites 100000] [--warmup 2] [--repeat 5] [--out profiles/find_route_ab.json]"""
import argparse
import copy
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_table(n_sites, n_kids, seed=23):
    """decoder-shaped columns, cheap to make: a random block of 4096 sites per sample, tiled along the table"""
    import numpy as np
    from unfazed_amd.model import SitesTable
    n_par = 2 * ((n_kids + 2) // 3)
    names = ["k%04d" % i for i in range(n_kids)] + ["p%04d" % i for i in range(n_par)]
    ns = len(names)
    rng = np.random.default_rng(seed)
    t = SitesTable(names, ["1"])
    reps = (n_sites + 4095) // 4096

    def tiled(block, dtype):
        out = np.empty((ns, n_sites), dtype)
        for s in range(ns):
            out[s] = np.tile(block[s], reps)[:n_sites]
        return out
    t.gt = tiled(rng.choice(np.asarray([0, 1, 1, 3], np.uint8), (ns, 4096)), np.uint8)
    t.ref_depth = tiled(rng.integers(8, 40, (ns, 4096)).astype(np.int32), np.int32)
    t.alt_depth = tiled(rng.integers(8, 40, (ns, 4096)).astype(np.int32), np.int32)
    hom_ref, hom_alt = t.gt == 0, t.gt == 3
    t.alt_depth[hom_ref] //= 16
    t.ref_depth[hom_alt] //= 16
    t.gq = tiled(np.floor(rng.uniform(15, 99, (ns, 4096))), np.float64)
    t.pos = np.sort(rng.integers(1, 30 * n_sites, n_sites)).astype(np.int32)
    t.end = t.pos + 1
    t.sflags = np.zeros(n_sites, np.uint8)
    t.sflags[::33] = 1
    t.ref_base = np.where(t.sflags == 0, ord("A"), 0).astype(np.uint8)
    t.alt_base = np.where(t.sflags == 0, ord("C"), 0).astype(np.uint8)
    t.contig_off = np.asarray([0, n_sites], np.int64)
    ped = {}
    for k in range(n_kids):
        kid = names[k]
        ped[kid] = {"kid": kid, "dad": "p%04d" % (2 * (k // 3)), "mom": "p%04d" % (2 * (k // 3) + 1), "sex": "2"}
    return t, ped, rng


def digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, default=lambda a: a.tolist()).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kids", type=int, default=600)
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--snvs", type=int, default=48, help="SNV DNMs per kid")
    ap.add_argument("--cnvs", type=int, default=2, help="DEL / DUP per kid")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_route_ab.json"))
    a = ap.parse_args()
    from unfazed_amd import abi
    from unfazed_amd.engine import HipEngine
    from unfazed_amd.hostpath import PhasingHost
    t, ped, rng = make_table(a.sites, a.kids)
    span = int(t.pos[-1])
    snvs, cnvs = [], []
    for kid in list(ped):
        for p in rng.integers(10_000, span - 10_000, a.snvs).tolist():
            snvs.append({"chrom": "1", "start": p, "end": p + 1, "kid": kid, "vartype": "POINT", "bam": "", "cram_ref": None})
        for j, p in enumerate(rng.integers(10_000, span - 30_000, a.cnvs).tolist()):
            cnvs.append({"chrom": "1", "start": p, "end": p + int(rng.integers(2_000, 20_000)), "kid": kid, "vartype": ("DEL", "DUP")[j % 2], "bam": "", "cram_ref": None})
    eng = HipEngine(0)
    host = PhasingHost(eng, t, {})
    P = abi.make_params()
    host.prepare_families((k, ped[k]["dad"], ped[k]["mom"]) for k in ped)
    big = 1 << 30  # multithread_proc_min: the per-DNM `find`, not find_many

    def run_find():
        _, info = host.find(copy.deepcopy(snvs), ped, 5000, 1, "38", big, True, P, whole_region=False, defer_attach=True)
        return info["found"]

    def run_cnv():
        return host.run_cnv_phasing(copy.deepcopy(cnvs), ped, 1, "38", big, True, P, annotate=False)

    times = {(s, r): [] for s in ("find", "cnv") for r in ("kid", "cohort")}
    calls, shas = {}, {}
    for it in range(a.warmup + a.repeat):
        for route in ("kid", "cohort"):
            os.environ["UZ_FIND_ROUTE"] = route
            for stage, fn in (("find", run_find), ("cnv", run_cnv)):
                eng.drop_derived()
                eng.sync()
                keys = ("find_cohort_calls", "find_kid_calls", "cnv_cohort_calls", "cnv_kid_calls")
                before = {k: host.stats[k] for k in keys}
                t0 = time.perf_counter()
                out = fn()
                dt = time.perf_counter() - t0
                if it >= a.warmup:
                    times[(stage, route)].append(dt)
                calls[(stage, route)] = {k: host.stats[k] - before[k] for k in keys}
                if it == 0:
                    shas[(stage, route)] = digest({str(k): v for k, v in out.items()})
    res = dict(what="wall time of PhasingHost.find (SNV windows, lists only) and run_cnv_phasing (annotate off) over one cohort batch: one device call "
                    "per kid (UZ_FIND_ROUTE=kid, the code before the cohort calls) against one call for all kids; one process, turn by turn, every "
                    "timed call from stale site classes",
               kids=a.kids, samples=len(t.samples), sites=a.sites, snv_dnms=len(snvs), cnv_events=len(cnvs), warmup=a.warmup, repeat=a.repeat)
    ok = True
    for stage in ("find", "cnv"):
        for route in ("kid", "cohort"):
            res["%s_%s_s" % (stage, route)] = times[(stage, route)]
            res["%s_%s_median_s" % (stage, route)] = statistics.median(times[(stage, route)])
            res["%s_%s_calls" % (stage, route)] = calls[(stage, route)]
        res["%s_same_result_on_both_routes" % stage] = shas[(stage, "kid")] == shas[(stage, "cohort")]
        res["%s_speedup" % stage] = res["%s_kid_median_s" % stage] / res["%s_cohort_median_s" % stage]
        ok = ok and res["%s_same_result_on_both_routes" % stage] and res["%s_cohort_median_s" % stage] <= res["%s_kid_median_s" % stage]
    res["cohort_route_not_slower"] = ok
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
