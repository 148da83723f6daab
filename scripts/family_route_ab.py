#!/usr/bin/env python
"""A/B of the two routes that make a cohort's families: "all families ready on the device" timed for
  old   per trio: SitesTable.family_columns (numpy) + uz_family_upload (ten blocking copies)      -- run on the code of --parent-root
  new   once: SitesTable.sample_columns (uz_samples_pack) + uz_samples_upload, then ONE uz_families_from_samples -- run on this tree
over a synthetic decoder-shaped table ([ns][S]: u8 gt, int32 depths, f64 GQ), default 600 samples as 200 trios at 1.6 M sites.
Each run is a fresh child process under its own `timeout -k 10`; old and new alternate, --runs of each.  The new route's total includes
its one-time pack and upload.  The bar: every run of the new route beats every run of the old one (exit status 1 otherwise).
    python scripts/family_route_ab.py [--sites N] [--trios N] [--runs 3] [--parent-root DIR] [--out profiles/r09_family_route_ab.json]
A child that ends by a signal, an abort or its time limit ends the whole measurement: nothing more is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_ACHIEVABLE_TBS = 6.3  # MI355X: 8 TB/s spec, about 6.3 TB/s achievable by a streaming kernel


def make_table(n_sites, n_trios, seed=11):
    """decoder-shaped columns, cheap to make: a random block of 4096 sites per sample, tiled along the table (the routes' cost does not
    depend on the values; a few too-deep sites keep the wide list in play)"""
    import numpy as np
    sys.path.insert(0, os.getcwd())
    from unfazed_amd.model import SitesTable
    ns = 3 * n_trios
    rng = np.random.default_rng(seed)
    t = SitesTable(["s%04d" % i for i in range(ns)], ["1"])
    reps = (n_sites + 4095) // 4096

    def tiled(block, dtype):
        out = np.empty((ns, n_sites), dtype)
        for s in range(ns):
            out[s] = np.tile(block[s], reps)[:n_sites]
        return out
    t.gt = tiled(rng.integers(0, 4, (ns, 4096)).astype(np.uint8), np.uint8)
    t.ref_depth = tiled(rng.integers(-1, 60, (ns, 4096)).astype(np.int32), np.int32)
    t.alt_depth = tiled(rng.integers(-1, 60, (ns, 4096)).astype(np.int32), np.int32)
    t.gq = tiled(np.floor(rng.uniform(-1, 99, (ns, 4096)) * 4) / 4, np.float64)
    for k in range(min(16, n_sites)):
        t.ref_depth[(7 * k) % ns, (k * 104729) % n_sites] = 40000
    t.pos = np.arange(1, n_sites + 1, dtype=np.int32) * 50 % (1 << 30)
    t.pos.sort()
    t.end = t.pos + 1
    t.sflags = np.zeros(n_sites, np.uint8)
    t.sflags[:: 33] = 1
    t.ref_base = np.where(t.sflags == 0, ord("A"), 0).astype(np.uint8)
    t.alt_base = np.where(t.sflags == 0, ord("C"), 0).astype(np.uint8)
    t.contig_off = np.asarray([0, n_sites], np.int64)
    trios = [(t.samples[3 * k], t.samples[3 * k + 1], t.samples[3 * k + 2]) for k in range(n_trios)]
    return t, trios


def child(route, n_sites, n_trios):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    from unfazed_amd.engine import HipEngine
    t, trios = make_table(n_sites, n_trios)
    eng = HipEngine(0)
    sid = eng.upload_sites(t)
    eng.sync()
    res = dict(route=route, sites=n_sites, trios=n_trios, samples=len(t.samples))
    t0 = time.perf_counter()
    if route == "old":
        fams = []
        for tr in trios:
            gt, rd, ad, gq = t.family_columns(*tr)
            wide = getattr(t, "wide_depths", None)
            fams.append(eng.add_family(sid, gt, rd, ad, gq, wide=wide) if wide is not None else eng.add_family(sid, gt, rd, ad, gq))
        eng.sync()
        res["total_s"] = time.perf_counter() - t0
    else:
        from unfazed_amd.engine import K_FAMILY_PACK
        eng.prof_enable([K_FAMILY_PACK])
        names = [s for tr in trios for s in tr]
        cols = t.sample_columns(names, impl="native")
        t1 = time.perf_counter()
        mid = eng.upload_samples(sid, cols)
        row = {s: r for r, s in enumerate(names)}
        fams = eng.families_from_samples(mid, [row[tr[0]] for tr in trios], [row[tr[1]] for tr in trios], [row[tr[2]] for tr in trios])
        eng.sync()
        t2 = time.perf_counter()
        ms, launches = eng.prof_get(K_FAMILY_PACK)
        n_wide = 0 if cols.wide is None else int(cols.wide[0].size)
        up_bytes = sum(int(a.nbytes) for a in (cols.gt, cols.ref_depth, cols.alt_depth, cols.gq))
        k_bytes = n_trios * (5 * n_sites + 48 * n_wide)  # three gt rows + the site flags read, one byte written, per site and trio
        res.update(total_s=t2 - t0, pack_s=t1 - t0, upload_and_make_s=t2 - t1, upload_bytes=up_bytes,
                   upload_GBps=up_bytes / max(1e-9, (t2 - t1) - ms / 1e3) / 1e9, kernel_ms=ms, kernel_launch_sequences=launches, n_wide=n_wide,
                   kernel_bytes=k_bytes, kernel_TBps=(k_bytes / (ms / 1e3) / 1e12) if ms > 0 else None, hbm_achievable_TBps=HBM_ACHIEVABLE_TBS)
    res["per_trio_s"] = res["total_s"] / n_trios
    # the two routes made the same thing: the class bytes of the first and the last trio, as a digest
    import hashlib
    from unfazed_amd import abi
    P = abi.make_params()
    res["class_sha"] = hashlib.sha256(b"".join(eng.classify(fams[k], P, n_sites).tobytes() for k in (0, n_trios - 1))).hexdigest()[:16]
    eng.free_sites(sid)
    eng.close()
    print("AB_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=1_600_000)
    ap.add_argument("--trios", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-root", default=ROOT, help="a checkout of the parent commit, built: the old route runs on its code")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_family_route_ab.json"))
    ap.add_argument("--limit", type=int, default=0, help="seconds a child may take (default: sized by the table)")
    ap.add_argument("--child", choices=["old", "new"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.sites, a.trios)
    limit = a.limit or int(120 + a.trios * a.sites / 1.6e6 * 1.5)
    runs = {"old": [], "new": []}
    for k in range(a.runs):
        for route in ("old", "new"):
            root = a.parent_root if route == "old" else ROOT
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", route, "--sites", str(a.sites), "--trios", str(a.trios)]
            p = subprocess.run(cmd, cwd=root, capture_output=True, text=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("AB_RESULT ")]
            if p.returncode != 0 or not line:
                print("run %d of the %s route ended with status %d: stopping here\n%s" % (k, route, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                return 2
            r = json.loads(line[-1][len("AB_RESULT "):])
            runs[route].append(r)
            print("%s run %d: %.3f s total, %.4f s per trio" % (route, k, r["total_s"], r["per_trio_s"]), flush=True)
    old_t, new_t = [r["total_s"] for r in runs["old"]], [r["total_s"] for r in runs["new"]]
    bar = max(new_t) < min(old_t)
    same = len({r["class_sha"] for r in runs["old"] + runs["new"]}) == 1
    last = runs["new"][-1]
    out = dict(what="all families of a cohort ready on the device: per-trio family_columns + uz_family_upload (old, the parent's code) against "
                    "sample_columns + uz_samples_upload + one uz_families_from_samples (new); fresh process per run, alternating",
               sites=a.sites, trios=a.trios, samples=3 * a.trios, old_total_s=old_t, new_total_s=new_t,
               old_per_trio_s=[r["per_trio_s"] for r in runs["old"]], new_per_trio_s=[r["per_trio_s"] for r in runs["new"]],
               new_pack_s=[r["pack_s"] for r in runs["new"]], new_upload_and_make_s=[r["upload_and_make_s"] for r in runs["new"]],
               new_upload_GBps=[r["upload_GBps"] for r in runs["new"]], kernel_ms=[r["kernel_ms"] for r in runs["new"]],
               kernel_TBps=[r["kernel_TBps"] for r in runs["new"]], hbm_achievable_TBps=HBM_ACHIEVABLE_TBS, kernel_bytes=last["kernel_bytes"],
               pack_share_of_new_total=[r["pack_s"] / r["total_s"] for r in runs["new"]], n_wide=last["n_wide"],
               every_new_run_beats_every_old_run=bar, same_class_bytes_on_both_routes=same, parent_root_is_this_tree=os.path.samefile(a.parent_root, ROOT))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0 if (bar and same) else 1


if __name__ == "__main__":
    sys.exit(main())
