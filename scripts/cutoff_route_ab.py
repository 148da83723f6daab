#!/usr/bin/env python
"""A/B of the two routes to the insert cutoffs of a cohort call's kids (UZ_CUTOFF_ROUTE; read_collector.py:11-25):
  host    every file's first insert_size_max_sample + 1 records are read when its source is opened -- one host thread, one file at a time,
          inflating block after block (csrc/io_stage.cpp open_source) -- and numpy takes the percentile of the column: the parent's code path
  device  the sources are opened without a head; the heads of all files are gathered, inflated, walked and ranked on the device
          (PhasingHost.prepare_cutoffs -> HipEngine.head_ranks: uz_head_walk, uz_head_rank), the percentile's arithmetic stays on the host
Timed: wall and host CPU seconds (all threads of the process) from "files known" to "every kid's cutoff known", through the product's own code
(session._LazyReads, PhasingHost.prepare_cutoffs, PhasingHost.kid_cutoff); nothing of an earlier run is kept but the page cache, which one
untimed pass over every file warms for both.  One process, the routes turn by turn, --repeat runs each.  The device runs also record the kernel
times of the inflate (+ CRC-32), k_head_walk and k_head_rank (uz_prof_get).
Input: synth/bigsynth.py's writer.  --distinct files are generated, each with at least --records records, and stand under --files names (copies
of one file are different files to both routes; what they share is the page cache, which is warm anyway).
Shapes of profiles/cutoff_route_ab.json:
  (a) --files 600 --records 100001 --sample 100000     the cohort's file count
  (b) --files 16 --records 1000001 --sample 1000000    the default head length
    timeout -k 10 1100 python scripts/cutoff_route_ab.py --shape a [--files 600] [--records 100001] [--sample 100000] [--distinct 6] [--repeat 3] [--out profiles/cutoff_route_ab.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_file(path, min_records, seed):
    """one BAM + BAI of at least min_records records: the read pile-ups of as many DNMs as that takes -> its record count"""
    from synth import bigsynth
    from synth.sites_np import make_clusters, make_sites, place_dnms_full
    lens = [200_000_000]
    base = make_sites(400_000, seed=seed, contig_lens=lens, complex_frac=0.0, weird_frac=0.0)
    n_dnms, got = 64, 0
    while True:
        dn = place_dnms_full(base, n_dnms, seed=seed + 1, indel_frac=0.0)
        cl = make_clusters(dn)
        cfg = bigsynth.make_cfg(seed=seed + 2)
        cfg.n_clusters = cl.n
        got = bigsynth.write_bam(path, cfg, base, dn, cl, contig_len=lens, level=1, threads=8)["records"]
        if got >= min_records:
            return got
        n_dnms = int(n_dnms * min_records / max(got, 1) * 1.15) + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="a", help="the key of this run in the output file")
    ap.add_argument("--files", type=int, default=600)
    ap.add_argument("--records", type=int, default=100_001, help="records per file, at least")
    ap.add_argument("--sample", type=int, default=100_000, help="insert_size_max_sample")
    ap.add_argument("--distinct", type=int, default=6, help="files generated; the others are copies under their own names")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--readlen", type=int, default=151)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--gen-only", action="store_true", help="write the files and stop (no device)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cutoff_route_ab.json"))
    a = ap.parse_args()
    tmp = a.dir or tempfile.mkdtemp(prefix="cutoff_route_ab_")
    os.makedirs(tmp, exist_ok=True)
    t0 = time.perf_counter()
    made, paths = [], []
    for d in range(min(a.distinct, a.files)):
        p = os.path.join(tmp, "gen%03d.bam" % d)
        made.append((p, make_file(p, a.records, 700 + 10 * d)))
    for f in range(a.files):
        src = made[f % len(made)][0]
        p = os.path.join(tmp, "kid%04d.bam" % f)
        shutil.copyfile(src, p)
        shutil.copyfile(src + ".bai", p + ".bai")
        paths.append(p)
    file_bytes = sum(os.path.getsize(p) for p in paths)
    print("[cutoff_route_ab] %d files (%d distinct, %s records), %.1f MB, written in %.1f s" %
          (a.files, len(made), [m[1] for m in made], file_bytes / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)
    if a.gen_only:
        return 0
    for p in paths:  # the page cache, warm for both routes
        with open(p, "rb") as fh:
            while fh.read(1 << 24):
                pass

    import numpy as np
    from unfazed_amd import engine, hostpath, session
    from unfazed_amd.hostpath import PhasingHost, _Stats
    eng = engine.HipEngine(0)
    kernels = dict(inflate_crc=engine.K_HEAD_INFLATE, k_head_walk=engine.K_HEAD_WALK, k_head_rank=engine.K_HEAD_RANK)
    eng.prof_enable(list(kernels.values()))
    batch = [("kid%04d" % f, p) for f, p in enumerate(paths)]

    def one(route):
        os.environ["UZ_CUTOFF_ROUTE"] = route
        session._STAGERS.clear()
        hostpath._CUTOFF_RANKS.clear()
        eng.prof_reset()
        h = PhasingHost.__new__(PhasingHost)  # what prepare_cutoffs and kid_cutoff read of a host, and no sites table
        h.backend, h.cutoffs, h.stats, h._indexed_memo = eng, {}, _Stats(), None
        h.reads_by_bam = session._LazyReads(a.sample)
        w0, c0 = time.perf_counter(), time.process_time()
        h.prepare_cutoffs(batch, a.readlen, 3, a.sample)
        cut = [h.kid_cutoff(kid, bam, a.readlen, 3, a.sample) for kid, bam in batch]
        run = dict(wall_s=time.perf_counter() - w0, host_cpu_s=time.process_time() - c0,
                   counters={k: h.stats[k] for k in ("cutoff_device_files", "cutoff_host_files", "cutoff_walk_calls")})
        if route == "device":
            run["kernel_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
        return run, np.asarray(cut, np.float64)

    runs = {"host": [], "device": []}
    cuts = {}
    for it in range(a.repeat):
        for route in ("host", "device"):
            run, cut = one(route)
            runs[route].append(run)
            cuts.setdefault(route, cut)
            assert cuts[route].tobytes() == cut.tobytes()
            print("[cutoff_route_ab] %s run %d: %.3f s wall, %.3f s host CPU" % (route, it, run["wall_s"], run["host_cpu_s"]), file=sys.stderr, flush=True)
    eng.close()
    res = dict(what="wall and host CPU seconds from 'files known' to 'every kid's cutoff known', UZ_CUTOFF_ROUTE=host (the parent's code path) against "
                    "device; one process, turn by turn, page cache warm",
               files=a.files, distinct_files=len(made), head_max_bytes=int(os.environ.get("UZ_HEAD_MAX_BYTES", engine.HEAD_MAX_BYTES)), records_per_distinct_file=[m[1] for m in made], insert_size_max_sample=a.sample, file_bytes=file_bytes,
               repeat=a.repeat, runs=runs, same_cutoffs_on_both_routes=cuts["host"].tobytes() == cuts["device"].tobytes(),
               host_median_wall_s=statistics.median(r["wall_s"] for r in runs["host"]),
               device_median_wall_s=statistics.median(r["wall_s"] for r in runs["device"]),
               host_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["host"]),
               device_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["device"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
    allres[a.shape] = res
    json.dump(allres, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    if not a.dir:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0 if res["same_cutoffs_on_both_routes"] else 1


if __name__ == "__main__":
    sys.exit(main())
