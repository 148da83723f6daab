#!/usr/bin/env python
"""A/B of the two routes from files to BED text (UZ_BED_ROUTE):
  host    phase_snvs builds the records dict -- vote lists fetched, every read name and position a Python str -- and summarize.bed_lines
          walks it (the parent's code path)
  device  phase_snvs_bed: every device result's lines are written by k_bed_size / k_bed_fill from the result where it lies (uz_bed_rows)
Every run is a FRESH process (this script started again with --child); the routes alternate, --repeat runs each, verbose and not, page cache
warm (one untimed pass over the files).  Timed in the child: wall and host CPU seconds (all threads) of the driver's own function from
"arguments parsed" to "text written", HIP start-up and library load excluded (a first empty context is made before the timer).
Shapes:
  one     ONE kid, --dnms point DNMs (default 20 000) from synth/bigsynth.py's files -- BAM + BAI, BGZF sites VCF + TBI, ped, DNM BED -- through
          unfazed_amd.unfazed.unfazed(args), what `python -m unfazed_amd` calls: the chunked route
  cohort  --kids kids x 48 DNMs, one BAM + BAI per kid, the sample table built in memory in every child (the generator writes no multi-sample
          VCF), through the two calls the driver makes of it: phase_snvs + write_bed_output against phase_snvs_bed + BedRows.write
The two routes' texts must be byte-identical: asserted per shape and mode.  Device runs also record k_bed_size / k_bed_fill (uz_prof_get), the
bytes of text, and the time of a device-to-host copy of as many bytes into page-locked memory (HIP events, median of five).
`device_beats_host`: every device run below every host run -- in every shape and mode the rule UZ_BED_ROUTE's default is changed by.
    timeout -k 10 1100 python scripts/bed_route_ab.py [--shape one|cohort] [--dnms 20000] [--kids 100] [--repeat 3] [--dir D] [--gen-only] [--out profiles/bed_route_ab.json]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARGV = (2, "38", False, 10 ** 9, True, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10, 5000, 1000000, 3, 1, 151, 5)


def gen_one(d, n_dnms, seed=311):
    """one kid's files -> nothing (they lie in d)"""
    from synth import bigsynth
    from synth.sites_np import make_clusters, make_sites, place_dnms_full
    lens = [200_000_000]
    sc = make_sites(20 * n_dnms, seed=seed, contig_lens=lens, complex_frac=0.0, weird_frac=0.0)
    dn = place_dnms_full(sc, n_dnms, seed=seed + 1, indel_frac=0.0)
    cl = make_clusters(dn)
    cfg = bigsynth.make_cfg(seed=seed + 2)
    cfg.n_clusters = cl.n
    bigsynth.write_bam(os.path.join(d, "kid.bam"), cfg, sc, dn, cl, contig_len=lens, level=1, threads=8)
    bigsynth.write_vcf(os.path.join(d, "sites.vcf.gz"), sc, contig_len=lens, level=1, threads=8)
    with open(os.path.join(d, "kid.ped"), "w") as fh:
        fh.write("fam\tkid\tdad\tmom\t2\t2\n")
    with open(os.path.join(d, "dnms.bed"), "w") as fh:
        for j in range(n_dnms):
            fh.write("%s\t%d\t%d\tkid\tPOINT\n" % (sc.contig_names[int(dn.contig[j])], int(dn.start[j]), int(dn.end[j])))


def cohort(d, n_kids, write_bams):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    keep = {k: os.environ.get(k) for k in ("UZ_HOST_TRACE", "UZ_HOST_CHUNKS")}
    import reads_route_ab  # (its generator; the two switches it sets at import are put back)
    for k, v in keep.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if not write_bams:
        from synth import bigsynth
        real, bigsynth.write_bam = bigsynth.write_bam, lambda *a, **k: None  # the files lie there already: only the table is rebuilt
        try:
            return reads_route_ab.make_cohort(n_kids, 48, 400_000, d)
        finally:
            bigsynth.write_bam = real
    return reads_route_ab.make_cohort(n_kids, 48, 400_000, d)


def d2h_copy_ms(n_bytes):
    """a device-to-host copy of n_bytes into page-locked memory, HIP events around it: the median of five after a first one (the runtime the
    library has loaded, through ctypes)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    dev, host, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()

    def ck(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed: %d" % rc)
    ck(hip.hipMalloc(C.byref(dev), C.c_size_t(n_bytes)))
    ck(hip.hipHostMalloc(C.byref(host), C.c_size_t(n_bytes), C.c_uint(0)))
    ck(hip.hipEventCreate(C.byref(e0)))
    ck(hip.hipEventCreate(C.byref(e1)))
    out = []
    for _ in range(6):
        ck(hip.hipEventRecord(e0, None))
        ck(hip.hipMemcpyAsync(host, dev, C.c_size_t(n_bytes), C.c_int(2), None))  # hipMemcpyDeviceToHost
        ck(hip.hipEventRecord(e1, None))
        ck(hip.hipEventSynchronize(e1))
        ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        out.append(ms.value)
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1), hip.hipFree(dev), hip.hipHostFree(host)
    return statistics.median(out[1:])


def child(a):
    """one run of one route in this (fresh) process -> a JSON line on stdout"""
    os.environ["UZ_BED_ROUTE"] = a.child
    from unfazed_amd import engine, session, summarize
    eng = session.get_backend()  # (HIP start-up, the library, the context: before the timer)
    kernels = dict(k_bed_size=engine.K_BED_SIZE, k_bed_fill=engine.K_BED_FILL)
    eng.prof_enable(list(kernels.values()))
    out = os.path.join(a.dir, "out_%s_%d.bed" % (a.child, int(a.verbose)))
    if a.shape == "one":
        from unfazed_amd.__main__ import setup_args
        from unfazed_amd.unfazed import unfazed
        argv = ["-d", os.path.join(a.dir, "dnms.bed"), "-s", os.path.join(a.dir, "sites.vcf.gz"), "-p", os.path.join(a.dir, "kid.ped"), "--build", "38", "-t", "2", "-q",
                "-o", "bed", "--outfile", out, "--bam-pairs", "kid:" + os.path.join(a.dir, "kid.bam")] + (["--verbose"] if a.verbose else [])
        w0, c0 = time.perf_counter(), time.process_time()
        unfazed(setup_args().parse_args(argv))
        n = a.dnms
    else:
        from unfazed_amd.snv_phaser import phase_snvs, phase_snvs_bed
        table, ped, dnms = cohort(a.dir, a.kids, write_bams=False)
        session.register_sites("mem://bed_route_ab", table)
        w0, c0 = time.perf_counter(), time.process_time()
        if a.child == "device":
            phase_snvs_bed(dnms, list(ped), ped, "mem://bed_route_ab", *ARGV, include_ambiguous=False, verbose=a.verbose).write(out)
        else:
            summarize.write_bed_output(phase_snvs(dnms, list(ped), ped, "mem://bed_route_ab", *ARGV), False, a.verbose, out, 10)
        n = len(dnms)
    wall, cpu = time.perf_counter() - w0, time.process_time() - c0
    text = open(out, "rb").read()
    run = dict(wall_s=wall, host_cpu_s=cpu, dnms=n, dnms_per_s=n / wall, text_bytes=len(text), lines=text.count(b"\n"), sha=hashlib.sha256(text).hexdigest()[:16])
    if a.child == "device":
        run["kernel_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
        stats = {}
        for h in session._HOSTS.values():
            for k in ("bed_device_rows", "bed_host_rows", "bed_calls"):
                stats[k] = stats.get(k, 0) + h.stats[k]
        run["counters"] = stats
        run["d2h_copy_of_the_text_ms"] = d2h_copy_ms(max(1, len(text)))
    print("BED_ROUTE_AB " + json.dumps(run), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="one", choices=["one", "cohort"])
    ap.add_argument("--dnms", type=int, default=20000)
    ap.add_argument("--kids", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--gen-only", action="store_true", help="write the files and stop (no device)")
    ap.add_argument("--child", default=None, choices=["host", "device"])
    ap.add_argument("--verbose", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bed_route_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    a.dir = a.dir or tempfile.mkdtemp(prefix="bed_route_ab_")
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    marker = os.path.join(a.dir, "generated_%s" % a.shape)
    if not os.path.exists(marker):
        gen_one(a.dir, a.dnms) if a.shape == "one" else cohort(a.dir, a.kids, write_bams=True)
        open(marker, "w").write("ok\n")
    print("[bed_route_ab] files of shape %s in %.1f s" % (a.shape, time.perf_counter() - t0), file=sys.stderr, flush=True)
    if a.gen_only:
        return 0
    for fn in os.listdir(a.dir):  # the page cache, warm for both routes
        with open(os.path.join(a.dir, fn), "rb") as fh:
            while fh.read(1 << 24):
                pass
    res = dict(what="files -> BED text, UZ_BED_ROUTE=host (the parent's code path) against device; a fresh process per run, routes alternating, page cache warm; "
                    "wall and host CPU seconds of the driver's own function, HIP start-up excluded",
               shape=a.shape, repeat=a.repeat, modes={})
    ok = True
    for verbose in (0, 1):
        runs = {"host": [], "device": []}
        for it in range(a.repeat):
            for route in ("host", "device"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--shape", a.shape, "--dnms", str(a.dnms), "--kids", str(a.kids), "--dir", a.dir,
                       "--verbose", str(verbose)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:  # (a child that failed ends the measurement: nothing more is started)
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    return 1
                run = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("BED_ROUTE_AB ")][-1][len("BED_ROUTE_AB "):])
                runs[route].append(run)
                print("[bed_route_ab] %s verbose=%d %s run %d: %.3f s wall, %.3f s host CPU, %.0f DNMs/s" %
                      (a.shape, verbose, route, it, run["wall_s"], run["host_cpu_s"], run["dnms_per_s"]), file=sys.stderr, flush=True)
        same = len({r["sha"] for rr in runs.values() for r in rr}) == 1
        assert same, "the two routes' texts differ (shape %s, verbose %d)" % (a.shape, verbose)
        beats = max(r["wall_s"] for r in runs["device"]) < min(r["wall_s"] for r in runs["host"])
        ok = ok and beats
        res["modes"]["verbose" if verbose else "plain"] = dict(
            runs=runs, same_text_on_both_routes=same, device_beats_host=beats,
            host_median_wall_s=statistics.median(r["wall_s"] for r in runs["host"]), device_median_wall_s=statistics.median(r["wall_s"] for r in runs["device"]),
            host_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["host"]), device_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["device"]))
    res["device_beats_host"] = ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
    allres[a.shape] = res
    json.dump(allres, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "modes"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
