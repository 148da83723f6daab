#!/usr/bin/env python
"""A/B of the two routes from a records dict to the annotated VCF (UZ_VCF_ROUTE):
  host    write_vcf_output: io_vcf.read_vcf makes an object per cell, the writer splits, pads and formats every cell (the parent's code path)
  device  the DNM file decoded natively, one host loop over RECORDS for the annotations, the record lines rewritten by k_vcfout_size /
          k_vcfout_fill (uz_vcf_rows), the header and any handed-back record by the host
Every run is a FRESH process (this script started again with --child); the routes alternate, --repeat runs each, page cache warm (one untimed
pass over the file).  Timed in the child: wall and host CPU seconds (all threads) of unfazed.write_vcf_output from "records dict known" to
"output file written" -- the input file's decode is inside on both routes; HIP start-up and library load are outside (the context is made
before the timer).  No phasing is run: the records dict is made up, 48 DNMs a kid, in the smallest form summarize_record takes.
Shapes: `cohort` 600 samples x 20 000 records, `trio` 3 samples x 20 000 records.
The two routes' files must be byte-identical: asserted per shape.  Device runs also record k_vcfout_size / k_vcfout_fill (uz_prof_get), the bytes
that went up (text + records + annotations) and came down (text), and the counters.
`device_beats_host`: every device run below every host run -- in both shapes the rule UZ_VCF_ROUTE's default is changed by.
    timeout -k 10 1100 python scripts/vcf_route_ab.py [--shape cohort|trio] [--repeat 3] [--dir D] [--gen-only] [--out profiles/vcf_route_ab.json]"""
import argparse
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"cohort": (600, 20000), "trio": (3, 20000)}
DNMS_PER_KID = 48


def dnm_cells(n_samples, n_records, seed=411):
    """(record, sample) of every DNM: 48 records a kid"""
    rng = random.Random(seed)
    return sorted((r, s) for s in range(n_samples) for r in rng.sample(range(n_records), DNMS_PER_KID))


def generate(path, n_samples, n_records, seed=411):
    rng = random.Random(seed + 1)
    names = ["kid%03d" % i for i in range(n_samples)]
    pool = ["0/0:%d,0:%d:%d" % (d, d, q) for d in range(18, 60) for q in (60, 87, 99)] + ["./.", "0/0:31,0:31:99:0,93,1395"]
    het = {}
    for r, s in dnm_cells(n_samples, n_records, seed):
        het.setdefault(r, []).append(s)
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##contig=<ID=chr2>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for r in range(n_records):
            cells = rng.choices(pool, k=n_samples)
            for s in het.get(r, ()):
                d = rng.randrange(20, 60)
                cells[s] = "0/1:%d,%d:%d:99:812,0,790" % (d - d // 2, d // 2, d)
            fh.write("chr%d\t%d\t.\t%s\t%s\t%d\tPASS\tAC=%d;AN=%d\tGT:AD:DP:GQ:PL\t" % (1 + (r >= n_records // 2), 10000 + 37 * r, "ACGT"[r % 4], "CGTA"[r % 4],
                                                                                   rng.randrange(30, 900), len(het.get(r, ())), 2 * n_samples))
            fh.write("\t".join(cells))
            fh.write("\n")


def records_dict(n_samples, n_records, seed=411):
    rng = random.Random(seed + 2)
    out = {}
    for r, s in dnm_cells(n_samples, n_records, seed):
        chrom, start = "chr%d" % (1 + (r >= n_records // 2)), 10000 + 37 * r - 1
        kid = "kid%03d" % s
        nd, nm = rng.choice([(3, 0), (0, 2), (1, 1), (5, 0), (0, 0), (12, 1)])
        out["{}_{}_{}_{}_{}".format(chrom, start, start + 1, kid, "POINT")] = {
            "region": {"chrom": chrom, "start": start, "end": start + 1}, "vartype": "POINT", "kid": kid, "dad": "dad_" + kid, "mom": "mom_" + kid,
            "evidence_type": "READBACKED", "dad_reads": ["r%d" % i for i in range(nd)], "mom_reads": ["q%d" % i for i in range(nm)],
            "dad_sites": [str(start - 40 * (i + 1)) for i in range(nd)], "mom_sites": [str(start + 40 * (i + 1)) for i in range(nm)],
            "cnv_dad_sites": [], "cnv_mom_sites": []}
    return out


def child(a):
    """one run of one route in this (fresh) process -> a JSON line on stdout"""
    os.environ["UZ_VCF_ROUTE"] = a.child
    from unfazed_amd import engine, session, unfazed
    n_samples, n_records = SHAPES[a.shape]
    eng = session.get_backend()  # (HIP start-up, the library, the context: before the timer)
    kernels = dict(k_vcfout_size=engine.K_VCFOUT_SIZE, k_vcfout_fill=engine.K_VCFOUT_FILL)
    eng.prof_enable(list(kernels.values()))
    moved = {}
    real = eng.vcf_rows

    def counted(text, line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet):
        res = real(text, line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet)
        moved["bytes_up"] = int(text.text_bytes) + 32 * int(text.n_records) + 10 * len(ann_col)
        moved["bytes_down"] = len(res[0]) + 17 * int(text.n_records)
        return res
    eng.vcf_rows = counted
    records = records_dict(n_samples, n_records)
    src, out = os.path.join(a.dir, "dnms_%s.vcf" % a.shape), os.path.join(a.dir, "out_%s_%s.vcf" % (a.shape, a.child))
    w0, c0 = time.perf_counter(), time.process_time()
    unfazed.write_vcf_output(src, records, True, False, out, 10)
    wall, cpu = time.perf_counter() - w0, time.process_time() - c0
    h = hashlib.sha256()
    n_bytes = 0
    with open(out, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 24), b""):
            h.update(block)
            n_bytes += len(block)
    run = dict(wall_s=wall, host_cpu_s=cpu, cells=n_samples * n_records, cells_per_s=n_samples * n_records / wall, text_bytes=n_bytes, sha=h.hexdigest()[:16],
               counters=dict(unfazed.VCF_STATS))
    if a.child == "device":
        run["kernel_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
        run.update(moved)
    os.remove(out)
    print("VCF_ROUTE_AB " + json.dumps(run), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cohort", choices=sorted(SHAPES))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--gen-only", action="store_true", help="write the file and stop (no device)")
    ap.add_argument("--child", default=None, choices=["host", "device"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_route_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    a.dir = a.dir or tempfile.mkdtemp(prefix="vcf_route_ab_")
    os.makedirs(a.dir, exist_ok=True)
    n_samples, n_records = SHAPES[a.shape]
    src = os.path.join(a.dir, "dnms_%s.vcf" % a.shape)
    t0 = time.perf_counter()
    if not os.path.exists(src):
        generate(src + ".part", n_samples, n_records)
        os.replace(src + ".part", src)
    print("[vcf_route_ab] file of shape %s (%d bytes) in %.1f s" % (a.shape, os.path.getsize(src), time.perf_counter() - t0), file=sys.stderr, flush=True)
    if a.gen_only:
        return 0
    with open(src, "rb") as fh:  # the page cache, warm for both routes
        while fh.read(1 << 24):
            pass
    runs = {"host": [], "device": []}
    for it in range(a.repeat):
        for route in ("host", "device"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--shape", a.shape, "--dir", a.dir]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:  # (a child that failed ends the measurement: nothing more is started)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            run = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("VCF_ROUTE_AB ")][-1][len("VCF_ROUTE_AB "):])
            runs[route].append(run)
            print("[vcf_route_ab] %s %s run %d: %.3f s wall, %.3f s host CPU" % (a.shape, route, it, run["wall_s"], run["host_cpu_s"]), file=sys.stderr, flush=True)
    same = len({r["sha"] for rr in runs.values() for r in rr}) == 1
    assert same, "the two routes' files differ (shape %s)" % a.shape
    beats = max(r["wall_s"] for r in runs["device"]) < min(r["wall_s"] for r in runs["host"])
    res = dict(what="records dict -> annotated VCF file, UZ_VCF_ROUTE=host (the parent's code path) against device; a fresh process per run, routes alternating, "
                    "page cache warm; wall and host CPU seconds of unfazed.write_vcf_output (the input file's decode inside), HIP start-up excluded",
               shape=a.shape, samples=n_samples, records=n_records, dnms_per_kid=DNMS_PER_KID, input_bytes=os.path.getsize(src), repeat=a.repeat, runs=runs,
               same_file_on_both_routes=same, device_beats_host=beats,
               host_median_wall_s=statistics.median(r["wall_s"] for r in runs["host"]), device_median_wall_s=statistics.median(r["wall_s"] for r in runs["device"]),
               host_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["host"]), device_median_cpu_s=statistics.median(r["host_cpu_s"] for r in runs["device"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
    allres[a.shape] = res
    json.dump(allres, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
