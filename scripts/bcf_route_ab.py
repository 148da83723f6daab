#!/usr/bin/env python
"""A/B of the two routes from a records dict to the annotated VCF of a BCF of DNMs (UZ_BCF_ROUTE):
  host    every record converted to its VCF line by unfazed_amd/bcf_text.py (a Python loop over the cells), then the host writer's loop over the cells
  device  the records' text written by k_bcfout_size / k_bcfout_fill (uz_bcf_rows), then rewritten by k_vcfout_size / k_vcfout_fill (uz_vcf_rows);
          the header and any handed-back record by the host
Every run is a FRESH process (this script started again with --child); the routes alternate, --repeat runs each, page cache warm (one untimed
pass over the file).  Timed in the child: wall and host CPU seconds (all threads) of unfazed.write_vcf_output from "records dict known" to
"output file written" -- the BCF's decode is inside on both routes; HIP start-up and library load are outside (the context is made before the
timer, on both routes).  No phasing is run: the records dict is made up, 48 DNMs a kid, in the smallest form summarize_record takes.
Shapes: `cohort` 600 samples x 20 000 records, `trio` 3 samples x 20 000 records; FORMAT GT:AD:DP:GQ:PL in int8 / int16.
The two routes' files must be byte-identical: asserted per shape.  Device runs also record the four kernel slots (uz_prof_get), the bytes that
went up (records, then text) and came down (text, twice), and the counters.
`device_beats_host`: every device run below every host run.  Unset stays the refusal whatever this says: the A/B decides only which value of the
switch README recommends.
    timeout -k 10 1100 python scripts/bcf_route_ab.py [--shape cohort|trio] [--repeat 3] [--dir D] [--gen-only] [--append] [--out profiles/bcf_route_ab.json]"""
import argparse
import hashlib
import json
import os
import random
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"cohort": (600, 20000), "trio": (3, 20000)}
DNMS_PER_KID = 48
DICT = ["PASS", "AC", "AN", "GT", "AD", "DP", "GQ", "PL"]


def dnm_cells(n_samples, n_records, seed=411):
    """(record, sample) of every DNM: 48 records a kid"""
    rng = random.Random(seed)
    return sorted((r, s) for s in range(n_samples) for r in rng.sample(range(n_records), DNMS_PER_KID))


def _block(data):
    comp = zlib.compressobj(1, zlib.DEFLATED, -15)
    cdata = comp.compress(data) + comp.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def generate(path, n_samples, n_records, seed=411):
    """a BGZF-framed BCF: hom-ref cells with depths and likelihoods, 0/1 at the DNM cells, some no-calls with every value missing"""
    rng = np.random.default_rng(seed + 1)
    names = ["kid%03d" % i for i in range(n_samples)]
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>', "##contig=<ID=chr1,IDX=0>", "##contig=<ID=chr2,IDX=1>"]
    lines += ['##INFO=<ID=%s,Number=1,Type=Integer,Description="x",IDX=%d>' % (k, DICT.index(k)) for k in ("AC", "AN")]
    lines += ['##FORMAT=<ID=%s,Number=.,Type=%s,Description="x",IDX=%d>' % (k, "String" if k == "GT" else "Integer", DICT.index(k)) for k in DICT[3:]]
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names))
    text = ("\n".join(lines) + "\n").encode() + b"\0"
    het = {}
    for r, s in dnm_cells(n_samples, n_records, seed):
        het.setdefault(r, []).append(s)
    key = lambda k, t, n: bytes([0x11, DICT.index(k), n << 4 | t])
    buf = bytearray(b"BCF\x02\x02" + struct.pack("<I", len(text)) + text)
    with open(path, "wb") as fh:
        for r in range(n_records):
            hs = np.asarray(het.get(r, ()), np.int64)
            nocall = rng.random(n_samples) < 0.02
            nocall[hs] = False
            gt = np.full((n_samples, 2), 2, np.int8)
            gt[hs, 1] = 4
            gt[nocall] = 0
            dp = rng.integers(18, 60, n_samples).astype(np.int16)
            ad = np.stack([dp, np.zeros(n_samples, np.int16)], 1)
            ad[hs] = np.stack([dp[hs] - dp[hs] // 2, dp[hs] // 2], 1)
            gq = rng.choice(np.asarray([60, 87, 99], np.int8), n_samples)
            pl = np.stack([np.zeros(n_samples, np.int16), 3 * dp, 45 * dp], 1).astype(np.int16)
            pl[hs] = np.asarray([812, 0, 790], np.int16)
            ad[nocall] = [-32768, -32767]
            dp[nocall] = -32768
            gq[nocall] = -128
            pl[nocall] = [-32768, -32767, -32767]
            indiv = (key("GT", 1, 2) + gt.tobytes() + key("AD", 2, 2) + ad.tobytes() + key("DP", 2, 1) + dp.tobytes() + key("GQ", 1, 1) + gq.tobytes()
                     + key("PL", 2, 3) + pl.tobytes())
            shared = struct.pack("<iiifII", int(r >= n_records // 2), 10000 + 37 * r - 1, 1, float(int(rng.integers(30, 900))), 2 << 16 | 2, 5 << 24 | n_samples)
            shared += bytes([0x07, 0x17, ord("ACGT"[r % 4]), 0x17, ord("CGTA"[r % 4]), 0x11, 0])
            shared += bytes([0x11, 1, 0x12]) + struct.pack("<h", len(hs)) + bytes([0x11, 2, 0x12]) + struct.pack("<h", 2 * n_samples)
            buf += struct.pack("<II", len(shared), len(indiv)) + shared + indiv
            while len(buf) >= 60000:
                fh.write(_block(bytes(buf[:60000])))
                del buf[:60000]
        if buf:
            fh.write(_block(bytes(buf)))
        fh.write(_block(b""))


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
    os.environ["UZ_BCF_ROUTE"] = a.child
    os.environ.pop("UZ_VCF_ROUTE", None)
    from unfazed_amd import engine, session, unfazed
    n_samples, n_records = SHAPES[a.shape]
    eng = session.get_backend()  # (HIP start-up, the library, the context: before the timer, on both routes)
    kernels = dict(k_bcfout_size=engine.K_BCFOUT_SIZE, k_bcfout_fill=engine.K_BCFOUT_FILL, k_vcfout_size=engine.K_VCFOUT_SIZE, k_vcfout_fill=engine.K_VCFOUT_FILL)
    eng.prof_enable(list(kernels.values()))
    moved = {}
    real_bcf, real_vcf = eng.bcf_rows, eng.vcf_rows

    def counted_bcf(view):
        res = real_bcf(view)
        moved["bcf_bytes_up"] = int(view.data_bytes) + 8 * int(view.n_records)
        moved["bcf_bytes_down"] = len(res[0]) + 21 * int(view.n_records)
        return res

    def counted_vcf(text, line_at, *ann):
        res = real_vcf(text, line_at, *ann)
        moved["vcf_bytes_up"] = int(text.text_bytes) + 32 * int(text.n_records) + 10 * len(ann[1])
        moved["vcf_bytes_down"] = len(res[0]) + 17 * int(text.n_records)
        return res
    eng.bcf_rows, eng.vcf_rows = counted_bcf, counted_vcf
    records = records_dict(n_samples, n_records)
    src, out = os.path.join(a.dir, "dnms_%s.bcf" % a.shape), os.path.join(a.dir, "out_%s_%s.vcf" % (a.shape, a.child))
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
               counters=dict(unfazed.BCF_STATS, **unfazed.VCF_STATS))
    if a.child == "device":
        run["kernel_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
        run.update(moved)
    os.remove(out)
    print("BCF_ROUTE_AB " + json.dumps(run), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cohort", choices=sorted(SHAPES))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--gen-only", action="store_true", help="write the file and stop (no device)")
    ap.add_argument("--append", action="store_true", help="add this call's runs to those --out already holds for the shape (a long shape measured in several calls)")
    ap.add_argument("--child", default=None, choices=["host", "device"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcf_route_ab.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    a.dir = a.dir or tempfile.mkdtemp(prefix="bcf_route_ab_")
    os.makedirs(a.dir, exist_ok=True)
    n_samples, n_records = SHAPES[a.shape]
    src = os.path.join(a.dir, "dnms_%s.bcf" % a.shape)
    t0 = time.perf_counter()
    if not os.path.exists(src):
        generate(src + ".part", n_samples, n_records)
        os.replace(src + ".part", src)
    print("[bcf_route_ab] file of shape %s (%d bytes) in %.1f s" % (a.shape, os.path.getsize(src), time.perf_counter() - t0), file=sys.stderr, flush=True)
    if a.gen_only:
        return 0
    with open(src, "rb") as fh:  # the page cache, warm for both routes
        while fh.read(1 << 24):
            pass
    runs = {"host": [], "device": []}
    if a.append and os.path.exists(a.out):
        held = json.load(open(a.out)).get(a.shape)
        if held:
            runs = {k: list(held["runs"][k]) for k in runs}
    for it in range(a.repeat):
        for route in ("host", "device"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--shape", a.shape, "--dir", a.dir]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:  # (a child that failed ends the measurement: nothing more is started)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            run = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("BCF_ROUTE_AB ")][-1][len("BCF_ROUTE_AB "):])
            runs[route].append(run)
            print("[bcf_route_ab] %s %s run %d: %.3f s wall, %.3f s host CPU" % (a.shape, route, it, run["wall_s"], run["host_cpu_s"]), file=sys.stderr, flush=True)
    same = len({r["sha"] for rr in runs.values() for r in rr}) == 1
    assert same, "the two routes' files differ (shape %s)" % a.shape
    beats = max(r["wall_s"] for r in runs["device"]) < min(r["wall_s"] for r in runs["host"])
    res = dict(what="records dict -> annotated VCF file of a BCF of DNMs, UZ_BCF_ROUTE=host (bcf_text.py, then the host writer) against device (uz_bcf_rows, then "
                    "uz_vcf_rows); a fresh process per run, routes alternating, page cache warm; wall and host CPU seconds of unfazed.write_vcf_output (the BCF's "
                    "decode inside), HIP start-up excluded",
               shape=a.shape, samples=n_samples, records=n_records, dnms_per_kid=DNMS_PER_KID, input_bytes=os.path.getsize(src), repeat=len(runs["host"]), runs=runs,
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
