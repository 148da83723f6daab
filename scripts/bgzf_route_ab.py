#!/usr/bin/env python
"""A/B of the four ways the annotated VCF reaches a file called out.vcf.gz (UZ_OUT_BGZF, UZ_OUT_BGZF_CODE):
  unset   plain text under the ".gz" name (what the driver did before the switch)
  host    BGZF by zlib, one block per 65 280 bytes, UZ_OUT_BGZF_LEVEL (6)
  device  the same blocks by k_bgzf_deflate / k_bgzf_frame (uz_bgzf_deflate)
  device-dynamic  the device route with UZ_OUT_BGZF_CODE=dynamic: k_bgzf_deflate_dyn in k_bgzf_deflate's place (uz_bgzf_deflate_coded)
The protocol of scripts/vcf_route_ab.py, whose generator and records dict this script uses: one MI355X, every run a FRESH process (this script
started again with --child), the routes alternating, --repeat runs each, page cache warm.  Timed in the child: wall and host CPU seconds of
unfazed.write_vcf_output from "records dict known" to "output file written"; the annotated text itself comes from the device route of
UZ_VCF_ROUTE on all three; HIP start-up and library load are outside (the context is made before the timer).
Shapes: `cohort` 600 samples x 20 000 records, `trio` 3 samples x 20 000 records.
The four files must hold the same text (the BGZF ones inflated by gzip): asserted per shape.  Device runs also record, outside the timer,
kernel_ms of their code's kernel over the whole text (repeat=3), the profile slots of the timed call, and the kernel's distance from one copy of
its input plus its output at the 6.3 TB/s a copy reaches on the box; a device-dynamic run records kernel_ms of both kernels, same process,
alternating (fixed, dynamic, fixed, dynamic), and the split of its blocks.  It decides no default: unset stays unset.
(profiles/bgzf_route_ab.json is the three-leg measurement from before the fourth leg.)
The index leg (--index; UZ_OUT_INDEX=tbi): under the same rules the routes are device / device-index / host / host-index, "files written" includes
the .tbi, the data file of a route must be the same bytes with and without the index (asserted), and a device-index run records the profile
slots of the index kernels (UZ_K_TBX_KEYS: mark + scan + starts + keys per chunk; UZ_K_TBX_TABLE: the passes behind the last chunk), the
rows the host settled and the .tbi's size.  It writes profiles/tbx_route_ab.json.
    timeout -k 10 1100 python scripts/bgzf_route_ab.py [--shape cohort|trio] [--repeat 3] [--dir D] [--out profiles/bgzf_dynamic_ab.json] [--index]"""
import argparse
import gzip
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcf_route_ab as shape  # noqa: E402 -- the generator, the records dict, the shapes

ROUTES = ("unset", "host", "device", "device-dynamic")
INDEX_ROUTES = ("device", "device-index", "host", "host-index")
COPY_BYTES_PER_S = 6.3e12


def child(a):
    """one run of one route in this (fresh) process -> a JSON line on stdout"""
    os.environ.pop("UZ_OUT_BGZF", None)
    os.environ.pop("UZ_OUT_BGZF_CODE", None)
    os.environ.pop("UZ_OUT_INDEX", None)
    if a.child.endswith("-index"):
        os.environ["UZ_OUT_INDEX"] = "tbi"
    if a.child != "unset":
        os.environ["UZ_OUT_BGZF"] = a.child.split("-")[0]
    if a.child == "device-dynamic":
        os.environ["UZ_OUT_BGZF_CODE"] = "dynamic"
    from unfazed_amd import engine, outfile, session, unfazed
    n_samples, n_records = shape.SHAPES[a.shape]
    eng = session.get_backend()  # (HIP start-up, the library, the context: before the timer)
    kernels = dict(k_bgzf_deflate=engine.K_DEFLATE, k_bgzf_frame=engine.K_DEFLATE_FRAME)
    if a.child.endswith("-index"):
        kernels.update(k_tbx_keys=engine.K_TBX_KEYS, k_tbx_table=engine.K_TBX_TABLE)
    eng.prof_enable(list(kernels.values()))
    records = shape.records_dict(n_samples, n_records)
    src, out = os.path.join(a.dir, "dnms_%s.vcf" % a.shape), os.path.join(a.dir, "out_%s_%s.vcf.gz" % (a.shape, a.child))
    w0, c0 = time.perf_counter(), time.process_time()
    unfazed.write_vcf_output(src, records, True, False, out, 10)
    wall, cpu = time.perf_counter() - w0, time.process_time() - c0
    raw = open(out, "rb").read()
    text = raw if a.child == "unset" else gzip.decompress(raw)
    run = dict(wall_s=wall, host_cpu_s=cpu, file_bytes=len(raw), text_bytes=len(text), text_sha=hashlib.sha256(text).hexdigest()[:16],
               file_sha=hashlib.sha256(raw).hexdigest()[:16], counters=dict(outfile.OUT_STATS), vcf_counters=dict(unfazed.VCF_STATS))
    if a.child.endswith("-index"):
        run["tbi_bytes"] = os.path.getsize(out + ".tbi")  # (a text that got no index ends the measurement here)
        os.remove(out + ".tbi")
    if a.child == "device-index":
        run["prof_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
    elif a.child.startswith("device"):
        code = "dynamic" if a.child == "device-dynamic" else "fixed"
        run["prof_ms"] = {name: dict(zip(("total_ms", "launches"), eng.prof_get(k))) for name, k in kernels.items()}
        run["kinds"] = dict(outfile.OUT_KINDS)
        blocks, n_blocks, ms = eng.bgzf_deflate(text, repeat=3, code=code)
        bound_ms = (len(text) + len(blocks)) / COPY_BYTES_PER_S * 1e3
        run.update(kernel_ms=ms, blocks=n_blocks, copy_bound_ms=bound_ms, times_the_bound=ms / bound_ms, kernel_gb_per_s=len(text) / ms / 1e6)
        if code == "dynamic":  # both kernels in one process, alternating
            run["kernel_ms_alternating"] = [dict(code=c, kernel_ms=eng.bgzf_deflate(text, repeat=3, code=c)[2]) for c in ("fixed", "dynamic", "fixed", "dynamic")]
    os.remove(out)
    print("BGZF_ROUTE_AB " + json.dumps(run), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cohort", choices=sorted(shape.SHAPES))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", default=None, choices=sorted(set(ROUTES + INDEX_ROUTES)))
    ap.add_argument("--index", action="store_true", help="the index leg: device / device-index / host / host-index -> profiles/tbx_route_ab.json")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    routes = INDEX_ROUTES if a.index else ROUTES
    a.out = a.out or os.path.join(ROOT, "profiles", "tbx_route_ab.json" if a.index else "bgzf_dynamic_ab.json")
    a.dir = a.dir or tempfile.mkdtemp(prefix="bgzf_route_ab_")
    os.makedirs(a.dir, exist_ok=True)
    n_samples, n_records = shape.SHAPES[a.shape]
    src = os.path.join(a.dir, "dnms_%s.vcf" % a.shape)
    if not os.path.exists(src):
        shape.generate(src + ".part", n_samples, n_records)
        os.replace(src + ".part", src)
    with open(src, "rb") as fh:  # the page cache, warm for every route
        while fh.read(1 << 24):
            pass
    runs = {r: [] for r in routes}
    for it in range(a.repeat):
        for route in routes:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", route, "--shape", a.shape, "--dir", a.dir]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:  # (a child that failed ends the measurement: nothing more is started)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            run = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("BGZF_ROUTE_AB ")][-1][len("BGZF_ROUTE_AB "):])
            runs[route].append(run)
            print("[bgzf_route_ab] %s %s run %d: %.3f s wall, %.3f s host CPU, %d bytes" % (a.shape, route, it, run["wall_s"], run["host_cpu_s"], run["file_bytes"]),
                  file=sys.stderr, flush=True)
    same = len({r["text_sha"] for rr in runs.values() for r in rr}) == 1
    assert same, "the routes' files hold different text (shape %s)" % a.shape
    if a.index:
        for base in ("device", "host"):
            assert len({r["file_sha"] for r in runs[base] + runs[base + "-index"]}) == 1, "the %s route's data file differs with the index" % base
    res = dict(what="records dict -> out.vcf.gz (+ out.vcf.gz.tbi), UZ_OUT_BGZF device / host, each without and with UZ_OUT_INDEX=tbi; a fresh process per run, routes alternating, "
                    "page cache warm; wall and host CPU seconds of unfazed.write_vcf_output, HIP start-up excluded" if a.index else "records dict -> out.vcf.gz, UZ_OUT_BGZF unset (plain text) / host (zlib level 6) / device (uz_bgzf_deflate) / device-dynamic (UZ_OUT_BGZF_CODE=dynamic); a fresh process per run, "
                    "routes alternating, page cache warm; wall and host CPU seconds of unfazed.write_vcf_output, HIP start-up excluded",
               shape=a.shape, samples=n_samples, records=n_records, input_bytes=os.path.getsize(src), repeat=a.repeat, runs=runs, same_text_on_every_route=same)
    for route in routes:
        res[route.replace("-", "_") + "_median_wall_s"] = statistics.median(r["wall_s"] for r in runs[route])
        res[route.replace("-", "_") + "_file_bytes"] = runs[route][0]["file_bytes"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
    allres[a.shape] = res
    json.dump(allres, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
