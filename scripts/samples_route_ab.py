#!/usr/bin/env python
"""A/B of the two routes that bring a cohort's sample table to the device from an indexed BGZF VCF: "sample table ready on the device" timed for
  host    eager region decode (every sample cell parsed on the host) + SitesTable.sample_columns (uz_samples_pack) + uz_samples_upload
  device  lazy region decode (no sample cell parsed) + the record text streamed up + k_vcf_tabs / k_vcf_cells + the settle round trip
over a synthetic text VCF, default 600 samples x 20 000 sites (about 15 bytes per cell), written once as BGZF + TBI.  Each run is a fresh child
process under its own `timeout -k 10`; the routes alternate, --runs of each.  Recorded beside the totals: text bytes, the host-to-device rate the
chunks' copies reached, per-chunk kernel time beside per-chunk copy time, host CPU-seconds of both routes.  The bar: every run of the device
route beats every run of the host route (exit status 1 otherwise).
    python scripts/samples_route_ab.py [--samples 600] [--sites 20000] [--runs 3] [--out profiles/samples_route_ab.json]
--bcf: the same table written as BCF + CSI (int8 GT, int16 AD -- int32 in the records with a depth above 32767 --, float GQ), the device route
through uz_samples_from_bcf / k_bcf_cells; the result goes to profiles/samples_route_bcf_ab.json, with the bytes each route sends over the link.
A child that ends by a signal, an abort or its time limit ends the whole measurement: nothing more is started on the device."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_vcf(path, n_samples, n_sites, seed=7):
    """a plain cohort file: GT:AD:GQ cells of 1-2 digit depths and integer GQ, sites 50 bases apart on 20 contigs (the region decode shares a
    file among its threads contig by contig); the sample regions come from
    a pool of 64 distinct lines (the routes' cost does not depend on which), every 97th record carries a depth above 32767 (the wide list and
    the settle round trip stay in play)"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    from filesio import write_bgzf_text, write_tbi
    rng = np.random.default_rng(seed)
    gts = ["0/0", "0/1", "1/1", "./.", "0|1"]
    pool = []
    for _ in range(64):
        g = rng.integers(0, 5, n_samples)
        r, a, q = rng.integers(0, 60, n_samples), rng.integers(0, 60, n_samples), rng.integers(0, 100, n_samples)
        pool.append("\t".join("%s:%d,%d:%d" % (gts[g[s]], r[s], a[s], q[s]) for s in range(n_samples)))
    n_contigs = min(20, max(1, n_sites // 64))
    per = (n_sites + n_contigs - 1) // n_contigs
    head = ["##fileformat=VCFv4.2"] + ["##contig=<ID=chr%d>" % (c + 1) for c in range(n_contigs)] + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%04d" % s for s in range(n_samples))]
    lines = []
    for i in range(n_sites):
        region = pool[i % 64]
        if i % 97 == 5:
            region = "0/1:40000,12:50" + region[region.index("\t"):] if n_samples > 1 else "0/1:40000,12:50"
        lines.append("chr%d\t%d\t.\tA\tG\t50\tPASS\t.\tGT:AD:GQ\t%s" % (i // per + 1, 101 + 50 * (i % per), region))
    text = "\n".join(head + lines) + "\n"
    write_bgzf_text(path, text, block_bytes=60000)
    write_tbi(path)
    return len(text)


def write_bcf(path, n_samples, n_sites, seed=7):
    """the same plain cohort table as BCF + CSI, built with numpy: GT int8 x 2, AD int16 x 2, GQ float per sample, sites 50 bases apart on 20
    contigs; every 97th record has a first sample with a depth of 40000 and carries its AD as int32 (the wide list and the settle round trip
    stay in play)"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import bcfcases
    rng = np.random.default_rng(seed)
    n_contigs = min(20, max(1, n_sites // 64))
    per = (n_sites + n_contigs - 1) // n_contigs
    i = np.arange(n_sites)
    codes = np.array([[2, 2], [2, 4], [4, 4], [0, 0], [2, 5]], np.int8)  # 0/0 0/1 1/1 ./. 0|1
    gt = codes[rng.integers(0, 5, (n_sites, n_samples))]
    ad = rng.integers(0, 60, (n_sites, n_samples, 2)).astype(np.int16)
    gq = rng.integers(0, 100, (n_sites, n_samples)).astype(np.float32)
    samples = ["s%04d" % s for s in range(n_samples)]
    data = bytearray(bcfcases.table_bcf_bytes(samples, ["chr%d" % (c + 1) for c in range(n_contigs)], i // per, 100 + 50 * (i % per), gt, ad, gq))
    # the deep records: AD as int32, 40000 in the first sample -- the record grows by 4 bytes per sample, so the file is stitched from slices
    head = len(bcfcases.header_bytes(samples, ["chr%d" % (c + 1) for c in range(n_contigs)]))
    rec_len = (len(data) - head) // n_sites
    out = bytearray(data[:head])
    ad_at = rec_len - 4 * n_samples - 3 - 4 * n_samples  # the AD values of a record: behind them the GQ key, its descriptor and the GQ values
    done = head
    for k in range(5, n_sites, 97):
        at = head + k * rec_len
        out += data[done:at]
        r = data[at: at + rec_len]
        wide = ad[k].astype("<i4")
        wide[0, 0] = 40000
        assert r[ad_at - 1] == 0x22
        r = r[:ad_at - 1] + bytes([0x23]) + wide.tobytes() + r[ad_at + 4 * n_samples:]
        r[4:8] = (int.from_bytes(r[4:8], "little") + 4 * n_samples).to_bytes(4, "little")
        out += r
        done = at + rec_len
    out += data[done:]
    bcfcases.write_indexed(path, bytes(out))
    return len(out)


def child(route, path):
    sys.path.insert(0, os.getcwd())
    import numpy as np
    from unfazed_amd import abi, io_native
    from unfazed_amd.engine import K_BCF_CELLS, K_BCF_COPY, K_VCF_CELLS, K_VCF_COPY, K_VCF_TABS, HipEngine
    bcf = path.endswith(".bcf")
    threads = int(os.environ.get("UZ_IO_THREADS", "0"))
    eng = HipEngine(0)
    eng.sync()
    names = io_native.tabix_contigs(path)
    whole = (list(range(len(names))), [0] * len(names), [2 ** 31 - 1] * len(names))
    res = dict(route=route)
    c0, t0 = time.process_time(), time.perf_counter()
    table = io_native.read_vcf_table_regions(path, *whole, threads=threads, lazy=(route == "device"))
    t1 = time.perf_counter()
    sid = eng.upload_sites(table)
    ns, n = len(table.samples), table.n_sites
    if route == "host":
        cols = table.sample_columns(table.samples)
        t2 = time.perf_counter()
        mid = eng.upload_samples(sid, cols)
        n_back = 0
        res.update(pack_s=t2 - t1, link_bytes=int(7 * ns * n + (0 if cols.wide is None else cols.wide[0].size * (8 + 8 * ns))))
    else:
        if bcf:
            eng.prof_enable([K_BCF_CELLS, K_BCF_COPY])
            mid, n_back = eng.samples_from_bcf(sid, table, np.arange(ns), settle=False)
        else:
            eng.prof_enable([K_VCF_TABS, K_VCF_CELLS, K_VCF_COPY])
            mid, n_back = eng.samples_from_text(sid, table, np.arange(ns), settle=False)
        t2 = time.perf_counter()
        if n_back:
            eng.settle_samples(mid, table, np.arange(ns), n_back)
        res.update(parse_s=t2 - t1, settle_s=time.perf_counter() - t2)
    fams = eng.families_from_samples(mid, [0, ns - 3], [1, ns - 2], [2, ns - 1])  # (the table is ready when a family can be made of it)
    eng.sync()
    t3, c3 = time.perf_counter(), time.process_time()
    res.update(samples=ns, sites=n, total_s=t3 - t0, decode_s=t1 - t0, table_s=t3 - t1, host_cpu_s=c3 - c0, sites_unsettled=n_back)
    if route == "device" and bcf:
        import ctypes as C
        assert table.genotypes_deferred and table.is_bcf
        v = io_native.vcf_samples_bcf(table)
        desc = np.ctypeslib.as_array(C.cast(v.fld_desc, C.POINTER(C.c_uint32)), (n, 5)).astype(np.int64)
        size = np.array([0, 1, 2, 4, 0, 4, 0, 0], np.int64)[desc & 15]
        values = int((((desc >> 4) * size * ns + 3) // 4 * 4).sum())  # the five arrays of every record, each on a 4-byte boundary
        (cells_ms, chunks), (copy_ms, _) = eng.prof_get(K_BCF_CELLS), eng.prof_get(K_BCF_COPY)
        res.update(value_bytes=values, link_bytes=values + 40 * n + int(n_back) * ns * 7, chunks=int(chunks), cells_ms_per_chunk=cells_ms / max(1, chunks),
                   copy_ms_per_chunk=copy_ms / max(1, chunks), h2d_GBps=(values / (copy_ms / 1e3) / 1e9) if copy_ms > 0 else None,
                   parse_no_longer_than_copy=cells_ms <= copy_ms)
    elif route == "device":
        assert table.genotypes_deferred
        text = io_native.vcf_samples_text(table)
        (tabs_ms, chunks), (cells_ms, _), (copy_ms, _) = eng.prof_get(K_VCF_TABS), eng.prof_get(K_VCF_CELLS), eng.prof_get(K_VCF_COPY)
        res.update(text_bytes=int(text.text_bytes), chunks=int(chunks), tabs_ms_per_chunk=tabs_ms / max(1, chunks), cells_ms_per_chunk=cells_ms / max(1, chunks),
                   copy_ms_per_chunk=copy_ms / max(1, chunks), h2d_GBps=(text.text_bytes / (copy_ms / 1e3) / 1e9) if copy_ms > 0 else None,
                   parse_no_longer_than_copy=(tabs_ms + cells_ms) <= copy_ms)
    P = abi.make_params()
    h = hashlib.sha256()
    for f in fams:
        gt, cols16 = eng.family_fetch(f, n)
        h.update(gt.tobytes() + cols16.tobytes() + eng.classify(f, P, n).tobytes())
    res["rows_sha"] = h.hexdigest()[:16]
    eng.free_sites(sid)
    eng.close()
    print("AB_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=600)
    ap.add_argument("--sites", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bcf", action="store_true", help="the table as BCF + CSI (device route: uz_samples_from_bcf)")
    ap.add_argument("--out", default=None, help="default: profiles/samples_route_ab.json, with --bcf profiles/samples_route_bcf_ab.json")
    ap.add_argument("--limit", type=int, default=0, help="seconds a child may take (default: sized by the file)")
    ap.add_argument("--child", choices=["host", "device"])
    ap.add_argument("--path")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.path)
    a.out = a.out or os.path.join(ROOT, "profiles", "samples_route_bcf_ab.json" if a.bcf else "samples_route_ab.json")
    limit = a.limit or int(120 + a.samples * a.sites / 12e6 * 30)
    runs = {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cohort.bcf" if a.bcf else "cohort.vcf.gz")
        t0 = time.perf_counter()
        text_bytes = (write_bcf if a.bcf else write_vcf)(path, a.samples, a.sites)
        print("wrote %d bytes as %d bytes of BGZF in %.1f s" % (text_bytes, os.path.getsize(path), time.perf_counter() - t0), flush=True)
        for k in range(a.runs):
            for route in ("host", "device"):
                cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", route, "--path", path]
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
                line = [x for x in p.stdout.splitlines() if x.startswith("AB_RESULT ")]
                if p.returncode != 0 or not line:
                    print("run %d of the %s route ended with status %d: stopping here\n%s" % (k, route, p.returncode, p.stderr[-2000:]), file=sys.stderr)
                    return 2
                r = json.loads(line[-1][len("AB_RESULT "):])
                runs[route].append(r)
                print("%s run %d: %.3f s total (decode %.3f s), %.2f CPU-s" % (route, k, r["total_s"], r["decode_s"], r["host_cpu_s"]), flush=True)
    host_t, dev_t = [r["total_s"] for r in runs["host"]], [r["total_s"] for r in runs["device"]]
    bar = max(dev_t) < min(host_t)
    same = len({r["rows_sha"] for r in runs["host"] + runs["device"]}) == 1
    keys = ("decode_s", "table_s", "host_cpu_s")
    what = ("sample table ready on the device from a BCF with its CSI: eager decode + pack + upload (host) against lazy decode + value arrays up + k_bcf_cells + settle (device)"
            if a.bcf else "sample table ready on the device from an indexed BGZF VCF: eager decode + pack + upload (host) against lazy decode + text up + parse + settle (device)")
    out = dict(what=what + "; fresh process per run, alternating; UZ_IO_THREADS=%s" % os.environ.get("UZ_IO_THREADS", "0 (every CPU the process may use)"),
               samples=a.samples, sites=a.sites, text_bytes=text_bytes, host_total_s=host_t, device_total_s=dev_t,
               host={k: [r.get(k) for r in runs["host"]] for k in keys + ("pack_s", "link_bytes")},
               device={k: [r.get(k) for r in runs["device"]] for k in keys + ("parse_s", "settle_s", "sites_unsettled", "chunks", "tabs_ms_per_chunk", "cells_ms_per_chunk", "copy_ms_per_chunk",
                                                                              "h2d_GBps", "parse_no_longer_than_copy", "value_bytes", "link_bytes")},
               every_device_run_beats_every_host_run=bar, same_rows_and_class_bytes_on_both_routes=same)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))
    return 0 if (bar and same) else 1


if __name__ == "__main__":
    sys.exit(main())
