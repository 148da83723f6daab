#!/usr/bin/env python
"""How far the BGZF writer's streams (csrc/deflate_body.hpp: LZ77 by one probe per position, fixed Huffman) are from zlib's, on the CPU build of
the body, which emits the device's bytes (tests/bgzf_body_main.cpp; tests/test_bgzf_deflate_gpu.py holds the device to it).  No device needed.
Inputs, all cut into the same 65 280-byte slices:
  panel_text_vcf   the panel's ~300 KB of annotated-VCF text (tests/bgzfoutcases.py text/vcf)
  trio / cohort    the input files of scripts/vcf_route_ab.py's shapes (the same cells the annotated output holds, before UOPS / UET are
                   appended); the cohort file's first --cohort-bytes bytes (whole slices)
Against: zlib level 1 with Z_FIXED (the same code family: the difference is the matcher alone), zlib level 1 and zlib level 6 with the default
strategy (dynamic Huffman).  The dynamic route (csrc/deflate_dyn.hpp through tests/bgzf_dyn_main.cpp: the same parse, per slice the shortest of a
dynamic, the fixed and a stored block) stands beside the body in columns of its own.  -> profiles/bgzf_deflate_ratio.json
    python scripts/bgzf_ratio.py [--cohort-bytes 33423360] [--out profiles/bgzf_deflate_ratio.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
SLICE = 0xFF00


def zlib_bytes(data, level, strategy):
    total = 0
    for at in range(0, len(data), SLICE):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(z.compress(data[at:at + SLICE]) + z.flush())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cohort-bytes", type=int, default=512 * SLICE)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_deflate_ratio.json"))
    a = ap.parse_args()
    import bgzfoutcases as panel
    import dyncases as dyn
    import vcf_route_ab as shape
    d = tempfile.mkdtemp(prefix="bgzf_ratio_")
    exe = os.path.join(d, "bgzf_body")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "unfazed_amd", "csrc"),
                           os.path.join(ROOT, "tests", "bgzf_body_main.cpp"), "-o", exe])
    exe_dyn = os.path.join(d, "bgzf_dyn")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "unfazed_amd", "csrc"),
                           os.path.join(ROOT, "tests", "bgzf_dyn_main.cpp"), "-o", exe_dyn])
    inputs = {"panel_text_vcf": panel.BY_NAME["text/vcf"]}
    for name, (n_samples, n_records) in sorted(shape.SHAPES.items()):
        path = os.path.join(d, name + ".vcf")
        shape.generate(path, n_samples, n_records)
        data = open(path, "rb").read()
        inputs[name] = data[:a.cohort_bytes // SLICE * SLICE] if name == "cohort" else data
        os.remove(path)
    res = {"what": "bytes of raw DEFLATE streams over 65 280-byte slices: the body (fixed code) and the dynamic route (CPU builds, the device's bytes) against zlib", "inputs": {}}
    for name, data in inputs.items():
        (blocks, stored), = panel.run_program(exe, [(name, data)], d)
        parts = panel.check_blocks(data, blocks)
        body = sum(len(p[1]) for p in parts)
        (dyn_blocks, kinds), = dyn.run_program(exe_dyn, [(name, data)], d)
        dynamic = sum(len(p[1]) for p in panel.check_blocks(data, dyn_blocks))
        fixed1, dyn1, dyn6 = zlib_bytes(data, 1, zlib.Z_FIXED), zlib_bytes(data, 1, zlib.Z_DEFAULT_STRATEGY), zlib_bytes(data, 6, zlib.Z_DEFAULT_STRATEGY)
        res["inputs"][name] = dict(text_bytes=len(data), slices=len(parts), stored_slices=sum(stored), body_bytes=body, zlib_level1_fixed_bytes=fixed1,
                                   zlib_level1_bytes=dyn1, zlib_level6_bytes=dyn6, body_over_text=round(body / len(data), 4),
                                   body_over_zlib_level1_fixed=round(body / fixed1, 4), body_over_zlib_level1=round(body / dyn1, 4),
                                   body_over_zlib_level6=round(body / dyn6, 4),
                                   dynamic_bytes=dynamic, dynamic_kinds=dict(stored=kinds.count(dyn.STORED), fixed=kinds.count(dyn.FIXED), dynamic=kinds.count(dyn.DYNAMIC)),
                                   dynamic_over_text=round(dynamic / len(data), 4), dynamic_over_body=round(dynamic / body, 4),
                                   dynamic_over_zlib_level1_fixed=round(dynamic / fixed1, 4), dynamic_over_zlib_level1=round(dynamic / dyn1, 4),
                                   dynamic_over_zlib_level6=round(dynamic / dyn6, 4))
        print(name, res["inputs"][name], flush=True)
    json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
