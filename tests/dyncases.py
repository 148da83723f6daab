"""The panel of the dynamic coder (unfazed_amd/csrc/deflate_dyn.hpp: k_bgzf_deflate_dyn on the device, tests/bgzf_dyn_main.cpp on the host): the
fixed coder's panel (tests/bgzfoutcases.py), whose every payload is an edge of the shared parse, and the payloads that reach the edges of the code
construction.  tests/test_bgzf_dyn_body.py runs it through the host program, tests/test_bgzf_dyn_gpu.py holds the device's bytes to the
program's."""
import os
import random
import struct
import subprocess

import bgzfoutcases as panel

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
STORED, FIXED, DYNAMIC = 0, 1, 2
FIB_TAIL = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233]


def deep_litlen(values, copies):
    """`values` byte values at `copies` each and twelve more at Fibonacci counts, shuffled: a literal histogram whose Huffman code is deeper than
    15 bits.  All bytes lie under 144, so the fixed form takes 8 bits each and is not stored."""
    assert values + len(FIB_TAIL) <= 144
    data = bytearray()
    for v in range(values):
        data += bytes([v]) * copies
    for k, c in enumerate(FIB_TAIL):
        data += bytes([values + k]) * c
    random.Random(1).shuffle(data)
    return bytes(data)


STRICT_TAIL = [1, 3, 7, 13, 24, 42, 73, 126, 216, 369]  # each above the sum of the two before it with room to spare: a chain in EVERY optimal tree


def deep_strict(values, copies):
    """deep_litlen's shape with a tail that a stray match symbol does not unmake.  A Fibonacci tail is a chain only while nothing else is as
    rare as its first members: the two or three matches the parse finds in the shuffled bytes add symbols that occur once or twice, and the
    optimal code of deep/litlen's TOKENS is 13 bits deep, not the 17 of its bytes.  Here the tail is STRICT_TAIL's counts below `copies`:
    (100, 300) gives 30 505 bytes whose tokens' every optimal code is 16 bits deep, (110, 560) 62 474 bytes and 17 bits."""
    tail = [c for c in STRICT_TAIL if c < copies]
    assert values + len(tail) <= 144
    data = bytearray()
    for v in range(values):
        data += bytes([v]) * copies
    for k, c in enumerate(tail):
        data += bytes([values + k]) * c
    random.Random(1).shuffle(data)
    return bytes(data)


def cl_deep(seed):
    """a candidate for a code-length code deeper than 7 bits without the limit: 140 literals whose counts are spread evenly over thirteen
    octaves, so that the literal code uses many lengths, few of them often (seed 10 is the first hit of a search over seeds 1 .. 400:
    unlimited depth 8)"""
    rng = random.Random(seed)
    data = bytearray()
    for v in range(140):
        data += bytes([v]) * max(1, int(2 ** (rng.random() * 13)))
    rng.shuffle(data)
    return bytes(data[:panel.SLICE])


def build_cases():
    cases = list(panel.CASES)
    cases.append(("deep/litlen", deep_litlen(120, 300)))
    cases.append(("deep/litlen/full", deep_litlen(127, 509)))
    cases.append(("deep/strict", deep_strict(100, 300)))
    cases.append(("deep/strict/full", deep_strict(110, 560)))
    cases.append(("deep/codelen", cl_deep(10)))
    return cases


CASES = build_cases()
BY_NAME = dict(CASES)
assert len(BY_NAME) == len(CASES)
assert len(BY_NAME["deep/litlen"]) == 36608 and len(BY_NAME["deep/litlen/full"]) == 65251


def build_program(tmp_dir, san="address,undefined"):
    """tests/bgzf_dyn_main.cpp as a program of its own -> its path, or None when this toolchain cannot link the sanitizers' runtime"""
    def gxx(src, out):
        return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                               "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                              capture_output=True, text=True, timeout=300)
    probe = os.path.join(str(tmp_dir), "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    if gxx(probe, os.path.join(str(tmp_dir), "probe")).returncode != 0:
        return None
    exe = os.path.join(str(tmp_dir), "bgzf_dyn")
    cc = gxx(os.path.join(_HERE, "bgzf_dyn_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    return exe


def run_program(exe, cases, tmp_dir):
    """-> per case (blocks' bytes, [kind of each block])"""
    src, dst = os.path.join(str(tmp_dir), "dyn_cases.bin"), os.path.join(str(tmp_dir), "dyn_out.bin")
    panel.dump(cases, src)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "bgzf dyn ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        nb, size = struct.unpack_from("<IQ", raw, at)
        at += 12
        out.append((raw[at:at + size], list(raw[at + size:at + size + nb])))
        at += size + nb
    assert at == len(raw)
    return out


def run_code(exe, vectors, tmp_dir):
    """vectors: [(limit, counts)] -> the lengths uz_dy_build gives each"""
    src = os.path.join(str(tmp_dir), "vectors.txt")
    with open(src, "w") as fh:
        for limit, counts in vectors:
            fh.write(" ".join(str(v) for v in [limit] + list(counts)) + "\n")
    run = subprocess.run([exe, "--code", src], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    out = [[int(v) for v in line.split()] for line in run.stdout.split("\n") if line.strip()]
    assert [len(v) for v in out] == [len(c) for _, c in vectors]
    return out
