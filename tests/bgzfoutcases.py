"""The panel of the BGZF writer (unfazed_amd/csrc/deflate_body.hpp: k_bgzf_deflate on the device, tests/bgzf_body_main.cpp on the host): every
payload is the smallest input at which one rule of the body can go wrong.  tests/test_bgzf_body.py runs it through the host program,
tests/test_bgzf_deflate_gpu.py holds the device's bytes to the host program's.

The body's hash is stated here (body_hash) and held to the program's own (`bgzf_body --hash`) by test_bgzf_body.py."""
import gzip
import os
import random
import struct
import subprocess
import zlib

SLICE = 0xFF00
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
DIST_EDGES = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
LEN_EDGES = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 257, 258, 259]

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def body_hash(four: bytes) -> int:
    """deflate_body.hpp uz_df_hash of the four bytes at a position"""
    return ((struct.unpack("<I", four)[0] * 2654435761) & 0xFFFFFFFF) >> 19


def copy_at(dist, length, seed):
    """`length` bytes copied from `dist` back, so that the body finds exactly that match: the source lies in an earlier group of 64 than the
    copy, a byte that differs ends the match, and between source and copy stands nothing that hashes like the source -- a run of zero bytes for
    dist >= 64 (one table entry), random bytes for the short distances, where source and copy overlap"""
    if dist < 64:
        pre = bytearray(rnd(128, seed))
        for k in range(length):
            pre.append(pre[len(pre) - dist])
        pre.append(pre[len(pre) - dist] ^ 0xFF)
        return bytes(pre) + rnd(32, seed + 1)
    src = bytes(1 + b % 255 for b in rnd(min(length, dist), seed))
    data = bytearray(rnd(64, seed + 1) + src + bytes(dist - len(src)))
    for k in range(length):
        data.append(data[len(data) - dist])
    data.append(data[len(data) - dist] ^ 0xFF)
    return bytes(data) + rnd(32, seed + 2)


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DEXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in (0, 1)]


def tokens(stream: bytes):
    """the tokens of a one-block fixed-Huffman stream (RFC 1951, 3.2.6): a literal as an int, a match as (length, distance)"""
    bits, at = int.from_bytes(stream, "little"), 3
    assert bits & 7 == 3

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    def code(n):  # Huffman codes arrive most-significant bit first
        v = 0
        for _ in range(n):
            v = (v << 1) | take(1)
        return v
    out = []
    while True:
        c = code(7)
        if c <= 0b0010111:
            sym = 256 + c
        else:
            c = (c << 1) | take(1)
            if 0b00110000 <= c <= 0b10111111:
                sym = c - 0b00110000
            elif 0b11000000 <= c <= 0b11000111:
                sym = 280 + c - 0b11000000
            else:
                sym = 144 + ((c << 1) | take(1)) - 0b110010000
        if sym == 256:
            assert (at + 7) // 8 == len(stream) and bits >> at == 0  # zero padding to the byte, nothing behind it
            return out
        if sym < 256:
            out.append(sym)
            continue
        assert sym <= 285
        length = LBASE[sym - 257] + take(LEXTRA[sym - 257])
        d = code(5)
        assert d < 30
        out.append((length, DIST_EDGES[d] + take(DEXTRA[d])))


def colliding_words(count, seed):
    """`count` distinct four-byte strings with one hash"""
    rng, want, out = random.Random(seed), None, []
    while len(out) < count:
        w = rng.randbytes(4)
        h = body_hash(w)
        if want is None:
            want = h
        if h == want and w not in out:
            out.append(w)
    return out


def vcf_text():
    """about 300 KB of annotated-VCF text: the host writer's output of vcfrowcases' seeded cases, back to back (lines straddle the slices)"""
    import tempfile

    import vcfrowcases
    out = []
    with tempfile.TemporaryDirectory() as d:
        for case in vcfrowcases.fuzz_cases(20241020, 3600):
            kind, text = vcfrowcases.host_output(case, d)
            if kind == "text":
                out.append(text)
    return b"".join(out)


def build_cases():
    cases = []
    add = lambda name, payload: cases.append((name, bytes(payload)))
    for n in (0, 1, 2, 3):
        add("tiny/%d" % n, b"xyz"[:n])
    add("aaa", b"aaa")
    add("edge/65280", rnd(255, 1) * 256)
    add("edge/65281", rnd(255, 2) * 256 + b"!")
    add("zeros/65280", bytes(SLICE))
    add("ab/1000", b"ab" * 1000)
    add("ab/40000", b"ab" * 40000)
    for d in DIST_EDGES + [32768]:
        add("dist/%d" % d, copy_at(d, 40, 100 + d))
        if d - 1 not in DIST_EDGES and d > 1:
            add("dist/%d" % (d - 1), copy_at(d - 1, 40, 200 + d))
    add("dist/32769", copy_at(32769, 40, 300))
    for ln in LEN_EDGES:
        add("len/%d" % ln, copy_at(300, ln, 400 + ln))
    add("len/600", copy_at(300, 600, 399))
    line = rnd(200, 5)
    add("across/65280", line * (2 * SLICE // 200 + 1))
    add("lit9", bytes(144 + (b % 112) for b in rnd(5000, 6)))
    add("all256", bytes(range(256)) * 3 + bytes(reversed(range(256))))
    add("random/65280", rnd(SLICE, 7))
    add("random/40000", rnd(40000, 8))
    words = colliding_words(40, 9)
    add("collide/words", b"".join(w + rnd(60, 10 + i) for i, w in enumerate(words)) * 2)
    add("collide/near", b"".join(words[i % 40] + words[(i * 7) % 40][:3] + b"#" * (i % 5) for i in range(2000)))
    add("text/line", b"chr1\t100\t.\tA\tT\t.\t.\t.\tGT:DP\t0/1:30\t0/0:28\t0/0:31\n" * 400)
    add("text/vcf", vcf_text())
    return cases


CASES = build_cases()
BY_NAME = dict(CASES)
assert len(BY_NAME) == len(CASES)


def dump(cases, path):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, payload in cases:
            fh.write(struct.pack("<Q", len(payload)))
            fh.write(payload)


def build_program(tmp_dir, san="address,undefined"):
    """tests/bgzf_body_main.cpp as a program of its own -> its path, or None when this toolchain cannot link the sanitizers' runtime"""
    def gxx(src, out):
        return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                               "-I", os.path.join(_ROOT, "include"), "-I", os.path.join(_ROOT, "unfazed_amd", "csrc"), src, "-o", out],
                              capture_output=True, text=True, timeout=300)
    probe = os.path.join(str(tmp_dir), "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    if gxx(probe, os.path.join(str(tmp_dir), "probe")).returncode != 0:
        return None
    exe = os.path.join(str(tmp_dir), "bgzf_body")
    cc = gxx(os.path.join(_HERE, "bgzf_body_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    return exe


def run_program(exe, cases, tmp_dir):
    """-> per case (blocks' bytes, [stored?])"""
    src, dst = os.path.join(str(tmp_dir), "cases.bin"), os.path.join(str(tmp_dir), "out.bin")
    dump(cases, src)
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "bgzf body ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        nb, size = struct.unpack_from("<IQ", raw, at)
        at += 12
        out.append((raw[at:at + size], [bool(b) for b in raw[at + size:at + size + nb]]))
        at += size + nb
    assert at == len(raw)
    return out


def split_blocks(blocks: bytes):
    """-> per block (header 18 bytes, stream, crc, isize); asserts the fixed bytes and BSIZE"""
    out, at = [], 0
    while at < len(blocks):
        assert blocks[at:at + 16] == HEAD, at
        size = struct.unpack_from("<H", blocks, at + 16)[0] + 1
        assert 26 < size <= 65536 and at + size <= len(blocks)
        crc, isize = struct.unpack_from("<II", blocks, at + size - 8)
        out.append((blocks[at:at + 18], blocks[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def check_blocks(payload: bytes, blocks: bytes):
    """everything a BGZF reader and the body's own bound ask of `blocks` as the image of `payload`"""
    assert gzip.decompress(blocks + EOF_MARKER) == payload
    parts = split_blocks(blocks)
    k, rest = divmod(len(payload), SLICE)
    assert [p[3] for p in parts] == [SLICE] * k + ([rest] if rest else [])
    for i, (_, stream, crc, isize) in enumerate(parts):
        piece = payload[i * SLICE:i * SLICE + isize]
        assert crc == zlib.crc32(piece) & 0xFFFFFFFF
        assert len(stream) <= 5 + len(piece)
        z = zlib.decompressobj(-15)
        assert z.decompress(stream) == piece and z.eof and z.unused_data == b""
    return parts
