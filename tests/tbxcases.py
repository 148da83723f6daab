"""The panel of the tabix index writer (unfazed_amd/csrc/tbx_key.hpp, csrc/k_tbx.hip, unfazed_amd/tabix_index.py): every payload is a small text
with one place where the line rules, the kernels' tiles and steps, a chunk's edge or the table rules can go wrong.  Chunk edges come from
UZ_BGZF_CHUNK_BYTES = 65 280 and 130 560, not from size: E = 130 560 is an edge at both.

CASES: (name, preset, payload, verdict): verdict None = indexable, else the model's reason ("order", "contig", "range", "meta", "empty", "cr",
"pos"); the preset is the one the tests ask for by name (write_output takes its own from the text).  HOST_ROWS: for the payloads built around a chunk edge, the rows the host has to settle at each chunk size, counted by hand from how
the payload was built (the model's count is held to them in test_tbx_model.py)."""
SLICE = 0xFF00
CHUNKS = (65280, 130560)
E = 130560
HEADER = b"##fileformat=VCFv4.2\n##contig=<ID=chr1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\n"
BED_HEADER = b"#chrom\tstart\tend\tkid_id\tvar_type\n"


def line(chrom=b"chr1", pos=100, ref=b"A", info=b".", ident=b".", tail=b"GT:DP\t0/1:30\t0/0:28"):
    out = b"\t".join([chrom, b"%d" % pos, ident, ref, b"C", b"50", b"PASS", info])
    return out + (b"\t" + tail if tail is not None else b"") + b"\n"


class Text:
    """a VCF text under construction: records ascend by themselves, fillers bring the text to an exact length"""

    def __init__(self, header=HEADER, chrom=b"chr1", pos=100):
        self.b, self.chrom, self.pos = bytearray(header), chrom, pos

    def __len__(self):
        return len(self.b)

    def add(self, raw: bytes):
        at = len(self.b)
        self.b += raw
        return at

    def rec(self, step=7, **kw):
        self.pos += step
        kw.setdefault("chrom", self.chrom)
        kw.setdefault("pos", self.pos)
        return self.add(line(**kw))

    def fill_to(self, target: int):
        """filler records (their length is in the sample column, behind the key columns) until the text is `target` bytes long"""
        while len(self.b) < target:
            self.pos += 3
            base = line(self.chrom, self.pos, tail=b"GT\t")
            room = target - len(self.b)
            assert room >= len(base), "no room for a filler"
            want = room if room < 2 * len(base) + 24 else min(room - len(base) - 12, 100 + self.pos % 211)
            self.b += base[:-1] + b"x" * (want - len(base)) + b"\n"
        assert len(self.b) == target

    def cut_in(self, edge: int, inside: bytes, by: int, **kw):
        """a record placed so that byte `by` of its first `inside` is the first byte behind `edge`"""
        kw.setdefault("chrom", self.chrom)
        kw.setdefault("pos", 500000)  # (behind every filler's)
        raw = line(**kw)
        self.fill_to(edge - raw.index(inside) - by)
        assert self.pos < kw["pos"]
        self.pos = kw["pos"]
        return self.add(raw)

    def done(self, records=3):
        for _ in range(records):
            self.rec()
        return bytes(self.b)


def build_cases():
    cases = []

    def add(name, payload, verdict=None, preset="vcf"):
        cases.append((name, preset, bytes(payload), verdict))

    # ---- lines and slices
    add("lines/header-only", HEADER)
    add("lines/one-record", HEADER + line())
    add("lines/no-header", line(pos=5) + line(pos=9))
    add("lines/no-trailing-newline", HEADER + line() + line(pos=200)[:-1])
    add("lines/end-at-text-end", HEADER + line() + line(pos=200, info=b"SVTYPE=DEL;END=7000", tail=None)[:-1])
    t = Text()
    t.fill_to(SLICE)
    at0 = t.rec()
    t.fill_to(2 * SLICE - 1)
    at1 = t.rec()
    assert at0 % SLICE == 0 and at1 % SLICE == SLICE - 1
    add("lines/slice-0-and-65279", t.done())
    t = Text()
    t.fill_to(1000)
    t.rec(tail=b"GT" + b"\t0/1:12,9:99" * 11700)  # ~140 KB: starts in block 0, ends in block 2
    assert len(t) > 2 * SLICE + 1000 and len(t) < 3 * SLICE
    add("lines/long-140k", t.done())
    # ---- tile and lane edges of k_tbx_mark / k_tbx_starts
    t = Text()
    for target in (2048, 4097, 5120 + 16, 6144 + 17 + 64, 7168 + 1008, 9216):  # '\n' at tile byte 1023, 0 (= 1024), lane byte 15, 0 (= 16), ...
        t.fill_to(target)
    assert t.b[2047] == 10 and t.b[4096] == 10 and t.b[5120 + 15] == 10 and t.b[6144 + 16 + 64] == 10
    add("tiles/newline-edges", t.done())
    # ---- 64-byte steps of k_tbx_keys, counted from the line's first byte
    t = Text(chrom=b"c" * 63)
    t.rec()  # the first tab at byte 63
    t.chrom = b"d" * 64
    t.rec()  # ... at byte 64
    t.chrom = b"e" * 60
    t.rec(pos=1234567)  # POS over bytes 61 .. 67
    t.chrom, t.pos = b"f", 100
    for shift in range(5):  # "END=" begins at bytes 60 .. 64 of the line, ';' before it
        raw = line(b"f", 1000 + shift, info=b"SVTYPE=DEL;END=%d" % (5000 + shift), ident=b"i" * 40)
        k = raw.index(b"END=")
        t.add(line(b"f", 1000 + shift, info=b"SVTYPE=DEL;END=%d" % (5000 + shift), ident=b"i" * (40 + 60 + shift - k)))
    raw = line(b"f", 2000, info=b"END=123456", ident=b"i" * 10)
    t.add(line(b"f", 2000, info=b"END=123456", ident=b"i" * (10 + 62 - raw.index(b"123456"))))  # END's digits over bytes 62 .. 67
    add("steps/straddles", bytes(t.b))
    # ---- chunk edges (E is one at both chunk sizes).  At 65 280 the payloads built by fill_to have an ordinary line over that edge: its
    # key columns are some 30 bytes, so it is cut only where the edge falls in them; the hand counts below hold that by an assert
    def edge_case(name, build):
        t = Text()
        build(t)
        add(name, t.done())
    edge_case("edge/cut-chrom", lambda t: t.cut_in(E, b"chr1", 2))
    edge_case("edge/cut-pos", lambda t: t.cut_in(E, b"\t", 3))
    edge_case("edge/cut-ref", lambda t: t.cut_in(E, b"ACGTACGTACGTACGTACGT", 9, ref=b"ACGTACGTACGTACGTACGT"))
    edge_case("edge/cut-end-key", lambda t: t.cut_in(E, b"END=", 2, info=b"SVTYPE=DEL;END=900000"))
    edge_case("edge/cut-end-digits", lambda t: t.cut_in(E, b"END=", 7, info=b"SVTYPE=DEL;END=900000"))
    edge_case("edge/cut-behind-keys", lambda t: t.cut_in(E, b"GT:DP", 2))  # the keys end before the edge: not cut
    edge_case("edge/newline-last", lambda t: t.fill_to(E))

    def contig_change(t):
        t.fill_to(E)
        t.chrom, t.pos = b"chr2", 50
    edge_case("edge/contig-change", contig_change)
    # ---- INFO
    t = Text()
    for info in (b"END=5000;SVTYPE=DEL", b"SVTYPE=DEL;END=6000", b"XEND=9999999", b"SVTYPE=DEL;XEND=9999999;Y=1", b"END=abc", b"END=70x0;A=1", b"END=5", b".",
                 b"END=", b"A=1;END=8000;END=7500", b"END=9000", b"ZEND=1;END=9500;"):
        t.rec(info=info)
    t.add(b"chr1\t%d\t.\tACGT\tA\n" % (t.pos + 9))  # five columns: no INFO
    t.pos += 20
    t.rec(ref=b"ACGTACGTAC" * 30)
    add("info/forms", t.done())
    # (no meta line: held to the model alone.  write_tbi takes any integer behind "END=", the rules take ten digits)
    add("info/end-11-digits", line(pos=5, info=b"END=12345678901") + line(pos=9, info=b"A=1;END=12345678901;B=2") + line(pos=12, info=b"END=1234567890"), "range")
    # ---- positions: every bin level, the scheme's first and last base
    t = Text(pos=0)
    t.rec(step=1)  # POS = 1
    for k in (14, 17, 20, 23, 26):
        t.rec(pos=(1 << k) - 1, ref=b"ACGT")  # [2^k - 2, 2^k + 2)
    t.rec(pos=(1 << 29) - 3, ref=b"ACGT")  # end = 2^29
    add("pos/levels", bytes(t.b))
    add("pos/end-by-info", HEADER + line(pos=1000, info=b"END=%d" % (1 << 29)))
    add("pos/beyond", HEADER + line(pos=1000) + line(pos=(1 << 29) + 1), "range")
    add("pos/end-beyond", HEADER + line(pos=1000, info=b"END=%d" % ((1 << 29) + 1)), "range")
    # ---- contigs and sortedness
    add("contigs/prefixes", HEADER + b"".join(line(c, p) for c, p in ((b"chr1", 5), (b"chr1", 9), (b"chr10", 3), (b"chr10", 3), (b"chr1x", 4), (b"chr", 8), (b"chr100", 1))))
    add("order/equal-begins", HEADER + line(pos=50) + line(pos=50, ref=b"AC") + line(pos=50))
    add("order/decreasing", HEADER + line(pos=50) + line(pos=49), "order")
    add("order/contig-back", HEADER + line(b"chr1", 50) + line(b"chr2", 10) + line(b"chr1", 60), "contig")
    # ---- bins and the linear index
    add("bins/a-b-a", HEADER + line(pos=100) + line(pos=200, info=b"END=20000") + line(pos=300) + line(pos=400))
    add("linear/gaps", HEADER + line(pos=100000) + line(pos=100500) + line(pos=330000, info=b"END=400000") + line(pos=900000)
        + line(b"chr2", 70000) + line(b"chr2", 70001, info=b"SVTYPE=DUP;END=75000"))
    # ---- bad lines
    add("bad/meta-behind-data", HEADER + line(pos=5) + b"##late=1\n" + line(pos=9), "meta")
    add("bad/empty-line", HEADER + line(pos=5) + b"\n" + line(pos=9), "empty")
    add("bad/cr", HEADER + line(pos=5) + b"chr1\t7\t.\tA\tC\r\n", "cr")
    add("bad/cr-header", HEADER.replace(b"\n", b"\r\n") + line(pos=5), "cr")
    add("bad/pos-11-digits", HEADER + line(pos=5) + line(pos=12345678901), "pos")
    add("bad/pos-text", HEADER + line(pos=5).replace(b"\t5\t", b"\t5x\t"), "pos")
    add("cr/behind-keys", HEADER + line(pos=5)[:-1] + b"\r\n" + line(pos=9))  # never read: the key columns end before it
    # ---- BED
    bed = lambda c, s, e, rest=b"kid1\tSNV": b"%s\t%d\t%d\t%s\n" % (c, s, e, rest)
    add("bed/rows", BED_HEADER + bed(b"chr1", 10, 11) + bed(b"chr1", 20, 20) + bed(b"chr1", 16000, 40000) + bed(b"chr2", 5, 90), preset="bed")
    add("bed/three-columns", BED_HEADER + b"chr1\t10\t11\nchr1\t12\t13", preset="bed")
    add("bed/decreasing", BED_HEADER + bed(b"chr1", 10, 11) + bed(b"chr1", 9, 11), "order", preset="bed")
    add("bed/no-end", BED_HEADER + b"chr1\t10\n", "pos", preset="bed")
    # ---- bulk: some 300 KB of records over four contigs, windows with gaps, runs of every length
    t = Text()
    for c in (b"chr1", b"chr2", b"chr10", b"chrX"):
        t.chrom, t.pos = c, 1000
        for i in range(330):
            t.rec(step=1 + (i * 7919) % 9000, ref=b"A" * (1 + i % 5), info=b"END=%d" % (t.pos + 40000) if i % 37 == 0 else b"DP=%d" % i,
                  tail=b"GT:DP" + b"\t0/1:30" * (5 + i % 50))
    add("bulk/four-contigs", bytes(t.b))
    return cases


CASES = build_cases()
BY_NAME = {c[0]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# By hand, from how the edge payloads were built.  A payload of this panel is below 3 * 65 280 bytes unless noted, so it has 3 chunks of 65 280
# and 2 of 130 560, each with lines: 3 and 2 first lines.  Added to them: the record cut_in put over E where E falls inside its key columns.
# (The filler over the edge at 65 280 has its key columns in its first 30 bytes and fill_to never ends one there: the tests hold that.)
HOST_ROWS = {
    "edge/cut-chrom": {65280: 3 + 1, 130560: 2 + 1},
    "edge/cut-pos": {65280: 3 + 1, 130560: 2 + 1},
    "edge/cut-ref": {65280: 3 + 1, 130560: 2 + 1},
    "edge/cut-end-key": {65280: 3 + 1, 130560: 2 + 1},
    "edge/cut-end-digits": {65280: 3 + 1, 130560: 2 + 1},
    "edge/cut-behind-keys": {65280: 3, 130560: 2},
    "edge/newline-last": {65280: 3, 130560: 2},
    "edge/contig-change": {65280: 3, 130560: 2},
    "lines/long-140k": {65280: 2, 130560: 2},  # three chunks of 65 280, the middle one inside the long line: no line starts in it
    "lines/header-only": {65280: 1, 130560: 1},
}


def dump(cases, path):
    import struct
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, preset, payload, _ in cases:
            fh.write(struct.pack("<IQ", {"vcf": 0, "bed": 1}[preset], len(payload)))
            fh.write(payload)


def build_program(tmp_dir, san="address,undefined"):
    """tests/tbx_key_main.cpp as a program of its own -> its path, or None when this toolchain cannot link the sanitizers' runtime"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)

    def gxx(src, out):
        return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=" + san, "-fno-sanitize-recover=all",
                               "-I", os.path.join(root, "include"), "-I", os.path.join(root, "unfazed_amd", "csrc"), src, "-o", out],
                              capture_output=True, text=True, timeout=300)
    probe = os.path.join(str(tmp_dir), "probe.cpp")
    with open(probe, "w") as fh:
        fh.write("int main() { return 0; }\n")
    if gxx(probe, os.path.join(str(tmp_dir), "probe")).returncode != 0:
        return None
    exe = os.path.join(str(tmp_dir), "tbx_key")
    cc = gxx(os.path.join(here, "tbx_key_main.cpp"), exe)
    assert cc.returncode == 0, cc.stderr
    return exe


def run_program(exe, cases, tmp_dir, chunk):
    """-> per case its rows: (start, kind, why, name_len, bin, beg, end)"""
    import os
    import struct
    import subprocess
    src, dst = os.path.join(str(tmp_dir), "cases.bin"), os.path.join(str(tmp_dir), "out_%d.bin" % chunk)
    dump(cases, src)
    run = subprocess.run([exe, src, dst, str(chunk)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "tbx key ok" in run.stdout, run.stdout + run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        n = struct.unpack_from("<I", raw, at)[0]
        at += 4
        out.append([struct.unpack_from("<QIIIIqq", raw, at + 40 * k) for k in range(n)])
        at += 40 * n
    assert at == len(raw)
    return out
