"""Hand-built BCF2 records for the BCF-to-text line body (unfazed_amd/csrc/bcf_row.hpp, k_bcfout.hip, unfazed_amd/bcf_text.py, UZ_BCF_ROUTE).

The encoder here emits what it is told, malformed records included (tests/bcfio.py writes only well-formed ones and is not touched).  A case
holds its records' bytes, the dictionary, the contigs, the header's sample count and, per record, the EXPECTED LINE AS A LITERAL -- or the
statement "handed back", with what the plain converter makes of the record: a line, or ValueError.  Nothing a case expects is computed by the
code under test.

The same cases go to bcf_text.line, to the one-lane host program (dump -> tests/bcf_row_main.cpp), to engine.bcf_rows and to the driver."""
import random
import struct

import numpy as np

DICT = ["PASS", "q10", "DP", "AF", "DB", "SVTYPE", "END", "GT", "AD", "GQ", "FT", "PL", "", "s50"]  # (id 12 is not defined)
D = {name: i for i, name in enumerate(DICT) if name}
CONTIGS = ["chr1", "chr2", "", "chrX"]  # (id 2 is not defined)
PREFIX = b"BCF\x02\x02" + struct.pack("<I", 7) + b"header\0"  # bytes ahead of the first record, which no rule reads
I8_MISS, I8_EOV, I16_MISS, I16_EOV, I32_MISS, I32_EOV = -128, -127, -32768, -32767, -2147483648, -2147483647
F_MISS, F_EOV = 0x7F800001, 0x7F800002
INT_FMT = {1: "<b", 2: "<h", 3: "<i"}
SIZE = {0: 0, 1: 1, 2: 2, 3: 4, 5: 4, 7: 1}


# ---------------------------------------------------------------- the encoder: it emits what it is told
def tint(v, t=None):
    """a typed scalar integer, in the smallest type that holds it or in type t"""
    if t is None:
        t = 1 if -120 <= v <= 127 else 2 if -32000 <= v <= 32767 else 3
    return bytes([0x10 | t]) + struct.pack(INT_FMT[t], v)


def desc(n, t, esc=None):
    """a descriptor byte for n entries of type t; esc: the length goes through the escape whatever it is, as a typed integer of type esc"""
    if n < 15 and esc is None:
        return bytes([n << 4 | t])
    return bytes([0xF0 | t]) + tint(n, esc)


def tstr(s, esc=None):
    s = s.encode() if isinstance(s, str) else s
    return desc(len(s), 7, esc) + s


def ints(vals, t, esc=None):
    return desc(len(vals), t, esc) + b"".join(struct.pack(INT_FMT[t], v) for v in vals)


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def floats(bits, esc=None):
    return desc(len(bits), 5, esc) + b"".join(struct.pack("<I", b) for b in bits)


def fmt_ints(key, per_sample, t, count=None, key_bytes=None):
    """a FORMAT field of integers: per_sample = one list per sample, padded to `count` with end-of-vector"""
    count = max([len(v) for v in per_sample] + [0]) if count is None else count
    eov = {1: I8_EOV, 2: I16_EOV, 3: I32_EOV}[t]
    body = b"".join(struct.pack(INT_FMT[t], x) for v in per_sample for x in list(v) + [eov] * (count - len(v)))
    return (tint(D[key]) if key_bytes is None else key_bytes) + desc(count, t) + body


def fmt_floats(key, per_sample, count=None):
    count = max([len(v) for v in per_sample] + [0]) if count is None else count
    return tint(D[key]) + desc(count, 5) + b"".join(struct.pack("<I", x) for v in per_sample for x in list(v) + [F_EOV] * (count - len(v)))


def fmt_strs(key, per_sample, count=None):
    per_sample = [s.encode() if isinstance(s, str) else s for s in per_sample]
    count = max([len(s) for s in per_sample] + [0]) if count is None else count
    return tint(D[key]) + desc(count, 7) + b"".join(s + b"\0" * (count - len(s)) for s in per_sample)


def gt(text):
    """the entries of a genotype's text: "0/1", "1|0", "./.", "0/1/2", "1", "." (one entry, its allele missing)"""
    out, phased = [], 0
    tok = ""
    for ch in text + "/":
        if ch in "/|":
            out.append(((0 if tok == "." else int(tok) + 1) << 1) | phased)
            phased, tok = int(ch == "|"), ""
        else:
            tok += ch
    return out


def record(chrom=0, pos=99, rlen=1, qual=fbits(50.0), ident=None, alleles=("A", "T"), filt=None, info=(), fmt=(), n_sample=0, n_allele=None,
           n_info=None, n_fmt=None, d_shared=0, d_indiv=0):
    """one record.  ident / alleles / filt: typed bytes, or a str to encode; info: (key bytes, value bytes) pairs; fmt: whole fields (fmt_*).  The
    counts and the two block lengths say what they are told: n_* override, d_shared / d_indiv are added to the true lengths."""
    enc = lambda x: tstr(x) if isinstance(x, str) else x
    shared = struct.pack("<iiiIII", chrom, pos, rlen, qual, (len(alleles) if n_allele is None else n_allele) << 16 | (len(info) if n_info is None else n_info),
                         (len(fmt) if n_fmt is None else n_fmt) << 24 | n_sample)
    shared += enc("" if ident is None else ident) + b"".join(enc(a) for a in alleles) + (tint(0) if filt is None else filt)
    shared += b"".join(k + v for k, v in info)
    indiv = b"".join(fmt)
    return struct.pack("<II", len(shared) + d_shared, len(indiv) + d_indiv) + shared + indiv


def key(name, t=None):
    return tint(D[name], t)


BASE = "chr1\t100\t.\tA\tT\t50\tPASS\t."  # record()'s line
RAISE = "raise"


def build_cases():
    cases = []

    def add(name, records, lines, conv=None, n_samples=0, chunk=None, rec_at=None, cut=0, dict_names=None, contigs=None, file_ok=None):
        """lines[k]: the expected line, or None = handed back, then conv[k] is the converter's line or RAISE.  rec_at: given instead of end-to-end;
        cut: bytes taken off the data's end."""
        conv = dict(conv or {})
        hb = [k for k, ln in enumerate(lines) if ln is None]
        assert len(records) == len(lines) and sorted(conv) == hb, name
        cases.append({"name": name, "records": list(records), "lines": list(lines), "conv": conv, "hb": hb, "n_samples": n_samples, "chunk": chunk,
                      "rec_at": rec_at, "cut": cut, "dict": DICT if dict_names is None else dict_names, "contigs": CONTIGS if contigs is None else contigs,
                      "file_ok": (not hb and rec_at is None and not cut and dict_names is None) if file_ok is None else file_ok})

    def one(name, rec, line, conv=None, **kw):
        add(name, [rec], [line], None if line is not None else {0: conv}, **kw)

    tail = lambda t: "\t".join(BASE.split("\t")[:7]) + "\t" + t  # BASE with another INFO (and what follows)

    # ---- every column's empty form, and a full one
    one("empty/all", record(qual=F_MISS, alleles=("A",), filt=desc(0, 0)), "chr1\t100\t.\tA\t.\t.\t.\t.")
    one("empty/id", record(ident=tstr("")), BASE)
    one("empty/alt", record(alleles=("ACG",)), "chr1\t100\t.\tACG\t.\t50\tPASS\t.")
    one("empty/qual", record(qual=F_MISS), "chr1\t100\t.\tA\tT\t.\tPASS\t.")
    one("empty/filter", record(filt=desc(0, 1)), "chr1\t100\t.\tA\tT\t50\t.\t.")
    one("empty/filter_eov_first", record(filt=ints([I8_EOV, 1], 1)), "chr1\t100\t.\tA\tT\t50\t.\t.")
    one("empty/info", record(info=()), BASE)
    one("full/shared", record(chrom=3, pos=2147483646, ident="rs9;rs10", alleles=("A", "T", "<DEL>", "ACGT"), qual=fbits(0.5), filt=ints([1, 13], 1),
                              info=[(key("DP"), tint(44)), (key("DB"), desc(0, 0)), (key("AF"), floats([fbits(0.25), fbits(0.5)])), (key("SVTYPE"), tstr("DEL"))]),
        "chrX\t2147483647\trs9;rs10\tA\tT,<DEL>,ACGT\t0.5\tq10;s50\tDP=44;DB;AF=0.25,0.5;SVTYPE=DEL")
    one("pos/0", record(pos=-1), "chr1\t0\t.\tA\tT\t50\tPASS\t.")
    one("pos/max", record(pos=2147483647), "chr1\t2147483648\t.\tA\tT\t50\tPASS\t.")
    one("filter/int16", record(filt=ints([13, 0], 2)), "chr1\t100\t.\tA\tT\t50\ts50;PASS\t.")
    one("filter/eov_mid", record(filt=ints([1, I32_EOV, 0], 3)), "chr1\t100\t.\tA\tT\t50\tq10\t.")
    # ---- flags
    one("flag/type0", record(info=[(key("DB"), desc(0, 0))]), tail("DB"))
    one("flag/len0_int", record(info=[(key("DB"), desc(0, 1))]), tail("DB"))
    one("flag/type0_len3", record(info=[(key("DB"), desc(3, 0)), (key("DP"), tint(1))]), tail("DB;DP=1"))
    one("flag/two", record(info=[(key("DB"), desc(0, 0)), (key("q10"), desc(0, 7))]), tail("DB;q10"))
    # ---- integers: value, missing, end-of-vector first and mid, in each width
    for t, lo, miss, eov in ((1, -120, I8_MISS, I8_EOV), (2, -32000, I16_MISS, I16_EOV), (3, -2147483646, I32_MISS, I32_EOV)):
        hi = {1: 127, 2: 32767, 3: 2147483647}[t]
        w = {1: "int8", 2: "int16", 3: "int32"}[t]
        one("%s/value" % w, record(info=[(key("PL"), ints([0, hi, lo, -1], t))]), tail("PL=0,%d,%d,-1" % (hi, lo)))
        one("%s/missing" % w, record(info=[(key("PL"), ints([miss], t)), (key("AD"), ints([4, miss, 5], t))]), tail("PL=.;AD=4,.,5"))
        one("%s/eov_first" % w, record(info=[(key("PL"), ints([eov, 7], t))]), tail("PL=."))
        one("%s/eov_mid" % w, record(info=[(key("PL"), ints([3, eov, 7], t))]), tail("PL=3"))
        one("%s/key" % w, record(info=[(key("DP", t), tint(9, t))]), tail("DP=9"))
    # ---- typed lengths 14 / 15 / 16: 15 and 16 need the escape
    for n in (14, 15, 16):
        s = "ACGTACGTACGTACGT"[:n]
        one("len/str_%d" % n, record(ident=tstr(s), alleles=(s, "T"), info=[(key("SVTYPE"), tstr(s))]), "chr1\t100\t%s\t%s\tT\t50\tPASS\tSVTYPE=%s" % (s, s, s))
        one("len/vec_%d" % n, record(info=[(key("PL"), ints(list(range(n)), 1)), (key("AF"), floats([fbits(1.0)] * n))]),
            tail("PL=%s;AF=%s" % (",".join(str(i) for i in range(n)), ",".join(["1"] * n))))
        one("len/fmt_%d" % n, record(fmt=[fmt_ints("PL", [list(range(n)), [5]], 1), fmt_strs("FT", [s, "x"])], n_sample=2),
            BASE + "\tPL:FT\t%s:%s\t5:x" % (",".join(str(i) for i in range(n)), s), n_samples=2)
    one("len/escape_int16", record(ident=tstr("ab", esc=2)), "chr1\t100\tab\tA\tT\t50\tPASS\t.")
    one("len/escape_int32", record(info=[(key("PL"), ints([1, 2], 1, esc=3))]), tail("PL=1,2"))
    one("len/escape_of_3", record(ident=tstr("abc", esc=1)), "chr1\t100\tabc\tA\tT\t50\tPASS\t.")
    one("len/300", record(alleles=("A" * 300, "T")), "chr1\t100\t.\t%s\tT\t50\tPASS\t." % ("A" * 300))
    # ---- INFO strings
    one("str/nul_cut", record(info=[(key("SVTYPE"), tstr(b"DEL\0\x01\x01"))]), tail("SVTYPE=DEL"))
    one("str/nul_first", record(info=[(key("SVTYPE"), tstr(b"\0DEL"))]), tail("SVTYPE=."))
    one("str/edges", record(info=[(key("SVTYPE"), tstr(" ~"))]), tail("SVTYPE= ~"))
    # ---- GT
    g = lambda per, t=1, count=None: fmt_ints("GT", per, t, count)
    gt_line = lambda cells, f="GT": BASE + "\t" + f + "\t" + "\t".join(cells)
    one("gt/haploid", record(fmt=[g([gt("1"), gt("0")])], n_sample=2), gt_line(["1", "0"]), n_samples=2)
    one("gt/diploid", record(fmt=[g([gt("0/1"), gt("1/1")])], n_sample=2), gt_line(["0/1", "1/1"]), n_samples=2)
    one("gt/triploid", record(fmt=[g([gt("0/1/2"), gt("0/1")])], n_sample=2), gt_line(["0/1/2", "0/1"]), n_samples=2)
    one("gt/phased", record(fmt=[g([gt("1|0"), gt("0|1|1"), gt("0/1|2")])], n_sample=3), gt_line(["1|0", "0|1|1", "0/1|2"]), n_samples=3)
    one("gt/half_missing", record(fmt=[g([gt("./1"), gt("0/."), gt("./."), gt(".|.")])], n_sample=4), gt_line(["./1", "0/.", "./.", ".|."]), n_samples=4)
    one("gt/empty", record(fmt=[g([[], gt("0/1")])], n_sample=2), gt_line([".", "0/1"]), n_samples=2)
    one("gt/missing_marker", record(fmt=[g([[I8_MISS, 4], [2, I8_MISS]])], n_sample=2), gt_line(["./1", "0/."]), n_samples=2)
    one("gt/phase_bit_first", record(fmt=[g([[5, 2]])], n_sample=1), gt_line(["1/0"]), n_samples=1)
    one("gt/int8_allele62", record(fmt=[g([[126, 127]])], n_sample=1), gt_line(["62|62"]), n_samples=1)
    # allele 126 would be the entry 254: an int8 cannot hold it -- the byte 0xFE reads as -2, which no rule prints
    one("gt/int8_allele126", record(fmt=[g([[2, -2]])], n_sample=1), None, RAISE, n_samples=1)
    one("gt/int16_allele126", record(fmt=[g([[254, 255]], 2)], n_sample=1), gt_line(["126|126"]), n_samples=1)
    one("gt/int16_allele127", record(fmt=[g([[256, 257]], 2)], n_sample=1), gt_line(["127|127"]), n_samples=1)
    one("gt/int32", record(fmt=[g([[2000002, 4]], 3)], n_sample=1), gt_line(["1000000/1"]), n_samples=1)
    one("gt/chars", record(fmt=[fmt_strs("GT", ["0/1", "1"])], n_sample=2), gt_line(["0/1", "1"]), n_samples=2)
    one("gt/floats", record(fmt=[fmt_floats("GT", [[fbits(2.0), fbits(4.0)]])], n_sample=1), gt_line(["2,4"]), n_samples=1)
    one("gt/not_first", record(fmt=[fmt_ints("DP", [[7], [8]], 1), g([gt("0/1"), gt("1|1")])], n_sample=2), gt_line(["7:0/1", "8:1|1"], "DP:GT"), n_samples=2)
    one("gt/name_prefix", record(fmt=[fmt_ints("GQ", [[2, 4]], 1)], n_sample=1), gt_line(["2,4"], "GQ"), n_samples=1)
    # ---- per-sample values
    one("cell/strings", record(fmt=[fmt_strs("FT", ["PASS", "", "q10;s50"])], n_sample=3), BASE + "\tFT\tPASS\t.\tq10;s50", n_samples=3)
    one("cell/string_padding_unread", record(fmt=[fmt_strs("FT", [b"ab\0\x01\x7f", b"cdefg"])], n_sample=2), BASE + "\tFT\tab\tcdefg", n_samples=2)
    one("cell/floats", record(fmt=[fmt_floats("GQ", [[fbits(99.0)], [F_MISS], []]), fmt_floats("AF", [[fbits(0.5), F_MISS, fbits(0.25)], [fbits(1.0)], [F_MISS]])],
                              n_sample=3), BASE + "\tGQ:AF\t99:0.5,.,0.25\t.:1\t.:.", n_samples=3)
    one("cell/ints", record(fmt=[fmt_ints("AD", [[10, 0], [I16_MISS], []], 2), fmt_ints("DP", [[I32_MISS], [70000], [-5]], 3)], n_sample=3),
        BASE + "\tAD:DP\t10,0:.\t.:70000\t.:-5", n_samples=3)
    one("cell/type0", record(fmt=[tint(D["DB"]) + desc(0, 0), fmt_ints("DP", [[1], [2]], 1)], n_sample=2), BASE + "\tDB:DP\t.:1\t.:2", n_samples=2)
    one("cell/count0", record(fmt=[tint(D["AD"]) + desc(0, 1), fmt_ints("DP", [[1], [2]], 1)], n_sample=2), BASE + "\tAD:DP\t.:1\t.:2", n_samples=2)
    one("format/none", record(n_sample=2), BASE, n_samples=2)
    one("format/no_samples", record(fmt=[tint(D["GT"]) + desc(2, 1)], n_sample=0), BASE, n_samples=0)
    # ---- sample counts: 0, 1, and the wavefront's edges
    for ns in (0, 1, 63, 64, 65, 130):
        texts = ["0/1", "1|0", "./.", "1", "0/1/2"]
        cells = [(texts[i % 5], [i, 3 * i], "s%d" % i if i % 3 else "") for i in range(ns)]
        rec = record(fmt=[g([gt(c[0]) for c in cells]), fmt_ints("AD", [c[1] for c in cells], 2), fmt_strs("FT", [c[2] for c in cells])] if ns else (), n_sample=ns)
        one("samples/%d" % ns, rec, BASE + ("\tGT:AD:FT\t" + "\t".join("%s:%d,%d:%s" % (c[0], c[1][0], c[1][1], c[2] or ".") for c in cells) if ns else ""),
            n_samples=ns)
    # ---- record counts, and chunk edges (UZ_BCFOUT_CHUNK_BYTES)
    def many(n, ns=3):
        recs = [record(pos=10 * k, ident="id%d" % k if k % 4 else None, info=[(key("DP"), tint(k))] if k % 3 else (),
                       fmt=[g([gt("0/1"), gt("1|0") if k % 2 else gt("0/0"), gt("./.")]), fmt_ints("DP", [[k], [k + 1], [I16_MISS]], 2)], n_sample=ns) for k in range(n)]
        lines = ["chr1\t%d\t%s\tA\tT\t50\tPASS\t%s\tGT:DP\t0/1:%d\t%s:%d\t./.:." % (10 * k + 1, "id%d" % k if k % 4 else ".", "DP=%d" % k if k % 3 else ".", k,
                                                                              "1|0" if k % 2 else "0/0", k + 1) for k in range(n)]
        return recs, lines
    for n in (0, 1, 65, 257, 1025, 2049):  # (1025, 2049: past the first and the second tile of the length scan)
        add("records/%d" % n, *many(n), n_samples=3)
    recs, lines = many(9)
    t0 = len(PREFIX) & ~15
    add("chunks/after_first", recs, lines, n_samples=3, chunk=len(PREFIX) - t0 + len(recs[0]))
    add("chunks/before_last", recs, lines, n_samples=3, chunk=len(PREFIX) - t0 + sum(len(r) for r in recs) - 1)
    big = record(pos=35, alleles=("A" * 5000, "T"), fmt=[g([gt("0/1")] * 3)], n_sample=3)
    add("chunks/long_record", recs[:4] + [big] + recs[4:], lines[:4] + ["chr1\t36\t.\t%s\tT\t50\tPASS\t.\tGT\t0/1\t0/1\t0/1" % ("A" * 5000)] + lines[4:], n_samples=3,
        chunk=1024)
    add("chunks/every_record", recs, lines, n_samples=3, chunk=1)
    # ---- floats (QUAL, and the same values in an INFO vector)
    near = lambda x, d: int(np.float32(x).view(np.uint32)) + d  # the float d ulps beside float32(x)
    f_ok = [("0", fbits(0.0), "0"), ("neg0", 0x80000000, "-0"), ("1e-4", fbits(0.0001), "0.0001"), ("below_1e-4_rounds_up", near(0.0001, -1), "0.0001"),
            ("999999", fbits(999999.0), "999999"), ("999999.4375", near(999999.5, -1), "999999"), ("50", fbits(50.0), "50"), ("0.1", fbits(0.1), "0.1"),
            ("tie_even_down", fbits(125000.5), "125000"), ("tie_even_up", fbits(125001.5), "125002"), ("tie_1024.125", fbits(1024.125), "1024.12"),
            ("tie_1024.375", fbits(1024.375), "1024.38"), ("tie_exact_half", fbits(100000.5), "100000"),
            ("tie_exact_half_odd", fbits(100001.5), "100002"), ("carry", fbits(9.999995), "10"), ("carry_99999.95", fbits(99999.96), "100000"),
            ("neg", fbits(-12.5), "-12.5"), ("third", fbits(1.0 / 3), "0.333333"), ("0.000123456", fbits(0.000123456), "0.000123456"), ("123456", fbits(123456.0), "123456"),
            ("100", fbits(100.0), "100"), ("1.5", fbits(1.5), "1.5"), ("0.00099", fbits(0.00099), "0.00099")]
    f_hb = [("1e6", fbits(1e6), "1e+06"), ("999999.5", fbits(999999.5), "1e+06"), ("9.99994e-5", fbits(9.99994e-5), "9.99994e-05"), ("1e-5", fbits(1e-5), "1e-05"),
            ("inf", 0x7F800000, "inf"), ("neg_inf", 0xFF800000, "-inf"), ("nan", 0x7FC00000, "nan"), ("subnormal", 1, "1.4013e-45"), ("max", 0x7F7FFFFF, "3.40282e+38"),
            ("1e10", fbits(1e10), "1e+10")]
    for name, bits, text in f_ok:
        one("float/" + name, record(qual=bits, info=[(key("AF"), floats([bits, F_MISS, bits]))]), "chr1\t100\t.\tA\tT\t%s\tPASS\tAF=%s,.,%s" % (text, text, text))
    for name, bits, text in f_hb:
        one("float/qual_" + name, record(qual=bits), None, "chr1\t100\t.\tA\tT\t%s\tPASS\t." % text)
        one("float/info_" + name, record(info=[(key("AF"), floats([fbits(1.0), bits]))]), None, tail("AF=1,%s" % text))
    one("float/cell_1e6", record(fmt=[fmt_floats("GQ", [[fbits(3.0)], [fbits(1e6)]])], n_sample=2), None, BASE + "\tGQ\t3\t1e+06", n_samples=2)
    one("float/reserved", record(qual=F_MISS, info=[(key("AF"), floats([F_MISS, fbits(2.0), F_EOV, fbits(3.0)]))]), "chr1\t100\t.\tA\tT\t.\tPASS\tAF=.,2")
    one("float/reserved_eov_qual", record(qual=F_EOV), None, "chr1\t100\t.\tA\tT\tnan\tPASS\t.")
    # ---- one case per hand-back rule
    one("handback/no_allele", record(alleles=()), None, RAISE)
    one("handback/dict_one_beyond", record(info=[(tint(len(DICT)), tint(1))]), None, RAISE)
    one("handback/dict_undefined", record(info=[(tint(12), tint(1))]), None, RAISE)
    one("handback/dict_negative", record(filt=ints([-1], 1)), None, RAISE)
    one("handback/filter_missing", record(filt=ints([I8_MISS], 1)), None, RAISE)
    one("handback/fmt_dict_one_beyond", record(fmt=[tint(len(DICT)) + desc(1, 1) + b"\1"], n_sample=1), None, RAISE, n_samples=1)
    one("handback/contig_one_beyond", record(chrom=len(CONTIGS)), None, RAISE)
    one("handback/contig_undefined", record(chrom=2), None, RAISE)
    one("handback/contig_negative", record(chrom=-1), None, RAISE)
    one("handback/fmt_key_vector", record(fmt=[fmt_ints("DP", [[1]], 1, key_bytes=ints([D["DP"], D["DP"]], 1))], n_sample=1), None, RAISE, n_samples=1)
    one("handback/fmt_key_chars", record(fmt=[fmt_ints("DP", [[1]], 1, key_bytes=tstr("D"))], n_sample=1), None, RAISE, n_samples=1)
    one("handback/fmt_key_missing", record(fmt=[fmt_ints("DP", [[1]], 1, key_bytes=tint(I8_MISS, 1))], n_sample=1), None, RAISE, n_samples=1)
    one("handback/info_key_float", record(info=[(floats([fbits(2.0)]), tint(1))]), None, RAISE)
    for t in (4, 6, 8, 15):
        one("handback/type_%d" % t, record(info=[(key("DP"), bytes([0x10 | t, 0, 0, 0, 0, 0, 0, 0, 0]))]), None, RAISE)
    one("handback/fmt_type_6", record(fmt=[tint(D["DP"]) + bytes([0x16]) + b"\0" * 8], n_sample=1), None, RAISE, n_samples=1)
    one("handback/id_ints", record(ident=ints([65], 1)), None, RAISE)
    one("handback/allele_ints", record(alleles=(ints([65], 1), "T")), None, RAISE)
    one("handback/filter_chars", record(filt=tstr("PASS")), None, RAISE)
    one("handback/byte_1f_id", record(ident=tstr(b"rs\x1f")), None, RAISE)
    one("handback/byte_7f_info", record(info=[(key("SVTYPE"), tstr(b"DE\x7f"))]), None, RAISE)
    one("handback/byte_1f_cell", record(fmt=[fmt_strs("FT", [b"ok", b"a\x1f"])], n_sample=2), None, RAISE, n_samples=2)
    one("handback/byte_7f_cell", record(fmt=[fmt_strs("FT", [b"\x7f", b"ok"])], n_sample=2), None, RAISE, n_samples=2)
    one("handback/byte_80_allele", record(alleles=("A", b"\x17\x80")), None, RAISE)
    one("handback/tab_in_name", record(info=[(key("DP"), tint(1))]), None, RAISE, dict_names=[x.replace("DP", "D\tP") for x in DICT])
    one("handback/n_sample_differs", record(fmt=[fmt_ints("DP", [[1], [2]], 1)], n_sample=2), None, RAISE, n_samples=3)
    one("handback/length_negative", record(ident=bytes([0xF7]) + tint(-3, 1) + b"abc"), None, RAISE)
    one("handback/length_vector", record(ident=bytes([0xF7, 0x21, 3, 3]) + b"abc"), None, RAISE)
    one("handback/length_float", record(ident=bytes([0xF7, 0x15]) + struct.pack("<f", 3.0) + b"abc"), None, RAISE)
    # each bound overrun by exactly one byte: first the record that just fits, then the one that does not
    v3 = [(key("PL"), ints([1, 2, 3], 2))]
    one("bound/info_value_fits", record(info=v3), tail("PL=1,2,3"))
    one("bound/info_value_over_l_shared", record(info=v3, d_shared=-1), None, RAISE)
    one("bound/info_descriptor_at_end", record(info=v3, n_info=2), None, RAISE)
    one("bound/info_value_descriptor_at_end", record(info=[(key("PL"), b"")]), None, RAISE)
    one("bound/escape_length_over", record(info=[(key("PL"), bytes([0xF1, 0x12, 1]))]), None, RAISE)
    one("bound/escape_type_at_end", record(info=[(key("PL"), bytes([0xF1]))]), None, RAISE)
    one("bound/filter_over", record(filt=bytes([0x21, 0]), alleles=("A", "T")), None, RAISE)
    one("bound/l_shared_23", record(alleles=(), ident=b"", filt=b"", n_allele=1, d_shared=-1), None, RAISE)
    f2 = [fmt_ints("AD", [[1, 2], [3, 4]], 2)]
    one("bound/fmt_fits", record(fmt=f2, n_sample=2), BASE + "\tAD\t1,2\t3,4", n_samples=2)
    one("bound/fmt_array_over_l_indiv", record(fmt=f2, n_sample=2, d_indiv=-1), None, RAISE, n_samples=2)
    one("bound/fmt_descriptor_at_end", record(fmt=f2, n_sample=2, n_fmt=2), None, RAISE, n_samples=2)
    one("bound/fmt_no_descriptor", record(fmt=[tint(D["AD"])], n_sample=2), None, RAISE, n_samples=2)
    one("bound/fmt_huge_count", record(fmt=[tint(D["AD"]) + desc(0x7FFFFFFF, 3, esc=3)], n_sample=0xFFFFFF), None, RAISE, n_samples=0xFFFFFF)
    one("bound/data_end_fits", record(info=v3), tail("PL=1,2,3"), cut=0, file_ok=False)
    one("bound/data_end_over", record(info=v3), None, RAISE, cut=1)
    one("bound/l_indiv_over_data", record(info=v3, d_indiv=1), None, RAISE)
    one("bound/header_over_data", record()[:7], None, RAISE)
    add("bound/rec_at_is_data_end", [record(), b""], [BASE, None], {1: RAISE})
    # ---- handed-back records first, last, adjacent, all
    bad, good = record(qual=fbits(1e6)), record(pos=7)
    bad_line, good_line = "chr1\t100\t.\tA\tT\t1e+06\tPASS\t.", "chr1\t8\t.\tA\tT\t50\tPASS\t."
    for name, pat in (("first", "bgg"), ("last", "ggb"), ("adjacent", "gbbg"), ("all", "bbb"), ("alternate", "bgbgb")):
        add("handback/" + name, [bad if ch == "b" else good for ch in pat], [None if ch == "b" else good_line for ch in pat],
            {k: bad_line for k, ch in enumerate(pat) if ch == "b"}, chunk=64 if name == "adjacent" else None)
    return cases


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---------------------------------------------------------------- what the code under test is given, and what it is held to
def layout(case):
    """-> (data bytes, rec_at uint64 [n])"""
    data, at = bytearray(PREFIX), []
    for r in case["records"]:
        at.append(len(data))
        data += r
    if case["rec_at"] is not None:
        at = list(case["rec_at"])
    if case["cut"]:
        del data[-case["cut"]:]
    return bytes(data), np.asarray(at, np.uint64)


def expected(case):
    """-> per record: the line's bytes with its '\\n' (b"" for a record handed back), and where column 10 starts in it"""
    out = []
    for ln in case["lines"]:
        if ln is None:
            out.append((b"", 0))
            continue
        cols = ln.split("\t")
        out.append((ln.encode("latin-1") + b"\n", len("\t".join(cols[:9])) + 1 if len(cols) > 9 else len(ln)))
    return out


def converter_holds(case, line_fn):
    """bcf_text.line over the case: every expected line, and for the records handed back the stated line or ValueError"""
    data, rec_at = layout(case)
    for k, ln in enumerate(case["lines"]):
        want = ln if ln is not None else case["conv"][k]
        try:
            got = line_fn(data, int(rec_at[k]), case["dict"], case["contigs"], case["n_samples"], index=k)
        except ValueError as e:
            got = RAISE
            assert str(k) in str(e), (case["name"], k, e)
        assert got == want, (case["name"], k, got, want)


def header_lines(case, samples=None):
    """the header of a case's file: the dictionary and the contigs defined by IDX, undefined ids left out"""
    samples = ["s%d" % i for i in range(case["n_samples"])] if samples is None else samples
    lines = ["##fileformat=VCFv4.2"]
    kind = {"PASS": "FILTER", "q10": "FILTER", "s50": "FILTER", "GT": "FORMAT", "AD": "FORMAT", "GQ": "FORMAT", "FT": "FORMAT", "PL": "FORMAT"}
    for i, name in enumerate(case["dict"]):
        if name:
            k = kind.get(name, "INFO")
            lines.append('##%s=<ID=%s,%sDescription="x",IDX=%d>' % (k, name, "" if k == "FILTER" else "Number=.,Type=String,", i))
            if name in ("DP", "AF"):  # (used as INFO and as FORMAT)
                lines.append('##FORMAT=<ID=%s,Number=.,Type=String,Description="x",IDX=%d>' % (name, i))
    lines += ["##contig=<ID=%s,IDX=%d>" % (c, i) for i, c in enumerate(case["contigs"]) if c]
    lines.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] + (["FORMAT"] + samples if samples else [])))
    return lines


def file_bytes(case, samples=None):
    """a whole BCF of a case whose records a decoder takes (case["file_ok"]): BGZF framed"""
    from unfazed_amd.io_bam import _bgzf_block
    assert case["file_ok"], case["name"]
    text = ("\n".join(header_lines(case, samples)) + "\n").encode() + b"\0"
    data = b"BCF\x02\x02" + struct.pack("<I", len(text)) + text + b"".join(case["records"])
    return b"".join(_bgzf_block(data[i:i + 60000]) for i in range(0, len(data), 60000)) + _bgzf_block(b"")


def text_file_bytes(case, lines=None, samples=None):
    """the text VCF that holds the case's header and its expected lines (or `lines`): what the host writer is run on for the expectation"""
    lines = case["lines"] if lines is None else lines
    return ("\n".join(header_lines(case, samples) + list(lines)) + "\n").encode()


def route_records(case, lines=None):
    """a read_records dict that annotates the first and the last sample at every record of the case.  A record's key is entered under both ends
    it can have: the table's pos + rlen (the panel's rlen is 1) and the text's start + len(REF)."""
    from vcfrowcases import rec
    out, ns = {}, case["n_samples"]
    for k, ln in enumerate(case["lines"] if lines is None else lines):
        f = ln.split("\t")
        start = int(f[1]) - 1
        vt = ([kv[7:] for kv in f[7].split(";") if kv.startswith("SVTYPE=")] + ["POINT"])[0]
        for end in {start + 1, start + len(f[3])}:
            for kid, nd, nm in (("s0", 2 + k % 3, 0), ("s%d" % (ns - 1), 0, 1 + k % 2)):
                key, r = rec(kid, start, end, chrom=f[0], vartype=vt, nd=nd, nm=nm)
                out.setdefault(key, r)
    return out


def host_writer(path_in, path_out, records, route_env, monkeypatch):
    """unfazed.write_vcf_output under the environment route_env -> ("text", bytes) or ("raise", type)"""
    from unfazed_amd import unfazed
    for k in ("UZ_BCF_ROUTE", "UZ_VCF_ROUTE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in route_env.items():
        monkeypatch.setenv(k, v)
    try:
        unfazed.write_vcf_output(path_in, records, False, False, path_out, 10)
    except SystemExit:
        raise
    except Exception as e:  # noqa: BLE001 -- compared between the routes
        return ("raise", type(e))
    finally:
        for k in route_env:
            monkeypatch.delenv(k, raising=False)
    return ("text", open(path_out, "rb").read())


def dump(cases, path):
    """the cases with what they expect, for tests/bcf_row_main.cpp: int64 case count; per case int64 n, n_samples, then arrays (int64 byte count,
    bytes, padding to 8): data, rec_at i64, dict_off u32, dict_bytes, contig_off u32, contig_bytes, exp_off i64, exp, exp_hb u8, exp_samp i64"""
    def arr(a, dtype):
        b = np.ascontiguousarray(a, dtype).tobytes()
        return struct.pack("<q", len(b)) + b + b"\0" * (-len(b) % 8)

    def names(ns):
        blobs = [x.encode("latin-1") if isinstance(x, str) else x for x in ns]
        return arr(np.cumsum([0] + [len(b) for b in blobs]), np.uint32) + arr(np.frombuffer(b"".join(blobs), np.uint8), np.uint8)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)))
        for c in cases:
            data, rec_at = layout(c)
            exp = expected(c)
            fh.write(struct.pack("<qq", len(rec_at), c["n_samples"]) + arr(np.frombuffer(data, np.uint8), np.uint8) + arr(rec_at, np.int64))
            fh.write(names(c["dict"]) + names(c["contigs"]))
            fh.write(arr(np.cumsum([0] + [len(e[0]) for e in exp]), np.int64) + arr(np.frombuffer(b"".join(e[0] for e in exp), np.uint8), np.uint8))
            fh.write(arr([int(ln is None) for ln in c["lines"]], np.uint8) + arr([e[1] for e in exp], np.int64))


# ---------------------------------------------------------------- the seeded fuzz: the TEXT first, then its encoding
def _f32_text(x):
    return "%g" % float(np.float32(x))


def fuzz_cases(seed, n_records, per_case=40):
    """cases of random records.  A record's text is made first and then encoded, with random widths, escapes and paddings; expected = that text.
    Floats: expected = "%g" % float(np.float32(x)).  Every record carries the builder's own statement of whether it holds a handed-back
    ingredient (an exponent-form float, an infinity or NaN, a byte outside the printable range, an id without a name, a negative GT entry): the
    handed-back set must EQUAL that statement."""
    rng = random.Random(seed)
    cases = []

    def some_float(hb_ok):
        r = rng.random()
        if hb_ok and r < 0.5:
            return rng.choice([1e6, 2.5e7, 1e-5, 3.3e-9, float("inf"), float("-inf"), float("nan"), 999999.5, 9.9999e-5])
        if r < 0.3:
            return float(rng.randrange(0, 1000))
        if r < 0.5:
            return rng.randrange(-9999, 9999) / 10.0
        if r < 0.7:
            return rng.randrange(1, 99999) / 1e7 + 1e-4
        if r < 0.9:
            return rng.uniform(1e-4, 999999.0)
        return rng.choice([0.0, -0.0, 1e-4, 999999.0, 9.999995, 99999.95, 0.1])

    def width(vals):
        lo = min([v for v in vals] + [0])
        hi = max([v for v in vals] + [0])
        t = 1 if -120 <= lo and hi <= 127 else 2 if -32000 <= lo and hi <= 32767 else 3
        return rng.randrange(t, 4)

    def enc_ints(text, t=None, count=None):  # "1,.,3" or "."
        vals = [] if text == "." and rng.random() < 0.5 else [None if x == "." else int(x) for x in text.split(",")]
        t = width([v for v in vals if v is not None]) if t is None else t
        miss, eov = {1: (I8_MISS, I8_EOV), 2: (I16_MISS, I16_EOV), 3: (I32_MISS, I32_EOV)}[t]
        return [miss if v is None else v for v in vals], t, eov

    remaining = n_records
    while remaining > 0:
        n = min(per_case, remaining)
        remaining -= n
        ns = rng.choice([0, 1, 2, 3, 5, 8, 64, 65, 70])
        fmt_keys = rng.sample(["GT", "AD", "GQ", "FT", "DP"], rng.randrange(0, 5)) if ns else []
        records, lines, conv = [], [], {}
        for k in range(n):
            hb = rng.random() < 0.12
            why = rng.choice(["float", "float", "byte", "contig", "dict", "gt" if "GT" in fmt_keys else "float"]) if hb else None
            raises = why in ("byte", "contig", "dict", "gt")
            chrom = rng.choice([0, 1, 3])
            pos = rng.randrange(0, 1 << 28)
            ident = rng.choice(["", "rs%d" % rng.randrange(1 << 20), "a;b"])
            ref = "".join(rng.choice("ACGT") for _ in range(rng.choice([1, 1, 2, 15, 16, 40])))
            alts = ["".join(rng.choice("ACGT") for _ in range(rng.choice([1, 1, 3, 20]))) for _ in range(rng.randrange(0, 4))]
            qx = None if rng.random() < 0.3 else some_float(why == "float")
            filt = rng.choice([[], [0], [1, 13], [13]])
            info, info_b = [], []
            for name in rng.sample(["DP", "AF", "DB", "SVTYPE", "END"], rng.randrange(0, 5)):
                if name == "DB":
                    info.append("DB"); info_b.append((key("DB", rng.randrange(1, 4)), desc(0, rng.choice([0, 1, 7]))))
                elif name in ("DP", "END"):
                    v = rng.randrange(-50000, 5000000)
                    info.append("%s=%d" % (name, v)); info_b.append((key(name), tint(v, width([v]))))
                elif name == "AF":
                    xs = [some_float(why == "float") for _ in range(rng.randrange(1, 4))]
                    info.append("AF=" + ",".join(_f32_text(x) for x in xs))
                    info_b.append((key("AF"), floats([fbits(x) for x in xs] + [F_EOV] * rng.randrange(0, 2), esc=rng.choice([None, None, 1, 2]))))
                else:
                    s = rng.choice(["DEL", "DUP", "INS", "x" * 15, "y" * 16])
                    info.append("SVTYPE=" + s); info_b.append((key("SVTYPE"), tstr(s.encode() + b"\0" * rng.randrange(0, 3))))
            cells, fields = [[] for _ in range(ns)], []
            for name in fmt_keys:
                if name == "GT":
                    texts = [rng.choice(["0/1", "1|0", "./.", ".", "1", "0/1/2", "0|.", "12/3", "0/0"]) for _ in range(ns)]
                    t = rng.randrange(1, 4)
                    fields.append(fmt_ints("GT", [[] if x == "." and rng.random() < 0.5 else gt(x) for x in texts], t, count=3 + rng.randrange(0, 2)))
                elif name in ("AD", "DP"):
                    texts = [rng.choice([".", "%d" % rng.randrange(300), "%d,%d" % (rng.randrange(300), rng.randrange(70000)), "3,.,%d" % rng.randrange(-9, 9)]) for _ in range(ns)]
                    t = 3 if name == "AD" else rng.choice([2, 3])
                    t = 3
                    fields.append(fmt_ints(name, [enc_ints(x, t)[0] for x in texts], t, count=3 + rng.randrange(0, 13)))
                elif name == "GQ":
                    xs = [[some_float(False) for _ in range(rng.randrange(0, 3))] for _ in range(ns)]
                    texts = [",".join(_f32_text(x) for x in v) or "." for v in xs]
                    fields.append(fmt_floats("GQ", [[fbits(x) for x in v] if v or rng.random() < 0.5 else [F_MISS] for v in xs], count=2 + rng.randrange(0, 2)))
                else:
                    texts = [rng.choice([".", "PASS", "q10;s50", "lowGQ"]) for _ in range(ns)]
                    fields.append(fmt_strs("FT", ["" if x == "." else x for x in texts], count=7 + rng.randrange(0, 10)))
                for s in range(ns):
                    cells[s].append(texts[s])
            cols = [CONTIGS[chrom], str(pos + 1), ident or ".", ref, ",".join(alts) or ".", "." if qx is None else _f32_text(qx), ";".join(DICT[i] for i in filt) or ".",
                    ";".join(info) or "."]
            if fmt_keys:
                cols += [":".join(fmt_keys)] + [":".join(c) for c in cells]
            text = "\t".join(cols)
            if why == "float" and "e" not in text.split("\t", 5)[5] and "inf" not in text and "nan" not in text:  # (no float came out in exponent form)
                qx = 2.5e7
                cols[5] = _f32_text(qx)
                text = "\t".join(cols)
            ident_b = tstr(ident, esc=rng.choice([None, None, 1, 3]))
            if why == "byte":
                ident_b = tstr(rng.choice([b"\x1f", b"a\x7f", b"\x80b", b"\tq"]))
            if why == "contig":
                chrom = rng.choice([2, 4, -1, 1000])
            if why == "dict":
                info_b.append((tint(rng.choice([12, len(DICT), -2, 30000])), tint(1)))
            if why == "gt":
                fields[fmt_keys.index("GT")] = fmt_ints("GT", [[2, -2]] * ns, 1, count=2)
            records.append(record(chrom=chrom, pos=pos, qual=F_MISS if qx is None else fbits(qx), ident=ident_b, alleles=[ref] + alts,
                                  filt=ints(filt, width(filt)) if filt or rng.random() < 0.5 else desc(0, 0), info=info_b, fmt=fields, n_sample=ns))
            lines.append(None if hb else text)
            if hb:
                conv[k] = RAISE if raises else text
        cases.append({"name": "fuzz/%d" % len(cases), "records": records, "lines": lines, "conv": conv, "hb": sorted(conv), "n_samples": ns, "chunk": None,
                      "rec_at": None, "cut": 0, "dict": DICT, "contigs": CONTIGS, "file_ok": False})
    return cases
