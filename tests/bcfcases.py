"""A hand-built edge table for the per-sample FORMAT values of a BCF, and the BCF writers its tests need (tests/test_bcf_cell.py,
test_bcf_lazy.py, test_bcf_device_gpu.py; tests/bcfio.py writes GT:AD:GQ in one shape only).

A case is one record: its FORMAT fields -- (key, BCF type, values per sample) in file order -- and a few sample cells.  A cell gives, field by
field, the raw entries of that sample -- integers, floats, M (the type's missing marker), E (its end-of-vector marker) or ("bits", pattern) --
the values the DECODER holds for it (gt code, int depths, float GQ: the semantics of unfazed_amd/io_vcf.py, read off the BCF2 rules by hand,
never back from the code) and a label:
  plain      the device's body (unfazed_amd/csrc/bcf_cell.hpp) settles it
  unsettled  it goes back to the host: a depth above 32767 or below 0, or a field in a type the kernel does not take
The rules: GT entry x -> allele (x >> 1) - 1, below 0 = missing, only the first two entries before end-of-vector are read, one entry = haploid
(homozygous), a half-missing call counts with its called allele; AD's first two entries, a missing first entry followed by end-of-vector (or
by nothing) is the text form's bare "." and falls through to RO / AO when the record has both; GQ's first entry, float or integer.

A record repeats the case's cells cyclically over the file's NS samples, so that any pick of samples meets every cell.  `pack_raises`: the
cell's depths cannot be packed (ValueError) -- such cases stand in no file that must go through the product, only in the cell test and the
error test."""
import math
import struct

import numpy as np

from unfazed_amd.io_bam import _bgzf_block

NS = 70
SAMPLES = ["s%03d" % i for i in range(NS)]
P, U = "plain", "unsettled"
M, E = "missing", "end-of-vector"
INT8, INT16, INT32, FLOAT, CHAR = 1, 2, 3, 5, 7
SIZE = {INT8: 1, INT16: 2, INT32: 4, FLOAT: 4, CHAR: 1}
KEYS = ["GT", "AD", "RO", "AO", "GQ", "DP", "PL", "XX"]  # the FORMAT keys of the header: dictionary ids 1 .. 8 (PASS is 0)
NAN = float("nan")
F32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]  # noqa: E731  (what a float32 holds of x)


def _c(name, fields, cells, **kw):
    return dict(name=name, fields=fields, cells=cells, **kw)


GT2, GT1, GT3 = ("GT", INT8, 2), ("GT", INT8, 1), ("GT", INT8, 3)
HET = [2, 4]  # 0/1

CASES = [
    # ---- GT: (allele + 1) << 1 | phased
    _c("gt_int8_diploid", [GT2], [([[2, 2]], (0, -1, -1, -1.0), P), ([[2, 4]], (1, -1, -1, -1.0), P), ([[4, 2]], (1, -1, -1, -1.0), P), ([[4, 4]], (3, -1, -1, -1.0), P),
                                  ([[4, 6]], (1, -1, -1, -1.0), P), ([[6, 6]], (3, -1, -1, -1.0), P)]),
    _c("gt_phased_bit", [GT2], [([[2, 5]], (1, -1, -1, -1.0), P), ([[4, 5]], (3, -1, -1, -1.0), P), ([[2, 3]], (0, -1, -1, -1.0), P), ([[3, 4]], (1, -1, -1, -1.0), P)]),
    _c("gt_one_entry", [GT1], [([[2]], (0, -1, -1, -1.0), P), ([[4]], (3, -1, -1, -1.0), P), ([[0]], (2, -1, -1, -1.0), P), ([[M]], (2, -1, -1, -1.0), P),
                               ([[E]], (2, -1, -1, -1.0), P), ([[6]], (3, -1, -1, -1.0), P)]),
    _c("gt_three_entries", [GT3], [([[2, 2, 4]], (0, -1, -1, -1.0), P), ([[2, 4, 4]], (1, -1, -1, -1.0), P), ([[4, 4, 2]], (3, -1, -1, -1.0), P),
                                   ([[0, 0, 0]], (2, -1, -1, -1.0), P), ([[2, E, E]], (0, -1, -1, -1.0), P), ([[4, E, E]], (3, -1, -1, -1.0), P),
                                   ([[2, 4, E]], (1, -1, -1, -1.0), P)]),
    _c("gt_haploid_padded", [GT2], [([[4, E]], (3, -1, -1, -1.0), P), ([[2, E]], (0, -1, -1, -1.0), P), ([[0, E]], (2, -1, -1, -1.0), P), ([[E, E]], (2, -1, -1, -1.0), P),
                                    ([[M, E]], (2, -1, -1, -1.0), P)]),
    _c("gt_missing", [GT2], [([[0, 0]], (2, -1, -1, -1.0), P), ([[M, M]], (2, -1, -1, -1.0), P), ([[0, 1]], (2, -1, -1, -1.0), P), ([[1, 1]], (2, -1, -1, -1.0), P)]),
    _c("gt_half_missing", [GT2], [([[0, 2]], (0, -1, -1, -1.0), P), ([[0, 4]], (1, -1, -1, -1.0), P), ([[2, 0]], (0, -1, -1, -1.0), P), ([[4, 1]], (1, -1, -1, -1.0), P),
                                  ([[M, 4]], (1, -1, -1, -1.0), P), ([[2, M]], (0, -1, -1, -1.0), P)]),
    _c("gt_int16_allele_127", [("GT", INT16, 2)], [([[256, 256]], (3, -1, -1, -1.0), P), ([[2, 256]], (1, -1, -1, -1.0), P), ([[600, 2]], (1, -1, -1, -1.0), P),
                                                   ([[M, 2]], (0, -1, -1, -1.0), P), ([[256, E]], (3, -1, -1, -1.0), P), ([[257, 259]], (1, -1, -1, -1.0), P)]),
    _c("gt_int32", [("GT", INT32, 2)], [([[2, 4]], (1, -1, -1, -1.0), P), ([[M, M]], (2, -1, -1, -1.0), P), ([[70000, 70000]], (3, -1, -1, -1.0), P), ([[4, E]], (3, -1, -1, -1.0), P)]),
    _c("gt_negative_entries", [GT2], [([[-3, 2]], (0, -1, -1, -1.0), P), ([[-3, -5]], (2, -1, -1, -1.0), P)]),
    # ---- AD
    _c("ad_int8", [GT2, ("AD", INT8, 2)], [([HET, [5, 3]], (1, 5, 3, -1.0), P), ([HET, [0, 0]], (1, 0, 0, -1.0), P), ([HET, [127, 1]], (1, 127, 1, -1.0), P),
                                           ([HET, [M, 3]], (1, -1, 3, -1.0), P), ([HET, [5, M]], (1, 5, -1, -1.0), P), ([HET, [M, M]], (1, -1, -1, -1.0), P)]),
    _c("ad_int16_three", [GT2, ("AD", INT16, 3)], [([HET, [300, 200, 7]], (1, 300, 200, -1.0), P), ([HET, [32767, 32767, 0]], (1, 32767, 32767, -1.0), P),
                                                   ([HET, [9, E, E]], (1, 9, -1, -1.0), P), ([HET, [M, E, E]], (1, -1, -1, -1.0), P), ([HET, [M, 4, E]], (1, -1, 4, -1.0), P)]),
    _c("ad_int32_one", [GT2, ("AD", INT32, 1)], [([HET, [9]], (1, 9, -1, -1.0), P), ([HET, [M]], (1, -1, -1, -1.0), P), ([HET, [E]], (1, -1, -1, -1.0), P),
                                                 ([HET, [32767]], (1, 32767, -1, -1.0), P)]),
    _c("ad_second_end_of_vector", [GT2, ("AD", INT8, 2)], [([HET, [9, E]], (1, 9, -1, -1.0), P), ([HET, [0, E]], (1, 0, -1, -1.0), P)]),
    _c("ad_dot_ro_ao", [GT2, ("AD", INT8, 2), ("RO", INT8, 1), ("AO", INT8, 1)],
       [([HET, [M, E], [12], [7]], (1, 12, 7, -1.0), P), ([HET, [3, 4], [12], [7]], (1, 3, 4, -1.0), P), ([HET, [M, E], [M], [7]], (1, -1, 7, -1.0), P),
        ([HET, [M, M], [12], [7]], (1, -1, -1, -1.0), P), ([HET, [E, E], [12], [7]], (1, 12, 7, -1.0), P), ([HET, [M, E], [12], [E]], (1, 12, -1, -1.0), P),
        ([HET, [E, 4], [12], [7]], (1, -1, 4, -1.0), P)]),
    _c("ad_one_entry_dot_ro_ao", [GT2, ("AD", INT16, 1), ("RO", INT16, 1), ("AO", INT32, 2)],
       [([HET, [M], [30], [2, 9]], (1, 30, 2, -1.0), P), ([HET, [8], [30], [2, 9]], (1, 8, -1, -1.0), P), ([HET, [M], [300], [M, E]], (1, 300, -1, -1.0), P)]),
    _c("ad_dot_no_ro_ao", [GT2, ("AD", INT16, 2)], [([HET, [M, E]], (1, -1, -1, -1.0), P), ([HET, [6, 2]], (1, 6, 2, -1.0), P)]),
    _c("ad_dot_ro_without_ao", [GT2, ("AD", INT8, 2), ("RO", INT8, 1)], [([HET, [M, E], [12]], (1, -1, -1, -1.0), P), ([HET, [1, 2], [12]], (1, 1, 2, -1.0), P)]),
    _c("ro_ao_only", [GT2, ("RO", INT16, 1), ("AO", INT16, 2)], [([HET, [30], [2, 9]], (1, 30, 2, -1.0), P), ([HET, [M], [M, E]], (1, -1, -1, -1.0), P),
                                                                 ([HET, [400], [E, E]], (1, 400, -1, -1.0), P)]),
    # ---- depth edge values
    _c("depth_32767", [GT2, ("AD", INT16, 2)], [([HET, [32767, 1]], (1, 32767, 1, -1.0), P), ([HET, [1, 32767]], (1, 1, 32767, -1.0), P)]),
    _c("depth_32768", [GT2, ("AD", INT32, 2)], [([HET, [32768, 1]], (1, 32768, 1, -1.0), U), ([HET, [1, 32768]], (1, 1, 32768, -1.0), U), ([HET, [1, 1]], (1, 1, 1, -1.0), P)]),
    _c("depth_two_to_30", [GT2, ("AD", INT32, 2)], [([HET, [1 << 30, 5]], (1, 1 << 30, 5, -1.0), U), ([HET, [6, 5]], (1, 6, 5, -1.0), P)]),
    _c("depth_32768_in_ro", [GT2, ("RO", INT32, 1), ("AO", INT32, 1)], [([HET, [40000], [3]], (1, 40000, 3, -1.0), U), ([HET, [4], [3]], (1, 4, 3, -1.0), P)]),
    _c("depth_minus_one", [GT2, ("AD", INT8, 2)], [([HET, [-1, 5]], (1, -1, 5, -1.0), U), ([HET, [5, -1]], (1, 5, -1, -1.0), U), ([HET, [5, 5]], (1, 5, 5, -1.0), P)]),
    _c("depth_minus_five", [GT2, ("AD", INT8, 2)], [([HET, [-5, 5]], (1, -5, 5, -1.0), U)], pack_raises=True),
    # ---- GQ
    _c("gq_float", [GT2, ("GQ", FLOAT, 1)], [([HET, [99.9]], (1, -1, -1, F32(99.9)), P), ([HET, [40000.0]], (1, -1, -1, 40000.0), P), ([HET, [0.0]], (1, -1, -1, 0.0), P),
                                             ([HET, [20.0]], (1, -1, -1, 20.0), P), ([HET, [32767.5]], (1, -1, -1, 32767.5), P), ([HET, [0.99]], (1, -1, -1, F32(0.99)), P)]),
    _c("gq_float_reserved", [GT2, ("GQ", FLOAT, 1)], [([HET, [M]], (1, -1, -1, -1.0), P), ([HET, [E]], (1, -1, -1, -1.0), P), ([HET, [NAN]], (1, -1, -1, NAN), P),
                                                      ([HET, [-1.0]], (1, -1, -1, -1.0), P), ([HET, [-0.5]], (1, -1, -1, -0.5), P), ([HET, [float("inf")]], (1, -1, -1, float("inf")), P),
                                                      ([HET, [float("-inf")]], (1, -1, -1, float("-inf")), P), ([HET, [("bits", 0x7F800003)]], (1, -1, -1, NAN), P),
                                                      ([HET, [-0.0]], (1, -1, -1, -0.0), P)]),
    _c("gq_int8", [GT2, ("GQ", INT8, 1)], [([HET, [40]], (1, -1, -1, 40.0), P), ([HET, [M]], (1, -1, -1, -1.0), P), ([HET, [E]], (1, -1, -1, -1.0), P),
                                           ([HET, [-3]], (1, -1, -1, -3.0), P), ([HET, [127]], (1, -1, -1, 127.0), P), ([HET, [0]], (1, -1, -1, 0.0), P)]),
    _c("gq_int16", [GT2, ("GQ", INT16, 1)], [([HET, [300]], (1, -1, -1, 300.0), P), ([HET, [32767]], (1, -1, -1, 32767.0), P), ([HET, [M]], (1, -1, -1, -1.0), P)]),
    _c("gq_int32_above_the_clamp", [GT2, ("GQ", INT32, 1)], [([HET, [40000]], (1, -1, -1, 40000.0), P), ([HET, [99]], (1, -1, -1, 99.0), P)]),
    _c("gq_float_two_entries", [GT2, ("GQ", FLOAT, 2)], [([HET, [55.5, 1.0]], (1, -1, -1, 55.5), P), ([HET, [M, 7.0]], (1, -1, -1, -1.0), P)]),
    # ---- records and fields
    _c("no_format_fields", [], []),
    _c("all_three", [GT2, ("AD", INT8, 2), ("GQ", FLOAT, 1)], [([[2, 2], [30, 0], [60.0]], (0, 30, 0, 60.0), P), ([HET, [14, 15], [99.0]], (1, 14, 15, 99.0), P),
                                                               ([[4, 4], [0, 28], [75.5]], (3, 0, 28, 75.5), P), ([[0, 0], [M, E], [M]], (2, -1, -1, -1.0), P)]),
    _c("other_fields_around", [("DP", INT8, 1), GT2, ("PL", INT16, 16), ("AD", INT16, 2), ("XX", FLOAT, 2), ("GQ", INT8, 1)],
       [([[33], HET, list(range(100, 116)), [20, 13], [1.5, 2.5], [50]], (1, 20, 13, 50.0), P),
        ([[M], [4, 4], [M] + [E] * 15, [0, 41], [M, E], [M]], (3, 0, 41, -1.0), P)]),
    _c("other_fields_only", [("DP", INT16, 1), ("PL", INT32, 15)], [([[7], list(range(15))], (2, -1, -1, -1.0), P)]),
    _c("gt_as_characters", [("GT", CHAR, 3), ("AD", INT8, 2), ("GQ", INT8, 1)], [([[ord("0"), ord("/"), ord("1")], [5, 3], [40]], (2, 5, 3, 40.0), U),
                                                                                 ([[ord("1"), ord("/"), ord("1")], [1, 9], [M]], (2, 1, 9, -1.0), U)]),
    _c("ad_as_floats", [GT2, ("AD", FLOAT, 2)], [([HET, [5.0, 3.0]], (1, -1, -1, -1.0), U)]),
    _c("gq_as_characters", [GT2, ("GQ", CHAR, 2)], [([HET, [ord("4"), ord("0")]], (1, -1, -1, -1.0), U)]),
]

FILE_CASES = [c for c in CASES if not c.get("pack_raises")]


def record_cells(case):
    """the NS cells of a case's record: [(raw entries per field, decoder values, label)]"""
    cells = case["cells"]
    if not cells:
        return [(None, (2, -1, -1, -1.0), P)] * NS
    return [cells[s % len(cells)] for s in range(NS)]


def unsettled_records(used, pick):
    """records with an `unsettled` cell in a picked sample"""
    return [i for i, c in enumerate(used) if any(record_cells(c)[s][2] == U for s in set(pick))]


def packed(values):
    """a cell's decoder values under the pack rules (uz_samples_pack), by hand: (gt, rd, ad, gq) in the 16-bit encoding"""
    gt, rd, ad, gq = values
    d16 = lambda d: 0xFFFF if d < 0 else min(d, 32767)  # noqa: E731
    g = math.floor(gq) if not (math.isnan(gq) or math.isinf(gq)) else gq
    return gt, d16(rd), d16(ad), (0xFFFF if not (g >= 0) else 32767 if g > 32767 else int(g))


# ------------------------------------------------------------------------------------------------ writing
_MISSING = {INT8: 0x80, INT16: 0x8000, INT32: 0x80000000, FLOAT: 0x7F800001, CHAR: 0}
_FMT = {INT8: "<b", INT16: "<h", INT32: "<i", FLOAT: "<f", CHAR: "<B"}
_UFMT = {INT8: "<B", INT16: "<H", INT32: "<I", FLOAT: "<I", CHAR: "<B"}


def entry_bytes(t, x):
    if x is M:
        return struct.pack(_UFMT[t], _MISSING[t])
    if x is E:
        return struct.pack(_UFMT[t], _MISSING[t] + 1)
    if isinstance(x, tuple):
        return struct.pack(_UFMT[t], x[1])
    return struct.pack(_FMT[t], x)


def _typed_int(v):
    if -120 <= v <= 127:
        return bytes([0x11]) + struct.pack("<b", v)
    if -32000 <= v <= 32767:
        return bytes([0x12]) + struct.pack("<h", v)
    return bytes([0x13]) + struct.pack("<i", v)


def _descriptor(n, t):
    if n < 15:
        return bytes([(n << 4) | t])
    return bytes([0xF0 | t]) + _typed_int(n)  # the long form: the count follows as a typed integer


def _typed_str(s):
    b = s.encode()
    return _descriptor(len(b), 7) + b


def header_bytes(samples, contigs):
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed">'] + ["##contig=<ID=%s>" % c for c in contigs]
    lines += ['##FORMAT=<ID=%s,Number=.,Type=String,Description="%s">' % (k, k) for k in KEYS]
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples))
    text = ("\n".join(lines) + "\n").encode() + b"\0"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


def _shared(chrom, pos0, n_fmt, n_samples):
    s = struct.pack("<iiifII", chrom, pos0, 1, 50.0, (2 << 16) | 0, (n_fmt << 24) | n_samples)
    return s + bytes([0x07]) + _typed_str("A") + _typed_str("G") + bytes([0x11, 0x00])  # ID ".", REF, ALT, FILTER PASS


def record_bytes(case, pos0, chrom=0, truncate=0):
    """one record of the table's BCF; truncate: bytes cut off the end of its FORMAT block (l_indiv says so too: the record itself is whole)"""
    cells = record_cells(case)
    indiv = b""
    for f, (key, t, n) in enumerate(case["fields"]):
        indiv += _typed_int(1 + KEYS.index(key)) + _descriptor(n, t)
        for raw, _, _ in cells:
            assert len(raw[f]) == n, (case["name"], key)
            indiv += b"".join(entry_bytes(t, x) for x in raw[f])
    if truncate:
        indiv = indiv[:-truncate]
    shared = _shared(chrom, pos0, len(case["fields"]), NS)
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


def bcf_bytes(n_records, cases=None, truncate_last=0):
    """the table's BCF: n_records records that run through `cases` (FILE_CASES) cyclically, 10 bases apart on chr1 -> (bytes, the case of every record)"""
    cases = FILE_CASES if cases is None else cases
    used = [cases[i % len(cases)] for i in range(n_records)]
    out = bytearray(header_bytes(SAMPLES, ["chr1"]))
    for i, c in enumerate(used):
        out += record_bytes(c, 100 + 10 * i, truncate=truncate_last if i == n_records - 1 else 0)
    return bytes(out), used


def write_bgzf(path, data, block_bytes=60000):
    with open(path, "wb") as fh:
        for i in range(0, len(data), block_bytes):
            fh.write(_bgzf_block(data[i: i + block_bytes]))
        fh.write(_bgzf_block(b""))


def write_indexed(path, data, block_bytes=60000):
    from filesio import write_csi
    write_bgzf(path, data, block_bytes)
    write_csi(path)
    return path


def table_bcf_bytes(samples, contigs, chrom, pos0, gt, ad, gq, ref=None, alt=None):
    """A plain cohort BCF built with numpy, record rows at once: GT int8 [n][ns][2] (BCF-coded entries), AD int16 [n][ns][2] (-1: missing),
    GQ float32 [n][ns] (negative: missing); chrom [n] indices into contigs, pos0 [n]; ref / alt: one base per record (default A / G)."""
    n, ns = gq.shape
    ref = np.full(n, ord("A"), np.uint8) if ref is None else np.asarray(ref, np.uint8)
    alt = np.full(n, ord("G"), np.uint8) if alt is None else np.asarray(alt, np.uint8)
    adv = np.where(ad < 0, np.int16(-32768), ad).astype("<i2")
    gqb = np.where(gq < 0, np.uint32(0x7F800001), gq.astype("<f4").view("<u4")).astype("<u4")
    shared = np.zeros((n, 24 + 1 + 2 + 2 + 2), np.uint8)
    shared[:, 0:4] = np.asarray(chrom, "<i4").reshape(n, 1).view(np.uint8)
    shared[:, 4:8] = np.asarray(pos0, "<i4").reshape(n, 1).view(np.uint8)
    shared[:, 8:12] = np.full((n, 1), 1, "<i4").view(np.uint8)
    shared[:, 12:16] = np.full((n, 1), 50.0, "<f4").view(np.uint8)
    shared[:, 16:20] = np.full((n, 1), 2 << 16, "<u4").view(np.uint8)
    shared[:, 20:24] = np.full((n, 1), (3 << 24) | ns, "<u4").view(np.uint8)
    shared[:, 24] = 0x07
    shared[:, 25], shared[:, 26] = 0x17, ref
    shared[:, 27], shared[:, 28] = 0x17, alt
    shared[:, 29], shared[:, 30] = 0x11, 0x00
    k = lambda key: _typed_int(1 + KEYS.index(key))  # noqa: E731
    h_gt, h_ad, h_gq = k("GT") + bytes([0x21]), k("AD") + bytes([0x22]), k("GQ") + bytes([0x15])
    l_indiv = len(h_gt) + 2 * ns + len(h_ad) + 4 * ns + len(h_gq) + 4 * ns
    rec = np.zeros((n, 8 + shared.shape[1] + l_indiv), np.uint8)
    rec[:, 0:4] = np.full((n, 1), shared.shape[1], "<u4").view(np.uint8)
    rec[:, 4:8] = np.full((n, 1), l_indiv, "<u4").view(np.uint8)
    at = 8
    rec[:, at: at + shared.shape[1]] = shared
    at += shared.shape[1]
    for head, body in ((h_gt, np.ascontiguousarray(gt, np.int8).reshape(n, 2 * ns).view(np.uint8)), (h_ad, np.ascontiguousarray(adv).reshape(n, 2 * ns).view(np.uint8)),
                       (h_gq, np.ascontiguousarray(gqb).reshape(n, ns).view(np.uint8))):
        rec[:, at: at + len(head)] = np.frombuffer(head, np.uint8)
        at += len(head)
        rec[:, at: at + body.shape[1]] = body
        at += body.shape[1]
    assert at == rec.shape[1]
    return header_bytes(samples, contigs) + rec.tobytes()
