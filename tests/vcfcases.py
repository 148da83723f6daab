"""A hand-built edge table for the sample cells of a text VCF (tests/test_vcf_cell.py, test_vcf_lazy.py, test_vcf_device_gpu.py).

A case is one record: its FORMAT and a few sample cells.  Every cell carries the values the DECODER holds for it (gt code, int depths, float
GQ: unfazed_amd/io_vcf.py's semantics) and a label, `plain` or `unsettled`, derived by hand from the grammar the device's parser documents
(unfazed_amd/csrc/vcf_cell.hpp) -- never read back from the code:

  pieces   a field whose slot the column does not reach, or whose key FORMAT lacks, keeps its default (gt 2, depths and GQ -1)
  GT       alleles of 1-3 digits or ".", '/' or '|' between them, only the first two read; anything else unsettled
  depths   "." / empty = missing; 1-5 digits, value <= 32767; signs, longer numbers, larger values, other characters: unsettled
  AD       first two comma-separated entries; one entry: alt missing; a bare "." falls through to RO / AO (AO up to its first comma)
  GQ       "." / empty = missing; 1-5 digits (<= 32767), optionally '.' and 1-6 digits; everything else unsettled

A record of the table's VCF repeats the case's cells cyclically over the file's sample columns (NS of them), so that any pick of columns
meets every cell.  `raises`: the host decoder refuses the cell (UZ_IO_E_FORMAT) -- such cases cannot stand in a file that must decode, and
`pack_raises` ones cannot be packed; both are used cell by cell and in the error tests only."""

NS = 140
SAMPLES = ["s%03d" % i for i in range(NS)]
P, U = "plain", "unsettled"
D = (2, -1, -1, -1.0)  # every field at its default


def _c(name, fmt, cells, **kw):
    return dict(name=name, fmt=fmt, cells=cells, **kw)


CASES = [
    # ---- GT: every form of parse_gt
    _c("gt_diploid_slash", "GT", [("0/0", (0, -1, -1, -1.0), P), ("0/1", (1, -1, -1, -1.0), P), ("1/0", (1, -1, -1, -1.0), P), ("1/1", (3, -1, -1, -1.0), P)]),
    _c("gt_diploid_phased", "GT", [("0|0", (0, -1, -1, -1.0), P), ("0|1", (1, -1, -1, -1.0), P), ("1|0", (1, -1, -1, -1.0), P), ("1|1", (3, -1, -1, -1.0), P)]),
    _c("gt_missing", "GT", [(".", D, P), ("./.", D, P), (".|.", D, P)]),
    _c("gt_half_missing", "GT", [("./0", (0, -1, -1, -1.0), P), ("./1", (1, -1, -1, -1.0), P), ("0/.", (0, -1, -1, -1.0), P), ("1|.", (1, -1, -1, -1.0), P)]),
    _c("gt_haploid", "GT", [("0", (0, -1, -1, -1.0), P), ("1", (3, -1, -1, -1.0), P), ("2", (3, -1, -1, -1.0), P)]),
    _c("gt_multiallelic", "GT", [("1/2", (1, -1, -1, -1.0), P), ("2/2", (3, -1, -1, -1.0), P), ("0/2", (1, -1, -1, -1.0), P), ("10/10", (3, -1, -1, -1.0), P),
                                 ("999/0", (1, -1, -1, -1.0), P), ("007/7", (3, -1, -1, -1.0), P)]),
    _c("gt_triploid", "GT", [("0/0/1", (0, -1, -1, -1.0), P), ("0/1/1", (1, -1, -1, -1.0), P), ("1|1|0", (3, -1, -1, -1.0), P), ("./././.", D, P)]),
    _c("gt_four_digits", "GT", [("1000/0", (1, -1, -1, -1.0), U), ("0/1", (1, -1, -1, -1.0), P)]),
    _c("gt_signed", "GT", [("+1/0", (1, -1, -1, -1.0), U), ("-1/0", (0, -1, -1, -1.0), U), ("0/0", (0, -1, -1, -1.0), P)]),
    _c("gt_empty", "GT:AD", [(":5,3", None, U)], raises=True),
    _c("gt_letters", "GT", [("a/b", None, U)], raises=True),
    _c("gt_empty_second", "GT", [("0/", None, U)], raises=True),
    _c("gt_carriage_return", "GT", [("0/1\r", None, U)], raises=True),
    # ---- pieces and FORMAT
    _c("short_column", "GT:AD:GQ", [("0/1", (1, -1, -1, -1.0), P), ("0/1:5,3", (1, 5, 3, -1.0), P), ("1/1:5,3:40", (3, 5, 3, 40.0), P)]),
    _c("short_line", "GT:AD:GQ", [("0/1:5,3:40", (1, 5, 3, 40.0), P), ("0/0:8,0:30", (0, 8, 0, 30.0), P)], short_line=True),
    _c("no_format", None, []),
    _c("format_without_samples", "GT:AD:GQ", [], short_line=True),
    _c("format_without_gt", "AD:GQ", [("5,3:40", (2, 5, 3, 40.0), P), (".:.", D, P)]),
    _c("duplicated_key", "GT:AD:GT", [("0/0:5,3:1/1", (3, 5, 3, -1.0), P), ("0/0:5,3", (2, 5, 3, -1.0), P)]),
    _c("other_keys", "GT:XX:AD:YY:GQ", [("0/1:foo:7,8:bar,-1e9:55", (1, 7, 8, 55.0), P), ("0/1:+:7,8:nan:55", (1, 7, 8, 55.0), P)]),
    _c("fifteen_keys", "GT:K1:K2:K3:K4:K5:K6:K7:K8:K9:RO:AO:KA:GQ:KB", [("0/1:a:b:c:d:e:f:g:h:i:21:4:x:33:y", (1, 21, 4, 33.0), P)]),
    _c("empty_cell", "AD:GQ", [("", (2, -1, -1, -1.0), P), ("4,4:9", (2, 4, 4, 9.0), P)]),
    # ---- depths
    _c("ad_dot_no_ro_ao", "GT:AD", [("0/1:.", (1, -1, -1, -1.0), P)]),
    _c("ad_dot_ro_ao", "GT:AD:RO:AO", [("0/1:.:12:7", (1, 12, 7, -1.0), P), ("0/1:.:12:7,9", (1, 12, 7, -1.0), P), ("0/1:.:.:.", (1, -1, -1, -1.0), P),
                                       ("0/1:.:12", (1, -1, -1, -1.0), P), ("0/1:3,4:12:7", (1, 3, 4, -1.0), P), ("0/1:.:1,2:7", (1, -1, 7, -1.0), U)]),
    _c("ro_ao_only", "GT:RO:AO", [("0/1:30:2", (1, 30, 2, -1.0), P), ("0/1:30", (1, -1, -1, -1.0), P)]),
    _c("ad_entries", "GT:AD", [("0/1:9", (1, 9, -1, -1.0), P), ("0/1:9,4,2", (1, 9, 4, -1.0), P), ("0/1:,4", (1, -1, 4, -1.0), P), ("0/1:9,", (1, 9, -1, -1.0), P),
                               ("0/1:.,4", (1, -1, 4, -1.0), P), ("0/1:9,4,zz", (1, 9, 4, -1.0), P)]),
    _c("depth_zero_and_top", "GT:AD", [("0/0:0,0", (0, 0, 0, -1.0), P), ("0/1:32767,32767", (1, 32767, 32767, -1.0), P), ("0/1:00012,3", (1, 12, 3, -1.0), P)]),
    _c("depth_32768", "GT:AD", [("0/1:32768,1", (1, 32768, 1, -1.0), U), ("0/1:1,32768", (1, 1, 32768, -1.0), U), ("0/1:1,1", (1, 1, 1, -1.0), P)]),
    _c("depth_two_to_30", "GT:AD", [("0/1:1073741824,5", (1, 1 << 30, 5, -1.0), U), ("0/1:6,5", (1, 6, 5, -1.0), P)]),
    _c("depth_minus_one", "GT:AD", [("0/1:-1,5", (1, -1, 5, -1.0), U), ("0/1:5,-1", (1, 5, -1, -1.0), U)]),
    _c("depth_minus_five", "GT:AD", [("0/1:-5,5", (1, -5, 5, -1.0), U)], pack_raises=True),
    _c("depth_six_digits", "GT:AD", [("0/1:000012,5", (1, 12, 5, -1.0), U)]),
    _c("depth_other_characters", "GT:AD", [("0/1:1x,3", (1, -1, 3, -1.0), U), ("0/1:+5,3", (1, 5, 3, -1.0), U), ("0/1:5,3e1", (1, 5, -1, -1.0), U)]),
    # ---- GQ
    _c("gq_plain", "GT:GQ", [("0/1:99", (1, -1, -1, 99.0), P), ("0/1:99.5", (1, -1, -1, 99.5), P), ("0/1:0.000001", (1, -1, -1, 0.000001), P),
                             ("0/1:32767.9", (1, -1, -1, 32767.9), P), ("0/1:007", (1, -1, -1, 7.0), P), ("0/1:.", (1, -1, -1, -1.0), P), ("0/1:", (1, -1, -1, -1.0), P),
                             ("0/1:0", (1, -1, -1, 0.0), P)]),
    _c("gq_trailing_point", "GT:GQ", [("0/1:99.", (1, -1, -1, 99.0), U)]),
    _c("gq_seven_fraction_digits", "GT:GQ", [("0/1:1.0000001", (1, -1, -1, 1.0000001), U), ("0/1:99.9999999999999999", (1, -1, -1, 100.0), U)]),
    _c("gq_exponent", "GT:GQ", [("0/1:1e2", (1, -1, -1, 100.0), U)]),
    _c("gq_signed_zero", "GT:GQ", [("0/1:-0.0", (1, -1, -1, -0.0), U)]),
    _c("gq_nan_inf", "GT:GQ", [("0/1:nan", (1, -1, -1, float("nan")), U), ("0/1:inf", (1, -1, -1, float("inf")), U)]),
    _c("gq_32768", "GT:GQ", [("0/1:32768", (1, -1, -1, 32768.0), U), ("0/1:100000", (1, -1, -1, 100000.0), U)]),
    _c("gq_leading_point", "GT:GQ", [("0/1:.5", (1, -1, -1, 0.5), U)]),
    # ---- line forms: a trailing '\r' belongs to the line's last sample column (tail: that cell's own values and label)
    _c("carriage_return_in_gq", "GT:GQ", [("0/1:50", (1, -1, -1, 50.0), P)], tail=("\r", (1, -1, -1, -1.0), U)),
    _c("carriage_return_in_unread_piece", "GT:GQ:XX", [("0/1:50:zz", (1, -1, -1, 50.0), P)], tail=("\r", (1, -1, -1, 50.0), P)),
]

FILE_CASES = [c for c in CASES if not c.get("raises") and not c.get("pack_raises")]


def record_cells(case):
    """the NS cells of a case's record: [(text or None when the line is too short for the column, decoder values, label)]"""
    cells = case["cells"]
    if case["fmt"] is None or not cells:
        return [(None, D, P)] * NS
    n = len(cells) if case.get("short_line") else NS
    out = [cells[s % len(cells)] for s in range(n)] + [(None, D, P)] * (NS - n)
    if case.get("tail"):
        add, values, label = case["tail"]
        out[n - 1] = (out[n - 1][0] + add, values, label)
    return out


def record_line(case, pos1, chrom="chr1"):
    fixed = [chrom, str(pos1), ".", "A", "G", "50", "PASS", "."]
    if case["fmt"] is None:
        return "\t".join(fixed)
    return "\t".join(fixed + [case["fmt"]] + [t for t, _, _ in record_cells(case) if t is not None])


def vcf_text(n_records, cases=None, final_newline=False):
    """the table's VCF: n_records records that run through `cases` (FILE_CASES) cyclically, 10 bases apart -> (text, the case of every record).
    The last line has no newline unless asked for."""
    cases = FILE_CASES if cases is None else cases
    used = [cases[i % len(cases)] for i in range(n_records)]
    head = ["##fileformat=VCFv4.2", "##contig=<ID=chr1>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(SAMPLES)]
    lines = head + [record_line(c, 101 + 10 * i) for i, c in enumerate(used)]
    return "\n".join(lines) + ("\n" if final_newline else ""), used


def unsettled_records(used, pick):
    """records with an `unsettled` cell in a picked column"""
    return [i for i, c in enumerate(used) if any(record_cells(c)[s][2] == U for s in set(pick))]
