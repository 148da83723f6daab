"""Hand-built DNM VCFs for the annotated-VCF writer's device route (unfazed_amd/csrc/vcf_row.hpp, k_vcfout.hip, unfazed.write_vcf_output).

A case holds a header, record lines (bytes, each with its own line end), a `read_records`-shaped dict in the smallest form summarize_record
accepts, and the set of records the device body is stated to hand back.  What a case EXPECTS is never computed by the code under test: it is
the host write_vcf_output's text (host_output, expected_rows).  `rules_text` is a plain-Python statement of vcf_row.hpp's rules over an
annotation table; tests/test_vcf_route_host.py holds it to the host writer over the whole panel, and it is the expectation only of the one
case no records dict can reach (uet 5: summarize_record never returns AMBIGUOUS_BOTH, its branches need an origin that READBACKED sets).

The same cases go to the one-lane host program (dump -> tests/vcf_row_main.cpp), to engine.vcf_rows and to the driver."""
import os
import random
import struct

import numpy as np

from unfazed_amd import unfazed
from unfazed_amd.io_vcf import site_of

GATE_FORMS = ["0/0", "0/1", "1/1", "1|0", "./.", ".", "./1", "0/.", "1", "0", "0/1/1", "10/11", "123/0"]
BAD_GT_FORMS = ["1234/0", "", "a/b"]
FIXED = "##fileformat=VCFv4.2\n##contig=<ID=chr1>\n"


def header(samples):
    return (FIXED + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples)).split("\n")


def line(pos, cells, fmt="GT:DP", chrom="chr1", ident=".", ref="A", alt="T", info=".", end=b"\n"):
    cols = [chrom, str(pos), ident, ref, alt, "50", "PASS", info]
    if fmt is not None:
        cols += [fmt] + list(cells)
    return "\t".join(cols).encode() + end


def rec(kid, start, end=None, chrom="chr1", vartype="POINT", nd=2, nm=0, sd=None, sm=None, cd=0, cm=0, etype="READBACKED"):
    """(key, record): nd / nm read names and sd / sm sites for dad / mom, cd / cm allele-balance sites"""
    end = start + 1 if end is None else end
    sd, sm = nd if sd is None else sd, nm if sm is None else sm
    r = {"region": {"chrom": chrom, "start": start, "end": end}, "vartype": vartype, "kid": kid, "dad": "dad", "mom": "mom", "evidence_type": etype,
         "dad_reads": ["r"] * nd, "mom_reads": ["q"] * nm, "dad_sites": ["1"] * sd, "mom_sites": ["2"] * sm,
         "cnv_dad_sites": ["3"] * cd, "cnv_mom_sites": ["4"] * cm}
    return "{}_{}_{}_{}_{}".format(chrom, start, end, kid, vartype), r


def build_cases():
    cases = []

    def add(name, samples, lines, records=(), amb=False, hb=(), chunk=None, raw_ann=None, head=None):
        cases.append({"name": name, "header": head if head is not None else header(samples), "samples": list(samples), "lines": list(lines),
                      "records": dict(records), "amb": amb, "hb": sorted(hb), "chunk": chunk, "raw_ann": raw_ann})

    two = ["kid", "other"]
    # the gate: an annotated cell of every genotype form
    for g in GATE_FORMS:
        add("gate/" + g.replace("/", "_").replace("|", "p").replace(".", "d"), two, [line(100, [g + ":7", "0/0:3"])], [rec("kid", 99)])
    # the forms that go back to the host
    for g, tag in zip(BAD_GT_FORMS, ("1234_0", "empty", "a_b")):
        add("handback/gt_" + tag, two, [line(100, ["0/1:7", "0/0:3"]), line(200, ["0/1:7", g + ":3"]), line(300, ["1/1:7", "0/0:3"])],
            [rec("kid", 99), rec("kid", 199), rec("kid", 299)], hb=[1])
    add("handback/col_few", two, [line(100, ["0/1:7", "0/0:3"]), line(200, ["0/1:7"])], [rec("kid", 99)], hb=[1])
    add("handback/col_many", two, [line(100, ["0/1:7", "0/0:3", "0/1:9"]), line(200, ["0/1:7", "0/0:3"])], [rec("kid", 99), rec("kid", 199)], hb=[0])
    add("handback/no_format", two, [line(100, ["0/1:7", "0/0:3"]), line(200, [], fmt=None)], [rec("kid", 99)], hb=[1])
    add("handback/gt_twice", two, [line(100, ["0/1:0/0", "0/0:0/1"], fmt="GT:GT"), line(200, ["0/1:7", "0/0:3"])], [rec("kid", 99), rec("other", 99)], hb=[0])
    add("handback/gt_third_allele", two, [line(100, ["0/1/x:7", "0/0:3"]), line(200, ["0/1:7", "0/0:3"])], [rec("kid", 199)], hb=[0])
    # where GT stands in FORMAT
    add("gtslot/0", two, [line(100, ["0/1:7:9", "0/0:3:1"], fmt="GT:DP:GQ")], [rec("kid", 99)])
    add("gtslot/mid", two, [line(100, ["7:0/1:9", "3:0/0:1"], fmt="DP:GT:GQ")], [rec("kid", 99)])
    add("gtslot/last", two, [line(100, ["7:9:0/1", "3:1:0/0"], fmt="DP:GQ:GT")], [rec("kid", 99)])
    add("gtslot/none", two, [line(100, ["7:9", "3:1"], fmt="DP:GQ")], [rec("kid", 99)])
    add("gtslot/not_reached", two, [line(100, ["7", "3:1:1/1"], fmt="DP:GQ:GT")], [rec("kid", 99), rec("other", 99, nd=0, nm=3)])
    # padding
    f5 = "GT:DP:GQ:AD:PL"
    add("pad/short1", two, [line(100, ["0/1:7:9:1,2", "0/0:3:1:4,0:0,1,2"], fmt=f5)], [rec("kid", 99)])
    add("pad/short3", two, [line(100, ["0/1:7", "0/0:3:1:4,0:0,1,2"], fmt=f5)], [rec("kid", 99)])
    add("pad/equal", two, [line(100, ["0/1:7:9:1,2:0,1,2", "0/0:3:1:4,0:0,1,2"], fmt=f5)], [rec("kid", 99)])
    add("pad/longer", two, [line(100, ["0/1:7:9:1,2:0,1,2:x:y", "0/0:3:1:4,0:0,1,2"], fmt=f5)], [rec("kid", 99)])
    add("pad/dot5", two, [line(100, [".", "0/1"], fmt=f5)], [rec("kid", 99), rec("other", 99)])
    # gt codes and evidence types
    add("gtcode/0", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=1, nm=1)], amb=True)
    add("gtcode/0_dropped", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=1, nm=1)], amb=False)
    add("gtcode/1", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=3, nm=0)])
    add("gtcode/2", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=0, nm=3)])
    add("uet/-1", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=0, nm=0)], amb=True)
    add("uet/0", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=2)])
    add("uet/1", two, [line(100, ["0/1:7", "0/0:3"], info="SVTYPE=DEL;END=500")], [rec("kid", 99, 500, vartype="DEL", nd=0, cd=4)])
    add("uet/2", two, [line(100, ["0/1:7", "0/0:3"], info="SVTYPE=DEL;END=500")], [rec("kid", 99, 500, vartype="DEL", nd=2, cd=4)])
    add("uet/3", two, [line(100, ["0/1:7", "0/0:3"])], [rec("kid", 99, nd=1, nm=1)], amb=True)
    add("uet/4", two, [line(100, ["0/1:7", "0/0:3"], info="SVTYPE=DUP;END=500")], [rec("kid", 99, 500, vartype="DUP", nd=0, cd=1, cm=1)], amb=True)
    add("uet/5", two, [line(100, ["0/1:7", "1/1:3"])], raw_ann=[(0, 0, 0, 12, 5), (0, 1, 2, 3, 5)])
    add("uet/6", two, [line(100, ["0/1:7", "0/0:3"], chrom="chrX"), line(100, ["1:7", "0/0:3"], chrom="chrY")],
        [rec("kid", 99, chrom="chrX", etype="SEX-CHROM"), rec("kid", 99, chrom="chrY", etype="SEX-CHROM")])
    add("uet/mom_allele_balance", two, [line(100, ["0/1:7", "0/0:3"], info="SVTYPE=DEL;END=500")], [rec("kid", 99, 500, vartype="DEL", nd=0, nm=2, cm=4)])
    # the count
    for n in (0, 9, 10, 999999, 1000000):
        add("uops/%d" % n, two, [line(100, ["0/1:7", "0/0:3"]), line(200, ["0/1:7", "0/1:3"])], [rec("kid", 99, sd=n), rec("other", 199, sd=5)],
            hb=[0] if n > 999999 else [])
    # keys
    add("keys/same_site_twice", two, [line(100, ["0/1:7", "0/0:3"]), line(100, ["1/1:8", "0/0:3"], alt="G")], [rec("kid", 99)])
    add("keys/homref_and_het", two, [line(100, ["0/0:7", "0/0:3"]), line(100, ["0/1:8", "0/0:3"], alt="G")], [rec("kid", 99)])
    add("keys/end_abc", two, [line(100, ["0/1:7", "0/0:3"], info="END=abc")], [rec("kid", 99)])
    add("keys/end_empty", two, [line(100, ["0/1:7", "0/0:3"], info="DP=4;END=")], [rec("kid", 99)])
    add("keys/end_number", two, [line(100, ["0/1:7", "0/0:3"], info="END=180")], [rec("kid", 99, 180), rec("other", 99)])
    add("keys/sv_and_point", two, [line(100, ["0/1:7", "0/1:3"], info="SVTYPE=DEL;END=100"), line(100, ["0/1:7", "0/1:3"], info="END=100")],
        [rec("kid", 99, 100, vartype="DEL", nd=0, cd=3), rec("other", 99, 100, nd=0, nm=2)])
    add("keys/dup_sample", ["kid", "other", "kid"], [line(100, ["0/1:7", "0/0:3", "1/1:2"]), line(200, ["0/0:7", "0/1:3", "0/1:2"])], [rec("kid", 99), rec("kid", 199, nd=0, nm=2)])
    add("keys/unknown_kid", two, [line(100, ["0/1:7", "0/1:3"])], [rec("nobody", 99), rec("other", 99)])
    # sample counts
    for ns in (1, 3, 63, 64, 65, 130):
        names = ["s%d" % i for i in range(ns)]
        cells = [GATE_FORMS[i % len(GATE_FORMS)] + ":%d" % i for i in range(ns)]
        add("samples/%d" % ns, names, [line(100, cells), line(200, cells[::-1])],
            [rec("s0", 99), rec("s%d" % (ns - 1), 99, nd=0, nm=2), rec("s%d" % (ns // 2), 199), rec("s%d" % (ns - 1), 199, nd=1, nm=1)], amb=True)
    # byte edges: a tab, a ':' and a (rewritten) GT piece on bytes 1023 / 1024 / 1025 of the 1 KiB step that holds the sample region's start, and
    # on a 16-byte lane edge.  The step's base is the line start rounded down to 16; the first cell is a filler that moves the feature there.
    three = ["fill", "kid", "other"]
    head_bytes = len("\n".join(header(three)).encode()) + 1
    for kind in ("tab", "colon", "gt"):
        for target in (1023, 1024, 1025, 527, 528, 529):
            prefix = line(100, [], fmt="GT:DP")[:-1] + b"\t"
            base = head_bytes & ~15
            lead = {"tab": 0, "colon": 1 + 5, "gt": 1 + 2}[kind]  # bytes between the filler's end and the feature: "\t10/11" + ":" / "\t10" + "/11"
            k = base + target - (head_bytes + len(prefix) + 4 + lead)
            cells = ["0/0:" + "9" * k, "10/11:7", "0/1:3"]
            add("edge/%s/%d" % (kind, target), three, [line(100, cells)], [rec("kid", 99), rec("other", 99, nd=0, nm=2)])
    for a in range(16):
        add("align/%d" % a, two, [line(100, ["0/1:7", "1/1:3"], ident="i" * (1 + a))], [rec("kid", 99), rec("other", 99, nd=0, nm=4)])
    add("long/64k_cell", three, [line(100, ["0/0:" + "9" * 70000, "0/1:7", "1|1:3"]), line(200, ["0/1:1", "0/1:7", "1|1:3"])], [rec("kid", 99), rec("other", 199, nd=0, nm=2)])
    many = ["s%d" % i for i in range(10000)]
    add("long/64k_cells", many, [line(100, [GATE_FORMS[i % 13] + ":%d" % (i % 97) for i in range(10000)])],
        [rec("s%d" % i, 99, nd=i % 3, nm=(i + 1) % 2) for i in range(0, 10000, 7)], amb=True)
    add("ends/no_final_newline", two, [line(100, ["0/1:7", "0/0:3"]), line(200, ["0/1:7", "1/1:3"], end=b"")], [rec("kid", 99), rec("other", 199)])
    add("ends/no_final_newline_short_cell", two, [line(100, ["0/1:7", "1/1"], fmt=f5, end=b"")], [rec("other", 99)])
    add("ends/crlf", two, [line(100, ["0/1:7", "0/0:3"], end=b"\r\n"), line(200, ["0/1:7", "1/1:3"])], [rec("kid", 99), rec("other", 199)], hb=[0])
    add("ends/empty_lines", two, [b"\n", line(100, ["0/1:7", "0/0:3"]), b"\n", b"\n", line(200, ["0/1:7", "1/1:3"]), b"\n"], [rec("kid", 99), rec("other", 199)])
    # record counts
    for n in (0, 1, 65, 257):
        add("records/%d" % n, two, [line(100 + 10 * i, [GATE_FORMS[i % 13] + ":7", GATE_FORMS[(i + 5) % 13] + ":3"]) for i in range(n)],
            [rec("kid", 99 + 10 * i, nd=i % 4, nm=(i + 1) % 3) for i in range(0, n, 2)] + [rec("other", 99 + 10 * i) for i in range(0, n, 3)], amb=True)
    # 1025 short lines in one chunk: the length scan's second tile
    add("records/1025", three, [line(100 + 10 * i, ["0/0:1", GATE_FORMS[i % 13] + ":7", "0/1:3"]) for i in range(1025)],
        [rec("kid", 99 + 10 * i, nd=i % 4, nm=(i + 1) % 3) for i in range(0, 1025, 5)], amb=True)
    # chunks
    wide = ["s%d" % i for i in range(20)]
    add("chunks/4096", wide, [line(100 + i, [GATE_FORMS[(i + j) % 13] + ":%d" % j for j in range(20)]) for i in range(250)],
        [rec("s%d" % (i % 20), 99 + i, nd=i % 3, nm=(i + 1) % 2) for i in range(250)], amb=True, chunk=4096)
    add("chunks/long_line", three, [line(100, ["0/1:7", "0/1:7", "1|1:3"]), line(200, ["0/0:" + "9" * 9000, "0/1:7", "1|1:3"]), line(300, ["0/1:1", "0/1:7", "1|1:3"])],
        [rec("kid", 99), rec("kid", 199), rec("other", 299, nd=0, nm=2)], chunk=4096)
    add("chunks/all_handed_back", two, [line(100 + i, ["0/1:" + "7" * 700, ("a/b" if 3 <= i < 8 else "0/1") + ":3"]) for i in range(12)],
        [rec("kid", 99 + i) for i in range(12)], hb=range(3, 8), chunk=3600)
    return cases


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}


def file_bytes(case, skip=()):
    """the case's file; skip: record indices whose lines are left out"""
    out, k = ["\n".join(case["header"]).encode() + b"\n"], 0
    for ln in case["lines"]:
        if ln.strip(b"\r\n"):
            if k not in skip:
                out.append(ln)
            k += 1
        else:
            out.append(ln)
    return b"".join(out)


def decode(case):
    """the file as the native decoder's text view holds it: text, line_at / samp_at / line_end [n] (samp_at = line_end: no sample column)"""
    text = file_bytes(case)
    line_at, samp_at, line_end, p = [], [], [], 0
    while p < len(text):
        e = text.find(b"\n", p)
        e = len(text) if e < 0 else e
        if e > p and text[p:p + 1] != b"#":
            line_at.append(p)
            line_end.append(e)
            cols, q = 0, p
            while cols < 9:
                t = text.find(b"\t", q, e)
                if t < 0:
                    break
                cols, q = cols + 1, t + 1
            samp_at.append(q if cols == 9 else e)
        p = e + 1
    return {"text": text, "line_at": np.asarray(line_at, np.int64), "samp_at": np.asarray(samp_at, np.uint64), "line_end": np.asarray(line_end, np.uint64),
            "n_samples": len(case["samples"])}


def host_output(case, tmp_dir, skip=()):
    """the HOST writer on the case's file -> ("text", bytes) or ("raise", exception type)"""
    src, dst = os.path.join(str(tmp_dir), "in.vcf"), os.path.join(str(tmp_dir), "out.vcf")
    with open(src, "wb") as fh:
        fh.write(file_bytes(case, skip))
    was = os.environ.get("UZ_VCF_ROUTE")
    os.environ["UZ_VCF_ROUTE"] = "host"
    try:
        unfazed.write_vcf_output(src, case["records"], case["amb"], False, dst, 10)
    except Exception as e:  # noqa: BLE001 -- whatever the host raises is the expectation
        return "raise", type(e)
    finally:
        os.environ.pop("UZ_VCF_ROUTE")
        if was is not None:
            os.environ["UZ_VCF_ROUTE"] = was
    with open(dst, "rb") as fh:
        return "text", fh.read()


def sites_of(case, d=None):
    d = d or decode(case)
    out = []
    for a, s, e in zip(d["line_at"], d["samp_at"], d["line_end"]):
        if s >= e:
            out.append(None)
            continue
        chrom, start, _, _, end, info = site_of(d["text"][int(a):int(s) - 1].decode().split("\t"))
        vartype = info.get("SVTYPE")
        out.append((chrom, start, end, "POINT" if vartype is None else vartype))
    return out


def annotations(case, d=None):
    """the table the device gets: the driver's builder over the case's records dict (a record the builder keeps for the host carries a count
    the device does not print, so that the body hands it back too), or the case's raw rows"""
    d = d or decode(case)
    n = len(d["line_at"])
    if case["raw_ann"] is not None:
        rows = sorted(case["raw_ann"], key=lambda r: r[0])
        off = np.zeros(n + 1, np.int64)
        for r in rows:
            off[r[0] + 1:] += 1
        return (off, np.asarray([r[1] for r in rows], np.int32), np.asarray([r[2] for r in rows], np.uint8), np.asarray([r[3] for r in rows], np.int32),
                np.asarray([r[4] for r in rows], np.int8))
    off, col, gt, uops, uet, host_rows = unfazed.vcf_annotations(sites_of(case, d), case["samples"], case["records"], case["amb"], False, 10)
    for k in host_rows:
        at = int(off[k])
        col, gt, uops, uet = np.insert(col, at, 0), np.insert(gt, at, 0), np.insert(uops, at, 1000000), np.insert(uet, at, 0)
        off[k + 1:] += 1
    return off, col.astype(np.int32), gt.astype(np.uint8), uops.astype(np.int32), uet.astype(np.int8)


def _gt_code(piece):
    """0 HOM_REF, 1 HET, 2 UNKNOWN, 3 HOM_ALT of a GT piece inside the grammar"""
    v = [-1 if x == "." else int(x) for x in piece.replace("|", "/").split("/")]
    if len(v) == 1:
        return 2 if v[0] < 0 else (0 if v[0] == 0 else 3)
    a, b = v[0], v[1]
    if a < 0 and b < 0:
        return 2
    if a < 0 or b < 0:
        return 0 if max(a, b) == 0 else 1
    return 1 if a != b else (0 if a == 0 else 3)


def rules_text(d, ann, hb):
    """vcf_row.hpp's rules in plain Python over the decoded file and an annotation table -> the record lines (None at a record of hb)"""
    off, col, gt, uops, uet = ann
    out = []
    for k in range(len(d["line_at"])):
        if k in hb:
            out.append(None)
            continue
        f = d["text"][int(d["line_at"][k]):int(d["line_end"][k])].decode().split("\t")
        fmt = f[8].split(":")
        slot = fmt.index("GT") if "GT" in fmt else None
        f[8] += ":UOPS:UET"
        mine = {int(col[a]): a for a in range(int(off[k]), int(off[k + 1]))}
        for i in range(d["n_samples"]):
            pieces = f[9 + i].split(":")
            tail = ":-1:-1"
            if i in mine and slot is not None and slot < len(pieces):
                het_or_alt = _gt_code(pieces[slot]) in (1, 3)
                if het_or_alt:
                    m = mine[i]
                    if gt[m]:
                        pieces[slot] = "1|0" if gt[m] == 1 else "0|1"
                    tail = ":%d:%d" % (uops[m], uet[m])
            pieces += ["."] * (len(fmt) - len(pieces))
            f[9 + i] = ":".join(pieces) + tail
        out.append(("\t".join(f) + "\n").encode())
    return out


def expected_rows(case, tmp_dir):
    """the record lines the host writer prints, with their '\\n' (None at a record of the stated handed-back set: the host writes the file
    without those lines, so that a line it would raise on does not hide the others)"""
    hb = set(case["hb"])
    d = decode(case)
    n = len(d["line_at"])
    if case["raw_ann"] is not None:
        return rules_text(d, annotations(case, d), hb)
    kind, text = host_output(case, tmp_dir, skip=hb)
    assert kind == "text", (case["name"], text)
    rows = text.split(b"\n")[len(case["header"]) + 3:-1]
    assert len(rows) == n - len(hb), case["name"]
    it = iter(rows)
    return [None if k in hb else next(it) + b"\n" for k in range(n)]


def fuzz_cases(seed, n_records, per_case=50):
    """seeded cases of random cells drawn from the panel's forms; a record made to go back says so"""
    rng = random.Random(seed)
    out = []
    fmts = ["GT", "GT:DP", "DP:GT", "DP:GQ:GT", "GT:DP:GQ:AD:PL", "DP:GQ"]
    for ci in range((n_records + per_case - 1) // per_case):
        ns = rng.choice([1, 2, 3, 5, 8, 17, 64, 70])
        names = ["s%d" % i for i in range(ns)]
        lines, records, hb = [], [], []
        for k in range(min(per_case, n_records - ci * per_case)):
            fmt = rng.choice(fmts)
            keys = fmt.split(":")
            slot = keys.index("GT") if "GT" in keys else None
            bad = rng.random() < 0.06
            cells = []
            for i in range(ns):
                n_pieces = rng.choice([len(keys)] * 4 + [1, max(1, len(keys) - 1), len(keys) + 1])
                pieces = [str(rng.randrange(0, 120)) if rng.random() < 0.9 else "." for _ in range(n_pieces)]
                if slot is not None and slot < n_pieces:
                    pieces[slot] = rng.choice(GATE_FORMS)
                cells.append(":".join(pieces))
            if bad:
                how = rng.choice(["gt", "few", "many"]) if slot is not None else rng.choice(["few", "many"])
                if how == "gt":
                    i = rng.randrange(ns)
                    pieces = cells[i].split(":") + ["."] * len(keys)
                    pieces[slot] = rng.choice(BAD_GT_FORMS)
                    cells[i] = ":".join(pieces[:max(slot + 1, rng.randrange(1, len(keys) + 1))])
                elif how == "few":
                    cells = cells[:-1]
                    if not cells:
                        fmt = None  # (a line of one sample loses its only column: no sample column at all)
                else:
                    cells.append("0/1:1")
                hb.append(k)
            pos = 100 + 10 * (ci * per_case + k)
            sv = rng.random() < 0.2
            lines.append(line(pos, cells, fmt=fmt, info="SVTYPE=DEL;END=%d" % (pos + 50) if sv else ".", ident="v" * rng.randrange(1, 18)))
            for i in rng.sample(range(ns), min(ns, rng.choice([0, 1, 1, 2, 3]))):
                records.append(rec(names[i], pos - 1, pos + 50 if sv else pos, vartype="DEL" if sv else "POINT", nd=rng.randrange(0, 4), nm=rng.randrange(0, 3),
                                   sd=rng.choice([0, 1, 9, 10, 123, 4567]), cd=rng.randrange(0, 3) if sv else 0, cm=rng.randrange(0, 2) if sv else 0))
        out.append({"name": "fuzz/%d" % ci, "header": header(names), "samples": names, "lines": lines, "records": dict(records), "amb": rng.random() < 0.5,
                    "hb": hb, "chunk": None, "raw_ann": None})
    return out


def _arr(a):
    b = np.ascontiguousarray(a).tobytes()
    return struct.pack("<q", len(b)) + b + b"\0" * (-len(b) % 8)


def dump(cases, path, tmp_dir):
    """the cases with their expected lines, as tests/vcf_row_main.cpp reads them"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)))
        for c in cases:
            d = decode(c)
            off, col, gt, uops, uet = annotations(c, d)
            rows = expected_rows(c, tmp_dir)
            exp_off = np.cumsum([0] + [0 if r is None else len(r) for r in rows]).astype(np.int64)
            fh.write(struct.pack("<qq", len(rows), d["n_samples"]))
            for a in (np.frombuffer(d["text"], np.uint8), d["line_at"], d["samp_at"].astype(np.int64), d["line_end"].astype(np.int64), off, col, gt, uops, uet, exp_off,
                      np.frombuffer(b"".join(r for r in rows if r is not None), np.uint8), np.asarray([r is None for r in rows], np.uint8)):
                fh.write(_arr(a))
