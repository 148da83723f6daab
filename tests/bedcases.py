"""The hand-built panel of BED rows (unfazed_amd/csrc/bed_row.hpp; uz_bed_rows_lists): every edge of the decision, the site order, the list
joins, the integers and the dropped rows.  A case is

    dict(name, ratio, include_ambiguous, verbose, names=[str], dnms=[dict(status, lists=(dad_reads, mom_reads, dad_sites, mom_sites))],
         rows=[dict(chrom, start, end, vartype, kid, dad, mom, dnm)])       # dnm None: a SEX-CHROM row

with read lists as ids into `names`.  The expected text of a row is what summarize.bed_lines prints for the equivalent one-record dict
(`expected_rows`); `pack` lays a case out as the arrays of uz_bed_rows_lists, `dump` writes cases with their expected text for
tests/bed_row_main.cpp."""
import random
import struct

import numpy as np

from unfazed_amd import abi, summarize

ST_OK = 0


def _dnm(n_dad, n_mom, s_dad=None, s_mom=None, status=ST_OK, first_id=0):
    """lists of the given lengths: read ids ascending from first_id, sites ascending from 1000"""
    s_dad = list(range(1000, 1000 + 7 * max(1, n_dad), 7))[: max(1, n_dad)] if s_dad is None else s_dad
    s_mom = list(range(2000, 2000 + 3 * max(1, n_mom), 3))[: max(1, n_mom)] if s_mom is None else s_mom
    return dict(status=status, lists=(list(range(first_id, first_id + n_dad)), list(range(first_id + n_dad, first_id + n_dad + n_mom)), s_dad, s_mom))


def _row(dnm, chrom="chr1", start=100, end=101, vartype="POINT", kid="kid1", dad="dad1", mom="mom1"):
    return dict(chrom=chrom, start=start, end=end, vartype=vartype, kid=kid, dad=dad, mom=mom, dnm=dnm)


def _names(n, length=None):
    return ["r%d" % k if length is None else ("%0*d" % (length, k))[-length:] for k in range(n)]


def _flags():
    return [(v, a) for v in (False, True) for a in (False, True)]


def build_cases():
    cases = []

    def add(name, dnms, rows, ratio=10, names=None, flags=None):
        if names is None:
            top = max([q for d in dnms for lst in d["lists"][:2] for q in lst] + [-1])
            names = _names(top + 1)
        for verbose, amb in (flags or _flags()):
            cases.append(dict(name="%s/v%d/a%d" % (name, verbose, amb), ratio=ratio, include_ambiguous=amb, verbose=verbose, names=names, dnms=dnms, rows=rows))

    # ---- the decision's edges
    for ratio, pairs in ((10, [(0, 0), (1, 0), (0, 1), (10, 1), (9, 1), (1, 10), (1, 9), (1, 1), (20, 2), (19, 2)]), (1, [(1, 1)]), (0, [(0, 0), (0, 3)])):
        for nd, nm in pairs:
            add("decision/r%d/%d_%d" % (ratio, nd, nm), [_dnm(nd, nm)], [_row(0)], ratio=ratio)
    # ---- SEX-CHROM rows (the host names the origin; the chrom test stays in Python)
    add("sex", [], [_row(None, chrom=c, vartype="POINT") for c in ("chrY", "Y", "y", "chrX", "X")])
    add("sex/mixed", [_dnm(3, 0)], [_row(None, chrom="chrY"), _row(0), _row(None, chrom="X")])
    # ---- site lists in string order
    for k, sites in enumerate(([9, 10], [99999, 100000, 100001], [10 ** e for e in range(10)], [2147483647], [0], [0, 1, 9, 10, 11, 19, 20, 99, 100, 101, 1000000000, 2147483647])):
        add("sites/%d" % k, [_dnm(2, 0, s_dad=sites, s_mom=[]), _dnm(0, 2, s_dad=[5], s_mom=sites, first_id=2)], [_row(0), _row(1)], flags=[(True, False)])
    # ---- list lengths (site lists and read lists alike)
    for n in (0, 1, 63, 64, 65, 129, 1025, 5000):
        sites = sorted(random.Random(n).sample(range(0, 3000000), n))
        add("len/%d" % n, [_dnm(n, 0, s_dad=sites, s_mom=[]), _dnm(0, n, s_dad=[], s_mom=sites, first_id=n)], [_row(0), _row(1)], ratio=0, flags=[(True, True), (False, True)])
    # ---- names of 1, 8 and 254 bytes
    for ln in (1, 8, 254):
        add("names/%d" % ln, [_dnm(4, 1)], [_row(0)], ratio=1, names=_names(5, ln), flags=[(True, False)])
    add("names/mixed", [_dnm(70, 3)], [_row(0)], names=[("n%d" % k) * (1 + k % 9) for k in range(73)], flags=[(True, False)])
    # ---- a line longer than 64 KiB
    add("long_line", [_dnm(400, 2)], [_row(0)], names=_names(402, 200), flags=[(True, False)])
    # ---- start / end
    add("ints", [_dnm(2, 0)], [_row(0, start=s, end=e) for s, e in ((0, 0), (-1, 0), (0, -1), (2147483647, 2147483647), (-2147483648, 7), (10, 1000000000), (99, 100))])
    # ---- numbers of rows; dropped rows between kept ones; all rows dropped
    add("rows/0", [], [])
    add("rows/1", [_dnm(2, 0)], [_row(0)])
    kinds = [(3, 0), (1, 1), (0, 0), (0, 2)]
    dn65 = []
    for k in range(65):
        nd, nm = kinds[k % 4]
        dn65.append(_dnm(nd, nm, status=ST_OK if k % 7 else 2, first_id=3 * k))
    add("rows/65", dn65, [_row(k, start=1000 - k, end=1001 + k, kid="kid%d" % (k % 3), chrom="chr%d" % (k % 5)) for k in range(65)])
    add("rows/all_dropped", [_dnm(0, 0), _dnm(1, 1), _dnm(5, 0, status=1)], [_row(0), _row(1), _row(2)], flags=[(False, False), (True, False)])
    # ---- rows that share a DNM, rows out of DNM order, long fixed strings
    add("rows/shared", [_dnm(2, 0), _dnm(0, 2, first_id=2)], [_row(1), _row(0), _row(1, chrom="c" * 300, kid="", vartype="v" * 70)])
    return cases


CASES = build_cases()


def sex_origin(chrom: str) -> int:
    return 0 if chrom.lower().strip("chr") == "y" else 1


def record_of(case, row):
    """the records-dict entry summarize.bed_lines takes for the row (hostpath.run_read_phasing_impl, pass 3); None: no record"""
    region = {"chrom": row["chrom"], "start": row["start"], "end": row["end"]}
    base = {"region": region, "vartype": row["vartype"], "kid": row["kid"], "dad": row["dad"], "mom": row["mom"]}
    if row["dnm"] is None:
        return dict(base, cnv_dad_sites="NA", cnv_mom_sites="NA", cnv_evidence_type="SEX-CHROM", dad_sites="", mom_sites="", evidence_type="SEX-CHROM",
                    dad_reads=[], mom_reads=[])
    d = case["dnms"][row["dnm"]]
    if d["status"] != ST_OK:
        return None
    dr, mr, ds, ms = d["lists"]
    nm = case["names"]
    return dict(base, dad_sites=[str(p) for p in ds], mom_sites=[str(p) for p in ms], evidence_type="readbacked", dad_reads=[nm[q] for q in dr],
                mom_reads=[nm[q] for q in mr], cnv_dad_sites="", cnv_mom_sites="", cnv_evidence_type="")


def expected_rows(case):
    """per row the bytes of its line ('' for a dropped row), by summarize.bed_lines over the equivalent records dict"""
    out = []
    for row in case["rows"]:
        rec = record_of(case, row)
        lines = [] if rec is None else summarize.bed_lines({"k": rec}, case["include_ambiguous"], case["verbose"], case["ratio"])[1:]
        out.append((lines[0] + "\n").encode() if lines else b"")
    return out


def pack(case):
    """the arrays of uz_bed_rows_lists for the case"""
    st = abi.StringTable()
    rows = np.zeros(len(case["rows"]), abi.BED_ROW)
    for k, r in enumerate(case["rows"]):
        rows[k] = (-1 if r["dnm"] is None else r["dnm"], r["start"], r["end"], st.id(r["chrom"]), st.id(r["vartype"]), st.id(r["kid"]), st.id(r["dad"]),
                   st.id(r["mom"]), 0, sex_origin(r["chrom"]) if r["dnm"] is None else 0)
    str_off, str_bytes = st.arrays()
    lens = [len(lst) for d in case["dnms"] for lst in d["lists"]]
    list_off = np.zeros(len(lens) + 1, np.int64)
    list_off[1:] = np.cumsum(np.asarray(lens, np.int64)) if lens else 0
    vals = [x for d in case["dnms"] for lst in d["lists"] for x in lst]
    nb = [n.encode() for n in case["names"]]
    name_off = np.zeros(len(nb) + 1, np.uint32)
    name_off[1:] = np.cumsum(np.asarray([len(b) for b in nb], np.int64)) if nb else 0
    return dict(rows=rows, str_off=str_off, str_bytes=str_bytes, status=np.asarray([d["status"] for d in case["dnms"]], np.int32), list_off=list_off,
                list_val=np.asarray(vals, np.int32), name_off=name_off, name_bytes=np.frombuffer(b"".join(nb) + b"\0", np.uint8))


def fuzz_cases(seed, n_rows, rows_per_case=100):
    """seeded random cases, n_rows rows in all: every branch of the decision, empty and long lists, dropped rows, SEX-CHROM rows"""
    rng = random.Random(seed)
    cases = []
    while n_rows > 0:
        m = min(rows_per_case, n_rows)
        n_rows -= m
        names = ["q%d:%s" % (k, "x" * rng.randrange(0, 40)) for k in range(rng.randrange(1, 60))]
        dnms, rows = [], []
        for k in range(m):
            def ids():
                return sorted(rng.sample(range(len(names)), min(len(names), rng.choice((0, 0, 1, 2, 3, 20)))))

            def sites():
                top = rng.choice((12, 1200, 120000, 2147483647))
                return sorted(rng.sample(range(0, top), rng.choice((0, 1, 2, 5, 11))))
            dnms.append(dict(status=rng.choice((0, 0, 0, 0, 1, 2, 3, 5)), lists=(ids(), ids(), sites(), sites())))
            rows.append(_row(None if rng.random() < 0.05 else k, chrom=rng.choice(("chr1", "1", "chrY", "Y", "chrX", "10")), start=rng.choice((0, -1, 5, rng.randrange(1, 1 << 31) - 1)),
                             end=rng.randrange(-5, 1 << 31), vartype=rng.choice(("POINT", "DEL", "")), kid="k%d" % rng.randrange(4)))
        cases.append(dict(name="fuzz/%d" % len(cases), ratio=rng.choice((0, 1, 2, 10)), include_ambiguous=rng.random() < 0.5, verbose=rng.random() < 0.7, names=names,
                          dnms=dnms, rows=rows))
    return cases


def dump(cases, path):
    """cases + expected text for tests/bed_row_main.cpp: per case a header of int64s, then the arrays as they lie, each padded to 8 bytes"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)))
        for c in cases:
            p = pack(c)
            exp = expected_rows(c)
            eoff = np.zeros(len(exp) + 1, np.int64)
            eoff[1:] = np.cumsum(np.asarray([len(b) for b in exp], np.int64)) if exp else 0
            arrays = [p["rows"], p["str_off"], p["str_bytes"], p["status"], p["list_off"], p["list_val"], p["name_off"], p["name_bytes"], eoff,
                      np.frombuffer(b"".join(exp) + b"\0", np.uint8)]
            fh.write(struct.pack("<8q", c["ratio"], int(c["verbose"]), int(c["include_ambiguous"]), len(c["rows"]), len(c["dnms"]), int(p["str_off"].size) - 1,
                                 len(c["names"]), int(p["list_val"].size)))
            for a in arrays:
                b = a.tobytes()
                fh.write(struct.pack("<q", len(b)))
                fh.write(b + b"\0" * (-len(b) % 8))
