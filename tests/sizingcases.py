"""Hand-built edge tables for the sizing pass (k_phase_bounds / k_bounds_reduce), shared by tests/test_sizing_model.py (the numpy model against
the kernel body's generic form, on the CPU) and tests/test_sizing_gpu.py (the device's staged form against the model).

Tables are numpy columns, not Segment lists: every record is 16M with 16 valid bases, mapq 60, its own name, no mate.  Every site is kid het,
dad het, mom hom-ref with ordinary depths and GQ 99.  A case is the table, the sites, one batch of DNMs and the parameters of its call."""
import numpy as np

from unfazed_amd import abi
from unfazed_amd.model import HET, HOM_REF, ReadsTable, SitesTable

CUTOFF = 800.5  # (not an integer: the +-cutoff windows take its integer part)
SAMPLES = ["kid", "dad", "mom"]


def make_reads(contig_starts, long_first=None):
    """contig_starts: one ascending array of record starts per contig.  long_first = (contig, length): that contig's first record is one
    `length`M record instead of 16M."""
    names = ["c%d" % k for k in range(len(contig_starts))]
    t = ReadsTable(names)
    sizes = [len(s) for s in contig_starts]
    n = int(sum(sizes))
    t.contig_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    t.start = np.concatenate([np.asarray(s, np.int64) for s in contig_starts] + [np.zeros(0, np.int64)]).astype(np.int32)
    lens = np.full(n, 16, np.int64)
    if long_first is not None:
        lens[int(t.contig_off[long_first[0]])] = long_first[1]
    for s in contig_starts:
        assert len(s) < 2 or np.all(np.diff(np.asarray(s, np.int64)) >= 0)
    t.end = (t.start.astype(np.int64) + lens).astype(np.int32)
    t.flag = np.zeros(n, np.uint16)
    t.mapq = np.full(n, 60, np.uint8)
    t.aux = np.zeros(n, np.uint8)
    t.tlen = np.zeros(n, np.int32)
    t.qname = np.arange(n, dtype=np.uint32)
    t.qnames = ["r%d" % i for i in range(n)]
    t.mate = np.full(n, -1, np.int32)
    t.n_cigar = np.ones(n, np.uint16)
    t.cigar_off = np.arange(n, dtype=np.uint32)
    t.cigar = ((lens << 4) | 0).astype(np.uint32)
    t.l_seq = lens.astype(np.uint16)
    pad = (lens + 15) & ~15
    off = np.concatenate([[0], np.cumsum(pad)])
    t.sq_off16 = (off[:-1] >> 4).astype(np.uint32)
    t.seq = np.full(int(off[-1]), ord("A"), np.uint8)
    t.qual = np.full(int(off[-1]), 30, np.uint8)
    t.max_span = np.zeros(len(names), np.int32)
    for c in range(len(names)):
        lo, hi = int(t.contig_off[c]), int(t.contig_off[c + 1])
        if hi > lo:
            t.max_span[c] = int((t.end[lo:hi].astype(np.int64) - t.start[lo:hi]).max())
    return t


def make_sites(contig_pos):
    """contig_pos: one array of site positions per contig (made ascending and unique here)"""
    names = ["c%d" % k for k in range(len(contig_pos))]
    t = SitesTable(SAMPLES, names)
    cols = [np.unique(np.asarray(p, np.int64)) for p in contig_pos]
    for p in cols:
        assert p.size == 0 or p.min() >= 0
    n = int(sum(p.size for p in cols))
    t.contig_off = np.concatenate([[0], np.cumsum([p.size for p in cols])]).astype(np.int64)
    t.pos = np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.int32)
    t.end = t.pos + 1
    t.sflags = np.zeros(n, np.uint8)
    t.ref_base = np.full(n, ord("A"), np.uint8)
    t.alt_base = np.full(n, ord("C"), np.uint8)
    t.gt = np.tile(np.array([[HET], [HET], [HOM_REF]], np.uint8), (1, n))
    t.ref_depth = np.tile(np.array([[20], [20], [40]], np.int32), (1, n))
    t.alt_depth = np.tile(np.array([[20], [20], [0]], np.int32), (1, n))
    t.gq = np.full((3, n), 99.0)
    t.ref_str = ["A"] * n
    t.alt_strs = [["C"]] * n
    return t


class Case:
    def __init__(self, name, reads, sites, dnms, search_dist, no_extended=False):
        """dnms: dicts with contig, start and optionally vartype, dflags, rcontig, end"""
        self.name, self.reads, self.sites = name, reads, sites
        self.params = abi.make_params(search_dist=search_dist, no_extended=no_extended)
        self.no_extended = no_extended
        n = len(dnms)
        g = lambda k, dflt: np.array([d[k] if k in d else dflt(d) for d in dnms], np.int64)  # noqa: E731
        self.contig = g("contig", None)
        self.rcontig = g("rcontig", lambda d: d["contig"])
        self.start = g("start", None)
        self.vartype = g("vartype", lambda d: abi.VT_POINT)
        self.end = g("end", lambda d: d["start"] + 1)
        self.dflags = g("dflags", lambda d: 0)
        self.n = n

    def subset(self, k, name):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name, c.n = name, k
        for f in ("contig", "rcontig", "start", "vartype", "end", "dflags"):
            setattr(c, f, getattr(self, f)[:k])
        return c

    def dnms_view(self):
        point = self.vartype == abi.VT_POINT
        return abi.dnms_view(self.contig, self.rcontig, self.start, self.end, self.vartype, [b"A" if p else b"" for p in point],
                             [b"C" if p else b"" for p in point], CUTOFF, dflags=self.dflags)

    def model(self, found):
        import sizingmodel
        co, ci, cf, ho, hi = found
        rt = self.reads
        return sizingmodel.sizing(rt.start, rt.contig_off, rt.max_span, self.sites.pos, self.rcontig, self.start, self.end, self.vartype, self.dflags,
                                  CUTOFF, co, ho, hi, no_extended=self.no_extended)

    def branches(self, found):
        import sizingmodel
        co, ci, cf, ho, hi = found
        rt = self.reads
        return sizingmodel.branch_stats(rt.start, rt.contig_off, rt.max_span, self.sites.pos, self.rcontig, self.start, self.vartype, self.dflags,
                                        co, ho, hi, no_extended=self.no_extended)


def _around(v, span=16):
    """het-site positions whose searched values (hp + 1, hp - span) are v - 1, v, v + 1"""
    return [v - 2, v - 1, v, v + span - 1, v + span, v + span + 1]


# ---- contig sizes and alignments
CONTIG_RECORDS = [5, 7, 0, 1, 8, 9, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, 15818]


def contig_sizes_case():
    """Contigs of every size at which the search takes another path (the mid level above 128 records, the coarse level above 8192), none of
    the larger ones starting on a multiple of 8, 64 or 4096: the 5- and 7-record contigs in front see to that.  The 8193-record contig holds
    exactly one coarse entry, the 15818-record one three; it ends 40 records past a multiple of 4096."""
    starts = [100 + 3 * np.arange(k, dtype=np.int64) for k in CONTIG_RECORDS]
    rt = make_reads(starts)
    off = rt.contig_off
    for c, k in enumerate(CONTIG_RECORDS):
        if k > 128:
            assert off[c] % 8 and off[c] % 64 and off[c] % 4096
    assert (int(off[15]) >> 12) - ((int(off[14]) + 4095) >> 12) == 1 and (int(off[16]) >> 12) - ((int(off[15]) + 4095) >> 12) == 3
    assert int(off[16]) % 4096 == 40
    sites, dnms = [], []
    for c, k in enumerate(CONTIG_RECORDS):
        s = starts[c]
        clo = int(off[c])
        if k == 0:
            sites.append([100, 120, 300])
            dnms.append(dict(contig=c, start=110))
            continue
        first, last = int(s[0]), int(s[-1])
        p = [first - 30, first - 20] + _around(first) + _around(last) + [last + 20, last + 40]
        at = [first - 5, first + 2, last + 1, last + 30]  # some values fall below the first start (-> clo), some above the last (-> chi)
        if k > 128:  # every cell boundary of the index: the contig's first and last entry of every level, and every coarse entry
            marks = set()
            for sh in (3, 6, 12):
                lo_k, hi_k = (clo + (1 << sh) - 1) >> sh, (clo + k - 1) >> sh
                marks.update(x << sh for x in (lo_k, lo_k + 1, hi_k - 1, hi_k) if clo <= (x << sh) < clo + k)
                if sh == 12:
                    marks.update(x << sh for x in range(lo_k, hi_k + 1) if clo <= (x << sh) < clo + k)
            for gidx in sorted(marks):
                v = int(s[gidx - clo])
                p += _around(v)
                at += [v + 1, v - 40]
        sites.append([x for x in p if x >= 0])
        dnms += [dict(contig=c, start=x) for x in sorted(set(at)) if x >= 0]
    return Case("contig_sizes", rt, make_sites(sites), dnms, search_dist=200)


# ---- ties
def ties_case():
    """Runs of equal starts of length 9, 65, 130 and 4100 that straddle an 8-record, a 64-record and (the last) both 4096-record boundaries of
    a 8995-record contig behind a 5-record one; het sites whose searched values are the run's start and its neighbours."""
    runs = {100: 9, 250: 65, 600: 130, 4094: 4100}  # global record index of the run's first record -> its length
    n_glob, clo = 9000, 5
    assert 100 < 104 < 109 and 250 < 256 < 315 and 600 < 640 < 704 < 730 and 4094 < 4096 < 8192 < 8194
    st, pos, g, run_pos = [], 1000, clo, []
    while g < n_glob:
        if g in runs:
            st += [pos] * runs[g]
            run_pos.append(pos)
            g += runs[g]
        else:
            st.append(pos)
            g += 1
        pos += 2
    rt = make_reads([100 + 3 * np.arange(5), np.array(st, np.int64)])
    assert rt.n_segs == n_glob and int(rt.start[4096]) == int(rt.start[8192]) == run_pos[3]
    p, dnms = [], []
    for v in run_pos:
        p += _around(v)
        dnms += [dict(contig=1, start=v), dict(contig=1, start=v - 30), dict(contig=1, start=v + 40)]
    dnms.append(dict(contig=1, start=run_pos[3], vartype=abi.VT_DEL, end=run_pos[3] + 500))
    return Case("ties", rt, make_sites([[100, 110], p]), dnms, search_dist=300)


def long_span_case():
    """One 3000M record first in a 200-record contig: the contig's span is 3000 and hp - span is negative for every site near its start."""
    rt = make_reads([100 + 3 * np.arange(5), np.concatenate([[10], 20 + 4 * np.arange(199)]).astype(np.int64)], long_first=(1, 3000))
    assert int(rt.max_span[1]) == 3000
    p = [5, 9, 10, 11, 30, 200, 400, 799, 2990, 3010, 3011, 3026, 3500]
    dnms = [dict(contig=1, start=x) for x in (8, 10, 300, 810, 3000, 3400)] + [dict(contig=1, start=50, vartype=abi.VT_DEL, end=400)]
    return Case("long_span", rt, make_sites([[100], p]), dnms, search_dist=600)


# ---- staged and far chains
def _dense_tables():
    rt = make_reads([100 + 3 * np.arange(5), 1000 + np.arange(30000, dtype=np.int64)])
    return rt, make_sites([[100], 1000 + 40 * np.arange(750)])


def dense_case(search_dist):
    """One record per base over 30 000 bases, a site every 40 bases.  search_dist 5000: a DNM's het sites span about 10 000 records, more than
    the 64 x 64 the stage covers -- far chains; 1500: none.  The DNMs past the contig's end have their lowest bound within the last 4096 records
    (`whole`), the last two so near the end that fewer than 64 entries are staged."""
    rt, sites = _dense_tables()
    at = [1003, 4000, 11000, 20003, 27000, 31500, 32500, 34000, 35900] if search_dist >= 5000 else [1003, 2000, 11000, 27000, 29990, 31000, 31900, 32400]
    return Case("dense_%d" % search_dist, rt, sites, [dict(contig=1, start=x) for x in at], search_dist=search_dist)


# ---- groups and lanes
LANE_NH = [0, 1, 15, 16, 17, 40]
BATCH_SIZES = [1, 15, 16, 17, 33, 255]


def lanes_pool(no_extended=False):
    """255 DNMs over a 2000-record contig with clusters of 0, 1, 15, 16, 17 and 40 sites (search_dist 120, the clusters 600 bases apart): DNMs
    without candidates between DNMs with them, rcontig -1, the fetch fall-back, DEL-typed DNMs whose start - cutoff is negative."""
    rt = make_reads([100 + 3 * np.arange(5), 100 + 2 * np.arange(2000, dtype=np.int64)])
    centre = [400 + 600 * k for k in range(len(LANE_NH))]
    p = []
    for c0, nh in zip(centre, LANE_NH):
        p += [c0 - 100 + 5 * j for j in range(nh)]
    dnms = []
    for i in range(255):
        k = (i * 5 + 2 + i // 7) % len(LANE_NH)
        d = dict(contig=1, start=centre[k] + (i % 11) - 5)
        if i % 13 == 5:
            d["rcontig"] = -1
        elif i % 13 == 7:
            d["dflags"] = abi.DF_FETCH_FALLBACK
        elif i % 13 == 9:
            d.update(vartype=abi.VT_DEL, end=d["start"] + 300)
        dnms.append(d)
    return Case("lanes" + ("_no_extended" if no_extended else ""), rt, make_sites([[100], p]), dnms, search_dist=120, no_extended=no_extended)


# ---- the reduction
def reduce_big_case():
    """12 289 DNMs -- one more than the 48 x 256 a round of k_bounds_reduce takes -- a handful of het sites each, over three stretches of one
    contig with one, five and fifteen records per five bases: the arena estimates fall into distinct bins."""
    a = 100 + 5 * np.arange(8000, dtype=np.int64)
    b = a[-1] + 5 + np.arange(20000, dtype=np.int64)
    c = b[-1] + 5 + np.repeat(np.arange(8000, dtype=np.int64), 3)
    rt = make_reads([100 + 3 * np.arange(5), np.concatenate([a, b, c])])
    hi = int(c[-1])
    sites = make_sites([[100], 100 + 37 * np.arange((hi - 100) // 37)])
    at = np.linspace(60, hi + 300, 12289).astype(np.int64)
    return Case("reduce_big", rt, sites, [dict(contig=1, start=int(x)) for x in at], search_dist=200)


def all_cases():
    pool = lanes_pool()
    cases = [contig_sizes_case(), ties_case(), long_span_case(), dense_case(5000), dense_case(1500)]
    cases += [pool.subset(k, "lanes_%d" % k) for k in BATCH_SIZES]
    cases += [lanes_pool(no_extended=True).subset(33, "lanes_33_no_extended"), reduce_big_case()]
    return cases


BOTH_UPLOADS = ("contig_sizes", "ties", "long_span")  # run once through the ASCII upload and once through the staged one
