"""Hand-built edge tables for the site stage (k_build_ab_lut, k_site_scan, k_site_scan_wide, k_window_wave, k_window_region, k_scan2,
k_cnv_count), shared by tests/test_site_model.py (the numpy model of tests/sitemodel.py against the C oracle, on the CPU) and
tests/test_site_edges_gpu.py (the device against the oracle).  Pure numpy.

A Table holds a trio's columns twice: as the reference sees them (`true`: genotype, depths and qualities per member, -1 = missing) and in
the form the library takes (packed genotype byte, 16-bit columns with 0xFFFF = missing, the list of sites too deep for 16 bits)."""
import itertools

import numpy as np

from sitemodel import HET, HOM_ALT, HOM_REF, UNKNOWN
from unfazed_amd import abi

MIN_DEPTHS = (10, -5, 0, 1)
MIN_GQS = (20, -1, 0, 255)
GOOD_GQ = 32767
CHUNK = 256 * 8  # sites per workgroup trip of k_site_scan (SPT = 8)
BIG_N = 4096 * CHUNK + CHUNK + 5  # a second trip of the grid stride, a partial chunk, a scalar tail
BATCH_FAMS, BATCH_N = 256, 16 * CHUNK + CHUNK + 3  # nb = max(ceil(4096 / 256), 16) = 16 workgroups per family, 18 chunks


class Table:
    def __init__(self, name, gt, rd, ad, gq, complex_=None, contigs=None, wide_sites=None, wide_fill=0xFFFF):
        """gt, rd, ad, gq: [3][n] integers in kid, dad, mom order; contigs: one ascending position array per contig (default: one contig,
        a site every 10 bases).  wide_sites: the sites to list as wide (default: those with a depth above 32767); their 16-bit depths
        are `wide_fill`."""
        self.name = name
        gt, rd, ad, gq = (np.asarray(x, np.int64) for x in (gt, rd, ad, gq))
        n = gt.shape[1]
        self.true = (gt, rd, ad, gq)
        self.complex = np.zeros(n, bool) if complex_ is None else np.asarray(complex_, bool)
        if contigs is None:
            contigs = [np.arange(n, dtype=np.int64) * 10]
        self._finish(contigs)
        deep = (np.maximum(rd, ad) > 32767).any(axis=0)
        ws = np.nonzero(deep)[0] if wide_sites is None else np.unique(np.asarray(wide_sites, np.int64))
        assert np.all(np.isin(np.nonzero(deep)[0], ws))  # (a listed site need not be deep; a deep one must be listed)
        to16 = lambda x: np.where(x < 0, 0xFFFF, x).astype(np.uint16)  # noqa: E731
        r16, a16 = np.where(deep, 0, rd), np.where(deep, 0, ad)
        assert r16.max(initial=0) <= 32767 and a16.max(initial=0) <= 32767 and gq.max(initial=0) <= 32767 and min(rd.min(initial=0), ad.min(initial=0), gq.min(initial=0)) >= -1
        self.gt = (gt[0] | (gt[1] << 2) | (gt[2] << 4)).astype(np.uint8)
        self.rd, self.ad, self.gq = to16(r16), to16(a16), to16(gq)
        self.wide = None
        if ws.size:
            self.rd[:, ws] = wide_fill
            self.ad[:, ws] = wide_fill
            self.wide = (ws, rd[:, ws].astype(np.int32), ad[:, ws].astype(np.int32))
        self.base = None

    def _finish(self, contigs):
        sizes = [len(p) for p in contigs]
        for p in contigs:
            assert len(p) < 2 or np.all(np.diff(np.asarray(p, np.int64)) >= 0)
        self.contig_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.pos = np.concatenate([np.asarray(p, np.int64) for p in contigs] + [np.zeros(0, np.int64)]).astype(np.int32)
        self.n_sites = int(self.pos.size)
        assert self.n_sites == len(self.complex)
        self.contigs = ["c%d" % k for k in range(len(contigs))]
        self.sflags = self.complex.astype(np.uint8)  # UZ_SF_COMPLEX = 1
        self.ref_base = np.full(self.n_sites, ord("A"), np.uint8)
        self.alt_base = np.full(self.n_sites, ord("C"), np.uint8)

    @classmethod
    def tiled(cls, base, n, roll, name=None):
        """n sites drawn from `base` (no wide list) by a fixed walk that starts at `roll`: site i is base site (roll + 7919 i) mod base.n"""
        assert base.wide is None and base.base is None
        t = cls.__new__(cls)
        t.name = name or "%s_n%d_r%d" % (base.name, n, roll)
        t.base, t.idx = base, (roll + 7919 * np.arange(n, dtype=np.int64)) % base.n_sites
        t.true, t.wide = None, None
        t.complex = base.complex[t.idx]
        t.gt, t.rd, t.ad, t.gq = base.gt[t.idx], base.rd[:, t.idx], base.ad[:, t.idx], base.gq[:, t.idx]
        t._finish([np.arange(n, dtype=np.int64)])
        return t

    def true_columns(self):
        if self.base is not None:
            return tuple(x[:, self.idx] for x in self.base.true)
        return self.true

    def model_classes(self, P):
        """a class is a function of the site alone: a tiled table's classes are its base's, drawn the same way"""
        import sitemodel
        if self.base is not None:
            return self.base.model_classes(P)[self.idx]
        return sitemodel.classes(P, self.complex, *self.true)

    def sites_view(self):
        return abi.sites_view(self)

    def family_columns(self):
        return self.gt, self.rd, self.ad, self.gq, self.wide

    def family_view(self):
        return abi.family_view(*self.family_columns())


# ---------------------------------------------------------------------------------------------------------------------- K1, thresholds
AB_POINTS = (0.0, 0.2, 0.8, 1.0, 0.5, 0.33, 0.67)
TOTALS = sorted({-2, -1, 0, 1, 2, 3, 4, 5, 509, 510, 511, 512, 1000, 32766, 32767, 32768, 65533, 65534} |
                {m + d for m in MIN_DEPTHS for d in (-1, 0, 1) if m + d >= -2})
GQS = sorted({-1, GOOD_GQ} | {m + d for m in MIN_GQS for d in (-1, 0) if m + d >= -1})


def depth_pairs():
    """(rd, ad) over the grid of totals and alt depths: every value is -1 (missing) or in 0..32767"""
    ok = lambda v: v == -1 or 0 <= v <= 32767  # noqa: E731
    out = []
    for t in TOTALS:
        A = {-1, 0, 1, t - 1, t}
        for x in AB_POINTS:
            for f in (int(np.floor(x * t)), int(np.ceil(x * t))):
                A |= {f - 1, f, f + 1}
        out += [(t - a, a) for a in sorted(A) if ok(a) and ok(t - a)]
    return out


# the members held good while one is varied: far from every threshold of every parameter set that leaves their genotype alone
_GOOD = {HET: (20, 20), HOM_REF: (36, 4), HOM_ALT: (4, 36), UNKNOWN: (20, 20)}


def _threshold_rows():
    pairs = depth_pairs()
    rows = []  # (gt3, rd3, ad3, gq3)
    for member, g in itertools.product(range(3), (HOM_REF, HET, UNKNOWN, HOM_ALT)):
        if member == 0:
            gts = [g, HET, HOM_REF]  # a pattern: the kid's test shows in the CAND bit
        else:
            other = HOM_REF if g == HET else HET  # the kid is het: the parents' tests show in the HET bit
            gts = [HET, g, other] if member == 1 else [HET, other, g]
        for (r, a), q in itertools.product(pairs, GQS):
            rd, ad, gq = ([_GOOD[x][0] for x in gts], [_GOOD[x][1] for x in gts], [GOOD_GQ] * 3)
            rd[member], ad[member], gq[member] = r, a, q
            rows.append((gts, rd, ad, gq))
    return rows


KID_DEPTHS = [(4, 0), (0, 4), (5, 0), (0, 5), (2, 2), (2, 3), (3, 2), (3, 3), (2, 8), (8, 2), (3, 7), (7, 3), (3, 8), (8, 3), (5, 5), (5, 6),
              (67, 33), (33, 67), (66, 34), (34, 66), (50, 50), (1, 1), (30, 10), (10, 30), (-1, 6), (6, -1), (0, 0)]
PARENT_DEPTHS = [  # per genotype; the sums of two parents' balances fall below, on and above 1.0
    {HOM_REF: (36, 4), HET: (20, 20), HOM_ALT: (4, 36), UNKNOWN: (20, 20)},
    {HOM_REF: (40, 0), HET: (20, 20), HOM_ALT: (0, 40), UNKNOWN: (20, 20)},  # alt + ref = 1.0, alt + het = 1.5, het + ref = 0.5
    {HOM_REF: (32, 8), HET: (8, 32), HOM_ALT: (2, 38), UNKNOWN: (20, 20)},  # 0.8 + 0.2 = 1.0 exactly, both on their thresholds
    {HOM_REF: (36, 4), HET: (-1, 1), HOM_ALT: (4, 36), UNKNOWN: (20, 20)},  # a parent with total 0: +inf
    {HOM_REF: (36, 4), HET: (0, 0), HOM_ALT: (4, 36), UNKNOWN: (20, 20)},  # ... and nan
]


def _cnv_rows():
    rows = []
    for gts in itertools.product((HOM_REF, HET, UNKNOWN, HOM_ALT), repeat=3):  # the unique-allele table: all 64 triples
        for pd, (kr, ka) in itertools.product(PARENT_DEPTHS, KID_DEPTHS):
            rows.append((list(gts), [kr, pd[gts[1]][0], pd[gts[2]][0]], [ka, pd[gts[1]][1], pd[gts[2]][1]], [GOOD_GQ] * 3))
    return rows


_CACHE = {}


def threshold_table():
    """the threshold blocks (one per varied member and genotype), the CNV block, and the CNV block again under the complex bit"""
    if "thr" not in _CACHE:
        thr, cnv = _threshold_rows(), _cnv_rows()
        rows = thr + cnv + cnv
        cols = [np.array([r[k] for r in rows], np.int64).T for k in range(4)]
        cx = np.zeros(len(rows), bool)
        cx[len(thr) + len(cnv):] = True
        t = Table("thresholds", *cols, complex_=cx)
        t.n_threshold_rows, t.n_cnv_rows = len(thr), len(cnv)
        _CACHE["thr"] = t
    return _CACHE["thr"]


def _nudge(w, d):
    return tuple(float(np.nextafter(x, d)) for x in w)


DEFAULT_AB = dict(ab_homref=(0.0, 0.2), ab_homalt=(0.8, 1.0), ab_het=(0.2, 0.8))
SPECIAL_AB = dict(empty=(0.6, 0.4), beyond=(-0.5, 1.5), inf=(-np.inf, np.inf), half_inf=(0.5, np.inf))


def threshold_sets():
    sets = [("default", dict(DEFAULT_AB)),
            ("ulp_up", {k: _nudge(w, np.inf) for k, w in DEFAULT_AB.items()}),
            ("ulp_down", {k: _nudge(w, -np.inf) for k, w in DEFAULT_AB.items()})]
    for (sname, w), key in itertools.product(SPECIAL_AB.items(), DEFAULT_AB):
        sets.append(("%s_%s" % (sname, key[3:]), dict(DEFAULT_AB, **{key: w})))
    return sets


def k1_param_sets():
    """every threshold set under every min_depth and min_gt_qual -> [(name, keyword arguments of abi.make_params)]"""
    out = []
    for (tname, ab), md, mq in itertools.product(threshold_sets(), MIN_DEPTHS, MIN_GQS):
        out.append(("%s-d%d-q%d" % (tname, md, mq), dict(ab, min_depth=md, min_gt_qual=mq)))
    return out


SHAPE_PARAMS = [("default", {}), ("ulp_up-d0", dict(dict(threshold_sets())["ulp_up"], min_depth=0)),
                ("inf_het-d0-q0", dict(dict(threshold_sets())["inf_het"], min_depth=0, min_gt_qual=0))]
SHAPE_NS = (1, 7, 8, 9, 2047, 2048, 2049)


def shape_tables():
    base = threshold_table()
    return [Table.tiled(base, n, roll=131 * n) for n in SHAPE_NS]


def big_table():
    return Table.tiled(threshold_table(), BIG_N, roll=5, name="big")


def batch_tables():
    """the families of the batch form: different walks over the threshold table (a family reading a neighbour's pointer shows)"""
    base = threshold_table()
    return [Table.tiled(base, BATCH_N, roll=613 * k + 1) for k in range(BATCH_FAMS)]


# ----------------------------------------------------------------------------------------------------------------------- K1, wide list
WIDE_DEPTHS = (32768, 65535, 100_000, 10 ** 9)
WIDE_N = CHUNK + 5  # one full chunk and a scalar tail


def _wide_pair(g, D, tie):
    """depths of a deep member (the library takes wide depths up to 2^30): 1/6 or, `tie`, exactly on the genotype's threshold"""
    q = min(D, 10 ** 9 // 4)
    if g == HOM_REF:
        return (4 * q, q) if tie else (D, D // 5)
    if g == HOM_ALT:
        return (q, 4 * q) if tie else (D // 5, D)
    return (D, D)


def wide_tables():
    """n_wide of 1 (first site; last site), 256 and 257; the 16-bit depths at the listed sites missing or ordinary"""
    base = Table.tiled(threshold_table(), WIDE_N, roll=77)
    out = []
    fixed = [0] + list(range(1000, 1008)) + list(range(CHUNK, WIDE_N))  # first, one lane's vector, the scalar tail with the last
    for name, sites, fill in (("first", [0], 0xFFFF), ("last", [WIDE_N - 1], 30), ("w256", None, 0xFFFF), ("w257", None, 30)):
        if sites is None:
            want = int(name[1:])
            rest = [s for s in range(3, WIDE_N, 7) if s not in fixed]
            sites = sorted(fixed + rest[: want - len(fixed)])
            assert len(sites) == want
        gt, rd, ad, gq = (x.copy() for x in base.true_columns())
        cx = base.complex.copy()
        for k, s in enumerate(sites):
            D, m = WIDE_DEPTHS[k % 4], k % 3
            gt[:, s] = [(HET, HET, HOM_REF), (HET, HOM_ALT, HET), (HOM_ALT, HET, HOM_REF), (HET, HOM_REF, HOM_ALT)][(k // 4) % 4]
            for j in range(3):
                rd[j, s], ad[j, s] = _GOOD[int(gt[j, s])]
            gq[:, s] = 99
            rd[m, s], ad[m, s] = _wide_pair(int(gt[m, s]), D, tie=(k // 3) % 2 == 1)
            cx[s] = k % 11 == 5  # under the complex bit
            if k % 13 == 7:
                gt[k % 3, s] = UNKNOWN
            if k % 17 == 9:  # total 0 in the list, beside a deep member
                rd[(m + 1) % 3, s], ad[(m + 1) % 3, s] = [(0, 0), (-1, 1), (1, -1)][(k // 17) % 3]
            assert max(int(rd[:, s].max()), int(ad[:, s].max())) <= 2 ** 30  # (and a sum stays below 2^31: the oracle adds in int)
        out.append(Table("wide_" + name, gt, rd, ad, gq, complex_=cx, wide_sites=sites, wide_fill=fill))
    return out


WIDE_PARAMS = [("default", {}), ("inf_het-d0", dict(dict(threshold_sets())["inf_het"], min_depth=0)),
               ("inf_homref-d-5-q-1", dict(dict(threshold_sets())["inf_homref"], min_depth=-5, min_gt_qual=-1))]

# --------------------------------------------------------------------------------------------------------------------------- K2, windows
KIND = {  # gt triple, then (rd, ad) of kid, dad, mom; GQ 99 throughout
    "het": ((HET, HET, HOM_REF), (20, 20), (20, 20), (36, 4)),  # HET | CAND | ALT_DAD
    "del_dad_a": ((HOM_REF, HOM_ALT, HET), (40, 0), (4, 36), (20, 20)),  # kid has the alt parent's allele, the alt parent is dad
    "del_dad_b": ((HOM_ALT, HOM_REF, HET), (0, 40), (36, 4), (20, 20)),  # kid has the ref parent's allele, the ref parent is dad
    "del_mom_a": ((HOM_REF, HET, HOM_ALT), (40, 0), (20, 20), (4, 36)),
    "del_mom_b": ((HOM_ALT, HET, HOM_REF), (0, 40), (20, 20), (36, 4)),
    "dup_dad": ((HET, HOM_ALT, HET), (10, 30), (0, 40), (20, 20)),  # kid 0.75, parents' sum 1.5: alt parent, dad
    "dup_mom": ((HET, HET, HOM_REF), (30, 10), (20, 20), (36, 4)),  # kid 0.25, parents' sum 0.6: ref parent, mom
}


KINDS = list(KIND)


def table_of_kinds(name, kinds, complex_, contigs):
    """kinds: indices into KINDS, one per site"""
    kinds = np.asarray(kinds, np.int64).reshape(-1)
    gt = np.array([KIND[k][0] for k in KINDS], np.int64)[kinds].T
    rd = np.array([[KIND[k][1 + m][0] for m in range(3)] for k in KINDS], np.int64)[kinds].T
    ad = np.array([[KIND[k][1 + m][1] for m in range(3)] for k in KINDS], np.int64)[kinds].T
    return Table(name, gt, rd, ad, np.full(gt.shape, 99), complex_=complex_, contigs=contigs)


CONTIG_SIZES = (0, 1, 64, 65, 4096, 4097, 4160, 262_144, 262_145, 262_209)
EVENT_LENGTHS = (0, 1, 5, 6, 9, 10, 11, 19, 20, 50, 5000, 5001, 9999, 10000, 10001, 50000)  # sd, sd + 1, 2 sd - 1, 2 sd, 2 sd + 1, 10 sd for sd = 5, 5000
SEARCH_DISTS = (0, 5, 5000)
WINDOW_SITES = (0, 1, 63, 64, 65, 127, 128, 129)
RUNS = (2, 64, 130)
END_BASE = 9_500_000


class Dnms:
    def __init__(self):
        self.rows = []

    def add(self, contig, st, en, mult=1, tag=""):
        self.rows.append((contig, st, en, mult, tag))

    def arrays(self, vartypes=(abi.VT_POINT,), rows=None):
        rows = self.rows if rows is None else rows
        n = len(rows)
        return dict(contig=np.array([r[0] for r in rows], np.int32), start=np.array([r[1] for r in rows], np.int32),
                    end=np.array([r[2] for r in rows], np.int32), mult=np.array([r[3] for r in rows], np.uint8),
                    vartype=np.array([vartypes[d % len(vartypes)] for d in range(n)], np.uint8), tags=[r[4] for r in rows])


def probe_indices(n):
    """the first round's probes of the 64-ary search over a contig of n sites (lo + lane * step), lane 1..63"""
    step = (n + 63) >> 6
    return [lane * step for lane in range(1, 64) if lane * step < n - 1]


def window_world():
    """-> (contigs: position arrays, marks: table indices of the class-0 sites, Dnms)"""
    if "world" in _CACHE:
        return _CACHE["world"]
    contigs, dn = [np.arange(37, dtype=np.int64)], Dnms()  # contig 0: a site at pos 0, and every later contig starts off a multiple of 64
    for st, en in ((0, 1), (3, 4), (0, 0), (2, 30), (4, 5004)):  # start 0, start < search_dist: the window is clipped to 1
        dn.add(0, st, en, tag="clip")
    for n in CONTIG_SIZES:
        c = len(contigs)
        p = 1000 + 10 * np.arange(n, dtype=np.int64)
        probes = probe_indices(n) if n > 64 else []
        for q in probes:  # an equal run across every probe index
            p[q - 1] = p[q + 1] = p[q]
        contigs.append(p)
        first, last = (int(p[0]), int(p[-1])) if n else (1000, 1000)
        for st in (100, first, last, last + 7000):  # before the first site, on it, on the last, past it
            dn.add(c, st, st + 1, tag="contig%d" % n)
        dn.add(c, first, last + 100, mult=3, tag="whole_contig%d" % n)
        for k, q in enumerate(probes):
            v = int(p[q])
            dn.add(c, v + 1 + 5, v + 2 + 5, tag="probe")  # search_dist 5: w0 - 1 is the run's position
            if k in (0, 30, len(probes) - 1):
                dn.add(c, v + 1 + 5000, v + 2 + 5000, tag="probe")  # ... and 5000
                dn.add(c, max(v - 40, 0), v - 5, tag="probe_hi")  # w1 of a region (search_dist 5) on the run
    # the block contig: one block of sites per scenario, 100 kb and more apart
    c_blocks = len(contigs)
    pos, marks_local = [], []

    def block(sites, marked=()):
        marked = list(marked)
        for s in sorted(sites):
            assert s >= 0 and (not pos or s >= pos[-1])
            if s in marked:  # (the first site at that position)
                marked.remove(s)
                marks_local.append(len(pos))
            pos.append(s)
    for k, L in enumerate(EVENT_LENGTHS):  # sites on both sides of every edge of both windows, for every search_dist
        st = 1_000_000 + 300_000 * k + 20_000
        en = st + L
        sites = {st - 1, st, en - 1, en}
        for sd, anchor, off in itertools.product(SEARCH_DISTS, (st, en), (-2, -1, 0)):
            sites |= {anchor - sd + off, anchor + sd + off}  # POS = pos + 1: pos = w0 - 2, w0 - 1 (first inside), w1 - 1 (last inside), w1
        mid = (st + en) // 2
        block(sorted(sites | {mid, mid + 1}) + [mid], marked=(mid,))  # two sites at mid: the marked one twice -> class 0 in the shared span
        for mult in ((1, 2, 255) if L >= 5 else (1,)):
            dn.add(c_blocks, st, en, mult=mult, tag="len%d" % L)
    for k, (R, sd, side) in enumerate(itertools.product(RUNS, (5, 5000), ("w0", "w1"))):  # equal-position runs on both sides of an edge
        st = 6_000_000 + 100_000 * k + 20_000
        a = st - sd - 2 if side == "w0" else st + sd - 1
        block([a] * R + [a + 1] * R)
        dn.add(c_blocks, st, st + 1, tag="run%d" % R)
        dn.add(c_blocks, st - 3 * sd - 7, st, tag="run%d_second" % R)  # the same edges on a second window
    for k, n_in in enumerate(WINDOW_SITES):  # windows (search_dist 5000) and regions (0) of exactly n_in sites
        st = 8_000_000 + 100_000 * k
        block([st + 30 + j for j in range(n_in)])
        dn.add(c_blocks, st, st + 1, tag="size%d" % n_in)
        dn.add(c_blocks, st + 25, st + 25 + max(n_in + 10, 25), tag="region%d" % n_in)
    block([END_BASE + j for j in range(5)])
    dn.add(c_blocks, END_BASE + 4, END_BASE + 5, tag="contig_end")  # runs into chi, the next contig's low positions behind it
    dn.add(c_blocks, END_BASE - 20_000, END_BASE + 4, tag="contig_end")
    contigs.append(np.array(pos, np.int64))
    marks = [int(sum(len(p) for p in contigs[:-1])) + m for m in marks_local]
    tail = np.concatenate([END_BASE - 3000 + 60 * np.arange(100), END_BASE + 3000 + np.arange(7)]).astype(np.int64)
    contigs.append(tail)  # its first positions lie inside the window above; its own end is the table's end
    dn.add(len(contigs) - 1, int(tail[-1]), int(tail[-1]) + 1, tag="table_end")
    dn.add(len(contigs) - 1, int(tail[-1]) - 30, int(tail[-1]), mult=2, tag="table_end")
    for c in (-1, len(contigs), 1):  # a contig the table does not have (twice) and an empty one
        dn.add(c, 1000, 1001, tag="no_contig")
    off = np.concatenate([[0], np.cumsum([len(p) for p in contigs])])
    assert all(int(o) % 64 for o in off[1:-1])
    _CACHE["world"] = (contigs, marks, dn)
    return _CACHE["world"]


def window_table(mixed):
    """mixed = False: every site kid-het with good parents (HET and CAND), the marked ones complex (class 0); mixed = True: kinds that
    carry DEL / DUP codes in turn, for the whole-region mode"""
    key = "wt%d" % mixed
    if key not in _CACHE:
        contigs, marks, _ = window_world()
        n = sum(len(p) for p in contigs)
        turn = np.array([KINDS.index(k) for k in ("het", "del_dad_a", "dup_mom", "del_mom_b")])
        kinds = turn[np.arange(n) % 4] if mixed else np.full(n, KINDS.index("het"))
        cx = np.zeros(n, bool)
        cx[marks] = True
        _CACHE[key] = table_of_kinds("windows_mixed" if mixed else "windows", kinds, cx, contigs)
    return _CACHE[key]


WINDOW_RUNS = [(sd, mode) for sd in SEARCH_DISTS for mode in (0, abi.FIND_SECOND_WINDOW, abi.FIND_WHOLE_REGION)]
WHOLE_VARTYPES = (abi.VT_DEL, abi.VT_DUP, abi.VT_OTHER_SV, abi.VT_POINT)
BATCH_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)


def window_dnms(mode):
    _, _, dn = window_world()
    return dn.arrays(WHOLE_VARTYPES if mode & abi.FIND_WHOLE_REGION else (abi.VT_POINT,))


def batch_dnms(size):
    """the world's DNMs repeated to `size`, zero-count DNMs (no such contig) on both sides of every k_scan2 tile edge and at the end"""
    _, _, dn = window_world()
    rows = [dn.rows[d % len(dn.rows)] for d in range(size)]
    for d in range(size):
        if (d > 0 and d % 4096 in (0, 4095)) or d == 2 or (size > 5 and d == size - 1):
            rows[d] = (-1,) + rows[d][1:]
    return dn.arrays(rows=rows)


# ---------------------------------------------------------------------------------------------------------------------------------- K6
CNV_COUNTS = (0, 1, 2, 9, 10, 11, 20, 63, 64, 65, 130)
CNV_PAIRS = list(itertools.product(CNV_COUNTS, repeat=2))  # (n_dad, n_mom) of a DEL; the same region gives a DUP (n_mom, n_dad)
RATIOS = (1, 2, 10)
RB_VALUES = (0, 1, 9, 10, 11)
RB_ROWS = np.array(list(itertools.product(RB_VALUES, repeat=4)), np.int32)
CROSS_PAIRS = [(0, 0), (1, 0), (0, 1), (1, 1), (10, 1), (9, 1), (1, 10), (2, 1)]


def cnv_world():
    """-> (Table, regions: (start, end) per pair of CNV_PAIRS, then two small events)"""
    if "cnv" not in _CACHE:
        rng = np.random.default_rng(64)
        kinds, pos, regions = [], [], []
        for k, (nd, nm) in enumerate(CNV_PAIRS):
            st = 10_000 + 1000 * k
            ks = [("del_dad_a", "del_dad_b")[j % 2] for j in range(nd)] + [("del_mom_a", "del_mom_b")[j % 2] for j in range(nm)]
            ks += ["dup_dad"] * nm + ["dup_mom"] * nd
            ks = [ks[j] for j in rng.permutation(len(ks))]
            kinds += ks
            pos += [st + 1 + j for j in range(len(ks))]
            regions.append((st, st + len(ks) + 25))
            assert regions[-1][1] < st + 1000
        for st in (500_000, 501_000):  # small events: every site inside is left out
            kinds += ["del_dad_a", "del_mom_a", "dup_dad"]
            pos += [st, st + 1, st + 14]
            regions.append((st, st + 15))
        kinds = ["het"] * 11 + kinds  # (contig 0: the events' contig starts off a multiple of 64)
        cx = np.zeros(len(kinds), bool)
        _CACHE["cnv"] = (table_of_kinds("cnv", [KINDS.index(k) for k in kinds], cx, [np.arange(11) * 3, np.array(pos, np.int64)]), regions)
    return _CACHE["cnv"]


def cnv_cases():
    """-> [(name, dnm arrays, rb_counts or None)]: every region as DEL, DUP, other SV and point; then the decision crossed with every
    read-backed row on the pairs with ratio ties"""
    _, regions = cnv_world()
    grid = Dnms()
    for rep in range(2):
        for st, en in regions:
            for _ in WHOLE_VARTYPES:
                grid.add(1, st, en)
    g = grid.arrays(WHOLE_VARTYPES)
    rb = RB_ROWS[(np.arange(len(grid.rows)) * 131 + 17) % len(RB_ROWS)]
    cross = Dnms()
    for pair in CROSS_PAIRS:
        st, en = regions[CNV_PAIRS.index(pair)]
        for _ in RB_ROWS:
            cross.add(1, st, en)
    c = cross.arrays((abi.VT_DEL,))
    return [("grid", g, None), ("grid_rb", g, rb), ("cross", c, np.tile(RB_ROWS, (len(CROSS_PAIRS), 1)))]


def dnms_view(dn):
    n = len(dn["start"])
    return abi.dnms_view(dn["contig"], dn["contig"], dn["start"], dn["end"], dn["vartype"], [b""] * n, [b""] * n, 0.0, mult=dn["mult"])
