"""Hand-built source tables for the link form of the alignment records, and the forms the product's packer emits of them.

A case is a ReadsTable whose records stand at chosen slots (the record's index in the table decides which round of 256 and which span of 1024
records of the header build it meets), two sets of fetches -- single positions, which stage some 32-base units and list bases, and whole contigs,
which take everything -- and the name of the branch it is there to reach.  form_list(case) and select() push it through io_native.pack_reads and
ReadsSource.select in the packer's switches; tests/linkmodel.py decodes every result, tests/test_link_model.py holds model and packer to the source on
the CPU and asserts what every case reaches, tests/test_link_cases_gpu.py holds every build of the device to the model."""
import numpy as np

from unfazed_amd import abi, io_native
from unfazed_amd.model import ReadsTable

BAM_CODES = "=ACMGRSVTWYHKDBN"
CODE_OF = {ch: k for k, ch in enumerate(BAM_CODES)}
THRESHOLD = 20
ASCII_THRESHOLDS = (0, 20, 255, 300)  # the ASCII route's plane: nothing below 0, the run's default, all but quality 255, beyond the clamp
M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8
PAIRED, PROPER, UNMAPPED, REVERSE, MREVERSE, READ1, READ2 = 1, 2, 4, 16, 32, 64, 128
F1, F2 = PAIRED | PROPER | MREVERSE | READ1, PAIRED | PROPER | REVERSE | READ2
EVERYTHING_HI = 2 ** 31 - 1


def cig(*ops):
    return [(ln << 4) | op for op, ln in ops]


def endpos(start, flag, words):
    """htslib's bam_endpos"""
    if (flag & UNMAPPED) or not words:
        return start + 1
    rl = sum(w >> 4 for w in words if (w & 15) in (M, D, N, EQ, X))
    return start + max(rl, 1)


def bases(length, salt):
    """`length` bases of A / C / G / T, a different row for every salt"""
    k = np.arange(length, dtype=np.int64)
    return "".join("ACGT"[int(x)] for x in ((k * 7 + salt * 13 + (k * k + salt) // 5) & 3))


class Rec:
    """one alignment record of a source table; mate: the Rec it names, or None"""

    def __init__(self, contig, start, length=151, words=None, flag=0, mapq=60, seq=None, low=(), name=None, tlen=0, aux=0, salt=0, qual_low=7, qual=None):
        self.contig, self.start, self.flag, self.mapq, self.name, self.tlen, self.aux = contig, int(start), flag, mapq, name, tlen, aux
        self.words = cig((M, length)) if words is None and length else (words or [])
        self.seq = bases(length, salt) if seq is None else seq
        assert len(self.seq) == length
        if length == 0:
            self.aux |= 4  # UZ_AUX_DECODE_BAD: no SEQ / QUAL / CIGAR
            self.words = []
        self.qual = np.full(length, 35, np.uint8) if qual is None else np.asarray(qual, np.uint8)
        for p in low:
            self.qual[p] = qual_low
        self.mate = None
        self.end = endpos(self.start, flag, self.words)

    def put(self, pos, ch):
        self.seq = self.seq[:pos] + ch + self.seq[pos + 1:]
        return self


def couple(a, b, tlen=None):
    """two records that name each other, one query name, template lengths +-(the pair's span) unless given"""
    a.mate, b.mate = b, a
    b.name = a.name
    a.flag, b.flag = a.flag | F1, b.flag | F2
    a.aux |= 1
    b.aux |= 1
    t = max(a.end, b.end) - a.start
    a.tlen, b.tlen = (t, -t) if tlen is None else tlen
    return a, b


class Case:
    def __init__(self, name, reaches, recs, n_contigs, points, extra=1, lists_only=False, forms=None):
        """points: [(contig, pos)] single-base fetches (+ `extra` bases on); reaches: the branch the case is named for"""
        self.name, self.reaches = name, reaches
        order = sorted(range(len(recs)), key=lambda k: (recs[k].contig, recs[k].start))
        recs = [recs[k] for k in order]
        at = {id(r): k for k, r in enumerate(recs)}
        ids, n = {}, len(recs)
        t = ReadsTable(["c%d" % k for k in range(n_contigs)])
        t.contig_off = np.searchsorted([r.contig for r in recs], np.arange(n_contigs + 1)).astype(np.int64)
        t.start = np.array([r.start for r in recs], np.int32)
        t.end = np.array([r.end for r in recs], np.int32)
        t.flag = np.array([r.flag for r in recs], np.uint16)
        t.mapq = np.array([r.mapq for r in recs], np.uint8)
        t.aux = np.array([r.aux for r in recs], np.uint8)
        t.tlen = np.array([r.tlen for r in recs], np.int32)
        t.mate = np.array([-1 if r.mate is None else at[id(r.mate)] for r in recs], np.int32)
        qn = np.zeros(n, np.uint32)
        for k, r in enumerate(recs):
            if isinstance(r.name, (int, np.integer)):  # an id of the case's own choosing (a table whose ids do not ascend by first appearance)
                qn[k] = int(r.name)
            else:
                qn[k] = ids.setdefault(("rec", k) if r.name is None else r.name, len(ids))
        t.qname = qn
        t.n_cigar = np.array([len(r.words) for r in recs], np.uint16)
        t.cigar_off = np.concatenate([[0], np.cumsum(t.n_cigar.astype(np.int64))])[:-1].astype(np.uint32)
        t.cigar = np.array([w for r in recs for w in r.words] or [0], np.uint32)
        t.l_seq = np.array([len(r.seq) for r in recs], np.uint16)
        rows16 = (t.l_seq.astype(np.int64) + 15) >> 4
        t.sq_off16 = np.concatenate([[0], np.cumsum(rows16)])[:-1].astype(np.uint32)
        t.seq = np.zeros(max(16, 16 * int(rows16.sum())), np.uint8)
        t.qual = np.zeros(t.seq.size, np.uint8)
        for k, r in enumerate(recs):
            o = 16 * int(t.sq_off16[k])
            t.seq[o: o + len(r.seq)] = np.frombuffer(r.seq.encode(), np.uint8)
            t.qual[o: o + len(r.seq)] = r.qual
        ms = np.zeros(n_contigs, np.int32)
        for k in range(n_contigs):
            lo, hi = int(t.contig_off[k]), int(t.contig_off[k + 1])
            if hi > lo:
                ms[k] = int((t.end[lo:hi] - t.start[lo:hi]).max())
        t.max_span = ms
        self.table, self.recs, self.n = t, recs, n
        width = 32 * ((int(t.l_seq.max()) + 31) // 32 + 1) if n else 32
        self.code_mat = np.zeros((n, width), np.uint8)   # BAM's four-bit code of every base, zero beyond the read
        self.qual_mat = np.full((n, width), 255, np.int64)  # ... and its quality (beyond the read: below no threshold the tests use but 300's clamp)
        lut = np.zeros(256, np.uint8)
        for ch, k in CODE_OF.items():
            lut[ord(ch)] = k
        for k, r in enumerate(recs):
            self.code_mat[k, : len(r.seq)] = lut[np.frombuffer(r.seq.encode(), np.uint8)]
            self.qual_mat[k, : len(r.seq)] = r.qual
        self.contig_of = np.array([r.contig for r in recs], np.int32)
        fc = np.unique(self.contig_of).astype(np.int32)
        self.everything = (fc, np.zeros(fc.size, np.int32), np.full(fc.size, EVERYTHING_HI, np.int32), np.full(fc.size, extra, np.uint16))
        pc = np.array([p[0] for p in points], np.int32)
        pp = np.array([p[1] for p in points], np.int32)
        self.points = (pc, pp, pp + 1, np.full(pc.size, extra, np.uint16))
        self.lists_only, self.only_forms = lists_only, forms
        self._sources = {}

    def view(self):
        return abi.reads_view(self.table)

    def source(self, threshold=THRESHOLD, two_bit=True, lists=True):
        key = (threshold, two_bit, lists)
        if key not in self._sources:
            self._sources[key] = io_native.ReadsSource(io_native.pack_reads(self.view(), threshold, two_bit=two_bit, lists=lists, with_end=True))
        return self._sources[key]


# ---- the forms: (name, source switches, select switches, which fetches)
WIDE_KW = [("plain", dict(d16=False)), ("d16", dict(start8=False)), ("start8", dict(pair8=False, narrow8=False)), ("narrow8", dict(pair8=False)), ("pair8", dict())]


def form_list(case, every=False):
    """The link form proper (pair8 + dictionary + masks) in all of its own switches, and every other switch of the packer turned on its own and
    against the five forms of the wide columns: the cross of ALL switches is some six hundred selections a table, where every switch but the three of
    the base lists acts on columns of its own."""
    out = []
    for fetch in ("points", "everything"):
        for tup8 in (True, False):
            for bl, bq in ((True, True), (True, False), (False, False)):
                out.append(("pair8/%s/tup8=%d/bl=%d/bq=%d" % (fetch, tup8, bl, bq), {}, dict(tup8=tup8, base_lists=bl, base_quals=bq), fetch))
        for wname, kw in WIDE_KW[:-1]:
            for with_end in (None, True):
                out.append(("%s/%s/end=%s" % (wname, fetch, with_end), {}, dict(kw, with_end=with_end, base_quals=True), fetch))
        out.append(("pair8/%s/end" % fetch, {}, dict(with_end=True, base_quals=True), fetch))
        out.append(("pair8/%s/cigar_words" % fetch, {}, dict(cigar_compact=False), fetch))
        out.append(("pair8/%s/columns" % fetch, {}, dict(tuples=False), fetch))  # (bl_qlow travels with tup_n_bl only: unfazed_hip.h)
        out.append(("plain/%s/columns/cigar_words/end" % fetch, {}, dict(tuples=False, d16=False, cigar_compact=False, with_end=True), fetch))
        out.append(("pair8/%s/all_units" % fetch, {}, dict(), fetch + "_nomask"))
        out.append(("pair8/%s/seq4" % fetch, dict(two_bit=False), dict(base_lists=False), fetch))
        if not case.lists_only:
            out.append(("pair8/%s/plane" % fetch, dict(lists=False), dict(lists=False), fetch + "_nomask"))
            out.append(("d16/%s/plane/seq4/columns" % fetch, dict(lists=False, two_bit=False), dict(lists=False, tuples=False, start8=False, with_end=True), fetch + "_nomask"))
    if case.only_forms is not None and not every:
        out = [f for f in out if any(f[0].startswith(p) or p in f[0] for p in case.only_forms)]
    return out


def select(case, form, threshold=THRESHOLD):
    """-> (packed view, indices of its records in the source table)"""
    name, src_kw, sel_kw, fetch = form
    src = case.source(threshold, **src_kw)
    f = case.points if fetch.startswith("points") else case.everything
    extra = None if fetch.endswith("_nomask") else f[3]
    part, idx = src.select(f[0], f[1], f[2], want_index=True, extra=extra, **sel_kw)
    return part, idx


# ---- the tables
def _pair_up(recs, prefix):
    """adjacent free records (in table order) become pairs"""
    free = [r for r in sorted(recs, key=lambda r: (r.contig, r.start)) if r.mate is None and getattr(r, "single", False) is False]
    for k in range(0, len(free) - 1, 2):
        if free[k].contig == free[k + 1].contig:
            free[k].name = "%s%d" % (prefix, k)
            couple(free[k], free[k + 1])


def _plain(n, contig=0, base=5000, step=3, salt0=0, length=151):
    return [Rec(contig, base + step * k, length, salt=salt0 + k) for k in range(n)]


def _points_over(recs, every=37):
    out = []
    for c in sorted({r.contig for r in recs}):
        lo = min(r.start for r in recs if r.contig == c)
        hi = max(r.end for r in recs if r.contig == c)
        out += [(c, p) for p in range(lo + 5, hi, every)]
    return out


def case_counts(n):
    recs = _plain(n)
    for k, r in enumerate(recs):
        r.mapq = 60 if k % 5 else 17
        if k % 11 == 0 and len(r.seq):
            r.qual[(k * 7) % len(r.seq)] = 3
    _pair_up(recs, "p")
    return Case("count_%d" % n, "n = %d: the last round / the last span / k_tup_expand's tail at n mod 4 = %d" % (n, n % 4), recs, 1, _points_over(recs, 61),
                forms=("pair8/points/tup8", "pair8/everything/tup8", "plain/", "d16/"))


def case_edges():
    """lengths, CIGARs, bases, qualities, start differences and every pair code, at chosen slots of three spans"""
    n = 2100
    gaps = np.full(n, 2, np.int64)
    gaps[40], gaps[41], gaps[42], gaps[43] = 0, 254, 255, 100000  # start differences 0 / 254 / 255 (the escape value as a real value) / a large gap
    starts = 5000 + np.cumsum(gaps)
    contig = np.where(np.arange(n) < 1500, 0, 1)  # a contig change: the start falls back
    starts[1500:] -= starts[1500] - 700
    recs = [Rec(int(contig[k]), int(starts[k]), salt=k) for k in range(n)]

    def redo(k, **kw):
        recs[k] = Rec(int(contig[k]), int(starts[k]), salt=k, **kw)
        recs[k].single = True
        return recs[k]
    # lengths (records on their own: NEW without a mate); IUPAC codes, N and '=' and low qualities at 0, 31, 32 and l_seq - 1
    for j, L in enumerate((0, 1, 31, 32, 33, 64, 151, 255, 256)):
        r = redo(60 + j, length=L)
        for q, (p, ch) in enumerate(((0, "N"), (31, "R"), (32, "="), (L - 1, "Y"))):
            if 0 <= p < L:
                r.put(p, ch)
                r.qual[p] = 5 + q
    # CIGARs
    redo(80, words=cig((EQ, 151)))
    redo(81, words=cig((X, 151)))
    redo(82, words=cig((M, 100)))                       # one M shorter than the read
    redo(83, words=cig((I, 151)))                       # reference length 0: end = start + 1
    redo(84, words=cig((S, 151)))
    redo(85, words=cig((M, 50), (D, 7), (M, 51), (N, 300), (M, 50)))
    redo(86, flag=UNMAPPED, words=cig((M, 151)))        # flag 4 with a CIGAR: end = start + 1
    redo(87, words=[])                                  # n_cigar 0 with bases
    redo(88, words=cig(*([(M, 1), (D, 1)] * 149 + [(M, 1), (I, 1)])))  # 300 operations over 151 bases: more than a span's LDS room by itself
    assert len(recs[88].words) == 300
    redo(89, length=100, words=cig((M, 100)), mapq=0)
    # qualities: counts of 0 .. 255 low bases (300: the wide case)
    for j, cnt in enumerate((0, 1, 10, 11, 254, 255)):
        redo(100 + j, length=256, low=tuple(range(cnt)) if cnt > 11 else tuple((k * 25 + 3) % 256 for k in range(cnt)))
    redo(110, low=(0, 31, 32, 150))
    for k in (112, 113, 114, 115):  # bases that are not A / C / G / T inside paired records' units, at the unit edges
        recs[k].put(0, "N").put(31, "K").put(32, "N").put(150, "B")
    recs[116].put(64, "=")  # '=' keeps a record off the list form
    # pairs at chosen slots
    def pair(a, b, name, **kw):
        recs[a].name = name
        return couple(recs[a], recs[b], **kw)
    pair(250, 260, "round_edge")               # FIRST / SECOND across a round edge
    pair(255, 507, "dist252")                  # distance 252 from a round's last record: across two rounds
    pair(1023, 1024, "span_edge")              # across a span edge: k_pair_link's job
    pair(1000, 1040, "span_edge2")
    pair(300, 301, "own_tlen", tlen=(400, -400))   # SECOND_TLEN
    recs[303] = Rec(0, int(starts[303]), salt=303, words=cig((M, 100), (D, 500), (M, 51)))
    pair(302, 303, "second_ends_later")        # tlen from max(end)
    pair(310, 311, "lopsided", tlen=(300, -299))  # template lengths that are no +-t: spelled out (NEW + OLD with mates)
    pair(320, 320 + 253, "too_far")            # one beyond the largest distance: spelled out
    recs[330].name, recs[331].name, recs[332].name = "three", "three", "three"  # a name carried by three records
    couple(recs[330], recs[331])
    recs[332].single = True
    recs[332].flag = PAIRED | 2048
    recs[332].aux |= 2  # UZ_AUX_HAS_SA
    recs[340].single = recs[341].single = True  # a one-way mate link
    recs[340].name = recs[341].name = "one_way"
    recs[340].mate = recs[341]
    recs[340].flag, recs[341].flag = F1, F2
    recs[350].single = True  # NEW without a mate
    recs[351].single = True
    recs[351].name = "round_edge"  # OLD without a mate
    for k in range(1100, 1400, 7):  # mapping qualities and flags of their own: more combinations
        recs[k].mapq = k % 50
    for k in range(1600, 1700):  # mates 200 bases on: a fetch that returns the one reaches the other only as a mate, staged without its bases
        pair(k, k + 100, "far%d" % k)
    _pair_up(recs, "e")
    # contig 0: a position every 37 bases; contig 1: two positions -- records 1625 .. 1700 with rows, 1725 .. 1764 without bases, 1765 .. 1840 with rows
    pts = _points_over([r for r in recs if r.contig == 0], 37) + [(1, recs[1650].start + 100), (1, recs[1790].start + 100)]
    def fetched(k):  # the first fetched base of record k
        return min(p for c, p in pts if c == recs[k].contig and p >= recs[k].start) - recs[k].start
    recs[116].seq = bases(151, 116)
    recs[116].put(fetched(116), "=")   # '=' at a fetched position keeps the record off the list form
    recs[113].put(fetched(113), "N")   # N and another IUPAC code as listed bases: two-bit code 0 and an exception
    recs[114].put(fetched(114) + 1, "S")
    return Case("edges", "every length, CIGAR shape, base code, quality count, start difference and pair code", recs, 2, pts)


def case_wide():
    """reads longer than 256 bases: two-byte positions (qlow_pos_wide, bl_wide) -> the build from memory; masks at the 480-base limit"""
    recs = _plain(64, step=40)
    lengths = {5: 257, 6: 300, 9: 480, 10: 481, 20: 300, 21: 481, 22: 480}
    for k, L in lengths.items():
        recs[k] = Rec(0, recs[k].start, L, salt=k)
    recs[6].qual[:] = 2          # 300 low bases: the count saturates at 255
    for p in (0, 256, 299):
        recs[20].qual[p] = 1
        recs[20].put(p, "N")
    for p in (0, 31, 32, 479, 448):
        recs[9].qual[p] = 1
    recs[9].put(479, "N").put(448, "M")
    recs[10].put(480, "N").qual[480] = 0
    recs[22].qual[470] = 4
    _pair_up(recs, "w")
    pts = _points_over(recs, 29) + [(0, recs[9].start + 479), (0, recs[10].start + 480), (0, recs[20].start + 256), (0, recs[20].start + 299)]
    return Case("wide", "l_seq 257 / 300: qlow_pos_wide and bl_wide; 480 bases: the last unit a mask can name; 481: UZ_UMASK_ALL", recs, 1, pts, extra=0)


def case_dict(combos, n=600):
    """`combos` combinations of the small columns in use (tup8's hot table holds 255)"""
    recs = _plain(n)
    _pair_up(recs, "d")
    for k, r in enumerate(recs):  # combination j: flag from its parity, mapping quality and the SA bit from the rest
        j = k % combos
        r.flag = F1 if j % 2 == 0 else F2
        r.mapq = (j // 2) % 251
        if j // 2 >= 251:
            r.aux |= 2
    return Case("dict_%d" % combos, "%d combinations in at most 1024 records" % combos, recs, 1, [], forms=("pair8/everything/tup8", "pair8/everything/columns"))


def case_dict_edges():
    """the one-byte dictionary index: 256 combinations, the one the hot table has no room for at the first and the last record of two spans"""
    n = 2048
    recs = _plain(n)
    _pair_up(recs, "d")
    for k, r in enumerate(recs):
        j = 255 if k in (0, 1023, 1024, 2047) else k % 255
        r.flag = F1 if j % 2 == 0 else F2
        r.mapq = (j // 2) % 251
    return Case("dict_edges", "tup8 escapes at records 0, 1023, 1024 and 2047", recs, 1, [], forms=("pair8/everything/tup8=1/bl=1/bq=1",))


def case_room_cigar():
    """travelled CIGAR words of a span: exactly UZ_PL_CIG (256), then one more, then a span well inside"""
    recs = _plain(2300)
    two, three = cig((M, 100), (S, 51)), cig((S, 10), (M, 100), (S, 41))
    for k in range(128):
        recs[8 * k].words = list(two)
    for k in range(127):
        recs[1024 + 8 * k].words = list(two)
    recs[1024 + 1020].words = list(three)
    recs[2100].words = list(two)
    recs[2100].mapq = 33  # (a combination of its own: tests/linkrefusals.py gives it a simple-CIGAR code)
    for r in recs:
        r.end = endpos(r.start, r.flag, r.words)
    _pair_up(recs, "g")
    return Case("room_cigar", "UZ_PL_CIG: 256 / 257 travelled CIGAR words in a span", recs, 1, [], forms=("pair8/everything/tup8=1/bl=1/bq=1", "pair8/everything/end"))


def case_room_esc():
    """escape entries of a span: exactly UZ_PL_ESC (64), then one more; escapes at the first and last record of a span"""
    n = 2300
    gaps = np.full(n, 2, np.int64)
    gaps[np.arange(1, 64) * 16] = 300     # span 0: the first record's start + 63 gaps = 64
    gaps[1024 + np.arange(0, 64) * 15] = 300  # span 1: 65, the first at its first record ...
    gaps[2047] = 300                      # ... the last at its last
    gaps[2048 + 5] = 300
    starts = 5000 + np.cumsum(gaps)
    recs = [Rec(0, int(starts[k]), salt=k) for k in range(n)]
    _pair_up(recs, "x")
    return Case("room_esc", "UZ_PL_ESC: 64 / 65 escapes in a span, at its first and last record", recs, 1, [], forms=("pair8/everything/tup8=1/bl=1/bq=1", "pair8/everything/tup8=0/bl=1/bq=1"))


def case_room_qpos():
    """listed low-quality positions of a span: exactly UZ_PL_QP (4096), then one more"""
    recs = _plain(2300)
    for k, r in enumerate(recs[:2048]):
        for p in (3, 40, 77, 140):
            r.qual[(p + k) % 151] = 9
    recs[1500].qual[:] = 35
    for p in (0, 31, 32, 64, 150):
        recs[1500].qual[p] = 9
    recs[2100].qual[5] = 1
    _pair_up(recs, "q")
    return Case("room_qpos", "UZ_PL_QP: 4096 / 4097 listed low-quality positions in a span", recs, 1, [], lists_only=True,
                forms=("pair8/everything/tup8=1/bl=0", "pair8/everything/tup8=1/bl=1/bq=0", "pair8/everything/all_units"))


def case_room_bl():
    """listed bases of a span: exactly UZ_PL_BL (4096), then one more; five fetch points on the record that brings it"""
    s0, s1 = 5000, 6000
    recs = [Rec(0, s0, salt=k) for k in range(1024)] + [Rec(0, s1 - 5, salt=7)] + [Rec(0, s1, salt=3 * k) for k in range(1023 + 101)]
    recs[1024].single = True
    for k, r in enumerate(recs):
        if k % 3 == 0:
            r.qual[(s0 + 50 - r.start) % 151] = 2
            r.qual[(s1 + 90 - r.start) % 151] = 2
    recs[5].put(10, "N")
    recs[1030].put(50, "W")
    _pair_up(recs, "b")
    pts = [(0, s0 + p) for p in (10, 50, 90, 130)] + [(0, s1 - 3)] + [(0, s1 + p) for p in (10, 50, 90, 130)]
    return Case("room_bl", "UZ_PL_BL: 4096 / 4097 listed bases in a span", recs, 1, pts, extra=0, lists_only=True,
                forms=("pair8/points/tup8=1/bl=1", "pair8/points/tup8=0/bl=1/bq=1", "d16/points/end=None", "plain/points/end=True"))


def case_b0(r):
    """a span whose slice of bl_code / bl_qlow starts r entries into a byte (r = the listed bases in front of it, mod 8)"""
    s0, s1 = 5000, 6000
    recs = [Rec(0, s0 - 20, salt=90 + k) for k in range(r)] + [Rec(0, s0, salt=k) for k in range(1024 - r)] + [Rec(0, s1, salt=5 * k + r) for k in range(76)]
    for k, rec in enumerate(recs):
        if k % 3 == 1:
            rec.qual[(s1 + 50 - rec.start) % 151] = 2
        if k % 7 == 2:
            rec.qual[(s0 + 50 - rec.start) % 151] = 2
    _pair_up(recs, "r")
    pts = [(0, s0 - 15), (0, s0 + 50), (0, s1 + 50)]
    return Case("b0_%d" % r, "a span's first listed base at residue %d mod 8 (mod 4: %d)" % (r, r & 3), recs, 1, pts, extra=0, lists_only=True,
                forms=("pair8/points/tup8=1/bl=1", "d16/points/end=None"))  # (d16: base lists and their quality bits outside the link form)


def case_sentinels():
    """the escape and no-mate values of the difference columns as real values: the packer must escape them, the device must not confuse them"""
    n = 33100
    recs = [Rec(0, 5000 + k, 40, salt=k % 97) for k in range(n)]
    for r in recs:
        r.single = True
    ids = np.arange(n, dtype=np.int64) * 2
    at = 100
    for d in (32767, -32767, -32768, 32766, -127, -128, 126, 127, -126, -129, 128):  # 16- and 8-bit name-id differences
        ids[at:] += d - 2
        at += 3
    for k, r in enumerate(recs):
        r.name = int(ids[k] + 70000)
    for k, t in zip((200, 201, 202, 203), (32767, -32767, -32768, -32769)):
        recs[k].tlen = t
    def link(a, b):
        recs[a].mate, recs[b].mate = recs[b], recs[a]
    link(10, 10 + 32767)      # mate_d 32767 / -32767
    link(300, 300 + 32768)    # 32768 / -32768
    link(400, 400 + 127)      # mate_d8 127 / -127
    link(410, 410 + 128)      # 128 / -128
    link(420, 420 + 126)
    link(430, 431)            # mate distances 1, 252, 253
    link(440, 440 + 252)
    link(450, 450 + 253)
    # start differences: 32767 forward, and -32767 / -32768 back over contig changes
    c1 = [Rec(1, recs[-1].start - 32767 + k, 40, salt=k) for k in range(3)]
    c1[1].start = c1[0].start + 32767
    c1[2].start = c1[1].start + 32768
    c2 = [Rec(2, c1[2].start - 32768, 40, salt=1)]
    for r in c1 + c2:
        r.single = True
        r.end = endpos(r.start, r.flag, r.words)
        r.name = int(ids[-1] + 70000 + 5)
    return Case("sentinels", "32767 / -32767 / -32768 and -127 / -128 / 126 / 127 as real differences; mate distances 1, 252, 253", recs + c1 + c2, 3, [],
                forms=("d16/everything/end=None", "narrow8/everything/end=None", "start8/everything/end=None", "plain/everything/end=None"))


def panel():
    out = [case_edges(), case_wide(), case_room_cigar(), case_room_esc(), case_room_qpos(), case_room_bl(), case_sentinels()]
    out += [case_dict(c) for c in (1, 255, 256, 257)] + [case_dict(300, n=1000), case_dict_edges()]
    out += [case_b0(r) for r in range(8)]
    out += [case_counts(n) for n in (1, 255, 256, 257, 1023, 1024, 1025, 2049, 1026, 1027)]
    return out
