"""Hand-built edge panel for the read stage (k_phase: csrc/phase_body.hpp, csrc/k_reads.hip), shared by tests/test_read_edges.py (oracle, kernel
body's CPU twin and reach rule against the reference's recorded answers) and tests/test_read_edges_gpu.py (the device by every route).

Two panels, each one SmallDataset (one kid, samples kid1 / dad1 / mom1, readlen 151): `point_panel()` for SNV / MNP / indel DNMs
(collect_reads_snv, read_collector.py:339-432) and `sv_panel()` for SV breakpoints (collect_reads_sv, :435-602).  A panel holds K cases; a case is
its own DNM, 30 kb from the next on contig "1", with its own sites and its own pairs -- no read or window of one case reaches another, so a
panel is one batch and one device call.  Nothing is drawn: every read, CIGAR, base, quality, flag and tlen is written out below.

A case has a name, the rule it probes (line numbers of the reference's read_collector.py) and named probe pairs with the outcome worked out
by hand.  **Visibility.**  Every site of a case is kid HET, dad HOM_ALT, mom HOM_REF (a candidate site with alt_parent = dad and a het site at
once), and every pair carries the ALT base at every site it covers, so (snv_phaser.py:20-70) a pair grouped with the DNM's allele ("alt") shows in
the record's `dad_reads`, a pair grouped with the other haplotype ("ref") in `mom_reads`, and a pair that no rule took ("none") in neither.  The
builder asserts that every probe pair, itself or through its mate, covers a site of its case, and that the probes of a case do not all expect
the same outcome: each case has a probe on either side of its edge.

An expectation names the run it is stated for:
  noext    no_extended=True: what collect_reads_snv / collect_reads_sv classify directly (in an extended run a pair that no DNM rule took may
           still be chained in at a het site);
  default  the extended run, for the rules of group_reads_by_haplotype / connect_reads (:76-263);
  mapq20   min_map_qual=20 (extended: a record that fails goodread is refused at het sites too, so "none" holds);
  small    insert_size_max_sample=SMALL_SAMPLE: the head of the file (background pairs only) decides the cutoff, and the same number is the read
           goal of the fetch loop (:178-179).

htslib semantics relied on (what pysam gives the reference; tests/refshim/pysam.py follows them -- get_reference_positions :100-114 lists S and I
as None, walks M / = / X, advances over D and N, and ignores H and P; reference_end is pos + the M/D/N/=/X lengths):
  M = X   consume query and reference            I S   consume the query only (no reference position: None)
  D N     consume the reference only             H P   consume neither
"""
from synth.small import SmallDataset, otherbase, refbase
from unfazed_amd.model import (FDUP, FMREVERSE, FMUNMAP, FPAIRED, FPROPER, FQCFAIL, FREAD1, FREAD2, FREVERSE, FSECONDARY, FSUPP, FUNMAP,
                               OP_D, OP_EQ, OP_H, OP_I, OP_M, OP_N, OP_P, OP_S, OP_X, Segment, SiteRecord)

L = 151
KID, DAD, MOM = "kid1", "dad1", "mom1"
SAMPLES = [KID, DAD, MOM]
CONTIGS = ["1", "2"]  # every record lies on "1"; "2" exists for the mate-contig condition of goodread
SPACING = 30000
FIRST = 100000
TLEN = 400            # template length of an ordinary pair: |tlen - 2 L| is 98 on the forward record, 702 on the reverse one
CUTOFF = 702.0        # int(p99.5(|tlen - 302|)) (quirk Q8: read_collector.py:11-25) -- of the whole file and of its head alike, asserted below
SMALL_SAMPLE = 40     # insert_size_max_sample of the `small` run: the head is the first 41 records, the read goal 40
N_BACKGROUND = 300    # ordinary pairs in front of the first case: the head of the file, and enough records that the probes' few long inserts lie above p99.5
DEFAULT_SITES = (-400, -260, -120, 120, 260, 400)  # 140 apart: every 151-base record near the DNM covers one

RUNS = {
    "default": dict(),
    "noext": dict(no_extended=True),
    "mapq20": dict(min_map_qual=20),
    "small": dict(insert_size_max_sample=SMALL_SAMPLE),
}
SV_RUNS = {
    "default": dict(),
    "noext": dict(no_extended=True),
}
MARGIN = 5            # split_error_margin (the default)
SV_BACKGROUND = 1600  # enough ordinary records that the few discordant probes stay above the 99.5th percentile: the cutoff is 702 here too

_REF_OPS = (OP_M, OP_D, OP_N, OP_EQ, OP_X)
_OPS = {"M": OP_M, "I": OP_I, "D": OP_D, "N": OP_N, "S": OP_S, "H": OP_H, "P": OP_P, "=": OP_EQ, "X": OP_X}


def cig(text):
    """'5S146M' -> [(OP_S, 5), (OP_M, 146)]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((_OPS[ch], int(n)))
            n = ""
    assert n == ""
    return out


def ref_len(cigar):
    return sum(l for op, l in cigar if op in _REF_OPS)


def query_len(cigar):
    return sum(l for op, l in cigar if op in (OP_M, OP_I, OP_S, OP_EQ, OP_X))


def ref_positions(start, cigar):
    """get_reference_positions(full_length=True) by the semantics of the module docstring"""
    out, q = [], start
    for op, l in cigar:
        if op in (OP_M, OP_EQ, OP_X):
            out.extend(range(q, q + l))
            q += l
        elif op in (OP_I, OP_S):
            out.extend([None] * l)
        elif op in (OP_D, OP_N):
            q += l
    return out


class Rd:
    """One record of a pair as the case table writes it: start, CIGAR text, and what differs from an ordinary record."""

    def __init__(self, at, cigar="151M", low=None, flag_or=0, flag_clear=0, mapq=60, mtid=0, ins="T", has_sa=False):
        self.at, self.cigar = at, cig(cigar) if isinstance(cigar, str) else list(cigar)
        self.low = dict(low or {})  # query index -> quality (37 elsewhere)
        self.flag_or, self.flag_clear, self.mapq, self.mtid, self.ins, self.has_sa = flag_or, flag_clear, mapq, mtid, ins, has_sa

    @property
    def end(self):
        return self.at + ref_len(self.cigar)


class Case:
    def __init__(self, name, rule, pos, ref, alt, sites, vartype="POINT", end=None, group=None):
        self.name, self.rule, self.pos, self.ref, self.alt, self.vartype = name, rule, pos, ref, alt, vartype
        self.group = group or name  # cases that form one edge between them (each its own fetch) share a group
        self.end = pos + len(ref) if end is None else end
        self.sites = [pos + s for s in sites]
        self.pairs = []    # (qname, first Rd, second Rd)
        self.expect = []   # (run, qname, outcome)

    @property
    def key(self):
        return "1_%d_%d_%s_%s" % (self.pos, self.end, KID, self.vartype)


class Panel:
    def __init__(self, runs):
        self.runs = runs
        self.cases = []
        self.segs = []
        self._next = FIRST

    def case(self, name, rule, ref=None, alt=None, sites=DEFAULT_SITES, vartype="POINT", length=None, group=None):
        p = self._next
        self._next += SPACING
        if ref is None:  # an SNV
            ref = refbase(0, p)
            alt = otherbase(ref, 0)
        elif callable(ref):
            ref, alt = ref(p)
        c = Case(name, rule, p, ref, alt, sites, vartype, None if length is None else p + length, group)
        self.cases.append(c)
        return c

    def pair(self, c, probe, first, second=None, allele="alt", expect=None, run="noext", tlen=None):
        """One pair of case c.  `first` is the forward record (READ1, mate reverse), `second` the reverse one (READ2); by default `second` is
        151M placed so that the template is TLEN long.  allele: which bases the pair carries at an SNV / MNP DNM -- "alt", "ref", or a string
        written out.  expect: the outcome for `run` (or a dict run -> outcome)."""
        name = "%s.%s" % (c.name, probe)
        if second is None:
            second = Rd(first.at + TLEN - L)
        over = {s: _site_alt(s) for s in c.sites}
        if c.vartype == "POINT" and len(c.ref) == len(c.alt) and allele != "ref":
            bases = c.alt if allele == "alt" else allele
            assert len(bases) == len(c.alt)
            over.update({c.pos + k: b for k, b in enumerate(bases)})
        lo, hi = min(first.at, second.at), max(first.end, second.end)
        t = hi - lo if tlen is None else tlen  # (a tuple: the two records' own fields, +first / -second)
        t1, t2 = t if isinstance(t, tuple) else (t, t)
        recs = []
        for which, r, other in ((0, first, second), (1, second, first)):
            flag = FPAIRED | FPROPER | ((FREAD1 | FMREVERSE) if which == 0 else (FREAD2 | FREVERSE))
            flag = (flag | r.flag_or) & ~r.flag_clear
            seq = _bases(r.at, r.cigar, over, r.ins)
            qual = [37] * len(seq)
            for i, q in r.low.items():
                qual[i] = q
            recs.append(Segment(name, flag, 0, r.at, r.mapq, list(r.cigar), r.mtid, other.at, t1 if which == 0 else -t2, seq, qual, has_sa=r.has_sa))
        assert abs(lo - c.pos) < SPACING // 2 - 6000 and abs(hi - c.pos) < SPACING // 2 - 6000, name
        self.segs.extend(recs)
        c.pairs.append((name, first, second))
        if expect is not None:
            for rn, o in (expect.items() if isinstance(expect, dict) else [(run, expect)]):
                assert rn in self.runs and o in ("alt", "ref", "none")
                c.expect.append((rn, name, o))
        return name

    def finish(self, n_background=N_BACKGROUND, step=250):
        for i in range(n_background):  # the head of the file: ordinary pairs that touch nothing
            a = 1000 + step * i
            assert a + TLEN < FIRST - 10000
            for which, at in ((0, a), (1, a + TLEN - L)):
                flag = FPAIRED | FPROPER | ((FREAD1 | FMREVERSE) if which == 0 else (FREAD2 | FREVERSE))
                self.segs.append(Segment("bg.%04d" % i, flag, 0, at, 60, [(OP_M, L)], 0, a + TLEN - L if which == 0 else a,
                                         TLEN if which == 0 else -TLEN, _bases(at, [(OP_M, L)], {}, "T"), [37] * L))
        self.segs.sort(key=lambda s: (s.tid, s.pos))  # (stable: ties keep the order of the case table)
        sites = []
        for c in self.cases:
            own = SiteRecord("1", c.pos, c.ref, [c.alt], [1, 0, 0], [15, 30, 30], [15, 0, 0], [99.0] * 3)
            for s in sorted(c.sites + [c.pos]) if c.vartype == "POINT" else sorted(c.sites):
                if s == c.pos and c.vartype == "POINT":
                    sites.append(own)
                else:
                    sites.append(SiteRecord("1", s, refbase(0, s), [_site_alt(s)], [1, 3, 0], [15, 0, 30], [15, 30, 0], [99.0] * 3))
        assert all(a.start < b.start for a, b in zip(sites, sites[1:]))
        dnms = [{"chrom": "1", "start": c.pos, "end": c.end, "kid": KID, "vartype": c.vartype, "bam": "mem://%s.bam" % KID, "cram_ref": None}
                for c in self.cases]
        ped = {KID: {"kid": KID, "dad": DAD, "mom": MOM, "sex": "2"}}
        self.dataset = SmallDataset(list(SAMPLES), list(CONTIGS), sites, {KID: self.segs}, dnms, ped, {})
        self._check()
        return self

    def _check(self):
        from unfazed_amd.hostpath import concordant_cutoff
        import numpy as np
        names = set()
        sides = {}
        for c in self.cases:
            assert c.expect, c.name
            for rn, name, o in c.expect:
                sides.setdefault((c.group, rn), set()).add(o)
        for g in {c.group for c in self.cases if getattr(c, "two_sided", True)}:
            assert any(len(v) >= 2 for (gg, rn), v in sides.items() if gg == g), "case %s has no probe on either side of its edge" % g
        for c in self.cases:
            probes = {name for _, name, _ in c.expect}
            for name, first, second in c.pairs:
                assert name not in names, name
                names.add(name)
                if name in probes:  # visibility
                    seen = [s for r in (first, second) for s in c.sites if s in ref_positions(r.at, r.cigar)]
                    assert seen, "probe pair %s covers no site of its case" % name
        tl = np.array([s.tlen for s in self.segs], np.int32)
        assert concordant_cutoff(tl, L, 3) == CUTOFF, concordant_cutoff(tl, L, 3)
        head = self.segs[: SMALL_SAMPLE + 1]
        assert all(s.qname.startswith("bg.") for s in head)
        assert concordant_cutoff(tl[: SMALL_SAMPLE + 1], L, 3) == CUTOFF


def _site_alt(s):
    return otherbase(refbase(0, s), 0)


def _bases(start, cigar, over, ins):
    out, q, k = [], start, 0
    for op, l in cigar:
        if op in (OP_M, OP_EQ, OP_X):
            out.extend(over.get(p) or refbase(0, p) for p in range(q, q + l))
            q += l
        elif op == OP_I:
            out.extend(ins[(k + j) % len(ins)] for j in range(l))
            k += l
        elif op == OP_S:
            out.extend("GA"[j & 1] for j in range(l))
        elif op in (OP_D, OP_N):
            q += l
    return "".join(out)


def outcome(record, qname):
    """what a golden / oracle / device record says of a pair (record None: the DNM produced none)"""
    dad = record is not None and qname in record["dad_reads"]
    mom = record is not None and qname in record["mom_reads"]
    return "both" if dad and mom else "alt" if dad else "ref" if mom else "none"


# =====================================================================================================================================
# point variants
# =====================================================================================================================================
def _third(c, k=0):
    """a base that is neither REF nor ALT at offset k of the DNM"""
    return next(b for b in "ACGT" if b not in (c.ref[k], c.alt[k]))


def point_panel():
    pn = Panel(RUNS)
    P = pn.pair

    # ---- get_allele_at (:56-73) --------------------------------------------------------------------------------------------------
    c = pn.case("idx", "get_allele_at :63 read_pos < 4 or read_pos > READLEN - 4 (147)")
    P(c, "i3", Rd(c.pos - 3), expect="none")
    P(c, "i4", Rd(c.pos - 4), expect="alt")
    P(c, "i4ref", Rd(c.pos - 4), allele="ref", expect="ref")
    P(c, "i147", Rd(c.pos - 147), expect="alt")
    P(c, "i148", Rd(c.pos - 148), expect="none")
    P(c, "i75third", Rd(c.pos - 75), allele=_third(c), expect="none")  # neither allele: snv_match_alleles :311-336 takes nothing

    c = pn.case("idx_clip", "get_allele_at :62-63 the index counts a leading soft clip (clip + offset)")
    P(c, "s2o1", Rd(c.pos - 1, "2S149M"), expect="none")    # index 3
    P(c, "s2o2", Rd(c.pos - 2, "2S149M"), expect="alt")     # index 4
    P(c, "s2o145", Rd(c.pos - 145, "2S149M"), expect="alt")  # index 147
    P(c, "s2o146", Rd(c.pos - 146, "2S149M"), expect="none")  # index 148

    c = pn.case("short", "get_allele_at :65 len(query_sequence) > read_pos + var_len, a 100-base read; the mate is not consulted (quirk Q10)")
    P(c, "i98", Rd(c.pos - 98, "100M"), expect="alt")    # 100 > 98 + 1
    P(c, "i99", Rd(c.pos - 99, "100M"), expect="none")   # 100 > 99 + 1 fails: falls through to `return False`

    def mnp(p):
        ref = "".join(refbase(0, p + k) for k in range(3))
        return ref, "".join(otherbase(b, k) for k, b in enumerate(ref))
    c = pn.case("mnp", "get_allele_at :66 a 3-base MNP read across a 32-base unit boundary (i = 30: 30 31 | 32; i = 62: 62 63 | 64); "
                "snv_match_alleles :311-323", ref=mnp)
    for i in (30, 62):
        P(c, "i%dalt" % i, Rd(c.pos - i), expect="alt")
        P(c, "i%dref" % i, Rd(c.pos - i), allele="ref", expect="ref")
        # only the base in the NEXT unit (index 32 / 64) differs from ALT: neither allele
        P(c, "i%dlast" % i, Rd(c.pos - i), allele=c.alt[:2] + _third(c, 2), expect="none")
        P(c, "i%dfirst" % i, Rd(c.pos - i), allele=_third(c, 0) + c.alt[1:], expect="none")
    P(c, "short_i96", Rd(c.pos - 96, "100M"), expect="alt")   # 100 > 96 + 3
    P(c, "short_i97", Rd(c.pos - 97, "100M"), expect="none")  # 100 > 97 + 3 fails

    # ---- position in a gap ---------------------------------------------------------------------------------------------------------
    for op in "DN":
        c = pn.case("gap_" + op, "get_allele_at :61 `pos in read_ref_positions`: a position inside a %s operation has no query index" % op)
        P(c, "before", Rd(c.pos - 69, "70M5%s81M" % op), expect="alt")   # the last base before the gap (index 69)
        P(c, "in_first", Rd(c.pos - 70, "70M5%s81M" % op), expect="none")
        P(c, "in_last", Rd(c.pos - 74, "70M5%s81M" % op), expect="none")
        P(c, "after", Rd(c.pos - 75, "70M5%s81M" % op), expect="alt")     # the first base after it (index 70)

    for op, n in (("N", 200), ("D", 160)):
        c = pn.case("gapmate_" + op, "collect_reads_snv :411-418 + get_allele_at :67-72: the mate lies strictly inside a %d%s gap of the read, the overlap "
                    "test passes and the allele is read from the MATE (the j branch of uz_classify_dnm_read)" % (n, op))
        for probe, j, o in (("j10", 10, "alt"), ("j4", 4, "alt"), ("j3", 3, "none")):
            # read: 40M <gap> 111M from a; gap = [a + 40, a + 40 + n); mate 151M from a + 43 (ends at a + 194 < a + 200); DNM at mate index j
            a = c.pos - j - 43
            P(c, probe, Rd(a, "40M%d%s111M" % (n, op)), Rd(a + 43), expect=o)

    # ---- operations the generator never writes ---------------------------------------------------------------------------------------
    c = pn.case("hard", "H consumes neither query nor reference: the index rule of :63 is untouched by hard clips in front or behind")
    P(c, "front_i3", Rd(c.pos - 3, "5H151M"), expect="none")
    P(c, "front_i4", Rd(c.pos - 4, "5H151M"), expect="alt")
    P(c, "back_i147", Rd(c.pos - 147, "151M5H"), expect="alt")
    P(c, "back_i148", Rd(c.pos - 148, "151M5H"), expect="none")
    P(c, "both_i4ref", Rd(c.pos - 4, "3H151M4H"), allele="ref", expect="ref")

    c = pn.case("pad", "P consumes neither query nor reference: positions and indices behind it are unshifted")
    P(c, "i100", Rd(c.pos - 100, "75M2P76M"), expect="alt")
    P(c, "i147", Rd(c.pos - 147, "75M2P76M"), expect="alt")
    P(c, "i148", Rd(c.pos - 148, "75M2P76M"), expect="none")
    P(c, "i100ref", Rd(c.pos - 100, "75M2P76M"), allele="ref", expect="ref")

    c = pn.case("eqx", "= and X walk query and reference like M; X at the site carries ALT, = carries REF")
    P(c, "x_at", Rd(c.pos - 50, "50=1X100="), expect="alt")
    P(c, "eq_at", Rd(c.pos - 50, "151="), allele="ref", expect="ref")
    P(c, "x_i3", Rd(c.pos - 3, "3=1X147="), expect="none")

    c = pn.case("clip_both", "S at both ends: the index counts the leading clip, READLEN - 4 does not care about the trailing one")
    P(c, "o1", Rd(c.pos - 1, "2S147M2S"), expect="none")      # index 3
    P(c, "o2", Rd(c.pos - 2, "2S147M2S"), expect="alt")       # index 4
    P(c, "o145", Rd(c.pos - 145, "2S147M2S"), expect="alt")   # index 147
    P(c, "o146", Rd(c.pos - 146, "2S147M2S"), expect="none")  # index 148 (the last aligned base)

    # ---- goodread (:28-53) ---------------------------------------------------------------------------------------------------------
    c = pn.case("lowq", "goodread :43-52 low_quals > 10 with qual < MIN_BASE_QUAL (20)")
    ten, eleven = {20 + 3 * k: 19 for k in range(10)}, {20 + 3 * k: 19 for k in range(11)}
    P(c, "r10", Rd(c.pos - 75, low=ten), expect="alt")
    P(c, "r11", Rd(c.pos - 75, low=eleven), expect="none")
    P(c, "r11q20", Rd(c.pos - 75, low={i: 20 for i in eleven}), expect="alt")  # exactly at the threshold: not low
    P(c, "m10", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, low=ten), expect="alt")
    P(c, "m11", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, low=eleven), expect="none")
    P(c, "r_at_dnm_q0", Rd(c.pos - 75, low={75: 0}), expect="alt")  # no quality rule at an SNV DNM itself (quirk Q16)

    c = pn.case("ncigar", "goodread :47-52 counts every CIGAR operation (quirk Q9): > 10 refuses")
    ops10, ops11 = "10=1X10=1X10=1X10=1X10=97M", "10=1X10=1X10=1X10=1X10=1X96M"
    assert len(cig(ops10)) == 10 and len(cig(ops11)) == 11 and query_len(cig(ops10)) == query_len(cig(ops11)) == L
    P(c, "r10", Rd(c.pos - 120, ops10), expect="alt")
    P(c, "r11", Rd(c.pos - 120, ops11), expect="none")
    P(c, "m10", Rd(c.pos - 120), Rd(c.pos - 120 + TLEN - L, ops10), expect="alt")
    P(c, "m11", Rd(c.pos - 120), Rd(c.pos - 120 + TLEN - L, ops11), expect="none")

    c = pn.case("mapq", "goodread :35 int(mapping_quality) < MIN_MAPQ, at the default (1) and at 20")
    both = lambda d, m: {"noext": d, "mapq20": m}  # noqa: E731
    P(c, "r0", Rd(c.pos - 75, mapq=0), expect=both("none", "none"))
    P(c, "r1", Rd(c.pos - 75, mapq=1), expect=both("alt", "none"))
    P(c, "r19", Rd(c.pos - 75, mapq=19), expect=both("alt", "none"))
    P(c, "r20", Rd(c.pos - 75, mapq=20), expect=both("alt", "alt"))
    P(c, "m0", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, mapq=0), expect=both("none", "none"))
    P(c, "m1", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, mapq=1), expect=both("alt", "none"))
    P(c, "m19", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, mapq=19), expect=both("alt", "none"))
    P(c, "m20", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, mapq=20), expect=both("alt", "alt"))

    c = pn.case("flags", "goodread :31-41 the eight conditions, on the read and on the mate")
    P(c, "clean", Rd(c.pos - 75), expect="alt")
    conds = [("qcfail", dict(flag_or=FQCFAIL)), ("dup", dict(flag_or=FDUP)), ("mapq", dict(mapq=0)), ("secondary", dict(flag_or=FSECONDARY)),
             ("supp", dict(flag_or=FSUPP)), ("mate_unmapped", dict(flag_or=FMUNMAP)), ("mate_contig", dict(mtid=1))]
    for nm, kw in conds:
        P(c, "r_" + nm, Rd(c.pos - 75, **kw), expect="none")
        P(c, "m_" + nm, Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, **kw), expect="none")
    # an unmapped record ends at pos + 1 (bam_endpos): the fetch at the DNM returns it only from pos - 1 .. pos; the mate look-up finds it at its start
    P(c, "r_unmapped", Rd(c.pos, flag_or=FUNMAP), expect="none")
    P(c, "m_unmapped", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, flag_or=FUNMAP), expect="none")

    # ---- fetch filters ---------------------------------------------------------------------------------------------------------------
    c = pn.case("nopos", "collect_reads_snv :405-408 count(None) > 5 on the read or on the mate")
    P(c, "r5", Rd(c.pos - 70, "5S146M"), expect="alt")
    P(c, "r6", Rd(c.pos - 70, "6S145M"), expect="none")
    P(c, "r5mix", Rd(c.pos - 60, "3S70M2I76M"), expect="alt")
    P(c, "r6mix", Rd(c.pos - 60, "3S70M3I75M"), expect="none")
    P(c, "m5", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L, "146M5S"), expect="alt")
    P(c, "m6", Rd(c.pos - 75), Rd(c.pos - 75 + TLEN - L + 1, "145M6S"), expect="none")

    c = pn.case("overlap", "collect_reads_snv :409-418 the inclusive overlap test on [reference_start, reference_end]")
    P(c, "fwd_touch", Rd(c.pos - 100), Rd(c.pos - 100 + L), expect="none")        # mate start == read end
    P(c, "fwd_clear", Rd(c.pos - 100), Rd(c.pos - 100 + L + 1), expect="alt")     # read end + 1
    P(c, "rev_touch", Rd(c.pos - 50 - L), Rd(c.pos - 50), expect="none")          # the read is the reverse record: read start == mate end
    P(c, "rev_clear", Rd(c.pos - 50 - L - 1), Rd(c.pos - 50), expect="alt")
    # the other two equalities, with a 100-base mate inside the read's span.  One past them the read CONTAINS its mate: neither end of the read lies
    # in the mate, and the test lets the pair through (what the gapmate cases use)
    P(c, "end_eq", Rd(c.pos - 130), Rd(c.pos - 130 + 51, "100M"), expect="none")    # read end == mate end
    P(c, "end_in", Rd(c.pos - 130), Rd(c.pos - 130 + 51, "99M"), expect="alt")      # mate end == read end - 1
    P(c, "start_eq", Rd(c.pos - 130), Rd(c.pos - 130, "100M"), expect="none")       # read start == mate start
    P(c, "start_in", Rd(c.pos - 130), Rd(c.pos - 130 + 1, "100M"), expect="alt")    # mate start == read start + 1

    # ---- insert cutoff -------------------------------------------------------------------------------------------------------------------
    c = pn.case("insert", "collect_reads_snv :395-396 (double) insert_size > concordant_upper_len, cutoff %d from the head of the file" % CUTOFF)
    # (fwd_past stays "none" when extended: its forward record is refused at het sites by the same test and its reverse one covers no site)
    every = lambda o: {"noext": o, "small": o}  # noqa: E731
    P(c, "fwd_at", Rd(c.pos - 20), Rd(c.pos - 20 + 1004 - L), expect=every("alt"))    # |1004 - 302| == 702
    P(c, "fwd_past", Rd(c.pos - 20), Rd(c.pos - 20 + 1005 - L), expect=every("none"))  # 703
    P(c, "rev_at", Rd(c.pos - 130 - TLEN + L), Rd(c.pos - 130), expect="alt")   # the reverse record is fetched: |-400 - 302| == 702
    P(c, "rev_past", Rd(c.pos - 130 - TLEN + L - 1), Rd(c.pos - 130), expect="none")  # |-401 - 302| == 703
    by_name = {sg.qname: sg for sg in pn.segs if sg.pos <= c.pos < sg.pos + L}  # the fetched record of each probe
    assert [abs(by_name["insert." + k].tlen - 2 * L) for k in ("fwd_at", "fwd_past", "rev_at", "rev_past")] == [int(CUTOFF), int(CUTOFF) + 1] * 2

    # ---- indel DNMs (indel_match_alleles :266-293) ---------------------------------------------------------------------------------------
    def ins2(p):
        return refbase(0, p), refbase(0, p) + "TT"

    def del2(p):
        return "".join(refbase(0, p + k) for k in range(3)), refbase(0, p)

    for kind, mk in (("ins", ins2), ("del", del2)):
        op = "I" if kind == "ins" else "D"

        def carrier(c, rp, at_op, total=L):
            """a read with the DNM position at query index rp and a 2-base I / D starting at expanded-operation index at_op"""
            rest = total - at_op - (2 if op == "I" else 0)
            return Rd(c.pos - rp, "%dM2%s%dM" % (at_op, op, rest))

        c = pn.case(kind + "_rp", "indel_match_alleles :290 `7 < read_pos < len(read_ref_positions) - 7`; the length counts soft clips", ref=mk)
        P(c, "rp7", Rd(c.pos - 7), expect="none")
        P(c, "rp8", Rd(c.pos - 8), expect="ref")
        P(c, "rp143", Rd(c.pos - 143), expect="ref")
        P(c, "rp144", Rd(c.pos - 144), expect="none")
        P(c, "clip_rp7", Rd(c.pos - 3, "4S147M"), expect="none")
        P(c, "clip_rp8", Rd(c.pos - 4, "4S147M"), expect="ref")
        P(c, "clip_rp143", Rd(c.pos - 143, "147M4S"), expect="ref")    # 143 < 151 - 7: the four clipped bases count
        P(c, "clip_rp144", Rd(c.pos - 144, "147M4S"), expect="none")
        P(c, "alt_rp3", carrier(c, 3, 4), expect="alt")  # the I / D branch has no position rule

        c = pn.case(kind + "_qual", "indel_match_alleles :281-284 qualities of [rp, rp + var_len) (var_len 3) must reach MIN_BASE_QUAL", ref=mk)
        P(c, "ref_in", Rd(c.pos - 50, low={52: 19}), expect="none")     # rp + var_len - 1
        P(c, "ref_out", Rd(c.pos - 50, low={53: 19}), expect="ref")     # rp + var_len
        P(c, "ref_first", Rd(c.pos - 50, low={50: 19}), expect="none")
        P(c, "ref_before", Rd(c.pos - 50, low={49: 19}), expect="ref")
        P(c, "ref_q20", Rd(c.pos - 50, low={50: 20, 51: 20, 52: 20}), expect="ref")
        r = carrier(c, 50, 51)
        r.low = {52: 19}
        P(c, "alt_in", r, expect="none")
        r = carrier(c, 50, 51)
        r.low = {53: 19}
        P(c, "alt_out", r, expect="alt")

        c = pn.case(kind + "_ops", "indel_match_alleles :277-286 the expansion holds EVERY operation and is sliced by the query index (quirk Q16)", ref=mk)
        P(c, "at_anchor", carrier(c, 60, 61), expect="alt")    # the natural alignment: operations[61] is the first I / D
        P(c, "last", carrier(c, 60, 62), expect="alt")         # the operation starts at rp + var_len - 1
        P(c, "beyond", carrier(c, 60, 63), expect="ref")       # ... at rp + var_len: outside the slice
        # a 2D in front shifts the expansion two entries against the query: expansion = 20 M, 2 D, 50 M, 2 <op>, M ...; the <op> sits at entries 72-73
        shifted = "20M2D50M2%s%dM" % (op, L - 70 - (2 if op == "I" else 0))
        assert [o for o, l in cig(shifted) for _ in range(l)][72] == _OPS[op]
        P(c, "shift_first", _shifted(c, 72, shifted, op), expect="alt")   # slice [72, 75) starts on it
        P(c, "shift_inside", _shifted(c, 73, shifted, op), expect="alt")  # slice [73, 76): its second entry
        P(c, "shift_past", _shifted(c, 74, shifted, op), expect="ref")   # slice [74, 77): the operation ended at entry 73

    def del12(p):
        return "".join(refbase(0, p + k) for k in range(12)), refbase(0, p)
    c = pn.case("del_long", "indel_match_alleles :280-281 var_len 12 reaches past l_seq: the slices end with the read", ref=del12)
    P(c, "rp141", Rd(c.pos - 141), expect="ref")                  # [141, 153) cut at 151
    P(c, "rp143_q19_last", Rd(c.pos - 143, low={150: 19}), expect="none")
    P(c, "short_rp92", Rd(c.pos - 92, "100M"), expect="ref")      # 92 < 100 - 7
    P(c, "short_rp93", Rd(c.pos - 93, "100M"), expect="none")

    # ---- connect_reads (:76-152) and the het-site fetch loop (:165-222) ------------------------------------------------------------------
    # One het site H = DNM + 200.  The finder pair covers the DNM with its forward record (index 140, ALT) and H with its reverse one (index 91).  A probe
    # pair covers H but not the DNM; chained in, it joins the DNM's haplotype and shows through H itself.
    c = pn.case("connect", "group_reads_by_haplotype :181-214, connect_reads :113-124: the chained read's own index, quality and CIGAR at the het site",
                sites=(200,))
    H = c.pos + 200
    P(c, "finder", Rd(c.pos - 140))
    ex = dict(run="default")
    P(c, "i3", Rd(H - 3), expect="none", **ex)
    P(c, "i4", Rd(H - 4), expect="alt", **ex)
    P(c, "i147", Rd(H - 147), expect="alt", **ex)
    P(c, "i148", Rd(H - 148), expect="none", **ex)
    P(c, "q19", Rd(H - 60, low={60: 19}), expect="none", **ex)
    P(c, "q20", Rd(H - 60, low={60: 20}), expect="alt", **ex)
    five, six = "20M1X1D20M1X1D20M1X88M", "20M1X1D20M1X1D20M1X1D88M"  # non-M/= operations: 5 and 6 (:190-196), both within goodread's 10
    assert sum(1 for o, _ in cig(five) if o not in (OP_M, OP_EQ)) == 5 and sum(1 for o, _ in cig(six) if o not in (OP_M, OP_EQ)) == 6
    assert query_len(cig(five)) == query_len(cig(six)) == L and len(cig(six)) == 10
    P(c, "nonm5", Rd(H - 100, five), expect="alt", **ex)
    P(c, "nonm6", Rd(H - 100, six), expect="none", **ex)
    P(c, "nopos5", Rd(H - 60, "5S146M"), expect="alt", **ex)
    P(c, "nopos6", Rd(H - 60, "6S145M"), expect="none", **ex)
    # H inside a 160D of the read while the mate, strictly inside the gap, covers it: the allele is the mate's, but :120-121 wants the READ to hold the site
    P(c, "gap_mate", Rd(H - 60, "40M160D111M"), Rd(H - 60 + 43), expect="none", **ex)
    P(c, "plain", Rd(H - 30), expect="alt", **ex)  # (control: an ordinary chained pair)
    # the fetch loop's own filters on the chained pair (:181-214): the mate's goodread and its bases without a position, the inclusive overlap test,
    # the insert at the cutoff
    P(c, "m_nopos5", Rd(H - 60), Rd(H - 60 + TLEN - L, "146M5S"), expect="alt", **ex)
    P(c, "m_nopos6", Rd(H - 60), Rd(H - 60 + TLEN - L + 1, "145M6S"), expect="none", **ex)
    P(c, "m_lowq10", Rd(H - 60), Rd(H - 60 + TLEN - L, low={20 + 3 * k: 19 for k in range(10)}), expect="alt", **ex)
    P(c, "m_lowq11", Rd(H - 60), Rd(H - 60 + TLEN - L, low={20 + 3 * k: 19 for k in range(11)}), expect="none", **ex)
    P(c, "touch", Rd(H - 60), Rd(H - 60 + L), expect="none", **ex)
    P(c, "clear", Rd(H - 60), Rd(H - 60 + L + 1), expect="alt", **ex)
    P(c, "insert_at", Rd(H - 60), Rd(H - 60 + int(CUTOFF) + L), expect="alt", **ex)        # tlen 1004
    P(c, "insert_past", Rd(H - 60), Rd(H - 60 + int(CUTOFF) + L + 1), expect="none", **ex)  # tlen 1005

    # ---- read goal (:178-179) -----------------------------------------------------------------------------------------------------------------
    for total in (SMALL_SAMPLE + 1, SMALL_SAMPLE + 2):
        c = pn.case("goal%d" % total, "group_reads_by_haplotype :178-179 `i > EXTENDED_RB_READ_GOAL`: the fetch at H returns %d records, goal %d"
                    % (total, SMALL_SAMPLE), sites=(200,), group="goal")
        H = c.pos + 200
        P(c, "finder", Rd(c.pos - 140))  # its reverse record [pos + 109, pos + 260) is the FIRST record of the fetch at H
        for k in range(total - 2):
            P(c, "fill%02d" % k, Rd(c.pos + 110 + k))
        last = Rd(c.pos + 110 + total)   # the last record of the fetch: index total - 1
        P(c, "last", last, expect={"small": "alt" if total - 1 <= SMALL_SAMPLE else "none", "default": "alt"})
    # (goal41's last record has i == 40: `40 > 40` fails, taken; goal42's has i == 41: skipped.  Each is its own fetch; the two together are the edge.)

    # ---- arena build's index width (phase_body.hpp `if (LDS && nh > 127)`) -------------------------------------------------------------------------
    for nh in (127, 128):
        lo = -(nh // 2)
        js = [j for j in range(lo, lo + nh + 1) if j != 0]
        assert len(js) == nh
        c = pn.case("ladder%d" % nh, "k_phase arena build: %d het sites, 70 apart, one pair per site chaining to the next (connect_reads recursion :143-150)"
                    % nh, sites=tuple(70 * j for j in js))
        c.n_het = nh
        P(c, "root", Rd(c.pos - 75))  # DNM at index 75, sites -1 / +1 at 5 / 145
        for j in js:
            # A rung is the REVERSE record of its pair: a pair's "primary" record is the one registered last (quirk Q11), that is at the highest site
            # either record covers, and connect_reads :120-121 wants the primary record itself to hold the connecting site.
            if j > 0 and j + 1 in js:      # rung j: sites j, j + 1 at indices 40, 110 (the forward records of rungs 3 and 4 cover the DNM and are seeds too)
                P(c, "up%03d" % j, Rd(c.pos + 70 * j - 40 - TLEN + L), Rd(c.pos + 70 * j - 40), expect="alt" if j + 1 == js[-1] else None, run="default")
            if j < 0 and j - 1 in js:      # rung j downwards: sites j - 1, j at indices 40, 110
                P(c, "dn%03d" % -j, Rd(c.pos + 70 * (j - 1) - 40 - TLEN + L), Rd(c.pos + 70 * (j - 1) - 40),
                  expect="alt" if j - 1 == js[0] else None, run="default")
        c.two_sided = False  # (the edge is the kernel's own, 127 / 128 sites: both sides give the same records by another build)
    return pn.finish()


def _shifted(c, rp, cigar, op):
    """a read with `cigar` (20M2D in front) whose query index rp holds the DNM position"""
    pos_of = ref_positions(0, cig(cigar))
    assert pos_of[rp] is not None
    return Rd(c.pos - pos_of[rp], cigar)


# =====================================================================================================================================
# SV breakpoints (collect_reads_sv :435-602)
# =====================================================================================================================================
def sv_panel():
    """Every supporting read of an SV goes to "alt" (:596): a pair is "alt" (taken) or "none".  Each case has an anchor, a split read right on the
    start breakpoint, so that the two supporting records of :594 are there whatever its probes decide.  Events are INV-typed (no allele-balance
    record is merged in) except where said."""
    pn = Panel(SV_RUNS)
    P = pn.pair

    def sv(name, rule, length, vartype="INV"):
        c = pn.case(name, rule, ref="N", alt="<%s>" % vartype, sites=tuple(range(-840, length + 841, 140)), vartype=vartype, length=length)
        P(c, "anchor", Rd(c.pos, "60S91M", has_sa=True), expect="alt")
        # one ordinary pair over every site: the reference's connect_reads (:106) looks a seed's sites up in a table that holds only sites where the
        # fetch loop registered somebody, and ends with a KeyError otherwise -- an extended run needs every site of a supporting read covered
        for k, st in enumerate(c.sites):
            P(c, "tile%02d" % k, Rd(st - 75))
        return c

    c = sv("ban", ":515-522 fewer than 7 M/= among the first ten AND the last ten expanded operations bans the read name", 1300)
    s = c.pos
    P(c, "s6e6", Rd(s + 2, "4S143M4S", has_sa=True), expect="none")
    P(c, "s7e6", Rd(s + 2, "3S144M4S", has_sa=True), expect="alt")
    P(c, "s6e7", Rd(s + 2, "4S144M3S", has_sa=True), expect="alt")
    P(c, "s6e6_ins", Rd(s + 2, "6M4I131M4I6M", has_sa=True), expect="none")  # I counts against M/= like a clip
    P(c, "s7e6_eq", Rd(s + 2, "7=3X131M4I6M", has_sa=True), expect="alt")     # = counts as a match, X does not

    c = sv("split", ":524-533 a split read (SA tag) whose start or end lies within +-split_error_margin (%d) of the breakpoint, inclusive" % MARGIN, 1300)
    s, e = c.pos, c.end
    for tag, bp in (("s", s), ("e", e)):
        P(c, tag + "_start_p5", Rd(bp + MARGIN, "60S91M", has_sa=True), expect="alt")
        P(c, tag + "_start_p6", Rd(bp + MARGIN + 1, "60S91M", has_sa=True), expect="none")
        P(c, tag + "_start_m5", Rd(bp - MARGIN, "60S91M", has_sa=True), expect="alt")
        P(c, tag + "_start_m6", Rd(bp - MARGIN - 1, "60S91M", has_sa=True), expect="none")
        P(c, tag + "_end_p5", Rd(bp + MARGIN - 91, "91M60S", has_sa=True), expect="alt")      # reference_end == bp + 5
        P(c, tag + "_end_p6", Rd(bp + MARGIN + 1 - 91, "91M60S", has_sa=True), expect="none")
        P(c, tag + "_end_m5", Rd(bp - MARGIN - 91, "91M60S", has_sa=True), expect="alt")
        P(c, tag + "_end_m6", Rd(bp - MARGIN - 1 - 91, "91M60S", has_sa=True), expect="none")
    P(c, "no_sa", Rd(s + 40, "151M"), expect="none")  # the same place without the tag: an ordinary record

    # A discordant pair: the FETCHED record's own |tlen - 302| is the insert.  The reverse records carry -400 (insert 702: not above the cutoff, and
    # unclipped: the last branch takes nothing), so that the forward record alone decides -- the two fields of a pair are written independently here.
    c = sv("ratio", ":534-536 0.7 < var_len / insert < 1.3 with var_len 1300: 1300 / 1000 is 1.3 to the last bit (IEEE division is correctly rounded, "
           "and the literal is the nearest double too), 1300 / 1857 = 0.70005 and 1300 / 1858 = 0.69968 are far from 0.7", 1300)
    s, e = c.pos, c.end
    for probe, ins, o in (("hi_eq", 1000, "none"), ("hi_in", 1001, "alt"), ("lo_in", 1857, "alt"), ("lo_out", 1858, "none")):
        P(c, probe, Rd(s - 100), Rd(e - 50), tlen=(ins + 2 * L, TLEN), expect=o)

    # (as INV, and as DEL and DUP: there phase_svs merges the read-backed record with the allele-balance pass over the same event)
    for vt in ("INV", "DEL", "DUP"):
        c = sv("cutoff_" + vt, ":534 insert_size > concordant_upper_len (%d), var_len 800 so that the ratio passes either way" % CUTOFF, 800, vt)
        s, e = c.pos, c.end
        P(c, "at", Rd(s - 100), Rd(e - 50), tlen=(int(CUTOFF) + 2 * L, TLEN), expect="none")       # 702: falls to the clipped-read branch, which takes nothing
        P(c, "past", Rd(s - 100), Rd(e - 50), tlen=(int(CUTOFF) + 1 + 2 * L, TLEN), expect="alt")  # 703; 800 / 703 = 1.138

    W = int(CUTOFF)
    c = sv("window", ":551-560 left start within (start - %d, start + %d) and right start within (end - %d, end + %d), all four bounds strict" % (W, W, W, W), 1300)
    s, e = c.pos, c.end
    disc = dict(tlen=(1500, TLEN))  # insert 1198, ratio 1.085
    P(c, "left_lo_at", Rd(s - W), Rd(e), expect="none", **disc)
    P(c, "left_lo_in", Rd(s - W + 1), Rd(e), expect="alt", **disc)
    P(c, "left_hi_in", Rd(s + W - 1), Rd(e + 300), expect="alt", **disc)
    P(c, "left_hi_at", Rd(s + W), Rd(e + 300), expect="none", **disc)  # (in reach of the fetch around the END breakpoint only)
    P(c, "right_lo_at", Rd(s - 300), Rd(e - W), expect="none", **disc)
    P(c, "right_lo_in", Rd(s - 300), Rd(e - W + 1), expect="alt", **disc)
    P(c, "right_hi_in", Rd(s), Rd(e + W - 1), expect="alt", **disc)
    P(c, "right_hi_at", Rd(s), Rd(e + W), expect="none", **disc)

    c = sv("clip", ":564-586 a clipped read without SA: region_pos < 2 or > len - 4 refused; everything before index region_pos - 1, or after region_pos, "
           "must be clipped; the breakpoint is looked for at position, position - 1, position + 1 in that order", 1300)
    s = c.pos
    P(c, "rp1", Rd(s, "1S150M"), expect="none")              # position at index 1
    P(c, "rp2", Rd(s, "2S149M"), expect="alt")               # index 2, lead 2
    P(c, "rp2_lead1", Rd(s - 1, "1S150M"), expect="alt")     # index 2, lead == rp - 1: [:1] is the clip alone
    P(c, "rp3_lead1", Rd(s - 2, "1S150M"), expect="none")    # index 3, lead == rp - 2: [:2] holds an aligned base
    P(c, "rp40_lead39", Rd(s - 1, "39S112M"), expect="alt")
    P(c, "rp40_lead38", Rd(s - 2, "38S113M"), expect="none")
    P(c, "rp147", Rd(s - 147, "148M3S"), expect="alt")       # len - 4: the last aligned base, three clipped behind it
    P(c, "rp148", Rd(s - 148, "149M2S"), expect="none")      # len - 3
    P(c, "tail_one_more", Rd(s - 99, "101M50S"), expect="none")  # index 99, an aligned base at 100 behind it
    P(c, "via_minus1", Rd(s - 100, "100M51S"), expect="alt")  # the last aligned base is position - 1
    P(c, "via_minus2", Rd(s - 101, "100M51S"), expect="none")
    P(c, "via_plus1", Rd(s + 1, "51S100M"), expect="alt")     # the first aligned base is position + 1
    P(c, "via_plus2", Rd(s + 2, "51S100M"), expect="none")
    return pn.finish(n_background=SV_BACKGROUND, step=50)
