"""Hand-built tables for the link forms of a site window (uz_types.h: uz_sites_view.pos_d16 ..., uz_family_view.ref_depth8 ..., het9 ...),
shared by tests/test_site_form_model.py (the model of tests/siteformmodel.py against the packer and the host twin, no GPU) and
tests/test_site_forms_gpu.py (the device's expansion against the model and, on the world tables, the C oracle).

Two kinds of table.  FORM tables take any int32 position and are only read back.  WORLD tables ascend within each contig
(sitecases.Table with the genotype columns of hetcases.table) and also run through classify and find.  Every view comes out of
io_native.pack_sites, except the hand-edited ones (`hand`): views the header allows and the packer never writes, laid out here in a
256-byte aligned block.  Pure numpy."""
import numpy as np

import hetcases
import sitecases
from siteformmodel import D16_LIMIT, SPAN
from unfazed_amd import abi, io_native

CODES = np.frombuffer(b"\0ACGTN", np.uint8)
JUMP = 40000  # a difference that escapes
SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, 3 * 1024 + 1)
# one escape per span at these local indices: both sides of every lane-63 / wave hand-over (255 | 256, 511 | 512, 767 | 768), the first and last lanes
ONE_ESCAPE_AT = (1, 2, 3, 4, 5, 7, 252, 253, 254, 255, 256, 257, 258, 259, 260, 511, 512, 513, 767, 768, 769, 1020, 1021, 1022, 1023)
GT_EDGE = (0x00, 0x3F, 0x40, 0x80, 0xFF)  # incoming genotype bytes: bit 6 is the library's, bit 7 is dropped
GTS = np.array(GT_EDGE + (0x15, 0x01, 0x11, 0x05), np.uint8)  # ... and four with a het kid (the het form ranks them)
BYTES = np.array((0, 1, 253, 254, 255, 17, 40), np.uint8)  # what an eight-bit column holds at its edges, and two ordinary values
N_CASES = 52  # pinned by tests/test_site_form_model.py: a case that drops out does not do so unseen


def _arr(ptr, dtype, k):
    if not k or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * k).from_address(ptr)).copy()


def parts_of(v):
    """the columns of a compact SitesView as numpy copies"""
    n, e = int(v.n_sites), int(v.n_pos_esc)
    ns = (n + SPAN - 1) // SPAN
    return dict(n=n, contig_off=_arr(v.contig_off, np.int64, int(v.n_contigs) + 1), d16=_arr(v.pos_d16, np.uint16, n), b8=_arr(v.bases8, np.uint8, n),
                span=_arr(v.span_pos, np.int32, ns), eidx=_arr(v.pos_esc_idx, np.int32, e), eval=_arr(v.pos_esc_val, np.int32, e),
                eoff=_arr(v.pos_esc_off, np.int32, ns + 1))


def hand_view(n, contig_off, d16, b8, span, eidx, eval, eoff, null_esc=False, null_span=False, n_pos_esc=None):  # noqa: A002
    """a compact SitesView laid out by hand: the six columns 256-byte aligned in one block, as uz_sites_pack lays them out"""
    cols = [np.ascontiguousarray(d16, np.uint16), np.ascontiguousarray(b8, np.uint8), np.ascontiguousarray(span, np.int32),
            np.ascontiguousarray(eidx, np.int32), np.ascontiguousarray(eval, np.int32), np.ascontiguousarray(eoff, np.int32)]
    at, end = [], 0
    for c in cols:
        at.append(end)
        end = (end + c.nbytes + 255) & ~255
    raw = np.zeros(max(end, 256) + 256, np.uint8)
    k = (-raw.ctypes.data) % 256
    block = raw[k: k + max(end, 256)]
    for c, a in zip(cols, at):
        block[a: a + c.nbytes] = c.view(np.uint8).reshape(-1)
    coff = np.ascontiguousarray(contig_off, np.int64)
    v = abi.SitesView()
    v.n_sites, v.n_contigs, v.contig_off = n, coff.size - 1, coff.ctypes.data
    base = block.ctypes.data
    v.pos_d16, v.bases8, v.span_pos = base + at[0], base + at[1], (0 if null_span else base + at[2])
    v.n_pos_esc = len(cols[3]) if n_pos_esc is None else n_pos_esc
    v.pos_esc_idx, v.pos_esc_val = (0, 0) if null_esc else (base + at[3], base + at[4])
    v.pos_esc_off = base + at[5]
    return abi.Held(v, dict(block=block, raw=raw, contig_off=coff))


def default_bases(n):
    """-> (sflags, ref_base, alt_base): the 36 pairs of codes 0 .. 5 times complex 0 / 1 in turn, the turn moved on by one every 72 sites --
    in 288 sites every residue mod 4 has met each of the 72"""
    i = np.arange(n)
    combo = (i + i // 72) % 72
    pair = combo % 36
    return (combo // 36).astype(np.uint8), CODES[pair % 6], CODES[pair // 6]


def form_family(n, roll=0):
    """-> (gt, [rd8 x 3], [ad8 x 3], [gq8 x 3], wide): column q of site i holds BYTES[(i + 3 q + roll) % 7], gt GTS[(i + roll) % 9] -- both
    periods are coprime with 4, so every column meets every byte at every residue within 28 sites.  255 in a depth column stands only at
    wide-listed sites: every site with one is listed, with depths of a few hundred."""
    i = np.arange(n)
    gt = GTS[(i + roll) % GTS.size]
    c8 = np.stack([BYTES[(i + 3 * q + roll) % BYTES.size] for q in range(9)])
    ws = np.nonzero((c8[:6] == 255).any(axis=0))[0].astype(np.int64)
    wide = None
    if ws.size:
        wr = np.stack([300 + (ws + m) % 50 for m in range(3)]).astype(np.int32)
        wa = np.stack([280 + (ws + 2 * m) % 70 for m in range(3)]).astype(np.int32)
        wide = (ws, wr, wa)
    return gt, list(c8[0:3]), list(c8[3:6]), list(c8[6:9]), wide


class Case:
    """name; held (the compact view), parts (its columns); want = the source's (pos, sflags, ref_base, alt_base) or, where a hand-edited
    view has no source, None; c8 = the trio's columns in the eight-bit link form; table = the sitecases.Table of a world table"""

    def __init__(self, name, held, want, c8, table=None, hand=False, reach=None):
        self.name, self.held, self.want, self.c8, self.table, self.hand = name, held, want, c8, table, hand
        self.parts = parts_of(held.view)
        self.n = self.parts["n"]
        self.reach = reach or {}
        self._model = None

    def model(self):
        if self._model is None:
            import siteformmodel
            p = self.parts
            self._model = siteformmodel.site_columns(p["d16"], p["b8"], p["span"], p["eidx"], p["eval"], p["eoff"], p["n"])
        return self._model

    def cols8(self):
        return np.stack(list(self.c8[1]) + list(self.c8[2]) + list(self.c8[3])).reshape(9, self.n)

    def ascends(self):
        """whether find may run on it: the positions ascend within every contig"""
        pos, off = self.model()[0].astype(np.int64), self.parts["contig_off"]
        return all(np.all(np.diff(pos[a:b]) >= 0) for a, b in zip(off[:-1], off[1:]))

    def __repr__(self):
        return self.name


def packed(name, pos, contig_off=None, bases=None, roll=0, c8=None, table=None, reach=None):
    pos = np.asarray(pos, np.int64)
    assert pos.min(initial=0) >= -(1 << 31) and pos.max(initial=0) < (1 << 31)
    n = pos.size
    sf, rb, ab = bases if bases is not None else default_bases(n)
    cols = dict(pos=np.ascontiguousarray(pos, np.int32), contig_off=np.ascontiguousarray([0, n] if contig_off is None else contig_off, np.int64),
                sflags=np.ascontiguousarray(sf, np.uint8), ref_base=np.ascontiguousarray(rb, np.uint8), alt_base=np.ascontiguousarray(ab, np.uint8))
    v = abi.SitesView()
    v.n_sites, v.n_contigs = n, cols["contig_off"].size - 1
    for k, a in cols.items():
        setattr(v, k, a.ctypes.data)
    cv, block, _ = io_native.pack_sites(v)
    held = abi.Held(cv, dict(block=block, cols=cols, plain=v))
    want = (cols["pos"], cols["sflags"], cols["ref_base"], cols["alt_base"])
    return Case(name, held, want, c8 if c8 is not None else form_family(n, roll), table=table, reach=reach)


def edited(name, src, want, reach=None, **edit):
    """a hand-edited view: the columns of a packer-built case with `edit` laid over them"""
    p = dict(src.parts)
    flags = {k: edit.pop(k) for k in ("null_esc",) if k in edit}
    p.update(edit)
    return Case(name, hand_view(**p, **flags), want, src.c8, hand=True, reach=reach)


def walk(n, start=1000, step=7):
    """ascending positions with differences 1 .. step + 3 that fit (and a repeated position now and then: difference 0)"""
    i = np.arange(n, dtype=np.int64)
    return start + np.cumsum((i * step + i // 5) % (step + 4))


def with_jumps(pos, at, jump=JUMP):
    """the same walk with `jump` added from each index of `at` on: that site's difference escapes"""
    pos = np.asarray(pos, np.int64).copy()
    for a in at:
        pos[a:] += jump
    return pos


def span_pattern(name, locals_, n=2 * SPAN + 3, span=1, **kw):
    """escapes at the local indices `locals_` of span `span` and nowhere else"""
    at = [span * SPAN + l for l in locals_]
    return packed(name, with_jumps(walk(n), at), reach=dict(esc=sorted(at)), **kw)


# ------------------------------------------------------------------------------------------------------------------------- world tables
def world(name, n, seed, contig_starts, jumps, **het_kw):
    """n sites in the contigs that start at `contig_starts` (site indices; 0 first), about ten bases apart, with jumps of 32768 and more in
    front of the sites `jumps`; the trio of hetcases.table; bases mixed, none at the complex sites"""
    t0 = hetcases.table(n, seed=seed, **het_kw)
    rng = np.random.default_rng(9000 + seed)
    gaps = rng.integers(1, 20, n).astype(np.int64)
    gaps[rng.random(n) < 0.02] = 0  # repeated positions
    for j in list(jumps) + list(contig_starts[1:]):
        gaps[j + 1: j + 2] = np.maximum(gaps[j + 1: j + 2], 1)  # (the site behind an escape: a difference to get wrong)
    for k, j in enumerate(jumps):
        gaps[j] = (D16_LIMIT, JUMP, 3 * JUMP)[k % 3]
    bounds = list(contig_starts) + [n]
    contigs = [500 * (c + 1) + np.cumsum(gaps[a:b]) for c, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
    gt, rd, ad, gq = (x.copy() for x in t0.true)
    cx = t0.complex.copy()
    # an escape site and the site behind it are candidates (kid het, dad hom-ref, mom hom-alt, good depths): a position that is off by one
    # there shows in the lists of the DNM that stands on it -- but a span that is to hold no het site keeps none
    for j in sorted(set(jumps) | set(contig_starts[1:])):
        for i in (j, j + 1):
            if i < n and i // SPAN != het_kw.get("no_het_span"):
                gt[:, i], rd[:, i], ad[:, i], gq[:, i], cx[i] = (1, 0, 3), (20, 30, 1), (20, 1, 30), 99, False
    t = sitecases.Table(name, gt, rd, ad, gq, complex_=cx, contigs=contigs)
    i = np.arange(n)
    acgtn = np.frombuffer(b"ACGTN", np.uint8)
    t.ref_base = np.where(t.complex, 0, acgtn[(i * 7 + seed) % 5]).astype(np.uint8)
    t.alt_base = np.where(t.complex, 0, acgtn[(i * 3 + seed + 1 + (i // 5) % 3) % 4]).astype(np.uint8)
    esc = sorted(j for j in set(jumps) | set(contig_starts[1:]) if j % SPAN)
    return packed(name, t.pos, t.contig_off, bases=(t.sflags, t.ref_base, t.alt_base), c8=hetcases.columns8(t), table=t, reach=dict(esc=esc))


def dnms_of(case):
    """point DNMs as tests/test_family_het_form_gpu.py builds them -- the table's start, middle and end, both sides of every span boundary --
    plus one at each escape site, at each of its two neighbours, and at each contig's first and last site (any case whose positions ascend)"""
    pos, off, n = case.model()[0], case.parts["contig_off"], case.n
    at = {0, n - 1, n // 2} | {s for b in range(SPAN, n, SPAN) for s in (b - 1, b)}
    for e in case.parts["eidx"]:
        at |= {int(e) - 1, int(e), int(e) + 1}
    for a, b in zip(off[:-1], off[1:]):
        if b > a:
            at |= {int(a), int(b) - 1}
    at = np.array(sorted(s for s in at if 0 <= s < n), np.int64)
    contig = (np.searchsorted(off, at, side="right") - 1).astype(np.int32)
    st = pos[at].astype(np.int32)
    return dict(contig=contig, start=st, end=st + 1, vartype=np.zeros(at.size, np.uint8), mult=np.ones(at.size, np.uint8), tags=["s%d" % i for i in at], at=at)


# -------------------------------------------------------------------------------------------------------------------------------- cases
_CACHE = {}


def cases():
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = []
    # sizes, no escapes: every residue of n mod 4 in the scalar tail, a last span of one site, a last span one short of full
    for n in SIZES:
        out.append(packed("size_%d" % n, walk(n), roll=n % 7, reach=dict(esc=[])))
    # one escape per span, on both sides of every hand-over between lanes and waves
    at = [s * SPAN + l for s, l in enumerate(ONE_ESCAPE_AT)]
    n = len(ONE_ESCAPE_AT) * SPAN
    out.append(packed("one_escape_per_span", with_jumps(walk(n), at), reach=dict(esc=at)))
    out.append(packed("one_escape_per_span_partial", with_jumps(walk(n + 5), at + [n + 4]), reach=dict(esc=at + [n + 4])))
    # dense escapes
    out.append(span_pattern("dense_whole_span", range(1, SPAN)))
    out.append(span_pattern("dense_one_lane", range(4 * 37, 4 * 38)))
    out.append(span_pattern("dense_lane_k1_k3", (4 * 130 + 1, 4 * 130 + 3)))
    out.append(span_pattern("dense_last_of_every_lane", range(3, SPAN, 4)))
    out.append(span_pattern("dense_first_of_every_lane", range(4, SPAN, 4)))
    out.append(span_pattern("dense_wave_1", range(256, 512)))
    at = [5, 700, 2 * SPAN + 1, 2 * SPAN + 1023]
    out.append(packed("span_without_escapes_between", with_jumps(walk(3 * SPAN), at), reach=dict(esc=at)))
    # values
    out.append(packed("differences_0_1_32767_32768", [100, 100, 101, 101 + D16_LIMIT - 1, 101 + D16_LIMIT - 1, 100 + 2 * D16_LIMIT, 101 + 2 * D16_LIMIT, 7],
                      reach=dict(esc=[5, 7])))
    out.append(packed("negative_zero_minus5_int32_max", [0, 0, 5, -5, -2, (1 << 31) - 1, 7, 7 + D16_LIMIT - 1, -(1 << 31), -(1 << 31) + 9],
                      reach=dict(esc=[3, 5, 6, 8])))
    top = (1 << 31) - 1
    ramp = top - (D16_LIMIT - 1) * np.arange(SPAN - 1, -1, -1, dtype=np.int64)
    out.append(packed("span_of_32767_up_to_int32_max", np.concatenate([walk(SPAN), ramp, walk(3)]), reach=dict(esc=[])))
    out.append(packed("span_from_negative_across_zero", np.concatenate([walk(SPAN, start=-3000, step=5), walk(SPAN + 2, start=-4000, step=9)]), reach=dict(esc=[])))
    out.append(packed("escape_below_its_predecessor", [50000, 50003, 40, 45, 45, 20000, 3, 4], reach=dict(esc=[2, 6])))
    # contigs
    n = 3 * SPAN + 5
    pos = walk(n, step=3)  # (every difference fits: a contig's start escapes because it is one)
    out.append(packed("contig_starts_l0_l1_l1023", pos, [0, SPAN, SPAN + 1, 2 * SPAN + 1023, n], reach=dict(esc=[SPAN + 1, 2 * SPAN + 1023])))
    out.append(packed("empty_contigs", walk(SPAN + 9), [0, 0, 0, 300, 300, SPAN + 2, SPAN + 9, SPAN + 9], reach=dict(esc=[300, SPAN + 2])))
    out.append(packed("contigs_300_of_one_site", walk(300, step=3), list(range(301)), reach=dict(esc=list(range(1, 300)))))
    # bases: all 36 pairs times complex 0 / 1 at every residue in full lanes; the scalar tail meets A C G T N and none
    for name, tail in (("bases_tail_ACGTN0", (b"AGN", b"CT\0")), ("bases_tail_CTN0AG", (b"C\0T", b"ANG"))):
        sf, rb, ab = default_bases(291)
        rb[288:], ab[288:] = np.frombuffer(tail[0], np.uint8), np.frombuffer(tail[1], np.uint8)
        out.append(packed(name, walk(291), bases=(sf, rb, ab), reach=dict(esc=[])))
    # family columns: every column at every residue and -- three rolls of a three-site table -- in the scalar tail
    for r in (0, 3, 6):
        out.append(packed("family_tail_roll%d" % r, walk(3), roll=r, reach=dict(esc=[])))
    for n in (29, 290):
        out.append(packed("family_n%d" % n, walk(n), roll=1, reach=dict(esc=[])))
    # world tables: escapes at the wave edges, contig starts inside a span, jumps of 32768 and more
    out.append(world("world_a", 3 * SPAN + 5, 11, [0, SPAN + 500], [255, 256, 257, SPAN + 1, 2 * SPAN - 1, 2 * SPAN + 511, 2 * SPAN + 512]))
    out.append(world("world_b", 5 * SPAN + 300, 12, [0, SPAN + 512, SPAN + 513, 3 * SPAN + 1023], [767, 768, 769, 2 * SPAN + 1020, 4 * SPAN + 3, 5 * SPAN + 299],
                     all_het_span=2))
    out.append(world("world_c", 2 * SPAN, 13, [0, 700, SPAN], [1, 511, 513, SPAN + 255, SPAN + 1023], no_het_span=0))
    by = {c.name: c for c in out}
    # hand-edited views: what the header leaves open
    src = by["bases_tail_ACGTN0"]
    b8 = src.parts["b8"].copy()
    rb, ab = src.want[2].copy(), src.want[3].copy()
    i = np.arange(src.n)
    six, seven, eight = i % 5 == 1, i % 7 == 2, i % 3 != 0
    b8[six] = (b8[six] & 0xF8) | 6
    rb[six] = ord("N")
    b8[seven] = (b8[seven] & 0xC7) | (7 << 3)
    ab[seven] = ord("N")
    b8[i % 9 == 3] = (b8[i % 9 == 3] & 0xC7) | (6 << 3)
    ab[i % 9 == 3] = ord("N")
    b8[i % 13 == 5] |= 7
    rb[i % 13 == 5] = ord("N")
    b8[i % 11 == 4] |= 0x3F  # both codes 7
    rb[i % 11 == 4] = ab[i % 11 == 4] = ord("N")
    b8[eight] |= 0x80  # bit 7: ignored
    out.append(edited("hand_codes_6_7_bit_7", src, (src.want[0], src.want[1], rb, ab), b8=b8, reach=dict(esc=[])))
    for name in ("one_escape_per_span_partial", "contig_starts_l0_l1_l1023", "dense_whole_span", "world_b"):
        src = by[name]
        d16 = src.parts["d16"].copy()
        d16[::SPAN] = 0xFFFF
        d16[src.parts["eidx"]] = 0xFFFF
        out.append(edited("hand_d16_ffff_at_anchors_" + name, src, src.want, d16=d16, reach=dict(esc=[int(e) for e in src.parts["eidx"]])))
    src = by["size_1027"]
    out.append(edited("hand_no_escapes_null_lists", src, src.want, null_esc=True, reach=dict(esc=[])))
    src = by["size_2049"]
    at_, val = SPAN + 258, -77
    pos = src.want[0].astype(np.int64).copy()
    pos[at_: 2 * SPAN] += val - pos[at_]  # the escape's value wins over a difference that fits; the sites behind it in the span follow
    assert 0 < src.parts["d16"][at_] < D16_LIMIT
    out.append(edited("hand_escape_where_the_difference_fits", src, (pos.astype(np.int32),) + src.want[1:], eidx=[at_], eval=[val], eoff=[0, 0, 1, 1],
                      reach=dict(esc=[at_])))
    src = by["size_5"]
    top = (1 << 31) - 3
    pos = top + np.cumsum(src.parts["d16"].astype(np.int64)) - int(src.parts["d16"][0])  # past 2^31 - 1: the sum wraps, as any 32-bit adder's
    assert pos[-1] >= (1 << 31)
    out.append(edited("hand_sum_wraps_past_int32_max", src, (pos.astype(np.uint32).view(np.int32),) + src.want[1:], span=[top], reach=dict(esc=[])))
    assert len({c.name for c in out}) == len(out)
    _CACHE["cases"] = out
    return out


def world_cases():
    return [c for c in cases() if c.table is not None]


def family_cases():
    """the cases whose trio comes from form_family (the world tables carry hetcases' columns)"""
    return [c for c in cases() if c.table is None]
