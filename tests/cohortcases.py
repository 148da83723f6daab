"""The sites table and the batches shared by tests/test_find_cohort_gpu.py and tests/test_cnv_cohort_gpu.py: 2 000 sites on two contigs, seven
samples, three trios (the third shares a parent with each of the others) whose genotype columns are laid out from the kinds of
tests/sitecases.py, so that stretches of the first contig hold known candidates.  Pure numpy; nothing here touches a device."""
import numpy as np

from sitecases import KIND, KINDS
from unfazed_amd import abi
from unfazed_amd.model import SitesTable

SAMPLES = ["kidA", "dadA", "momA", "kidB", "dadB", "momB", "kidC"]
TRIOS = [("kidA", "dadA", "momA"), ("kidB", "dadB", "momB"), ("kidC", "dadA", "momB")]  # C's parents are A's dad and B's mom
N0, N1 = 1300, 700
GAP_AFTER = 1000  # 20 kb without a site behind this site of the first contig
SEARCH_DIST = 300
# stretches of the first contig (site indices) and the kinds trio A / trio B hold there
MIXED_DEL = (200, 500)   # A: all four DEL kinds in turn -- 300 candidates of a DEL (five ballot rounds), none of a DUP
DAD_ONLY = (500, 580)    # A: every candidate votes dad; B: every candidate votes mom
MOM_ONLY = (580, 660)    # A: every candidate votes mom; B: DUP kinds, dad
DUPS = (660, 760)        # A: the two DUP kinds in turn

_CACHE = {}


def _k(*names):
    return [KINDS.index(x) for x in names]


def table() -> SitesTable:
    if "t" in _CACHE:
        return _CACHE["t"]
    n = N0 + N1
    i = np.arange(n)
    every = np.arange(len(KINDS))
    kA, kB, kC = every[i % 7], every[(i + 3) % 7], every[(3 * i + 1) % 7]
    for (lo, hi), a, b in ((MIXED_DEL, _k("del_dad_a", "del_mom_b", "del_dad_b", "del_mom_a"), None),
                           (DAD_ONLY, _k("del_dad_a", "del_dad_b"), _k("del_mom_a", "del_mom_b")),
                           (MOM_ONLY, _k("del_mom_a", "del_mom_b"), _k("dup_dad")),
                           (DUPS, _k("dup_dad", "dup_mom"), None)):
        j = np.arange(lo, hi)
        kA[lo:hi] = np.asarray(a)[j % len(a)]
        if b is not None:
            kB[lo:hi] = np.asarray(b)[j % len(b)]
    gts = np.array([KIND[k][0] for k in KINDS], np.int64)                              # [kind][member]
    rds = np.array([[KIND[k][1 + m][0] for m in range(3)] for k in KINDS], np.int64)
    ads = np.array([[KIND[k][1 + m][1] for m in range(3)] for k in KINDS], np.int64)
    t = SitesTable(SAMPLES, ["1", "2"])
    p0 = 1000 + 10 * np.arange(N0, dtype=np.int64)
    p0[GAP_AFTER + 1:] += 20_000
    p0[40:43] = p0[40]  # a run of equal positions inside a window
    p1 = 500 + 7 * np.arange(N1, dtype=np.int64)
    t.contig_off = np.asarray([0, N0, n], np.int64)
    t.pos = np.concatenate([p0, p1]).astype(np.int32)
    t.end = t.pos + 1
    t.sflags = (i % 13 == 5).astype(np.uint8)  # complex sites: class 0 in every family
    t.ref_base = np.where(t.sflags == 0, ord("A"), 0).astype(np.uint8)
    t.alt_base = np.where(t.sflags == 0, ord("C"), 0).astype(np.uint8)
    t.gt = np.zeros((7, n), np.uint8)
    t.ref_depth = np.zeros((7, n), np.int32)
    t.alt_depth = np.zeros((7, n), np.int32)
    t.gq = np.full((7, n), 99.0)
    for rows, kinds in (((0, 1, 2), kA), ((3, 4, 5), kB), ((6,), kC)):  # kidC: the kid column of its own walk over the kinds
        for m, r in enumerate(rows):
            t.gt[r], t.ref_depth[r], t.alt_depth[r] = gts[kinds, m], rds[kinds, m], ads[kinds, m]
    t.gq[:, 77::101] = 5.0  # a few sites nobody is sure of
    t.ref_str = ["A"] * n
    t.alt_strs = [["C"]] * n
    _CACHE["t"] = t
    return t


def pos0(k):
    return int(table().pos[k])


def family_held(trio):
    """the trio's columns as the oracle takes them"""
    t = table()
    gt, rd, ad, gq = t.family_columns(*trio)
    return abi.family_view(gt, rd, ad, gq, t.wide_depths)


def make_families(engine, sites_h):
    """the three trios made on the device from one sample table, not scanned"""
    cols = table().sample_columns(SAMPLES)
    mid = engine.upload_samples(sites_h, cols)
    return engine.families_from_samples(mid, [cols.row(t[0]) for t in TRIOS], [cols.row(t[1]) for t in TRIOS], [cols.row(t[2]) for t in TRIOS])


def view(rows, mode=None):
    """rows: (contig, start, end, mult, vartype); mult counts in find_many's mode (0) only"""
    return abi.dnms_view([r[0] for r in rows], [-1] * len(rows), [r[1] for r in rows], [r[2] for r in rows], np.asarray([r[4] for r in rows], np.uint8),
                         [b""] * len(rows), [b""] * len(rows), 0.0, mult=[r[3] if mode == 0 else 1 for r in rows])


def find_batch():
    """-> (rows of the 12 DNMs, groups [(trio index, first, count)]): sizes 0, 1, 5 and 6, listed out of DNM order, the last two on one
    family, the empty one at the batch's end"""
    gap = pos0(GAP_AFTER)
    DEL, DUP, SV, PT = abi.VT_DEL, abi.VT_DUP, abi.VT_OTHER_SV, abi.VT_POINT
    rows = [
        (-1, 5000, 5001, 1, DEL),                                            # no such contig
        (1, int(table().pos[N0 + 100]), int(table().pos[N0 + 100]) + 1, 1, DUP),  # the second contig
        (0, pos0(150), pos0(150) + 400, 1, SV),                              # search_dist < length <= 2 search_dist: the two windows overlap (lane 0 walks them)
        (0, gap + 9000, gap + 9001, 1, PT),                                  # no site in reach
        (0, pos0(900), pos0(900) + 1, 2, DEL),
        (0, pos0(41), pos0(41) + 1, 3, DUP),                                 # group of one, family B: on the run of equal positions
        (0, pos0(MIXED_DEL[0]) - 1, pos0(MIXED_DEL[1] - 1) + 1, 1, DEL),     # a DEL over 300 candidates of A; two windows far apart otherwise
        (0, gap + 3000, gap + 6000, 1, DEL),                                 # a DEL over none
        (0, pos0(DUPS[0]) - 1, pos0(DUPS[1] - 1) + 1, 1, DUP),
        (0, pos0(0), pos0(0) + 1, 1, PT),                                    # the window starts before the contig's first site
        (0, pos0(300), pos0(300) + 15, 1, DEL),                              # a small event: the sites inside are left out
        (0, pos0(N0 - 1), pos0(N0 - 1) + 1, 1, DUP),                         # the contig's last site
    ]
    groups = [(2, 12, 0), (1, 5, 1), (0, 0, 5), (0, 6, 6)]
    return rows, groups


def cnv_batch():
    """-> (rows of the 9 events, groups): three kids, kid by kid"""
    gap = pos0(GAP_AFTER)
    DEL, DUP, SV = abi.VT_DEL, abi.VT_DUP, abi.VT_OTHER_SV
    span = lambda lo, hi: (pos0(lo) - 1, pos0(hi - 1) + 1)  # noqa: E731
    t = table()
    rows = [
        (0,) + span(*MIXED_DEL) + (1, DEL),   # A: 300 candidates, both parents
        (0,) + span(*DAD_ONLY) + (1, DEL),    # A: every vote dad's
        (0,) + span(*MOM_ONLY) + (1, DEL),    # A: every vote mom's
        (0,) + span(*DUPS) + (1, DUP),        # A
        (0, gap + 3000, gap + 6000, 1, DEL),  # B: no candidate
        (0,) + span(*DAD_ONLY) + (1, SV),     # B: not a CNV -- candidates in reach, nobody votes
        (0,) + span(*MOM_ONLY) + (1, DUP),    # B: every vote dad's
        (1, int(t.pos[N0 + 50]), int(t.pos[N0 + 400]), 1, DEL),  # C, second contig
        (0,) + span(0, 200) + (1, DUP),       # C
    ]
    groups = [(0, 0, 4), (1, 4, 3), (2, 7, 2)]
    return rows, groups
