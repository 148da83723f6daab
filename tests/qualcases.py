"""The table of the base-quality-bit tests (uz_types.h bl_qlow; tests/test_pack_select_quals.py on the CPU, tests/test_base_quals_gpu.py on the
device): a generated workload as tests/test_pack_select.py builds it, its quality bytes overwritten so that every rule of the form has records
that meet it BY CONSTRUCTION.

Which records of a selection carry a base list, and at which positions, depends on the fetches, the CIGARs and the bases only, never on the
qualities: the lists of a first selection say where to put the low qualities.

260 DNMs, not the ~40 a packer test needs.  The device test wants this table built by k_pack_link, which takes a table only while its dictionary
of small-column combinations (unit masks x list lengths x counts) fits the build's scratch: 6 combinations per span of 1 024 records, 256 at the
least.  A selection of 40 DNMs has 17 spans and ~240 combinations, which only just fits the 256; this one has ~110 spans, room for ~670, and
~350 combinations."""
import functools
import types

import numpy as np

from oracle import oracle as orc
from test_pack_select import _sites_views, _workload
from unfazed_amd import abi, io_native
from unfazed_amd.hostpath import concordant_cutoff
from unfazed_amd.staging import fetch_points

ROW = 160  # bytes of a record's row in the generator's seq / qual columns (151 bases, rows at multiples of 16)
HIGH, LOW = 40, 3
N_LISTED_LOW, N_UNLISTED_LOW, N_MANY_LOW = 80, 80, 12  # records rewritten per group


@functools.lru_cache(maxsize=None)
def table():
    """-> namespace: the source table (rh / arrs, qualities rewritten), the selection's fetches, and per group the SOURCE indices of the records
    whose qualities were written: listed_low (one low-quality LISTED base, two low unlisted ones -- one of them in the listed base's own
    unit), unlisted_low (low-quality bases at unlisted positions only, some in the staged unit), many_low (more than UZ_QLOW_LIST_MAX low
    bases, a listed one among them)"""
    sc, dn, cl, rh, arrs = _workload(260, seed=31)
    n = dn.n
    sh, fh = _sites_views(sc)
    P = abi.make_params()
    thr = int(P.min_gt_qual)
    cutoff = concordant_cutoff(arrs["tlen"], 151, 3)
    dv = abi.dnms_view(dn.contig, dn.contig, dn.start, dn.end, np.zeros(n, np.uint8), dn.refs, dn.alts, cutoff)
    found = orc.find(P, sh, fh, dv, abi.FIND_SECOND_WINDOW)
    alen = np.array([max(len(r), len(x)) for r, x in zip(dn.refs, dn.alts)], np.int64)
    fc, flo, fhi, fex = fetch_points(dn.contig, dn.start, np.zeros(n, np.uint8), sc.pos, found[3], found[4], P, allele_len=alen)
    first, idx = io_native.ReadsSource(io_native.pack_reads(rh, thr, with_end=True)).select(fc, flo, fhi, want_index=True, extra=fex)
    off, pos, _ = abi.base_lists(first)
    cnt = np.diff(off)
    ls = abi.small_columns(first)["l_seq"][: idx.size].astype(np.int64)
    listed = np.nonzero((cnt > 0) & (ls == 151))[0]
    assert listed.size > N_LISTED_LOW + N_UNLISTED_LOW + N_MANY_LOW
    # spread over the whole selection: every span of 1 024 records gets some of each group
    pick = listed[np.linspace(0, listed.size - 1, N_LISTED_LOW + N_UNLISTED_LOW + N_MANY_LOW).astype(np.int64)]
    qual = arrs["qual"]
    # Every other record keeps at most the first of its generated low-quality bases: the generator's counts of 0 .. 15 low bases alone would
    # multiply the dictionary's combinations by sixteen, past the scratch of k_pack_link (the module's docstring)
    N = int(rh.view.n_segs)
    rows = qual[: N * ROW].reshape(N, ROW)
    assert np.array_equal(arrs["sq_off16"][:N].astype(np.int64) * 16, np.arange(N, dtype=np.int64) * ROW)
    low = rows[:, :151] < thr
    first_low = low & (np.cumsum(low, axis=1) == 1)
    rows[:, :151][low & ~first_low] = HIGH
    groups = {"listed_low": [], "unlisted_low": [], "many_low": []}

    def unlisted_near(lp, want):
        """`want` positions of the read that are not listed, the first of them in the unit of the first listed base"""
        u0 = int(lp[0]) >> 5
        out = [q for q in range(32 * u0, min(32 * u0 + 32, 151)) if q not in lp][:1]
        out += [q for q in range(150, -1, -1) if q not in lp and q not in out][: want - 1]
        return out

    for j, k in enumerate(pick):
        i = int(idx[k])
        lp = [int(x) for x in pos[off[k]: off[k + 1]]]
        r0 = int(arrs["sq_off16"][i]) * 16
        qual[r0: r0 + 151] = HIGH
        g = ("listed_low", "unlisted_low", "many_low")[j % 3 if j < 3 * N_MANY_LOW else j % 2]
        if g == "listed_low":
            qual[r0 + lp[j % len(lp)]] = LOW
            qual[[r0 + q for q in unlisted_near(lp, 2)]] = LOW
        elif g == "unlisted_low":
            qual[[r0 + q for q in unlisted_near(lp, 3)]] = LOW
        else:
            qual[r0 + lp[0]] = LOW
            qual[[r0 + q for q in unlisted_near(lp, abi.QLOW_LIST_MAX + 2)]] = LOW
        groups[g].append(i)
    return types.SimpleNamespace(sc=sc, dn=dn, rh=rh, arrs=arrs, P=P, thr=thr, sh=sh, fh=fh, dv=dv, found=found, cutoff=cutoff,
                                 fetches=(fc, flo, fhi, fex), groups={k: np.array(v, np.int64) for k, v in groups.items()})


def source():
    """the table packed for its threshold, opened for selections (a fresh source: the packed columns are its own)"""
    t = table()
    return io_native.ReadsSource(io_native.pack_reads(t.rh, t.thr, with_end=True))


def select(src, base_quals, **kw):
    t = table()
    fc, flo, fhi, fex = t.fetches
    return src.select(fc, flo, fhi, want_index=True, extra=fex, base_quals=base_quals, **kw)


def low_bits(i):
    """0 / 1 per base of source record i: quality below the threshold, from the source's quality bytes"""
    t = table()
    r0 = int(t.arrs["sq_off16"][i]) * 16
    return (t.arrs["qual"][r0: r0 + int(t.arrs["l_seq"][i])].astype(np.int64) < t.thr).astype(np.uint8)
