"""The entry points that take a wide-depth list -- uz_family_upload, uz_samples_upload, uz_samples_settle (csrc/tables.hip) -- go through the
one check of csrc/table_views.hpp (tests/test_table_views.py holds its rules without a device): on a table of 5 sites, with one trio or two
sample rows and a wide list of 2 entries, a list with descending sites and one with a depth of 2^30 + 1 are refused with the check's code and
text, the same call with the repaired list succeeds -- the refusal left the context usable -- and uz_family_fetch returns the columns."""
from types import SimpleNamespace

import numpy as np
import pytest

import vcfcases
from filesio import write_bgzf_text, write_tbi
from unfazed_amd import abi, io_native
from unfazed_amd.model import SampleColumns, SitesTable

pytestmark = pytest.mark.gpu

N = 5
E_ARG, E_RANGE = "(-1)", "(-5)"  # unfazed_hip.h UZ_E_ARG, UZ_E_RANGE as the engine words them
TOO_DEEP = (1 << 30) + 1
GOOD_SITES = [1, 3]


def _sites(n=N):
    return SimpleNamespace(contig_off=np.array([0, n], np.int64), pos=np.arange(100, 100 + 10 * n, 10, dtype=np.int32), sflags=np.zeros(n, np.uint8),
                           ref_base=np.full(n, ord("A"), np.uint8), alt_base=np.full(n, ord("G"), np.uint8), n_sites=n, contigs=["chr1"])


def _rows(k, seed):
    """k rows of 5 sites: gt codes 0 .. 3, depths and qualities below 100; the wide list of 2 entries with depths above 32767"""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 4, (k, N)).astype(np.uint8)
    rd, ad, gq = (rng.integers(0, 100, (k, N)).astype(np.uint16) for _ in range(3))
    wide = (np.array(GOOD_SITES, np.int64), rng.integers(40000, 1 << 30, (k, 2)).astype(np.int32), rng.integers(40000, 1 << 30, (k, 2)).astype(np.int32))
    return gt, rd, ad, gq, wide


def _broken(wide):
    """-> [(the list with one rule broken, code, a part of the text for the table's sites, for settled sites)]"""
    site, wr, wa = wide
    deep = wr.copy()
    deep[-1, -1] = TOO_DEEP
    return [((site[::-1].copy(), wr, wa), E_ARG, "ascending site indices of the table", "ascending indices of the settled sites"),
            ((site, deep, wa), E_RANGE, "wide depth outside", "wide depth outside")]


def test_family_upload(engine):
    from unfazed_amd.engine import UnfazedHipError
    gt3, rd, ad, gq, wide = _rows(3, 1)
    gt = (gt3[0] | gt3[1] << 2 | gt3[2] << 4).astype(np.uint8)
    sid = engine.upload_sites(_sites())
    try:
        for bad, code, text, _ in _broken(wide):
            with pytest.raises(UnfazedHipError, match=text) as e:
                engine.add_family(sid, gt, rd, ad, gq, bad)
            assert code in str(e.value)
            fid = engine.add_family(sid, gt, rd, ad, gq, wide)  # the same call, the list repaired
            got_gt, got = engine.family_fetch(fid, N)
            assert np.array_equal(got_gt, gt) and np.array_equal(got, np.concatenate([rd, ad, gq]))
    finally:
        engine.free_sites(sid)


def _trio_of_rows(engine, table_h, gt, rd, ad, gq):
    """the trio (row 0, row 1, row 0) of a table of two rows: its columns are the rows"""
    fid, = engine.families_from_samples(table_h, [0], [1], [0])
    got_gt, got = engine.family_fetch(fid, N)
    assert np.array_equal(got_gt & 0x3F, gt[0] | gt[1] << 2 | gt[0] << 4)
    assert np.array_equal(got, np.stack([rd[0], rd[1], rd[0], ad[0], ad[1], ad[0], gq[0], gq[1], gq[0]]))


def test_samples_upload(engine):
    from unfazed_amd.engine import UnfazedHipError
    gt, rd, ad, gq, wide = _rows(2, 2)
    sid = engine.upload_sites(_sites())
    try:
        for bad, code, text, _ in _broken(wide):
            with pytest.raises(UnfazedHipError, match=text) as e:
                engine.upload_samples(sid, SampleColumns(["a", "b"], gt, rd, ad, gq, bad))
            assert code in str(e.value)
            h = engine.upload_samples(sid, SampleColumns(["a", "b"], gt, rd, ad, gq, wide))
            _trio_of_rows(engine, h, gt, rd, ad, gq)
    finally:
        engine.free_sites(sid)


def _whole(path, **kw):
    names = io_native.tabix_contigs(path)
    k = len(names)
    return io_native.read_vcf_table_regions(path, list(range(k)), [0] * k, [2 ** 31 - 1] * k, **kw)


def test_samples_settle(engine, tmp_path):
    """five records, two of them with a depth above 32767 in the picked columns: the device hands those two back (the unsettled-site cases of
    tests/vcfcases.py), and their cells come with a wide list of 2 entries over the settled sites"""
    from unfazed_amd.engine import UnfazedHipError
    pick = [0, 1]
    by = {c["name"]: c for c in vcfcases.FILE_CASES}
    plain = next(c for c in vcfcases.FILE_CASES if c["fmt"] and not vcfcases.unsettled_records([c], pick))
    text, used = vcfcases.vcf_text(N, cases=[plain, by["depth_32768"], plain, by["depth_two_to_30"], plain])
    assert vcfcases.unsettled_records(used, pick) == GOOD_SITES
    path = str(tmp_path / "five.vcf.gz")
    write_bgzf_text(path, text)
    write_tbi(path)
    eager, lazy = _whole(path), _whole(path, lazy=True)
    want = eager.sample_columns([eager.samples[c] for c in pick])
    assert eager.n_sites == N and want.wide is not None and list(want.wide[0]) == GOOD_SITES
    sid = engine.upload_sites(eager)
    try:
        for k in range(2):
            h, n_back = engine.samples_from_text(sid, lazy, pick, settle=False)
            site = engine.unsettled_sites(h, n_back)
            assert list(site) == GOOD_SITES
            sub = SitesTable(["row0", "row1"], [])  # the cells of the two sites, as HipEngine.settle_samples reads them
            sub.pos = np.zeros(site.size, np.int32)
            sub.gt, sub.ref_depth, sub.alt_depth, sub.gq = io_native.vcf_record_samples(lazy, site, np.asarray(pick, np.int32))
            cells = io_native.pack_samples(sub, np.arange(2))
            assert cells[4] is not None and list(cells[4][0]) == [0, 1]  # (indices of the settled sites)

            def settle(wide):
                v = abi.samples_view(SampleColumns(["row0", "row1"], *cells[:4], wide))
                engine._ck(engine.L.uz_samples_settle(engine.h, h, int(site.size), site.ctypes.data, v.ref()), "uz_samples_settle")

            bad, code, _, text_ = _broken(cells[4])[k]
            with pytest.raises(UnfazedHipError, match=text_) as e:
                settle(bad)
            assert code in str(e.value)
            with pytest.raises(UnfazedHipError, match="unsettled sites"):  # the refused call settled nothing
                engine.families_from_samples(h, [0], [1], [0])
            settle(cells[4])
            _trio_of_rows(engine, h, want.gt, want.ref_depth, want.alt_depth, want.gq)
    finally:
        engine.free_sites(sid)
