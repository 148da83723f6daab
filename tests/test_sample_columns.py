"""SitesTable.sample_columns: the device-facing columns made once per SAMPLE (the cohort form, uz_samples_view) hold exactly what
family_columns makes per TRIO -- for every trio drawn from a table, its three rows are family_columns' nine columns, and the table-level
wide list restricted to the trio's own too-deep sites is family_columns' `wide_depths`.  The native packer (uz_samples_pack) and the numpy
version give the same bytes, on a decoder-made table and on a from_records one."""
import itertools

import numpy as np
import pytest

from unfazed_amd import io_native
from unfazed_amd.model import SiteRecord, SitesTable

SPECIAL_DEPTHS = [-1, 0, 1, 32766, 32767, 32768, 40000, 1 << 30]


def _records(n, ns, seed, deep=True):
    rng = np.random.default_rng(seed)
    recs, pos = [], 100
    for i in range(n):
        pos += int(rng.integers(1, 900))
        cx = rng.random() < 0.1
        ref = "AT" if cx else "ACGT"[int(rng.integers(4))]
        alts = ["C", "G"] if (cx and rng.random() < 0.5) else ["ACGT"[int(rng.integers(4))]]
        rd = rng.integers(0, 70, ns)
        ad = rng.integers(0, 70, ns)
        gq = rng.integers(0, 100, ns).astype(np.float64)
        frac = rng.random(ns) < 0.3
        gq[frac] += rng.choice([0.25, 0.5, 0.75], int(frac.sum()))  # fractional GQ: floor
        for s in range(ns):
            u = rng.random()
            if u < 0.08:
                rd[s] = ad[s] = -1  # missing AD ("." in the file)
            elif deep and u < 0.14:
                rd[s] = SPECIAL_DEPTHS[int(rng.integers(len(SPECIAL_DEPTHS)))]
                ad[s] = max(0, SPECIAL_DEPTHS[int(rng.integers(len(SPECIAL_DEPTHS)))]) if rd[s] >= 0 else -1
            v = rng.random()
            if v < 0.07:
                gq[s] = -1.0  # missing
            elif v < 0.12:
                gq[s] = np.nan
        recs.append(SiteRecord("1" if i < n * 2 // 3 else "2", pos, ref, alts, rng.integers(0, 4, ns).tolist(), rd.tolist(), ad.tolist(), gq.tolist()))
        if i == n * 2 // 3 - 1:
            pos = 50
    return recs


def _decoder_table(tmp_path, recs, samples):
    """the records as a multi-sample VCF, decoded by the native decoder ([ns][S] columns in the library's memory)"""
    import filesio
    from filesio import vcf_text
    for r in recs:  # (the text form has no NaN: "." is the file's missing GQ; the from_records table covers NaN)
        r.gt_quals = [(-1.0 if (q != q) else q) for q in r.gt_quals]
    p = tmp_path / "multi.vcf"
    num = filesio._num
    # (the writer's "%g" keeps six digits: 2^30 would come back as 1.07374e+09 -- whole numbers are written in full here)
    filesio._num = lambda x: "." if (x is None or x < 0) else (str(int(x)) if float(x).is_integer() else repr(float(x)))
    try:
        p.write_text(vcf_text(samples, recs, ["1", "2"]))
    finally:
        filesio._num = num
    return io_native.read_vcf_table(str(p))


def _check_trios(t, trios, cols):
    for kid, dad, mom in trios:
        gt, rd, ad, gq = t.family_columns(kid, dad, mom)
        wide = t.wide_depths
        rows = [cols.row(s) for s in (kid, dad, mom)]
        want_gt = (cols.gt[rows[0]] & 3) | ((cols.gt[rows[1]] & 3) << 2) | ((cols.gt[rows[2]] & 3) << 4)
        assert np.array_equal(want_gt.astype(np.uint8), gt)
        for m in range(3):
            assert np.array_equal(cols.ref_depth[rows[m]], rd[m]) and np.array_equal(cols.alt_depth[rows[m]], ad[m]) and np.array_equal(cols.gq[rows[m]], gq[m])
        if wide is None:
            # none of the trio's sites is too deep: whatever the table lists for OTHER samples' sake holds depths the 16-bit columns hold too
            if cols.wide is not None:
                assert (cols.wide[1][rows] <= 32767).all() and (cols.wide[2][rows] <= 32767).all()
            continue
        ws, wr, wa = wide
        at = np.searchsorted(cols.wide[0], ws)
        assert np.array_equal(cols.wide[0][at], ws)  # every wide site of the trio stands in the table's list
        assert np.array_equal(cols.wide[1][rows][:, at], wr) and np.array_equal(cols.wide[2][rows][:, at], wa)
        others = np.setdiff1d(np.arange(cols.wide[0].size), at)
        assert (cols.wide[1][rows][:, others] <= 32767).all() and (cols.wide[2][rows][:, others] <= 32767).all()


def _same_bytes(a, b):
    for k in ("gt", "ref_depth", "alt_depth", "gq"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert (a.wide is None) == (b.wide is None)
    if a.wide is not None:
        for x, y in zip(a.wide, b.wide):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind", ["from_records", "decoder"])
def test_sample_rows_are_the_family_columns_of_every_trio(tmp_path, kind):
    samples = ["s%d" % i for i in range(7)]
    recs = _records(400, len(samples), seed=31)
    t = SitesTable.from_records(recs, samples) if kind == "from_records" else _decoder_table(tmp_path, recs, samples)
    assert t.n_sites == 400 and (t.ref_depth > 32767).any() and (t.ref_depth == 32767).any() and (t.alt_depth == (1 << 30)).any()
    if kind == "from_records":
        assert np.isnan(t.gq).any() and (t.gq != np.floor(t.gq))[~np.isnan(t.gq)].any()
    names = [samples[i] for i in (5, 0, 3, 6, 1, 2)]  # (a subset, in another order than the file's)
    native, plain = t.sample_columns(names, impl="native"), t.sample_columns(names, impl="numpy")
    _same_bytes(native, plain)
    default = t.sample_columns(names)
    _same_bytes(default, native)
    assert native.wide is not None and native.wide[0].size >= 3 and np.all(np.diff(native.wide[0]) > 0)
    assert native.gt.shape == (6, 400) and native.names == names
    _check_trios(t, list(itertools.permutations(names, 3))[::3], native)


def test_a_table_without_deep_sites_has_no_wide_list_and_an_empty_table_packs():
    samples = ["a", "b", "c", "d"]
    t = SitesTable.from_records(_records(120, 4, seed=5, deep=False), samples)
    for impl in ("native", "numpy"):
        c = t.sample_columns(samples, impl=impl)
        assert c.wide is None
        _check_trios(t, [("a", "b", "c"), ("d", "b", "c"), ("b", "d", "a")], c)
    e = SitesTable(samples, ["1"])
    for impl in ("native", "numpy"):
        c = e.sample_columns(["c", "a", "b"], impl=impl)
        assert c.gt.shape == (3, 0) and c.gq.shape == (3, 0) and c.ref_depth.dtype == np.uint16 and c.wide is None
    _same_bytes(e.sample_columns(samples, impl="native"), e.sample_columns(samples, impl="numpy"))
    none = t.sample_columns([], impl="native")
    assert none.gt.shape == (0, 120)
    _same_bytes(none, t.sample_columns([], impl="numpy"))


def test_the_rows_can_be_written_into_the_callers_memory():
    samples = ["a", "b", "c"]
    t = SitesTable.from_records(_records(90, 3, seed=8), samples)
    for impl in ("native", "numpy"):
        got = []

        def alloc(nbytes):
            got.append(np.zeros(nbytes + 64, np.uint8))
            return got[-1]
        c = t.sample_columns(samples, alloc=alloc, impl=impl)
        assert len(got) == 4
        assert all(any(np.shares_memory(x, g) for g in got) for x in (c.gt, c.ref_depth, c.alt_depth, c.gq))
        _same_bytes(c, t.sample_columns(samples, impl=impl))


@pytest.mark.parametrize("impl", ["native", "numpy"])
def test_a_depth_below_minus_one_or_above_two_to_the_thirty_is_refused(impl):
    samples = ["a", "b", "c", "d"]
    t = SitesTable.from_records(_records(60, 4, seed=9), samples)
    t.alt_depth[2, 17] = -2
    with pytest.raises(ValueError):
        t.sample_columns(samples, impl=impl)
    with pytest.raises(ValueError):
        t.family_columns("a", "b", "c")
    t.sample_columns(["a", "b", "d"], impl=impl)  # (the bad value is another sample's: as family_columns of a trio without it)
    t.alt_depth[2, 17] = 3
    t.ref_depth[0, 5] = (1 << 30) + 1
    with pytest.raises(OverflowError):
        t.sample_columns(samples, impl=impl)
