"""The site stage on the device (k_build_ab_lut, k_site_scan and its T0 / CNV / BATCH / SPT builds, k_site_scan_wide, k_window_wave,
k_window_region, k_scan2, k_cnv_count) held EXACTLY to the C oracle on the hand-built edge tables of tests/sitecases.py.
tests/test_site_model.py holds the oracle to the numpy model of tests/sitemodel.py on the same cases, and asserts that the cases reach
the branches they are named for; it must pass before this file is trusted.

Every comparison is np.array_equal; there are no tolerances.  The SPT = 16 build is compared in one child process (UZ_SITE_SPT is read
once per process): this module, run as a script, classifies the threshold, shape and wide tables and writes the classes to a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import sitecases
from unfazed_amd import abi

pytestmark = pytest.mark.gpu
LISTS = ("cand_off", "cand_idx", "cand_flags", "het_off", "het_idx")


def _upload(engine, t):
    sid = engine.upload_sites(t)
    return sid, engine.add_family(sid, *t.family_columns())


def _first_diff(want, got):
    i = np.nonzero(want != got)[0]
    return "%d sites differ, first %s: want %s got %s" % (i.size, i[:5].tolist(), want[i[:5]].tolist(), got[i[:5]].tolist())


def _assert_lists(want, got, what, dn=None):
    for name, a, b in zip(LISTS, want, got):
        if not np.array_equal(a, b):
            msg = "%s: %s differs" % (what, name)
            if dn is not None:
                off = 0 if name.startswith("cand") else 3
                d = np.nonzero(np.diff(want[off]) != np.diff(got[off]))[0]
                if d.size == 0 and a.shape == b.shape:
                    d = np.unique(np.searchsorted(want[off], np.nonzero(a != b)[0], "right") - 1)
                msg += "; DNMs %s: %s" % (d[:5].tolist(), [(dn["tags"][i], int(dn["contig"][i]), int(dn["start"][i]), int(dn["end"][i]), int(dn["mult"][i])) for i in d[:5]])
            raise AssertionError(msg)


def _cover_all(t, sd):
    """one point DNM whose window holds the whole table (positions 0 .. n - 1)"""
    return dict(contig=np.zeros(1, np.int32), start=np.zeros(1, np.int32), end=np.ones(1, np.int32), vartype=np.zeros(1, np.uint8),
                mult=np.ones(1, np.uint8), tags=["all"])


# --------------------------------------------------------------------------------------------------------------------------------- K1
def test_point_mode_lists_of_a_fresh_family(engine):
    """find() in point and breakpoint mode scans a family that has no classes yet with the kernel's CNV = false build; it shows only in
    the lists.  First in this file, on families of their own: the threshold table under the default, the one-ulp and the T0 parameter
    sets (one window over the whole table), then the window table."""
    from oracle import oracle as orc
    t = sitecases.Table.tiled(sitecases.threshold_table(), sitecases.threshold_table().n_sites, roll=0, name="thresholds_in_order")
    sid, fid = _upload(engine, t)
    sv, fv = t.sites_view(), t.family_view()
    dn = _cover_all(t, t.n_sites)
    for name, kw in sitecases.SHAPE_PARAMS:
        P = abi.make_params(search_dist=t.n_sites + 10, **kw)
        dv = sitecases.dnms_view(dn)
        want = orc.find(P, sv, fv, dv, 0)
        _assert_lists(want, engine.find(fid, dv, P, 0), "thresholds, " + name)
        assert want[0][1] > 100 and want[3][1] > 100
    engine.free_sites(sid)
    t = sitecases.window_table(False)
    sid, fid = _upload(engine, t)
    sv, fv = t.sites_view(), t.family_view()
    dn = sitecases.window_dnms(0)
    dv = sitecases.dnms_view(dn)
    for sd in sitecases.SEARCH_DISTS:
        for mode in (0, abi.FIND_SECOND_WINDOW):
            P = abi.make_params(search_dist=sd)
            _assert_lists(orc.find(P, sv, fv, dv, mode), engine.find(fid, dv, P, mode), "windows sd %d mode %d" % (sd, mode), dn)
    engine.free_sites(sid)


def test_threshold_table_under_every_parameter_set(engine):
    """k_build_ab_lut's interval table (LDS copy below total 510, global above; ties; empty, unbounded and infinite windows; the T0 build)
    and the CNV bits at their edges: the classes of the threshold table under every parameter set of sitecases.k1_param_sets"""
    from oracle import oracle as orc
    t = sitecases.threshold_table()
    sid, fid = _upload(engine, t)
    sv, fv = t.sites_view(), t.family_view()
    bad = []
    for name, kw in sitecases.k1_param_sets():
        P = abi.make_params(**kw)
        want, got = orc.classify(P, sv, fv), engine.classify(fid, P, t.n_sites)
        if not np.array_equal(want, got):
            bad.append("%s: %s" % (name, _first_diff(want, got)))
    engine.free_sites(sid)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("n", sitecases.SHAPE_NS)
def test_shapes(engine, n):
    from oracle import oracle as orc
    t = sitecases.shape_tables()[sitecases.SHAPE_NS.index(n)]
    sid, fid = _upload(engine, t)
    for name, kw in sitecases.SHAPE_PARAMS:
        P = abi.make_params(**kw)
        want, got = orc.classify(P, t.sites_view(), t.family_view()), engine.classify(fid, P, n)
        assert np.array_equal(want, got), (name, _first_diff(want, got))
    engine.free_sites(sid)


def test_grid_stride_second_trip(engine):
    """4096 * 2048 + 2048 + 5 sites: every workgroup of the capped grid takes a second chunk, then a partial chunk and a scalar tail"""
    from oracle import oracle as orc
    t = sitecases.big_table()
    sid, fid = _upload(engine, t)
    sv, fv = t.sites_view(), t.family_view()
    for name, kw in (sitecases.SHAPE_PARAMS[0], sitecases.SHAPE_PARAMS[2]):
        P = abi.make_params(**kw)
        want, got = orc.classify(P, sv, fv), engine.classify(fid, P, t.n_sites)
        assert np.array_equal(want, got), (name, _first_diff(want, got))
    engine.free_sites(sid)


def test_batch_form_strides(engine):
    """256 families of 18 chunks: 16 workgroups per family, so blockIdx.x strides in the BATCH build; every family is another walk over
    the threshold table"""
    from oracle import oracle as orc
    fams = sitecases.batch_tables()
    sid = engine.upload_sites(fams[0])
    fids = [engine.add_family(sid, *t.family_columns()) for t in fams]
    sv = fams[0].sites_view()
    for name, kw in (sitecases.SHAPE_PARAMS[0], sitecases.SHAPE_PARAMS[2]):
        P = abi.make_params(**kw)
        engine.set_params(P)
        engine.site_scan_many(fids)
        for k, (t, f) in enumerate(zip(fams, fids)):
            want, got = orc.classify(P, sv, t.family_view()), engine.classify(f, P, t.n_sites)  # (fresh: no rescan)
            assert np.array_equal(want, got), (name, k, _first_diff(want, got))
    engine.free_sites(sid)


@pytest.mark.parametrize("k", range(4), ids=["first", "last", "w256", "w257"])
def test_wide_list(engine, k):
    from oracle import oracle as orc
    t = sitecases.wide_tables()[k]
    sid, fid = _upload(engine, t)
    for name, kw in sitecases.WIDE_PARAMS:
        P = abi.make_params(**kw)
        want, got = orc.classify(P, t.sites_view(), t.family_view()), engine.classify(fid, P, t.n_sites)
        assert np.array_equal(want, got), (name, _first_diff(want, got))
    engine.free_sites(sid)


# --------------------------------------------------------------------------------------------------------------------------------- K2
@pytest.fixture(scope="module")
def window_family(engine):
    out = {}
    for mixed in (False, True):
        t = sitecases.window_table(mixed)
        out[mixed] = (t,) + _upload(engine, t)
    yield out
    for t, sid, fid in out.values():
        engine.free_sites(sid)


@pytest.mark.parametrize("sd,mode", sitecases.WINDOW_RUNS)
def test_windows(engine, window_family, sd, mode):
    from oracle import oracle as orc
    t, sid, fid = window_family[bool(mode & abi.FIND_WHOLE_REGION)]
    dn = sitecases.window_dnms(mode)
    dv = sitecases.dnms_view(dn)
    P = abi.make_params(search_dist=sd)
    want = orc.find(P, t.sites_view(), t.family_view(), dv, mode)
    _assert_lists(want, engine.find(fid, dv, P, mode), "sd %d mode %d" % (sd, mode), dn)


@pytest.mark.parametrize("size", sitecases.BATCH_SIZES)
def test_batch_sizes_across_scan_tiles(engine, window_family, size):
    """k_scan2's 4096-count tile: one DNM short of a tile, a whole tile, the hand-over to a second and a third, zero counts at the edges"""
    from oracle import oracle as orc
    t, sid, fid = window_family[False]
    dn = sitecases.batch_dnms(size)
    dv = sitecases.dnms_view(dn)
    P = abi.make_params(search_dist=5)
    want = orc.find(P, t.sites_view(), t.family_view(), dv, abi.FIND_SECOND_WINDOW)
    _assert_lists(want, engine.find(fid, dv, P, abi.FIND_SECOND_WINDOW), "batch of %d" % size, dn)


def test_fill_pass_with_too_little_room(engine, window_family):
    """UZ_TEST_FIND_CAP (the room the first fill pass may use): 1, exactly one DNM's end offset, one less, the total; each followed by a
    smaller batch on the same context"""
    from oracle import oracle as orc
    t, sid, fid = window_family[False]
    dn = sitecases.window_dnms(0)
    dv = sitecases.dnms_view(dn)
    small = sitecases.batch_dnms(50)
    dvs = sitecases.dnms_view(small)
    P = abi.make_params(search_dist=5000)
    mode = abi.FIND_SECOND_WINDOW
    want = orc.find(P, t.sites_view(), t.family_view(), dv, mode)
    want_small = orc.find(P, t.sites_view(), t.family_view(), dvs, mode)
    d = len(dn["start"]) // 3
    edge = int(want[3][d + 1])
    assert 1 < edge - 1 and edge < int(want[3][-1]) and want[3][d + 1] > want[3][d]
    try:
        for cap in (1, edge, edge - 1, int(want[3][-1])):
            os.environ["UZ_TEST_FIND_CAP"] = str(cap)
            engine.drop_derived()
            _assert_lists(want, engine.find(fid, dv, P, mode), "room %d" % cap, dn)
            _assert_lists(want_small, engine.find(fid, dvs, P, mode), "smaller batch behind room %d" % cap, small)
    finally:
        os.environ.pop("UZ_TEST_FIND_CAP", None)


# --------------------------------------------------------------------------------------------------------------------------------- K6
@pytest.mark.parametrize("ratio", sitecases.RATIOS)
def test_cnv_counts_and_decision(engine, ratio):
    from oracle import oracle as orc
    t, _ = sitecases.cnv_world()
    sid, fid = _upload(engine, t)
    P = abi.make_params(evidence_min_ratio=ratio)
    for name, dn, rb in sitecases.cnv_cases():
        dv = sitecases.dnms_view(dn)
        want = orc.phase_cnv(P, t.sites_view(), t.family_view(), dv, rb)
        got = engine.phase_cnv(fid, dv, P, rb)
        for k in ("cnv_counts", "origin", "evidence", "etype"):
            assert np.array_equal(want[k], got[k]), (name, k, np.nonzero((want[k] != got[k]).reshape(len(dn["start"]), -1).any(axis=1))[0][:5].tolist())
        for d in range(len(dn["start"])):
            for j in range(2):
                assert np.array_equal(want["lists"][d][j], got["lists"][d][j]), (name, d, j)
    engine.free_sites(sid)


# ------------------------------------------------------------------------------------------------------------------- the SPT = 16 build
def _spt_tables():
    return [sitecases.threshold_table()] + sitecases.shape_tables() + sitecases.wide_tables() + [sitecases.batch_tables()[3]]


def test_spt16_build_in_a_child_process(hip_lib, tmp_path):
    """the ColVec<16> path (UZ_SITE_SPT = 16, read once per process): one child classifies the threshold, shape and wide tables and one
    18-chunk walk (everything but the 8 M-site table; UZ_SITE_WGS is left alone) and writes the classes; compared here with the oracle"""
    from oracle import oracle as orc
    out = str(tmp_path / "classes.npy")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, UZ_SITE_SPT="16"), timeout=240,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "child failed (%d):\n%s" % (r.returncode, r.stdout[-4000:])
    got = np.load(out)
    at = 0
    for t in _spt_tables():
        for name, kw in sitecases.SHAPE_PARAMS:
            want = orc.classify(abi.make_params(**kw), t.sites_view(), t.family_view())
            g = got[at: at + t.n_sites]
            assert g.size == t.n_sites and np.array_equal(want, g), (t.name, name, _first_diff(want, g))
            at += t.n_sites
    assert at == got.size


def _child(out):
    assert os.environ.get("UZ_SITE_SPT") == "16"
    from unfazed_amd import build
    from unfazed_amd.engine import HipEngine
    build.build()
    e = HipEngine(0)
    parts = []
    try:
        for t in _spt_tables():
            sid, fid = _upload(e, t)
            for name, kw in sitecases.SHAPE_PARAMS:
                parts.append(e.classify(fid, abi.make_params(**kw), t.n_sites).copy())
            e.free_sites(sid)
    finally:
        e.close()
    np.save(out, np.concatenate(parts))


if __name__ == "__main__":
    _child(sys.argv[1])
