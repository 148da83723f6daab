"""The compact site form on the device (uz_types.h: uz_sites_view.pos_d16 ...): a chunk's site windows staged compact must give the same
site classes, the same find and the same staged results as the same windows staged in the plain columns; a broken escape list is refused."""
import ctypes as C

import numpy as np
import pytest

from unfazed_amd import abi, pipeline

pytestmark = pytest.mark.gpu

MODE = abi.FIND_SECOND_WINDOW
KEYS = ("status", "counts", "origin", "evidence")


@pytest.fixture(scope="module")
def load(engine):
    from synth.benchload import BenchLoad
    ld = BenchLoad(6000, 1_500_000, workload="snv")
    P = abi.make_params()
    engine.set_params(P)
    sid, fid, rid = ld.adopt(engine, P)
    yield ld, P, fid, rid
    engine.free_reads(rid)
    engine.free_sites(sid)
    ld.free()


def _upload(engine, ld, pool, sel, compact):
    held, hs, hg, wide, ns = ld.pinned_sites(pool, sel, compact=compact)
    sid, fid = engine.upload_sites_family_async(held, hs["gt"], hg["rd"], hg["ad"], hg["gq"], wide)
    return sid, fid, (held, hs, hg, wide)


def test_site_classes_and_find_match_the_plain_form(engine, load):
    from unfazed_amd.engine import PinnedPool
    ld, P, _, _ = load
    pool = PinnedPool()
    try:
        for a, b in ((0, 2000), (2000, 6000)):
            sel = ld.window_sites(a, b, P)
            assert sel.size > 2 * 1024
            out = []
            for compact in (False, True):
                sid, fid, keep = _upload(engine, ld, pool, sel, compact)
                dv = ld.view_of(a, b)
                co, ci, cf, ho, hi = engine.find(fid, dv, P, MODE)
                cls = engine.classify(fid, P, int(sel.size))
                out.append((cls.copy(), co.copy(), np.asarray(ci).copy(), np.asarray(cf).copy(), ho.copy(), np.asarray(hi).copy()))
                engine.free_sites(sid)
            for x, y in zip(*out):
                np.testing.assert_array_equal(x, y)
            v = keep[0].view
            assert int(v.n_pos_esc) > 0  # (windows apart: the escapes are exercised)
    finally:
        pool.free_all()


def test_staged_pass_matches_the_plain_form(engine, load):
    from unfazed_amd.engine import PinnedPool
    ld, P, fid, _ = load
    res, nbytes = [], []
    for compact in (False, True):
        pool = PinnedPool()
        try:
            chunks, st = ld.stage(engine, P, MODE, fid, pool, chunks=3, compact_sites=compact)
            res.append(pipeline.run_pipelined(engine, P, MODE, ld.n, chunks, cnv=False))
            engine.sync()
            nbytes.append(st["site_bytes"])
        finally:
            pool.free_all()
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(res[0][k]), np.asarray(res[1][k]), err_msg=k)
    assert nbytes[1] < nbytes[0]


def test_broken_escape_list_is_refused(engine, load):
    from unfazed_amd.engine import PinnedPool, UnfazedHipError
    ld, P, _, _ = load
    pool = PinnedPool()
    try:
        sel = ld.window_sites(0, 2000, P)
        held, hs, hg, wide, ns = ld.pinned_sites(pool, sel, compact=True)
        v = held.view
        assert int(v.n_pos_esc) > 0
        idx = np.ctypeslib.as_array((C.c_int32 * int(v.n_pos_esc)).from_address(v.pos_esc_idx))
        first = int(idx[0])
        idx[0] = first + 1024  # an escape listed under the span before its own
        with pytest.raises(UnfazedHipError, match="escape"):
            engine.upload_sites_family_async(held, hs["gt"], hg["rd"], hg["ad"], hg["gq"], wide)
        idx[0] = first
    finally:
        pool.free_all()
