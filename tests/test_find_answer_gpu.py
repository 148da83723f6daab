"""uz_find_answer (engine.find(..., transient=True): the whole answer of a find in one page-locked block, one kernel behind the fill pass, one
wait of the host) and the one-launch scan of the two count arrays (k_scan2_tile), held EXACTLY to the C oracle on the hand-built window
tables of tests/sitecases.py.  Every comparison is np.array_equal; there are no tolerances.  uz_find_stats gives the waits, the launches and
the fall-back bits of the last find."""
import os

import numpy as np
import pytest

import sitecases
from unfazed_amd import abi

pytestmark = pytest.mark.gpu
LISTS = ("cand_off", "cand_idx", "cand_flags", "het_off", "het_idx")
T = 2048  # UZ_SCAN2_TILE (csrc/k_sites.hip)
GREW, BLOCK_SMALL = 1, 2  # UZ_FA_* (unfazed_hip.h)
ONE_MAX = 16 * T  # UZ_SCAN2_ONE_MAX: larger batches take the two-launch scan in tiles of 4 096
SIZES = (1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 4095, 4096, ONE_MAX - 1, ONE_MAX, ONE_MAX + 1)  # (2 T + 1 is 4097)


def _assert_lists(want, got, what):
    for name, a, b in zip(LISTS, want, got):
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs" % (what, name)


def _batch(size):
    """sitecases.batch_dnms for the new tile: the world's DNMs repeated to `size`, zero-count DNMs (no such contig) on both sides of every
    tile edge and at the end"""
    _, _, dn = sitecases.window_world()
    rows = [dn.rows[d % len(dn.rows)] for d in range(size)]
    for d in range(size):
        if (d > 0 and d % T in (0, T - 1)) or d == 2 or (size > 5 and d == size - 1):  # (every edge of the 4 096-count tile is one of these too)
            rows[d] = (-1,) + rows[d][1:]
    return dn.arrays(rows=rows)


@pytest.fixture(scope="module")
def families(engine):
    out = {}
    for mixed in (False, True):
        t = sitecases.window_table(mixed)
        sid = engine.upload_sites(t)
        out[mixed] = (t, sid, engine.add_family(sid, *t.family_columns()))
    yield out
    for t, sid, fid in out.values():
        engine.free_sites(sid)


def _want(t, P, dv, mode):
    from oracle import oracle as orc
    return orc.find(P, t.sites_view(), t.family_view(), dv, mode)


def _warm(engine, fid, dv, P, mode, want, what):
    """The library keeps the lists of the last three finds and the engine three page-locked blocks, each set in its turn: a warmed engine is
    one whose three sets have all held a batch of this size.  Every answer on the way is held to the oracle too."""
    for k in range(3):
        _assert_lists(want, engine.find(fid, dv, P, mode, transient=True), "%s, find %d" % (what, k))


def _one_wait(engine, what):
    waits, launches, code, _ = engine.find_stats()
    assert (waits, code) == (1, 0) and launches <= 6, "%s: %d waits, %d launches, fall-back bits %d" % (what, waits, launches, code)


@pytest.mark.parametrize("sd,mode", sitecases.WINDOW_RUNS)
def test_windows(engine, families, sd, mode):
    t, sid, fid = families[bool(mode & abi.FIND_WHOLE_REGION)]
    dv = sitecases.dnms_view(sitecases.window_dnms(mode))
    P = abi.make_params(search_dist=sd)
    want = _want(t, P, dv, mode)
    _warm(engine, fid, dv, P, mode, want, "sd %d mode %d" % (sd, mode))
    _assert_lists(want, engine.find(fid, dv, P, mode, transient=True), "sd %d mode %d, warmed" % (sd, mode))
    _one_wait(engine, "sd %d mode %d" % (sd, mode))


@pytest.mark.parametrize("size", SIZES)
def test_batch_sizes_across_scan_tiles(engine, families, size):
    t, sid, fid = families[False]
    dv = sitecases.dnms_view(_batch(size))
    P = abi.make_params(search_dist=5)
    want = _want(t, P, dv, abi.FIND_SECOND_WINDOW)
    if size > 3:
        assert want[0][size - 1] == want[0][size]  # (the last DNM has no such contig: its count is zero)
    _warm(engine, fid, dv, P, abi.FIND_SECOND_WINDOW, want, "batch of %d" % size)
    _assert_lists(want, engine.find(fid, dv, P, abi.FIND_SECOND_WINDOW, transient=True), "batch of %d, warmed" % size)
    _one_wait(engine, "batch of %d" % size)


def test_lists_without_room(engine, families):
    """UZ_TEST_FIND_CAP (the room the first fill pass may use): 1, exactly one DNM's end offset, one less, the het total; each followed by a
    smaller batch on the same engine, which is back on the one-wait path"""
    t, sid, fid = families[False]
    dv = sitecases.dnms_view(sitecases.window_dnms(0))
    dvs = sitecases.dnms_view(sitecases.batch_dnms(50))
    P = abi.make_params(search_dist=5000)
    mode = abi.FIND_SECOND_WINDOW
    want, want_small = _want(t, P, dv, mode), _want(t, P, dvs, mode)
    _warm(engine, fid, dv, P, mode, want, "warm-up")
    d = (len(want[3]) - 1) // 3
    edge = int(want[3][d + 1])
    assert 1 < edge - 1 and edge < int(want[3][-1]) and want[3][d + 1] > want[3][d]
    for cap in (1, edge, edge - 1, int(want[3][-1])):
        outgrown = int(want[0][-1]) > cap or int(want[3][-1]) > cap
        assert outgrown or cap == int(want[3][-1])
        os.environ["UZ_TEST_FIND_CAP"] = str(cap)
        try:
            engine.drop_derived()
            _assert_lists(want, engine.find(fid, dv, P, mode, transient=True), "room %d" % cap)
            waits, launches, code, _ = engine.find_stats()
        finally:
            os.environ.pop("UZ_TEST_FIND_CAP", None)
        if outgrown:
            assert code & GREW and waits == 2, "room %d: %d waits, fall-back bits %d" % (cap, waits, code)
        else:
            assert (waits, code) == (1, 0)
        _assert_lists(want_small, engine.find(fid, dvs, P, mode, transient=True), "smaller batch behind room %d" % cap)
        _one_wait(engine, "smaller batch behind room %d" % cap)


def test_block_one_byte_short_of_each_part(engine, families):
    t, sid, fid = families[False]
    dv = sitecases.dnms_view(sitecases.window_dnms(0))
    dvs = sitecases.dnms_view(sitecases.batch_dnms(50))
    P = abi.make_params(search_dist=5000)
    mode = abi.FIND_SECOND_WINDOW
    want, want_small = _want(t, P, dv, mode), _want(t, P, dvs, mode)
    n = len(want[0]) - 1
    off, total = engine.find_answer_layout(n, int(want[0][-1]), int(want[3][-1]))
    ends = off[1:] + [total]
    assert all(o % 256 == 0 for o in ends) and len(set(ends)) == 6
    _warm(engine, fid, dv, P, mode, want, "warm-up")  # (every set of lists in HBM has the room of this batch)
    for k, end in enumerate(ends):
        got = engine._find_answer(fid, dv, mode, block_bytes=end - 1)
        _assert_lists(want, got, "block one byte short of part %d" % k)
        waits, launches, code, need = engine.find_stats()
        assert code == BLOCK_SMALL and waits == 2 and need == total, "part %d: %d waits, fall-back bits %d, %d bytes" % (k, waits, code, need)
        _assert_lists(want_small, engine.find(fid, dvs, P, mode, transient=True), "smaller batch behind a block short of part %d" % k)
        _one_wait(engine, "smaller batch behind a block short of part %d" % k)
    got = engine._find_answer(fid, dv, mode, block_bytes=total)  # exactly its size
    _assert_lists(want, got, "block of exactly the answer's size")
    _one_wait(engine, "block of exactly the answer's size")


def test_four_finds_in_a_row(engine, families):
    """the three pinned sets in turn, a larger answer before a smaller one in every set: nothing of an earlier answer shows through"""
    t, sid, fid = families[False]
    P = abi.make_params(search_dist=5000)
    mode = abi.FIND_SECOND_WINDOW
    for rep in range(2):
        for size in (T + 1, 50, 7, 300, 3, 1):
            dv = sitecases.dnms_view(_batch(size))
            _assert_lists(_want(t, P, dv, mode), engine.find(fid, dv, P, mode, transient=True), "batch of %d, round %d" % (size, rep))


def test_old_pair_gives_the_same_arrays(engine, families):
    t, sid, fid = families[False]
    dv = sitecases.dnms_view(sitecases.window_dnms(0))
    P = abi.make_params(search_dist=500)
    old = engine.find(fid, dv, P, 0)  # uz_find + uz_find_fetch into pageable memory
    waits, launches, code, _ = engine.find_stats()
    assert waits == 2 and code == 0
    new = engine.find(fid, dv, P, 0, transient=True)
    _assert_lists(old, new, "uz_find + uz_find_fetch against uz_find_answer")
    _assert_lists(_want(t, P, dv, 0), new, "uz_find_answer")
