"""The heads of alignment files on the device (uz_head_walk / uz_head_rank through HipEngine.head_ranks; read_collector.py:11-25): the tlen
column of a file's first records against the writer's list and against the host's own head (BamSource.tlen_head), continuation over rounds,
many files in one call and in groups, the two order statistics against numpy.sort, and the files the device hands back to the host route."""
import os
import shutil

import numpy as np
import pytest

from headfiles import COLUMN_KINDS, column, read_blocks, write_head_bam
from unfazed_amd.hostpath import head_rank_index
from unfazed_amd.io_native import BamSource, IoError

pytestmark = pytest.mark.gpu


def _tlens(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    t = rng.integers(-2000, 2000, n)
    if n:
        t[rng.integers(0, n)] = -(1 << 31)
        t[rng.integers(0, n)] = (1 << 31) - 1
    return t.tolist()


def _ranks(col, readlen):
    keys = np.sort(np.abs(np.asarray(col, np.int64) - 2 * readlen))
    k = head_rank_index(keys.size)
    return keys.size, int(keys[k]), int(keys[min(k + 1, keys.size - 1)])


@pytest.mark.parametrize("payload", [60000, 700])
@pytest.mark.parametrize("R", [0, 1, 2, 200, 201, 5000])
def test_tlen_column(engine, tmp_path, R, payload):
    p = str(tmp_path / "a.bam")
    t = _tlens(R)
    info = write_head_bam(p, t, payload=payload)
    if payload == 700:
        assert info["header"] % payload != 0  # the header ends mid-block
    for want in sorted({1, 2, R - 1, R, R + 1, R + 5}):
        if want <= 0:
            continue
        (r,), (col,) = engine.head_ranks([p], want, 150, fetch=True)
        host = BamSource(p, insert_size_max_sample=want - 1).tlen_head
        assert host.tolist() == t[:want]
        if R == 0:
            assert r is None and col is None
            continue
        assert col.dtype == np.int32 and col.tolist() == t[:want], (R, payload, want)
        assert r == _ranks(t[:want], 150), (R, payload, want)


@pytest.mark.parametrize("where", ["boundary", "size_field", "body"])
def test_continuation(engine, tmp_path, monkeypatch, where):
    p = str(tmp_path / "a.bam")
    t = _tlens(200)
    info = write_head_bam(p, t)
    cut = info["rec_off"][50] + {"boundary": 0, "size_field": 2, "body": 20}[where]
    write_head_bam(p, t, cuts=[cut])
    assert int(np.cumsum(read_blocks(p)["isize"])[0]) == cut
    monkeypatch.setenv("UZ_HEAD_FIRST_BYTES", "1")  # round 1: the first block alone
    stats = {}
    (r,), (col,) = engine.head_ranks([p], 180, 100, stats=stats, fetch=True)
    assert col.tolist() == t[:180] and r == _ranks(t[:180], 100)
    assert stats["cutoff_walk_calls"] >= 2
    # many rounds: 700-byte blocks, one block in round 1, the estimate from there on
    q = str(tmp_path / "b.bam")
    write_head_bam(q, t, payload=700)
    stats = {}
    (r,), (col,) = engine.head_ranks([q], 200, 100, stats=stats, fetch=True)
    assert col.tolist() == t and 2 <= stats["cutoff_walk_calls"] <= 8


def test_many_files_in_one_call_and_in_groups(engine, tmp_path, monkeypatch):
    want = 150
    counts = [1000, 0, 3, 900, 50, 800]
    paths, cols, totals = [], [], []
    for i, n in enumerate(counts):
        p = str(tmp_path / ("f%d.bam" % i))
        t = _tlens(n, seed=i)
        totals.append(write_head_bam(p, t, payload=60000 if i % 2 else 3000)["total"])
        paths.append(p)
        cols.append(t[:want])
    twin = str(tmp_path / "twin.bam")
    shutil.copy(paths[3], twin)
    shutil.copy(paths[3] + ".bai", twin + ".bai")
    one_by_one = [engine.head_ranks([p], want, 150, fetch=True) for p in paths]
    stats = {}
    got, gcols = engine.head_ranks(paths + [twin], want, 150, stats=stats, fetch=True)
    assert stats["cutoff_walk_calls"] == 1
    for i, n in enumerate(counts):
        assert got[i] == one_by_one[i][0][0] and (got[i] is None) == (n == 0)
        if n:
            assert gcols[i].tolist() == cols[i] == one_by_one[i][1][0].tolist() and got[i] == _ranks(cols[i], 150)
    assert got[6] == got[3] and gcols[6].tolist() == cols[3]  # byte-identical copies under two names: two answers
    # the same files cut into three groups: a limit that the greedy cut turns into exactly three launches (every file fits one)
    limit = None
    for cand in range(max(totals), sum(totals) + 1, 64):
        groups, cur = 1, 0
        for s in totals:
            if cur and cur + s > cand:
                groups, cur = groups + 1, 0
            cur += s
        if groups == 3:
            limit = cand
            break
    assert limit is not None
    monkeypatch.setenv("UZ_HEAD_MAX_BYTES", str(limit))
    stats = {}
    got3, cols3 = engine.head_ranks(paths, want, 150, stats=stats, fetch=True)
    assert stats["cutoff_walk_calls"] == 3
    assert got3 == got[:6]
    for a, b in zip(cols3, gcols[:6]):
        assert (a is None and b is None) or a.tolist() == b.tolist()
    # a single file larger than the limit is a group of its own, cut by rounds
    monkeypatch.setenv("UZ_HEAD_MAX_BYTES", "20000")
    stats = {}
    (r,), (c,) = engine.head_ranks([paths[0]], 900, 150, stats=stats, fetch=True)
    assert c.tolist() == _tlens(1000, seed=0)[:900] and 2 <= stats["cutoff_walk_calls"] <= 8


@pytest.mark.parametrize("readlen", [0, 100, 150])
def test_ranks(engine, tmp_path, readlen):
    paths, colsw = [], []
    for n in (1, 2, 3, 201, 202, 5000):
        for kind in COLUMN_KINDS:
            p = str(tmp_path / ("%s_%d.bam" % (kind, n)))
            c = column(kind, n)
            write_head_bam(p, c.tolist())
            paths.append(p)
            colsw.append(c)
    got = engine.head_ranks(paths, 6000, readlen)
    for p, c, g in zip(paths, colsw, got):
        assert g == _ranks(c, readlen), (os.path.basename(p), readlen, g)
    # a head shorter than the file: the ranks are those of the first `want` records
    got = engine.head_ranks(paths[-6:], 777, readlen)
    for c, g in zip(colsw[-6:], got):
        assert g == _ranks(c[:777], readlen)


def _light_host(engine, cap):
    """a PhasingHost with what kid_cutoff and prepare_cutoffs read, and nothing else (no sites table)"""
    from unfazed_amd import session
    from unfazed_amd.hostpath import PhasingHost, _Stats
    h = PhasingHost.__new__(PhasingHost)
    h.backend, h.cutoffs, h.stats, h._indexed_memo = engine, {}, _Stats(), None
    h.reads_by_bam = session._LazyReads(cap)
    return h


def _cutoff_by(engine, route, bam, cap, monkeypatch):
    from unfazed_amd import hostpath
    monkeypatch.setenv("UZ_CUTOFF_ROUTE", route)
    hostpath._CUTOFF_RANKS.clear()
    h = _light_host(engine, cap)
    try:
        h.prepare_cutoffs([("kid", bam)], 150, 3, cap)
        v = h.kid_cutoff("kid", bam, 150, 3, cap)
        return ("value", np.float64(v).tobytes(), type(v)), h.stats
    except Exception as e:  # noqa: BLE001 -- the comparison is of whatever the route raises
        return ("raises", type(e), str(e)), h.stats


@pytest.mark.parametrize("how", ["block_size_16", "crc", "truncated", "good"])
def test_handed_back(engine, tmp_path, monkeypatch, how):
    p = str(tmp_path / (how + ".bam"))
    t = _tlens(600)
    write_head_bam(p, t, payload=3000, level=0 if how == "crc" else 6, bad_size_at=300 if how == "block_size_16" else None)
    blocks = read_blocks(p)
    raw = bytearray(open(p, "rb").read())
    if how == "crc":  # one payload byte of a stored block: its structure stands, its checksum does not
        raw[int(blocks["data"][4]) + 5 + 100] ^= 0x40
    if how == "truncated":  # inside a block of the head
        raw = raw[: int(blocks["off"][6]) + 30]
    open(p, "wb").write(bytes(raw))
    got = engine.head_ranks([p], 500, 150)
    assert (got[0] is None) == (how != "good")
    host, sh = _cutoff_by(engine, "host", p, 499, monkeypatch)
    dev, sd = _cutoff_by(engine, "device", p, 499, monkeypatch)
    assert dev == host
    assert host[0] == ("value" if how == "good" else "raises")
    if how != "good":
        assert issubclass(host[1], IoError)
    assert sh["cutoff_device_files"] == 0 and sh["cutoff_walk_calls"] == 0 and sh["cutoff_host_files"] == 0
    assert sd["cutoff_device_files"] == (1 if how == "good" else 0) and sd["cutoff_host_files"] == (0 if how == "good" else 1)


def test_no_record_at_all_is_the_host_routes_business(engine, tmp_path, monkeypatch):
    p = str(tmp_path / "empty.bam")
    write_head_bam(p, [])
    host, _ = _cutoff_by(engine, "host", p, 100, monkeypatch)
    dev, _ = _cutoff_by(engine, "device", p, 100, monkeypatch)
    assert dev == host and host[0] == "raises" and host[1] is IndexError
    q = str(tmp_path / "few.bam")
    write_head_bam(q, _tlens(5))
    for cap in (-1, -5):  # want <= 0
        assert _cutoff_by(engine, "device", q, cap, monkeypatch)[0] == _cutoff_by(engine, "host", q, cap, monkeypatch)[0]
