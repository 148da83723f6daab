"""The sliced staging of gathered BGZF blocks (csrc/bgzf_batch.hpp states the rules, uz_queue_inflate of csrc/k_inflate.hip runs them) past its
first slice: a batch is cut after 8192 blocks while at least 4096 remain, the slices alternate between two streams, and a refused block is
reported by its number in the BATCH (the slice's first block + the number the kernel saw).  20 480 tiny blocks -- three slices, the third on
the first stream again -- each holding its own index, so a slice that landed in another's place shows; on the staged route
(uz_bgzf_inflate_to_host), the one-launch route (uz_bgzf_inflate) and the walk (uz_bam_walk with a plan of no tasks: the blocks only)."""
import functools
import struct

import numpy as np
import pytest

import deflatecases as dc
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu

N = 20480


@functools.lru_cache(maxsize=None)
def frames():
    return tuple(dc.bgzf_block(struct.pack("<I", k), 1) for k in range(N))


@functools.lru_cache(maxsize=None)
def bad_case():
    return next(c for c in dc.refused() if c.name == "R/dist-two-2-bit-codes")


def batch(n, bad=()):
    """the first n frames laid end to end, the refused frame in the place of every index in `bad` -> the tables of the staged route and the walk"""
    c = bad_case()
    fr = [c.frame if k in bad else f for k, f in enumerate(frames()[:n])]
    sizes = [c.isize if k in bad else 4 for k in range(n)]
    coff = np.concatenate([[0], np.cumsum([len(f) for f in fr])]).astype(np.int64)
    comp = np.frombuffer(b"".join(fr), np.uint8)
    assert all(f[10:12] == b"\x06\x00" for f in (c.frame, fr[0]))  # (18 bytes of framing in front of the stream)
    crc = np.asarray([struct.unpack("<I", f[-8:-4])[0] for f in fr], np.uint32)
    return dict(comp=comp, comp_bytes=int(comp.size), n_blocks=n, in_off=coff[:-1] + 18, out_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                blk_coff=np.ascontiguousarray(coff[:-1]), blk_crc=crc)


def want_bytes(n):
    return np.arange(n, dtype="<u4").view(np.uint8)


def staged(engine, b):
    out = np.full(max(1, int(b["out_off"][-1])), 0xEE, np.uint8)
    engine.inflate_blocks(b["comp"], b["comp_bytes"], b["in_off"], b["out_off"], out)
    return out[: int(b["out_off"][-1])]


@pytest.mark.parametrize("n", [12287, 12288, 20480])
def test_staged_route_one_two_and_three_slices(engine, n):
    assert np.array_equal(staged(engine, batch(n)), want_bytes(n))


@pytest.mark.parametrize("k", [8191, 8192, 20479])
def test_staged_route_names_the_block_of_the_batch(engine, k):
    """the last block of the first slice, the first of the second, the last of the third"""
    with pytest.raises(UnfazedHipError) as e:
        staged(engine, batch(N, (k,)))
    assert "block %d of the batch" % k in str(e.value) and "(code %d)" % bad_case().code in str(e.value), str(e.value)
    assert np.array_equal(staged(engine, batch(N)), want_bytes(N))


def test_staged_route_names_the_lower_of_two_slices(engine):
    with pytest.raises(UnfazedHipError) as e:
        staged(engine, batch(N, (8192, 16384)))
    assert "block 8192 of the batch" in str(e.value), str(e.value)


def test_one_launch_route(engine):
    got, nb, _ = engine.bgzf_inflate(b"".join(frames()[:12288]))
    assert nb == 12288 and np.array_equal(got, want_bytes(12288))


def walk_plan(b):
    return dict(b, task=np.zeros((0, 10), np.int32), span=np.zeros((0, 6), np.int64), reach=np.zeros((0, 2), np.int32), fetch=np.zeros((0, 3), np.int32))


def good_walk(engine):
    wid, _ = engine.walk(walk_plan(batch(N)))
    assert wid >= 0
    engine.bam_walk_release(wid)


def test_walk_route_three_slices(engine):
    good_walk(engine)


def test_walk_route_names_a_crc_mismatch_in_the_second_slice(engine):
    p = walk_plan(batch(N))
    p["blk_crc"] = p["blk_crc"].copy()
    p["blk_crc"][8192] ^= 1
    with pytest.raises(UnfazedHipError) as e:
        engine.walk(p)
    assert "CRC mismatch in BGZF block 8192 of the batch (file offset %d)" % int(p["blk_coff"][8192]) in str(e.value), str(e.value)
    good_walk(engine)  # (the slot was given back)


def test_walk_route_names_a_refused_block_in_the_third_slice(engine):
    with pytest.raises(UnfazedHipError) as e:
        engine.walk(walk_plan(batch(N, (16384,))))
    assert "BGZF block 16384 of the batch" in str(e.value), str(e.value)
    good_walk(engine)
