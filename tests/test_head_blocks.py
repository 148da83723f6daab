"""Where a file's head lies (include/unfazed_io.h: uz_bamsrc_first_voff, uz_bamsrc_list_blocks, uz_bamsrc_gather_ranges) against a Python reader
of the same file: the first record's virtual offset for a header shorter than a block and for one longer than two blocks, the block table, the
three ways the listing stops, and the two refusals."""
import os

import numpy as np
import pytest

from headfiles import read_blocks, write_head_bam
from unfazed_amd.io_native import BamSource, IoError

COLS = ("off", "csize", "isize", "crc", "data")
UZ_IO_E_FORMAT = -2  # unfazed_io.h


def _voff(blocks, u):
    """virtual offset of inflated offset u (the end of a block is the start of the next)"""
    at = np.concatenate([[0], np.cumsum(blocks["isize"].astype(np.int64))])
    k = int(np.searchsorted(at, u, side="right")) - 1
    while k + 1 < blocks["off"].size and u - at[k] >= blocks["isize"][k]:
        k += 1
    return (int(blocks["off"][k]) << 16) | int(u - at[k])


@pytest.mark.parametrize("payload,n_sq", [(60000, 2), (700, 2), (700, 120), (700, 0)])
def test_first_record_offset(tmp_path, payload, n_sq):
    p = str(tmp_path / "a.bam")
    info = write_head_bam(p, list(range(300)), payload=payload, n_sq=n_sq)
    if n_sq == 120:
        assert info["header"] > 2 * payload
    blocks = read_blocks(p)
    src = BamSource(p, insert_size_max_sample=-1)
    assert src.tlen_head.size == 0 and src.first_voff.size == 1
    assert int(src.first_voff[0]) == _voff(blocks, info["header"])
    # a source that read its head knows the same place
    assert int(BamSource(p, insert_size_max_sample=10).first_voff[0]) == int(src.first_voff[0])


def test_header_that_ends_with_its_block_and_a_file_without_records(tmp_path):
    p = str(tmp_path / "b.bam")
    info = write_head_bam(p, [5, 6, 7])
    info = write_head_bam(p, [5, 6, 7], cuts=[info["header"]])  # a block ends where the header does
    blocks = read_blocks(p)
    assert blocks["isize"][0] == info["header"]
    src = BamSource(p, insert_size_max_sample=-1)
    assert int(src.first_voff[0]) == int(blocks["off"][1]) << 16
    q = str(tmp_path / "c.bam")
    write_head_bam(q, [])
    e = BamSource(q, insert_size_max_sample=-1)
    b = read_blocks(q)
    assert int(e.first_voff[0]) == int(b["off"][1]) << 16  # the EOF block's start: the header filled its block
    got = e.list_blocks(int(e.first_voff[0]) >> 16, 1 << 20)
    assert got["at_end"] and got["isize"].tolist() == [0]  # the empty EOF block is listed like any other


def test_the_table_and_where_the_listing_stops(tmp_path):
    p = str(tmp_path / "a.bam")
    write_head_bam(p, list(range(2000)), payload=700)
    blocks = read_blocks(p)
    n = blocks["off"].size
    assert n > 100 and blocks["isize"][-1] == 0
    src = BamSource(p, insert_size_max_sample=-1)
    # the file's end
    got = src.list_blocks(0, 1 << 40)
    assert got["at_end"]
    for c in COLS:
        assert got[c].dtype == blocks[c].dtype and np.array_equal(got[c], blocks[c]), c
    # the wanted bytes: the first block with which the ISIZE sum reaches them, from any block on
    cum = np.cumsum(blocks["isize"].astype(np.int64))
    for k0, want in ((0, 1), (0, 700), (0, 701), (3, 5000), (n - 2, 1)):
        got = src.list_blocks(int(blocks["off"][k0]), want)
        base = int(cum[k0 - 1]) if k0 else 0
        k1 = min(int(np.searchsorted(cum - base, want, side="left")), n - 1)
        assert got["off"].tolist() == blocks["off"][k0: k1 + 1].tolist(), (k0, want)
        assert not got["at_end"]
    # the capacity (the raw export: BamSource.list_blocks asks again until the bytes are there)
    import ctypes as C
    cols = [np.zeros(4, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint32), np.zeros(4, np.int64)]
    m, end = C.c_int64(0), C.c_int(0)
    assert src.lib.uz_bamsrc_list_blocks(src._h.ptr, 0, 1 << 40, 4, *[c.ctypes.data for c in cols], C.byref(m), C.byref(end)) == 0
    assert m.value == 4 and end.value == 0 and cols[0].tolist() == blocks["off"][:4].tolist()
    assert src.list_blocks(0, 1 << 40, cap=3)["off"].tolist() == blocks["off"].tolist()
    # the end itself
    got = src.list_blocks(os.path.getsize(p), 1)
    assert got["at_end"] and got["off"].size == 0


def test_refusals(tmp_path):
    p = str(tmp_path / "a.bam")
    write_head_bam(p, list(range(500)), payload=700)
    blocks = read_blocks(p)
    raw = bytearray(open(p, "rb").read())
    k = 5
    src = BamSource(p, insert_size_max_sample=-1)
    # a block that runs beyond the file's end: the file cut inside block k (the source maps the file: a fresh name, a fresh source)
    q = str(tmp_path / "cut.bam")
    open(q, "wb").write(bytes(raw[: int(blocks["off"][k]) + 40]))
    open(q + ".bai", "wb").write(open(p + ".bai", "rb").read())
    cut = BamSource(q, insert_size_max_sample=-1)
    with pytest.raises(IoError) as e:
        cut.list_blocks(0, 1 << 40)
    assert e.value.code == UZ_IO_E_FORMAT and "truncated" in str(e.value)
    assert cut.list_blocks(0, 1000)["off"].tolist() == blocks["off"][:2].tolist()  # (the blocks before it are listed)
    # a header that is not a BGZF header
    bad = bytearray(raw)
    bad[int(blocks["off"][k]) + 1] = 0x8c
    r = str(tmp_path / "bad.bam")
    open(r, "wb").write(bytes(bad))
    open(r + ".bai", "wb").write(open(p + ".bai", "rb").read())
    with pytest.raises(IoError) as e:
        BamSource(r, insert_size_max_sample=-1).list_blocks(0, 1 << 40)
    assert e.value.code == UZ_IO_E_FORMAT and "not a BGZF block" in str(e.value)
    # fewer than a header's bytes behind the last block
    s = str(tmp_path / "tail.bam")
    open(s, "wb").write(bytes(raw) + b"\x1f\x8b\x08")
    open(s + ".bai", "wb").write(open(p + ".bai", "rb").read())
    with pytest.raises(IoError):
        BamSource(s, insert_size_max_sample=-1).list_blocks(int(blocks["off"][-1]), 1 << 20)


def test_gather_ranges(tmp_path):
    srcs, raws = [], []
    for i in range(5):
        p = str(tmp_path / ("g%d.bam" % i))
        write_head_bam(p, list(range(100 * i + 1)), payload=900)
        srcs.append(BamSource(p, insert_size_max_sample=-1))
        raws.append(open(p, "rb").read())
    src_off = [0, 10, 28, 0, 5]
    nbytes = [len(r) - o for r, o in zip(raws, src_off)]
    nbytes[3] = 0
    dst_off = np.concatenate([[0], np.cumsum(nbytes)])[:-1] + 3
    dst = np.full(sum(nbytes) + 8, 0xEE, np.uint8)
    BamSource.gather_ranges(srcs, src_off, nbytes, dst_off, dst, threads=4)
    for r, o, n, d in zip(raws, src_off, nbytes, dst_off):
        assert bytes(dst[d: d + n]) == r[o: o + n]
    assert dst[:3].tolist() == [0xEE] * 3 and dst[-5:].tolist() == [0xEE] * 5
    with pytest.raises(IoError):  # a range beyond its file
        BamSource.gather_ranges(srcs[:1], [0], [len(raws[0]) + 1], [0], np.zeros(len(raws[0]) + 64, np.uint8))
    with pytest.raises(IoError):  # ... beyond the buffer
        BamSource.gather_ranges(srcs[:1], [0], [len(raws[0])], [0], np.zeros(16, np.uint8))
