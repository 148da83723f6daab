"""Alignment files for the tests of the head route (the insert cutoff's input: the first records of a BAM, read_collector.py:11-25): a BAM writer
whose template lengths, BGZF block cuts and compression level are the caller's, a Python reader of a file's BGZF blocks, and the ways a head can
be broken."""
import struct
import zlib

import numpy as np


def bgzf_block(data: bytes, level: int = 6) -> bytes:
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = comp.compress(data) + comp.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25)
            + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def record(i: int, tlen: int, block_size=None) -> bytes:
    """record i: mapped on contig i % 2 at an ascending position, every seventh unmapped (refID -1); name, CIGAR and bases vary with i so that no
    two neighbours have one size"""
    unmapped = i % 7 == 3
    name = ("r%d" % i).encode() + b"x" * (i % 13) + b"\0"
    l_seq = i % 23
    cig = [] if unmapped else [(l_seq or 1) << 4]
    body = struct.pack("<iiBBHHHiiii", -1 if unmapped else i % 2, -1 if unmapped else 100 + 3 * i, len(name), 30, 4680, len(cig), 4 if unmapped else 0,
                       l_seq, -1, -1, int(tlen)) + name + b"".join(struct.pack("<I", c) for c in cig) + b"\x11" * ((l_seq + 1) // 2) + b"\x20" * l_seq
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def write_head_bam(path, tlens, payload: int = 60000, n_sq: int = 2, cuts=None, level: int = 6, bad_size_at=None):
    """-> dict(rec_off: where every record starts in the inflated stream, header: the header's bytes, total: the stream's).  payload: inflated
    bytes per BGZF block; cuts: further offsets of the stream at which a block ends; n_sq: @SQ lines (contigs) -- many make a header longer than
    a block; bad_size_at: that record declares a block_size of 16.  An empty index goes beside the file (no fetch is made on these files)."""
    contigs = [("c%d" % k, 1 << 28) for k in range(n_sq)]
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    out = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs)))
    for name, length in contigs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    header = len(out)
    rec_off = []
    for i, t in enumerate(tlens):
        rec_off.append(len(out))
        out += record(i, t, 16 if bad_size_at == i else None)
    ends = sorted(set(list(range(payload, len(out), payload)) + [c for c in (cuts or []) if 0 < c < len(out)] + [len(out)]))
    with open(path, "wb") as fh:
        at = 0
        for e in ends:
            fh.write(bgzf_block(bytes(out[at:e]), level))
            at = e
        fh.write(bgzf_block(b""))
    with open(str(path) + ".bai", "wb") as fh:
        fh.write(b"BAI\x01" + struct.pack("<i", n_sq) + struct.pack("<ii", 0, 0) * n_sq)
    return dict(rec_off=rec_off, header=header, total=len(out))


def read_blocks(path):
    """the BGZF blocks of a file, read with struct and zlib: off, csize, isize, crc, data (where the DEFLATE stream starts) per block"""
    raw = open(path, "rb").read()
    rows, p = [], 0
    while p < len(raw):
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        assert len(zlib.decompress(raw[p + 12 + xlen: p + bsize - 8], -15)) == isize
        rows.append((p, bsize, isize, crc, p + 12 + xlen))
        p += bsize
    cols = list(zip(*rows)) if rows else [[]] * 5
    return dict(off=np.array(cols[0], np.int64), csize=np.array(cols[1], np.int32), isize=np.array(cols[2], np.int32), crc=np.array(cols[3], np.uint32),
                data=np.array(cols[4], np.int64))


def column(kind: str, n: int, seed: int = 5) -> np.ndarray:
    """template-length columns for the rank tests"""
    rng = np.random.default_rng(seed + n)
    lo, hi = -(1 << 31), (1 << 31) - 1
    if kind == "equal":
        return np.full(n, 417, np.int64)
    if kind == "two":
        return rng.choice(np.array([250, 9000]), n)
    if kind == "ascending":
        return np.arange(n, dtype=np.int64) * 7 - 300
    if kind == "descending":
        return (np.arange(n, dtype=np.int64) * 7 - 300)[::-1].copy()
    if kind == "random":
        return rng.integers(lo, hi + 1, n)
    if kind == "extremes":
        return rng.choice(np.array([lo, hi, 0]), n)
    raise ValueError(kind)


COLUMN_KINDS = ("equal", "two", "ascending", "descending", "random", "extremes")
