"""The hand-built DEFLATE cases of tests/deflatecases.py against the host's inflaters: what makes the table trustworthy without a device.
Every valid case's token expansion is what zlib (and libdeflate, where it loads) inflate its stream to, every refused case is refused by
both, and the table's size is fixed here: no case can drop out unseen."""
import collections
import ctypes
import gzip
import struct
import zlib

import pytest

import deflatecases as dc

N_VALID = {"A": 16, "B": 4, "C": 504 + 512, "D": 20, "E": 1512, "F": 6, "G": 12, "H": 5}
N_REFUSED = {1: 3, 2: 15, 3: 4, 4: 3, 5: 1}


def test_the_table_has_every_case():
    assert dict(collections.Counter(c.family for c in dc.valid())) == N_VALID
    assert dict(collections.Counter(c.code for c in dc.refused())) == N_REFUSED
    names = [c.name for c in dc.valid() + dc.refused()]
    assert len(set(names)) == len(names) == sum(N_VALID.values()) + sum(N_REFUSED.values())
    # family C: every length with every distance from every source by both paths; family E: at least 96 consecutive bit positions around
    # bit 2048 k at whatever alignment the stream's first byte has in its dword, for every copy kind
    assert N_VALID["C"] == sum(len(dc.c_distances(l)) for l in dc.C_LENGTHS) * len(dc.C_SOURCES) * 2 + 256 * 2
    assert dc.E_SPAN[1] - dc.E_SPAN[0] - 24 >= 96 and dc.E_SPAN[0] + 24 < -32 and dc.E_SPAN[1] > 0
    assert N_VALID["E"] == len(dc.E_KINDS) * 2 * (dc.E_SPAN[1] - dc.E_SPAN[0]) + 61 * 8


def test_valid_cases_are_what_zlib_inflates():
    for c in dc.valid():
        assert zlib.decompress(c.stream, -15) == c.payload, c.name
        assert len(c.payload) <= 65536 and len(c.frame) <= 65536, c.name
        assert struct.unpack("<II", c.frame[-8:]) == (zlib.crc32(c.payload) & 0xFFFFFFFF, len(c.payload)), c.name
        assert c.frame[len(c.frame) - 8 - len(c.stream): -8] == c.stream, c.name
    assert gzip.decompress(b"".join(c.frame for c in dc.valid())) == b"".join(c.payload for c in dc.valid())
    for shift in range(4):
        assert len(dc.pad_block(shift)) % 4 == shift and gzip.decompress(dc.pad_block(shift)) == b""


def test_the_cases_reach_what_they_are_named_for():
    """spot checks of the writer itself: the lengths of the codes a case names, the values zlib's compressor never emits"""
    by = {c.name: c for c in dc.valid()}
    assert sorted(dc.ladder(list(range(16))).values()) == list(range(1, 16)) + [15]
    for ds in (0, 3, 4, 29):
        for l in (8, 9, 15):
            assert dc.dist_ladder({ds: l})[ds] == l and sorted(dc.dist_ladder({ds: l}).values()) == list(range(1, 16)) + [15]
    assert all(l >= 9 for s, l in dc.dist_slow([0, 2, 5]).items() if s in (0, 2, 5))
    assert dc.length_token(258, 32768) == (285, 0, 29, 8191)
    assert len(by["B/distances/fast"].payload) > 32768 and len(by["G/largest-stored"].frame) == 65536
    assert dc.unspell([3, (16, 4), (17, 3), (18, 11)]) == [3] * 5 + [0] * 14
    for name in ("G/zlib-sync-flush", "G/zlib-full-flush"):
        assert by[name].stream.count(b"\x00\x00\xff\xff") >= 14, name  # the flush markers: empty stored blocks


def test_the_distance_sweep_holds_every_distance_whose_reciprocal_needs_correcting():
    """the copy loops' k mod dist: q = (int)((float)k * (1.0f / dist)), r = k - q * dist, then one correction either way.  In IEEE single precision
    r >= dist happens at exactly the distances of C_RECIPROCAL for k < 258 (and r < 0 never): the sweep of family C has them all"""
    def f32(x):
        return struct.unpack("f", struct.pack("f", x))[0]
    high = []
    for d in range(2, 258):
        rd = f32(1.0 / d)
        r = [k - int(f32(k * rd)) * d for k in range(258)]
        assert min(r) >= 0 and max(r) < 2 * d
        if max(r) >= d:
            high.append(d)
    assert tuple(high) == dc.C_RECIPROCAL
    names = {c.name for c in dc.valid()}
    assert all("C/sweep/dist%d/%s" % (d, p) in names for d in range(2, 258) for p in ("fast", "slow"))


def test_refused_cases_are_refused_by_zlib():
    for c in dc.refused():
        if c.level == "stream":
            with pytest.raises(zlib.error):
                zlib.decompress(c.stream, -15)
        else:  # the stream is a valid one of another size than the frame declares
            assert c.level == "frame" and len(zlib.decompress(c.stream, -15)) != c.isize, c.name
        with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
            gzip.decompress(c.frame)
        assert struct.unpack("<I", c.frame[-4:])[0] == c.isize, c.name


@pytest.fixture(scope="module")
def libdeflate():
    try:
        L = ctypes.CDLL("libdeflate.so.0")
    except OSError as e:
        print("libdeflate.so.0 does not load (%s): its half of the host checks is skipped, zlib's half has run" % e)
        pytest.skip("libdeflate.so.0 does not load")
    L.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
    L.libdeflate_deflate_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]
    L.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
    d = ctypes.c_void_p(L.libdeflate_alloc_decompressor())

    def inflate(stream, isize):
        """-> (libdeflate's result, the bytes it wrote) into a buffer of the size the frame declares: the host route's call (io_common.hpp)"""
        out, got = ctypes.create_string_buffer(max(1, isize)), ctypes.c_size_t(0)
        rc = L.libdeflate_deflate_decompress(d, stream, len(stream), out, isize, ctypes.byref(got))
        return rc, out.raw[: got.value]
    yield inflate
    L.libdeflate_free_decompressor(d)


def test_valid_cases_are_what_libdeflate_inflates(libdeflate):
    for c in dc.valid():
        assert libdeflate(c.stream, c.isize) == (0, c.payload), c.name


def test_refused_cases_are_refused_by_libdeflate(libdeflate):
    for c in dc.refused():
        rc, got = libdeflate(c.stream, c.isize)
        if c.name in dc.ZLIB_ONLY:  # (nothing asserted: releases of libdeflate differ here)
            print("%s: libdeflate returns %d with %d bytes -- %s" % (c.name, rc, len(got), dc.ZLIB_ONLY[c.name]))
            continue
        assert rc != 0 or len(got) != c.isize, c.name  # (the host route's test: a result other than 0, or another size than declared)
