"""The compact link form of a site table (uz_types.h: uz_sites_view.pos_d16 ...): uz_sites_pack and its host twin uz_sites_unpack, which
computes what the device's expansion (k_sites_expand) writes.  No GPU.  (The twin and the device are both held to a model written from the
header: tests/test_site_form_model.py on the CPU, tests/test_site_forms_gpu.py on the device.)"""
import numpy as np
import pytest

from unfazed_amd import abi, io_native

SPAN, LIMIT = 1024, 1 << 15


def plain_view(pos, contig_off, sflags=None, ref=None, alt=None):
    n = len(pos)
    rng = np.random.default_rng(n)
    cols = dict(
        pos=np.ascontiguousarray(pos, np.int32),
        contig_off=np.ascontiguousarray(contig_off, np.int64),
        sflags=np.ascontiguousarray(sflags if sflags is not None else (rng.random(n) < 0.1), np.uint8),
    )
    bases = np.frombuffer(b"ACGTN", np.uint8)
    cols["ref_base"] = np.ascontiguousarray(ref if ref is not None else np.where(cols["sflags"] == 1, 0, bases[rng.integers(0, 5, n)]), np.uint8)
    cols["alt_base"] = np.ascontiguousarray(alt if alt is not None else np.where(cols["sflags"] == 1, 0, bases[rng.integers(0, 4, n)]), np.uint8)
    v = abi.SitesView()
    v.n_sites, v.n_contigs = n, len(contig_off) - 1
    for k, a in cols.items():
        setattr(v, k, a.ctypes.data)
    return v, cols


def packed(v):
    cv, block, nb = io_native.pack_sites(v)
    n = int(cv.n_sites)
    n_spans = (n + SPAN - 1) // SPAN
    esc = int(cv.n_pos_esc)
    arr = lambda p, dt, k: np.ctypeslib.as_array((dt * max(k, 1)).from_address(p))[:k].copy() if k else np.zeros(0)  # noqa: E731
    import ctypes as C
    return dict(view=cv, block=block, bytes=nb, esc_idx=arr(cv.pos_esc_idx, C.c_int32, esc), esc_val=arr(cv.pos_esc_val, C.c_int32, esc), esc_off=arr(cv.pos_esc_off, C.c_int32, n_spans + 1),
                span=arr(cv.span_pos, C.c_int32, n_spans), d16=arr(cv.pos_d16, C.c_uint16, n))


def round_trip(v, cols):
    p = packed(v)
    pos, sf, rb, ab = io_native.unpack_sites(p["view"])
    np.testing.assert_array_equal(pos, cols["pos"])
    np.testing.assert_array_equal(sf, cols["sflags"])
    np.testing.assert_array_equal(rb, cols["ref_base"])
    np.testing.assert_array_equal(ab, cols["alt_base"])
    return p


def device_twin(p, n):
    """the arithmetic of k_sites_expand, span by span in numpy: inclusive sums of the differences, the last anchor at or before each site"""
    out = np.zeros(n, np.int64)
    for s in range(len(p["span"])):
        lo, hi = s * SPAN, min(n, (s + 1) * SPAN)
        ssum = np.cumsum(p["d16"][lo:hi].astype(np.int64))
        mark = np.full(hi - lo, -1)
        for e in range(p["esc_off"][s], p["esc_off"][s + 1]):
            mark[p["esc_idx"][e] - lo] = e
        anchor = np.maximum.accumulate(np.where(mark >= 0, np.arange(hi - lo), -1))
        a = np.maximum(anchor, 0)
        ev = np.append(p["esc_val"], 0).astype(np.int64)  # (mark -1 where no escape: the last entry, not used)
        base = np.where(anchor < 0, p["span"][s] - ssum[0], ev[mark[a]] - ssum[a])
        out[lo:hi] = base + ssum
    return out


def test_round_trip_windows_and_contigs():
    rng = np.random.default_rng(7)
    # three contigs of sorted window unions: gaps of ~150 bp inside a window, jumps of ~100 kb between windows
    parts, off = [], [0]
    for c in range(3):
        gaps = rng.integers(1, 300, 2500)
        jump = rng.random(2500) < 0.015
        gaps[jump] = rng.integers(LIMIT, 200000, int(jump.sum()))
        p = np.cumsum(gaps) + rng.integers(0, 1000)
        parts.append(p)
        off.append(off[-1] + len(p))
    pos = np.concatenate(parts)
    v, cols = plain_view(pos, off)
    p = round_trip(v, cols)
    n = len(pos)
    np.testing.assert_array_equal(device_twin(p, n), pos)
    # escapes: the first site of every contig that does not start a span, every jump of 2^15 or more
    d = np.diff(pos.astype(np.int64), prepend=pos[0])
    want = [i for i in range(n) if i % SPAN and (i in off[1:-1] or not 0 <= d[i] < LIMIT)]
    assert list(p["esc_idx"]) == want
    # 13 B per site in all (with gt and the nine genotype bytes) -> about 2 + 1 + escapes and span anchors for the site columns
    assert p["bytes"] < n * 3.3


def test_gap_of_exactly_two_to_the_fifteen():
    pos = np.array([100, 100 + LIMIT - 1, 100 + 2 * LIMIT - 1, 100 + 2 * LIMIT - 1 + 5], np.int32)
    v, cols = plain_view(pos, [0, 4])
    p = round_trip(v, cols)
    assert list(p["esc_idx"]) == [2]  # LIMIT - 1 fits, LIMIT escapes


def test_empty_chunk():
    v, cols = plain_view(np.zeros(0, np.int32), [0, 0, 0])
    p = round_trip(v, cols)
    assert int(p["view"].n_pos_esc) == 0 and list(p["esc_off"]) == [0]


def test_span_without_escapes():
    pos = np.cumsum(np.full(3 * SPAN + 17, 9)).astype(np.int32)
    v, cols = plain_view(pos, [0, len(pos)])
    p = round_trip(v, cols)
    assert int(p["view"].n_pos_esc) == 0
    np.testing.assert_array_equal(p["span"], pos[::SPAN])
    np.testing.assert_array_equal(device_twin(p, len(pos)), pos)


def test_unsorted_and_negative_differences_escape():
    pos = np.array([50, 40, 40, 2_000_000_000, -5, 7], np.int32)
    v, cols = plain_view(pos, [0, 6])
    p = round_trip(v, cols)
    assert list(p["esc_idx"]) == [1, 3, 4]


def test_what_the_form_cannot_carry_is_refused():
    pos = np.arange(10, dtype=np.int32)
    v, _ = plain_view(pos, [0, 10], ref=np.full(10, ord("a"), np.uint8))
    with pytest.raises(io_native.IoError):
        io_native.pack_sites(v)
    v, _ = plain_view(pos, [0, 10], sflags=np.full(10, 2, np.uint8))
    with pytest.raises(io_native.IoError):
        io_native.pack_sites(v)
    v, _ = plain_view(pos, [0, 4])  # contig_off does not end at n_sites
    with pytest.raises(io_native.IoError):
        io_native.pack_sites(v)


def test_every_column_is_aligned_for_one_copy():
    pos = np.cumsum(np.full(5000, 3)).astype(np.int32)
    v, _ = plain_view(pos, [0, 5000])
    cv, block, nb = io_native.pack_sites(v)
    base = block.ctypes.data
    assert base % 256 == 0 and nb <= block.nbytes
    for k in ("pos_d16", "bases8", "span_pos", "pos_esc_idx", "pos_esc_val", "pos_esc_off"):
        assert (getattr(cv, k) - base) % 256 == 0, k
    assert not cv.pos and not cv.sflags and not cv.ref_base and not cv.alt_base
