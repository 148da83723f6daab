"""The het form of a trio's genotype columns (uz_types.h: uz_family_view.het9 ...): uz_family_pack_het and its host twin
uz_family_unpack_het, which computes what the device's expansion (k_sites_expand) writes -- the widened columns at the kid-het sites, zeros
at all others.  No GPU."""
import numpy as np
import pytest

import hetcases
from unfazed_amd import io_native

SPAN = hetcases.SPAN


def _pack(t):
    c8 = hetcases.columns8(t)
    h9, hoff, nb = io_native.pack_family_het(*c8[:4])
    return c8, h9, hoff, nb


@pytest.mark.parametrize("t", hetcases.edge_tables(), ids=lambda t: t.name)
def test_round_trip(t):
    c8, h9, hoff, nb = _pack(t)
    gt, n = c8[0], t.n_sites
    het = (gt & 3) == 1
    n_spans = (n + SPAN - 1) // SPAN
    # the offsets: kid-het sites before every span; the bytes: the nine columns of those sites, in site order
    np.testing.assert_array_equal(hoff, np.concatenate([[0], np.cumsum(het)[np.minimum(np.arange(1, n_spans + 1) * SPAN, n) - 1]]))
    assert h9.size == 9 * int(het.sum())
    np.testing.assert_array_equal(h9.reshape(-1, 9).T, np.stack(c8[1] + c8[2] + c8[3])[:, het])
    assert nb == ((h9.size + 255) // 256 + (4 * (n_spans + 1) + 255) // 256) * 256
    # the twin: the widened columns where the kid is het, zeros elsewhere
    want = np.where(het[None, :], hetcases.widened(c8), 0).astype(np.uint16)
    np.testing.assert_array_equal(io_native.unpack_family_het(gt, h9, hoff), want)


def test_the_named_edges_are_in_the_tables():
    by = {t.name: t for t in hetcases.edge_tables()}
    het = lambda t: (t.gt & 3) == 1  # noqa: E731
    assert sorted(t.n_sites for t in by.values())[:5] == [1, 1023, 1024, 1025, 1324]
    t = by["span_without_het"]
    assert not het(t)[SPAN: 2 * SPAN].any() and het(t)[:SPAN].any() and het(t)[2 * SPAN:].any()
    t = by["span_of_het_only"]
    assert het(t)[SPAN: 2 * SPAN].all() and not het(t)[:SPAN].all()
    t = by["wide_het_sites"]
    assert t.wide is not None and het(t)[t.wide[0]].all() and list(t.wide[0]) == [0, 1023, 1024, SPAN + 299]
    for n in (1023, 2049):  # every one of the 64 genotype bytes
        assert np.unique(by["het_n%d_s0" % n].gt & 0x3F).size == 64


def test_empty_table():
    z = np.zeros(0, np.uint8)
    h9, hoff, nb = io_native.pack_family_het(z, [z] * 3, [z] * 3, [z] * 3)
    assert h9.size == 0 and list(hoff) == [0]
    assert io_native.unpack_family_het(z, h9, hoff).shape == (9, 0)


def test_block_is_aligned_for_one_copy():
    t = hetcases.table(5000, seed=11)
    _, h9, hoff, nb = _pack(t)
    assert h9.ctypes.data % 256 == 0 and hoff.ctypes.data % 256 == 0 and hoff.ctypes.data - h9.ctypes.data + hoff.nbytes <= nb


def test_twin_refuses_offsets_that_do_not_match_gt():
    t = hetcases.table(2 * SPAN + 9, seed=2)
    c8, h9, hoff, _ = _pack(t)
    bad = hoff.copy()
    bad[1] += 1  # (still ascending, still ending at n_het)
    with pytest.raises(io_native.IoError, match="het_span_off"):
        io_native.unpack_family_het(c8[0], h9, bad)
    bad = hoff.copy()
    bad[-1] -= 1
    with pytest.raises(io_native.IoError, match="het_span_off"):
        io_native.unpack_family_het(c8[0], h9, bad)


def test_packer_takes_the_eight_bit_columns_only():
    t = hetcases.table(100)
    with pytest.raises(ValueError):
        io_native.pack_family_het(t.gt, list(t.rd), list(t.ad), list(t.gq))
