"""The quality bits of listed bases on the host (uz_types.h bl_qlow; uz_reads_select_* with unit_masks & 8, ReadsSource.select(base_quals=True)):
a record with a base list sends one bit per listed base instead of its low-quality positions.  On the table of tests/qualcases.py -- quality
bytes written so that every rule has records that meet it -- every bit, the remaining position lists, the counts and the span sums are held
to the source's quality bytes; and the default (off) is byte for byte the form of a select without the argument."""
import numpy as np
import pytest

import qualcases
from unfazed_amd import abi


@pytest.fixture(scope="module")
def forms():
    t = qualcases.table()
    src = qualcases.source()
    new, idx = qualcases.select(src, True)
    old, idx_old = qualcases.select(src, False)
    assert np.array_equal(idx, idx_old)
    return t, src, new, old, idx


def _views(part, idx):
    sm = abi.small_columns(part)
    m = idx.size
    off, pos, code = abi.base_lists(part)
    return sm, m, off, pos.astype(np.int64), np.diff(off)


def test_the_table_meets_every_rule_by_construction(forms):
    """asserted before anything is compared: enough records of every kind, full spans, and spans that start inside a byte of both bit columns"""
    t, src, new, old, idx = forms
    sm, m, off, pos, cnt = _views(new, idx)
    where = {int(i): k for k, i in enumerate(idx)}
    n_a = n_b = n_c = 0
    for i in t.groups["listed_low"]:
        k = where[int(i)]
        low = qualcases.low_bits(i)
        assert cnt[k] > 0 and low[pos[off[k]: off[k + 1]]].any() and low.sum() <= abi.QLOW_LIST_MAX
        n_a += 1
    for i in t.groups["unlisted_low"]:
        k = where[int(i)]
        low = qualcases.low_bits(i)
        um = int(sm["umask"][k])
        in_units = [q for q in np.nonzero(low)[0] if (um >> (int(q) >> 5)) & 1]
        assert cnt[k] > 0 and not low[pos[off[k]: off[k + 1]]].any() and 0 < low.sum() <= abi.QLOW_LIST_MAX and in_units  # (the old form lists some of them)
        n_b += 1
    for i in t.groups["many_low"]:
        k = where[int(i)]
        assert cnt[k] > 0 and qualcases.low_bits(i).sum() > abi.QLOW_LIST_MAX and not (sm["aux"][k] & abi.AUX_NO_SEQ)
        n_c += 1
    assert n_a >= 50 and n_b >= 50 and n_c >= 5
    assert m // 1024 >= 2 and int(new.view.n_pk_spans) == (m + 1023) // 1024
    before = new.arrays["pk_sums"].reshape(-1, abi.PK_SUMS)[1:-1, 8].astype(np.int64)  # listed bases in front of spans 1 ..
    assert (before % 8 != 0).any() and (before % 4 != 0).any()


def test_every_bit_is_the_quality_of_its_listed_base(forms):
    t, src, new, old, idx = forms
    sm, m, off, pos, cnt = _views(new, idx)
    bits = abi.base_qual_bits(new)
    assert bits is not None and bits.size == int(new.view.n_bl) == int(off[-1]) and abi.base_qual_bits(old) is None
    assert len(new.arrays["bl_qlow"]) == (bits.size + 7) // 8
    n_set = 0
    for k in np.nonzero(cnt)[0]:
        low = qualcases.low_bits(int(idx[k]))
        want = low[pos[off[k]: off[k + 1]]] if low.sum() <= abi.QLOW_LIST_MAX else np.zeros(cnt[k], np.uint8)  # (more than the list holds: all 0)
        assert np.array_equal(bits[off[k]: off[k + 1]], want), k
        n_set += int(want.sum())
    assert n_set >= 50 and n_set == int(bits.sum())
    pad = np.unpackbits(new.arrays["bl_qlow"], bitorder="little")[bits.size:]
    assert not pad.any()  # (the bits behind the last entry are 0)


def test_counts_and_position_lists_follow_the_rule(forms):
    """tup_n_low: the set bits of a record with a base list (the read's own count when it has more than UZ_QLOW_LIST_MAX low bases), as before for
    every other record; qlow_pos: exactly the lists of the records WITHOUT a base list, as the old form holds them"""
    t, src, new, old, idx = forms
    sm, m, off, pos, cnt = _views(new, idx)
    sm_old = abi.small_columns(old)
    bits = abi.base_qual_bits(new)
    nl, nl_old = sm["n_low"][:m].astype(np.int64), sm_old["n_low"][:m].astype(np.int64)
    no_seq = (sm["aux"][:m] & abi.AUX_NO_SEQ) != 0
    with_list = cnt > 0
    for k in ("flag", "l_seq", "n_cigar", "mapq", "aux", "umask", "bl_n"):
        assert np.array_equal(sm[k][:m], sm_old[k][:m]), k
    assert np.array_equal(nl[~with_list], nl_old[~with_list])
    for k in np.nonzero(with_list)[0]:
        full = int(qualcases.low_bits(int(idx[k])).sum())
        assert nl[k] == (int(bits[off[k]: off[k + 1]].sum()) if full <= abi.QLOW_LIST_MAX else min(full, 255)), k
    # the lists: the old form's, minus the entries of the records with a base list
    lists_old = ~no_seq & (nl_old <= abi.QLOW_LIST_MAX)
    lo_old = np.concatenate([[0], np.cumsum(np.where(lists_old, nl_old, 0))])
    assert lo_old[-1] == int(old.view.n_qlow_pos)
    keep = np.concatenate([old.arrays["qlow_pos"][lo_old[k]: lo_old[k + 1]] for k in np.nonzero(lists_old & ~with_list)[0]] + [np.zeros(0, np.uint8)])
    assert int(new.view.n_qlow_pos) == keep.size < int(old.view.n_qlow_pos)
    assert np.array_equal(new.arrays["qlow_pos"][: keep.size], keep)
    # ... and they are those records' low-quality positions inside their staged units
    lists_new = ~no_seq & (nl <= abi.QLOW_LIST_MAX) & ~with_list
    lo_new = np.concatenate([[0], np.cumsum(np.where(lists_new, nl, 0))])
    for k in np.nonzero(lists_new)[0][::5]:
        low = np.nonzero(qualcases.low_bits(int(idx[k])))[0]
        um = int(sm["umask"][k])
        want = low if um == abi.UMASK_ALL else low[((um >> (low >> 5)) & 1) == 1]
        assert np.array_equal(new.arrays["qlow_pos"][lo_new[k]: lo_new[k + 1]].astype(np.int64), want), k
    # every other column of the view is the old form's
    for name in old.arrays:
        if name not in ("qlow_pos", "pk_sums", "tup8", "tup_hot", "tup_esc", "tup_esc_off") and not name.startswith("tup_"):
            assert np.array_equal(new.arrays[name], old.arrays[name]), name
    print("bytes: %d listed positions -> %d, + %d bytes of bits for %d listed bases" % (int(old.view.n_qlow_pos), keep.size, (bits.size + 7) // 8, bits.size))


def test_span_sums_agree_with_the_view(forms):
    t, src, new, old, idx = forms
    sm, m, off, pos, cnt = _views(new, idx)
    S = new.arrays["pk_sums"].reshape(-1, abi.PK_SUMS).astype(np.int64)
    So = old.arrays["pk_sums"].reshape(-1, abi.PK_SUMS).astype(np.int64)
    nl = sm["n_low"][:m].astype(np.int64)
    q3 = np.where(((sm["aux"][:m] & abi.AUX_NO_SEQ) == 0) & (nl <= abi.QLOW_LIST_MAX) & (cnt == 0), nl, 0)  # quantity 3: 0 for a record with a base list
    run3 = np.concatenate([[0], np.cumsum(q3)])
    run8 = np.concatenate([[0], np.cumsum(cnt)])
    at = np.minimum(np.arange(S.shape[0]) * 1024, m)
    assert np.array_equal(S[:, 3], run3[at]) and np.array_equal(S[:, 8], run8[at])
    assert S[-1, 3] == int(new.view.n_qlow_pos) and S[-1, 8] == int(new.view.n_bl)
    other = [k for k in range(abi.PK_SUMS) if k != 3]
    assert np.array_equal(S[:, other], So[:, other])


def test_off_is_byte_identical_to_a_select_without_the_argument(forms):
    t, src, new, old, idx = forms
    fc, flo, fhi, fex = t.fetches
    plain, idx_p = src.select(fc, flo, fhi, want_index=True, extra=fex)
    assert np.array_equal(idx_p, idx) and sorted(plain.arrays) == sorted(old.arrays) and "bl_qlow" not in plain.arrays and not plain.view.bl_qlow
    for name in plain.arrays:
        assert plain.arrays[name].tobytes() == old.arrays[name].tobytes(), name
    for f, _ in abi.ReadsPackedView._fields_:
        v0, v1 = getattr(plain.view, f), getattr(old.view, f)
        if not isinstance(v0, int) or f in plain.arrays:  # (pointers: both set or both null)
            assert bool(v0) == bool(v1), f
        else:
            assert v0 == v1, f


def test_quality_bits_need_the_base_lists():
    """bit 8 of unit_masks is valid only together with 4: the library refuses it alone; select(base_lists=False, base_quals=True) asks for neither"""
    import ctypes as C
    IO_E_ARG = -5  # unfazed_io.h UZ_IO_E_ARG
    t = qualcases.table()
    src = qualcases.source()
    fc, flo, fhi, fex = (np.ascontiguousarray(x) for x in t.fetches)
    sel = C.c_void_p()
    rc = src.lib.uz_reads_select_plan(src._h.ptr, int(fc.size), fc.ctypes.data, flo.ctypes.data, fhi.ctypes.data, 0, 1 | 8, fex.ctypes.data, 7, 0, C.byref(sel))
    assert rc == IO_E_ARG and not sel.value
    part, _ = qualcases.select(src, True, base_lists=False)
    assert "bl_qlow" not in part.arrays and "bl_pos" not in part.arrays
