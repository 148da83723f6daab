"""The link forms of a site window on the CPU: the model of tests/siteformmodel.py (written from uz_types.h) against the packer's source
columns and against the host twin uz_sites_unpack, on every table of tests/siteformcases.py; each table reaches what it is named for; a
world table notices a wrong escape, a wrong difference and swapped bases.  tests/test_site_forms_gpu.py holds the device to the same model,
and is to be trusted only while this file passes.  Every comparison is np.array_equal.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import siteformcases as sfc
import siteformmodel as sfm
import sitecases
from siteformmodel import D16_LIMIT, SPAN
from unfazed_amd import abi, io_native

CASES = sfc.cases()
BY = {c.name: c for c in CASES}
COLS = ("pos", "sflags", "ref_base", "alt_base")
MODE = abi.FIND_SECOND_WINDOW
IO_E_ARG = -5  # unfazed_io.h UZ_IO_E_ARG


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_number_of_cases_is_pinned():
    assert len(CASES) == sfc.N_CASES == 52
    assert len({c.name for c in CASES}) == 52
    assert sum(c.hand for c in CASES) == 8 and len(sfc.world_cases()) == 3
    assert [c.n for c in CASES[:17]] == list(sfc.SIZES)


@pytest.mark.parametrize("c", [c for c in CASES if not c.hand], ids=repr)
def test_model_of_the_packers_output_equals_the_source(c):
    for name, got, want in zip(COLS, c.model(), c.want):
        assert got.dtype == want.dtype and np.array_equal(got, want), name


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_host_twin_equals_the_model(c):
    twin = io_native.unpack_sites(c.held.view)
    for name, got, want in zip(COLS, twin, c.model()):
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:5])
    if c.want is not None:  # (a hand-edited view whose result was worked out by hand)
        assert same(c.model(), c.want)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_het_form_twin_equals_the_model(c):
    gt, rd8, ad8, gq8, _ = c.c8
    h9, hoff, _ = io_native.pack_family_het(gt, rd8, ad8, gq8)
    want, open_ = sfm.het_columns(gt, h9, hoff)
    assert np.array_equal(io_native.unpack_family_het(gt, h9, hoff), want)
    full, open8 = sfm.widen8(c.cols8())
    het = (np.asarray(gt) & 3) == sfm.HET
    assert np.array_equal(want[:, het], full[:, het]) and not want[:, ~het].any() and np.array_equal(open_, open8 & het)


def test_twin_refuses_an_escape_at_a_spans_first_site():
    """the device takes span_pos there (k_sites_expand: l == 0) and the upload refuses the view; the twin took the escape's value"""
    src = BY["span_without_escapes_between"]
    eidx, ev = src.parts["eidx"].copy(), src.parts["eval"].copy()
    assert eidx[2] == 2 * SPAN + 1
    eidx[2], ev[2] = 2 * SPAN, 777
    v = sfc.hand_view(**dict(src.parts, eidx=eidx, eval=ev))
    with pytest.raises(io_native.IoError, match="first site") as e:
        io_native.unpack_sites(v.view)
    assert e.value.code == IO_E_ARG
    assert same(io_native.unpack_sites(sfc.hand_view(**src.parts).view), src.want)  # (the same view unbroken)


# ------------------------------------------------------------------------------------------------------- each case reaches what it names
@pytest.mark.parametrize("c", CASES, ids=repr)
def test_escape_index_sets(c):
    assert [int(e) for e in c.parts["eidx"]] == list(c.reach["esc"])
    assert int(c.held.view.n_pos_esc) == len(c.reach["esc"])
    assert not any(e % SPAN == 0 for e in c.reach["esc"])


def test_sizes_reach_every_tail_and_last_span():
    assert {n % 4 for n in sfc.SIZES} == {0, 1, 2, 3}
    assert {n % 4 for n in sfc.SIZES if n > SPAN} == {0, 1, 2, 3}  # (also behind a full span)
    assert any(n % SPAN == 1 and n > SPAN for n in sfc.SIZES) and any(n % SPAN == SPAN - 1 for n in sfc.SIZES)


def test_one_escape_per_span_reaches_every_hand_over():
    for name, extra in (("one_escape_per_span", []), ("one_escape_per_span_partial", [4])):
        c = BY[name]
        assert [int(e) % SPAN for e in c.parts["eidx"]] == list(sfc.ONE_ESCAPE_AT) + extra
        assert [int(e) // SPAN for e in c.parts["eidx"]] == list(range(len(sfc.ONE_ESCAPE_AT) + len(extra)))  # one span each, in this order
        assert np.all(np.diff(c.parts["eoff"]) == 1)
    assert BY["one_escape_per_span_partial"].n % SPAN == 5
    for edge in (256, 512, 768):  # lane 63 of a wave | lane 0 of the next
        assert {edge - 1, edge} <= set(sfc.ONE_ESCAPE_AT)
    assert {1, 2, 3, 1020, 1021, 1022, 1023} <= set(sfc.ONE_ESCAPE_AT)


def test_dense_escapes_reach_their_marks():
    per_span = lambda c: np.diff(c.parts["eoff"])  # noqa: E731
    local = lambda c: [int(e) - SPAN for e in c.parts["eidx"]]  # noqa: E731
    assert list(per_span(BY["dense_whole_span"])) == [0, SPAN - 1, 0]  # `mark` reaches 1023
    assert max(int(per_span(c).max()) for c in CASES) == SPAN - 1
    assert local(BY["dense_one_lane"]) == [148, 149, 150, 151]
    assert [l % 4 for l in local(BY["dense_lane_k1_k3"])] == [1, 3] and len({l // 4 for l in local(BY["dense_lane_k1_k3"])}) == 1
    assert local(BY["dense_last_of_every_lane"]) == [4 * t + 3 for t in range(256)]
    assert local(BY["dense_first_of_every_lane"]) == [4 * t for t in range(1, 256)]
    assert local(BY["dense_wave_1"]) == list(range(256, 512))
    eoff = BY["span_without_escapes_between"].parts["eoff"]
    assert eoff[1] == eoff[2] and eoff[0] < eoff[1] and eoff[2] < eoff[3]  # equal neighbours in pos_esc_off


def test_values_reach_their_edges():
    c = BY["differences_0_1_32767_32768"]
    pos = c.want[0].astype(np.int64)
    assert list(np.diff(pos)[:5]) == [0, 1, D16_LIMIT - 1, 0, D16_LIMIT] and list(c.parts["d16"][1:5]) == [0, 1, D16_LIMIT - 1, 0]
    pos = BY["negative_zero_minus5_int32_max"].want[0]
    assert {0, -5, (1 << 31) - 1, -(1 << 31)} <= set(int(p) for p in pos) and (np.diff(pos.astype(np.int64)) < 0).any()
    c = BY["span_of_32767_up_to_int32_max"]
    assert np.all(c.parts["d16"][SPAN + 1: 2 * SPAN] == D16_LIMIT - 1) and int(c.want[0][2 * SPAN - 1]) == (1 << 31) - 1
    c = BY["span_from_negative_across_zero"]
    for s in (0, 1):
        assert c.parts["span"][s] < 0 < c.want[0][(s + 1) * SPAN - 1]
    c = BY["escape_below_its_predecessor"]
    assert all(c.want[0][e] < c.want[0][e - 1] for e in c.parts["eidx"])


def test_contigs_reach_their_edges():
    c = BY["contig_starts_l0_l1_l1023"]
    off = [int(o) for o in c.parts["contig_off"]]
    assert [o % SPAN for o in off[1:4]] == [0, 1, 1023] and 1 in np.diff(off)  # (and a contig of one site)
    assert off[1] not in c.reach["esc"] and off[2] in c.reach["esc"] and off[3] in c.reach["esc"]
    d = np.diff(c.want[0].astype(np.int64))
    assert all(0 <= d[o - 1] < D16_LIMIT for o in off[2:4])  # a contig start whose difference would fit: an escape all the same
    off = [int(o) for o in BY["empty_contigs"].parts["contig_off"]]
    assert off[0] == off[1] == off[2] and off[3] == off[4] and off[-1] == off[-2] and len(set(off)) == 4  # empty at the front (two), in the middle and at the end
    c = BY["contigs_300_of_one_site"]
    assert np.all(np.diff(c.parts["contig_off"]) == 1) and c.parts["contig_off"].size == 301
    c = BY["hand_d16_ffff_at_anchors_contig_starts_l0_l1_l1023"]
    assert all(c.parts["d16"][e] == 0xFFFF for e in c.parts["eidx"])  # the escape must win over pos_d16


def test_bases_reach_every_pair_at_every_residue():
    every = {(r, a, x) for r in range(6) for a in range(6) for x in (0, 1)}
    for name in ("bases_tail_ACGTN0", "bases_tail_CTN0AG"):
        c = BY[name]
        b = c.parts["b8"]
        full = 4 * (c.n // 4)
        for res in range(4):
            assert {(int(v) & 7, int(v) >> 3 & 7, int(v) >> 6) for v in b[res:full:4]} == every, res
        assert c.n - full == 3
        assert {int(x) for col in c.want[2:] for x in col[full:]} == set(b"ACGTN\0")
    b = BY["hand_codes_6_7_bit_7"].parts["b8"]
    assert {6, 7} <= {int(v) & 7 for v in b} and {6, 7} <= {int(v) >> 3 & 7 for v in b} and (b & 0x80).any() and not (b & 0x80).all()
    for res in range(4):
        assert {6, 7} <= {int(v) & 7 for v in b[res::4]} | {int(v) >> 3 & 7 for v in b[res::4]}


def test_hand_views_leave_open_what_the_header_leaves_open():
    for c in CASES:
        if c.name.startswith("hand_d16_ffff"):
            anchors = np.concatenate([np.arange(0, c.n, SPAN), c.parts["eidx"]])
            assert np.all(c.parts["d16"][anchors] == 0xFFFF) and len(c.parts["eidx"]) > 0
    v = BY["hand_no_escapes_null_lists"].held.view
    assert v.n_pos_esc == 0 and not v.pos_esc_idx and not v.pos_esc_val and v.pos_esc_off
    c = BY["hand_escape_where_the_difference_fits"]
    e = int(c.parts["eidx"][0])
    assert 0 < c.parts["d16"][e] < D16_LIMIT and c.want[0][e] == c.parts["eval"][0] != BY["size_2049"].want[0][e]


def test_family_columns_reach_every_byte_at_every_residue_and_in_the_tail():
    edge = {0, 1, 253, 254, 255}
    c = BY["family_n290"]
    c8, full = c.cols8(), 4 * (c.n // 4)
    for q in range(9):
        for res in range(4):
            assert edge <= {int(v) for v in c8[q, res:full:4]}, (q, res)
    tails = [BY["family_tail_roll%d" % r] for r in (0, 3, 6)]
    for q in range(9):
        assert edge <= {int(v) for t in tails for v in t.cols8()[q]}, q  # (n = 3: every site is in the scalar tail)
    for n in (1, 255, 256, 257):
        assert BY["size_%d" % n].n == n
    pairs = set()
    for c in sfc.family_cases():
        c8 = c.cols8()
        listed = np.zeros(c.n, bool)
        if c.c8[4] is not None:
            listed[c.c8[4][0]] = True
        assert np.array_equal((c8[:6] == 255).any(axis=0), listed)  # 255 in a depth column only at wide-listed sites
        pairs |= {(int(g), int(x)) for g, x in zip(c.c8[0], c.model()[1])}
    assert {(g, x) for g in sfc.GT_EDGE for x in (0, 1)} <= pairs  # each incoming gt byte at complex and at non-complex sites


def test_family_model_on_hand_worked_bytes():
    """the eight-bit and the het form of three sites, worked out by hand from the header"""
    c8 = np.array([[0, 254, 255]] * 6 + [[0, 254, 255]] * 3, np.uint8)
    w, o = sfm.widen8(c8)
    assert [list(r) for r in w[:6]] == [[0, 0xFFFF, 255]] * 6 and [list(r) for r in w[6:]] == [[0, 254, 0xFFFF]] * 3
    assert [list(r) for r in o[:6]] == [[False, False, True]] * 6 and not o[6:].any()
    gt = np.array([0x01, 0x3F, 0xC5], np.uint8)  # kid het, hom-alt, het
    hw, ho = sfm.het_columns(gt, np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 254, 255, 0, 0, 0, 0, 255, 254, 17], np.uint8), [0, 2])
    assert list(hw[:, 0]) == [1, 2, 3, 4, 5, 6, 7, 8, 9] and not hw[:, 1].any() and list(hw[:, 2]) == [0xFFFF, 255, 0, 0, 0, 0, 0xFFFF, 254, 17]
    assert list(np.nonzero(ho.reshape(-1))[0]) == [1 * 3 + 2]
    assert list(sfm.folded_gt([0x00, 0x3F, 0x40, 0x80, 0xFF, 0xFF], [0, 1, 0, 1, 0, 1])) == [0x00, 0x7F, 0x00, 0x40, 0x3F, 0x7F]


def test_world_tables_are_what_the_device_tests_need():
    edges, inside, jumps = set(), 0, 0
    for c in sfc.world_cases():
        t = c.table
        assert sfm.n_spans(c.n) <= 6 and 2 <= len(t.contigs) <= 4 and c.ascends()
        edges |= {int(e) % SPAN for e in c.parts["eidx"]}
        inside += sum(1 for o in t.contig_off[1:-1] if o % SPAN)
        jumps += int((np.diff(t.pos.astype(np.int64)) >= D16_LIMIT).sum())
        assert len(set(t.ref_base)) >= 5 and len(set(t.alt_base)) >= 4 and 0 < t.complex.sum() < c.n
    assert {255, 256, 511, 512, 767, 768, 1023, 1} <= edges and inside >= 3 and jumps >= 3


# ------------------------------------------------------------------------------------------------------------ a world table notices
def _sites(t, cols):
    return abi.sites_view(SimpleNamespace(contig_off=t.contig_off, pos=cols[0], sflags=cols[1], ref_base=cols[2], alt_base=cols[3], n_sites=t.n_sites,
                                          contigs=t.contigs))


@pytest.mark.parametrize("c", sfc.world_cases(), ids=repr)
def test_world_table_notices_a_wrong_escape_difference_and_base(c):
    """one escape value moved by +1 and by -1, one pos_d16 raised by 1, ref and alt swapped at one site: the columns read back from the
    mutated view differ from the source, and the two wrong positions also change the oracle's find lists -- the DNM that stands on the
    moved site left it out (a site inside its own small event), and now lists it"""
    from oracle import oracle as orc
    t, p = c.table, c.parts
    fv, dv = t.family_view(), sitecases.dnms_view(sfc.dnms_of(c))
    P = abi.make_params(search_dist=250)
    het = (orc.classify(P, t.sites_view(), fv) & 1).astype(bool)  # UZ_CL_HET
    base = orc.find(P, _sites(t, c.want), fv, dv, MODE)
    assert base[0][-1] > 0 and base[3][-1] > 0  # (the lists are not empty)

    def decode(**edit):
        q = dict(p, **edit)
        return sfm.site_columns(q["d16"], q["b8"], q["span"], q["eidx"], q["eval"], q["eoff"], q["n"])

    def noticed(cols, by_find):
        assert not same(cols, c.want)
        if by_find:
            got = orc.find(P, _sites(t, cols), fv, dv, MODE)
            assert not all(np.array_equal(a, b) for a, b in zip(base, got))

    k = next(k for k, e in enumerate(p["eidx"]) if het[e])  # (a table without such an escape fails here)
    for step in (1, -1):
        ev = p["eval"].copy()
        ev[k] += step
        noticed(decode(eval=ev), by_find=True)
    anchors = set(int(e) for e in p["eidx"]) | set(range(0, c.n, SPAN))
    j = next(int(e) + 1 for e in p["eidx"] if int(e) + 1 < c.n and int(e) + 1 not in anchors and het[e + 1] and p["d16"][e + 1] > 0)
    d16 = p["d16"].copy()
    d16[j] += 1
    noticed(decode(d16=d16), by_find=True)
    s = next(i for i in range(c.n) if (p["b8"][i] & 7) != (p["b8"][i] >> 3 & 7))
    b8 = p["b8"].copy()
    b8[s] = (b8[s] & 0xC0) | (b8[s] & 7) << 3 | (b8[s] >> 3 & 7)
    noticed(decode(b8=b8), by_find=False)
