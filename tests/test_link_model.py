"""The plain decoder of the link form (tests/linkmodel.py) and the host packer (io_pack.cpp: pack_reads, ReadsSource.select) held to each other
through the source: for every table of the panel (tests/linkcases.py) and every form the packer emits of it, decode(select(source)) is the source
table restricted to the selection, its staged units and its listed bases -- headers, flags, CIGAR words with the omitted simple words restored,
every base of every staged unit, every quality word of every record with a quality row, the count that travelled.  Then the reach of the panel:
which pair codes occur, the escapes and list entries per span against the header build's LDS room on both sides, every residue of a span's first
listed base mod 8, the combinations in use, the escape values as real values, and which forms the packer chose.  No GPU: this file must pass
before tests/test_link_cases_gpu.py, which holds the device to the same model, is trusted."""
import numpy as np
import pytest

import linkcases as lc
import linkmodel as lm

_PANEL = {}


def panel():
    if not _PANEL:
        for c in lc.panel():
            _PANEL[c.name] = c
    return _PANEL


CASE_NAMES = ["edges", "wide", "room_cigar", "room_esc", "room_qpos", "room_bl", "sentinels", "dict_1", "dict_255", "dict_256", "dict_257", "dict_300",
              "dict_edges"] + ["b0_%d" % r for r in range(8)] + ["count_%d" % n for n in (1, 255, 256, 257, 1023, 1024, 1025, 2049, 1026, 1027)]


def test_the_panel_is_the_list_of_names():
    assert sorted(panel()) == sorted(CASE_NAMES)


def _words(bits):
    return (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)


def _popcount(w):
    return np.unpackbits(np.ascontiguousarray(w, np.uint32).view(np.uint8).reshape(-1, 4), axis=1).sum(1).astype(np.int64)


def against_source(case, form, part, idx, t, thr):
    """decode()'s table of a selection against the source table"""
    T, n, what = case.table, idx.size, (case.name, form[0], thr)
    assert t["n"] == n == int(part.view.n_segs), what
    for k in ("start", "end", "tlen", "flag", "mapq", "l_seq", "n_cigar"):
        assert np.array_equal(t[k], getattr(T, k)[idx]), (k, what)
    new_of = np.full(case.n, -1, np.int64)
    new_of[idx] = np.arange(n)
    m = T.mate[idx]
    assert np.array_equal(t["mate"], np.where(m >= 0, new_of[np.maximum(m, 0)], -1)), ("mate", what)
    q = t["qname"] if getattr(part, "qname_map", None) is None else part.qname_map[t["qname"]]
    assert np.array_equal(q, T.qname[idx]), ("qname", what)
    assert np.array_equal(t["aux"] & ~np.uint8(lm.AUX_SIMPLE_MASK | lm.AUX_NO_SEQ), T.aux[idx]), ("aux", what)
    assert part.view.cigar_compact or not (t["aux"] & lm.AUX_SIMPLE_MASK).any(), what
    nc = T.n_cigar[idx].astype(np.int64)
    at = np.repeat(T.cigar_off[idx].astype(np.int64), nc) + (np.arange(int(nc.sum())) - np.repeat(np.concatenate([[0], np.cumsum(nc)])[:-1], nc))
    assert np.array_equal(t["cigar"], T.cigar[at] if at.size else np.zeros(0, np.uint32)), ("cigar", what)
    # bases
    k32 = np.arange(32)
    rows, cols = idx[t["b_rec"]], 32 * t["b_unit"][:, None] + k32[None, :]
    src = case.code_mat[rows[:, None], cols]
    listed_unit = t["listed"][t["b_rec"]]
    assert np.array_equal(t["codes"][~listed_unit], src[~listed_unit]), ("bases of the rows", what)
    at_list = np.zeros(src.shape, bool)
    at_list[t["bl_at"], t["bl_pos"] & 31] = True
    assert np.array_equal(t["codes"][at_list], src[at_list]) and np.all(src[at_list] != 0), ("listed bases ('=' is never listed)", what)
    rest = listed_unit[:, None] & ~at_list  # code 0, but for a base that is none of the four: its exception lies in a staged unit and is applied
    four = np.isin(src, (1, 2, 4, 8))
    assert np.array_equal(t["codes"][rest], np.where(four, 0, src)[rest]), ("unlisted bases of a listed record", what)
    if form[3].startswith("everything"):  # every unit of every record travelled
        assert t["has_seq"].all() and t["b_rec"].size == int(lm.row_units(T.l_seq[idx]).sum()), what
    # qualities
    low = case.qual_mat < thr
    qsrc = _words(low[idx[t["q_rec"]][:, None], 32 * t["q_unit"][:, None] + k32[None, :]])
    if t["lists"] and t["bl_quals"]:  # a listed record's bits: at its listed positions and nowhere else
        only = _words(at_list)
        sel = t["listed"][t["q_rec"]]
        qsrc = np.where(sel, qsrc & only, qsrc)
    has = t["q_has"]
    assert np.array_equal(t["q_word"][has], qsrc[has]), ("quality words", what)
    full = low[idx].sum(1)
    sat = np.minimum(full, 255)
    nl = t["n_low"].astype(np.int64)
    if not t["lists"]:
        assert np.array_equal(nl, sat), ("n_low of the plane", what)
    else:
        keeps = (full > lm.QLOW_LIST_MAX) | ~t["has_seq"]
        assert np.array_equal(nl[keeps], sat[keeps]), ("n_low of a record without a list", what)
        sent = np.bincount(t["q_rec"][has], weights=_popcount(t["q_word"][has]), minlength=n).astype(np.int64)
        assert np.array_equal(nl[~keeps], sent[~keeps]), ("n_low of a record with a list: the positions / bits that travelled", what)
        rec_has = np.zeros(n, bool)
        rec_has[t["q_rec"][has]] = True
        staged_any = np.zeros(n, bool)
        staged_any[t["b_rec"]] = True
        assert np.array_equal(rec_has, staged_any & (nl <= lm.QLOW_LIST_MAX)), ("which records get a quality row", what)
    # masks
    um = t["umask"].astype(np.int64)
    assert np.all((um[t["listed"]] & lm.UMASK_LISTED) != 0) and np.all(um[T.l_seq[idx] > 480] == lm.UMASK_ALL), ("stored masks", what)


_SEEN = {}


def _decoded(name):
    """every form of a case, decoded once: {form name: (form, part, idx, table)}"""
    if name not in _SEEN:
        case = panel()[name]
        _SEEN[name] = {}
        for form in lc.form_list(case):
            part, idx = lc.select(case, form)
            _SEEN[name][form[0]] = (form, part, idx, lm.decode(part))
    return _SEEN[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_form_decodes_to_the_source(name):
    case = panel()[name]
    for form, part, idx, t in _decoded(name).values():
        against_source(case, form, part, idx, t, lc.THRESHOLD)


@pytest.mark.parametrize("thr", [0, 255])
def test_the_thresholds_at_their_ends(thr):
    """nothing lies below 0; everything but a quality of 255 lies below 255"""
    for name in ("edges", "wide"):
        case = panel()[name]
        for form in lc.form_list(case):
            if form[0] in ("pair8/points/tup8=1/bl=1/bq=1", "pair8/everything/tup8=1/bl=1/bq=0", "pair8/everything/plane", "pair8/points/tup8=1/bl=0/bq=0"):
                part, idx = lc.select(case, form, threshold=thr)
                t = lm.decode(part)
                against_source(case, form, part, idx, t, thr)
                assert (t["n_low"].max() == 0) if thr == 0 else (t["n_low"].max() == 255), (name, form[0])


LINK = "pair8/everything/tup8=1/bl=1/bq=1"
POINTS = "pair8/points/tup8=1/bl=1/bq=1"


def test_reach_of_the_edges_table():
    d = _decoded("edges")
    form, part, idx, t = d[LINK]
    case = panel()["edges"]
    assert idx.size == case.n == 2100 and np.array_equal(idx, np.arange(case.n))
    p = part.arrays["pair_d8"][: case.n].astype(int)
    assert {0, 253, 254, 255} <= set(p.tolist()), "SECOND, SECOND_TLEN, NEW and OLD"
    assert p[250] == 10 and p[260] == 0, "FIRST / SECOND across a round edge"
    assert p[255] == 252 and p[507] == 0, "distance 252 from a round's last record"
    assert p[1023] == 1 and p[1024] == 0, "a pair across the span edge"
    assert p[300] == 1 and p[301] == 253, "SECOND_TLEN"
    assert p[302] == 1 and t["end"][303] > t["end"][302] and t["tlen"][302] == t["end"][303] - t["start"][302], "tlen from the SECOND's end"
    assert p[320] >= 254 and p[320 + 253] >= 254, "one beyond the largest distance is spelled out"
    assert p[332] == 255 and t["qname"][332] == t["qname"][330] == t["qname"][331], "a name carried by three records"
    assert p[340] in (254, 255) and t["mate"][340] == 341 and t["mate"][341] == -1, "a one-way mate link"
    assert p[350] == 254 and t["mate"][350] == -1 and p[351] == 255 and t["mate"][351] == -1, "NEW and OLD without a mate"
    assert {p[310], p[311]} == {254, 255} and t["mate"][310] == 311, "NEW and OLD with a mate"
    sd = part.arrays["start_d8"][: case.n].astype(int)
    assert sd[40] == 0 and sd[41] == 254 and sd[42] == 255 and sd[43] == 255 and sd[1500] == 255, "start differences 0 / 254, and 255 / a large gap / a contig change escaped"
    assert t["start"][42] - t["start"][41] == 255 and t["start"][1500] < t["start"][1499]
    assert set(t["l_seq"][60:69].tolist()) == {0, 1, 31, 32, 33, 64, 151, 255, 256}
    assert t["n_cigar"][60] == 0 and (t["aux"][60] & lm.AUX_DECODE_BAD)
    codes = (t["aux"].astype(int) & lm.AUX_SIMPLE_MASK) >> lm.AUX_SIMPLE_SHIFT
    assert codes[70] == 1 and codes[80] == 2 and codes[81] == 3 and codes[82] == 0, "simple codes 1, 2, 3; an M shorter than the read keeps its word"
    for k in (83, 84, 86, 87):
        assert t["end"][k] == t["start"][k] + 1, "reference length 0 / flag 4 / no CIGAR: end = start + 1"
    assert t["n_cigar"][87] == 0 and t["l_seq"][87] == 151 and t["n_cigar"][88] == 300 and t["n_cigar"][85] == 5
    assert t["n_low"][100:106].tolist() == [0, 1, 10, 11, 254, 255]
    # the same table through single-position fetches: masks, lists, records without bases, exceptions of units that stayed home
    form, part, idx, t = d[POINTS]
    um = t["umask"].astype(int)
    assert t["listed"].any() and (~t["listed"] & t["has_seq"]).any() and (~t["has_seq"]).any()
    assert ((um != 0xFFFF) & (um & 0x7FFF).astype(bool)).any() and not t["exc_used"].all() and t["exc_used"].any(), "an exception in a unit that stayed home is ignored"
    k = int(np.nonzero(idx == 116)[0][0])
    assert not t["listed"][k] and t["has_seq"][k] and t["listed"][k - 1], "'=' keeps the record off the list form"
    for src_rec, code in ((113, 15), (114, 6)):
        k = int(np.nonzero(idx == src_rec)[0][0])
        e = np.nonzero((t["bl_rec"] == k) & (case.code_mat[src_rec][t["bl_pos"]] == code))[0]
        assert t["listed"][k] and e.size == 1 and t["codes"][t["bl_at"][e[0]], t["bl_pos"][e[0]] & 31] == code, "N / S as a listed base: through the exceptions"
    hs = t["has_seq"]
    assert (hs[:-1] & ~hs[1:]).any() and (~hs[:-1] & hs[1:]).any(), "records without bases between records with rows"
    off_units = t["listed"] & (t["n_low"] == 0) & ((case.qual_mat[idx] < lc.THRESHOLD).sum(1) > 0)
    assert off_units.any(), "a listed record whose low bases lie only outside its staged units"


def test_reach_of_the_rooms():
    """both sides of each of the header build's four LDS rooms, a span inside its room beside each"""
    for name, form, col, room in (("room_cigar", LINK, 4, 256), ("room_qpos", "pair8/everything/tup8=1/bl=0/bq=0", 3, 4096),
                                  ("room_qpos", "pair8/everything/tup8=1/bl=1/bq=0", 3, 4096), ("room_bl", POINTS, 8, 4096)):
        t = _decoded(name)[form][3]
        share = t["span_share"][:, col].tolist()
        assert share[0] == room and share[1] == room + 1 and 0 < share[2] < room, (name, share)
    t = _decoded("room_esc")[LINK][3]
    assert t["span_esc"].tolist()[:2] == [64, 65] and 0 < t["span_esc"][2] < 64
    part = _decoded("room_esc")[LINK][1]
    rec = (part.arrays["esc16_key"][: int(part.view.n_esc16)] >> np.uint64(2)).astype(np.int64)
    assert {0, 1024, 2047} <= set(rec.tolist()), "escapes at the first and last record of a span"
    part = _decoded("room_bl")[POINTS][1]
    assert "bl_qlow" in part.arrays and not part.view.bl_wide
    t = _decoded("room_bl")[POINTS][3]
    assert np.bincount(t["bl_rec"]).max() == 5, "five fetch points on one read"


def test_reach_of_the_residues():
    seen = set()
    for r in range(8):
        t = _decoded("b0_%d" % r)[POINTS][3]
        assert t["span_share"][1, 8] > 0 and t["bl_quals"]
        seen.add(int(t["span_first_bl"][1]) % 8)
        assert int(t["span_first_bl"][1]) % 8 == r
    assert seen == set(range(8)), "every residue of a span's first listed base mod 8 (and so mod 4)"


def test_reach_of_the_dictionary():
    for combos in (1, 255, 256, 257, 300):
        form, part, idx, t = _decoded("dict_%d" % combos)[LINK]
        assert int(part.view.n_tup) == combos and "tup8" in part.arrays
        assert int(part.view.n_tup_esc) == (0 if combos <= 255 else ((t["tup"] >= 0) & ~np.isin(t["tup"], part.arrays["tup_hot"][:255])).sum())
        assert (int(part.view.n_tup_esc) > 0) == (combos > 255)
    assert _decoded("dict_300")[LINK][3]["n"] <= 1024, "more than UZ_PL_DICT_MIN combinations in a table of one span"
    part = _decoded("dict_edges")[LINK][1]
    assert np.nonzero(part.arrays["tup8"][:2048] == 255)[0].tolist() == [0, 1023, 1024, 2047]


def test_reach_of_the_sentinels():
    case = panel()["sentinels"]
    T, n = case.table, case.n
    d = _decoded("sentinels")
    md = (T.mate.astype(np.int64) - np.arange(n))[T.mate >= 0]
    assert {32767, -32767, 32768, -32768, 127, -127, 128, -128, 126, 1, 252, 253} <= set(md.tolist())
    assert {32767, -32767, -32768} <= set(T.tlen.tolist())
    qd = np.diff(T.qname.astype(np.int64))
    assert {32767, -32767, -32768, 127, -127, -128, 126} <= set(qd.tolist())
    st = np.diff(T.start.astype(np.int64))
    assert {32767, -32767, -32768, 32768} <= set(st.tolist())
    form, part, idx, t = d["d16/everything/end=None"]
    assert idx.size == n
    a = part.arrays
    # the real value 32767 travels in the column; -32767 (the no-mate value) and -32768 (the escape value) go through the escape list
    assert a["mate_d"][10] == 32767 and a["mate_d"][10 + 32767] == lm.D16_ESC and t["mate"][10 + 32767] == 10
    assert a["tlen_s"][200] == 32767 and a["tlen_s"][202] == lm.D16_ESC and t["tlen"][202] == -32768 and t["tlen"][201] == -32767
    form, part, idx, t = d["narrow8/everything/end=None"]
    a = part.arrays
    assert a["mate_d8"][400] == 127 and a["mate_d8"][400 + 127] == lm.D8S_ESC and a["mate_d8"][420] == 126 and a["mate_d8"][410] == lm.D8S_ESC
    assert (a["mate_d8"][:n] == lm.D8S_NONE).sum() == (T.mate < 0).sum()


def test_reach_of_the_wide_table_and_the_counts():
    d = _decoded("wide")
    form, part, idx, t = d[POINTS]
    assert part.view.qlow_pos_wide and part.view.bl_wide
    L = t["l_seq"].astype(int)
    um = t["umask"].astype(int)
    assert {257, 300, 480, 481} <= set(L.tolist())
    assert np.all(um[L == 481] == 0xFFFF) and ((um[L == 480] & 0x4000) != 0).any(), "481 bases travel as UZ_UMASK_ALL; unit 14 is the last a mask names"
    assert 255 in t["n_low"][L == 300].tolist(), "300 low bases: the count saturates"
    ns = sorted(panel()[k].n for k in panel() if k.startswith("count_"))
    assert ns == [1, 255, 256, 257, 1023, 1024, 1025, 1026, 1027, 2049] and {n % 4 for n in ns} == {0, 1, 2, 3}


def test_the_packer_chose_every_form():
    seen, cols = set(), set()
    for form, part, idx, t in _decoded("edges").values():
        seen.add(tuple(sorted(k for k in part.arrays if k.endswith(("_d", "_d8", "_s")))))
        cols |= set(part.arrays)
        cols.add("cigar_compact=%d" % part.view.cigar_compact)
    assert len(seen) == 5, seen
    assert {"tup8", "tup", "flag", "bl_qlow", "bl_pos", "qlow", "n_low", "tup_n_low", "seq2", "seq4", "end", "umask", "tup_umask", "pk_sums",
            "cigar_compact=0", "cigar_compact=1"} <= cols


def test_the_hand_edited_views_are_built_and_the_model_refuses_them_too():
    """tests/linkrefusals.py: every honest view decodes, every edited one contradicts itself for the model as well (the device's refusals are held
    in tests/test_link_cases_gpu.py)"""
    import linkrefusals
    assert set(linkrefusals.FLAG_OF) == {name for name, _ in linkrefusals.REFUSALS}
    for name, make in linkrefusals.REFUSALS:
        lm.decode(make(panel(), False))
        with pytest.raises(lm.LinkFormError):
            lm.decode(make(panel(), True))
            pytest.fail(name + ": the model decoded the edited view")
