"""Honest views of the panel (tests/linkcases.py) with ONE column edited by hand: what the header build must refuse, with the code and the sentence
of uz_check_upload_flag.  Every edit keeps an unchecked decode inside the table's own buffers: the moved position or index names an existing unit or
word, the view's totals and span sums follow the edit where it moves them -- a missing check shows as a wrong table or a missing error, never as a
stray write.  make(cases, broken) -> the view, honest (broken = False) or edited."""
import numpy as np

import linkmodel as lm
from unfazed_amd import io_native

POINTS16 = "pair8/points/tup8=0/bl=1/bq=1"      # the link form with the 16-bit dictionary index (the span sums can be counted again after an edit)
ROWS16 = "pair8/points/tup8=0/bl=0/bq=0"        # ... every record's staged units as rows, its low-quality positions in qlow_pos
LINK16 = "pair8/everything/tup8=0/bl=1/bq=1"

# name -> (flag of uz_check_upload_flag, the head of its sentence)
SENTENCE = {3: "exc_* columns of the reads view", 4: "qlow_pos / bl_qlow of the reads view", 5: "umask of the reads view", 6: "aux of the reads view",
            7: "mate_d / esc16_* of the reads view", 1: "n_cigar_total / n_row_units of the reads view do not match its columns"}


def _fresh(cases, case, form):
    import linkcases as lc
    c = cases[case]
    f = {x[0]: x for x in lc.form_list(c, every=True)}[form]
    return lc.select(c, f)[0]


def _grow(part, name, nbytes):
    """the column `name` in a larger array of its own (what lay in it stays where it was)"""
    old = part.arrays[name]
    new = np.zeros(old.nbytes + nbytes, np.uint8)
    new[: old.nbytes] = old.view(np.uint8)
    part.arrays[name] = new.view(old.dtype) if new.nbytes % old.dtype.itemsize == 0 else new
    setattr(part.view, name, part.arrays[name].ctypes.data)


def _combination(part, ok):
    """a dictionary entry in use that ok(entry index) accepts, and how many records carry it"""
    t = lm._small(part, int(part.view.n_segs))["tup"]
    cnt = np.bincount(t, minlength=int(part.view.n_tup))
    for c in np.nonzero(cnt)[0]:
        if ok(int(c)):
            return int(c), int(cnt[c])
    raise AssertionError("the panel holds no such combination")


def mask_bit_beyond_the_units(cases, broken):
    part = _fresh(cases, "edges", POINTS16)
    a = part.arrays
    c, cnt = _combination(part, lambda c: a["tup_l_seq"][c] == 151 and a["tup_umask"][c] != 0xFFFF and a["tup_n_bl"][c] == 0 and not (a["tup_aux"][c] & 8) and a["tup_umask"][c])
    if broken:
        a["tup_umask"][c] |= 1 << 5          # a 151-base read has units 0 .. 4
        part.view.n_seq_units += cnt         # (the rows the mask now claims exist: the view's total, the span sums and the row store follow)
        _grow(part, "seq2", 8 * cnt)
        io_native.block_sums(part)
    return part


def mask_on_a_481_base_read(cases, broken):
    part = _fresh(cases, "wide", POINTS16)
    a = part.arrays
    c, cnt = _combination(part, lambda c: a["tup_l_seq"][c] == 481 and not (a["tup_aux"][c] & 8))
    assert a["tup_umask"][c] == 0xFFFF
    if broken:
        a["tup_umask"][c] = 0x7FFF           # fifteen of its sixteen units
        part.view.n_seq_units -= cnt
        io_native.block_sums(part)
    return part


def simple_code_on_two_words(cases, broken):
    part = _fresh(cases, "room_cigar", LINK16)
    a = part.arrays
    c, cnt = _combination(part, lambda c: a["tup_n_cigar"][c] == 2 and a["tup_mapq"][c] == 33)
    assert cnt == 1
    if broken:
        a["tup_aux"][c] |= 1 << lm.AUX_SIMPLE_SHIFT
        part.view.n_cigar_total -= 2 * cnt   # (the words such a record now leaves at home: the view's two totals still add up to the plain total)
        part.view.n_cigar_omitted += 2 * cnt
        io_native.block_sums(part)
    return part


def _exception_of(part, t, want_len=151):
    ok = np.nonzero(t["exc_used"] & (t["l_seq"][part.arrays["exc_rec"][: t["exc_used"].size]] == want_len))[0]
    return int(ok[0])


def exception_on_a_record_without_bases(cases, broken):
    part = _fresh(cases, "edges", POINTS16)
    t = lm.decode(part)
    if broken:
        e = _exception_of(part, t)
        part.arrays["exc_rec"][e] = int(np.nonzero(~t["has_seq"] & (t["l_seq"] == 151))[0][0])
    return part


def exception_beyond_the_read(cases, broken):
    part = _fresh(cases, "edges", POINTS16)
    t = lm.decode(part)
    if broken:
        part.arrays["exc_pos"][_exception_of(part, t)] = 151  # (bases 128 .. 159 share a unit: the position names an existing nibble)
    return part


def exception_code_16(cases, broken):
    part = _fresh(cases, "edges", POINTS16)
    t = lm.decode(part)
    if broken:
        part.arrays["exc_code"][_exception_of(part, t)] = 16
    return part


def _own_positions(t):
    """first entry and count of every record's share of qlow_pos (quantity 3 of uz_types.h pk_sums)"""
    rec_own = np.where(t["has_seq"] & (t["n_low"] <= lm.QLOW_LIST_MAX) & ~(t["bl_quals"] & t["listed"]), t["n_low"].astype(np.int64), 0)
    return np.concatenate([[0], np.cumsum(rec_own)]), rec_own


def low_positions_not_ascending(cases, broken):
    part = _fresh(cases, "edges", ROWS16)
    t = lm.decode(part)
    off, own = _own_positions(t)
    if broken:
        k = int(np.nonzero(own >= 2)[0][0])
        qp = part.arrays["qlow_pos"]
        qp[off[k]], qp[off[k] + 1] = qp[off[k] + 1], qp[off[k]]
    return part


def low_position_beyond_the_read(cases, broken):
    part = _fresh(cases, "edges", ROWS16)
    t = lm.decode(part)
    off, own = _own_positions(t)
    if broken:
        k = int(np.nonzero((own >= 1) & (t["l_seq"] == 151))[0][0])
        part.arrays["qlow_pos"][off[k] + own[k] - 1] = 155  # (bit 27 of the word of bases 128 .. 159)
    return part


def one_quality_bit_more_than_the_count(cases, broken):
    part = _fresh(cases, "edges", POINTS16)
    assert "bl_qlow" in part.arrays
    if broken:
        bits = np.unpackbits(part.arrays["bl_qlow"][: (int(part.view.n_bl) + 7) // 8], bitorder="little")[: int(part.view.n_bl)]
        e = int(np.nonzero(bits == 0)[0][7])
        part.arrays["bl_qlow"][e >> 3] |= 1 << (e & 7)
    return part


def _escaped_mate(part, value, broken):
    ne = int(part.view.n_esc16)
    key = part.arrays["esc16_key"][:ne]
    if broken:
        e = int(np.nonzero((key & np.uint64(3)) == 2)[0][0])
        part.arrays["esc16_val"][e] = value
    return part


def escaped_mate_of_n(cases, broken):
    part = _fresh(cases, "edges", LINK16)
    return _escaped_mate(part, int(part.view.n_segs), broken)


def escaped_mate_of_minus_two(cases, broken):
    return _escaped_mate(_fresh(cases, "edges", LINK16), -2, broken)


def cigar_total_off_by_one(cases, broken):
    part = _fresh(cases, "edges", LINK16)
    part.view.pk_sums, part.view.n_pk_spans = None, 0  # (the device counts for itself: the packer's totals row would be refused before the build)
    if broken:
        _grow(part, "cigar", 4)
        part.view.n_cigar_total += 1
    return part


REFUSALS = [("mask_bit_beyond_the_units", mask_bit_beyond_the_units), ("mask_on_a_481_base_read", mask_on_a_481_base_read),
            ("simple_code_on_two_words", simple_code_on_two_words), ("exception_on_a_record_without_bases", exception_on_a_record_without_bases),
            ("exception_beyond_the_read", exception_beyond_the_read), ("exception_code_16", exception_code_16),
            ("low_positions_not_ascending", low_positions_not_ascending), ("low_position_beyond_the_read", low_position_beyond_the_read),
            ("one_quality_bit_more_than_the_count", one_quality_bit_more_than_the_count), ("escaped_mate_of_n", escaped_mate_of_n),
            ("escaped_mate_of_minus_two", escaped_mate_of_minus_two), ("cigar_total_off_by_one", cigar_total_off_by_one)]
FLAG_OF = dict(mask_bit_beyond_the_units=5, mask_on_a_481_base_read=5, simple_code_on_two_words=6, exception_on_a_record_without_bases=3,
               exception_beyond_the_read=3, exception_code_16=3, low_positions_not_ascending=4, low_position_beyond_the_read=4,
               one_quality_bit_more_than_the_count=4, escaped_mate_of_n=7, escaped_mate_of_minus_two=7, cigar_total_off_by_one=1)
