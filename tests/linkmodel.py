"""A plain decoder of the link form of the alignment records, written from the text of include/uz_types.h (uz_reads_packed_view and the UZ_*
constants under it) and pack.hpp's uz_bam_endpos -- not from the device's header build, and without the product's own decoders (abi.wide_columns,
record_ends, small_columns, base_lists, base_qual_bits).  decode() gives what a table must hold once the device has expanded it; tests compare the
device's read-back (uz_reads_headers, uz_reads_columns, uz_reads_marks) and the source table with it, exactly."""
import numpy as np

# uz_types.h
AUX_DECODE_BAD, AUX_NO_SEQ, AUX_SIMPLE_SHIFT, AUX_SIMPLE_MASK = 4, 8, 4, 48
QLOW_LIST_MAX = 10
TUP8_SPAN, PK_SUMS, PK_SHIFT_LARGE, PK_SHIFT_SMALL = 1024, 11, 12, 10
UMASK_LISTED, UMASK_ALL = 0x8000, 0xFFFF
P8_SECOND, P8_MAX_DIST, P8_SECOND_TLEN, P8_NEW, P8_OLD = 0, 252, 253, 254, 255
D8S_ESC, D8S_NONE, D8_ESC, D16_ESC, D16_NONE = -128, -127, 255, -32768, -32767


class LinkFormError(ValueError):
    """the view contradicts itself (the model decodes honest views only)"""


def _need(ok, what):
    if not ok:
        raise LinkFormError(what)


def pk_shift(n):
    return PK_SHIFT_LARGE if (int(n) >> PK_SHIFT_LARGE) >= 4096 else PK_SHIFT_SMALL


def row_units(l_seq):
    return (np.asarray(l_seq).astype(np.int64) + 31) >> 5


def _has(held, name):
    return name in held.arrays and bool(getattr(held.view, name))


def _small(held, n):
    """flag, l_seq, n_cigar, mapq, aux, n_low, umask, bl_n per record: the plain columns, or through the dictionary (tup, or tup8 + tup_hot + tup_esc)"""
    a, v = held.arrays, held.view
    names = ("flag", "l_seq", "n_cigar", "mapq", "aux", "n_low", "umask")
    if not (_has(held, "tup") or _has(held, "tup8")):
        out = {k: (a[k][:n].copy() if _has(held, k) else None) for k in names}
        out["bl_n"] = a["bl_n"][:n].copy() if _has(held, "bl_n") else None
        return out
    n_tup = int(v.n_tup)
    if _has(held, "tup"):
        t = a["tup"][:n].astype(np.int64)
    else:
        t8 = a["tup8"][:n].astype(np.int64)
        t = a["tup_hot"][:256].astype(np.int64)[np.minimum(t8, 255)]
        esc = t8 == 255
        n_esc = int(v.n_tup_esc)
        _need(int(esc.sum()) == n_esc, "tup8: escapes and n_tup_esc differ")
        t[esc] = a["tup_esc"][:n_esc]
        off = a["tup_esc_off"][: (n + TUP8_SPAN - 1) // TUP8_SPAN + 1].astype(np.int64)
        per_span = np.add.reduceat(esc.astype(np.int64), np.arange(0, n, TUP8_SPAN)) if n else np.zeros(0, np.int64)
        _need(np.array_equal(np.diff(off), per_span) and off[0] == 0 and off[-1] == n_esc, "tup8: tup_esc_off")
    _need(n == 0 or (t.min() >= 0 and t.max() < n_tup), "dictionary index beyond n_tup")
    out = {k: (a["tup_" + k][:n_tup][t] if _has(held, "tup_" + k) else None) for k in names}
    if out["umask"] is None and _has(held, "umask"):
        out["umask"] = a["umask"][:n].copy()
    out["bl_n"] = a["tup_n_bl"][:n_tup][t] if _has(held, "tup_n_bl") else (a["bl_n"][:n].copy() if _has(held, "bl_n") else None)
    out["tup"] = t
    return out


def _escapes(held):
    v, a = held.view, held.arrays
    ne = int(v.n_esc16)
    key, val = a["esc16_key"][:ne].astype(np.int64), a["esc16_val"][:ne].astype(np.int64)
    _need(np.all(np.diff(key) > 0), "escape keys do not ascend")
    return key >> 2, key & 3, val


def _column_escapes(esc, col, n, marked, what):
    """the escaped values of one column, scattered to their records; the records the column marks must be the ones the list holds"""
    rec, c, val = esc
    sel = c == col
    _need(np.array_equal(rec[sel], np.nonzero(marked)[0]), "escape list and column %s disagree" % what)
    out = np.zeros(n, np.int64)
    out[rec[sel]] = val[sel]
    return out


def _cigars(held, n, sm):
    """every record's CIGAR words, the omitted simple words restored -> (flat words, offsets [n + 1], words that travelled per record)"""
    a, v = held.arrays, held.view
    n_cigar, l_seq, aux = (sm[k].astype(np.int64) for k in ("n_cigar", "l_seq", "aux"))
    code = ((aux & AUX_SIMPLE_MASK) >> AUX_SIMPLE_SHIFT) if v.cigar_compact else np.zeros(n, np.int64)
    _need(np.all(n_cigar[code > 0] == 1), "a simple-CIGAR code on a record with n_cigar != 1")
    travelled = np.where(code > 0, 0, n_cigar)
    _need(int(travelled.sum()) == int(v.n_cigar_total), "n_cigar_total")
    _need(int((code > 0).sum()) == int(v.n_cigar_omitted), "n_cigar_omitted")
    off = np.concatenate([[0], np.cumsum(n_cigar)])
    words = np.zeros(int(off[-1]), np.uint32)
    src = np.concatenate([[0], np.cumsum(travelled)])
    staged = a["cigar"]
    own = np.repeat(code == 0, n_cigar)
    words[own] = staged[: int(src[-1])]
    simple = np.nonzero(code > 0)[0]
    op = np.array([0, 0, 7, 8], np.int64)[code[simple]]  # UZ_AUX_SIMPLE_*: 1 / 2 / 3 = one M / = / X over l_seq bases
    words[off[simple]] = ((l_seq[simple] << 4) | op).astype(np.uint32)
    return words, off, travelled


def _ref_len(words, off, n):
    w = words.astype(np.int64)
    op = w & 15
    share = np.where((op == 0) | (op == 2) | (op == 3) | (op == 7) | (op == 8), w >> 4, 0)  # M D N = X
    cs = np.concatenate([[0], np.cumsum(share)])
    return cs[off[1:]] - cs[off[:-1]]


def decode(held):
    """-> dict: the table the view describes (see the module text of tests/test_link_model.py for the keys)"""
    a, v = held.arrays, held.view
    n = int(v.n_segs)
    sm = _small(held, n)
    for k in ("flag", "l_seq", "n_cigar", "mapq", "aux"):
        _need(sm[k] is not None, "no " + k)
    flag, l_seq, n_cigar, aux = (sm[k].astype(np.int64) for k in ("flag", "l_seq", "n_cigar", "aux"))
    lists = sm["n_low"] is not None
    _need(lists != _has(held, "qlow"), "exactly one of qlow / n_low")
    units_all = row_units(l_seq)
    has_seq = (aux & AUX_NO_SEQ) == 0
    words, cig_off, travelled = _cigars(held, n, sm)
    # ---- start, tlen, mate, qname
    idx = np.arange(n, dtype=np.int64)
    diff_form = _has(held, "start_d") or _has(held, "start_d8")
    first = second = new_name = np.zeros(n, bool)
    d_start = d_qname = np.zeros(n, np.int64)
    if not diff_form:
        start, tlen, mate, qname = (a[k][:n].astype(np.int64) for k in ("start", "tlen", "mate", "qname"))
    else:
        esc = _escapes(held)
        if _has(held, "start_d8"):
            sd = a["start_d8"][:n].astype(np.int64)
            marked = sd == D8_ESC
        else:
            sd = a["start_d"][:n].astype(np.int64)
            marked = sd == D16_ESC
        d_start = np.where(marked, _column_escapes(esc, 0, n, marked, "start"), sd)
        start = (np.cumsum(d_start) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
        if _has(held, "pair_d8"):
            p = a["pair_d8"][:n].astype(np.int64)
            first, second = (p >= 1) & (p <= P8_MAX_DIST), (p == P8_SECOND) | (p == P8_SECOND_TLEN)
            given, new, old = p == P8_SECOND_TLEN, p == P8_NEW, p == P8_OLD
            new_name = first | new
            e_tlen = _column_escapes(esc, 1, n, given | new | old, "pair_d8 (tlen)")
            e_mate = _column_escapes(esc, 2, n, new | old, "pair_d8 (mate)")
            e_name = _column_escapes(esc, 3, n, old, "pair_d8 (name id)")
            qname = np.cumsum(new_name) - 1  # a new name's id is the number of new names before it
            qname[old] = e_name[old]
            mate = np.where(new | old, e_mate, -1)
            tlen = np.where(given | new | old, e_tlen, 0)
            fi = np.nonzero(first)[0]
            fj = fi + p[fi]
            _need(fj.size == 0 or fj.max() < n, "a FIRST names a record beyond the table")
            _need(np.all(second[fj]) and np.unique(fj).size == fj.size and fj.size == int(second.sum()), "every SECOND is named by exactly one FIRST")
            mate[fi], mate[fj] = fj, fi
            qname[fj] = qname[fi]
            d_qname = new_name.astype(np.int64)
        else:
            if _has(held, "mate_d8"):
                md, qd = a["mate_d8"][:n].astype(np.int64), a["qname_d8"][:n].astype(np.int64)
                m_esc, m_none, q_esc = md == D8S_ESC, md == D8S_NONE, qd == D8S_ESC
            else:
                md, qd = a["mate_d"][:n].astype(np.int64), a["qname_d"][:n].astype(np.int64)
                m_esc, m_none, q_esc = md == D16_ESC, md == D16_NONE, qd == D16_ESC
            ts = a["tlen_s"][:n].astype(np.int64)
            t_esc = ts == D16_ESC
            tlen = np.where(t_esc, _column_escapes(esc, 1, n, t_esc, "tlen_s"), ts)
            mate = np.where(m_esc, _column_escapes(esc, 2, n, m_esc, "mate"), np.where(m_none, -1, idx + md))
            d_qname = np.where(q_esc, _column_escapes(esc, 3, n, q_esc, "qname"), qd)
            qname = np.cumsum(d_qname) & 0xFFFFFFFF
        _need(np.all((mate >= -1) & (mate < n)), "a mate beyond the table")
    # ---- end: the column, or htslib's bam_endpos (pack.hpp uz_bam_endpos)
    if _has(held, "end"):
        end = a["end"][:n].astype(np.int64)
    else:
        rl = _ref_len(words, cig_off, n)
        end = np.where(((flag & 4) != 0) | (n_cigar == 0), start + 1, start + np.maximum(rl, 1))
    if _has(held, "pair_d8"):
        span = np.where(given[fj], -tlen[fj], np.maximum(end[fi], end[fj]) - start[fi])
        tlen[fi], tlen[fj] = span, -span
    # ---- which units were staged
    masks = sm["umask"] is not None
    um = sm["umask"].astype(np.int64) if masks else np.full(n, UMASK_ALL, np.int64)
    if masks:
        _need(lists, "unit masks need the list form of the qualities")
        part = um != UMASK_ALL
        _need(np.all(units_all[part] <= 15) and np.all((um[part] >> units_all[part]) == 0), "a mask bit beyond the read's units")
    bl_n = sm["bl_n"].astype(np.int64) if sm["bl_n"] is not None else np.zeros(n, np.int64)
    listed = bl_n > 0
    _need(not listed.any() or (masks and _has(held, "seq2")), "a base list needs masks and seq2")
    _need(not np.any(listed & ((um == UMASK_ALL) | ~has_seq)), "a base list on a record without a mask or without bases")
    max_u = int(units_all.max()) if n else 0
    ucol = np.arange(max(1, max_u), dtype=np.int64)[None, :]
    staged = np.where((um == UMASK_ALL)[:, None], ucol < units_all[:, None], ((um[:, None] >> np.minimum(ucol, 15)) & 1).astype(bool) & (ucol < 15))
    # (base rows: the records that carry bases; quality rows of the plane form: every record)
    base_bits = staged & has_seq[:, None]
    b_rec, b_unit = np.nonzero(base_bits)
    unit_index = np.full(base_bits.shape, -1, np.int64)
    unit_index[b_rec, b_unit] = np.arange(b_rec.size)
    first_unit = np.concatenate([[0], np.cumsum(base_bits.sum(1))])
    b_rank = np.arange(b_rec.size) - first_unit[b_rec]
    rows = ~listed[b_rec]  # units that travelled as rows, back to back
    n_rows = int(rows.sum())
    _need(n_rows == int(v.n_seq_units) and b_rec.size - n_rows == int(v.n_bl_units), "n_seq_units / n_bl_units")  # (n_seq_units: the units in seq2 / seq4)
    _need(int(units_all.sum()) == int(v.n_row_units), "n_row_units")
    codes = np.zeros((b_rec.size, 32), np.uint8)
    k32 = np.arange(32)
    if _has(held, "seq4"):
        by = a["seq4"][: 16 * n_rows].reshape(n_rows, 16)
        codes[rows] = (by[:, k32 >> 1] >> np.where(k32 & 1, 0, 4)) & 15  # base k: byte k >> 1, high nibble when k is even
    elif n_rows or _has(held, "seq2"):
        by = a["seq2"][: 8 * n_rows].reshape(n_rows, 8)
        two = (by[:, k32 >> 2] >> (6 - 2 * (k32 & 3))) & 3  # base k: byte k >> 2, bits 7-6 for k & 3 == 0 down to bits 1-0
        codes[rows] = (1 << two).astype(np.uint8)  # A 0, C 1, G 2, T 3 -> BAM's 1, 2, 4, 8
    valid = (32 * b_unit[:, None] + k32[None, :]) < l_seq[b_rec][:, None]
    # the listed bases
    n_bl = int(bl_n.sum())
    e_rec = np.repeat(idx, bl_n)
    bl_pos = bl_at = np.zeros(0, np.int64)
    if n_bl or _has(held, "bl_pos"):
        _need(n_bl == int(v.n_bl), "n_bl")
        bl_pos = (a["bl_pos"][: 2 * n_bl].view(np.uint16)[:n_bl] if v.bl_wide else a["bl_pos"][:n_bl]).astype(np.int64)
        e = np.arange(n_bl)
        two = (a["bl_code"][e >> 2].astype(np.int64) >> (2 * (e & 3))) & 3
        _need(np.all(bl_pos < l_seq[e_rec]) and np.all((bl_pos >> 5) < 15), "a listed base beyond the read")
        at = unit_index[e_rec, bl_pos >> 5]
        _need(np.all(at >= 0), "a listed base outside the record's mask")
        same = e_rec[1:] == e_rec[:-1]
        _need(np.all(bl_pos[1:][same] > bl_pos[:-1][same]), "listed bases do not ascend")
        hit = np.zeros(b_rec.size, bool)
        hit[at] = True
        bl_at = at
        _need(np.all(hit[~rows]), "a unit of a listed record's mask holds no listed base")
        codes[at, bl_pos & 31] = (1 << two).astype(np.uint8)
    # the exceptions: every base that is not one of the four, in the units that were staged
    n_exc = int(v.n_exc) if _has(held, "seq2") else 0
    exc_used = np.zeros(n_exc, bool)
    if n_exc:
        xr, xp, xc = a["exc_rec"][:n_exc].astype(np.int64), a["exc_pos"][:n_exc].astype(np.int64), a["exc_code"][:n_exc]
        _need(np.all(xr < n) and np.all(xc <= 15), "an exception beyond the table / a code beyond 15")
        _need(np.all(has_seq[xr]) and np.all(xp < l_seq[xr]), "an exception on a record without bases / beyond the read")
        key = xr * 65536 + xp
        _need(np.all(np.diff(key) > 0), "exceptions do not ascend")
        xu = xp >> 5
        at = np.where(xu < base_bits.shape[1], unit_index[xr, np.minimum(xu, base_bits.shape[1] - 1)], -1)
        exc_used = at >= 0
        codes[at[exc_used], xp[exc_used] & 31] = xc[exc_used]
    codes[~valid] = 0
    # ---- the qualities
    blq = _has(held, "bl_qlow")
    if lists:
        n_low = sm["n_low"].astype(np.int64)
        qrow = has_seq & (n_low <= QLOW_LIST_MAX)
        own = np.where(qrow & ~(blq & listed), n_low, 0)  # quantity 3: the record's listed low-quality positions
        nq = int(own.sum())
        _need(nq == int(v.n_qlow_pos), "n_qlow_pos")
        qp = (a["qlow_pos"][: 2 * nq].view(np.uint16)[:nq] if v.qlow_pos_wide else a["qlow_pos"][:nq]).astype(np.int64)
        q_rec = np.repeat(idx, own)
        _need(np.all(qp < l_seq[q_rec]), "a low-quality position beyond the read")
        same = q_rec[1:] == q_rec[:-1]
        _need(np.all(qp[1:][same] > qp[:-1][same]), "low-quality positions do not ascend")
        qword = np.zeros(b_rec.size, np.uint32)
        qu = qp >> 5
        at = np.where(qu < base_bits.shape[1], unit_index[q_rec, np.minimum(qu, base_bits.shape[1] - 1)], -1)
        np.bitwise_or.at(qword, at[at >= 0], (np.uint32(1) << (qp[at >= 0] & 31).astype(np.uint32)))
        if blq:
            e = np.arange(n_bl)
            bit = (a["bl_qlow"][e >> 3].astype(np.int64) >> (e & 7)) & 1
            per = np.bincount(e_rec, weights=bit, minlength=n).astype(np.int64)
            _need(np.all(per[listed] == np.where(qrow[listed], n_low[listed], 0)), "bl_qlow: set bits and the record's count differ")
            at = unit_index[e_rec, bl_pos >> 5]
            on = bit == 1
            np.bitwise_or.at(qword, at[on], (np.uint32(1) << (bl_pos[on] & 31).astype(np.uint32)))
        q_rows = dict(q_rec=b_rec, q_unit=b_unit, q_rank=b_rank, q_word=qword, q_has=qrow[b_rec])
        n_low_out = n_low
    else:
        # the plane: rows of ALL records, 4 bytes per unit, bit k & 7 of byte k >> 3
        q_rec, q_unit = np.nonzero(ucol < units_all[:, None])
        nu = q_rec.size
        qword = a["qlow"][: 4 * nu].view("<u4").astype(np.uint32)
        firstq = np.concatenate([[0], np.cumsum(units_all)])
        left = np.clip(l_seq[q_rec] - 32 * q_unit, 0, 32)
        keep = np.where(left >= 32, 0xFFFFFFFF, (np.int64(1) << left) - 1).astype(np.uint32)
        qword = qword & keep
        pop = np.array([bin(int(x)).count("1") for x in qword], np.int64)
        n_low_out = np.minimum(np.bincount(q_rec, weights=pop, minlength=n).astype(np.int64), 255)
        own = np.zeros(n, np.int64)
        q_rows = dict(q_rec=q_rec, q_unit=q_unit, q_rank=np.arange(nu) - firstq[q_rec], q_word=qword, q_has=np.ones(nu, bool))
    # ---- the spans' shares (uz_types.h pk_sums) and their escapes
    shift = pk_shift(n)
    nsp = (n + (1 << shift) - 1) >> shift
    staged_units = base_bits.sum(1)
    q = np.zeros((n, PK_SUMS), np.int64)
    q[:, 0], q[:, 1] = n_cigar, units_all
    q[:, 2] = np.where(listed, 0, staged_units)
    q[:, 3] = own
    q[:, 4] = travelled
    if diff_form:
        q[:, 5], q[:, 6] = d_start, d_qname
    q[:, 7], q[:, 8] = np.where(listed, staged_units, 0), bl_n
    q[:, 9], q[:, 10] = first, second
    edges = np.arange(0, n, 1 << shift)
    share = np.add.reduceat(q, edges, axis=0) if n else np.zeros((0, PK_SUMS), np.int64)
    share[:, 5] &= 0xFFFFFFFF
    share[:, 6] &= 0xFFFFFFFF
    esc_share = np.bincount(_escapes(held)[0] >> shift, minlength=nsp)[:nsp] if diff_form else np.zeros(nsp, np.int64)
    first_bl = np.concatenate([[0], np.cumsum(share[:, 8])])[:-1] if nsp else np.zeros(0, np.int64)
    stored_umask = np.where(listed, um | UMASK_LISTED, um).astype(np.uint16)
    out = dict(n=n, start=start.astype(np.int32), end=end.astype(np.int32), tlen=tlen.astype(np.int32), mate=mate.astype(np.int32),
               qname=qname.astype(np.uint32), flag=flag.astype(np.uint16), mapq=sm["mapq"].astype(np.uint8), aux=aux.astype(np.uint8),
               fm=(flag | (sm["mapq"].astype(np.int64) << 16) | (aux << 24)).astype(np.uint32),
               l_seq=l_seq.astype(np.uint16), n_cigar=n_cigar.astype(np.uint16), cigar=words, cigar_off=cig_off,
               n_low=n_low_out.astype(np.uint8), umask=stored_umask, listed=listed, has_seq=has_seq, lists=lists,
               b_rec=b_rec, b_unit=b_unit, b_rank=b_rank, codes=codes, valid=valid, exc_used=exc_used, bl_rec=e_rec, bl_pos=bl_pos, bl_at=bl_at, bl_quals=blq,
               span_share=share, span_esc=esc_share, span_first_bl=first_bl, tup=sm.get("tup"), pk_shift=shift)
    out.update(q_rows)
    if _has(held, "pk_sums"):  # the packer's own sums: the running sums of the shares, the last row the totals
        S = a["pk_sums"][: PK_SUMS * (nsp + 1)].reshape(nsp + 1, PK_SUMS).astype(np.int64)
        run = np.concatenate([np.zeros((1, PK_SUMS), np.int64), np.cumsum(share, axis=0)])
        run[:, 5] &= 0xFFFFFFFF
        run[:, 6] &= 0xFFFFFFFF
        S = S.copy()
        S[:, 5] &= 0xFFFFFFFF
        S[:, 6] &= 0xFFFFFFFF
        _need(int(v.n_pk_spans) == nsp and np.array_equal(S, run), "pk_sums are not the running sums of the spans' shares")
    return out


UZ_NO_QLOW_OFF = 0xFFFFFFFF


def readback_differences(t, hdr, cols, marks):
    """What the device holds of a table (HipEngine.reads_headers, reads_columns, reads_marks) against decode()'s table `t`: the names of the parts
    that differ (none: equal).  Units are found as the readers find them (uz_unit_of): sq_off + the unit's rank in the mask.  Padding nibbles
    beyond l_seq are not compared (the two-bit expansion writes code 1 there and no reader looks), nor is qoff of a record without a quality row."""
    bad = []
    n = t["n"]

    def eq(name, got, want):
        if not np.array_equal(np.asarray(got), np.asarray(want)):
            bad.append(name)
    for k in ("start", "end", "tlen", "mate", "qname"):
        eq(k, hdr[k], t[k])
    for k in ("fm", "l_seq", "n_cigar"):
        eq(k, cols[k], t[k])
    eq("nlow", marks["nlow"], t["n_low"])
    eq("umask", marks["umask"], t["umask"])
    # the CIGAR store at cigar_off
    nc = t["n_cigar"].astype(np.int64)
    total = int(nc.sum())
    at = np.repeat(cols["cigar_off"].astype(np.int64)[:n], nc) + (np.arange(total) - np.repeat(t["cigar_off"][:-1], nc))
    if total and (at.max() >= cols["cigar"].size or at.min() < 0):
        bad.append("cigar_off beyond the store")
    else:
        eq("cigar", cols["cigar"][at], t["cigar"])
    # every base below l_seq of every staged unit
    row = cols["sq_off"].astype(np.int64)[t["b_rec"]] + t["b_rank"]
    n_units = cols["seq4"].size // 16
    if row.size and (row.max() >= n_units or row.min() < 0):
        bad.append("sq_off beyond the base rows")
    else:
        if np.unique(row).size != row.size:
            bad.append("two units share a base row")
        k32 = np.arange(32)
        by = cols["seq4"].reshape(-1, 16)[row]
        got = (by[:, k32 >> 1] >> np.where(k32 & 1, 0, 4)) & 15
        if not np.array_equal(got[t["valid"]], t["codes"][t["valid"]]):
            bad.append("bases")
    # the whole quality word of every staged unit of a record that has a quality row
    has = t["q_has"]
    qrow = cols["qoff"].astype(np.int64)[t["q_rec"][has]] + t["q_rank"][has]
    if qrow.size and (qrow.max() >= cols["qlow"].size or qrow.min() < 0):
        bad.append("qoff beyond the plane")
    else:
        eq("quality words", cols["qlow"][qrow], t["q_word"][has])
    return bad
