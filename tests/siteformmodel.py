"""The link forms of a site window decoded from the text of include/uz_types.h alone: the compact site form (uz_sites_view.pos_d16 ...),
the eight-bit and the het form of a trio's nine columns (uz_family_view.ref_depth8 ..., het9 ...) and the genotype byte with the library's
complex bit.  Plain numpy, one statement per sentence of the header; it calls no unpacker of the package and shares no code with one, so
that the device's expansion (k_sites_expand, k_widen8, k_fold_complex) and the host twin (uz_sites_unpack) can both be held to it."""
import numpy as np

SPAN = 1024  # UZ_SITE_SPAN
D16_LIMIT = 32768  # UZ_POS_D16_LIMIT
BASE3 = np.frombuffer(b"\0ACGTN" + b"NN", np.uint8)  # UZ_BASE3_CODES; "the codes 6 and 7 as 'N'"
U8_MISSING, U8_SEE_WIDE = 254, 255
HET = 1  # UZ_HET


def n_spans(n):
    return (n + SPAN - 1) // SPAN


def site_columns(pos_d16, bases8, span_pos, esc_idx, esc_val, esc_off, n):
    """-> (pos i32, sflags u8, ref_base u8, alt_base u8).  "pos[i] is the value of the last anchor at or before i within its span (the
    span's first site, or an escape) plus the pos_d16 of the sites after that anchor up to i" -- in 32 bits that wrap, since an anchor
    may hold any int32.  pos_d16 at an anchor is "anything": never read.  esc_idx / esc_val may be None when esc_off names no escape."""
    d = np.asarray(pos_d16, np.uint16)[:n].astype(np.uint64)
    b = np.asarray(bases8, np.uint8)[:n]
    off = np.asarray(esc_off, np.int64)
    assert off.size == n_spans(n) + 1 and off[0] == 0
    pos = np.zeros(n, np.uint32)
    for s in range(n_spans(n)):
        lo, hi = s * SPAN, min(n, (s + 1) * SPAN)
        value = np.zeros(hi - lo, np.uint64)  # of an anchor
        anchor = np.zeros(hi - lo, bool)
        anchor[0], value[0] = True, np.uint32(np.int32(span_pos[s]))  # "span_pos[s]: pos of the span's first site"
        for e in range(int(off[s]), int(off[s + 1])):  # "pos_esc_off[s] = first escape of span s"
            l = int(esc_idx[e]) - lo
            assert 0 < l < hi - lo, "an escape outside its span or at its first site"
            anchor[l], value[l] = True, np.uint32(np.int32(esc_val[e]))
        last = np.maximum.accumulate(np.where(anchor, np.arange(hi - lo), 0))  # the last anchor at or before every site
        run = np.cumsum(np.where(anchor, 0, d[lo:hi]), dtype=np.uint64)  # differences summed; an anchor's own is not read
        pos[lo:hi] = ((value[last] + run - run[last]) & 0xFFFFFFFF).astype(np.uint32)
    # "bases8[i]: code of ref_base | code of alt_base << 3 | complex << 6"; bit 7 is ignored
    return pos.view(np.int32), (b >> 6 & 1).astype(np.uint8), BASE3[b & 7], BASE3[b >> 3 & 7]


def widen8(cols8):
    """the nine eight-bit columns (rd k d m, ad k d m, gq k d m: u8 [9][n]) -> (u16 [9][n], open: bool [9][n]).  "A depth byte below 254 is
    the depth; 254 = missing; 255 = the site stands in the wide list" -- there the 16-bit columns "may hold anything": those cells, and no
    others, are open.  "A quality byte below 255 is min(floor(GQ), 254); 255 = missing"."""
    c = np.asarray(cols8, np.uint8).reshape(9, -1)
    out = c.astype(np.uint16)
    out[:6][c[:6] == U8_MISSING] = 0xFFFF
    out[6:][c[6:] == 255] = 0xFFFF
    open_ = np.zeros(c.shape, bool)
    open_[:6] = c[:6] == U8_SEE_WIDE
    return out, open_


def het_columns(gt, het9, het_span_off):
    """the het form -> (u16 [9][n], open [9][n]): "het9[9 * e + q]: het site e in site order, q = rd kid, dad, mom, ad ..., gq ..., in the
    eight-bit encoding"; kid-het = "(gt & 3) == UZ_HET on this view's own gt"; "zeros for all others"; "het_span_off[s]: kid-het sites
    before span s"."""
    gt = np.asarray(gt, np.uint8)
    n = gt.size
    het = np.nonzero((gt & 3) == HET)[0]
    h9 = np.asarray(het9, np.uint8)[: 9 * het.size].reshape(-1, 9)
    assert h9.shape[0] == het.size
    off = np.asarray(het_span_off, np.int64)
    assert np.array_equal(off, np.searchsorted(het, np.arange(n_spans(n) + 1) * SPAN))
    w, o = widen8(h9.T)
    out, open_ = np.zeros((9, n), np.uint16), np.zeros((9, n), bool)
    out[:, het], open_[:, het] = w, o
    return out, open_


def folded_gt(gt, sflags):
    """the genotype byte as the device holds it: "bit 6 is written by the library (complex flag)", bit 7 is dropped"""
    return ((np.asarray(gt, np.uint8) & 0x3F) | ((np.asarray(sflags, np.uint8) & 1) << 6)).astype(np.uint8)
