// vcf_row.hpp -- one record line of a DNM VCF rewritten into a line of the annotated VCF (unfazed.py: write_vcf_output over io_vcf.read_vcf;
// reference unfazed.py:337-441).  __host__ __device__: k_vcfout_size / k_vcfout_fill (k_vcfout.hip) and tests/vcf_row_main.cpp run this very body.
//
// The body is written for a group of LANES lanes that share one record (the kernels: a wavefront; the host program: one lane).  The line is
// streamed 16 * LANES bytes a step, one 16-byte load per lane.  `W` gives the lane index and the cross-lane steps (shift up, broadcast, any);
// everything else is lane-private or uniform.
//
//   line     the eight fixed columns unchanged, FORMAT + ":UOPS:UET", every sample column + [":." padding] + ":<uops>:<uet>", '\n'
//   padding  a column with fewer ':'-pieces than FORMAT is padded with ":." up to FORMAT's piece count; a longer column is not cut
//   tail     ":-1:-1" unless the cell's column has an annotation AND the cell's genotype code, read from the cell's text at FORMAT's GT slot,
//            is HET (1) or HOM_ALT (3); a column that does not reach the slot, or a FORMAT without GT, is UNKNOWN
//   GT       an applied annotation with gt code 1 / 2 replaces the GT piece by "1|0" / "0|1" (the piece's length may change); code 0 leaves it
//   numbers  uops -1 .. 999 999 and uet -1 .. 6 as plain decimal digits ("%g" of such an integer)
//
// HANDED BACK (the record's flag is set, its length is 0, nothing is written; the host writes it with its per-record code):
//   a GT piece outside the genotype grammar -- vcf_cell.hpp's alleles (1-3 digits or "."), held for EVERY allele of the piece since read_vcf
//   converts them all; an empty piece; a count of sample columns that differs from the header's; a line without FORMAT or whose FORMAT names
//   GT twice (the caller's flag: uz_vr_format); an annotation with uops outside [-1, 999 999], uet outside -1 .. 6, a gt code above 2, a column
//   at or beyond n_samples, or columns that do not strictly ascend; a line that holds a '\r' (the host's text mode reads it as a line end).
//
// How a lane knows where its bytes go: out = in + shift, and shift grows at the TERMINATORS -- the tab behind FORMAT (9 bytes), the tab or
// line end behind a cell (padding + tail) and the end of a rewritten GT piece (3 - its length).  A step runs three scans over the lanes: tabs
// (the cell a lane starts in), ':' since the last tab (the piece it starts in) and, after a lane-private walk that sizes the insertions of the
// lane's own terminators, the insertions (the shift it starts with).  No table of cells is kept anywhere: a lane that needs more of a cell than
// its own 16 bytes -- the GT piece behind its terminator, the genotype of an ANNOTATED cell -- reads the text again, which lies in the caches.
//
// Size and fill are ONE walk (uz_vcf_row_walk<FILL>): the fill pass returns the bytes it walked, and its caller holds them against the sized
// length (UZ_VR_F_SIZE).  Every store of the fill pass is held inside the record's sized length as well.
#pragma once
#include <stdint.h>
#include <string.h>

#include "vcf_cell.hpp"

#if defined(__HIPCC__)
#define UZ_VR_HD __host__ __device__ __forceinline__
#else
#define UZ_VR_HD inline
#endif

#define UZ_VR_F_SIZE 1u /* a record's written bytes differ from its sized length (or the fill pass met a record it would hand back) */

#define UZ_VR_UOPS_MAX 999999
#define UZ_VR_UET_MAX 6

// one lane: the host program's group
struct UzVrLane1 {
    static constexpr uint32_t LANES = 1;
    UZ_VR_HD uint32_t lane() const { return 0; }
    UZ_VR_HD uint32_t shfl_up(uint32_t v, uint32_t) const { return v; }
    UZ_VR_HD uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    UZ_VR_HD bool any(bool v) const { return v; }
};

struct UzVrRec { // a record as the walk takes it; offsets into the chunk's text
    uint32_t line_at, fmt_end, line_end; // fmt_end: the tab behind FORMAT (the first sample column starts at fmt_end + 1)
    int32_t n_fmt, gt_slot;              // FORMAT's pieces, the piece that is GT (-1: none)
    uint32_t ann0, ann1;                 // the record's annotations: [ann0, ann1) of the chunk's table
    uint32_t hand_back;                  // the caller hands the record back itself
};

struct UzVrAnn { // the chunk's annotations
    const int32_t *col;
    const uint8_t *gt;
    const int32_t *uops;
    const int8_t *uet;
};

// FORMAT of a line whose sample columns start at samp_at (text[samp_at - 1] is a tab, line_at < samp_at): its pieces, the first piece that is
// "GT" (-1: none) -> false when GT is named more than once
UZ_VR_HD bool uz_vr_format(const uint8_t *text, uint64_t line_at, uint64_t samp_at, int32_t &n_fmt, int32_t &gt_slot) {
    const uint64_t e = samp_at - 1;
    uint64_t a = e;
    while (a > line_at && text[a - 1] != '\t') a--;
    int32_t k = 0, n_gt = 0;
    gt_slot = -1;
    uint64_t s = a;
    for (uint64_t i = a; i <= e; i++) {
        if (i < e && text[i] != ':') continue;
        if (i - s == 2 && text[s] == 'G' && text[s + 1] == 'T') {
            if (n_gt == 0) gt_slot = k;
            n_gt++;
        }
        k++;
        s = i + 1;
    }
    n_fmt = k;
    return n_gt <= 1;
}

// the record of a line [line_at, line_end) whose sample columns start at samp_at (line_end: none), offsets relative to t0.  Handed back by this
// very function: a line without a sample column (or without FORMAT), a FORMAT that names GT twice
UZ_VR_HD UzVrRec uz_vr_rec(const uint8_t *text, uint64_t t0, uint64_t line_at, uint64_t samp_at, uint64_t line_end) {
    UzVrRec R;
    R.line_at = (uint32_t)(line_at - t0); R.line_end = (uint32_t)(line_end - t0);
    R.fmt_end = R.line_at; R.n_fmt = 0; R.gt_slot = -1;
    R.ann0 = R.ann1 = 0;
    R.hand_back = 1;
    if (samp_at < line_end && samp_at > line_at && text[samp_at - 1] == '\t') {
        R.fmt_end = (uint32_t)(samp_at - 1 - t0);
        if (uz_vr_format(text, line_at, samp_at, R.n_fmt, R.gt_slot)) R.hand_back = 0;
    }
    return R;
}

// the genotype code of the piece [a, b) -> false: outside the grammar.  uz_vc_gt's code of the first two alleles; every further allele is held
// to the allele grammar too
UZ_VR_HD bool uz_vr_gt(const uint8_t *p, uint32_t a, uint32_t b, uint32_t &code) {
    if (!uz_vc_gt(p, a, b, code)) return false;
    uint32_t i = a, n = 0;
    for (;;) {
        int32_t v;
        if (!uz_vc_allele(p, i, b, v)) return false;
        n++;
        if (i >= b) break;
        i++; // the separator
    }
    return n >= 1;
}

UZ_VR_HD uint32_t uz_vr_digits(int32_t v) { // characters of "%d" for -1 .. 999 999
    if (v < 0) return 2;
    uint32_t d = 1;
    for (uint32_t u = (uint32_t)v; u >= 10u; u /= 10u) d++;
    return d;
}

// the annotation of column c among the record's (ascending) -> its index, or -1
UZ_VR_HD int32_t uz_vr_find(const UzVrAnn &A, const UzVrRec &R, int32_t c) {
    uint32_t a = R.ann0, b = R.ann1;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (A.col[m] < c) a = m + 1; else b = m;
    }
    return a < R.ann1 && A.col[a] == c ? (int32_t)a : -1;
}

UZ_VR_HD bool uz_vr_is_end(const uint8_t *T, const UzVrRec &R, uint32_t q) { return q >= R.line_end || T[q] == '\t'; }

// the GT piece that holds (or ends at) position p of a sample cell: [gs, ge)
UZ_VR_HD void uz_vr_gt_piece(const uint8_t *T, const UzVrRec &R, uint32_t p, uint32_t &gs, uint32_t &ge) {
    gs = p;
    while (gs > R.fmt_end + 1 && T[gs - 1] != ':' && T[gs - 1] != '\t') gs--;
    ge = p;
    while (!uz_vr_is_end(T, R, ge) && T[ge] != ':') ge++;
}

// the genotype code of the cell that ends at e (a tab or the line end) -> false: the cell does not reach the GT slot, or its piece is outside
// the grammar (which hands the record back where the piece's own terminator is walked)
UZ_VR_HD bool uz_vr_cell_gt(const uint8_t *T, const UzVrRec &R, uint32_t e, uint32_t &code) {
    if (R.gt_slot < 0) return false;
    uint32_t s = e;
    while (s > R.fmt_end + 1 && T[s - 1] != '\t') s--;
    int32_t k = 0;
    uint32_t a = s;
    for (uint32_t i = s; i <= e; i++) {
        if (i < e && T[i] != ':') continue;
        if (k == R.gt_slot) return uz_vr_gt(T, a, i, code);
        k++;
        a = i + 1;
    }
    return false;
}

// does the annotation `a` rewrite the GT piece [gs, ge)?
UZ_VR_HD bool uz_vr_rewrites(const uint8_t *T, const UzVrAnn &A, int32_t a, uint32_t gs, uint32_t ge) {
    if (a < 0 || A.gt[a] < 1 || A.gt[a] > 2) return false;
    uint32_t code = 2;
    return uz_vr_gt(T, gs, ge, code) && (code == 1u || code == 3u);
}

struct UzVrState { // where a lane stands: the cell (-1: the fixed columns and FORMAT), the ':' seen in it, out - in
    int32_t cell;
    uint32_t colons;
    uint32_t shift;
};

template <bool FILL>
UZ_VR_HD void uz_vr_put(uint8_t *out, uint32_t limit, uint32_t o, uint8_t ch) {
    if (FILL && o < limit) out[o] = ch;
}
template <bool FILL>
UZ_VR_HD void uz_vr_put_int(uint8_t *out, uint32_t limit, uint32_t o, int32_t v) { // ':' and the number
    uz_vr_put<FILL>(out, limit, o, ':');
    if (!FILL) return;
    if (v < 0) { uz_vr_put<FILL>(out, limit, o + 1, '-'); uz_vr_put<FILL>(out, limit, o + 2, '1'); return; }
    const uint32_t d = uz_vr_digits(v);
    uint32_t u = (uint32_t)v;
    for (uint32_t k = d; k >= 1; k--, u /= 10u) uz_vr_put<FILL>(out, limit, o + k, (uint8_t)('0' + u % 10u));
}

// The lane-private walk over the lane's 16 bytes [at, at + 16): `lo`, `hi` hold them (little endian).  st: the lane's state at `at`, moved to
// at + 16.  FILL: the bytes and the insertions are written at out[p - line_at + shift].  hb: raised on a record to hand back.
template <bool FILL>
UZ_VR_HD void uz_vr_lane_walk(const uint8_t *T, const UzVrRec &R, const UzVrAnn &A, int32_t n_samples, uint32_t at, uint64_t lo, uint64_t hi, UzVrState &st,
                              uint8_t *out, uint32_t limit, bool &hb) {
    int32_t skip = -1; // the GT piece the lane stands in: -1 not looked at, 0 copied, 1 rewritten (its bytes are not copied)
    const bool has_ann = R.ann1 > R.ann0;
    for (uint32_t k = 0; k < 16; k++, lo = (lo >> 8) | (hi << 56), hi >>= 8) {
        const uint32_t p = at + k;
        if (p < R.line_at || p > R.line_end) continue;
        const uint8_t ch = (uint8_t)(lo & 0xFFu);
        const bool eol = p == R.line_end;
        if (!eol && ch == '\r') hb = true;
        const bool in_gt = st.cell >= 0 && R.gt_slot >= 0 && st.colons == (uint32_t)R.gt_slot;
        const bool term = p >= R.fmt_end && (eol || ch == '\t');
        if (in_gt && (term || ch == ':')) { // the GT piece ends here
            uint32_t gs, ge, code = 2;
            uz_vr_gt_piece(T, R, p, gs, ge);
            if (!uz_vr_gt(T, gs, p, code)) hb = true;
            else if (has_ann) {
                const int32_t a = uz_vr_find(A, R, st.cell);
                if (a >= 0 && A.gt[a] >= 1 && A.gt[a] <= 2 && (code == 1u || code == 3u)) {
                    const uint32_t o = gs - R.line_at + st.shift;
                    uz_vr_put<FILL>(out, limit, o, A.gt[a] == 1 ? '1' : '0');
                    uz_vr_put<FILL>(out, limit, o + 1, '|');
                    uz_vr_put<FILL>(out, limit, o + 2, A.gt[a] == 1 ? '0' : '1');
                    st.shift += 3u - (p - gs);
                }
            }
        }
        if (term) {
            uint32_t o = p - R.line_at + st.shift;
            if (st.cell < 0) { // FORMAT
                const char *s = ":UOPS:UET";
                for (uint32_t b = 0; b < 9; b++) uz_vr_put<FILL>(out, limit, o + b, (uint8_t)s[b]);
                o += 9;
            } else {
                const uint32_t pieces = st.colons + 1;
                for (uint32_t b = pieces; (int32_t)b < R.n_fmt; b++) {
                    uz_vr_put<FILL>(out, limit, o, ':'); uz_vr_put<FILL>(out, limit, o + 1, '.');
                    o += 2;
                }
                int32_t uops = -1, uet = -1;
                if (has_ann) {
                    const int32_t a = uz_vr_find(A, R, st.cell);
                    uint32_t code = 2;
                    if (a >= 0 && uz_vr_cell_gt(T, R, p, code) && (code == 1u || code == 3u)) { uops = A.uops[a]; uet = A.uet[a]; }
                }
                uz_vr_put_int<FILL>(out, limit, o, uops);
                o += 1 + uz_vr_digits(uops);
                uz_vr_put_int<FILL>(out, limit, o, uet);
                o += 1 + uz_vr_digits(uet);
                if (eol && st.cell + 1 != n_samples) hb = true;
            }
            uz_vr_put<FILL>(out, limit, o, eol ? (uint8_t)'\n' : (uint8_t)'\t');
            st.shift = o - (p - R.line_at);
            st.cell++;
            st.colons = 0;
            skip = -1;
            continue;
        }
        if (st.cell >= 0 && ch == ':') {
            st.colons++;
            skip = -1;
        } else if (FILL && in_gt && has_ann) { // a byte of a GT piece: not copied when the piece is rewritten
            if (skip < 0) {
                uint32_t gs, ge;
                uz_vr_gt_piece(T, R, p, gs, ge);
                skip = uz_vr_rewrites(T, A, uz_vr_find(A, R, st.cell), gs, ge) ? 1 : 0;
            }
            if (skip > 0) continue;
        }
        uz_vr_put<FILL>(out, limit, p - R.line_at + st.shift, ch);
    }
}

// 0x80 in every byte of w that equals the byte repeated in `pat` (exact: no carry between bytes)
UZ_VR_HD uint64_t uz_vr_eq_bytes(uint64_t w, uint64_t pat) {
    const uint64_t x = w ^ pat, m = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & m) + m) | x | m);
}
UZ_VR_HD uint32_t uz_vr_mask16(uint64_t lo, uint64_t hi, uint8_t ch) { // bit k: byte k is ch
    const uint64_t pat = 0x0101010101010101ull * ch, g = 0x0102040810204080ull; // (gathers the eight low bits into the top byte)
    const uint32_t a = (uint32_t)(((uz_vr_eq_bytes(lo, pat) >> 7) * g) >> 56), b = (uint32_t)(((uz_vr_eq_bytes(hi, pat) >> 7) * g) >> 56);
    return a | b << 8;
}
UZ_VR_HD void uz_vr_load16(const uint8_t *p, uint64_t &lo, uint64_t &hi) { // p: 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    lo = (uint64_t)v.y << 32 | v.x; hi = (uint64_t)v.w << 32 | v.z;
#else
    memcpy(&lo, p, 8);
    memcpy(&hi, p + 8, 8);
#endif
}
UZ_VR_HD uint32_t uz_vr_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

// ---- the record.  -> its bytes (0: handed back, hb set).  FILL: written to out[0 ...), no store at or beyond `limit` (the sized length).
// T: the chunk's text, 16-byte aligned, with 16 * LANES readable bytes behind the last line end.
template <bool FILL, class W>
UZ_VR_HD uint32_t uz_vcf_row_walk(const W &w, const uint8_t *T, const UzVrRec &R, const UzVrAnn &A, int32_t n_samples, uint8_t *out, uint32_t limit, bool &hb) {
    bool bad = R.hand_back != 0 || R.fmt_end >= R.line_end || R.fmt_end < R.line_at;
    for (uint32_t a = R.ann0 + w.lane(); a < R.ann1; a += W::LANES) {
        if (A.col[a] < 0 || A.col[a] >= n_samples || (a > R.ann0 && A.col[a] <= A.col[a - 1])) bad = true;
        if (A.uops[a] < -1 || A.uops[a] > UZ_VR_UOPS_MAX || A.uet[a] < -1 || A.uet[a] > UZ_VR_UET_MAX || A.gt[a] > 2) bad = true;
    }
    if (w.any(bad)) { hb = true; return 0; }
    const uint32_t l = w.lane();
    uint32_t tabs_seen = 0, colons_seen = 0, shift = 0; // (uniform) tabs in [fmt_end, base), ':' since the last of them, out - in at base
    bool lane_hb = false;
    for (uint64_t base = R.line_at & ~15u; base <= R.line_end; base += 16 * W::LANES) { // (uniform trip count)
        const uint32_t at = (uint32_t)base + l * 16;
        uint64_t lo, hi;
        uz_vr_load16(T + at, lo, hi);
        // the lane's tabs and ':' inside [fmt_end, line_end)
        int64_t b0 = (int64_t)R.fmt_end - (int64_t)at, b1 = (int64_t)R.line_end - (int64_t)at;
        b0 = b0 < 0 ? 0 : (b0 > 16 ? 16 : b0);
        b1 = b1 < 0 ? 0 : (b1 > 16 ? 16 : b1);
        const uint32_t in = ((1u << (uint32_t)b1) - 1u) & ~((1u << (uint32_t)b0) - 1u);
        const uint32_t mt = uz_vr_mask16(lo, hi, '\t') & in, mc = uz_vr_mask16(lo, hi, ':') & in;
        // tabs before the lane
        const uint32_t nt = uz_vr_popc(mt);
        uint32_t it = nt;
        for (uint32_t d = 1; d < W::LANES; d <<= 1) {
            const uint32_t y = w.shfl_up(it, d);
            if (l >= d) it += y;
        }
        // ':' since the last tab before the lane: a scan of (holds a tab, ':' behind its last tab or all its ':')
        uint32_t f = nt ? 1u : 0u, cc = uz_vr_popc(nt ? mc & ~((2u << (31u - (uint32_t)__builtin_clz(mt))) - 1u) : mc);
        for (uint32_t d = 1; d < W::LANES; d <<= 1) {
            const uint32_t yf = w.shfl_up(f, d), yc = w.shfl_up(cc, d);
            if (l >= d) { cc = f ? cc : yc + cc; f |= yf; }
        }
        uint32_t ef = w.shfl_up(f, 1), ec = w.shfl_up(cc, 1);
        if (l == 0) { ef = 0; ec = 0; }
        UzVrState st;
        st.cell = (int32_t)(tabs_seen + it - nt) - 1;
        st.colons = ef ? ec : colons_seen + ec;
        st.shift = 0;
        // the insertions of the lane's own terminators, then their scan: the shift the lane starts with
        UzVrState sized = st;
        uz_vr_lane_walk<false>(T, R, A, n_samples, at, lo, hi, sized, nullptr, 0u, lane_hb);
        uint32_t is = sized.shift;
        for (uint32_t d = 1; d < W::LANES; d <<= 1) {
            const uint32_t y = w.shfl_up(is, d);
            if (l >= d) is += y;
        }
        if (FILL) {
            st.shift = shift + is - sized.shift;
            uz_vr_lane_walk<true>(T, R, A, n_samples, at, lo, hi, st, out, limit, lane_hb);
        }
        tabs_seen += w.bcast(it, W::LANES - 1);
        const uint32_t lf = w.bcast(f, W::LANES - 1), lc = w.bcast(cc, W::LANES - 1);
        colons_seen = lf ? lc : colons_seen + lc;
        shift += w.bcast(is, W::LANES - 1);
    }
    if (w.any(lane_hb)) { hb = true; return 0; }
    return R.line_end - R.line_at + shift + 1u;
}
