// tbx_key.hpp -- one line of tabix-indexed text (an annotated VCF, a BED) turned into its index key (kind, name span, beg, end): the body of
// k_tbx_keys (k_tbx.hip), where the 64 bytes of a step are a wavefront's lanes, of the host code that settles the rows a chunk cannot
// (k_tbx.hip: uz_tbx_settle), and of tests/tbx_key_main.cpp, where they are a plain loop.  tests/tbxmodel.py states the same rules per line in
// Python; unfazed_amd/tabix_index.py (build_host) is the host route's builder over them.
//
// How the body is written.  The only cross-lane step is W::step: the 64 bytes [pos, pos + 64) below `lim`, as four masks (bit b: byte pos + b
// is a tab, a newline, a '\r', a ';').  Everything else is the same scalar walk over those masks in every lane, and single bytes read at
// positions the masks gave (POS's digits, "END=" and its digits): at most some thirty of them a line.
//
// The rules.  p [at] is a line's first byte, at < lim; the line ends at its '\n', or at `lim` when the text ends there (text_end).
//   key columns   VCF: the first eight (CHROM .. INFO); BED: the first three; a line that begins with '#': the first one.  The walk stops
//                 at the tab that ends the last of them, or at the line's end.  NOTHING behind that is read: a line's cost does not depend on
//                 its sample count.
//   cut           the bytes ended (lim, not text_end) before the walk did: kind CUT, nothing else is stated.
//   bad           a '\r' among the bytes walked (WHY_CR), an empty line (WHY_EMPTY), or a position that is not 1 to 10 digits (WHY_POS: VCF's
//                 POS, which is also bad as 0; BED's start, and its end): kind BAD.
//   meta          begins with '#': kind META.
//   name          the first column, whatever the kind (not CUT).
//   VCF           beg = POS - 1; end = beg + max(1, len(REF)) (no REF column: 1).  A line with eight columns has INFO: at INFO's first byte
//                 and directly behind every ';' in it, "END=" followed by 1 to 10 digits and then ';' or INFO's end gives end = max(end, value).
//                 "XEND=" does not match; anything else behind "END=" is ignored.
//   BED           beg = column 2; end = max(column 3, beg + 1).
//   bin           uz_tbx_reg2bin(beg, end): the 14 / 5 scheme of io_index.hpp.
// Sortedness, the 2^29 limit and the order of contigs are table rules (k_tbx.hip, tabix_index.py), not the line's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UZ_TBX_HD __host__ __device__ __forceinline__
#else
#define UZ_TBX_HD inline
#endif

#define UZ_TBX_VCF 0
#define UZ_TBX_BED 1
#define UZ_TBX_META 0u
#define UZ_TBX_DATA 1u
#define UZ_TBX_CUT 2u
#define UZ_TBX_BAD 3u
#define UZ_TBX_WHY_EMPTY 1u
#define UZ_TBX_WHY_CR 2u
#define UZ_TBX_WHY_POS 3u
#define UZ_TBX_MAX_END ((int64_t)1 << 29) /* the 14 / 5 scheme's reach: end <= 2^29 */
#define UZ_TBX_PSEUDO_BIN 37450u

struct UzTbxKey {
    uint32_t kind, why; // UZ_TBX_META .. BAD; why a BAD line is bad
    uint32_t name_len;
    int64_t beg, end;
};

struct UzTbxHostWave { // the 64 bytes of a step as a plain loop
    void step(const uint8_t *p, uint64_t pos, uint64_t lim, uint64_t &tabs, uint64_t &nls, uint64_t &crs, uint64_t &semis) const {
        tabs = nls = crs = semis = 0;
        for (uint32_t b = 0; b < 64 && pos + b < lim; b++) {
            const uint8_t ch = p[pos + b];
            tabs |= (uint64_t)(ch == '\t') << b;
            nls |= (uint64_t)(ch == '\n') << b;
            crs |= (uint64_t)(ch == '\r') << b;
            semis |= (uint64_t)(ch == ';') << b;
        }
    }
};

UZ_TBX_HD uint32_t uz_tbx_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}

// the 1 to 10 digits that fill [a, b) -> their value, or -1
UZ_TBX_HD int64_t uz_tbx_digits(const uint8_t *p, uint64_t a, uint64_t b) {
    if (b <= a || b - a > 10) return -1;
    int64_t v = 0;
    for (uint64_t i = a; i < b; i++) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9) return -1;
        v = v * 10 + d;
    }
    return v;
}

UZ_TBX_HD uint32_t uz_tbx_ctz64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)v) - 1u;
#else
    return (uint32_t)__builtin_ctzll(v);
#endif
}

template <typename W>
UZ_TBX_HD void uz_tbx_key(const W &w, const uint8_t *p, uint64_t at, uint64_t lim, bool text_end, int preset, UzTbxKey &k) {
    k.kind = UZ_TBX_BAD; k.why = 0; k.name_len = 0; k.beg = k.end = 0;
    const bool meta = p[at] == '#';
    const uint32_t want = meta ? 1u : preset == UZ_TBX_VCF ? 8u : 3u;
    uint64_t col_end[8]; // where column i ends: its tab, the line's '\n', or lim
    uint32_t cols = 0;
    bool done = false, cr = false;
    for (uint64_t pos = at; pos < lim && !done; pos += 64) {
        uint64_t tabs, nls, crs, semis;
        w.step(p, pos, lim, tabs, nls, crs, semis);
        uint64_t ends = tabs | nls;
        uint32_t stop = 64; // the step's bytes below it were walked
        while (ends) {
            const uint32_t b = uz_tbx_ctz64(ends);
            ends &= ends - 1;
            col_end[cols++] = pos + b;
            if ((nls >> b & 1u) || cols == want) { done = true; stop = b; break; }
        }
        if (crs & (stop == 64 ? ~(uint64_t)0 : (((uint64_t)1 << stop) - 1))) cr = true;
    }
    if (!done) {
        if (!text_end) { k.kind = UZ_TBX_CUT; return; }
        col_end[cols++] = lim; // the text's end ends the line
    }
    k.name_len = (uint32_t)(col_end[0] - at);
    if (cr) { k.why = UZ_TBX_WHY_CR; return; }
    if (meta) { k.kind = UZ_TBX_META; return; }
    if (p[at] == '\n') { k.why = UZ_TBX_WHY_EMPTY; return; }
    k.why = UZ_TBX_WHY_POS;
    if (cols < 2) return;
    const int64_t first = uz_tbx_digits(p, col_end[0] + 1, col_end[1]);
    if (first < 0) return;
    if (preset == UZ_TBX_BED) {
        if (cols < 3) return;
        const int64_t last = uz_tbx_digits(p, col_end[1] + 1, col_end[2]);
        if (last < 0) return;
        k.beg = first;
        k.end = last > first + 1 ? last : first + 1;
    } else {
        if (first == 0) return;
        k.beg = first - 1;
        const int64_t ref = cols >= 4 ? (int64_t)(col_end[3] - col_end[2] - 1) : 0;
        k.end = k.beg + (ref > 1 ? ref : 1);
        if (cols == 8) { // INFO: [a, b)
            const uint64_t a = col_end[6] + 1, b = col_end[7];
            for (uint64_t pos = a; pos < b; pos += 64) {
                uint64_t tabs, nls, crs, semis;
                w.step(p, pos, b, tabs, nls, crs, semis);
                for (bool head = pos == a; head || semis; head = false) {
                    uint64_t c = a; // a candidate: INFO's first byte, then the byte behind each ';'
                    if (!head) {
                        c = pos + uz_tbx_ctz64(semis) + 1;
                        semis &= semis - 1;
                    }
                    if (c + 4 > b || p[c] != 'E' || p[c + 1] != 'N' || p[c + 2] != 'D' || p[c + 3] != '=') continue;
                    uint64_t e = c + 4;
                    while (e < b && e - (c + 4) <= 10 && (uint32_t)p[e] - '0' <= 9) e++;
                    if (e < b && p[e] != ';') continue;
                    const int64_t v = uz_tbx_digits(p, c + 4, e);
                    if (v > k.end) k.end = v;
                }
            }
        }
    }
    k.kind = UZ_TBX_DATA;
    k.why = 0;
}
