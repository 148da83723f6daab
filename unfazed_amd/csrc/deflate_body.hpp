// deflate_body.hpp -- one slice of at most 65 280 bytes (htslib's 0xff00) turned into one raw DEFLATE stream: the body of k_bgzf_deflate
// (k_deflate.hip), where its 64 lanes are a wavefront, and of tests/bgzf_body_main.cpp, where they are a plain loop.  Both builds emit THE SAME
// BYTES: every step below is either lane-private, or a cross-lane step whose result does not depend on the order the lanes run in.
// deflate_dyn.hpp is a second coder over the same parse (uz_df_group, the one statement of the group step) which may choose dynamic Huffman.
//
// How the body is written.  A value a lane keeps from step to step is a W::V<T> (the device: a register; the host: an array of 64); a step is
// a loop UZ_DF_EACH(w, l) over the lanes the caller runs (the device: its own; the host: all 64, ascending) that touches only v[l]; between
// steps stand the cross-lane calls of W (ballot, excl_scan, get, insert_max, or_word, sync).
//
// The parse rule.  The slice is walked in GROUPS of 64 consecutive positions, group k = positions [64 k, 64 k + 64).
//   hash     position p with p + 4 <= n hashes its next FOUR bytes: (little-endian word * 2654435761) >> 19, 13 bits.  The table holds 8192
//            16-bit entries in LDS (16 KiB): position + 1 of the LAST position seen with that hash, 0 for none.
//   state    every position of a group probes the table as it stands after ALL positions of the groups before it were inserted and NONE of
//            its own: the 64 probes come first, then the 64 inserts.  (So a candidate lies in an earlier group: distance >= lane + 1.)
//   insert   every position of the group with p + 4 <= n, whether a match covers it or not, ascending: where several positions of a group
//            share a hash the highest stays.  The device reaches the same state by raising an entry until no lane holds a higher position
//            (W::insert_max): the result is a maximum, which no order of the lanes changes.
//   probe    one candidate per position, verified byte for byte from its first byte (equal hashes are not equal strings): the match is the
//            common prefix of candidate and position, capped at 258 and at the slice's end; it is kept when its length is >= 4 and its
//            distance <= 32 768.  (DEFLATE's minimum of 3 is never undercut; a 3-byte match cannot be found through a 4-byte hash but by
//            a collision, and costs as much as three literals.)  Nothing is read before the slice's first byte or past its last.
//   greedy   left to right: `next` is the first position no token covers yet.  In a group, the first lane at or past `next` that kept a
//            match takes it, the positions between are literals, `next` moves behind the match, and so on (a ballot of the kept matches,
//            then a uniform walk over its set bits; a taken match's length is fetched from its lane).  A group that lies wholly inside a
//            match (next >= its end) probes nothing and only inserts.
// The coder: one block, BFINAL = 1, BTYPE = 01 (fixed Huffman).  A lane's token is at most 31 bits (length code 8 + extra 5 + distance
// code 5 + extra 13), Huffman codes bit-reversed so that they leave most-significant bit first, extra bits as they are; length 258 is symbol
// 285.  An exclusive scan of the bit lengths places every token; each lane ORs its token into a window of 96 words in LDS (OR commutes), and
// whenever 64 whole words stand in the window they leave as one coalesced store.  End of block (seven zero bits), zero padding to the byte.
// Stored fallback: before a group's tokens are placed the coder holds the stream's size with them, the end-of-block code and the padding
// against 5 + n; the moment it would pass, the coder stops and the slice is written as one stored block (BTYPE = 00, 5 + n bytes).  So a stream
// is never longer than 5 + n <= 65 285 bytes, and 65 285 + 26 bytes of BGZF framing fit a BGZF block.  Every store is also held against
// `cap`, the slot's size, by itself.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define UZ_DF_HD __host__ __device__ __forceinline__
#else
#define UZ_DF_HD inline
#endif

#define UZ_DF_SLICE 65280u    /* bytes of input per BGZF block */
#define UZ_DF_SLOT 65536u     /* bytes of a stream's scratch slot: >= 5 + UZ_DF_SLICE, rounded to whole words */
#define UZ_DF_HASH_BITS 13
#define UZ_DF_TABLE (1u << UZ_DF_HASH_BITS)
#define UZ_DF_WINDOW 96u      /* words of the staging window: 63 whole words waiting + a group's 598 bits + the word they start in */
#define UZ_DF_MIN_MATCH 4u
#define UZ_DF_MAX_MATCH 258u
#define UZ_DF_MAX_DIST 32768u
#define UZ_BGZF_HEAD 18u      /* bytes of a BGZF block before its stream, and ... */
#define UZ_BGZF_TAIL 8u       /* ... behind it: CRC-32, ISIZE */

#define UZ_DF_EACH(w, l) for (uint32_t l = (w).lane0(), l##_end = (w).lane1(); l < l##_end; l++)

UZ_DF_HD uint32_t uz_df_load32(const uint8_t *p) { // (little-endian, any alignment)
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
UZ_DF_HD uint32_t uz_df_hash(uint32_t word) { return (word * 2654435761u) >> (32 - UZ_DF_HASH_BITS); }
UZ_DF_HD uint32_t uz_df_rev(uint32_t v, uint32_t nbits) { // the low nbits of v, reversed
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - nbits);
}
UZ_DF_HD uint32_t uz_df_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } // v > 0
UZ_DF_HD uint64_t uz_df_below(uint32_t b) { return b >= 64 ? ~0ull : (1ull << b) - 1; } // the lanes under b

// the fixed code of a literal / length symbol, as the bits the stream takes (first bit lowest)
UZ_DF_HD uint32_t uz_df_litlen(uint32_t sym, uint32_t &nbits) {
    if (sym < 144) { nbits = 8; return uz_df_rev(0x30u + sym, 8); }
    if (sym < 256) { nbits = 9; return uz_df_rev(0x190u + (sym - 144), 9); }
    if (sym < 280) { nbits = 7; return uz_df_rev(sym - 256, 7); }
    nbits = 8;
    return uz_df_rev(0xC0u + (sym - 280), 8);
}
// a match length as its symbol, the count of its extra bits and their value; length 258 is symbol 285
UZ_DF_HD void uz_df_len_sym(uint32_t len, uint32_t &sym, uint32_t &le, uint32_t &lx) {
    const uint32_t l = len - 3;
    le = 0; lx = 0;
    if (len == UZ_DF_MAX_MATCH) sym = 285;
    else if (l < 8) sym = 257 + l;
    else { le = uz_df_log2(l) - 2; sym = 261 + 4 * le + ((l >> le) & 3u); lx = l & ((1u << le) - 1); }
}
// a distance likewise
UZ_DF_HD void uz_df_dist_sym(uint32_t dist, uint32_t &dsym, uint32_t &de, uint32_t &dx) {
    const uint32_t d = dist - 1;
    de = 0; dx = 0;
    if (d < 4) dsym = d;
    else { const uint32_t nb = uz_df_log2(d); de = nb - 1; dsym = 2 * nb + ((d >> de) & 1u); dx = d & ((1u << de) - 1); }
}
// a match as its token: length symbol, its extra bits, distance symbol, its extra bits
UZ_DF_HD uint32_t uz_df_match_token(uint32_t len, uint32_t dist, uint32_t &nbits) {
    uint32_t sym, le, lx, dsym, de, dx;
    uz_df_len_sym(len, sym, le, lx);
    uint32_t n = 0;
    uint32_t tok = uz_df_litlen(sym, n);
    tok |= lx << n; n += le;
    uz_df_dist_sym(dist, dsym, de, dx);
    tok |= uz_df_rev(dsym, 5) << n; n += 5;
    tok |= dx << n; n += de;
    nbits = n;
    return tok;
}

// the host program's wave: every lane in turn
struct UzDfHostWave {
    template <typename T>
    struct V {
        T x[64];
        T &operator[](uint32_t l) { return x[l]; }
        const T &operator[](uint32_t l) const { return x[l]; }
    };
    uint32_t lane0() const { return 0; }
    uint32_t lane1() const { return 64; }
    void sync() const {}
    void drain() const {}
    uint64_t ballot(const V<uint32_t> &p) const {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64; l++) m |= (uint64_t)(p[l] != 0) << l;
        return m;
    }
    void excl_scan(const V<uint32_t> &v, V<uint32_t> &out, uint32_t &total) const {
        uint32_t s = 0;
        for (uint32_t l = 0; l < 64; l++) { out[l] = s; s += v[l]; }
        total = s;
    }
    uint32_t get(const V<uint32_t> &v, uint32_t src) const { return v[src]; }
    void insert_max(uint16_t *tab, const V<uint32_t> &h, const V<uint32_t> &val, const V<uint32_t> &ok) const {
        for (uint32_t l = 0; l < 64; l++)
            if (ok[l]) tab[h[l]] = (uint16_t)val[l]; // ascending: the highest stays
    }
    void or_word(uint32_t *w, uint32_t v) const { *w |= v; }
    void add_word(uint32_t *w, uint32_t v) const { *w += v; } // (deflate_dyn.hpp: the histograms)
};

struct UzDfLds { // a wave's LDS
    uint16_t tab[UZ_DF_TABLE];
    uint32_t win[UZ_DF_WINDOW];
};

// the whole words of the window that lie under `upto` words leave for the slot; a store that would pass `cap` is not made
template <typename W>
UZ_DF_HD void uz_df_store_words(W &w, const uint32_t *win, uint32_t wbase, uint32_t count, uint8_t *out, uint32_t cap) {
    for (uint32_t k0 = 0; k0 < count; k0 += 64) {
        UZ_DF_EACH(w, l) {
            const uint32_t k = k0 + l;
            if (k < count && ((size_t)wbase + k) * 4 + 4 <= cap) reinterpret_cast<uint32_t *>(out)[wbase + k] = win[k];
        }
    }
}

// One group of the parse rule (the head of this file): the 64 positions from g probe, then insert; the greedy walk takes its matches.
// -> false: the whole group lies inside a match (inserted only, nothing to emit).  Otherwise mlen / mdist hold every lane's kept match,
// `taken` the lanes whose match the walk took, `covered` the lanes a token of an earlier lane covers, and `next` has moved.
template <typename W>
UZ_DF_HD bool uz_df_group(W &w, uint16_t *tab, const uint8_t *in, uint32_t n, uint32_t g, uint32_t &next, typename W::template V<uint32_t> &mlen,
                          typename W::template V<uint32_t> &mdist, uint64_t &taken, uint64_t &covered) {
    typedef typename W::template V<uint32_t> Lane;
    const uint32_t cnt = n - g < 64 ? n - g : 64;
    const bool inside = next >= g + cnt; // the whole group lies inside a match
    Lane h, val, can, has;
    UZ_DF_EACH(w, l) {
        const uint32_t p = g + l;
        can[l] = p + 4 <= n ? 1u : 0u;
        h[l] = can[l] ? uz_df_hash(uz_df_load32(in + p)) : 0u;
        val[l] = p + 1;
        mlen[l] = 0; mdist[l] = 0; has[l] = 0;
        if (can[l] && !inside) {
            const uint32_t c1 = tab[h[l]];
            if (c1) {
                const uint32_t c = c1 - 1, dist = p - c; // c < g <= p
                const uint32_t cap_len = n - p < UZ_DF_MAX_MATCH ? n - p : UZ_DF_MAX_MATCH;
                uint32_t m = 0;
                if (dist <= UZ_DF_MAX_DIST) {
                    while (m + 4 <= cap_len && uz_df_load32(in + c + m) == uz_df_load32(in + p + m)) m += 4;
                    while (m < cap_len && in[c + m] == in[p + m]) m++;
                }
                if (m >= UZ_DF_MIN_MATCH) { mlen[l] = m; mdist[l] = dist; has[l] = 1; }
            }
        }
    }
    w.sync(); // every probe before the first insert
    w.insert_max(tab, h, val, can);
    if (inside) return false;
    // greedy, left to right
    const uint64_t kept = w.ballot(has);
    uint32_t cur = next > g ? next - g : 0;
    covered = uz_df_below(cur);
    taken = 0;
    while (cur < cnt) {
        const uint64_t m = kept & ~uz_df_below(cur);
        if (!m) break;
        const uint32_t j = (uint32_t)__builtin_ctzll(m);
        const uint32_t len = w.get(mlen, j);
        taken |= 1ull << j;
        covered |= uz_df_below(j + len) & ~uz_df_below(j + 1);
        cur = j + len;
        next = g + cur;
    }
    if (next < g + cnt) next = g + cnt;
    return true;
}

// the slice as one stored block (BTYPE = 00): 5 + n bytes
template <typename W>
UZ_DF_HD uint32_t uz_df_store_raw(W &w, const uint8_t *in, uint32_t n, uint8_t *out) {
    w.drain(); // (the words that left before must not land on top of the stored bytes)
    w.sync();
    UZ_DF_EACH(w, l) {
        if (l == 0) {
            out[0] = 1; // BFINAL = 1, BTYPE = 00
            out[1] = (uint8_t)(n & 0xFF); out[2] = (uint8_t)(n >> 8);
            out[3] = (uint8_t)(~n & 0xFF); out[4] = (uint8_t)((~n >> 8) & 0xFF);
        }
        for (uint32_t i = l; i < n; i += 64) out[5 + i] = in[i];
    }
    return 5 + n;
}

// in [n] (0 < n <= UZ_DF_SLICE) -> out (a slot of cap >= 5 + n bytes, 4-byte aligned) -> the stream's bytes.  *stored: the fallback was taken.
template <typename W>
UZ_DF_HD uint32_t uz_deflate_slice(W &w, UzDfLds &S, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, bool &stored) {
    typedef typename W::template V<uint32_t> Lane;
    const uint32_t limit = 5 + n; // what the stored form takes
    stored = false;
    if (cap < limit || n == 0 || n > UZ_DF_SLICE) { stored = true; return 0; } // (no caller does this: nothing is written)
    for (uint32_t k0 = 0; k0 < UZ_DF_TABLE; k0 += 64) {
        UZ_DF_EACH(w, l) S.tab[k0 + l] = 0;
    }
    for (uint32_t k0 = 0; k0 < UZ_DF_WINDOW; k0 += 64) {
        UZ_DF_EACH(w, l) if (k0 + l < UZ_DF_WINDOW) S.win[k0 + l] = k0 + l == 0 ? 3u : 0u; // BFINAL = 1, BTYPE = 01
    }
    w.sync();
    uint32_t bitpos = 3, wbase = 0 /* the stream's word that window[0] is */, next = 0;
    bool give_up = false;
    for (uint32_t g = 0; g < n; g += 64) {
        const uint32_t cnt = n - g < 64 ? n - g : 64;
        Lane mlen, mdist;
        uint64_t taken = 0, covered = 0;
        if (!uz_df_group(w, S.tab, in, n, g, next, mlen, mdist, taken, covered)) continue;
        // tokens, their bit lengths, their places
        Lane tok, nb, at;
        UZ_DF_EACH(w, l) {
            uint32_t t = 0, b = 0;
            if ((taken >> l) & 1) t = uz_df_match_token(mlen[l], mdist[l], b);
            else if (l < cnt && !((covered >> l) & 1)) t = uz_df_litlen(in[g + l], b);
            tok[l] = t; nb[l] = b;
        }
        uint32_t total = 0;
        w.excl_scan(nb, at, total);
        if (((bitpos + total + 7 + 7) >> 3) > limit) { give_up = true; break; } // with the end-of-block code and the padding: past the stored form
        UZ_DF_EACH(w, l) {
            if (nb[l]) {
                const uint32_t o = bitpos + at[l], k = (o >> 5) - wbase, sh = o & 31u;
                w.or_word(&S.win[k], tok[l] << sh);
                if (sh && (tok[l] >> (32 - sh))) w.or_word(&S.win[k + 1], tok[l] >> (32 - sh));
            }
        }
        bitpos += total;
        w.sync();
        if ((bitpos >> 5) - wbase >= 64) { // 64 whole words leave; what stands behind them moves to the window's head
            uz_df_store_words(w, S.win, wbase, 64, out, cap);
            Lane keep;
            UZ_DF_EACH(w, l) keep[l] = l < UZ_DF_WINDOW - 64 ? S.win[64 + l] : 0u;
            w.sync();
            UZ_DF_EACH(w, l) {
                S.win[l] = keep[l];
                if (l < UZ_DF_WINDOW - 64) S.win[64 + l] = 0;
            }
            wbase += 64;
            w.sync();
        }
    }
    if (give_up) { // one stored block
        stored = true;
        return uz_df_store_raw(w, in, n, out);
    }
    bitpos += 7; // end of block: seven zero bits, which the window holds already
    const uint32_t words = ((bitpos + 31) >> 5) - wbase;
    uz_df_store_words(w, S.win, wbase, words, out, cap);
    return (bitpos + 7) >> 3;
}
