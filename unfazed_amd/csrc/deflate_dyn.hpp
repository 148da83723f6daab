// deflate_dyn.hpp -- the second coder over deflate_body.hpp's parse: one slice turned into one raw DEFLATE stream whose block is the shortest of
// dynamic Huffman (BTYPE = 10), fixed Huffman (01) and stored (00).  The body of k_bgzf_deflate_dyn (k_deflate.hip) and of
// tests/bgzf_dyn_main.cpp; the discipline is deflate_body.hpp's: one statement of every rule, lane-private steps and order-free cross-lane
// steps, so that the wavefront and the host loop emit THE SAME BYTES.
//
// Pass 1: the parse.  uz_df_group, the fixed coder's group step, over the WHOLE slice: there is no give-up in the middle.  The lanes that emit a
//   token write it into the slice's token buffer in HBM, compacted by their rank among the group's emitters (a ballot and a count of the bits
//   below the lane): one 32-bit word per token, a literal's byte, or bit 31 + (length - 3) << 16 + (distance - 1).  At most one token per input
//   byte: 65 280 words, 255 KiB a slice.  Every token adds its literal / length symbol, and a match its distance symbol, into the histograms
//   (LDS atomic adds on the device, plain adds on the host: addition commutes); end-of-block counts once.
// The codes: uz_dy_build gives a count vector its code lengths under a limit -- the used symbols ranked by (count, symbol), which is order-free
//   by construction; the lengths of a minimum-redundancy code over the sorted counts (Moffat and Katajainen's in-place pass: Huffman's cost);
//   lengths above the limit folded into it and the counts per length rebalanced until Kraft's sum is exactly 1 (the repair miniz and zlib use:
//   it moves nothing when the code fits); the lengths handed out most frequent first, canonical codes in symbol order.  The sort is every
//   lane's, the rest is lane 0's, a few thousand steps on LDS.  A symbol that does not occur gets length 0; one used symbol gets one bit.
//   Literal / length code and distance code at limit 15.  The distance code always holds two symbols, as zlib's does: with none used, symbols 0
//   and 1; with one, it and symbol 0 (symbol 1 beside symbol 0); they cost a header entry and no bit of the body.  The lengths of both codes,
//   HLIT + HDIST of them with no trailing zero (HLIT >= 257, HDIST >= 1), are run-length coded as one sequence, runs crossing the seam: a
//   length, then 16 for 3..6 repeats; 17 for 3..10 zeros, 18 for 11..138.  Their code (19 symbols, limit 7) is sent in the 16, 17, 18, 0, 8, 7,
//   ... order, HCLEN trimmed of trailing zeros, at least 4.
// The choice, from the histograms alone: the dynamic block's bits (3 + 14 + 3 HCLEN + the coded lengths + sum of count * (length + extra bits)),
//   the fixed block's bits with the fixed lengths, the stored form's 5 + n bytes.  In whole bytes: dynamic only when strictly shorter than
//   fixed; stored when the shorter of the two is past 5 + n (the fixed coder's rule: where it gives up, the fixed form is past 5 + n).  So a
//   slice's stream here is never longer than the fixed coder's, and a slice that comes out fixed comes out as uz_deflate_slice's bytes.
// Pass 2: the tokens are read back 64 at a time and coded from tables in LDS (code << 5 | length, the code bit-reversed); the hash table is
//   dead by then and the tables and the window lie over it.  A token is at most 48 bits (15 + 5 + 15 + 13): a lane ORs it into up to three
//   words of the window.  The window: at most 63 whole words wait, a group adds at most 64 * 48 bits = 96 words, and one more word holds
//   the bit they start in: 160.  Whenever 64 whole words stand in it they leave as one coalesced store.  The header goes through the same step:
//   lane 0 the 17 bits of BFINAL, BTYPE, HLIT, HDIST, HCLEN and lanes 1 .. HCLEN three bits each, then the coded lengths 64 at a time.
#pragma once
#include "deflate_body.hpp"

#define UZ_DY_WINDOW 160u /* words of the staging window: 63 whole words waiting + a group's 64 * 48 bits + the word they start in */
#define UZ_DY_LL 286u     /* literal / length symbols */
#define UZ_DY_D 30u       /* distance symbols */
#define UZ_DY_CL 19u      /* symbols of the code the lengths are sent in */
#define UZ_DY_HIST_D 288u /* the distance counters' place in the histogram */
#define UZ_DY_TOKENS UZ_DF_SLICE /* words of a slice's token buffer */
#define UZ_DY_STORED 0
#define UZ_DY_FIXED 1
#define UZ_DY_DYNAMIC 2

struct UzDyBuild { // uz_dy_build's workspace
    uint32_t key[288]; // the used symbols' counts ascending, then the tree's parents, then the depths
    uint16_t sym[288]; // ... and their symbols
    uint32_t num[16], nxt[16]; // codes per length, the next code of a length
};
struct UzDyCodes { // what stands between the passes, and pass 2's window
    uint32_t win[UZ_DY_WINDOW];
    uint32_t ll_code[288], d_code[32], cl_code[32]; // code (as the bits the stream takes) << 5 | length
    uint8_t ll_len[288], d_len[32], cl_len[32];
    uint8_t lens[320];     // the HLIT + HDIST lengths as sent
    uint16_t cl_list[320]; // their run-length form: symbol | extra value << 8
    uint32_t cl_hist[32], n_cl;
    UzDyBuild B;
};
struct UzDyLds { // a wave's LDS
    union {
        uint16_t tab[UZ_DF_TABLE]; // pass 1
        UzDyCodes c;               // behind it
    } u;
    uint32_t hist[320]; // [0, 286) literal / length, [288, 318) distance
};

UZ_DF_HD uint32_t uz_dy_ll_extra(uint32_t s) { return s >= 265 && s < 285 ? (s - 261) >> 2 : 0; } // extra bits of a literal / length symbol
UZ_DF_HD uint32_t uz_dy_d_extra(uint32_t d) { return d >= 4 ? (d >> 1) - 1 : 0; }
UZ_DF_HD uint32_t uz_dy_cl_extra(uint32_t s) { return s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u; }
UZ_DF_HD uint32_t uz_dy_cl_order(uint32_t k) { // the k-th symbol of the 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 order
    if (k < 3) return 16 + k;
    if (k == 3) return 0;
    return (k & 1) ? 8 - ((k - 3) >> 1) : 8 + ((k - 4) >> 1);
}

// cnt [n] (n <= 288, their sum under 2^32) -> len [n]: code lengths of at most `limit` (<= 15) bits, Huffman's cost where Huffman's code fits
// the limit; code [n]: canonical code, bit-reversed, << 5 | length.  Every lane of the wave calls it.
template <typename W>
UZ_DF_HD void uz_dy_build(W &w, UzDyBuild &B, const uint32_t *cnt, uint32_t n, uint32_t limit, uint8_t *len, uint32_t *code) {
    typedef typename W::template V<uint32_t> Lane;
    uint32_t m = 0; // the used symbols
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        Lane used;
        UZ_DF_EACH(w, l) {
            const uint32_t s = k0 + l;
            used[l] = 0;
            if (s < n) {
                const uint32_t c = cnt[s];
                if (c) { // its place among the used symbols by (count, symbol): no two share one
                    uint32_t r = 0;
                    for (uint32_t t = 0; t < n; t++) {
                        const uint32_t ct = cnt[t];
                        r += (ct && (ct < c || (ct == c && t < s))) ? 1u : 0u;
                    }
                    B.key[r] = c;
                    B.sym[r] = (uint16_t)s;
                    used[l] = 1;
                }
                len[s] = 0;
                code[s] = 0;
            }
        }
        m += (uint32_t)__builtin_popcountll(w.ballot(used));
    }
    w.sync();
    UZ_DF_EACH(w, l) {
        if (l != 0 || m == 0) continue;
        if (m == 1) {
            B.key[0] = 1;
        } else {
            // minimum redundancy in place: key[0, m) ascending counts -> internal nodes' weights and parents -> the leaves' depths
            B.key[0] += B.key[1];
            uint32_t root = 0, leaf = 2;
            for (uint32_t next = 1; next + 1 < m; next++) {
                if (leaf >= m || B.key[root] < B.key[leaf]) { B.key[next] = B.key[root]; B.key[root++] = next; }
                else B.key[next] = B.key[leaf++];
                if (leaf >= m || (root < next && B.key[root] < B.key[leaf])) { B.key[next] += B.key[root]; B.key[root++] = next; }
                else B.key[next] += B.key[leaf++];
            }
            B.key[m - 2] = 0;
            for (uint32_t next = m - 2; next-- > 0;) B.key[next] = B.key[B.key[next]] + 1;
            int32_t avail = 1, inner = 0, r = (int32_t)m - 2, next = (int32_t)m - 1;
            for (uint32_t depth = 0; avail > 0; depth++) {
                while (r >= 0 && B.key[r] == depth) { inner++; r--; }
                while (avail > inner) { B.key[next--] = depth; avail--; }
                avail = 2 * inner;
                inner = 0;
            }
        }
        // codes per length, the lengths above the limit folded into it; then Kraft's sum brought down to 1
        for (uint32_t i = 0; i < 16; i++) B.num[i] = 0;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t d = B.key[i];
            B.num[d > limit ? limit : d]++;
        }
        uint32_t total = 0;
        for (uint32_t i = 1; i <= limit; i++) total += B.num[i] << (limit - i);
        while (m > 1 && total > (1u << limit)) {
            B.num[limit]--;
            for (uint32_t i = limit - 1; i > 0; i--)
                if (B.num[i]) { B.num[i]--; B.num[i + 1] += 2; break; }
            total--;
        }
        // the most frequent symbol the shortest code
        uint32_t j = m;
        for (uint32_t i = 1; i <= limit; i++)
            for (uint32_t k = B.num[i]; k > 0; k--) len[B.sym[--j]] = (uint8_t)i;
        // canonical codes, in symbol order within a length
        uint32_t c = 0;
        B.nxt[0] = 0;
        for (uint32_t i = 1; i <= limit; i++) { c = (c + B.num[i - 1]) << 1; B.nxt[i] = c; }
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t ln = len[s];
            if (ln) code[s] = (uz_df_rev(B.nxt[ln]++, ln) << 5) | ln;
        }
    }
    w.sync();
}

// 64 lanes' bits (nb <= 48 each, 0: none) behind the stream's bitpos, in lane order; whole words leave 64 at a time
template <typename W>
UZ_DF_HD void uz_dy_put(W &w, uint32_t *win, const typename W::template V<uint64_t> &bits, const typename W::template V<uint32_t> &nb, uint32_t &bitpos,
                        uint32_t &wbase, uint8_t *out, uint32_t cap) {
    typedef typename W::template V<uint32_t> Lane;
    Lane at;
    uint32_t total = 0;
    w.excl_scan(nb, at, total);
    UZ_DF_EACH(w, l) {
        if (nb[l]) {
            const uint32_t o = bitpos + at[l], k = (o >> 5) - wbase, sh = o & 31u;
            const uint64_t lo = bits[l] << sh;
            const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = sh ? (uint32_t)(bits[l] >> (64 - sh)) : 0u;
            if (w0 && k < UZ_DY_WINDOW) w.or_word(&win[k], w0);
            if (w1 && k + 1 < UZ_DY_WINDOW) w.or_word(&win[k + 1], w1);
            if (w2 && k + 2 < UZ_DY_WINDOW) w.or_word(&win[k + 2], w2);
        }
    }
    bitpos += total;
    w.sync();
    while ((bitpos >> 5) - wbase >= 64) { // 64 whole words leave; what stands behind them moves to the window's head
        uz_df_store_words(w, win, wbase, 64, out, cap);
        Lane k0, k1;
        UZ_DF_EACH(w, l) {
            k0[l] = win[64 + l];
            k1[l] = 128 + l < UZ_DY_WINDOW ? win[128 + l] : 0u;
        }
        w.sync();
        UZ_DF_EACH(w, l) {
            win[l] = k0[l];
            win[64 + l] = k1[l];
            if (128 + l < UZ_DY_WINDOW) win[128 + l] = 0;
        }
        wbase += 64;
        w.sync();
    }
}

// in [n] (0 < n <= UZ_DF_SLICE) -> out (a slot of cap >= 5 + n bytes, 4-byte aligned) -> the stream's bytes; tok: the slice's token buffer
// (tok_cap >= n words); *kind: UZ_DY_STORED / UZ_DY_FIXED / UZ_DY_DYNAMIC
template <typename W>
UZ_DF_HD uint32_t uz_deflate_slice_dyn(W &w, UzDyLds &S, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *tok, uint32_t tok_cap,
                                       uint32_t &kind) {
    typedef typename W::template V<uint32_t> Lane;
    typedef typename W::template V<uint64_t> Lane64;
    const uint32_t limit = 5 + n; // what the stored form takes
    kind = UZ_DY_STORED;
    if (cap < limit || n == 0 || n > UZ_DF_SLICE || tok_cap < n) return 0; // (no caller does this: nothing is written)
    UzDyCodes &C = S.u.c;
    uint32_t *const hist_d = S.hist + UZ_DY_HIST_D;
    for (uint32_t k0 = 0; k0 < UZ_DF_TABLE; k0 += 64) {
        UZ_DF_EACH(w, l) S.u.tab[k0 + l] = 0;
    }
    for (uint32_t k0 = 0; k0 < 320; k0 += 64) {
        UZ_DF_EACH(w, l) S.hist[k0 + l] = k0 + l == 256 ? 1u : 0u; // end of block, once
    }
    w.sync();
    // pass 1
    uint32_t next = 0, n_tok = 0;
    for (uint32_t g = 0; g < n; g += 64) {
        const uint32_t cnt = n - g < 64 ? n - g : 64;
        Lane mlen, mdist;
        uint64_t taken = 0, covered = 0;
        if (!uz_df_group(w, S.u.tab, in, n, g, next, mlen, mdist, taken, covered)) continue;
        const uint64_t emits = taken | (~covered & uz_df_below(cnt));
        UZ_DF_EACH(w, l) {
            if ((emits >> l) & 1) {
                const uint32_t at = n_tok + (uint32_t)__builtin_popcountll(emits & uz_df_below(l));
                uint32_t t;
                if ((taken >> l) & 1) {
                    uint32_t sym, le, lx, dsym, de, dx;
                    uz_df_len_sym(mlen[l], sym, le, lx);
                    uz_df_dist_sym(mdist[l], dsym, de, dx);
                    w.add_word(&S.hist[sym], 1);
                    w.add_word(&hist_d[dsym], 1);
                    t = 0x80000000u | ((mlen[l] - 3) << 16) | (mdist[l] - 1);
                } else {
                    t = in[g + l];
                    w.add_word(&S.hist[t], 1);
                }
                if (at < tok_cap) tok[at] = t;
            }
        }
        n_tok += (uint32_t)__builtin_popcountll(emits);
    }
    w.drain(); // the tokens have landed; the table is dead
    w.sync();
    // the distance code holds two symbols
    Lane p;
    UZ_DF_EACH(w, l) p[l] = l < UZ_DY_D && hist_d[l] ? 1u : 0u;
    const uint64_t d_used = w.ballot(p);
    uint64_t forced = 0;
    if (d_used == 0) forced = 3;
    else if ((d_used & (d_used - 1)) == 0) forced = (d_used & 1) ? 2 : 1;
    UZ_DF_EACH(w, l) if ((forced >> l) & 1) hist_d[l] = 1;
    for (uint32_t k0 = 0; k0 < UZ_DY_WINDOW; k0 += 64) {
        UZ_DF_EACH(w, l) if (k0 + l < UZ_DY_WINDOW) C.win[k0 + l] = 0;
    }
    UZ_DF_EACH(w, l) if (l < 32) C.cl_hist[l] = 0;
    w.sync();
    uz_dy_build(w, C.B, S.hist, UZ_DY_LL, 15, C.ll_len, C.ll_code);
    uz_dy_build(w, C.B, hist_d, UZ_DY_D, 15, C.d_len, C.d_code);
    UZ_DF_EACH(w, l) if ((forced >> l) & 1) hist_d[l] = 0;
    // HLIT, HDIST; the lengths as one sequence
    uint32_t hlit = 257, hdist = 1;
    for (uint32_t k0 = 256; k0 < UZ_DY_LL; k0 += 64) {
        UZ_DF_EACH(w, l) p[l] = k0 + l < UZ_DY_LL && C.ll_len[k0 + l] ? 1u : 0u;
        const uint64_t m = w.ballot(p);
        if (m) hlit = k0 + 64 - (uint32_t)__builtin_clzll(m);
    }
    UZ_DF_EACH(w, l) p[l] = l < UZ_DY_D && C.d_len[l] ? 1u : 0u;
    {
        const uint64_t m = w.ballot(p);
        if (m) hdist = 64 - (uint32_t)__builtin_clzll(m);
    }
    const uint32_t n_lens = hlit + hdist;
    for (uint32_t k0 = 0; k0 < n_lens; k0 += 64) {
        UZ_DF_EACH(w, l) {
            const uint32_t k = k0 + l;
            if (k < n_lens) C.lens[k] = k < hlit ? C.ll_len[k] : C.d_len[k - hlit];
        }
    }
    w.sync();
    UZ_DF_EACH(w, l) {
        if (l != 0) continue;
        uint32_t n_cl = 0;
        for (uint32_t i = 0; i < n_lens;) {
            const uint32_t v = C.lens[i];
            uint32_t run = 1;
            while (i + run < n_lens && C.lens[i + run] == v) run++;
            i += run;
            uint32_t s, take;
            if (v) { C.cl_list[n_cl++] = (uint16_t)v; C.cl_hist[v]++; run--; }
            while (run >= 3) {
                if (v) { s = 16; take = run < 6 ? run : 6; C.cl_list[n_cl] = (uint16_t)(s | ((take - 3) << 8)); }
                else if (run >= 11) { s = 18; take = run < 138 ? run : 138; C.cl_list[n_cl] = (uint16_t)(s | ((take - 11) << 8)); }
                else { s = 17; take = run; C.cl_list[n_cl] = (uint16_t)(s | ((take - 3) << 8)); }
                n_cl++;
                C.cl_hist[s]++;
                run -= take;
            }
            for (; run; run--) { C.cl_list[n_cl++] = (uint16_t)v; C.cl_hist[v]++; }
        }
        C.n_cl = n_cl;
    }
    w.sync();
    const uint32_t n_cl = C.n_cl;
    uz_dy_build(w, C.B, C.cl_hist, UZ_DY_CL, 7, C.cl_len, C.cl_code);
    UZ_DF_EACH(w, l) p[l] = l < UZ_DY_CL && C.cl_len[uz_dy_cl_order(l < UZ_DY_CL ? l : 0)] ? 1u : 0u;
    uint32_t hclen = 4;
    {
        const uint64_t m = w.ballot(p);
        if (m && 64 - (uint32_t)__builtin_clzll(m) > hclen) hclen = 64 - (uint32_t)__builtin_clzll(m);
    }
    // the three sizes
    Lane bits_d, bits_f, unused;
    UZ_DF_EACH(w, l) {
        uint32_t d = 0, f = 0;
        for (uint32_t s = l; s < UZ_DY_LL; s += 64) {
            const uint32_t c = S.hist[s], x = uz_dy_ll_extra(s);
            d += c * (C.ll_len[s] + x);
            f += c * ((s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u) + x);
        }
        if (l < UZ_DY_D) {
            const uint32_t c = hist_d[l], x = uz_dy_d_extra(l);
            d += c * (C.d_len[l] + x);
            f += c * (5 + x);
        }
        if (l < UZ_DY_CL) d += C.cl_hist[l] * (C.cl_len[l] + uz_dy_cl_extra(l));
        bits_d[l] = d; bits_f[l] = f;
    }
    uint32_t dyn_bits = 0, fix_bits = 0;
    w.excl_scan(bits_d, unused, dyn_bits);
    w.excl_scan(bits_f, unused, fix_bits);
    dyn_bits += 3 + 14 + 3 * hclen;
    fix_bits += 3;
    const uint32_t dyn_bytes = (dyn_bits + 7) >> 3, fix_bytes = (fix_bits + 7) >> 3;
    kind = dyn_bytes < fix_bytes ? UZ_DY_DYNAMIC : UZ_DY_FIXED;
    if ((dyn_bytes < fix_bytes ? dyn_bytes : fix_bytes) > limit) {
        kind = UZ_DY_STORED;
        return uz_df_store_raw(w, in, n, out);
    }
    // pass 2
    uint32_t bitpos = 0, wbase = 0 /* the stream's word that window[0] is */;
    Lane64 bits;
    Lane nb;
    if (kind == UZ_DY_FIXED) {
        w.sync(); // (the sizes were read from the tables the fixed code now takes)
        for (uint32_t k0 = 0; k0 < UZ_DY_LL; k0 += 64) {
            UZ_DF_EACH(w, l) {
                if (k0 + l < UZ_DY_LL) {
                    uint32_t b = 0;
                    const uint32_t c = uz_df_litlen(k0 + l, b);
                    C.ll_code[k0 + l] = (c << 5) | b;
                }
            }
        }
        UZ_DF_EACH(w, l) if (l < UZ_DY_D) C.d_code[l] = (uz_df_rev(l, 5) << 5) | 5u;
        w.sync();
        UZ_DF_EACH(w, l) { bits[l] = 3; nb[l] = l == 0 ? 3u : 0u; } // BFINAL = 1, BTYPE = 01
        uz_dy_put(w, C.win, bits, nb, bitpos, wbase, out, cap);
    } else {
        UZ_DF_EACH(w, l) {
            bits[l] = 0; nb[l] = 0;
            if (l == 0) { bits[l] = 1u | (2u << 1) | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((hclen - 4) << 13); nb[l] = 17; } // BFINAL = 1, BTYPE = 10
            else if (l <= hclen) { bits[l] = C.cl_len[uz_dy_cl_order(l - 1)]; nb[l] = 3; }
        }
        uz_dy_put(w, C.win, bits, nb, bitpos, wbase, out, cap);
        for (uint32_t k0 = 0; k0 < n_cl; k0 += 64) {
            UZ_DF_EACH(w, l) {
                bits[l] = 0; nb[l] = 0;
                if (k0 + l < n_cl) {
                    const uint32_t e = C.cl_list[k0 + l], s = e & 31u, c = C.cl_code[s];
                    bits[l] = (c >> 5) | ((e >> 8) << (c & 31u));
                    nb[l] = (c & 31u) + uz_dy_cl_extra(s);
                }
            }
            uz_dy_put(w, C.win, bits, nb, bitpos, wbase, out, cap);
        }
    }
    for (uint32_t k0 = 0; k0 < n_tok + 1; k0 += 64) { // (behind the last token: end of block)
        UZ_DF_EACH(w, l) {
            const uint32_t k = k0 + l;
            uint64_t b = 0;
            uint32_t nbit = 0;
            if (k <= n_tok) {
                const uint32_t t = k < n_tok ? tok[k] : 256u;
                if (t >> 31) {
                    uint32_t sym, le, lx, dsym, de, dx;
                    uz_df_len_sym(((t >> 16) & 0xFFu) + 3, sym, le, lx);
                    uz_df_dist_sym((t & 0x7FFFu) + 1, dsym, de, dx);
                    const uint32_t c = C.ll_code[sym], d = C.d_code[dsym];
                    b = c >> 5; nbit = c & 31u;
                    b |= (uint64_t)lx << nbit; nbit += le;
                    b |= (uint64_t)(d >> 5) << nbit; nbit += d & 31u;
                    b |= (uint64_t)dx << nbit; nbit += de;
                } else {
                    const uint32_t c = C.ll_code[t];
                    b = c >> 5; nbit = c & 31u;
                }
            }
            bits[l] = b; nb[l] = nbit;
        }
        uz_dy_put(w, C.win, bits, nb, bitpos, wbase, out, cap);
    }
    const uint32_t words = ((bitpos + 31) >> 5) - wbase;
    uz_df_store_words(w, C.win, wbase, words, out, cap);
    return (bitpos + 7) >> 3; // zero padding to the byte
}
