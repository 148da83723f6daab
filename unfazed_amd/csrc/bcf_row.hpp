// bcf_row.hpp -- one BCF2 record into its VCF text line (unfazed.py: write_vcf_output on a BCF of DNMs, UZ_BCF_ROUTE; reference unfazed.py:530 takes
// such a file and writes text from it).  __host__ __device__: k_bcfout_size / k_bcfout_fill (k_bcfout.hip) and tests/bcf_row_main.cpp run this very
// body; unfazed_amd/bcf_text.py states the same rules in plain Python.
//
// The body is written for a group of LANES lanes that share one record (the kernels: a wavefront; the host program: one lane).  `W` gives the lane
// index and the cross-lane steps.  The shared block is a short chain of typed values that every lane walks alike (uniform); lane 0 stores its
// characters, strings are copied LANES bytes a step.  The individual block is lanes over SAMPLES: a lane sizes its own sample's cell, a scan over
// the lanes places the cells, the fill pass writes them; more samples than lanes run in rounds.
//
//   line     CHROM POS ID REF ALT QUAL FILTER INFO [FORMAT sample ...], tab-separated, closed by '\n' (the text is the rewriter's input as it is)
//   CHROM    the header's contig of id `chrom`            POS  pos + 1, decimal           ID  the typed string, length 0 -> "."
//   REF ALT  n_allele typed strings: the first, then the rest joined by ','; no alt -> "."
//   QUAL     bit pattern 0x7F800001 -> ".", else the float rule
//   FILTER   a typed integer vector of dictionary ids up to end-of-vector: the names joined by ';', none -> "."
//   INFO     n_info (key, value) joined by ';', none -> "."; a value of type 0 or length 0 is a Flag (the key alone), else key '=' the vector rule
//   FORMAT   only when n_fmt > 0 and n_sample > 0: the keys joined by ':', then per sample a tab and the sample's values of every field joined by
//            ':'; sample s of a field lies at s * count * size(type).  Otherwise the line ends behind INFO
//   vector   integers: entries up to end-of-vector joined by ',', the missing marker prints "."; floats the same with missing 0x7F800001 and
//            end-of-vector 0x7F800002; characters (type 7): the bytes up to the first NUL; nothing printed -> "."; type 0 -> "."
//   GT       a FORMAT field named exactly "GT" of an integer type, entries x up to end-of-vector, read SIGNED as every integer here (and as
//            bcf_cell.hpp reads them): entry k > 0 is preceded by '|' when x & 1 else '/'; the allele is "." when x >> 1 == 0 or x is the missing
//            marker, else (x >> 1) - 1; no entry -> ".".  int8 therefore holds alleles up to 62.  A GT of another type takes the vector rule
//   float    C's "%g" of the value widened to double, printed only where "%g" uses fixed notation: +-0, and values whose six-significant-digit
//            rounding lies in [1e-4, 1e6).  Exact in 64-bit integers: the value is m * 2^-s, m < 2^24, 4 <= s <= 37; m * 10^k, k <= 10, stays
//            below 2^58 and leaves an exact remainder for round-half-even; a carry to the next power of ten shifts the exponent
//   length   the escape 15 -> a typed scalar integer follows, wherever a length stands
//
// HANDED BACK (the record's flag is set, its length is 0, nothing is written; bcf_text.line writes the line or raises): a float outside the printed
// range; n_allele == 0; a dictionary id or contig id without a name; a key (INFO, FORMAT) that is not a scalar integer with a value; a type outside
// {0, 1, 2, 3, 5, 7}; an ID or allele that is not a string, a FILTER that is not an integer vector; a negative GT entry other than the two markers;
// a negative or non-scalar escaped length; a byte below 0x20 or above 0x7E in any copied string or name (the NUL padding behind a per-sample string
// is not copied); any typed value, length word or array that does not lie inside its block, a block outside the data; n_sample different from the
// header's sample count while n_fmt > 0; a line of 4 GiB.
//
// The body proves every bound itself, against l_shared / l_indiv and the data's end: it is safe on bytes no decoder has seen.  Size and fill are ONE
// walk (uz_bcf_row_walk<FILL>): the fill pass returns the bytes it walked and its caller holds them against the sized length (UZ_BR_F_SIZE); every
// store of the fill pass is held inside the record's sized length as well.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define UZ_BR_HD __host__ __device__ __forceinline__
#else
#define UZ_BR_HD inline
#endif

#define UZ_BR_F_SIZE 1u /* a record's written bytes differ from its sized length (or the fill pass met a record it would hand back) */

#define UZ_BR_FLOAT_MISSING 0x7F800001u
#define UZ_BR_FLOAT_EOV 0x7F800002u

// one lane: the host program's group
struct UzBrLane1 {
    static constexpr uint32_t LANES = 1;
    UZ_BR_HD uint32_t lane() const { return 0; }
    UZ_BR_HD uint32_t shfl_up(uint32_t v, uint32_t) const { return v; }
    UZ_BR_HD uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    UZ_BR_HD bool any(bool v) const { return v; }
};

struct UzBrTables { // what a record is read against
    const uint8_t *data;
    uint64_t data_bytes;
    const uint32_t *dict_off; // [n_dict + 1] FILTER / INFO / FORMAT names in dict_bytes; an undefined id is an empty name
    const uint8_t *dict_bytes;
    const uint32_t *ctg_off; // [n_ctg + 1] the header's contigs by id, likewise
    const uint8_t *ctg_bytes;
    uint32_t n_dict, n_ctg;
    uint32_t n_samples; // the header's
    uint32_t reserved0;
};

struct UzBrVal { // a typed value: n entries of `type` from `at`
    uint32_t type, n;
    uint64_t at;
};

UZ_BR_HD uint32_t uz_br_rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
UZ_BR_HD uint32_t uz_br_rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
UZ_BR_HD uint32_t uz_br_size(uint32_t type) { return type == 1u || type == 7u ? 1u : type == 2u ? 2u : (type == 3u || type == 5u) ? 4u : 0u; }
UZ_BR_HD bool uz_br_is_int(uint32_t type) { return type >= 1u && type <= 3u; }

#define UZ_BR_OK 0
#define UZ_BR_MISSING 1
#define UZ_BR_EOV 2
// entry k of an integer vector at p
UZ_BR_HD int uz_br_int(uint32_t type, const uint8_t *p, uint64_t k, int32_t &x) {
    int32_t lowest;
    if (type == 1u) { x = (int8_t)p[k]; lowest = -128; }
    else if (type == 2u) { x = (int16_t)uz_br_rd16(p + 2 * k); lowest = -32768; }
    else { x = (int32_t)uz_br_rd32(p + 4 * k); lowest = INT32_MIN; }
    return x == lowest ? UZ_BR_MISSING : x == lowest + 1 ? UZ_BR_EOV : UZ_BR_OK;
}

// the descriptor of a typed value at `at` inside [.., end): type, length (escape included) -> `at` moved behind it; false: outside the block or the rules
UZ_BR_HD bool uz_br_desc(const uint8_t *D, uint64_t &at, uint64_t end, UzBrVal &v) {
    if (at >= end) return false;
    const uint8_t b = D[at++];
    v.type = b & 15u;
    v.n = b >> 4;
    if (v.n == 15u) {
        if (at >= end) return false;
        const uint8_t b2 = D[at++];
        const uint32_t t2 = b2 & 15u, sz = uz_br_is_int(t2) ? uz_br_size(t2) : 0u;
        if (!sz || (b2 >> 4) != 1u || end - at < sz) return false;
        int32_t x = 0;
        if (uz_br_int(t2, D + at, 0, x) != UZ_BR_OK || x < 0) return false;
        at += sz;
        v.n = (uint32_t)x;
    }
    if (v.type > 7u || v.type == 4u || v.type == 6u) return false;
    v.at = at;
    return true;
}
// a typed value whose entries lie inside [.., end) as well -> `at` moved behind them
UZ_BR_HD bool uz_br_typed(const uint8_t *D, uint64_t &at, uint64_t end, UzBrVal &v) {
    if (!uz_br_desc(D, at, end, v)) return false;
    const uint64_t bytes = (uint64_t)v.n * uz_br_size(v.type);
    if (end - at < bytes) return false;
    at += bytes;
    return true;
}
// a key: a typed scalar integer with a value
UZ_BR_HD bool uz_br_key(const uint8_t *D, uint64_t &at, uint64_t end, int32_t &id) {
    UzBrVal v;
    if (!uz_br_typed(D, at, end, v) || !uz_br_is_int(v.type) || v.n != 1u) return false;
    return uz_br_int(v.type, D + v.at, 0, id) == UZ_BR_OK;
}
// the name of `id` in a table of names: [a, b) of its bytes; false: no such id, or an id without a name
UZ_BR_HD bool uz_br_name(const uint32_t *off, uint32_t n, int32_t id, uint32_t &a, uint32_t &b) {
    if (id < 0 || (uint32_t)id >= n) return false;
    a = off[id];
    b = off[id + 1];
    return b > a;
}

// Where the characters go.  `o` counts every character (the size pass only counts); a store needs FILL, `on` and o < limit.
template <bool FILL>
struct UzBrOut {
    uint8_t *out;
    uint32_t limit;
    uint64_t o;
    bool on;
    UZ_BR_HD void put(uint8_t ch) {
        if (FILL && on && o < limit) out[o] = ch;
        o++;
    }
    UZ_BR_HD void put_u32(uint32_t v) {
        uint32_t div = 1;
        while (v / div >= 10u) div *= 10u;
        for (; div; div /= 10u) put((uint8_t)('0' + v / div % 10u));
    }
    UZ_BR_HD void put_i64(int64_t v) { // |v| <= 2^31
        if (v < 0) { put('-'); v = -v; }
        put_u32((uint32_t)v);
    }
};

UZ_BR_HD bool uz_br_printable(uint8_t c) { return c >= 0x20u && c <= 0x7Eu; }

// n bytes copied by the whole group, LANES a step (every lane stores its own: `on` is not asked); a byte outside 0x20 .. 0x7E raises the LANE's flag
template <bool FILL, class W>
UZ_BR_HD void uz_br_copy(const W &w, UzBrOut<FILL> &E, const uint8_t *src, uint64_t n, bool &lane_bad) {
    for (uint64_t i = w.lane(); i < n; i += W::LANES) {
        const uint8_t c = src[i];
        if (!uz_br_printable(c)) lane_bad = true;
        if (FILL && E.o + i < E.limit) E.out[E.o + i] = c;
    }
    E.o += n;
}

// The float rule -> false: "%g" would not print fixed notation (nothing the caller keeps is written: the record goes back)
template <bool FILL>
UZ_BR_HD bool uz_br_float(UzBrOut<FILL> &E, uint32_t bits) {
    const uint32_t ex = bits >> 23 & 255u, fr = bits & 0x7FFFFFu;
    const bool neg = (bits >> 31) != 0;
    if (ex == 0u && fr == 0u) {
        if (neg) E.put('-');
        E.put('0');
        return true;
    }
    if (ex < 113u || ex > 146u) return false; // below 2^-14 (< 9.99995e-5) or from 2^20 (> 1e6) on; subnormals, infinities and NaNs with them
    const uint64_t m = fr | 0x800000u;
    const uint32_t s = 150u - ex; // 4 .. 37: the value is m / 2^s
    uint64_t p = 1, N = 0, q = 0;
    int32_t k = 0;
    for (; k <= 10; k++, p *= 10u) { // the k that brings the value into [1e5, 1e6); m * 10^10 < 2^58
        N = m * p;
        q = N >> s;
        if (q >= 100000u) break;
    }
    if (k > 10 || q >= 1000000u) return false;
    const uint64_t r = N & (((uint64_t)1 << s) - 1u), half = (uint64_t)1 << (s - 1u);
    if (r > half || (r == half && (q & 1u))) q++;
    if (q == 1000000u) { q = 100000u; k--; } // the carry
    if (k < 0 || k > 9) return false;        // 1e+06 and beyond, or an exponent below -4
    const int32_t X = 5 - k;                 // the decimal exponent, -4 .. 5
    uint32_t d = (uint32_t)q, nd = 6;
    while (nd > 1u && d % 10u == 0u) { d /= 10u; nd--; } // trailing zeros dropped
    if (neg) E.put('-');
    uint32_t div = 1;
    for (uint32_t i = 1; i < nd; i++) div *= 10u;
    if (X < 0) {
        E.put('0');
        E.put('.');
        for (int32_t z = 0; z < -X - 1; z++) E.put('0');
        for (; div; div /= 10u) E.put((uint8_t)('0' + d / div % 10u));
        return true;
    }
    const uint32_t ip = (uint32_t)X + 1u; // digits ahead of the point
    for (uint32_t i = 0; i < ip || i < nd; i++) {
        if (i == ip) E.put('.');
        if (i < nd) { E.put((uint8_t)('0' + d / div % 10u)); div /= 10u; }
        else E.put('0');
    }
    return true;
}

// The vector rule over value v (its entries proven inside the block).  STRIDED: called by the whole group alike (shared block) -- a string is
// copied LANES bytes a step; else lane-private (a sample's cell).
template <bool FILL, bool STRIDED, class W>
UZ_BR_HD void uz_br_vector(const W &w, UzBrOut<FILL> &E, const uint8_t *D, uint32_t type, uint64_t at, uint32_t n, bool &lane_bad) {
    const uint8_t *p = D + at;
    uint32_t printed = 0;
    if (type == 7u) {
        uint32_t len = 0;
        while (len < n && p[len] != 0u) len++;
        if (STRIDED) uz_br_copy<FILL>(w, E, p, len, lane_bad);
        else
            for (uint32_t i = 0; i < len; i++) {
                if (!uz_br_printable(p[i])) lane_bad = true;
                E.put(p[i]);
            }
        printed = len;
    } else if (type == 5u) {
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t bits = uz_br_rd32(p + 4 * (uint64_t)k);
            if (bits == UZ_BR_FLOAT_EOV) break;
            if (printed) E.put(',');
            if (bits == UZ_BR_FLOAT_MISSING) E.put('.');
            else if (!uz_br_float<FILL>(E, bits)) lane_bad = true;
            printed++;
        }
    } else if (uz_br_is_int(type)) {
        for (uint32_t k = 0; k < n; k++) {
            int32_t x = 0;
            const int st = uz_br_int(type, p, k, x);
            if (st == UZ_BR_EOV) break;
            if (printed) E.put(',');
            if (st == UZ_BR_MISSING) E.put('.');
            else E.put_i64(x);
            printed++;
        }
    }
    if (!printed) E.put('.');
}

template <bool FILL>
UZ_BR_HD void uz_br_gt(UzBrOut<FILL> &E, const uint8_t *D, uint32_t type, uint64_t at, uint32_t n, bool &lane_bad) {
    uint32_t printed = 0;
    for (uint32_t k = 0; k < n; k++) {
        int32_t x = 0;
        const int st = uz_br_int(type, D + at, k, x);
        if (st == UZ_BR_EOV) break;
        if (st == UZ_BR_MISSING) x = 0;
        if (x < 0) { lane_bad = true; break; }
        if (printed) E.put((x & 1) ? '|' : '/');
        if ((x >> 1) == 0) E.put('.');
        else E.put_u32((uint32_t)((x >> 1) - 1));
        printed++;
    }
    if (!printed) E.put('.');
}

// One sample's cell: a tab, then the sample's values of every FORMAT field joined by ':' (the chain [at, iend) of n_fmt fields, proven by the
// caller's uniform pass; every step is proven again here, and a step that fails raises the lane's flag)
template <bool FILL, class W>
UZ_BR_HD void uz_br_cell(const W &w, UzBrOut<FILL> &E, const UzBrTables &T, uint64_t at, uint64_t iend, uint32_t n_fmt, uint32_t n_smp, uint32_t s, bool &lane_bad) {
    const uint8_t *D = T.data;
    E.put('\t');
    for (uint32_t k = 0; k < n_fmt; k++) {
        int32_t id = 0;
        UzBrVal d;
        uint32_t a = 0, b = 0;
        if (!uz_br_key(D, at, iend, id) || !uz_br_name(T.dict_off, T.n_dict, id, a, b) || !uz_br_desc(D, at, iend, d)) { lane_bad = true; return; }
        const uint64_t per = (uint64_t)d.n * uz_br_size(d.type);
        if ((iend - at) / (n_smp ? n_smp : 1u) < per) { lane_bad = true; return; }
        const uint64_t mine = at + per * s;
        at += per * n_smp;
        if (k) E.put(':');
        const bool is_gt = b - a == 2u && T.dict_bytes[a] == 'G' && T.dict_bytes[a + 1] == 'T';
        if (is_gt && uz_br_is_int(d.type)) uz_br_gt<FILL>(E, D, d.type, mine, d.n, lane_bad);
        else uz_br_vector<FILL, false>(w, E, D, d.type, mine, d.n, lane_bad);
    }
}

// ---- the record at rec_at (the offset of its l_shared word in T.data).  -> its bytes, the closing '\n' included (0: handed back, hb set).
// FILL: written to out[0 ...), no store at or beyond `limit` (the sized length).  samp_at: where column 10 starts in the line (the '\n' when the
// line has none).
template <bool FILL, class W>
UZ_BR_HD uint32_t uz_bcf_row_walk(const W &w, const UzBrTables &T, uint64_t rec_at, uint8_t *out, uint32_t limit, uint32_t &samp_at, bool &hb) {
    const uint8_t *D = T.data;
    samp_at = 0;
    // (everything up to the sample rounds is uniform: every lane reads the same bytes and takes the same way)
    if (rec_at > T.data_bytes || T.data_bytes - rec_at < 8u) { hb = true; return 0; }
    const uint64_t ls = uz_br_rd32(D + rec_at), li = uz_br_rd32(D + rec_at + 4), rest = T.data_bytes - rec_at - 8u;
    if (ls < 24u || ls > rest || li > rest - ls) { hb = true; return 0; }
    uint64_t at = rec_at + 8u;
    const uint64_t send = at + ls, iend = send + li;
    const int32_t chrom = (int32_t)uz_br_rd32(D + at), pos = (int32_t)uz_br_rd32(D + at + 4);
    const uint32_t qual = uz_br_rd32(D + at + 12), nai = uz_br_rd32(D + at + 16), nfs = uz_br_rd32(D + at + 20);
    const uint32_t n_allele = nai >> 16, n_info = nai & 0xFFFFu, n_fmt = nfs >> 24, n_smp = nfs & 0xFFFFFFu;
    at += 24u;
    if (n_allele == 0u || (n_fmt && n_smp != T.n_samples)) { hb = true; return 0; }
    bool lane_bad = false; // (lane-private: bytes outside the printable range, floats outside the printed range)
    UzBrOut<FILL> E{out, limit, 0, w.lane() == 0u};
    UzBrVal v;
    uint32_t a = 0, b = 0;
    // CHROM, POS
    if (!uz_br_name(T.ctg_off, T.n_ctg, chrom, a, b)) { hb = true; return 0; }
    uz_br_copy<FILL>(w, E, T.ctg_bytes + a, b - a, lane_bad);
    E.put('\t');
    E.put_i64((int64_t)pos + 1);
    E.put('\t');
    // ID
    if (!uz_br_typed(D, at, send, v) || (v.type != 7u && v.n)) { hb = true; return 0; }
    if (v.n) uz_br_copy<FILL>(w, E, D + v.at, v.n, lane_bad); else E.put('.');
    E.put('\t');
    // REF, ALT
    for (uint32_t k = 0; k < n_allele; k++) {
        if (!uz_br_typed(D, at, send, v) || (v.type != 7u && v.n)) { hb = true; return 0; }
        if (k == 1u) E.put('\t');
        if (k > 1u) E.put(',');
        uz_br_copy<FILL>(w, E, D + v.at, v.n, lane_bad);
    }
    if (n_allele == 1u) { E.put('\t'); E.put('.'); }
    E.put('\t');
    // QUAL
    if (qual == UZ_BR_FLOAT_MISSING) E.put('.');
    else if (!uz_br_float<FILL>(E, qual)) { hb = true; return 0; }
    E.put('\t');
    // FILTER
    if (!uz_br_typed(D, at, send, v) || (!uz_br_is_int(v.type) && v.n)) { hb = true; return 0; }
    {
        uint32_t printed = 0;
        for (uint32_t k = 0; k < v.n; k++) {
            int32_t id = 0;
            const int st = uz_br_int(v.type, D + v.at, k, id);
            if (st == UZ_BR_EOV) break;
            if (st != UZ_BR_OK || !uz_br_name(T.dict_off, T.n_dict, id, a, b)) { hb = true; return 0; }
            if (printed) E.put(';');
            uz_br_copy<FILL>(w, E, T.dict_bytes + a, b - a, lane_bad);
            printed++;
        }
        if (!printed) E.put('.');
    }
    E.put('\t');
    // INFO
    for (uint32_t k = 0; k < n_info; k++) {
        int32_t id = 0;
        if (!uz_br_key(D, at, send, id) || !uz_br_name(T.dict_off, T.n_dict, id, a, b) || !uz_br_typed(D, at, send, v)) { hb = true; return 0; }
        if (k) E.put(';');
        uz_br_copy<FILL>(w, E, T.dict_bytes + a, b - a, lane_bad);
        if (v.type == 0u || v.n == 0u) continue; // a Flag
        E.put('=');
        uz_br_vector<FILL, true>(w, E, D, v.type, v.at, v.n, lane_bad);
    }
    if (!n_info) E.put('.');
    samp_at = 0;
    uint64_t samp = 0;
    const bool has_fmt = n_fmt && n_smp;
    if (has_fmt) {
        // FORMAT: the keys, and every field's array proven inside the block
        E.put('\t');
        uint64_t f = send;
        for (uint32_t k = 0; k < n_fmt; k++) {
            int32_t id = 0;
            if (!uz_br_key(D, f, iend, id) || !uz_br_name(T.dict_off, T.n_dict, id, a, b) || !uz_br_desc(D, f, iend, v)) { hb = true; return 0; }
            const uint64_t per = (uint64_t)v.n * uz_br_size(v.type);
            if ((iend - f) / n_smp < per) { hb = true; return 0; }
            f += per * n_smp;
            if (k) E.put(':');
            uz_br_copy<FILL>(w, E, T.dict_bytes + a, b - a, lane_bad);
        }
        samp = E.o + 1u;
        // the samples, LANES a round
        for (uint32_t s0 = 0; s0 < n_smp; s0 += W::LANES) { // (uniform trip count)
            const uint32_t s = s0 + w.lane();
            uint64_t len = 0;
            if (s < n_smp) {
                UzBrOut<false> C{nullptr, 0u, 0, true};
                uz_br_cell<false>(w, C, T, send, iend, n_fmt, n_smp, s, lane_bad);
                len = C.o;
            }
            uint64_t incl = len; // where the lane's cell ends among the round's
            for (uint32_t d = 1; d < W::LANES; d <<= 1) {
                const uint64_t y = (uint64_t)w.shfl_up((uint32_t)(incl >> 32), d) << 32 | w.shfl_up((uint32_t)incl, d);
                if (w.lane() >= d) incl += y;
            }
            if (FILL && s < n_smp) {
                UzBrOut<FILL> C{out, limit, E.o + incl - len, true};
                uz_br_cell<FILL>(w, C, T, send, iend, n_fmt, n_smp, s, lane_bad);
            }
            E.o += (uint64_t)w.bcast((uint32_t)(incl >> 32), W::LANES - 1u) << 32 | w.bcast((uint32_t)incl, W::LANES - 1u);
        }
    }
    if (!has_fmt) samp = E.o;
    E.put('\n');
    if (w.any(lane_bad) || E.o >= 0xFFFFFFFFull) { hb = true; return 0; }
    samp_at = (uint32_t)samp;
    return (uint32_t)E.o;
}
