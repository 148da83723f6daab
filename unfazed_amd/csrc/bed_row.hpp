// bed_row.hpp -- one row of the BED output as text, from the read stage's result where it lies: the decision of summarize_record
// (reference unfazed.py:206-234, a record without allele-balance lists), the SEX-CHROM row of summarize_autophased (:162-187) and the line of
// write_bed_output (:444-515).  __host__ __device__: k_bed_size / k_bed_fill (k_bed.hip) and tests/bed_row_main.cpp run this very body.
//
// The body is written for a group of LANES lanes that share one row (the kernels: a wavefront; the host program: one lane).  `W` gives the lane
// index and the three cross-lane steps the walk needs (exclusive scan, sum, broadcast); everything else is lane-private or uniform.
//
//   line     chrom start end vartype kid origin other count types [origin_sites origin_reads other_sites other_reads], tab-separated, '\n'
//   decision uz_bed_decide: the table of the four branches, 64-bit products
//   dropped  origin None or ambiguous without include_ambiguous; a DNM whose status is not UZ_ST_OK: zero bytes
//   lists    joined with ',', an empty list prints '-'; read names in list order; SITES SORTED AS DECIMAL STRINGS (:302-303: [9, 10] prints 10,9)
//   integers as Python's str(int): a sign is possible, no padding
//
// Site lists are ascending and distinct in the read stage's pool (and non-negative: positions).  Such a list is at most ten runs by digit count,
// each already in string order, and the string order of two numbers is the order of (v * 10^(10 - digits), digits).  So an element's rank and its
// byte offset in the sorted output are sums over the ten runs of binary searches in the list itself: no sort, no scratch, no length limit.  The
// size walk verifies what this assumes (UZ_BED_F_ORDER on a list that is not ascending, or holds a negative value).
//
// Size and fill are ONE walk (uz_bed_row_walk<FILL>): the fill pass returns the bytes it walked, and its caller holds them against the sized
// length (UZ_BED_F_SIZE).  Every store of the fill pass is held inside the row's sized length as well.
#pragma once
#include <stdint.h>

#include "uz_bamwalk.h"
#include "uz_types.h"

#if defined(__HIPCC__)
#define UZ_BR_HD __host__ __device__ __forceinline__
#else
#define UZ_BR_HD inline
#endif

#define UZ_BED_F_ORDER 1u /* a site list is not ascending (or holds a negative value) */
#define UZ_BED_F_NAME 2u  /* a name id at or beyond the table's n_qnames, or a name the table's store does not hold */
#define UZ_BED_F_SIZE 4u  /* a row's written bytes differ from its sized length */

// one lane: the host program's group
struct UzBedLane1 {
    static constexpr uint32_t LANES = 1;
    UZ_BR_HD uint32_t lane() const { return 0; }
    UZ_BR_HD uint32_t excl_scan(uint32_t v, uint32_t &total) const { total = v; return 0; }
    UZ_BR_HD uint32_t bcast(uint32_t v, uint32_t) const { return v; }
    UZ_BR_HD const uint8_t *bcast_ptr(const uint8_t *p, uint32_t) const { return p; }
};

struct UzBedDecision {
    int32_t origin; // UZ_OR_*
    int64_t count;
    bool ambiguous; // the AMBIGUOUS_READBACKED branch
};

// summarize_record's read-backed branches, in their order
UZ_BR_HD UzBedDecision uz_bed_decide(int64_t n_dad, int64_t n_mom, int64_t s_dad, int64_t s_mom, int64_t ratio) {
    UzBedDecision d;
    d.origin = UZ_OR_NONE; d.count = 0; d.ambiguous = false;
    if (n_dad > 0 && n_dad >= ratio * n_mom) { d.origin = UZ_OR_DAD; d.count = s_dad; }
    else if (n_mom > 0 && n_mom >= ratio * n_dad) { d.origin = UZ_OR_MOM; d.count = s_mom; }
    else if (n_dad > 0 && n_mom > 0) { d.origin = UZ_OR_AMBIGUOUS; d.count = n_dad + n_mom; d.ambiguous = true; }
    return d;
}

// the names a row's read ids belong to: the walked table's form (name_rec set) or a plain store (plain_off [n_qnames + 1], plain_bytes)
struct UzBedNames {
    const uint32_t *name_rec;
    const uz_kept_rec *kept;
    const uint8_t *names;
    int64_t n_recs, names_bytes;
    const uint32_t *plain_off;
    const uint8_t *plain_bytes;
    uint32_t n_qnames;
    uint32_t has_names;
};

// the name of id -> true; false (nothing read beyond the id's own entry, flag raised): an id out of range, a name outside the store
UZ_BR_HD bool uz_bed_name(const UzBedNames &T, uint32_t id, const uint8_t *&p, uint32_t &len, uint32_t &flags) {
    p = nullptr; len = 0;
    if (id >= T.n_qnames) { flags |= UZ_BED_F_NAME; return false; }
    if (T.name_rec) {
        const uint32_t r = T.name_rec[id];
        if ((int64_t)r >= T.n_recs) { flags |= UZ_BED_F_NAME; return false; }
        const int64_t a = T.kept[r].name_off, b = (int64_t)r + 1 < T.n_recs ? (int64_t)T.kept[r + 1].name_off : T.names_bytes;
        if (b < a || b > T.names_bytes) { flags |= UZ_BED_F_NAME; return false; }
        p = T.names + a; len = (uint32_t)(b - a);
    } else {
        const uint32_t a = T.plain_off[id], b = T.plain_off[id + 1];
        if (b < a) { flags |= UZ_BED_F_NAME; return false; }
        p = T.plain_bytes + a; len = b - a;
    }
    return true;
}

struct UzBedStrings { // the fixed strings of a call: id -> bytes [off[id], off[id + 1])
    const uint32_t *off;
    const uint8_t *bytes;
};

struct UzBedRowDev { // a row as the kernels take it (uz_bed_row of the view + the table's slot among the call's tables + the cohort's name base)
    int32_t dnm, start, end; // dnm < 0: a SEX-CHROM row
    uint32_t chrom, vartype, kid, dad, mom;
    int32_t table;
    uint32_t qbase;
    int32_t sex_origin; // SEX-CHROM: 0 dad is the origin, 1 mom
};

// where a batch's lists lie.  The read stage's form: pool + list_start [n] (< 0: no lists) + list_len [6 n]; without the pool (a batch run without
// lists) the four lengths are `counts` [4 n] and no list can be read.  The caller's form (uz_bed_rows_lists): off4 [4 n + 1] + pool.
struct UzBedLists {
    const int32_t *status;
    const int32_t *pool;
    const int64_t *off4;
    const long long *list_start;
    const int32_t *list_len;
    const int32_t *counts;
};
struct UzBedRowLists { // dad reads, mom reads, dad sites, mom sites
    const int32_t *rd, *rm, *sd, *sm;
    uint32_t n_rd, n_rm, n_sd, n_sm;
};
UZ_BR_HD UzBedRowLists uz_bed_row_lists(const UzBedLists &L, int32_t d) {
    UzBedRowLists r;
    r.rd = r.rm = r.sd = r.sm = nullptr;
    r.n_rd = r.n_rm = r.n_sd = r.n_sm = 0;
    if (L.off4) {
        const int64_t *o = L.off4 + (size_t)4 * (size_t)d;
        r.rd = L.pool + o[0]; r.rm = L.pool + o[1]; r.sd = L.pool + o[2]; r.sm = L.pool + o[3];
        r.n_rd = (uint32_t)(o[1] - o[0]); r.n_rm = (uint32_t)(o[2] - o[1]); r.n_sd = (uint32_t)(o[3] - o[2]); r.n_sm = (uint32_t)(o[4] - o[3]);
    } else if (L.list_start) {
        const long long s = L.list_start[d];
        if (s >= 0) {
            const int32_t *n = L.list_len + (size_t)6 * (size_t)d;
            r.n_rd = (uint32_t)n[0]; r.n_rm = (uint32_t)n[1]; r.n_sd = (uint32_t)n[2]; r.n_sm = (uint32_t)n[3];
            r.rd = L.pool + s; r.rm = r.rd + r.n_rd; r.sd = r.rm + r.n_rm; r.sm = r.sd + r.n_sd;
        }
    } else {
        const int32_t *n = L.counts + (size_t)4 * (size_t)d;
        r.n_rd = (uint32_t)n[0]; r.n_rm = (uint32_t)n[1]; r.n_sd = (uint32_t)n[2]; r.n_sm = (uint32_t)n[3];
    }
    return r;
}

// ---- the pieces of a line.  `o` is the row's running length (uniform over the lanes); FILL: the lanes write out[o ...), every store below `limit`
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_bytes(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, const uint8_t *s, uint32_t len) {
    if (FILL)
        for (uint32_t b = w.lane(); b < len; b += W::LANES)
            if (o + b < limit) out[o + b] = s[b];
    o += len;
}
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_lit(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, const char *s, uint32_t len) {
    uz_bed_put_bytes<FILL>(w, out, limit, o, reinterpret_cast<const uint8_t *>(s), len);
}
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_ch(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, char ch) {
    if (FILL && w.lane() == 0 && o < limit) out[o] = (uint8_t)ch;
    o += 1;
}
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_str(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, const UzBedStrings &S, uint32_t id) {
    const uint32_t a = S.off[id], b = S.off[id + 1];
    uz_bed_put_bytes<FILL>(w, out, limit, o, S.bytes + a, b >= a ? b - a : 0u);
}
UZ_BR_HD uint32_t uz_bed_digits(uint64_t u) {
    uint32_t d = 1;
    while (u >= 10u) { u /= 10u; d++; }
    return d;
}
UZ_BR_HD uint64_t uz_bed_pow10(uint32_t e) {
    uint64_t p = 1;
    for (uint32_t k = 0; k < e; k++) p *= 10u;
    return p;
}
// str(int): lane b writes character b
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_int(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, int64_t v) {
    const uint32_t neg = v < 0 ? 1u : 0u;
    const uint64_t u = neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    const uint32_t d = uz_bed_digits(u);
    if (FILL)
        for (uint32_t b = w.lane(); b < neg + d; b += W::LANES)
            if (o + b < limit) out[o + b] = b < neg ? (uint8_t)'-' : (uint8_t)('0' + (u / uz_bed_pow10(d - 1 - (b - neg))) % 10u);
    o += neg + d;
}

// first index of the ascending list whose value is >= x
UZ_BR_HD uint32_t uz_bed_lower(const int32_t *v, uint32_t n, int64_t x) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if ((int64_t)v[m] < x) a = m + 1; else b = m;
    }
    return a;
}

// a site list in the order of its decimal strings (see the head of the file)
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_sites(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, const int32_t *v, uint32_t n, uint32_t &flags) {
    if (n == 0) { uz_bed_put_ch<FILL>(w, out, limit, o, '-'); return; }
    if (!FILL) {
        for (uint32_t i = w.lane(); i < n; i += W::LANES)
            if (v[i] < 0 || (i > 0 && v[i] <= v[i - 1])) flags |= UZ_BED_F_ORDER;
    }
    // the list's bytes: every element its digits and a comma, less the last comma
    uint32_t total = 0;
    {
        uint32_t lo = 0;
        uint64_t p = 10; // 10^e
        for (uint32_t e = 1; e <= 10; e++, p *= 10u) {
            const uint32_t hi = e == 10 ? n : uz_bed_lower(v, n, (int64_t)p);
            total += (hi >= lo ? hi - lo : 0u) * (e + 1);
            lo = hi;
        }
        total -= 1;
    }
    if (FILL) {
        for (uint32_t i = w.lane(); i < n; i += W::LANES) {
            const uint64_t x = (uint64_t)(uint32_t)v[i];
            const uint32_t d = uz_bed_digits(x);
            // elements of run e (e digits) that stand before x: those below x * 10^(e - d) (e >= d), those at or below x / 10^(d - e) (e < d: a
            // proper prefix of equal leading digits is the shorter string)
            uint32_t rank = 0, pos = 0, lo = 0;
            uint64_t p = 10;
            for (uint32_t e = 1; e <= 10; e++, p *= 10u) {
                const uint32_t hi = e == 10 ? n : uz_bed_lower(v, n, (int64_t)p);
                const int64_t bound = e >= d ? (int64_t)(x * uz_bed_pow10(e - d)) : (int64_t)(x / uz_bed_pow10(d - e)) + 1;
                uint32_t k = uz_bed_lower(v, n, bound);
                k = k < lo ? lo : (k > hi ? hi : k);
                if (hi > lo) { rank += k - lo; pos += (k - lo) * (e + 1); }
                lo = hi;
            }
            for (uint32_t b = 0; b < d; b++)
                if (pos + b < total && o + pos + b < limit) out[o + pos + b] = (uint8_t)('0' + (x / uz_bed_pow10(d - 1 - b)) % 10u);
            if (rank + 1 < n && pos + d < total && o + pos + d < limit) out[o + pos + d] = (uint8_t)',';
        }
    }
    o += total;
}

// a list of read names in list order.  The lanes take LANES ids at a time: each looks its own name up, a scan places the names, and every name
// is then copied by all lanes together (consecutive lanes, consecutive bytes)
template <bool FILL, class W>
UZ_BR_HD void uz_bed_put_names(const W &w, uint8_t *out, uint32_t limit, uint32_t &o, const int32_t *ids, uint32_t n, uint32_t qbase, const UzBedNames &T,
                               uint32_t &flags) {
    if (n == 0) { uz_bed_put_ch<FILL>(w, out, limit, o, '-'); return; }
    for (uint32_t c0 = 0; c0 < n; c0 += W::LANES) { // (uniform trip count)
        const uint32_t i = c0 + w.lane();
        const uint8_t *p = nullptr;
        uint32_t len = 0;
        if (i < n) uz_bed_name(T, (uint32_t)ids[i] - qbase, p, len, flags);
        const uint32_t l = i < n ? len + (i + 1 < n ? 1u : 0u) : 0u; // (a comma behind every name but the last)
        uint32_t tot = 0;
        const uint32_t ex = w.excl_scan(l, tot);
        if (FILL) {
            const uint32_t m = n - c0 < W::LANES ? n - c0 : W::LANES;
            for (uint32_t k = 0; k < m; k++) {
                const uint8_t *sp = w.bcast_ptr(p, k);
                const uint32_t sl = w.bcast(len, k), so = o + w.bcast(ex, k);
                for (uint32_t b = w.lane(); b < sl; b += W::LANES)
                    if (so + b < limit) out[so + b] = sp[b];
                if (c0 + k + 1 < n && w.lane() == 0 && so + sl < limit) out[so + sl] = (uint8_t)',';
            }
        }
        o += tot;
    }
}

// ---- the row.  -> its bytes (0: the row is dropped).  FILL: written to out[0 ...), no store at or beyond `limit` (the row's sized length)
template <bool FILL, class W>
UZ_BR_HD uint32_t uz_bed_row_walk(const W &w, const UzBedRowDev &R, const UzBedLists &L, const UzBedNames *tables, const UzBedStrings &S, int64_t ratio,
                                  int verbose, int include_ambiguous, uint8_t *out, uint32_t limit, uint32_t &flags) {
    const bool sex = R.dnm < 0;
    UzBedRowLists q;
    UzBedDecision dec;
    if (sex) {
        q = UzBedRowLists();
        dec.origin = R.sex_origin ? UZ_OR_MOM : UZ_OR_DAD; dec.count = 1; dec.ambiguous = false;
    } else {
        if (L.status[R.dnm] != UZ_ST_OK) return 0;
        q = uz_bed_row_lists(L, R.dnm);
        dec = uz_bed_decide(q.n_rd, q.n_rm, q.n_sd, q.n_sm, ratio);
        if ((dec.origin == UZ_OR_NONE || dec.ambiguous) && !include_ambiguous) return 0;
        if (dec.origin == UZ_OR_NONE) q = UzBedRowLists(); // (no branch taken: summarize_record has moved no list into the row's four)
    }
    uint32_t o = 0;
    uz_bed_put_str<FILL>(w, out, limit, o, S, R.chrom); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    uz_bed_put_int<FILL>(w, out, limit, o, R.start); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    uz_bed_put_int<FILL>(w, out, limit, o, R.end); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    uz_bed_put_str<FILL>(w, out, limit, o, S, R.vartype); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    uz_bed_put_str<FILL>(w, out, limit, o, S, R.kid); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    // origin_parent, other_parent
    if (dec.origin == UZ_OR_DAD || dec.origin == UZ_OR_MOM) {
        const bool dad = dec.origin == UZ_OR_DAD;
        uz_bed_put_str<FILL>(w, out, limit, o, S, dad ? R.dad : R.mom); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
        uz_bed_put_str<FILL>(w, out, limit, o, S, dad ? R.mom : R.dad); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    } else {
        if (dec.origin == UZ_OR_AMBIGUOUS) {
            uz_bed_put_str<FILL>(w, out, limit, o, S, R.dad); uz_bed_put_ch<FILL>(w, out, limit, o, '|'); uz_bed_put_str<FILL>(w, out, limit, o, S, R.mom);
        } else
            uz_bed_put_lit<FILL>(w, out, limit, o, "None", 4);
        uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
        uz_bed_put_lit<FILL>(w, out, limit, o, "None", 4); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    }
    uz_bed_put_int<FILL>(w, out, limit, o, dec.count); uz_bed_put_ch<FILL>(w, out, limit, o, '\t');
    if (sex) uz_bed_put_lit<FILL>(w, out, limit, o, "SEX-CHROM", 9);
    else if (dec.ambiguous) uz_bed_put_lit<FILL>(w, out, limit, o, "AMBIGUOUS_READBACKED", 20);
    else if (dec.origin != UZ_OR_NONE) uz_bed_put_lit<FILL>(w, out, limit, o, "READBACKED", 10);
    if (verbose) {
        if (sex) {
            for (int k = 0; k < 4; k++) { uz_bed_put_ch<FILL>(w, out, limit, o, '\t'); uz_bed_put_lit<FILL>(w, out, limit, o, "NA", 2); }
        } else {
            // origin sites, origin reads, other sites, other reads: the origin is the dad's lists except in the mom branch
            const bool mom = dec.origin == UZ_OR_MOM;
            const UzBedNames &T = tables[R.table];
            uz_bed_put_ch<FILL>(w, out, limit, o, '\t'); uz_bed_put_sites<FILL>(w, out, limit, o, mom ? q.sm : q.sd, mom ? q.n_sm : q.n_sd, flags);
            uz_bed_put_ch<FILL>(w, out, limit, o, '\t'); uz_bed_put_names<FILL>(w, out, limit, o, mom ? q.rm : q.rd, mom ? q.n_rm : q.n_rd, R.qbase, T, flags);
            uz_bed_put_ch<FILL>(w, out, limit, o, '\t'); uz_bed_put_sites<FILL>(w, out, limit, o, mom ? q.sd : q.sm, mom ? q.n_sd : q.n_sm, flags);
            uz_bed_put_ch<FILL>(w, out, limit, o, '\t'); uz_bed_put_names<FILL>(w, out, limit, o, mom ? q.rd : q.rm, mom ? q.n_rd : q.n_rm, R.qbase, T, flags);
        }
    }
    uz_bed_put_ch<FILL>(w, out, limit, o, '\n');
    return o;
}
