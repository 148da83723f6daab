// io_vcf_cell.hpp -- the host's ONE statement of how a sample column of a text VCF is read: GT, AD (or RO / AO) and GQ of one cell, by the
// FORMAT slots of its record.  io_vcf.cpp runs it for the eager decode, for uz_vcf_fill_samples and for uz_vcf_record_samples;
// tests/vcf_cell_main.cpp holds the device's parser (vcf_cell.hpp) against it.  Host only, no dependency beyond the C++ library.
//
// Field semantics are those of unfazed_amd/io_vcf.py (cyvcf2 as the reference uses it, informative_site_finder.py:257-260): genotype codes
// HOM_REF 0, HET 1, UNKNOWN 2, HOM_ALT 3; half-missing calls count with their called allele, haploid calls as homozygous; depths from
// FORMAT/AD (first ALT) falling back to RO / AO, missing -> -1; GQ as a float, missing -> -1.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace uzcell {

struct Str {
    const char *p;
    size_t n;
    bool eq(const char *s) const { return strlen(s) == n && memcmp(p, s, n) == 0; }
};

struct BadAllele { // a genotype allele that is neither "." nor an integer: the decode fails (UZ_IO_E_FORMAT)
    std::string text;
};

// Python int(x) for the plain forms a VCF holds: optional sign, decimal digits
inline bool parse_int(Str s, long long &out) {
    if (s.n == 0 || s.n > 18) return false;
    size_t i = 0;
    bool neg = false;
    if (s.p[0] == '-' || s.p[0] == '+') { neg = s.p[0] == '-'; i = 1; }
    if (i >= s.n) return false;
    long long v = 0;
    for (; i < s.n; i++) {
        if (s.p[i] < '0' || s.p[i] > '9') return false;
        v = v * 10 + (s.p[i] - '0');
    }
    out = neg ? -v : v;
    return true;
}

inline long long num_int(Str s) { // io_vcf._num(x, int): "." / "" / unparsable -> -1
    long long v;
    if (s.n == 0 || s.eq(".")) return -1;
    return parse_int(s, v) ? v : -1;
}

inline double num_float(Str s) { // io_vcf._num(x, float, -1.0)
    if (s.n == 0 || s.eq(".") || s.n > 63) return -1.0;
    char buf[64];
    memcpy(buf, s.p, s.n);
    buf[s.n] = 0;
    char *e = nullptr;
    const double v = strtod(buf, &e);
    if (e == buf || *e != 0) return -1.0;
    return v;
}

// k-th ':'-separated piece of a sample column (or of FORMAT)
inline bool piece(Str col, int k, Str &out) {
    const char *p = col.p, *end = col.p + col.n;
    for (int i = 0;; i++) {
        const char *q = (const char *)memchr(p, ':', (size_t)(end - p));
        const char *stop = q ? q : end;
        if (i == k) { out = Str{p, (size_t)(stop - p)}; return true; }
        if (!q) return false;
        p = q + 1;
    }
}

inline int parse_gt(Str g) {
    enum { UNKNOWN = 2 };
    if (g.eq(".") || g.eq("./.") || g.eq(".|.")) return UNKNOWN;
    long long al[2] = {-1, -1};
    int na = 0;
    const char *p = g.p, *end = g.p + g.n;
    while (p <= end) {
        const char *q = p;
        while (q < end && *q != '/' && *q != '|') q++;
        if (na < 2) {
            const Str a{p, (size_t)(q - p)};
            long long v = -1;
            if (!a.eq(".")) { if (!parse_int(a, v)) throw BadAllele{std::string(a.p, a.n)}; }
            al[na] = v;
        }
        na++;
        if (q >= end) break;
        p = q + 1;
    }
    if (na == 1) return al[0] < 0 ? UNKNOWN : (al[0] == 0 ? 0 : 3);
    const long long a = al[0], b = al[1];
    if (a < 0 && b < 0) return UNKNOWN;
    if (a < 0 || b < 0) { const long long c = b < 0 ? a : b; return c == 0 ? 0 : 1; }
    if (a != b) return 1;
    return a == 0 ? 0 : 3;
}

// the FORMAT slots of the five keys a cell is read by (-1: the key is absent); the last occurrence of a key wins
enum { SLOT_GT = 0, SLOT_AD = 1, SLOT_RO = 2, SLOT_AO = 3, SLOT_GQ = 4 };
inline void format_slots(Str format, int slot[5]) {
    for (int k = 0; k < 5; k++) slot[k] = -1;
    Str pc;
    for (int k = 0; piece(format, k, pc); k++) {
        if (pc.eq("GT")) slot[SLOT_GT] = k; else if (pc.eq("AD")) slot[SLOT_AD] = k; else if (pc.eq("RO")) slot[SLOT_RO] = k;
        else if (pc.eq("AO")) slot[SLOT_AO] = k; else if (pc.eq("GQ")) slot[SLOT_GQ] = k;
    }
}

// one cell: `col` is the sample's column ("." for a column the line is too short to hold).  A field whose piece the column does not
// reach keeps its default: gt UNKNOWN, depths and GQ -1.
inline void sample_cell(Str col, const int slot[5], uint8_t &gt, int32_t &ref_depth, int32_t &alt_depth, double &gq) {
    gt = 2; ref_depth = alt_depth = -1; gq = -1.0;
    Str v;
    if (slot[SLOT_GT] >= 0 && piece(col, slot[SLOT_GT], v)) gt = (uint8_t)parse_gt(v);
    bool ad_done = false;
    if (slot[SLOT_AD] >= 0 && piece(col, slot[SLOT_AD], v) && !v.eq(".")) {
        const char *cm = (const char *)memchr(v.p, ',', v.n);
        const Str a0{v.p, cm ? (size_t)(cm - v.p) : v.n};
        ref_depth = (int32_t)num_int(a0);
        if (cm) {
            const char *c2 = (const char *)memchr(cm + 1, ',', (size_t)(v.p + v.n - cm - 1));
            const Str a1{cm + 1, c2 ? (size_t)(c2 - cm - 1) : (size_t)(v.p + v.n - cm - 1)};
            alt_depth = (int32_t)num_int(a1);
        } else alt_depth = -1;
        ad_done = true;
    }
    Str ro, ao;
    if (!ad_done && slot[SLOT_RO] >= 0 && slot[SLOT_AO] >= 0 && piece(col, slot[SLOT_RO], ro) && piece(col, slot[SLOT_AO], ao)) {
        ref_depth = (int32_t)num_int(ro);
        const char *cm = (const char *)memchr(ao.p, ',', ao.n);
        alt_depth = (int32_t)num_int(Str{ao.p, cm ? (size_t)(cm - ao.p) : ao.n});
    }
    if (slot[SLOT_GQ] >= 0 && piece(col, slot[SLOT_GQ], v)) gq = num_float(v);
}

} // namespace uzcell
