// vcf_cell.hpp -- one sample cell of a text VCF -> the sample table's values (uz_types.h: uz_samples_view): genotype code, ref / alt depth and
// floor(GQ) in the 16-bit encoding, OR "unsettled".  __host__ __device__: k_vcf_cells (k_vcf.hip) and tests/vcf_cell_main.cpp run this very body.
//
// The parser settles only a plain grammar; whatever lies outside it is unsettled and goes back to the host's own reader
// (csrc/io_vcf_cell.hpp: uzcell::sample_cell, then uz_samples_pack).  A settled cell equals what those two make of the same bytes:
//   pieces   a field whose slot lies beyond the column's last ':' (or whose key FORMAT does not name) keeps its default: gt 2, depths and GQ missing
//   GT       alleles of 1-3 digits or ".", separated by '/' or '|'; only the first two are read (any ploidy); one allele = haploid
//   depths   "." or empty = missing; 1-5 digits with value <= 32767; signs, longer numbers, larger values (the wide list is the host's
//            business) and any other character: unsettled
//   AD       the first two comma-separated entries; one entry: alt missing; a bare "." (or a column too short for it) falls through to
//            RO / AO when FORMAT names both and the column reaches both; AO is read up to its first comma
//   GQ       "." or empty = missing; 1-5 digits with value <= 32767, optionally '.' and 1-6 digits: the integer part.  More fraction digits
//            (strtod may round 99.9999999999999999 up to 100), "99.", signs, exponents, a leading '.', nan / inf: unsettled
// Replaces, for the cells it settles, cyvcf2's gt_types / gt_ref_depths / gt_alt_depths / gt_quals (informative_site_finder.py:257-260).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UZ_VC_HD __host__ __device__ __forceinline__
#else
#define UZ_VC_HD inline
#endif

#define UZ_VC_MISSING 0xFFFFu /* UZ_U16_MISSING */
#define UZ_VC_MAX 32767u

struct UzVcfCell {
    uint32_t gt;      // 0 / 1 / 2 / 3
    uint32_t rd, ad, gq; // 16-bit encoding
    bool settled;
};

// every field at its default: a sample column the line is too short to hold (it reads as "."), a record without FORMAT or sample columns
UZ_VC_HD UzVcfCell uz_vcf_cell_default() {
    UzVcfCell c;
    c.gt = 2u; c.rd = c.ad = c.gq = UZ_VC_MISSING; c.settled = true;
    return c;
}

// decimal digits of [p + a, p + b): 1 .. max_digits of them and nothing else, value <= UZ_VC_MAX -> true
UZ_VC_HD bool uz_vc_digits(const uint8_t *p, uint32_t a, uint32_t b, uint32_t max_digits, uint32_t &out) {
    if (b <= a || b - a > max_digits) return false;
    uint32_t v = 0;
    for (uint32_t i = a; i < b; i++) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9u) return false;
        v = v * 10u + d;
    }
    out = v;
    return v <= UZ_VC_MAX;
}

// a depth entry [a, b): missing, a value, or not settled (-> false)
UZ_VC_HD bool uz_vc_depth(const uint8_t *p, uint32_t a, uint32_t b, uint32_t &out) {
    if (b == a || (b - a == 1 && p[a] == '.')) { out = UZ_VC_MISSING; return true; }
    return uz_vc_digits(p, a, b, 5, out);
}

// one genotype allele starting at i (< b or == b): "." -> -1, 1-3 digits -> the value; must end at b or at a separator.  i moves behind it.
UZ_VC_HD bool uz_vc_allele(const uint8_t *p, uint32_t &i, uint32_t b, int32_t &out) {
    uint32_t j = i;
    while (j < b && p[j] != '/' && p[j] != '|') j++;
    if (j - i == 1 && p[i] == '.') { out = -1; i = j; return true; }
    uint32_t v = 0;
    if (!uz_vc_digits(p, i, j, 3, v)) return false;
    out = (int32_t)v;
    i = j;
    return true;
}

UZ_VC_HD bool uz_vc_gt(const uint8_t *p, uint32_t a, uint32_t b, uint32_t &gt) {
    int32_t x = -1, y = -1;
    uint32_t i = a;
    if (!uz_vc_allele(p, i, b, x)) return false;
    if (i >= b) { gt = x < 0 ? 2u : (x == 0 ? 0u : 3u); return true; } // haploid
    i++; // the separator
    if (!uz_vc_allele(p, i, b, y)) return false;
    // (further alleles are not read, as on the host)
    if (x < 0 && y < 0) gt = 2u;
    else if (x < 0 || y < 0) gt = (y < 0 ? x : y) == 0 ? 0u : 1u;
    else if (x != y) gt = 1u;
    else gt = x == 0 ? 0u : 3u;
    return true;
}

UZ_VC_HD bool uz_vc_gq(const uint8_t *p, uint32_t a, uint32_t b, uint32_t &out) {
    if (b == a || (b - a == 1 && p[a] == '.')) { out = UZ_VC_MISSING; return true; }
    uint32_t dot = a;
    while (dot < b && p[dot] != '.') dot++;
    if (!uz_vc_digits(p, a, dot, 5, out)) return false;
    if (dot == b) return true;
    if (b - (dot + 1) < 1 || b - (dot + 1) > 6) return false;
    for (uint32_t i = dot + 1; i < b; i++)
        if ((uint32_t)p[i] - '0' > 9u) return false;
    return true;
}

// The cell [p, p + len) -- the sample column without its tab or line end -- read by the FORMAT slots of GT, AD, RO, AO, GQ (-1: absent;
// a slot is a piece index, so at most one key has it).
UZ_VC_HD UzVcfCell uz_vcf_cell(const uint8_t *p, uint32_t len, int s_gt, int s_ad, int s_ro, int s_ao, int s_gq) {
    UzVcfCell c = uz_vcf_cell_default();
    // one pass over the column: where the five pieces lie (beg > end: the column does not reach the piece)
    uint32_t gt_a = 1, gt_b = 0, ad_a = 1, ad_b = 0, ro_a = 1, ro_b = 0, ao_a = 1, ao_b = 0, gq_a = 1, gq_b = 0;
    {
        int k = 0;
        uint32_t a = 0;
        for (uint32_t i = 0; i <= len; i++) {
            if (i < len && p[i] != ':') continue;
            if (k == s_gt) { gt_a = a; gt_b = i; }
            if (k == s_ad) { ad_a = a; ad_b = i; }
            if (k == s_ro) { ro_a = a; ro_b = i; }
            if (k == s_ao) { ao_a = a; ao_b = i; }
            if (k == s_gq) { gq_a = a; gq_b = i; }
            k++;
            a = i + 1;
        }
    }
    if (gt_a <= gt_b) c.settled &= uz_vc_gt(p, gt_a, gt_b, c.gt);
    bool ad_done = false;
    if (ad_a <= ad_b && !(ad_b - ad_a == 1 && p[ad_a] == '.')) {
        uint32_t c1 = ad_a;
        while (c1 < ad_b && p[c1] != ',') c1++;
        c.settled &= uz_vc_depth(p, ad_a, c1, c.rd);
        if (c1 < ad_b) {
            uint32_t c2 = c1 + 1;
            while (c2 < ad_b && p[c2] != ',') c2++;
            c.settled &= uz_vc_depth(p, c1 + 1, c2, c.ad);
        }
        ad_done = true;
    }
    if (!ad_done && ro_a <= ro_b && ao_a <= ao_b) {
        c.settled &= uz_vc_depth(p, ro_a, ro_b, c.rd);
        uint32_t c1 = ao_a;
        while (c1 < ao_b && p[c1] != ',') c1++;
        c.settled &= uz_vc_depth(p, ao_a, c1, c.ad);
    }
    if (gq_a <= gq_b) c.settled &= uz_vc_gq(p, gq_a, gq_b, c.gq);
    return c;
}
