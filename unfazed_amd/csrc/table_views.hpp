// table_views.hpp -- the site, family and sample tables on their way to the device: the ONE statement of which link form a view comes in and what
// its columns must hold (uz_types.h states the forms), of the rules of a wide-depth list and of a sample table's row stride.  Both readers of a
// link form go by it: the device library (tables.hip) throws a broken rule as its error, the host twins (io_vcf.cpp: uz_sites_unpack,
// uz_family_unpack_het) fail with the same text.  No HIP in here -- tests/table_views_main.cpp builds it with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "unfazed_hip.h"
#include "uz_types.h"

// the rule a view breaks: a code of unfazed_hip.h and what to say; code 0: none
struct UzBroken { int code = 0; const char *text = nullptr; };
#define UZ_VIEW_RULE(cond, code, text)               \
    do {                                             \
        if (!(cond)) return UzBroken{code, text};    \
    } while (0)

inline int64_t uz_site_spans(int64_t n_sites) { return (n_sites + UZ_SITE_SPAN - 1) / UZ_SITE_SPAN; }

// Which form the site columns of a view come in.  The escape list of the compact form (uz_sites_view.pos_d16 ...) is checked here, on the host:
// the expansion kernel and uz_sites_unpack place every escape in its span by it, and take span_pos at a span's first site -- no escape may name it.
enum UzSitesForm { UZ_SITES_PLAIN = 0, UZ_SITES_COMPACT = 1 };
inline UzBroken uz_sites_view_form(const uz_sites_view *v, UzSitesForm *form) {
    *form = UZ_SITES_PLAIN;
    UZ_VIEW_RULE(v->n_sites >= 0, UZ_E_ARG, "a sites view with a negative number of sites");
    if (!v->pos_d16 && !v->bases8) return {};
    const int64_t n = v->n_sites, n_spans = uz_site_spans(n);
    UZ_VIEW_RULE(v->pos_d16 && v->bases8 && !v->pos && !v->sflags && !v->ref_base && !v->alt_base, UZ_E_ARG,
                 "a compact sites view sets pos_d16 and bases8 and leaves pos / sflags / ref_base / alt_base null");
    UZ_VIEW_RULE(v->span_pos && v->pos_esc_off && v->n_pos_esc >= 0 && (v->n_pos_esc == 0 || (v->pos_esc_idx && v->pos_esc_val)), UZ_E_ARG,
                 "a compact sites view needs span_pos, pos_esc_off and its escape list");
    UZ_VIEW_RULE(v->pos_esc_off[0] == 0 && v->pos_esc_off[n_spans] == v->n_pos_esc, UZ_E_ARG, "pos_esc_off does not cover the escape list");
    for (int64_t sp = 0; sp < n_spans; sp++) UZ_VIEW_RULE(v->pos_esc_off[sp] <= v->pos_esc_off[sp + 1], UZ_E_ARG, "pos_esc_off must ascend");
    for (int64_t sp = 0; sp < n_spans; sp++) {
        const int64_t a = v->pos_esc_off[sp], b = v->pos_esc_off[sp + 1];
        for (int64_t e = a; e < b; e++)
            UZ_VIEW_RULE(v->pos_esc_idx[e] > sp * UZ_SITE_SPAN && v->pos_esc_idx[e] < std::min(n, (sp + 1) * UZ_SITE_SPAN) &&
                             (e == a || v->pos_esc_idx[e] > v->pos_esc_idx[e - 1]), UZ_E_ARG,
                         "an escape outside its span, at its span's first site, or out of order");
    }
    *form = UZ_SITES_COMPACT;
    return {};
}

// what takes the plain columns only (uz_sites_upload, uz_sites_adopt_device)
inline UzBroken uz_sites_view_plain(const uz_sites_view *v) {
    UZ_VIEW_RULE(!v->pos_d16 && !v->bases8, UZ_E_ARG, "the compact site form is taken by uz_sites_family_upload_async only");
    return {};
}

// Which form the nine columns of a family view come in: 16 bits (or none at all: a table without sites may leave every pointer null), eight bits
// (all nine of ref_depth8 / alt_depth8 / gq8) or the het form (uz_family_view.het9 ...: nine bytes per kid-het site).  Of the het form the offsets
// are checked here -- that they ascend from 0 to n_het; the expansion kernel and uz_family_unpack_het hold every span's count against them (no
// pass over gt here).  compact_sites: the form the sites of the table travel in.
enum UzFamilyForm { UZ_FAMILY_16 = 0, UZ_FAMILY_8 = 1, UZ_FAMILY_HET = 2 };
inline UzBroken uz_family_view_form(const uz_family_view *v, int64_t n_sites, bool compact_sites, UzFamilyForm *form) {
    *form = UZ_FAMILY_16;
    int n8 = 0, n16 = 0;
    for (int m = 0; m < 3; m++) {
        n8 += (v->ref_depth8[m] != nullptr) + (v->alt_depth8[m] != nullptr) + (v->gq8[m] != nullptr);
        n16 += (v->ref_depth[m] != nullptr) + (v->alt_depth[m] != nullptr) + (v->gq[m] != nullptr);
    }
    UZ_VIEW_RULE((n8 == 9 && n16 == 0) || (n8 == 0 && (n16 == 9 || n16 == 0)), UZ_E_ARG,
                 "a family view carries its nine columns in 16 bits OR in 8 bits (ref_depth8 / alt_depth8 / gq8), all nine");
    if (n8) *form = UZ_FAMILY_8;
    if (!v->het9 && !v->het_span_off) return {};
    const int64_t n_spans = uz_site_spans(n_sites);
    UZ_VIEW_RULE(n_sites >= 0 && v->het_span_off && v->n_het >= 0 && v->n_het <= n_sites && (v->n_het == 0 || v->het9), UZ_E_ARG,
                 "a het-form family view sets het_span_off, n_het and -- for any het site -- het9");
    UZ_VIEW_RULE(v->het_span_off[0] == 0 && v->het_span_off[n_spans] == v->n_het, UZ_E_ARG, "het_span_off does not cover het9");
    for (int64_t sp = 0; sp < n_spans; sp++) UZ_VIEW_RULE(v->het_span_off[sp] <= v->het_span_off[sp + 1], UZ_E_ARG, "het_span_off must ascend");
    UZ_VIEW_RULE(compact_sites && n8 == 0 && n16 == 0, UZ_E_ARG,
                 "the het form of a family travels with the compact site form and without the nine plain columns");
    *form = UZ_FAMILY_HET;
    return {};
}

// The sites whose depths the 16-bit columns cannot hold: wide_site ascending and below `bound` -- the sites of the table or, of_settled, the
// sites a uz_samples_settle brings --, and n_rows rows of 32-bit depths per side, none null, every depth in [-1, 2^30].  ref(r) / alt(r): row r
// (the three members of a family view, the samples of a sample view).
template <typename RefRow, typename AltRow>
inline UzBroken uz_wide_list_check(int64_t n_wide, const int64_t *wide_site, int64_t bound, bool of_settled, int64_t n_rows, RefRow ref, AltRow alt) {
    if (n_wide <= 0) return {};
    UZ_VIEW_RULE(wide_site != nullptr, UZ_E_ARG, "n_wide set but wide_site is null");
    for (int64_t k = 0; k < n_wide; k++)
        UZ_VIEW_RULE(wide_site[k] >= 0 && wide_site[k] < bound && (k == 0 || wide_site[k] > wide_site[k - 1]), UZ_E_ARG,
                     of_settled ? "wide_site must be ascending indices of the settled sites" : "wide_site must be ascending site indices of the table");
    for (int64_t r = 0; r < n_rows; r++) {
        const int32_t *rd = ref(r), *ad = alt(r);
        UZ_VIEW_RULE(rd && ad, UZ_E_ARG, "null wide depth column");
        for (int64_t k = 0; k < n_wide; k++)
            UZ_VIEW_RULE(rd[k] >= -1 && ad[k] >= -1 && rd[k] <= (1 << 30) && ad[k] <= (1 << 30), UZ_E_RANGE, "wide depth outside [-1, 2^30]");
    }
    return {};
}
// ... of a family view (three rows a side, each its own column) and of a sample view (n_samples rows a side, back to back)
inline UzBroken uz_family_wide_check(const uz_family_view *v, int64_t n_sites) {
    return uz_wide_list_check(v->n_wide, v->wide_site, n_sites, false, 3, [&](int64_t m) { return v->wide_ref_depth[m]; },
                              [&](int64_t m) { return v->wide_alt_depth[m]; });
}
inline UzBroken uz_samples_wide_check(const uz_samples_view *v, int64_t bound, bool of_settled) {
    const int64_t w = v->n_wide;
    return uz_wide_list_check(w, v->wide_site, bound, of_settled, v->n_samples, [&](int64_t r) { return v->wide_ref_depth ? v->wide_ref_depth + r * w : nullptr; },
                              [&](int64_t r) { return v->wide_alt_depth ? v->wide_alt_depth + r * w : nullptr; });
}

// elements between two rows of a sample table (of gt and of the 16-bit columns alike): every row 256-byte aligned, vector tail reads stay in-bounds
inline size_t uz_sample_row_stride(size_t n_sites) { return (n_sites + 64 + 255) & ~(size_t)255; }
