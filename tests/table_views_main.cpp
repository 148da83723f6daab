// table_views_main.cpp -- the rules of a site, family and sample view (unfazed_amd/csrc/table_views.hpp) on the host, built and run by
// tests/test_table_views.py under AddressSanitizer + UBSan: for every rule of the header one view just inside it and one just outside, the
// outside one held to the code and to a part of the text.  The views are laid out by hand at the sizes where a rule has an edge -- 0, 1,
// SPAN - 1, SPAN, SPAN + 1 and 2 SPAN + 1 sites, wide lists of 0, 1 and 2 entries, 1 and 2 sample rows -- and every column is a heap copy of
// exactly its size: a look past one is the sanitizer's finding.  Prints the number of cases; exit status 0: every check held.
#include "table_views.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static int n_cases = 0;
#define ACCEPTED(broken)                \
    do {                                \
        const UzBroken b__ = (broken);  \
        n_cases++;                      \
        CHECK(b__.code == 0);           \
    } while (0)
#define REFUSED(broken, want_code, part)                                                   \
    do {                                                                                   \
        const UzBroken b__ = (broken);                                                     \
        n_cases++;                                                                         \
        CHECK(b__.code == (want_code) && b__.text != nullptr && strstr(b__.text, (part))); \
    } while (0)

static const int64_t S = UZ_SITE_SPAN;
static const int64_t SIZES[] = {0, 1, S - 1, S, S + 1, 2 * S + 1};

// a column of exactly v.size() elements on the heap (never null, also when empty)
template <typename T>
struct Col {
    std::unique_ptr<T[]> p;
    Col() = default;
    explicit Col(const std::vector<T> &v) : p(new T[v.size()]) { std::copy(v.begin(), v.end(), p.get()); }
    const T *get() const { return p.get(); }
};

// ---------------------------------------------------------------------------------------------------------------- sites
struct Sites {
    int64_t n;
    std::vector<int32_t> eidx, eoff; // (eval: any)
    bool null_span = false, null_off = false, null_idx = false, null_val = false, null_d16 = false, null_b8 = false, plain_too = false;
    int64_t n_esc = -2;              // -2: eidx.size()
    Col<uint16_t> d16;
    Col<uint8_t> b8;
    Col<int32_t> span, idx, val, off, pos;
    Sites(int64_t n_, std::vector<int32_t> eidx_) : n(n_), eidx(std::move(eidx_)) { // the offsets of an ordered list
        const int64_t ns = uz_site_spans(n);
        eoff.assign((size_t)ns + 1, 0);
        for (int32_t e : eidx)
            for (int64_t s = std::min<int64_t>(e / S, ns - 1) + 1; s <= ns; s++) eoff[(size_t)s]++;
    }
    uz_sites_view view() {
        const int64_t ns = uz_site_spans(n);
        d16 = Col<uint16_t>(std::vector<uint16_t>((size_t)n, 1)); b8 = Col<uint8_t>(std::vector<uint8_t>((size_t)n, 1));
        span = Col<int32_t>(std::vector<int32_t>((size_t)ns, 100)); idx = Col<int32_t>(eidx); val = Col<int32_t>(std::vector<int32_t>(eidx.size(), 7));
        off = Col<int32_t>(eoff); pos = Col<int32_t>(std::vector<int32_t>((size_t)n, 5));
        uz_sites_view v;
        memset(&v, 0, sizeof(v));
        v.n_sites = n;
        v.pos_d16 = null_d16 ? nullptr : d16.get(); v.bases8 = null_b8 ? nullptr : b8.get(); v.span_pos = null_span ? nullptr : span.get();
        v.n_pos_esc = n_esc == -2 ? (int64_t)eidx.size() : n_esc;
        v.pos_esc_idx = null_idx ? nullptr : idx.get(); v.pos_esc_val = null_val ? nullptr : val.get(); v.pos_esc_off = null_off ? nullptr : off.get();
        if (plain_too) v.pos = pos.get();
        return v;
    }
};
static UzBroken sites_form(Sites t, UzSitesForm *form = nullptr) {
    const uz_sites_view v = t.view();
    UzSitesForm f;
    const UzBroken b = uz_sites_view_form(&v, &f);
    if (form) *form = f;
    return b;
}
static Sites with_off(Sites t, std::vector<int32_t> eoff) { t.eoff = std::move(eoff); return t; }
template <typename F>
static Sites edit(Sites t, F f) { f(t); return t; }

static void sites_views() {
    UzSitesForm form;
    {   // an empty table with every pointer null, a plain view: the plain form, nothing looked at
        uz_sites_view v;
        memset(&v, 0, sizeof(v));
        ACCEPTED(uz_sites_view_form(&v, &form)); CHECK(form == UZ_SITES_PLAIN);
        ACCEPTED(uz_sites_view_plain(&v));
        Sites p(5, {});
        p.plain_too = p.null_d16 = p.null_b8 = true;
        ACCEPTED(sites_form(std::move(p), &form)); CHECK(form == UZ_SITES_PLAIN);
        v.n_sites = -1;
        REFUSED(uz_sites_view_form(&v, &form), UZ_E_ARG, "negative");
        uz_sites_view c = Sites(5, {}).view(); // (its columns are gone: only the pointers are looked at)
        REFUSED(uz_sites_view_plain(&c), UZ_E_ARG, "compact site form");
    }
    for (int64_t n : SIZES) { // every size without escapes; with one at the first place that takes one, the last, and both
        ACCEPTED(sites_form(Sites(n, {}), &form)); CHECK(form == UZ_SITES_COMPACT);
        ACCEPTED(sites_form(edit(Sites(n, {}), [](Sites &t) { t.null_idx = t.null_val = true; }))); // no escapes: the lists may be null
        if (n < 2) continue;
        const int32_t last = (int32_t)(n - 1);
        ACCEPTED(sites_form(Sites(n, {1})));
        if (last % S) ACCEPTED(sites_form(Sites(n, {last})));
        else REFUSED(sites_form(Sites(n, {last})), UZ_E_ARG, "first site"); // (n = SPAN + 1, 2 SPAN + 1: the last site starts a span)
        if (last % S > 1) ACCEPTED(sites_form(Sites(n, {1, last})));
        REFUSED(sites_form(Sites(n, {(int32_t)n})), UZ_E_ARG, "outside its span"); // at n: beyond the (partial) last span
    }
    // an escape first, last and out of order in its span (span 1 of 2 SPAN + 1 sites: the sites SPAN .. 2 SPAN - 1)
    const int64_t n = 2 * S + 1;
    const int32_t lo = (int32_t)S, hi = (int32_t)(2 * S);
    ACCEPTED(sites_form(Sites(n, {lo + 1})));
    REFUSED(sites_form(Sites(n, {lo})), UZ_E_ARG, "first site");
    ACCEPTED(sites_form(Sites(n, {hi - 1})));
    REFUSED(sites_form(with_off(Sites(n, {hi}), {0, 0, 1, 1})), UZ_E_ARG, "outside its span"); // the next span's first site, listed in span 1
    REFUSED(sites_form(with_off(Sites(n, {lo - 1}), {0, 0, 1, 1})), UZ_E_ARG, "outside its span"); // below its span
    REFUSED(sites_form(with_off(Sites(n, {lo + 1}), {0, 1, 1, 1})), UZ_E_ARG, "outside its span"); // above its span
    ACCEPTED(sites_form(Sites(n, {lo + 1, lo + 2, hi - 1})));
    REFUSED(sites_form(Sites(n, {lo + 2, lo + 2})), UZ_E_ARG, "out of order"); // equal
    REFUSED(sites_form(with_off(Sites(n, {lo + 1, hi - 1, lo + 7}), {0, 0, 3, 3})), UZ_E_ARG, "out of order"); // descending
    ACCEPTED(sites_form(Sites(n, {1, S - 1, lo + 1})));                                                     // the order restarts with the span
    REFUSED(sites_form(Sites(n, {(int32_t)n, (int32_t)n + 100})), UZ_E_ARG, "outside its span");               // beyond n
    // pos_esc_off: from 0 to n_pos_esc, ascending
    ACCEPTED(sites_form(with_off(Sites(n, {1, lo + 1}), {0, 1, 2, 2})));
    REFUSED(sites_form(with_off(Sites(n, {1, lo + 1}), {1, 1, 2, 2})), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(with_off(Sites(n, {1, lo + 1}), {0, 1, 1, 1})), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(with_off(Sites(n, {1, lo + 1}), {0, 2, 1, 2})), UZ_E_ARG, "pos_esc_off must ascend");
    REFUSED(sites_form(with_off(Sites(n, {1, lo + 1}), {0, 3, 2, 2})), UZ_E_ARG, "pos_esc_off must ascend"); // (an offset beyond the list is never followed)
    REFUSED(sites_form(with_off(Sites(0, {}), {1})), UZ_E_ARG, "pos_esc_off");
    // the pointers of the form
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_span = true; })), UZ_E_ARG, "span_pos");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_off = true; })), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_idx = true; })), UZ_E_ARG, "escape list");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_val = true; })), UZ_E_ARG, "escape list");
    REFUSED(sites_form(edit(Sites(n, {}), [](Sites &t) { t.n_esc = -1; })), UZ_E_ARG, "escape list");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.plain_too = true; })), UZ_E_ARG, "compact sites view");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_d16 = true; })), UZ_E_ARG, "compact sites view");
    REFUSED(sites_form(edit(Sites(n, {1}), [](Sites &t) { t.null_b8 = true; })), UZ_E_ARG, "compact sites view");
    // the refusals of tests/test_site_forms_gpu.py::test_refusals, on its table: 3 SPAN + 5 sites, escapes at SPAN + 1 and 2 SPAN + 1023
    const int64_t g = 3 * S + 5;
    const int32_t a = (int32_t)(S + 1), b = (int32_t)(2 * S + 1023);
    ACCEPTED(sites_form(Sites(g, {a, b})));
    CHECK((Sites(g, {a, b}).eoff == std::vector<int32_t>{0, 0, 1, 2, 2}));
    REFUSED(sites_form(with_off(Sites(g, {a, (int32_t)(2 * S - 1)}), {0, 0, 1, 2, 2})), UZ_E_ARG, "outside its span");
    REFUSED(sites_form(with_off(Sites(g, {(int32_t)(2 * S + 5), b}), {0, 0, 1, 2, 2})), UZ_E_ARG, "outside its span");
    for (int32_t beyond : {(int32_t)g, (int32_t)g + 100}) REFUSED(sites_form(with_off(Sites(g, {a, b, beyond}), {0, 0, 1, 2, 3})), UZ_E_ARG, "outside its span");
    REFUSED(sites_form(with_off(Sites(g, {a, b, b}), {0, 0, 1, 3, 3})), UZ_E_ARG, "out of order");
    REFUSED(sites_form(with_off(Sites(g, {a, b, (int32_t)(2 * S + 7)}), {0, 0, 1, 3, 3})), UZ_E_ARG, "out of order");
    REFUSED(sites_form(with_off(Sites(g, {a, b}), {0, 2, 1, 2, 2})), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(with_off(Sites(g, {a, b}), {1, 1, 1, 2, 2})), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(with_off(Sites(g, {a, b}), {0, 0, 1, 1, 1})), UZ_E_ARG, "pos_esc_off");
    REFUSED(sites_form(edit(Sites(g, {a, b}), [](Sites &t) { t.null_span = true; })), UZ_E_ARG, "span_pos");
    REFUSED(sites_form(edit(Sites(g, {a, b}), [](Sites &t) { t.plain_too = true; })), UZ_E_ARG, "compact sites view");
    REFUSED(sites_form(with_off(Sites(g, {(int32_t)S, b}), {0, 0, 1, 2, 2})), UZ_E_ARG, "first site");
    REFUSED(sites_form(with_off(Sites(g, {a, (int32_t)(2 * S)}), {0, 0, 1, 2, 2})), UZ_E_ARG, "first site");
}

// ---------------------------------------------------------------------------------------------------------------- family
struct Family {
    int64_t n;
    int n16 = 0, n8 = 0; // how many of the nine columns are set, in 16 and in 8 bits
    bool het = false, null_hoff = false, null_h9 = false;
    int64_t n_het = 0;
    std::vector<int32_t> hoff;
    Col<uint16_t> c16;
    Col<uint8_t> c8, h9;
    Col<int32_t> off;
    explicit Family(int64_t n_) : n(n_) {}
    static Family het_form(int64_t n, int64_t n_het, std::vector<int32_t> hoff) {
        Family f(n);
        f.het = true; f.n_het = n_het; f.hoff = std::move(hoff);
        return f;
    }
    uz_family_view view() {
        c16 = Col<uint16_t>(std::vector<uint16_t>((size_t)n, 3)); c8 = Col<uint8_t>(std::vector<uint8_t>((size_t)n, 3));
        h9 = Col<uint8_t>(std::vector<uint8_t>((size_t)std::max<int64_t>(9 * n_het, 0), 3)); off = Col<int32_t>(hoff);
        uz_family_view v;
        memset(&v, 0, sizeof(v));
        const uint16_t **p16[9] = {&v.ref_depth[0], &v.ref_depth[1], &v.ref_depth[2], &v.alt_depth[0], &v.alt_depth[1], &v.alt_depth[2], &v.gq[0], &v.gq[1], &v.gq[2]};
        const uint8_t **p8[9] = {&v.ref_depth8[0], &v.ref_depth8[1], &v.ref_depth8[2], &v.alt_depth8[0], &v.alt_depth8[1], &v.alt_depth8[2], &v.gq8[0], &v.gq8[1], &v.gq8[2]};
        for (int k = 0; k < n16; k++) *p16[k] = c16.get();
        for (int k = 0; k < n8; k++) *p8[8 - k] = c8.get();
        if (het) { v.het9 = null_h9 ? nullptr : h9.get(); v.het_span_off = null_hoff ? nullptr : off.get(); v.n_het = n_het; }
        return v;
    }
};
static UzBroken family_form(Family t, bool compact_sites, UzFamilyForm *form = nullptr) {
    const uz_family_view v = t.view();
    UzFamilyForm f;
    const UzBroken b = uz_family_view_form(&v, t.n, compact_sites, &f);
    if (form) *form = f;
    return b;
}
template <typename F>
static Family edit(Family t, F f) { f(t); return t; }

static void family_views() {
    UzFamilyForm form;
    for (bool compact : {false, true}) {
        ACCEPTED(family_form(Family(0), compact, &form)); CHECK(form == UZ_FAMILY_16); // an empty table with every pointer null
        ACCEPTED(family_form(edit(Family(5), [](Family &f) { f.n16 = 9; }), compact, &form)); CHECK(form == UZ_FAMILY_16);
        ACCEPTED(family_form(edit(Family(5), [](Family &f) { f.n8 = 9; }), compact, &form)); CHECK(form == UZ_FAMILY_8);
        REFUSED(family_form(edit(Family(5), [](Family &f) { f.n16 = 8; }), compact), UZ_E_ARG, "all nine");
        REFUSED(family_form(edit(Family(5), [](Family &f) { f.n8 = 8; }), compact), UZ_E_ARG, "all nine");
        REFUSED(family_form(edit(Family(5), [](Family &f) { f.n8 = 9; f.n16 = 1; }), compact), UZ_E_ARG, "16 bits OR in 8 bits");
        REFUSED(family_form(edit(Family(5), [](Family &f) { f.n8 = 9; f.n16 = 9; }), compact), UZ_E_ARG, "16 bits OR in 8 bits");
    }
    for (int64_t n : SIZES) { // the het form at every size: no het site, and every site one
        const int64_t ns = uz_site_spans(n);
        ACCEPTED(family_form(Family::het_form(n, 0, std::vector<int32_t>((size_t)ns + 1, 0)), true, &form)); CHECK(form == UZ_FAMILY_HET);
        std::vector<int32_t> all((size_t)ns + 1);
        for (int64_t s = 0; s <= ns; s++) all[(size_t)s] = (int32_t)std::min(s * S, n);
        ACCEPTED(family_form(Family::het_form(n, n, all), true));
        all[(size_t)ns]++;
        REFUSED(family_form(Family::het_form(n, n + 1, all), true), UZ_E_ARG, "het-form family view"); // more het sites than sites
    }
    const int64_t n = 2 * S + 1;
    ACCEPTED(family_form(Family::het_form(n, 4, {0, 2, 4, 4}), true));
    ACCEPTED(family_form(Family::het_form(n, 4, {0, 3, 3, 4}), true)); // (whether a span's count is gt's: the readers hold that, no rule of the view)
    REFUSED(family_form(Family::het_form(n, 4, {1, 2, 4, 4}), true), UZ_E_ARG, "het_span_off");
    REFUSED(family_form(Family::het_form(n, 4, {0, 2, 3, 3}), true), UZ_E_ARG, "het_span_off");
    REFUSED(family_form(Family::het_form(n, 4, {0, 4, 2, 4}), true), UZ_E_ARG, "het_span_off must ascend");
    REFUSED(family_form(Family::het_form(n, -1, {0, 0, 0, -1}), true), UZ_E_ARG, "het-form family view");
    REFUSED(family_form(edit(Family::het_form(n, 4, {0, 2, 4, 4}), [](Family &f) { f.null_hoff = true; }), true), UZ_E_ARG, "het_span_off");
    REFUSED(family_form(edit(Family::het_form(n, 4, {0, 2, 4, 4}), [](Family &f) { f.null_h9 = true; }), true), UZ_E_ARG, "het9");
    ACCEPTED(family_form(edit(Family::het_form(n, 0, {0, 0, 0, 0}), [](Family &f) { f.null_h9 = true; }), true)); // no het site: het9 may be null
    // the refusals of tests/test_family_het_form_gpu.py on the offsets of 3 SPAN + 5 sites: two neighbours swapped, the last one short
    ACCEPTED(family_form(Family::het_form(3 * S + 5, 40, {0, 10, 20, 30, 40}), true));
    ACCEPTED(family_form(Family::het_form(3 * S + 5, 40, {0, 11, 20, 30, 40}), true)); // (one more in span 0: the device's count refuses it)
    REFUSED(family_form(Family::het_form(3 * S + 5, 40, {0, 20, 10, 30, 40}), true), UZ_E_ARG, "het_span_off");
    REFUSED(family_form(Family::het_form(3 * S + 5, 40, {0, 10, 20, 30, 39}), true), UZ_E_ARG, "het_span_off");
    // the cross rule: with compact sites, without the nine plain columns
    REFUSED(family_form(Family::het_form(n, 4, {0, 2, 4, 4}), false), UZ_E_ARG, "compact");
    REFUSED(family_form(Family::het_form(n, 4, {0, 2, 4, 4}), false), UZ_E_ARG, "het form");
    REFUSED(family_form(edit(Family::het_form(n, 4, {0, 2, 4, 4}), [](Family &f) { f.n8 = 9; }), true), UZ_E_ARG, "without the nine plain columns");
    REFUSED(family_form(edit(Family::het_form(n, 4, {0, 2, 4, 4}), [](Family &f) { f.n16 = 9; }), true), UZ_E_ARG, "without the nine plain columns");
}

// ---------------------------------------------------------------------------------------------------------------- wide lists
// a list of w entries and `rows` rows a side: as a family view (rows == 3: a column each) and as a sample view (rows back to back)
struct Wide {
    std::vector<int64_t> site;
    std::vector<int32_t> rd, ad; // [rows][w]
    int rows;
    bool null_site = false;
    int null_rd = -1, null_ad = -1; // family: the member whose column is null; samples: any value >= 0 -- the whole side
    Col<int64_t> c_site;
    std::vector<Col<int32_t>> c_rd, c_ad;
    Wide(std::vector<int64_t> site_, int rows_) : site(std::move(site_)), rd(site.size() * (size_t)rows_, 0), ad(site.size() * (size_t)rows_, 0), rows(rows_) {}
    size_t w() const { return site.size(); }
    uz_family_view family() {
        CHECK(rows == 3);
        uz_family_view v;
        memset(&v, 0, sizeof(v));
        c_site = Col<int64_t>(site);
        c_rd.clear(); c_ad.clear();
        for (int m = 0; m < 3; m++) {
            c_rd.emplace_back(std::vector<int32_t>(rd.begin() + m * w(), rd.begin() + (m + 1) * w()));
            c_ad.emplace_back(std::vector<int32_t>(ad.begin() + m * w(), ad.begin() + (m + 1) * w()));
        }
        v.n_wide = (int64_t)w(); v.wide_site = null_site ? nullptr : c_site.get();
        for (int m = 0; m < 3; m++) { v.wide_ref_depth[m] = m == null_rd ? nullptr : c_rd[m].get(); v.wide_alt_depth[m] = m == null_ad ? nullptr : c_ad[m].get(); }
        return v;
    }
    uz_samples_view samples() {
        uz_samples_view v;
        memset(&v, 0, sizeof(v));
        c_site = Col<int64_t>(site);
        c_rd.clear(); c_ad.clear();
        c_rd.emplace_back(rd); c_ad.emplace_back(ad);
        v.n_samples = rows; v.n_wide = (int64_t)w(); v.wide_site = null_site ? nullptr : c_site.get();
        v.wide_ref_depth = null_rd >= 0 ? nullptr : c_rd[0].get(); v.wide_alt_depth = null_ad >= 0 ? nullptr : c_ad[0].get();
        return v;
    }
};
// the verdict of every shape the list has: the family's (rows == 3), the sample table's at upload and at settle
static void wide_accepted(Wide t, int64_t bound) {
    if (t.rows == 3) { const uz_family_view v = t.family(); ACCEPTED(uz_family_wide_check(&v, bound)); }
    const uz_samples_view v = t.samples();
    ACCEPTED(uz_samples_wide_check(&v, bound, false));
    ACCEPTED(uz_samples_wide_check(&v, bound, true));
}
static void wide_refused(Wide t, int64_t bound, int code, const char *part, const char *settled_part = nullptr) {
    if (t.rows == 3) { const uz_family_view v = t.family(); REFUSED(uz_family_wide_check(&v, bound), code, part); }
    const uz_samples_view v = t.samples();
    REFUSED(uz_samples_wide_check(&v, bound, false), code, part);
    REFUSED(uz_samples_wide_check(&v, bound, true), code, settled_part ? settled_part : part);
}
template <typename F>
static Wide edit(Wide t, F f) { f(t); return t; }

static void wide_lists() {
    const char *TABLE = "ascending site indices of the table", *SETTLED = "ascending indices of the settled sites";
    {   // no entries: nothing is looked at, every pointer null
        uz_family_view f;
        memset(&f, 0, sizeof(f));
        ACCEPTED(uz_family_wide_check(&f, 5));
        uz_samples_view m;
        memset(&m, 0, sizeof(m));
        m.n_samples = 2;
        ACCEPTED(uz_samples_wide_check(&m, 5, false));
        ACCEPTED(uz_samples_wide_check(&m, 0, true));
    }
    for (int rows : {1, 2, 3}) { // (1 and 2: sample rows; 3: also the members of a family)
        const int64_t n = 5;
        // wide_site: inside [0, bound), ascending
        wide_accepted(Wide({0}, rows), n);
        wide_accepted(Wide({n - 1}, rows), n);
        wide_accepted(Wide({0, n - 1}, rows), n);
        wide_accepted(Wide({0}, rows), 1);
        wide_refused(Wide({-1}, rows), n, UZ_E_ARG, TABLE, SETTLED);
        wide_refused(Wide({n}, rows), n, UZ_E_ARG, TABLE, SETTLED);
        wide_refused(Wide({0}, rows), 0, UZ_E_ARG, TABLE, SETTLED);
        wide_refused(Wide({3, n}, rows), n, UZ_E_ARG, TABLE, SETTLED);
        wide_refused(Wide({3, 3}, rows), n, UZ_E_ARG, TABLE, SETTLED); // equal
        wide_refused(Wide({3, 1}, rows), n, UZ_E_ARG, TABLE, SETTLED); // descending
        wide_refused(edit(Wide({0}, rows), [](Wide &t) { t.null_site = true; }), n, UZ_E_ARG, "wide_site is null");
        // the depth columns: none null
        wide_refused(edit(Wide({0, 4}, rows), [&](Wide &t) { t.null_rd = rows - 1; }), n, UZ_E_ARG, "null wide depth column");
        wide_refused(edit(Wide({0, 4}, rows), [&](Wide &t) { t.null_ad = 0; }), n, UZ_E_ARG, "null wide depth column");
        // the depths: [-1, 2^30], at the last entry of the last row and at the first of the first
        for (size_t w : {(size_t)1, (size_t)2}) {
            const std::vector<int64_t> site = w == 1 ? std::vector<int64_t>{2} : std::vector<int64_t>{2, 4};
            const size_t last = (size_t)rows * w - 1;
            wide_accepted(edit(Wide(site, rows), [&](Wide &t) { t.rd[last] = -1; t.ad[0] = 1 << 30; }), n);
            wide_accepted(edit(Wide(site, rows), [&](Wide &t) { t.ad[last] = -1; t.rd[0] = 1 << 30; }), n);
            wide_refused(edit(Wide(site, rows), [&](Wide &t) { t.rd[last] = -2; }), n, UZ_E_RANGE, "wide depth outside");
            wide_refused(edit(Wide(site, rows), [&](Wide &t) { t.ad[0] = -2; }), n, UZ_E_RANGE, "wide depth outside");
            wide_refused(edit(Wide(site, rows), [&](Wide &t) { t.rd[0] = (1 << 30) + 1; }), n, UZ_E_RANGE, "wide depth outside");
            wide_refused(edit(Wide(site, rows), [&](Wide &t) { t.ad[last] = (1 << 30) + 1; }), n, UZ_E_RANGE, "wide depth outside");
        }
    }
}

static void strides() { // the smallest multiple of 256 that leaves 64 elements behind a row
    const size_t at[][2] = {{0, 256}, {1, 256}, {192, 256}, {193, 512}, {(size_t)S - 1, 1280}, {(size_t)S, 1280}, {(size_t)S + 1, 1280}, {2 * (size_t)S + 1, 2304}};
    for (const auto &p : at) {
        n_cases++;
        CHECK(uz_sample_row_stride(p[0]) == p[1] && p[1] % 256 == 0 && p[1] >= p[0] + 64 && p[1] - 256 < p[0] + 64);
    }
    for (int64_t n : SIZES) { n_cases++; CHECK(uz_site_spans(n) == (n + S - 1) / S); }
    CHECK(uz_site_spans(S) == 1 && uz_site_spans(S + 1) == 2 && uz_site_spans(0) == 0);
}

int main() {
    sites_views();
    family_views();
    wide_lists();
    strides();
    printf("table_views ok: %d cases\n", n_cases);
    return 0;
}
