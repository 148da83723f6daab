// tables.hip -- the site, family and sample tables of include/unfazed_hip.h: their look-ups and frees, the uploads of every link form, the
// tables adopted in place, the cohort's sample table and the trios made from it, the fetches.  table_views.hpp states the rules of a view; no
// kernel in here (the expansions, the fold and the parsers are k_sites.hip, k_vcf.hip and k_bcf.hip).
#include "uz_stage.hpp"
#include "table_views.hpp"

#include <algorithm>

void uz_fold_complex(uz_ctx *c, uint8_t *gt, const uint8_t *sflags, int64_t n);

// ---------------------------------------------------------------- look-ups and frees (uz_stage.hpp)
SitesDev &sites_of(uz_ctx *c, int id) {
    UZ_REQUIRE(id >= 0 && id < (int)c->sites.size() && c->sites[id].live, UZ_E_ARG, "unknown sites handle");
    SitesDev &s = c->sites[id];
    if (s.pending) { // queued by uz_sites_family_upload_async
        s.pending = false;
        UZ_HIP(hipStreamWaitEvent(c->stream, s.ready, 0));
    }
    uz_sites_expand(c, s, nullptr); // (compact form used before its family: the sites alone)
    return s;
}
FamilyDev &fam_of(uz_ctx *c, int id) {
    UZ_REQUIRE(id >= 0 && id < (int)c->fams.size() && c->fams[id].live, UZ_E_ARG, "unknown family handle");
    FamilyDev &f = c->fams[id];
    if (f.pending) { // queued by uz_sites_family_upload_async: the compute stream waits for the copies, then folds the complex flag
        f.pending = false;
        UZ_HIP(hipStreamWaitEvent(c->stream, f.ready, 0));
        SitesDev &s0 = c->sites[f.sites_id];
        if (f.het_only && s0.n) s0.expand_pending = true; // (sites used before their family: expanded again, now with the het columns)
        if (s0.expand_pending) { // compact site form: ONE launch expands the sites and readies the family
            if (s0.pending) { s0.pending = false; UZ_HIP(hipStreamWaitEvent(c->stream, s0.ready, 0)); }
            uz_sites_expand(c, s0, &f);
        } else {
            SitesDev &s = sites_of(c, f.sites_id);
            uz_family_widen(c, f, s.n);
            uz_fold_complex(c, f.gt, s.sflags, s.n);
        }
    }
    return f;
}
SamplesDev &samples_of(uz_ctx *c, int id) {
    UZ_REQUIRE(id >= 0 && id < (int)c->samples.size() && c->samples[id].live, UZ_E_ARG, "unknown sample table handle");
    return c->samples[id];
}

void free_family(uz_ctx *c, FamilyDev &f) {
    if (f.ready) { (void)hipEventSynchronize(f.ready); (void)hipEventDestroy(f.ready); f.ready = nullptr; }
    f.pending = false;
    if (f.samples_id >= 0 && f.samples_id < (int)c->samples.size()) c->samples[(size_t)f.samples_id].live_fams--; // (its gt / cls / wide depths lie in a block of the table's)
    uz_block_put(c, f.block);
    uz_block_put(c, f.wide_block);
    f = FamilyDev();
}
void free_samples(uz_ctx *c, SamplesDev &m) {
    if (m.ready) { (void)hipEventSynchronize(m.ready); (void)hipEventDestroy(m.ready); }
    uz_block_put(c, m.block);
    uz_block_put(c, m.wide_block);
    for (DevBlock &b : m.fam_blocks) uz_block_put(c, b);
    m = SamplesDev();
}
void free_sites(uz_ctx *c, SitesDev &s) {
    if (s.ready) { (void)hipEventSynchronize(s.ready); (void)hipEventDestroy(s.ready); }
    uz_block_put(c, s.block);
    uz_block_put(c, s.mirror);
    s = SitesDev();
}

void refuse_het_only(const FamilyDev &f, const char *what) {
    if (f.het_only) throw UzError{UZ_E_STATE, std::string(what) + ": this family was staged in the het form (genotype columns of the kid-het sites only)"};
}

namespace {

void require(const UzBroken &b) { // a rule of table_views.hpp as this library's error
    if (b.code) throw UzError{b.code, b.text};
}

// A table while it is built: what fails in `build` releases it as a finished table is released -- blocks, mirror, events (free_sites ...)
template <typename T, typename R, typename F>
void built_or_freed(uz_ctx *c, T &table, R &&release, F &&build) {
    try {
        build();
    } catch (...) {
        release(c, table);
        throw;
    }
}

// a host column into its place in the table's block -- or, under a slab plan, wherever in the mirror block it landed (uz_stage.hpp: h2d)
template <typename T>
void stage(hipStream_t st, T *&col, const T *host, size_t n) { col = const_cast<T *>(h2d(st, col, host, n)); }
template <typename T>
void stage(hipStream_t st, const T *&col, const T *host, size_t n) { col = h2d(st, const_cast<T *>(col), host, n); }

// ---- the layouts: one statement each.  The staged columns of a link form lie behind the table's own (the staged bytes may end up in the
// mirror block: the plain columns, which the expansion writes, are always the table's own)
// sites: [contig offsets | pos | sflags | ref_base | alt_base | compact form: pos_d16, bases8, span_pos, escape indices, values, offsets]; a table
// adopted in place owns the offsets alone
void carve_sites(Carver &cv, SitesDev &s, bool columns, UzSitesForm form, size_t n_esc) {
    const size_t n = (size_t)s.n, n_spans = (size_t)uz_site_spans(s.n);
    s.contig_off = cv.take<int64_t>((size_t)s.n_contigs + 1);
    if (!columns) return;
    s.pos = cv.take<int32_t>(n); s.sflags = cv.take<uint8_t>(n); s.ref_base = cv.take<uint8_t>(n); s.alt_base = cv.take<uint8_t>(n);
    if (form == UZ_SITES_COMPACT) {
        s.c_d16 = cv.take<uint16_t>(n); s.c_b8 = cv.take<uint8_t>(n); s.c_span = cv.take<int32_t>(n_spans);
        s.c_eidx = cv.take<int32_t>(n_esc); s.c_eval = cv.take<int32_t>(n_esc); s.c_eoff = cv.take<int32_t>(n_spans + 1);
    }
}
// family: [cls | gt | rd, ad, gq of kid, dad, mom | eight-bit form: the nine staged columns | het form: het9, het_span_off]; a family adopted in
// place owns the class column alone
void carve_family(Carver &cv, FamilyDev &f, size_t n, bool columns, UzFamilyForm form, size_t n_het) {
    f.cls = cv.take<uint8_t>(n);
    if (!columns) return;
    f.gt = cv.take<uint8_t>(n);
    for (int m = 0; m < 3; m++) { f.rd[m] = cv.take<uint16_t>(n); f.ad[m] = cv.take<uint16_t>(n); f.gq[m] = cv.take<uint16_t>(n); }
    if (form == UZ_FAMILY_8) for (int k = 0; k < 9; k++) f.stage8[k] = cv.take<uint8_t>(n);
    if (form == UZ_FAMILY_HET) { f.het9 = cv.take<uint8_t>(9 * n_het); f.het_off = cv.take<int32_t>((size_t)uz_site_spans((int64_t)n) + 1); }
}
// sample rows: [gt | rd | ad | gq], n_samples rows each at the table's stride
void carve_sample_rows(Carver &cv, SamplesDev &m, size_t n_sites) {
    const size_t ns = (size_t)m.n_samples;
    m.stride = uz_sample_row_stride(n_sites);
    m.gt = cv.take<uint8_t>(ns * m.stride);
    m.rd = cv.take<uint16_t>(ns * m.stride); m.ad = cv.take<uint16_t>(ns * m.stride); m.gq = cv.take<uint16_t>(ns * m.stride);
}

// ---- the staging: the columns of a view queued on `st`, with or without an active slab plan (then called once per pass of the plan)
void stage_sites(hipStream_t st, SitesDev &s, const uz_sites_view *v, UzSitesForm form) {
    const size_t n = (size_t)s.n, n_spans = (size_t)uz_site_spans(s.n), n_esc = form == UZ_SITES_COMPACT ? (size_t)v->n_pos_esc : 0;
    stage(st, s.contig_off, v->contig_off, (size_t)v->n_contigs + 1);
    if (form == UZ_SITES_COMPACT) {
        stage(st, s.c_d16, v->pos_d16, n); stage(st, s.c_b8, v->bases8, n); stage(st, s.c_span, v->span_pos, n_spans);
        stage(st, s.c_eidx, v->pos_esc_idx, n_esc); stage(st, s.c_eval, v->pos_esc_val, n_esc); stage(st, s.c_eoff, v->pos_esc_off, n_spans + 1);
    } else {
        stage(st, s.pos, v->pos, n); stage(st, s.sflags, v->sflags, n); stage(st, s.ref_base, v->ref_base, n); stage(st, s.alt_base, v->alt_base, n);
    }
    s.expand_pending = form == UZ_SITES_COMPACT && n;
}
void stage_family(hipStream_t st, FamilyDev &f, const uz_family_view *v, UzFamilyForm form, size_t n) {
    const size_t n_het = form == UZ_FAMILY_HET ? (size_t)v->n_het : 0;
    stage(st, f.gt, v->gt, n); // (bit 6 is written by the library: a mirror block is the library's own memory)
    if (form == UZ_FAMILY_8) {
        for (int m = 0; m < 3; m++) {
            stage(st, f.stage8[m], v->ref_depth8[m], n); stage(st, f.stage8[3 + m], v->alt_depth8[m], n); stage(st, f.stage8[6 + m], v->gq8[m], n);
        }
        f.widen_pending = true; f.gq_clamped = true;
    } else if (form == UZ_FAMILY_HET) { // (the expansion writes the family's own 16-bit columns from them)
        stage(st, f.het9, v->het9, 9 * n_het); stage(st, f.het_off, v->het_span_off, (size_t)uz_site_spans((int64_t)n) + 1);
        f.het_only = true; f.n_het = (int64_t)n_het; f.gq_clamped = true;
    } else
        for (int m = 0; m < 3; m++) { stage(st, f.rd[m], v->ref_depth[m], n); stage(st, f.ad[m], v->alt_depth[m], n); stage(st, f.gq[m], v->gq[m], n); }
}

// the too-deep sites of a family view (host pointers) -> the family's side table on the device
void family_wide(uz_ctx *c, hipStream_t st, const uz_family_view *v, FamilyDev &f, int64_t n_sites) {
    f.n_wide = 0;
    if (v->n_wide <= 0) return;
    require(uz_family_wide_check(v, n_sites));
    const size_t w = (size_t)v->n_wide;
    f.wide_host = std::make_shared<std::vector<int32_t>>(6 * w);
    std::vector<int32_t> &dep = *f.wide_host;
    for (int m = 0; m < 3; m++) {
        std::copy(v->wide_ref_depth[m], v->wide_ref_depth[m] + w, dep.begin() + (size_t)m * w);
        std::copy(v->wide_alt_depth[m], v->wide_alt_depth[m] + w, dep.begin() + (size_t)(3 + m) * w);
    }
    f.wide_block = uz_carve(c, [&](Carver &cv) { f.wide_site = cv.take<int64_t>(w); f.wide_depth = cv.take<int32_t>(6 * w); });
    UZ_HIP(hipMemcpyAsync(f.wide_site, v->wide_site, w * sizeof(int64_t), hipMemcpyHostToDevice, st));
    UZ_HIP(hipMemcpyAsync(f.wide_depth, dep.data(), 6 * w * sizeof(int32_t), hipMemcpyHostToDevice, st)); // (`dep` lives as long as the family)
    f.n_wide = (int64_t)w;
}

// a synchronous upload or adoption ends here: the complex flag folded into gt, the table ready when the call returns
void family_common(uz_ctx *c, int sites_id, FamilyDev &f) {
    SitesDev &s = sites_of(c, sites_id);
    f.live = true;
    f.sites_id = sites_id;
    uz_fold_complex(c, f.gt, s.sflags, s.n);
    UZ_HIP(hipStreamSynchronize(c->stream));
}

void sites_head(SitesDev &s, const uz_sites_view *v, bool owned) {
    s.live = true; s.owned = owned;
    s.n = v->n_sites; s.n_contigs = v->n_contigs;
}

// the table of uz_samples_from_text / uz_samples_from_bcf: rows carved as uz_samples_upload carves them, filled by parse(m, chunk bytes)
template <typename F>
void samples_from_records(uz_ctx *c, int sites_id, int64_t n_sites, int32_t n_pick, int *id, int64_t *n_unsettled, F parse) {
    size_t chunk = (size_t)32 << 20;
    if (const char *e = getenv("UZ_VCF_CHUNK_BYTES")) { // (read per call: a test hook for the multi-chunk path)
        const long long v = atoll(e);
        if (v > 0) chunk = (size_t)v;
    }
    chunk = std::min<size_t>(chunk, (size_t)1 << 31);
    SamplesDev m;
    m.live = true; m.sites_id = sites_id; m.n_samples = n_pick; m.n_wide = 0;
    m.block = uz_carve(c, [&](Carver &cv) { carve_sample_rows(cv, m, (size_t)n_sites); });
    built_or_freed(c, m, free_samples, [&] { parse(m, chunk); });
    m.need_settle = !m.unsettled.empty();
    *n_unsettled = (int64_t)m.unsettled.size();
    const int k = new_slot(c->samples);
    c->samples[(size_t)k] = m;
    *id = k;
}

} // namespace

extern "C" {

int uz_sites_upload(uz_ctx *c, const uz_sites_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id && v->n_sites >= 0 && v->n_contigs >= 0, UZ_E_ARG, "bad sites view");
        require(uz_sites_view_plain(v));
        UZ_REQUIRE(v->n_sites < (int64_t)0x7FFFFFF0, UZ_E_RANGE, "more than 2^31 sites");
        const int k = new_slot(c->sites);
        SitesDev s;
        sites_head(s, v, true);
        s.contig_off_h.assign(v->contig_off, v->contig_off + v->n_contigs + 1);
        s.block = uz_carve(c, [&](Carver &cv) { carve_sites(cv, s, true, UZ_SITES_PLAIN, 0); });
        built_or_freed(c, s, free_sites, [&] {
            stage_sites(c->stream, s, v, UZ_SITES_PLAIN);
            UZ_HIP(hipStreamSynchronize(c->stream));
        });
        c->sites[k] = s;
        *id = k;
    });
}

int uz_sites_adopt_device(uz_ctx *c, const uz_sites_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id && v->n_sites >= 0 && v->n_contigs >= 0, UZ_E_ARG, "bad sites view");
        require(uz_sites_view_plain(v));
        const int k = new_slot(c->sites);
        SitesDev s;
        sites_head(s, v, false);
        s.contig_off_h.resize((size_t)v->n_contigs + 1);
        UZ_HIP(hipMemcpy(s.contig_off_h.data(), v->contig_off, ((size_t)v->n_contigs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        s.block = uz_carve(c, [&](Carver &cv) { carve_sites(cv, s, false, UZ_SITES_PLAIN, 0); });
        built_or_freed(c, s, free_sites, [&] {
            h2d(c->stream, s.contig_off, (const int64_t *)s.contig_off_h.data(), (size_t)v->n_contigs + 1);
            s.pos = const_cast<int32_t *>(v->pos);
            s.sflags = const_cast<uint8_t *>(v->sflags);
            s.ref_base = const_cast<uint8_t *>(v->ref_base);
            s.alt_base = const_cast<uint8_t *>(v->alt_base);
            UZ_HIP(hipStreamSynchronize(c->stream));
        });
        c->sites[k] = s;
        *id = k;
    });
}

int uz_family_upload(uz_ctx *c, int sites_id, const uz_family_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id, UZ_E_ARG, "bad family view");
        SitesDev &s = sites_of(c, sites_id);
        FamilyDev f;
        f.owned = true;
        const size_t n = (size_t)s.n;
        UzFamilyForm form;
        require(uz_family_view_form(v, s.n, false, &form)); // (the het form: with its sites, through uz_sites_family_upload_async)
        f.block = uz_carve(c, [&](Carver &cv) { carve_family(cv, f, n, true, form, 0); });
        built_or_freed(c, f, free_family, [&] {
            stage_family(c->stream, f, v, form, n);
            uz_family_widen(c, f, s.n);
            family_wide(c, c->stream, v, f, s.n);
            family_common(c, sites_id, f);
        });
        const int k = new_slot(c->fams);
        c->fams[k] = f;
        *id = k;
    });
}

int uz_sites_family_upload_async(uz_ctx *c, const uz_sites_view *v, const uz_family_view *fv, int *sites_id, int *fam_id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && fv && sites_id && fam_id && v->n_sites >= 0 && v->n_contigs >= 0, UZ_E_ARG, "bad sites / family view");
        UZ_REQUIRE(v->n_sites < (int64_t)0x7FFFFFF0, UZ_E_RANGE, "more than 2^31 sites");
        SitesDev s;
        sites_head(s, v, true);
        s.contig_off_h.assign(v->contig_off, v->contig_off + v->n_contigs + 1);
        const size_t n = (size_t)s.n;
        FamilyDev f;
        f.owned = true;
        UzSitesForm sform;
        UzFamilyForm form;
        require(uz_sites_view_form(v, &sform));
        require(uz_family_view_form(fv, s.n, sform == UZ_SITES_COMPACT, &form));
        s.block = uz_carve(c, [&](Carver &cv) { carve_sites(cv, s, true, sform, sform == UZ_SITES_COMPACT ? (size_t)v->n_pos_esc : 0); });
        built_or_freed(c, s, free_sites, [&] {
            f.block = uz_carve(c, [&](Carver &cv) { carve_family(cv, f, n, true, form, form == UZ_FAMILY_HET ? (size_t)fv->n_het : 0); });
            built_or_freed(c, f, free_family, [&] {
                hipStream_t st = c->copy_stream;
                SlabPlan plan;
                SlabScope slab_scope(&plan);
                for (bool planned : {false, true}) { // (uz_stage.hpp: the planning pass, then the pass that yields the device pointers)
                    if (planned) slab_commit(c, st, plan, s.mirror);
                    stage_sites(st, s, v, sform);
                    stage_family(st, f, fv, form, n);
                }
                family_wide(c, st, fv, f, s.n);
                UZ_HIP(hipEventCreateWithFlags(&f.ready, hipEventDisableTiming));
                UZ_HIP(hipEventRecord(f.ready, st));
                UZ_HIP(hipEventCreateWithFlags(&s.ready, hipEventDisableTiming));
                UZ_HIP(hipEventRecord(s.ready, st));
                s.pending = true;
            });
        });
        const int ks = new_slot(c->sites);
        c->sites[ks] = s;
        f.live = true; f.sites_id = ks; f.pending = true;
        const int kf = new_slot(c->fams);
        c->fams[kf] = f;
        *sites_id = ks; *fam_id = kf;
    });
}

int uz_family_adopt_device(uz_ctx *c, int sites_id, const uz_family_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id, UZ_E_ARG, "bad family view");
        const int64_t n_sites = sites_of(c, sites_id).n;
        UzFamilyForm form;
        require(uz_family_view_form(v, n_sites, false, &form));
        UZ_REQUIRE(form == UZ_FAMILY_16, UZ_E_ARG, "uz_family_adopt_device takes the 16-bit columns (the kernels read them in place)");
        FamilyDev f;
        f.owned = false;
        f.gt = const_cast<uint8_t *>(v->gt); // bit 6 is written by the library (complex flag)
        for (int m = 0; m < 3; m++) {
            f.rd[m] = const_cast<uint16_t *>(v->ref_depth[m]);
            f.ad[m] = const_cast<uint16_t *>(v->alt_depth[m]);
            f.gq[m] = const_cast<uint16_t *>(v->gq[m]);
            UZ_REQUIRE(((uintptr_t)f.rd[m] | (uintptr_t)f.ad[m] | (uintptr_t)f.gq[m]) % 16 == 0, UZ_E_ARG,
                       "device columns must be 16-byte aligned");
        }
        UZ_REQUIRE((uintptr_t)f.gt % 16 == 0, UZ_E_ARG, "device columns must be 16-byte aligned");
        f.block = uz_carve(c, [&](Carver &cv) { carve_family(cv, f, (size_t)n_sites, false, form, 0); });
        built_or_freed(c, f, free_family, [&] {
            family_wide(c, c->stream, v, f, n_sites);
            family_common(c, sites_id, f);
        });
        const int k = new_slot(c->fams);
        c->fams[k] = f;
        *id = k;
    });
}

// ---- the cohort form: a sample table, and trios made from it (unfazed_hip.h) ----------------------------------------------------------
int uz_samples_upload(uz_ctx *c, int sites_id, const uz_samples_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id && v->n_samples >= 0 && v->n_wide >= 0, UZ_E_ARG, "bad samples view");
        SitesDev &s = sites_of(c, sites_id);
        const size_t n = (size_t)s.n, ns = (size_t)v->n_samples, w = (size_t)v->n_wide;
        UZ_REQUIRE(!(n && ns) || (v->gt && v->ref_depth && v->alt_depth && v->gq), UZ_E_ARG, "null column pointer");
        require(uz_samples_wide_check(v, s.n, false));
        SamplesDev m;
        m.live = true; m.sites_id = sites_id; m.n_samples = v->n_samples; m.n_wide = v->n_wide;
        m.block = uz_carve(c, [&](Carver &cv) {
            carve_sample_rows(cv, m, n);
            m.wide_site = cv.take<int64_t>(w); m.wide_rd = cv.take<int32_t>(ns * w); m.wide_ad = cv.take<int32_t>(ns * w);
        });
        auto release = [](uz_ctx *cx, SamplesDev &t) { (void)hipStreamSynchronize(cx->copy_stream); free_samples(cx, t); }; // (copies may be queued, no event behind them yet)
        built_or_freed(c, m, release, [&] {
            hipStream_t st = c->copy_stream;
            if (n && ns) { // one strided copy per column: the host rows lie back to back, the device rows at the aligned stride
                UZ_HIP(hipMemcpy2DAsync(m.gt, m.stride, v->gt, n, n, ns, hipMemcpyHostToDevice, st));
                UZ_HIP(hipMemcpy2DAsync(m.rd, m.stride * 2, v->ref_depth, n * 2, n * 2, ns, hipMemcpyHostToDevice, st));
                UZ_HIP(hipMemcpy2DAsync(m.ad, m.stride * 2, v->alt_depth, n * 2, n * 2, ns, hipMemcpyHostToDevice, st));
                UZ_HIP(hipMemcpy2DAsync(m.gq, m.stride * 2, v->gq, n * 2, n * 2, ns, hipMemcpyHostToDevice, st));
            }
            if (w) {
                UZ_HIP(hipMemcpyAsync(m.wide_site, v->wide_site, w * sizeof(int64_t), hipMemcpyHostToDevice, st));
                if (ns) {
                    UZ_HIP(hipMemcpyAsync(m.wide_rd, v->wide_ref_depth, ns * w * sizeof(int32_t), hipMemcpyHostToDevice, st));
                    UZ_HIP(hipMemcpyAsync(m.wide_ad, v->wide_alt_depth, ns * w * sizeof(int32_t), hipMemcpyHostToDevice, st));
                }
            }
            UZ_HIP(hipEventCreateWithFlags(&m.ready, hipEventDisableTiming));
            UZ_HIP(hipEventRecord(m.ready, st));
            m.pending = true;
        });
        const int k = new_slot(c->samples);
        c->samples[(size_t)k] = m;
        *id = k;
    });
}

int uz_samples_from_text(uz_ctx *c, int sites_id, const uz_vcf_text_view *t, int32_t n_pick, const int32_t *pick, int *id, int64_t *n_unsettled) {
    return guarded(c, [&] {
        UZ_REQUIRE(t && id && n_unsettled && n_pick >= 0 && (n_pick == 0 || pick) && t->n_samples >= 0, UZ_E_ARG, "bad text view or pick list");
        SitesDev &s = sites_of(c, sites_id);
        UZ_REQUIRE(t->n_records == s.n, UZ_E_ARG, "the text's records are not the sites of the table");
        UZ_REQUIRE(s.n == 0 || (t->text && t->samp_at && t->line_end && t->fmt_slot && t->text_bytes >= 0), UZ_E_ARG, "null pointer in the text view");
        for (int32_t r = 0; r < n_pick; r++) UZ_REQUIRE(pick[r] >= 0 && pick[r] < t->n_samples, UZ_E_ARG, "picked sample column outside the file's");
        samples_from_records(c, sites_id, s.n, n_pick, id, n_unsettled, [&](SamplesDev &m, size_t chunk) { uz_vcf_parse_text(c, t, n_pick, pick, m, chunk, m.unsettled); });
    });
}

int uz_samples_from_bcf(uz_ctx *c, int sites_id, const uz_vcf_bcf_view *t, int32_t n_pick, const int32_t *pick, int *id, int64_t *n_unsettled) {
    return guarded(c, [&] {
        UZ_REQUIRE(t && id && n_unsettled && n_pick >= 0 && (n_pick == 0 || pick) && t->n_samples >= 0, UZ_E_ARG, "bad BCF view or pick list");
        SitesDev &s = sites_of(c, sites_id);
        UZ_REQUIRE(t->n_records == s.n, UZ_E_ARG, "the BCF's records are not the sites of the table");
        UZ_REQUIRE(s.n == 0 || (t->data && t->fld_at && t->fld_desc && t->data_bytes >= 0), UZ_E_ARG, "null pointer in the BCF view");
        for (int32_t r = 0; r < n_pick; r++) UZ_REQUIRE(pick[r] >= 0 && pick[r] < t->n_samples, UZ_E_ARG, "picked sample outside the file's");
        samples_from_records(c, sites_id, s.n, n_pick, id, n_unsettled, [&](SamplesDev &m, size_t chunk) { uz_vcf_parse_bcf(c, t, n_pick, pick, m, chunk, m.unsettled); });
    });
}

int uz_samples_unsettled(uz_ctx *c, int samples_id, int64_t *site) {
    return guarded(c, [&] {
        SamplesDev &m = samples_of(c, samples_id);
        UZ_REQUIRE(m.unsettled.empty() || site, UZ_E_ARG, "null output");
        for (size_t k = 0; k < m.unsettled.size(); k++) site[k] = m.unsettled[k];
    });
}

int uz_samples_settle(uz_ctx *c, int samples_id, int64_t n, const int64_t *site, const uz_samples_view *v) {
    return guarded(c, [&] {
        SamplesDev &m = samples_of(c, samples_id);
        UZ_REQUIRE(n >= 0 && (n == 0 || (site && v)), UZ_E_ARG, "bad settle arguments");
        UZ_REQUIRE(m.need_settle || n == 0, UZ_E_STATE, "the sample table has no unsettled sites");
        UZ_REQUIRE((size_t)n == m.unsettled.size() && std::equal(m.unsettled.begin(), m.unsettled.end(), site), UZ_E_ARG,
                   "uz_samples_settle takes exactly the sites of uz_samples_unsettled, in that order");
        if (n == 0) return;
        const size_t un = (size_t)n, ns = (size_t)m.n_samples, w = (size_t)v->n_wide;
        UZ_REQUIRE(v->n_samples == m.n_samples && v->n_wide >= 0, UZ_E_ARG, "the cells are not a sample table of the table's rows");
        UZ_REQUIRE(!ns || (v->gt && v->ref_depth && v->alt_depth && v->gq), UZ_E_ARG, "null column pointer");
        require(uz_samples_wide_check(v, n, true));
        std::vector<int64_t> wide_site(w);
        for (size_t k = 0; k < w; k++) wide_site[k] = site[v->wide_site[k]];
        DevBlock tmp, wide;
        try {
            int64_t *d_site = nullptr;
            uint8_t *d_gt = nullptr;
            uint16_t *d_rd = nullptr, *d_ad = nullptr, *d_gq = nullptr;
            tmp = uz_carve(c, [&](Carver &cv) {
                d_site = cv.take<int64_t>(un); d_gt = cv.take<uint8_t>(ns * un);
                d_rd = cv.take<uint16_t>(ns * un); d_ad = cv.take<uint16_t>(ns * un); d_gq = cv.take<uint16_t>(ns * un);
            });
            UZ_HIP(hipMemcpyAsync(d_site, site, un * 8, hipMemcpyHostToDevice, c->stream));
            if (ns) {
                UZ_HIP(hipMemcpyAsync(d_gt, v->gt, ns * un, hipMemcpyHostToDevice, c->stream));
                UZ_HIP(hipMemcpyAsync(d_rd, v->ref_depth, ns * un * 2, hipMemcpyHostToDevice, c->stream));
                UZ_HIP(hipMemcpyAsync(d_ad, v->alt_depth, ns * un * 2, hipMemcpyHostToDevice, c->stream));
                UZ_HIP(hipMemcpyAsync(d_gq, v->gq, ns * un * 2, hipMemcpyHostToDevice, c->stream));
            }
            uz_launch_vcf_settle(c, n, m.n_samples, d_site, d_gt, d_rd, d_ad, d_gq, m);
            if (w) {
                wide = uz_carve(c, [&](Carver &cv) { m.wide_site = cv.take<int64_t>(w); m.wide_rd = cv.take<int32_t>(ns * w); m.wide_ad = cv.take<int32_t>(ns * w); });
                UZ_HIP(hipMemcpyAsync(m.wide_site, wide_site.data(), w * 8, hipMemcpyHostToDevice, c->stream));
                if (ns) {
                    UZ_HIP(hipMemcpyAsync(m.wide_rd, v->wide_ref_depth, ns * w * 4, hipMemcpyHostToDevice, c->stream));
                    UZ_HIP(hipMemcpyAsync(m.wide_ad, v->wide_alt_depth, ns * w * 4, hipMemcpyHostToDevice, c->stream));
                }
            }
            UZ_HIP(hipStreamSynchronize(c->stream)); // (the host arrays are the caller's)
        } catch (...) {
            (void)hipStreamSynchronize(c->stream);
            uz_block_put(c, tmp); uz_block_put(c, wide);
            m.wide_site = nullptr; m.wide_rd = m.wide_ad = nullptr;
            throw;
        }
        uz_block_put(c, tmp);
        m.wide_block = wide;
        m.n_wide = (int64_t)w;
        m.need_settle = false;
    });
}

int uz_families_from_samples(uz_ctx *c, int samples_id, int32_t n, const int32_t *kid, const int32_t *dad, const int32_t *mom, int *fam_ids) {
    return guarded(c, [&] {
        UZ_REQUIRE(n >= 0 && (n == 0 || (kid && dad && mom && fam_ids)), UZ_E_ARG, "bad trio list");
        SamplesDev &m0 = samples_of(c, samples_id);
        UZ_REQUIRE(!m0.need_settle, UZ_E_STATE, "the sample table has unsettled sites: uz_samples_settle first");
        UZ_REQUIRE(m0.sites_id >= 0 && m0.sites_id < (int)c->sites.size() && c->sites[(size_t)m0.sites_id].live, UZ_E_ARG, "the sample table's sites table is gone");
        std::vector<int32_t> trio((size_t)n * 3);
        for (int32_t t = 0; t < n; t++) {
            const int32_t idx[3] = {kid[t], dad[t], mom[t]};
            for (int q = 0; q < 3; q++) {
                UZ_REQUIRE(idx[q] >= 0 && idx[q] < m0.n_samples, UZ_E_ARG, "sample index outside the table");
                trio[(size_t)t * 3 + q] = idx[q];
            }
        }
        if (n == 0) return;
        SitesDev &s = sites_of(c, m0.sites_id);
        if (m0.pending) { m0.pending = false; UZ_HIP(hipStreamWaitEvent(c->stream, m0.ready, 0)); }
        const size_t S = (size_t)s.n, w = (size_t)m0.n_wide;
        const size_t A = uz_sample_row_stride(S); // (a row of the table) cls and gt of trio t: t * 2A and t * 2A + A; the wide depths behind them
        const size_t wide_at = (size_t)n * 2 * A;
        DevBlock blk = uz_block_get(c, wide_at + (size_t)n * 6 * w * sizeof(int32_t) + 512);
        int made = 0;
        try {
            c->trio_idx.ensure(trio.size());
            UZ_HIP(hipMemcpyAsync(c->trio_idx.p, trio.data(), trio.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            int32_t *wide_out = reinterpret_cast<int32_t *>(blk.p + wide_at);
            uz_launch_family_pack(c, m0, s, n, c->trio_idx.p, blk.p + A, 2 * A, wide_out);
            UZ_HIP(hipStreamSynchronize(c->stream)); // (`trio` is pageable host memory; the families are ready when the call returns)
            for (int32_t t = 0; t < n; t++) {
                const int k = new_slot(c->fams); // (may move c->fams: no reference into it is held across)
                FamilyDev f;
                f.live = true; f.owned = true; f.sites_id = m0.sites_id; f.samples_id = samples_id;
                f.cls = blk.p + (size_t)t * 2 * A;
                f.gt = blk.p + (size_t)t * 2 * A + A;
                SamplesDev &m = c->samples[(size_t)samples_id];
                const int32_t *ix = &trio[(size_t)t * 3];
                for (int q = 0; q < 3; q++) {
                    f.rd[q] = m.rd + (size_t)ix[q] * m.stride; f.ad[q] = m.ad + (size_t)ix[q] * m.stride; f.gq[q] = m.gq + (size_t)ix[q] * m.stride;
                }
                f.n_wide = m.n_wide;
                f.wide_site = m.wide_site;
                f.wide_depth = w ? wide_out + (size_t)t * 6 * w : nullptr;
                c->fams[(size_t)k] = f;
                m.live_fams++;
                fam_ids[t] = k;
                made++;
            }
            c->samples[(size_t)samples_id].fam_blocks.push_back(blk);
        } catch (...) {
            (void)hipStreamSynchronize(c->stream);
            for (int t = 0; t < made; t++) free_family(c, c->fams[(size_t)fam_ids[t]]);
            uz_block_put(c, blk);
            throw;
        }
    });
}

int uz_family_fetch(uz_ctx *c, int fam_id, uint8_t *gt, uint16_t *cols) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        refuse_het_only(f, "uz_family_fetch");
        SitesDev &s = sites_of(c, f.sites_id);
        const size_t n = (size_t)s.n;
        if (!n) return;
        UZ_REQUIRE(gt != nullptr && cols != nullptr, UZ_E_ARG, "null output");
        uz_family_widen(c, f, s.n);
        UZ_HIP(hipStreamSynchronize(c->stream));
        UZ_HIP(hipMemcpy(gt, f.gt, n, hipMemcpyDeviceToHost));
        for (int q = 0; q < 3; q++) {
            UZ_HIP(hipMemcpy(cols + (size_t)q * n, f.rd[q], n * 2, hipMemcpyDeviceToHost));
            UZ_HIP(hipMemcpy(cols + (size_t)(3 + q) * n, f.ad[q], n * 2, hipMemcpyDeviceToHost));
            UZ_HIP(hipMemcpy(cols + (size_t)(6 + q) * n, f.gq[q], n * 2, hipMemcpyDeviceToHost));
        }
    });
}

int uz_sites_fetch(uz_ctx *c, int sites_id, int32_t *pos, uint8_t *sflags, uint8_t *ref_base, uint8_t *alt_base) {
    return guarded(c, [&] {
        SitesDev &s = sites_of(c, sites_id); // (a pending compact table: expanded here, without its family)
        const size_t n = (size_t)s.n;
        if (!n) return;
        UZ_REQUIRE(pos != nullptr && sflags != nullptr && ref_base != nullptr && alt_base != nullptr, UZ_E_ARG, "null output");
        UZ_HIP(hipStreamSynchronize(c->stream));
        UZ_HIP(hipMemcpy(pos, s.pos, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        UZ_HIP(hipMemcpy(sflags, s.sflags, n, hipMemcpyDeviceToHost));
        UZ_HIP(hipMemcpy(ref_base, s.ref_base, n, hipMemcpyDeviceToHost));
        UZ_HIP(hipMemcpy(alt_base, s.alt_base, n, hipMemcpyDeviceToHost));
    });
}

int uz_samples_free(uz_ctx *c, int samples_id) {
    return guarded(c, [&] {
        SamplesDev &m = samples_of(c, samples_id);
        UZ_REQUIRE(m.live_fams == 0, UZ_E_STATE, "families made from this sample table are alive: uz_sites_free frees them with it");
        UZ_HIP(hipStreamSynchronize(c->stream));
        free_samples(c, m);
    });
}

int uz_sites_free(uz_ctx *c, int sites_id) {
    return guarded(c, [&] {
        SitesDev &s = sites_of(c, sites_id);
        UZ_HIP(hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < c->fams.size(); k++)
            if (c->fams[k].live && c->fams[k].sites_id == sites_id) { find_forget(c, (int)k); free_family(c, c->fams[k]); }
        for (auto &m : c->samples)
            if (m.live && m.sites_id == sites_id) free_samples(c, m);
        free_sites(c, s);
    });
}

} // extern "C"
