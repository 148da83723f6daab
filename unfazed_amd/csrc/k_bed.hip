// k_bed.hip -- BED rows as text on the device (unfazed_hip.h: uz_bed_rows, uz_bed_rows_lists).  bed_row.hpp is the body: the decision, the field
// walk, the site order.  Here: the three launches and the host side of a call (the wavefront is RowWave, text_out.hpp).
//
//   k_bed_size   one wavefront per row: the row's byte length (0: dropped), the checks of what the walk assumes
//   uz_len_scan  exclusive scan of the lengths -> off [n + 1] (one workgroup: a call has at most some ten thousand rows)
//   k_bed_fill   one wavefront per row: the bytes.  A field is written by the lanes together -- consecutive lanes, consecutive bytes -- a site
//                list by one lane per element at the offset its rank gives; no atomics but the OR of a raised flag, no LDS
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bed_row.hpp"
#include "text_out.hpp"

namespace {

struct BedArgs {
    int64_t n_rows;
    const UzBedRowDev *rows;
    UzBedLists L;
    const UzBedNames *tables;
    UzBedStrings S;
    int64_t ratio;
    int verbose, include_ambiguous;
    uint32_t *len;      // [n_rows]
    const int64_t *off; // [n_rows + 1]
    uint8_t *out;
    uint32_t *flags; // one word, behind off
};

#define UZ_BED_WAVES 4 /* rows of a workgroup */

__global__ __launch_bounds__(64 * UZ_BED_WAVES) void k_bed_size(BedArgs a) {
    const int64_t r = (int64_t)blockIdx.x * UZ_BED_WAVES + (threadIdx.x >> 6);
    if (r >= a.n_rows) return; // (the whole wavefront)
    RowWave w;
    uint32_t flags = 0;
    const UzBedRowDev R = a.rows[r];
    const uint32_t n = uz_bed_row_walk<false>(w, R, a.L, a.tables, a.S, a.ratio, a.verbose, a.include_ambiguous, nullptr, 0u, flags);
    if (w.lane() == 0) a.len[r] = n;
    if (flags) atomicOr(a.flags, flags);
}

__global__ __launch_bounds__(64 * UZ_BED_WAVES) void k_bed_fill(BedArgs a) {
    const int64_t r = (int64_t)blockIdx.x * UZ_BED_WAVES + (threadIdx.x >> 6);
    if (r >= a.n_rows) return;
    const int64_t o0 = a.off[r], o1 = a.off[r + 1];
    if (o1 <= o0) return; // a dropped row
    RowWave w;
    uint32_t flags = 0;
    const UzBedRowDev R = a.rows[r];
    const uint32_t limit = (uint32_t)(o1 - o0);
    const uint32_t n = uz_bed_row_walk<true>(w, R, a.L, a.tables, a.S, a.ratio, a.verbose, a.include_ambiguous, a.out + o0, limit, flags);
    if (n != limit) flags |= UZ_BED_F_SIZE;
    if (flags) atomicOr(a.flags, flags);
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct BedCall { // a call as its host side takes it: the lists as device pointers, the tables, per row its table and name base
    UzBedLists L;
    int32_t n_dnms = 0;
    std::vector<UzBedNames> tables;
    std::vector<int32_t> row_table;
    std::vector<uint32_t> row_qbase;
    int64_t ratio = 0;
};

void raise_flags(uint32_t f) {
    UZ_REQUIRE(!(f & UZ_BED_F_ORDER), UZ_E_STATE, "BED rows: a site list is not ascending");
    UZ_REQUIRE(!(f & UZ_BED_F_NAME), UZ_E_STATE, "BED rows: a name id at or beyond the table's names");
    UZ_REQUIRE(!(f & UZ_BED_F_SIZE), UZ_E_STATE, "BED rows: a row's written bytes differ from its sized length");
}

void bed_run(uz_ctx *c, const uz_bed_view *v, int verbose, int include_ambiguous, const BedCall &B, int64_t *off, const uint8_t **bytes) {
    const int64_t n = v->n_rows;
    off[0] = 0;
    *bytes = nullptr;
    if (n == 0) { c->bed_pin.room(64); *bytes = c->bed_pin.p; return; }
    const size_t ns = (size_t)v->n_strings, sb = ns ? (size_t)v->str_off[ns] : 0;
    // one image of the call's small inputs: rows, string offsets, string bytes, tables
    const size_t o_rows = 0, o_soff = up16(o_rows + (size_t)n * sizeof(UzBedRowDev)), o_sbytes = up16(o_soff + (ns + 1) * 4), o_tabs = up16(o_sbytes + sb + 1),
                 in_bytes = up16(o_tabs + std::max<size_t>(1, B.tables.size()) * sizeof(UzBedNames));
    c->bed_pin.room(in_bytes);
    c->bed_in.ensure(in_bytes + 64);
    UzBedRowDev *rows_h = reinterpret_cast<UzBedRowDev *>(c->bed_pin.p + o_rows);
    for (int64_t k = 0; k < n; k++) {
        const uz_bed_row &r = v->rows[k];
        UzBedRowDev &d = rows_h[k];
        d.dnm = r.dnm < 0 ? -1 : r.dnm; d.start = r.start; d.end = r.end;
        d.chrom = r.chrom; d.vartype = r.vartype; d.kid = r.kid; d.dad = r.dad; d.mom = r.mom;
        d.table = B.row_table.empty() ? 0 : B.row_table[(size_t)k];
        d.qbase = B.row_qbase.empty() ? 0u : B.row_qbase[(size_t)k];
        d.sex_origin = r.sex_origin ? 1 : 0;
    }
    memcpy(c->bed_pin.p + o_soff, v->str_off, (ns + 1) * 4);
    if (sb) memcpy(c->bed_pin.p + o_sbytes, v->str_bytes, sb);
    if (!B.tables.empty()) memcpy(c->bed_pin.p + o_tabs, B.tables.data(), B.tables.size() * sizeof(UzBedNames));
    hipStream_t st = c->stream;
    uz_kcopy(c, c->bed_in.p, c->bed_pin.p, in_bytes);
    c->bed_len.ensure((size_t)n + 16);
    c->bed_off.ensure((size_t)n + 2 + 16); // off [n + 1], then the flag word
    BedArgs a;
    a.n_rows = n;
    a.rows = reinterpret_cast<const UzBedRowDev *>(c->bed_in.p + o_rows);
    a.L = B.L;
    a.tables = reinterpret_cast<const UzBedNames *>(c->bed_in.p + o_tabs);
    a.S.off = reinterpret_cast<const uint32_t *>(c->bed_in.p + o_soff); a.S.bytes = c->bed_in.p + o_sbytes;
    a.ratio = B.ratio; a.verbose = verbose; a.include_ambiguous = include_ambiguous;
    a.len = c->bed_len.p; a.off = c->bed_off.p; a.out = nullptr;
    a.flags = reinterpret_cast<uint32_t *>(c->bed_off.p + (size_t)n + 1);
    const unsigned grid = (unsigned)((n + UZ_BED_WAVES - 1) / UZ_BED_WAVES);
    UZ_HIP(hipMemsetAsync(c->bed_off.p + (size_t)n + 1, 0, 8, st));
    {
        ProfScope ps(c, UZ_K_BED_SIZE);
        hipLaunchKernelGGL(k_bed_size, dim3(grid), dim3(64 * UZ_BED_WAVES), 0, st, a);
        UZ_HIP(hipGetLastError());
        uz_len_scan(c, st, n, c->bed_len.p, 0, c->bed_off.p);
    }
    UZ_HIP(hipStreamSynchronize(st)); // (the inputs have left the page-locked block)
    const size_t off_bytes = ((size_t)n + 2) * 8;
    c->bed_pin.room(off_bytes);
    uz_kcopy(c, c->bed_pin.p, c->bed_off.p, off_bytes);
    UZ_HIP(hipStreamSynchronize(st));
    const int64_t *off_h = reinterpret_cast<const int64_t *>(c->bed_pin.p);
    raise_flags((uint32_t)off_h[n + 1]);
    const int64_t total = off_h[n];
    UZ_REQUIRE(total >= 0 && total < ((int64_t)1 << 32), UZ_E_RANGE, "BED rows: 4 GiB or more of text in one call");
    memcpy(off, off_h, ((size_t)n + 1) * 8);
    if (total == 0) { *bytes = c->bed_pin.p; return; }
    const size_t text = ((size_t)total + 15) & ~(size_t)15;
    c->bed_out.ensure(text + 64);
    c->bed_pin.room(text + 16);
    a.out = c->bed_out.p;
    {
        ProfScope ps(c, UZ_K_BED_FILL);
        hipLaunchKernelGGL(k_bed_fill, dim3(grid), dim3(64 * UZ_BED_WAVES), 0, st, a);
        UZ_HIP(hipGetLastError());
    }
    uz_kcopy(c, c->bed_pin.p, c->bed_out.p, text);
    uz_kcopy(c, c->bed_pin.p + text, a.flags, 8);
    UZ_HIP(hipStreamSynchronize(st));
    raise_flags(*reinterpret_cast<const uint32_t *>(c->bed_pin.p + text));
    *bytes = c->bed_pin.p;
}

// what every call checks of its view: string ids, DNM indices
void check_view(const uz_bed_view *v, int64_t *off, const uint8_t **bytes, int32_t n_dnms) {
    UZ_REQUIRE(v && off && bytes && v->n_rows >= 0 && v->n_rows < 0x7FFFFFF0 && (v->n_rows == 0 || v->rows), UZ_E_ARG, "BED rows: bad arguments");
    UZ_REQUIRE(v->n_strings >= 0 && v->str_off && (v->str_bytes || v->n_strings == 0 || v->str_off[v->n_strings] == 0), UZ_E_ARG, "BED rows: no string table");
    for (int32_t k = 0; k < v->n_strings; k++) UZ_REQUIRE(v->str_off[k + 1] >= v->str_off[k], UZ_E_ARG, "BED rows: the string offsets descend");
    const uint32_t ns = (uint32_t)v->n_strings;
    for (int64_t k = 0; k < v->n_rows; k++) {
        const uz_bed_row &r = v->rows[k];
        UZ_REQUIRE(r.chrom < ns && r.vartype < ns && r.kid < ns && r.dad < ns && r.mom < ns, UZ_E_ARG, "BED rows: a string id out of range");
        UZ_REQUIRE(r.dnm < n_dnms, UZ_E_ARG, "BED rows: a DNM index out of range");
    }
}

} // namespace

int uz_bed_rows_impl(uz_ctx *c, const uz_bed_view *v, int verbose, int include_ambiguous, int64_t *off, const uint8_t **bytes) {
    BedCall B;
    memset(&B.L, 0, sizeof(B.L));
    uz_phase_lists_dev(c, &B.n_dnms, &B.L.status, &B.L.counts, &B.L.pool, &B.L.list_start, &B.L.list_len);
    check_view(v, off, bytes, B.n_dnms);
    B.ratio = c->P.evidence_min_ratio;
    const int64_t n = v->n_rows;
    if (verbose) {
        UZ_REQUIRE(B.L.pool != nullptr, UZ_E_STATE, "uz_bed_rows: verbose, and the last batch kept no lists");
        // the tables the rows name, each once
        std::vector<int> slot(c->reads.size(), -1);
        B.row_table.assign((size_t)n, 0);
        for (int64_t k = 0; k < n; k++) {
            const uz_bed_row &r = v->rows[k];
            if (r.dnm < 0) continue;
            UZ_REQUIRE(r.reads_id >= 0 && (size_t)r.reads_id < c->reads.size() && c->reads[(size_t)r.reads_id].live, UZ_E_ARG, "uz_bed_rows: a reads id out of range");
            if (slot[(size_t)r.reads_id] < 0) {
                const ReadsDev &t = c->reads[(size_t)r.reads_id];
                UZ_REQUIRE(t.kept_list && t.name_rec && t.names, UZ_E_STATE, "uz_bed_rows: verbose with a table that holds no names on the device");
                UzBedNames T;
                memset(&T, 0, sizeof(T));
                T.name_rec = t.name_rec; T.kept = t.kept_list; T.names = t.names; T.n_recs = t.n; T.names_bytes = t.names_bytes; T.n_qnames = t.n_qnames; T.has_names = 1;
                slot[(size_t)r.reads_id] = (int)B.tables.size();
                B.tables.push_back(T);
            }
            B.row_table[(size_t)k] = slot[(size_t)r.reads_id];
        }
        if (!c->phase_qbase.empty()) { // a cohort batch: the pool's ids are the merged table's (k_reads.hip: gather_lists)
            B.row_qbase.assign((size_t)n, 0u);
            for (int64_t k = 0; k < n; k++)
                if (v->rows[k].dnm >= 0) B.row_qbase[(size_t)k] = c->phase_qbase[(size_t)v->rows[k].dnm];
        }
    } else {
        B.L.pool = nullptr; B.L.list_start = nullptr; B.L.list_len = nullptr; // (the four lengths are the batch's counts: nothing else is read)
    }
    if (!B.L.pool) B.L.list_start = nullptr;
    bed_run(c, v, verbose, include_ambiguous, B, off, bytes);
    return 0;
}

int uz_bed_rows_lists_impl(uz_ctx *c, const uz_bed_view *v, int verbose, int include_ambiguous, int32_t n_dnms, const int32_t *status, const int64_t *list_off,
                           const int32_t *list_val, uint32_t n_qnames, const uint32_t *name_off, const uint8_t *name_bytes, int32_t ratio, int64_t *off,
                           const uint8_t **bytes) {
    UZ_REQUIRE(n_dnms >= 0 && (n_dnms == 0 || (status && list_off)), UZ_E_ARG, "uz_bed_rows_lists: bad arguments");
    check_view(v, off, bytes, n_dnms);
    const size_t nd = (size_t)n_dnms;
    int64_t n_val = 0;
    if (nd) {
        UZ_REQUIRE(list_off[0] == 0, UZ_E_ARG, "uz_bed_rows_lists: the list offsets start at 0");
        for (size_t k = 0; k < 4 * nd; k++)
            UZ_REQUIRE(list_off[k + 1] >= list_off[k] && list_off[k + 1] - list_off[k] < ((int64_t)1 << 31), UZ_E_ARG, "uz_bed_rows_lists: the list offsets descend");
        n_val = list_off[4 * nd];
        UZ_REQUIRE(n_val == 0 || list_val, UZ_E_ARG, "uz_bed_rows_lists: no list values");
    }
    const bool names = name_off != nullptr;
    size_t nb = 0;
    if (names) {
        for (uint32_t k = 0; k < n_qnames; k++) UZ_REQUIRE(name_off[k + 1] >= name_off[k], UZ_E_ARG, "uz_bed_rows_lists: the name offsets descend");
        nb = name_off[n_qnames];
        UZ_REQUIRE(nb == 0 || name_bytes, UZ_E_ARG, "uz_bed_rows_lists: no name bytes");
    }
    UZ_REQUIRE(!verbose || names, UZ_E_STATE, "uz_bed_rows_lists: verbose without names");
    // the caller's lists and names -> the device, one image
    const size_t o_status = 0, o_off = up16(o_status + nd * 4 + 4), o_val = up16(o_off + (4 * nd + 1) * 8), o_noff = up16(o_val + (size_t)n_val * 4 + 4),
                 o_nbytes = up16(o_noff + ((size_t)n_qnames + 1) * 4), total = up16(o_nbytes + nb + 1);
    c->bed_pin.room(total);
    c->bed_hook.ensure(total + 64);
    memset(c->bed_pin.p, 0, total);
    if (nd) {
        memcpy(c->bed_pin.p + o_status, status, nd * 4);
        memcpy(c->bed_pin.p + o_off, list_off, (4 * nd + 1) * 8);
        if (n_val) memcpy(c->bed_pin.p + o_val, list_val, (size_t)n_val * 4);
    }
    if (names) {
        memcpy(c->bed_pin.p + o_noff, name_off, ((size_t)n_qnames + 1) * 4);
        if (nb) memcpy(c->bed_pin.p + o_nbytes, name_bytes, nb);
    }
    uz_kcopy(c, c->bed_hook.p, c->bed_pin.p, total);
    UZ_HIP(hipStreamSynchronize(c->stream)); // (bed_run stages its own inputs in the same block)
    BedCall B;
    memset(&B.L, 0, sizeof(B.L));
    B.n_dnms = n_dnms;
    B.L.status = reinterpret_cast<const int32_t *>(c->bed_hook.p + o_status);
    B.L.off4 = reinterpret_cast<const int64_t *>(c->bed_hook.p + o_off);
    B.L.pool = reinterpret_cast<const int32_t *>(c->bed_hook.p + o_val);
    B.ratio = ratio;
    UzBedNames T;
    memset(&T, 0, sizeof(T));
    if (names) {
        T.plain_off = reinterpret_cast<const uint32_t *>(c->bed_hook.p + o_noff); T.plain_bytes = c->bed_hook.p + o_nbytes; T.n_qnames = n_qnames; T.has_names = 1;
    }
    B.tables.push_back(T);
    bed_run(c, v, verbose, include_ambiguous, B, off, bytes);
    return 0;
}
