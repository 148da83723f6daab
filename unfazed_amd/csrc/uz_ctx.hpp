// uz_ctx.hpp -- internal state of the C ABI context (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <memory>
#include <vector>

#include "unfazed_hip.h"
#include "uz_bamwalk.h"
#include "bgzf_batch.hpp"
#include "walk_book.hpp"

struct UzError {
    int code;
    std::string msg;
};

#define UZ_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            throw UzError{UZ_E_HIP, std::string(#call) + ": " + hipGetErrorString(e__)};               \
    } while (0)

#define UZ_REQUIRE(cond, code, text)          \
    do {                                      \
        if (!(cond)) throw UzError{code, text}; \
    } while (0)

// grow-only device buffer
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        size_t want = n + n / 4 + 64;
        UZ_HIP(hipMalloc((void **)&p, want * sizeof(T)));
        cap = want;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // The same for buffers that grow while OTHER work is running on the device (the slots of walked batches: uz_bam_walk on a decoder's thread,
    // beside the read stage of another chunk): hipFree waits for the whole device, so the block that was outgrown is not freed but handed back in
    // *old for the caller to park (uz_walk_grow), and the new one is sized for the largest request any buffer of this kind has seen (hi >= n: a
    // slot that grows once then fits every batch the process has staged).  used > 0: the first `used` elements are carried over (on stream st).
    // -> false: it fitted, nothing was allocated.
    bool ensure_parked(size_t n, size_t hi, std::pair<void *, size_t> *old, size_t used = 0, hipStream_t st = nullptr) {
        if (n <= cap) return false;
        const size_t want = hi + hi / 4 + 64;
        T *q = nullptr;
        UZ_HIP(hipMalloc((void **)&q, want * sizeof(T)));
        if (p && used) UZ_HIP(hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
        *old = {(void *)p, cap * sizeof(T)};
        p = q;
        cap = want;
        return true;
    }
};

// grow-only page-locked block
struct PinBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    void room(size_t need, size_t keep = 0) { // grown to `need`, its first `keep` bytes carried over
        if (cap >= need) return;
        const size_t want = need + need / 4 + 4096;
        uint8_t *q = nullptr;
        UZ_HIP(hipHostMalloc((void **)&q, want, hipHostMallocDefault));
        if (keep) memcpy(q, p, keep);
        if (p) (void)hipHostFree(p);
        p = q;
        cap = want;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The buffers of a call that writes a file's bytes chunk by chunk (text_out.hpp: ChunkLoop), kept from call to call: the two chunk images
// (page-locked, and their mirrors on the device), a chunk's lengths, its small results (offsets + flag word + what the call adds) and their page-
// locked landing place, a chunk's bytes on the device, the call's bytes (page-locked)
struct OutBufs {
    PinBuf pin[2], small_pin, res;
    DevBuf<uint8_t> in[2], small, out;
    DevBuf<uint32_t> len;
    void release() {
        for (int b = 0; b < 2; b++) { pin[b].release(); in[b].release(); }
        small_pin.release(); res.release(); small.release(); out.release(); len.release();
    }
};

// what a set of window lists was computed for
struct FindKey {
    bool valid = false;
    int fam = -1, mode = 0;
    int32_t n = -1;
    bool cohort = false;
    uint64_t hash = 0; // of the DNM columns the window emit reads
    uz_params P;
};
#define UZ_FIND_ALTS 2
struct FindSlot { // the window lists of one uz_find, parked
    FindKey key;
    unsigned long long stamp = 0;
    DevBuf<int32_t> cnt_c, cnt_h;
    DevBuf<int64_t> win_range;
    DevBuf<int64_t> cand_off, het_off;
    DevBuf<int32_t> cand_idx, het_idx;
    DevBuf<uint8_t> cand_flags;
    int64_t n_cand = 0, n_het = 0;
    std::vector<int64_t> cand_off_h, het_off_h;
};

// one device allocation out of the context's pool (tables come and go every staged pass: hipFree
// synchronises the device, so freed blocks are parked and handed out again)
struct DevBlock {
    uint8_t *p = nullptr;
    size_t cap = 0;
};

struct SitesDev {
    bool live = false, owned = false;
    DevBlock block; // owned tables: every column in one pooled block
    DevBlock mirror; // asynchronous upload of a slab of host columns: its image (sites + genotype columns; uz_stage.hpp: SlabPlan)
    int64_t n = 0;
    int32_t n_contigs = 0;
    std::vector<int64_t> contig_off_h;
    int64_t *contig_off = nullptr;
    int32_t *pos = nullptr;
    uint8_t *sflags = nullptr, *ref_base = nullptr, *alt_base = nullptr;
    hipEvent_t ready = nullptr; // asynchronous upload: end of the copies on the copy stream; the first use waits for it
    bool pending = false;
    // compact link form (uz_sites_view.pos_d16 ...): the staged columns, expanded into pos / sflags / ref_base / alt_base at first use
    // (uz_sites_expand: with the first family of the table in the same launch)
    bool expand_pending = false;
    const uint16_t *c_d16 = nullptr;
    const uint8_t *c_b8 = nullptr;
    const int32_t *c_span = nullptr, *c_eidx = nullptr, *c_eval = nullptr, *c_eoff = nullptr;
};

struct FamilyDev {
    bool live = false, owned = false;
    DevBlock block; // the class column and, for owned tables, the genotype columns
    int sites_id = -1;
    uint8_t *gt = nullptr; // bits 0-5 genotypes; bit 6 = the site's complex flag, folded in at upload
    uint16_t *rd[3] = {nullptr, nullptr, nullptr};
    uint16_t *ad[3] = {nullptr, nullptr, nullptr};
    uint16_t *gq[3] = {nullptr, nullptr, nullptr};
    uint8_t *cls = nullptr;
    // sites whose depths the 16-bit columns cannot hold (uz_family_view.wide_*): index + six 32-bit depths each, in a small block of
    // their own; their class bytes are rewritten after every site scan (k_site_scan_wide)
    int64_t n_wide = 0;
    int64_t *wide_site = nullptr;
    int32_t *wide_depth = nullptr; // [6][n_wide]: rd kid, dad, mom, ad kid, dad, mom
    DevBlock wide_block;
    std::shared_ptr<std::vector<int32_t>> wide_host; // the host copy the (asynchronous) upload of wide_depth reads: kept with the family
    // asynchronous upload (uz_sites_family_upload_async): the copies are queued on the copy stream; `ready` marks their end and
    // the first use of the family makes the compute stream wait for it and folds the complex flag (family_make_ready)
    hipEvent_t ready = nullptr;
    bool pending = false;
    // eight-bit link form (uz_family_view.ref_depth8 ...): the staged bytes, widened into rd / ad / gq at first use; gq was clamped at 254
    const uint8_t *stage8[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool widen_pending = false, gq_clamped = false;
    // het form (uz_family_view.het9 ...): the staged bytes of the kid-het sites; uz_sites_expand writes rd / ad / gq from them (zeros at every
    // other site).  het_only stays set for the family's life: the DEL / DUP classes and uz_family_fetch refuse it (uz_refuse_het_only)
    bool het_only = false;
    const uint8_t *het9 = nullptr;
    const int32_t *het_off = nullptr;
    int64_t n_het = 0;
    // made by uz_families_from_samples: rd / ad / gq are rows of that sample table, wide_site is the table's, and gt / cls / wide_depth
    // lie in a block the TABLE owns (one per call, SamplesDev::fam_blocks) -- `block` and `wide_block` stay empty
    int samples_id = -1;
    bool cls_valid = false;
    bool cls_has_cnv = false; // DEL / DUP codes (bits 3-6) computed
    uz_params cls_params;
};

// the 16-bit genotype columns of a cohort's samples, sample-major (uz_samples_view): rows are padded to a stride that keeps every row
// 256-byte aligned (the site scan reads a family's columns -- rows of this table -- in 16-byte vectors)
struct SamplesDev {
    bool live = false;
    int sites_id = -1;
    int32_t n_samples = 0;
    DevBlock block;                   // the rows, the wide list
    std::vector<DevBlock> fam_blocks; // gt / cls / wide depths of the families made from the table: one block per uz_families_from_samples
    int live_fams = 0;                // families that alias the rows: the table cannot be freed before them
    size_t stride = 0;                // elements between two rows (of gt and of the 16-bit columns alike)
    uint8_t *gt = nullptr;
    uint16_t *rd = nullptr, *ad = nullptr, *gq = nullptr;
    int64_t n_wide = 0;
    int64_t *wide_site = nullptr;
    int32_t *wide_rd = nullptr, *wide_ad = nullptr; // [n_samples][n_wide]
    hipEvent_t ready = nullptr; // end of the copies on the copy stream; the first uz_families_from_samples makes the compute stream wait for it
    bool pending = false;
    // a table parsed from the text on the device (uz_samples_from_text): the sites handed back to the host's reader, ascending; while
    // need_settle the rows of those sites are void and the table makes no family (uz_samples_settle overwrites them and brings the wide
    // list, which lies in a block of its own: its size is known only then)
    std::vector<int64_t> unsettled;
    bool need_settle = false;
    DevBlock wide_block;
};

// the fixed-width columns of a table as DEVICE pointers (staged by an upload, or the caller's for an adopted table)
struct RecColumns {
    const int32_t *start = nullptr, *end = nullptr, *tlen = nullptr, *mate = nullptr;
    const uint32_t *qname = nullptr;
    const uint16_t *flag = nullptr, *l_seq = nullptr, *n_cigar = nullptr;
    const uint8_t *mapq = nullptr, *aux = nullptr;
    // qualities of the staged form: the plane itself (plane_in: the header build counts its bits into nlow) or its list
    // form (n_low + qlow_pos: the header build copies the counts and writes the plane rows of the listed records); both
    // null for an ASCII upload, whose plane and counts are built from the quality bytes (uz_build_qlow)
    const uint32_t *cigar_staged = nullptr; // cigar_compact: the words that travelled (records with a simple code own none); the header build writes
    uint32_t *cigar_out = nullptr;          // ... every record's words here (the device's CIGAR store).  Both null: `cigar_in` is the store itself
    const uint32_t *cigar_in = nullptr; // the record's CIGAR words (at its cigar offset): `end` is derived from them when the column is left out (end == nullptr)
    const uint16_t *umask = nullptr;    // staged units per record (null: every unit)
    // dictionary form of the small columns (tup set: flag / l_seq / n_cigar / mapq / aux / n_low are read through the table)
    const uint16_t *tup = nullptr, *tup_flag = nullptr, *tup_l_seq = nullptr, *tup_n_cigar = nullptr;
    const uint8_t *tup_mapq = nullptr, *tup_aux = nullptr, *tup_n_low = nullptr;
    const uint16_t *tup_umask = nullptr;
    int64_t n_tup = 0; // entries of the dictionary (0: not known)
    // the index in one byte (uz_types.h tup8): the header build first rebuilds the 16-bit column into tup_out (k_tup_expand) and reads it as `tup`
    const uint8_t *tup8 = nullptr;
    const uint16_t *tup_hot = nullptr, *tup_esc = nullptr;
    const uint32_t *tup_esc_off = nullptr;
    int64_t n_tup_esc = 0;
    uint16_t *tup_out = nullptr;
    // bases as lists (uz_types.h: bl_*): per record the number of listed bases (plain column or through the dictionary), their query indices and
    // two-bit codes; seq4_out: the device's base rows (the header build writes the units of the listed records, behind the n_seq_link units that
    // travelled as rows)
    const uint8_t *bl_n = nullptr, *tup_n_bl = nullptr, *bl_pos = nullptr, *bl_code = nullptr;
    const uint8_t *bl_qlow = nullptr; // the quality bits of the listed bases (uz_types.h bl_qlow; null: such a record's positions stand in qlow_pos)
    int32_t bl_wide = 0;
    int64_t n_seq_link = 0;
    uint32_t *seq4_out = nullptr;
    __host__ __device__ bool bl_form() const { return bl_n != nullptr || tup_n_bl != nullptr; }
    // 16-bit difference form of start / tlen / mate / qname (start_d set: the plain four are null)
    const int16_t *start_d = nullptr, *tlen_s = nullptr, *mate_d = nullptr, *qname_d = nullptr;
    const uint8_t *start_d8 = nullptr; // the start differences in eight bits (then start_d is null)
    const int8_t *mate_d8 = nullptr, *qname_d8 = nullptr; // mate / name-id differences in eight bits (then mate_d / qname_d are null)
    const uint8_t *pair_d8 = nullptr; // the pair form: tlen, mate and name id in one byte (then tlen_s and the four above are null)
    __host__ __device__ bool diff_form() const { return tlen_s != nullptr || pair_d8 != nullptr; } // start (and the rest) travel as differences
    const unsigned long long *esc16_key = nullptr;
    const int32_t *esc16_val = nullptr;
    int64_t n_esc16 = 0;
    int64_t esc_lo = 0, esc_hi = 0;   // set by the header build's workgroups: the escape entries of their own span of records
    int32_t pk_shift = 12;            // set by the header build: records per span of its passes = 1 << pk_shift (a small table gets shorter spans: more workgroups)
    int32_t lists = 0; // the qualities came as counts (+ positions): n_low, or tup_n_low through the table
    const uint32_t *plane_in = nullptr;
    const uint8_t *n_low = nullptr, *qlow_pos = nullptr;
    int32_t qpos_wide = 0;
    // the span sums from the packer (uz_types.h pk_sums: [(spans + 1) * UZ_PK_SUMS], exclusive): null -- the header build computes them itself
    const unsigned long long *pk_sums = nullptr;
};

struct ReadsDev {
    bool live = false;
    int64_t n = 0;
    int32_t n_contigs = 0;
    uint32_t n_qnames = 0;
    int64_t n_cigar_total = 0, n_row_units = 0, n_seq_units = 0;
    DevBlock block;            // everything the library owns for this table lives in this one block
    DevBlock mirror;           // ... except, when the host columns came over the link as one slab, the slab's image (uz_stage.hpp: SlabPlan)
    int64_t *contig_off = nullptr;
    int32_t *max_span = nullptr;
    void *rec_a = nullptr, *rec_b = nullptr; // RecA / RecB headers (phase_body.hpp)
    uint32_t *fm = nullptr;    // flag | mapq << 16 | aux << 24
    uint32_t *qoff = nullptr;  // quality-plane row of every record (row units); UZ_NO_QLOW_OFF: none (its bits can never be asked for)
    uint16_t *umask = nullptr; // staged 32-base units of every record's rows (UZ_UMASK_ALL: every unit)
    uint8_t *nlow = nullptr;   // low-quality bases of every record, saturated at 255 (what K3a needs of the qualities)
    int64_t n_qlow_pos = 0;    // list form of the staged plane: entries (checked against the columns by the header build)
    int64_t n_plane_units = 0; // units the quality-plane store holds: n_row_units (plane / ASCII form: every record has a row), n_seq_units (list form)
    const uint32_t *cigar = nullptr;
    const uint8_t *seq4 = nullptr;
    uint8_t *qlow = nullptr;   // caller's memory for adopted tables (then never written)
    int32_t qlow_thr = 0;      // threshold the qlow plane holds
    bool qlow_valid = false;
    // ASCII uploads (uz_reads_upload) keep the full qualities so that the plane can be rebuilt for another threshold
    uint8_t *qual8 = nullptr;
    uint32_t *qual_off16 = nullptr;
    uint16_t *qs = nullptr;    // per-record QC word (phase_body.hpp: uz_qs_word), written by the header build
    int32_t *coarse = nullptr; // start of every 4096th record
    int32_t *mid = nullptr;    // start of every 64th record (phase_body.hpp: uz_lower_bounds_c)
    int32_t *mid8 = nullptr;   // start of every 8th record (uz_mid8_refine)
    hipEvent_t ready = nullptr; // asynchronous uploads: recorded behind the last copy of the upload
    bool pending = false;       // the copies may still be in flight and the headers not built yet: the first use waits (uz_reads_make_ready)
    // The header build of an asynchronous upload is queued with the upload on a stream of its own (uz_ctx::build_stream), behind the
    // copies' event: on the copy stream it would hold up the next table's copies, on the compute stream (where it ran at first use) it
    // sat in the chain of every chunk's read stage.  `built` marks its end; null: no build queued yet, the first use runs it
    // (UZ_BUILD_LAZY=1).
    hipEvent_t built = nullptr;
    RecColumns cols; // the staged columns of an asynchronous upload, as its header build takes them (an adopted table keeps none of the caller's)
    void *build_scratch = nullptr;
    int64_t n_cigar_staged = 0; // cigar_compact: words that travelled (checked by the header build)
    // a table that arrived with two-bit base rows (uz_reads_packed_view.seq2): the staged rows and the listed bases, expanded
    // into seq4 by the header build (uz_build_records); null afterwards / for four-bit tables
    const uint8_t *seq2_staged = nullptr;
    const uint32_t *exc_rec = nullptr;
    const uint16_t *exc_pos = nullptr;
    const uint8_t *exc_code = nullptr;
    int64_t n_exc = 0;
    // bases as lists (uz_types.h bl_*): the listed bases and the row units of the records that carry them (inside n_seq_units: their units
    // lie behind the n_seq_units - n_bl_units that travelled as rows)
    int64_t n_bl = 0, n_bl_units = 0;
    // a table built from a batch joined on the device (uz_reads_from_walk with names): the kept list, the record that brought every name id first and
    // the read names of the records, all in `mirror` -- uz_reads_names answers ids from them
    const uz_kept_rec *kept_list = nullptr;
    const uint32_t *name_rec = nullptr;
    const uint8_t *names = nullptr;
    int64_t names_bytes = 0;
};

// DNM batch staged on the device
template <typename T>
struct DevPtr { T *p = nullptr; };
struct DnmsDev { // the columns of a DNM batch: one block in HBM, laid out like its pinned staging copy (ONE copy brings a batch over)
    int32_t n = 0;
    DevBuf<uint8_t> block;
    DevPtr<int32_t> contig, rcontig, start, end;
    DevPtr<uint8_t> vartype, dflags, mult;
    DevPtr<uint32_t> allele_off;
    DevPtr<uint8_t> alleles;
    double cutoff = 0;
};

struct ProfSlot {
    double total_ms = 0;
    int64_t launches = 0;
    int64_t last_units = 0;
};
struct ProfPending {
    int kernel;
    hipEvent_t a, b;
};

struct uz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // compute (and the synchronous uploads)
    hipStream_t copy_stream = nullptr; // asynchronous uploads of packed tables: the copies
    hipStream_t build_stream = nullptr; // ... and their header builds (created at the first asynchronous upload)
    int32_t *hflags = nullptr;         // pinned, device-visible: [0] upload consistency error (totals / alphabet), [1] bases of a row-less
                                       // record requested; [4..7] two int64 mailboxes (list totals of the window emit)
    std::vector<DevBlock> block_pool;
    uz_params P;
    std::string err;
    std::mutex err_mu; // (err is written by whichever thread's call failed: uz_stage.hpp set_error)
    std::vector<SitesDev> sites;
    std::vector<FamilyDev> fams;
    std::vector<ReadsDev> reads;
    std::vector<SamplesDev> samples;
    DevBuf<int32_t> trio_idx; // uz_families_from_samples: kid / dad / mom sample indices of the batch's trios
    uint8_t *vcf_pin[2] = {nullptr, nullptr}; // uz_samples_from_text / _from_bcf: the two page-locked chunk images, kept from call to call
    size_t vcf_pin_cap[2] = {0, 0};

    // allele-balance threshold table of K1 (k_sites.hip), rebuilt when the thresholds change
    DevBuf<int32_t> ab_lut;
    DevBuf<uint8_t> fam_batch; // cohort scan: per-family column pointers
    bool ab_lut_valid = false;
    bool ab_lut_t0_special = false;
    uz_params ab_lut_params;

    // last find
    bool find_valid = false;
    int find_fam = -1, find_mode = 0;
    DnmsDev dn;
    uint8_t *dn_stage = nullptr; // pinned staging of a DNM batch
    PinBuf find_pin; // landing place of a find's offsets (copied there by a kernel: see uz_kcopy)
    // the last find call of the context (uz_find_stats): stream waits of the host, kernel launches, UZ_FA_* of a uz_find_answer, the block it needs
    int64_t find_stat[4] = {0, 0, 0, 0};
    bool find_counting = false; // inside a find call (FindCount): the copy helpers' launches are the find's
    bool find_answer_again = false; // the last find call was a uz_find_answer that fell back: the same batch may come again for its answer
    int32_t dn_n_of_find = 0; // DNMs of the batch the context's window lists are of
    size_t dn_stage_cap = 0;
    hipEvent_t dn_stage_done = nullptr; // behind the copies out of dn_stage: a batch queued by uz_phase_begin may still be reading it
    DevBuf<int64_t> scan_part;   // tile sums of a large find's two count arrays (k_scan2_sums -> k_scan2) and of the allele-balance stage's (k_scan1_sums -> k_scan1)
    DevBuf<int32_t> cnt_c, cnt_h;
    DevBuf<int64_t> win_range;
    DevBuf<int64_t> cand_off, het_off;
    DevBuf<int32_t> cand_idx, het_idx;
    DevBuf<uint8_t> cand_flags;
    int64_t n_cand = 0, n_het = 0;
    std::vector<int64_t> cand_off_h, het_off_h;
    // Whose window lists these are, and the lists of the two finds BEFORE the last one, kept aside (find_alt): a staged pass asks for
    // the lists of chunk k + 1 (uz_find: the decoder's input) before it queues the read stage of chunk k, whose own uz_find ran one
    // call earlier -- the read stage then takes those lists instead of running the window emit (and its host round trip) again; the
    // third set leaves room for the whole-region lists of an allele-balance stage in between.
    FindKey find_key;
    unsigned long long find_stamp = 0, find_counter = 0;
    FindSlot find_alt[UZ_FIND_ALTS];

    // cohort batch (uz_phase_cohort): per-DNM family / insert cutoff / query-name base, the class column of every family, and
    // the reads tables of the kids laid end to end as ONE table (virtual contigs = kid x contig)
    bool cohort_on = false;
    DevBuf<int32_t> dn_fam;
    DevBuf<double> dn_cutoff;
    DevBuf<uint8_t *> fam_cls;
    std::vector<uint32_t> phase_qbase; // per DNM: first query-name id of its kid in the merged table (empty: no offset)
    int cohort_reads = -1;             // slot in `reads` holding the merged table
    std::vector<int> cohort_ids;       // the tables it was built from

    // last CNV stage (K6)
    bool cnv_valid = false;
    int32_t cnv_n = 0;
    DevBuf<int32_t> cnv_counts, cnv_pos, cnv_origin, cnv_evidence, cnv_etype, cnv_rb;
    DevBuf<int64_t> cnv_off;   // [2n + 1] exclusive scan of cnv_counts: where every site list starts in cnv_dense
    DevBuf<int32_t> cnv_dense; // the site lists back to back (k_cnv_dense): what uz_phase_cnv_sites copies
    std::vector<int32_t> cnv_counts_h;
    std::vector<int64_t> cnv_off_h;

    // BGZF inflate (k_inflate.hip, uz_bgzf_inflate_to_host): buffers kept from call to call, streams of its own (a batch's blocks can
    // be inflated while the read stage of the batch before is still queued on the compute stream) -- what it hands uz_queue_inflate.  The call
    // may run on a decoder's worker thread beside the owner's: nothing of it is shared with the other routes
    DevBuf<uint8_t> inf_comp, inf_out;
    DevBuf<int64_t> inf_in, inf_off;
    DevBuf<int32_t> inf_flags;
    hipStream_t inf_stream = nullptr, inf_stream2 = nullptr;
    hipEvent_t inf_ready = nullptr;

    // the record walk on the device (k_bamwalk.hip, uz_bam_walk): a batch's inflated blocks stay in HBM from the walk until the batch's table has
    // been packed from them (uz_reads_from_bam); four batches can be in flight (a feed pipeline walks up to three chunks ahead of the read stage)
    struct WalkSlot { // (held or free: uz_ctx::book)
#define UZ_X(T, name) DevBuf<T> name;
        UZ_WALK_BUFS(UZ_X) // walk_book.hpp: the one table of the slot's buffers
        int64_t n_blocks = 0, out_bytes = 0, n_desc = 0, n_desc_all = 0, n_reach = 0;
        int32_t n_tasks = 0, max_host = -1; // (max_host: the last walk task's stage task, column 9 of the plan)
        hipStream_t s0 = nullptr, s1 = nullptr; // the slot's own streams (blocks up + inflate in slices on both, the walk on the first)
        hipEvent_t ev = nullptr;
        // the batch-wide joins on the device (k_bamjoin.hip, uz_bam_join): all descriptors of the batch -- the device's own (desc_kept[0 .. n_dev)) and
        // behind them what the host walked itself (tasks handed back, mates looked up through the index) -- with their join state
        struct Join {
            int64_t n_dev = 0, n_all = 0, aux_bytes = 0;
            int32_t n_host = 0, n_look = 0, n_ref = 0, round = 0, trips = 0; // trips: answered sets of needs (uz_bamwalk.h UZ_JOIN_MAX_TRIPS)
            int64_t n_need = 0;
            bool filled = false, started = false, done = false, all_bases = false;
            UZ_JOIN_BUFS(UZ_X)
#undef UZ_X
            int64_t tot_h[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // the totals of the finished join (k_bamjoin.hip: JT_*)
            std::vector<int64_t> contig_off_h;
            std::vector<int32_t> max_span_h;
        } join;
    };
    static constexpr int WALK_SLOTS = WalkBook::SLOTS;
    WalkSlot walk[WALK_SLOTS];
    WalkBook book; // which slots are held, the largest request every kind of buffer has seen, the blocks that were outgrown (its own lock)

    // the heads of a cohort's alignment files (k_bamhead.hip, uz_head_walk): a head holds the tlen columns of its files, file f's at first[f] with
    // room for want[f] records, have[f] of them written by the walks so far; the walk's own buffers (hd_*: what it hands uz_queue_inflate, on the
    // compute stream) are the context's and grow like the others
    struct HeadDev {
        bool live = false;
        int32_t n_files = 0;
        std::vector<int64_t> want, have, first; // first: [n_files + 1]
        DevBuf<int32_t> tlen;
        DevBuf<int64_t> first_d;
    };
    std::vector<HeadDev> heads;
    DevBuf<uint8_t> hd_comp, hd_out;
    DevBuf<int64_t> hd_i64;
    DevBuf<int32_t> hd_i32;
    DevBuf<uint32_t> hd_u32;

    // uz_reads_names: ids / lengths / offsets / bytes on the device and one page-locked staging block, kept from call to call
    DevBuf<uint32_t> nm_ids, nm_len, nm_off;
    DevBuf<int64_t> rf_first; // uz_reads_files: the files' first records, and ...
    DevBuf<uint32_t> rf_mm;   // ... their smallest and largest name ids
    DevBuf<uint8_t> nm_out;
    PinBuf nm_pin;

    // uz_bed_rows (k_bed.hip): the call's rows, strings and tables on the device (bed_in; the caller's lists of uz_bed_rows_lists behind them in
    // bed_hook), the rows' lengths, their offsets + the flag word, the text; one page-locked block, all kept from call to call
    DevBuf<uint8_t> bed_in, bed_hook, bed_out;
    DevBuf<uint32_t> bed_len;
    DevBuf<int64_t> bed_off;
    PinBuf bed_pin;
    // uz_vcf_rows (k_vcfout.hip), uz_bcf_rows (k_bcfout.hip) -- a set of its own: the text it returns is the input of the uz_vcf_rows call behind
    // it -- and uz_bgzf_deflate (k_deflate.hip: counts and CRC-32s among the small results, no lengths; df_slots: the streams' scratch slots;
    // df_tokens: the dynamic code's tokens between its passes, 65 280 words a slice of the chunk, allocated by the first call that asks for it)
    OutBufs vo, bo, df;
    DevBuf<uint8_t> df_slots;
    DevBuf<uint32_t> df_tokens;
    // uz_bgzf_deflate_indexed (k_tbx.hip): the row table of a call (resident across its chunks), a chunk's tile counts / offsets / line starts,
    // the work arrays and the tables of the passes behind the last chunk; their page-locked landing place
    DevBuf<uint8_t> tbx_rows, tbx_chunk, tbx_work, tbx_tab;
    PinBuf tbx_pin;

    // last phase (k_reads.hip)
    bool phase_valid = false;
    bool phase_open = false; // uz_phase_begin without its uz_phase_end
    int32_t phase_n = 0;
    void *phase_state = nullptr;

    // profiling
    uint32_t prof_mask = 0; // bit k: kernel id k is timed (uz_prof_enable)
    ProfSlot prof[UZ_K_COUNT];
    std::vector<ProfPending> prof_pending;
    std::vector<hipEvent_t> event_pool;
};

// A buffer of a walk slot grown without a hipFree (DevBuf::ensure_parked), to the largest request its kind has seen.  A grow site names the
// buffer once -- UZ_WGROW(w, comp, n), UZ_JGROW(J, jtask, N, carry, st) -- and the kind follows from the name (`c`: the context, in scope).
template <typename T>
inline void uz_walk_grow(uz_ctx *c, DevBuf<T> &b, WalkKind kind, size_t n, size_t used = 0, hipStream_t st = nullptr) {
    const size_t hi = c->book.note(kind, n);
    std::pair<void *, size_t> old;
    if (b.ensure_parked(n, hi, &old, used, st)) c->book.grew(old.first, old.second);
}
#define UZ_WGROW(w, name, ...) uz_walk_grow(c, (w).name, WK_##name, __VA_ARGS__)
#define UZ_JGROW(J, name, ...) uz_walk_grow(c, (J).name, JK_##name, __VA_ARGS__)

// the first slot of a handle table that is not live (a new one at its end)
template <typename V>
int new_slot(std::vector<V> &v) {
    for (size_t i = 0; i < v.size(); i++)
        if (!v[i].live) return (int)i;
    v.emplace_back();
    return (int)v.size() - 1;
}

// profiling helpers (abi.hip)
void uz_prof_begin(uz_ctx *c, int kernel, hipEvent_t *a, hipEvent_t *b);
void uz_prof_end(uz_ctx *c, int kernel, hipEvent_t a, hipEvent_t b);
void uz_prof_drain(uz_ctx *c);

struct ProfScope {
    uz_ctx *c;
    int k;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(uz_ctx *c_, int k_) : c(c_), k(k_) { uz_prof_begin(c, k, &a, &b); }
    ~ProfScope() { uz_prof_end(c, k, a, b); }
};

// device block pool (abi.hip)
DevBlock uz_block_get(uz_ctx *c, size_t bytes);
void uz_block_put(uz_ctx *c, DevBlock b);

// Small transfers on the COMPUTE path go through a copy kernel, one side in pinned host memory, never through
// hipMemcpyAsync: the DMA engine is in order, and a 2 KB result copy queued behind gigabytes of staged uploads would hold
// the kernels of the current table back until every later table has landed (measured: copies and kernels did not
// overlap at all).  dst / src: device memory or pinned host memory.
void uz_kcopy(uz_ctx *c, void *dst, const void *src, size_t bytes);
// up to UZ_KCOPY_SEGS such transfers by ONE launch (blockIdx.y picks the segment; empty segments are skipped): the small pieces a stage
// hands back together -- every launch on the compute stream stands in stream order between one chunk's read stage and the next
#define UZ_KCOPY_SEGS 4
struct KCopySeg { void *dst; const void *src; size_t bytes; };
void uz_kcopy_many(uz_ctx *c, const KCopySeg *segs, int n_segs);
// off[k] = sum of len[i] + add over i < k, off[n] the total, on stream `st`: one workgroup, a tile of 1024 lengths per round (a call's rows, a
// chunk's records or blocks: some ten thousand at most)
void uz_len_scan(uz_ctx *c, hipStream_t st, int64_t n, const uint32_t *len, uint32_t add, int64_t *off);
// waits for an asynchronous upload and builds its headers, on the compute stream (no-op for a table that is ready)
void uz_reads_make_ready(uz_ctx *c, ReadsDev &r);
// uz_reads_make_ready, and the table's quality plane brought to the threshold of the parameters.  The plane holds ONE threshold: a table that
// kept its full qualities is re-thresholded, one decoded for a threshold refuses another (UZ_E_STATE; `what` names the table in the message)
void uz_reads_ready_for_threshold(uz_ctx *c, ReadsDev &r, const char *what);
// hflags[0], the consistency flag of the header builds whose commands have run: read and cleared; set -> UzError (UZ_E_RANGE, what the code says)
void uz_check_upload_flag(uz_ctx *c);
// stage launchers
// offsets (prefix sums of n_cigar / row units), RecA / RecB / fm and the coarse index, on stream `st`;
// off_scratch: >= uz_rec_scratch_bytes(n) bytes of device memory
size_t uz_rec_scratch_bytes(int64_t n);
void uz_build_records(uz_ctx *c, hipStream_t st, ReadsDev &r, const RecColumns &col, void *off_scratch);
// ASCII upload: CIGAR words gathered back to back, bases packed to 4 bits (sets hflags[0] on a character outside the alphabet)
void uz_pack_ascii_rows(uz_ctx *c, hipStream_t st, ReadsDev &r, const uint32_t *cigar_in, const uint32_t *cigar_off_in,
                        const uint8_t *seq_in, const uint32_t *sq_off16_in, uint32_t *cigar_out, uint8_t *seq4_out);
void uz_build_qlow(uz_ctx *c, hipStream_t st, ReadsDev &r, int min_base_qual);
// appends table `src` to the merged table `dst` at the given bases (records, CIGAR words, row units, query names)
void uz_concat_table(uz_ctx *c, hipStream_t st, ReadsDev &dst, const ReadsDev &src, int64_t rec_base, int64_t cigar_base, int64_t unit_base,
                     int64_t seq_base, uint32_t qname_base);
void uz_finish_table(uz_ctx *c, hipStream_t st, ReadsDev &r); // coarse index of a table whose headers are in place
void uz_family_widen(uz_ctx *c, FamilyDev &f, int64_t n_sites); // eight-bit link columns -> the 16-bit ones, on the compute stream (once)
// compact site columns -> the plain ones, and -- f not null -- the family's first-use work in the same launch (widen, complex bit into gt)
void uz_sites_expand(uz_ctx *c, SitesDev &s, FamilyDev *f);
// n trios of a sample table: packed genotype bytes (complex bit folded in) and the members' depths at the table's wide sites, one launch each;
// trio: [3 n] sample indices on the device; gt_out / wide_out: trio t at t * gt_stride bytes / t * 6 * n_wide values
void uz_launch_family_pack(uz_ctx *c, const SamplesDev &sm, const SitesDev &s, int32_t n, const int32_t *trio, uint8_t *gt_out, size_t gt_stride, int32_t *wide_out);
// the sample cells of a text VCF parsed into the rows of `m` (k_vcf.hip): chunks of at most chunk_bytes of text, cut at line ends; -> the records
// handed back to the host, ascending.  uz_launch_vcf_settle: their cells ([n_rows][n], device memory) over the rows
void uz_vcf_parse_text(uz_ctx *c, const uz_vcf_text_view *t, int32_t n_pick, const int32_t *pick, SamplesDev &m, size_t chunk_bytes, std::vector<int64_t> &unsettled);
// the same from a BCF's value arrays (k_bcf.hip): chunks of at most chunk_bytes of gathered values, cut at record boundaries
void uz_vcf_parse_bcf(uz_ctx *c, const uz_vcf_bcf_view *t, int32_t n_pick, const int32_t *pick, SamplesDev &m, size_t chunk_bytes, std::vector<int64_t> &unsettled);
void uz_launch_vcf_settle(uz_ctx *c, int64_t n, int32_t n_rows, const int64_t *site, const uint8_t *gt_in, const uint16_t *rd_in, const uint16_t *ad_in,
                          const uint16_t *gq_in, SamplesDev &m);
void uz_launch_site_scan(uz_ctx *c, FamilyDev &f, const SitesDev &s, bool with_cnv);
void uz_launch_site_scan_many(uz_ctx *c, FamilyDev *const *fams, int n_fam, const SitesDev &s, bool with_cnv);
// the caller's block of a uz_find_answer (find_answer.hpp); code / need: what became of it (UZ_FA_*), the block this batch needs
// a find call's scope: only launches made inside one count for uz_find_stats (uz_kcopy / uz_kcopy_many serve every stage)
struct FindCount {
    uz_ctx *c;
    explicit FindCount(uz_ctx *c_) : c(c_) { c->find_counting = true; }
    ~FindCount() { c->find_counting = false; }
};
inline void uz_find_launched(uz_ctx *c, int k) { if (c->find_counting) c->find_stat[1] += k; }
inline void uz_find_waited(uz_ctx *c) { if (c->find_counting) c->find_stat[0]++; }
struct FindAnswer { uint8_t *block; size_t bytes; int code; uint64_t need; };
void uz_launch_find(uz_ctx *c, FamilyDev &f, const SitesDev &s, int mode, bool host_offsets = true, FindAnswer *ans = nullptr);
// the lists the context holds (a find's, or recalled) written into the block by one kernel, one wait: false -- the block is too small
bool uz_launch_find_answer(uz_ctx *c, FindAnswer *ans, int64_t room_c, int64_t room_h);
void uz_stage_dnms(uz_ctx *c, const uz_dnms_view *d);
void uz_launch_cnv(uz_ctx *c, const SitesDev &s, const int32_t *rb_counts_dev, int32_t *cnv_counts, int32_t *cnv_pos, int32_t *origin,
                   int32_t *evidence, int32_t *etype);
void uz_launch_cnv_dense(uz_ctx *c, const int32_t *cnv_counts, const int32_t *cnv_pos, int64_t *cnv_off, int32_t *dense);
void uz_launch_phase(uz_ctx *c, FamilyDev &f, const SitesDev &s, ReadsDev &r, int32_t *status, int32_t *counts,
                     int32_t *origin, int32_t *evidence, bool defer = false);
bool uz_finish_phase(uz_ctx *c, int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence);
// BGZF blocks inflated on the device (k_inflate.hip): device pointers; comp padded by UZ_BGZF_PAD, comp_bytes_padded: uz_bgzf_padded (bgzf_batch.hpp);
// cursor_and_err: two int32 of device memory
void uz_launch_inflate(uz_ctx *c, hipStream_t st, int64_t n_blocks, const uint8_t *comp, int64_t comp_bytes_padded, const int64_t *in_off,
                       const int64_t *out_off, uint8_t *out, int32_t *cursor_and_err);
// A batch of gathered BGZF blocks queued for the device (k_inflate.hip; bgzf_batch.hpp states the rules): the pad behind d_comp cleared and the
// tables sent on st[0], st[1] made to wait for them, then slice i of `cut` on st[i & 1] -- its bytes up, `before`, one uz_launch_inflate that
// leaves its flag words at d_flags + 2 i, `after`.  Nothing is waited for.  The routine owns no memory and touches nothing of the context but
// what it is handed: the caller has grown the buffers (d_comp: uz_bgzf_room(comp_bytes)), and brings the streams and the event.
struct InflateBatch {
    const uint8_t *comp; int64_t comp_bytes, n_blocks; const int64_t *in_off, *out_off; // the host's: tables that passed uz_bgzf_check_tables
    uint8_t *d_comp; int64_t *d_in, *d_off; uint8_t *d_out; int32_t *d_flags;           // the device's
    hipStream_t st[2]; hipEvent_t ev; // st[1] (and ev) null: everything on st[0]
    bool tables_there = false;        // d_in and d_off have been queued on st[0] by the caller
    std::function<void(size_t, hipStream_t)> before, after; // (slice, its stream), around the slice's launch; empty: nothing
};
void uz_queue_inflate(uz_ctx *c, const InflateBatch &b, const std::vector<int64_t> &cut);
// the record walk on the device (k_bamwalk.hip): every pointer device memory; fill = false: counts + offsets (count, first, walked, flags), fill = true: the descriptors
void uz_launch_bam_walk(uz_ctx *c, hipStream_t st, int n_tasks, const uint8_t *buf, const int64_t *blk_at, const int64_t *blk_coff, const int32_t *task,
                        const int64_t *span, const int32_t *reach, const int32_t *fetch, int64_t *count, const int64_t *first, int64_t *walked, int32_t *flags,
                        uz_walk_desc *out, int64_t *n_direct, int64_t *tab_first, const uz_walk_file *tfile = nullptr);
void uz_launch_desc_filter(uz_ctx *c, hipStream_t st, bool fill, int n_tasks, const uz_walk_desc *in, const int64_t *first, const int64_t *count,
                           const int32_t *task, const int64_t *tab_first, unsigned long long *tab, int64_t *kcount, int64_t *kfirst, uz_walk_desc *out);
size_t uz_bam_walk_pad(); // bytes the inflated buffer must be padded by (the walk's LDS windows read past the last record)
// the batch-wide joins on the device (k_bamjoin.hip).  Totals of a finished join (WalkSlot::Join::tot_h):
enum { JT_N = 0, JT_QNAMES = 1, JT_CIGAR = 2, JT_UNITS = 3, JT_SEQ_UNITS = 4, JT_NAME_BYTES = 5, JT_ERR = 6, JT_COUNT = 8 };
struct JoinPlanHost { // what the host knows when it starts the joins of a walked batch
    int32_t n_host = 0, n_ref = 0;
    const int32_t *h_flags = nullptr; // [n_host]: the tasks the host walked itself (their device descriptors are void)
    bool all_bases = false;
};
// first call: fills the filtered descriptors, sets the tables up.  Every call: appends what the host walked since the last one (x [n_x], aux bytes),
// sets the answers to the last call's needs (need_jtask [n_need of the last call]) and runs the closure until it needs the host again (-> n_need > 0:
// uz_join_needs) or is finished (n_need == 0: the kept list, its offsets and totals are in place)
void uz_join_run(uz_ctx *c, uz_ctx::WalkSlot &w, const JoinPlanHost &P, const uz_walk_desc *x, int64_t n_x, const uint8_t *xaux, int64_t xaux_bytes,
                 const int32_t *look_tid, int64_t n_look, const int32_t *need_jtask);
void uz_join_needs(uz_ctx *c, uz_ctx::WalkSlot &w, uz_need_rec *out);
// debug / parity: the kept records of a finished join in output order
void uz_join_fetch(uz_ctx *c, uz_ctx::WalkSlot &w, uint64_t *voff, uint32_t *qname, int32_t *mate, uint8_t *bases, uz_kept_rec *kept);
// the read names of name ids (a table built by uz_reads_from_walk with names): lengths, then bytes
void uz_launch_reads_files(uz_ctx *c, hipStream_t st, int32_t n_files, const void *rec_b, const int64_t *rec_first, uint32_t *mn, uint32_t *mx);
void uz_launch_name_lens(uz_ctx *c, hipStream_t st, int64_t n_ids, const uint32_t *ids, const uint32_t *name_rec, const uz_kept_rec *kept, int64_t n_recs, int64_t names_bytes,
                         uint32_t *len);
void uz_launch_name_gather(uz_ctx *c, hipStream_t st, int64_t n_ids, const uint32_t *ids, const uint32_t *name_rec, const uz_kept_rec *kept, const uint8_t *names,
                           const uint32_t *len, const uint32_t *off, uint8_t *out);
void uz_scan_u32(uz_ctx *c, hipStream_t st, const uint32_t *in, uint32_t *out, int64_t n, uz_ctx::WalkSlot::Join &J); // exclusive sum (scratch: J.tmp)
void uz_launch_bam_extract(uz_ctx *c, hipStream_t st, int64_t n, const uint8_t *buf, int64_t buf_bytes, const uint8_t *aux, int64_t aux_bytes, const uz_kept_rec *kept,
                           int thr, int32_t *start, int32_t *tlen, int32_t *mate, uint32_t *qname, uint16_t *flag, uint16_t *l_seq, uint16_t *n_cigar, uint8_t *mapq,
                           uint8_t *aux_col, uint32_t *cigar, uint8_t *seq4, uint32_t *plane, int32_t *err, uint8_t *names, int64_t n_cigar_total, int64_t n_row_units,
                           int64_t n_seq_units, int64_t names_bytes);
// CRC-32 of inflated blocks against their BGZF footers (k_inflate.hip): device pointers; *err: 0, or 1 + a block whose checksum differs
void uz_launch_crc32(uz_ctx *c, hipStream_t st, int64_t n_blocks, const uint8_t *out, const int64_t *out_off, const uint32_t *want, int32_t *err);
int uz_phase_votes_impl(uz_ctx *c, int64_t *vote_off, int32_t *vote_val);
int uz_phase_groups_impl(uz_ctx *c, int64_t *grp_off, int32_t *grp_q);
int uz_phase_sizing_fetch_impl(uz_ctx *c, int32_t *bounds, int32_t *pre_win, int32_t *pre_ha, int32_t *pre_hl, int64_t *reduced);
void uz_phase_state_free(uz_ctx *c);
// where the finished batch's per-DNM results and lists lie on the device (k_reads.hip): status [n], counts [4 n]; pool / list_start / list_len are
// null when the batch kept no lists.  UZ_E_STATE: no finished batch
void uz_phase_lists_dev(uz_ctx *c, int32_t *n, const int32_t **status, const int32_t **counts, const int32_t **pool, const long long **list_start,
                        const int32_t **list_len);
// BED rows as text (k_bed.hip; bed_row.hpp is the body): uz_bed_rows over the last batch, uz_bed_rows_lists over the caller's lists
int uz_bed_rows_impl(uz_ctx *c, const uz_bed_view *rows, int verbose, int include_ambiguous, int64_t *off, const uint8_t **bytes);
int uz_bed_rows_lists_impl(uz_ctx *c, const uz_bed_view *rows, int verbose, int include_ambiguous, int32_t n_dnms, const int32_t *status, const int64_t *list_off,
                           const int32_t *list_val, uint32_t n_qnames, const uint32_t *name_off, const uint8_t *name_bytes, int32_t ratio, int64_t *off,
                           const uint8_t **bytes);
// the annotated VCF's record lines as text (k_vcfout.hip; vcf_row.hpp is the body)
int uz_vcf_rows_impl(uz_ctx *c, const uz_vcf_text_view *text, const int64_t *line_at, const int64_t *ann_off, const int32_t *ann_col, const uint8_t *ann_gt,
                     const int32_t *ann_uops, const int8_t *ann_uet, int64_t *off, const uint8_t **bytes, uint8_t *handed_back);
// the blocks of a host buffer inflated and checked (k_inflate.hip), the heads of a cohort's alignment files (k_bamhead.hip)
void uz_bgzf_inflate_impl(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, uint8_t *out,
                         int repeat, double *kernel_ms);
void uz_bgzf_inflate_to_host_impl(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off,
                                 uint8_t *out);
void uz_crc32_blocks_impl(uz_ctx *c, const uint8_t *data, int64_t n_blocks, const int64_t *off, const uint32_t *want, int64_t *first_bad);
void uz_head_walk_impl(uz_ctx *c, int *head_id, int32_t n_files, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off,
                      const int32_t *isize, const uint32_t *crc, const int64_t *blk_first, const int64_t *start, const int64_t *want, const int64_t *have,
                      int64_t *taken, int64_t *cursor, int32_t *state);
void uz_head_rank_impl(uz_ctx *c, int head_id, int32_t readlen, const int64_t *k, uint32_t *a, uint32_t *b);
void uz_head_fetch_impl(uz_ctx *c, int head_id, int32_t file, int32_t *out, int64_t cap, int64_t *n);
void uz_head_free_impl(uz_ctx *c, int head_id);
// BGZF blocks of a host buffer (k_deflate.hip; deflate_body.hpp is the body)
// The index side of a deflate call (k_tbx.hip), hung into the chunk loop of uz_bgzf_deflate_impl: uz_tbx_mark before a chunk's host wait (the
// line starts of its tiles counted and scanned, the count sent down), uz_tbx_keys behind it (the chunk's rows appended to the row table; what the
// host has to settle noted), uz_tbx_tables behind the last chunk.  tbx == nullptr: uz_bgzf_deflate_coded, launch for launch.
struct TbxRow { // one line of the text
    uint64_t v0, name_off;
    int64_t beg, end;
    uint32_t name_len, kind; // kind: UZ_TBX_META .. BAD | why << 4 | same_as_prev << 8
};
struct TbxCall {
    int preset = 0;
    const uint8_t *data = nullptr;
    int64_t n_bytes = 0;
    size_t chunk_bytes = 0, n_chunks = 0;
    int64_t n_rows = 0;                               // of the chunks so far
    std::vector<std::pair<int64_t, TbxRow>> settled;  // rows the host settled: (row, what it holds)
    uz_tbx_view *view = nullptr;
};
void uz_tbx_mark(uz_ctx *c, TbxCall &t, size_t q, const uint8_t *d_in, size_t nb);
void uz_tbx_keys(uz_ctx *c, TbxCall &t, size_t q, const uint8_t *d_in, size_t nb, const int64_t *d_off, int64_t base);
void uz_tbx_tables(uz_ctx *c, TbxCall &t, int64_t eof_at);
int uz_bgzf_deflate_impl(uz_ctx *c, const uint8_t *data, int64_t n_bytes, int code, int64_t *kinds, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes,
                         int repeat, double *kernel_ms, TbxCall *tbx = nullptr);
// a BCF's records as VCF text lines (k_bcfout.hip; bcf_row.hpp is the body)
int uz_bcf_rows_impl(uz_ctx *c, const uz_bcf_lines_view *records, int64_t *off, uint64_t *samp_at, const uint8_t **bytes, uint8_t *handed_back);
