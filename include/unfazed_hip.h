/* unfazed_hip.h -- C ABI of the MI355X (gfx950) per-DNM phasing path.
 *
 * The reference (unfazed v1.0.3) has no FFI seam; the drop-in boundary is the
 * pair of Python calls its driver makes (reference unfazed/unfazed.py:601-646):
 *     phase_snvs(dnms, kids, pedigrees, sites, threads, build, ...)  snv_phaser.py:356-399
 *     phase_svs (same 20 positional parameters)                      sv_phaser.py:427-493
 * unfazed_amd/snv_phaser.py and sv_phaser.py keep those two signatures and call
 * the entry points below through ctypes (INTEGRATION.md shows the stub a
 * maintainer of the reference would add).  Each entry point names the reference
 * code it replaces.
 *
 * Conventions: every function returns 0 on success or a negative UZ_E_* code;
 * uz_last_error() gives the message.  No C++ exception, exit() or stdio crosses
 * this boundary.  All pointers are caller-owned HOST memory unless the function
 * name says `_device`.  One host thread drives one context; contexts are
 * independent (multi-GPU = one context per process/GPU, DNMs sharded by the
 * caller, no collective).
 */
#ifndef UNFAZED_HIP_H
#define UNFAZED_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "uz_types.h"
#include "uz_bamwalk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UZ_E_ARG (-1)      /* bad argument / unknown handle */
#define UZ_E_HIP (-2)      /* a HIP runtime call failed */
#define UZ_E_NODEVICE (-3) /* no gfx950 device visible */
#define UZ_E_STATE (-4)    /* call order (e.g. fetch before find) */
#define UZ_E_RANGE (-5)    /* input exceeds an index range of the device layout */

#define UZ_FIND_WHOLE_REGION 1  /* find(..., whole_region=True): CNV interior, sv_phaser.py:375-389 */
#define UZ_FIND_SECOND_WINDOW 2 /* find()'s second window around `end` (informative_site_finder.py:32-40); find_many has none */

/* kernels whose launches are timed with HIP events on the context's stream */
#define UZ_K_SITE_SCAN 0   /* K1 site classify (the roofline kernel) */
#define UZ_K_WINDOW_COUNT 1
#define UZ_K_WINDOW_FILL 2
#define UZ_K_PHASE 3       /* the per-DNM read stage (both builds of k_phase) */
#define UZ_K_SIZING 4      /* fetch-range sizing pass */
#define UZ_K_CNV 5         /* K6 allele-balance count + decision */
#define UZ_K_FAMILY_PACK 6 /* k_family_gt_pack (+ the wide-depth gather) of uz_families_from_samples */
#define UZ_K_CNV_DENSE 7   /* dense site lists of K6: scan of the 2n counts + k_cnv_dense */
#define UZ_K_VCF_TABS 8    /* k_vcf_tabs: field starts of the picked sample columns (uz_samples_from_text), one launch per chunk of text */
#define UZ_K_VCF_CELLS 9   /* k_vcf_cells: the cells parsed into the sample table's rows, one launch per chunk */
#define UZ_K_VCF_COPY 10   /* not a kernel: the chunks' host-to-device copies on the copy stream, timed beside the two kernels */
#define UZ_K_BCF_CELLS 11  /* k_bcf_cells: the values of a BCF's five FORMAT fields read into the sample table's rows (uz_samples_from_bcf), one launch per chunk */
#define UZ_K_BCF_COPY 12   /* not a kernel: the copies of that route's chunks on the copy stream */
#define UZ_K_HEAD_INFLATE 13 /* k_bgzf_inflate + k_bgzf_crc32 over the heads of a group of files (uz_head_walk) */
#define UZ_K_HEAD_WALK 14    /* k_head_walk */
#define UZ_K_HEAD_RANK 15    /* k_head_rank */
#define UZ_K_BED_SIZE 16    /* k_bed_size + the scan of the rows' lengths (uz_bed_rows) */
#define UZ_K_BED_FILL 17    /* k_bed_fill */
#define UZ_K_VCFOUT_SIZE 18 /* k_vcfout_size + the scan of the records' lengths (uz_vcf_rows), one launch per chunk of text */
#define UZ_K_VCFOUT_FILL 19 /* k_vcfout_fill */
#define UZ_K_BCFOUT_SIZE 20 /* k_bcfout_size + the scan of the records' lengths (uz_bcf_rows), one launch per chunk of records */
#define UZ_K_BCFOUT_FILL 21 /* k_bcfout_fill */
#define UZ_K_DEFLATE 22       /* k_bgzf_deflate + k_bgzf_crc32_out + the scan of the blocks' sizes (uz_bgzf_deflate), one launch per chunk of input */
#define UZ_K_DEFLATE_FRAME 23 /* k_bgzf_frame */
#define UZ_K_TBX_KEYS 24      /* k_tbx_mark + the scan of the tiles' line starts + k_tbx_starts + k_tbx_keys (uz_bgzf_deflate_indexed), per chunk of input */
#define UZ_K_TBX_TABLE 25     /* the passes over all rows behind the last chunk: k_tbx_flags, two scans, k_tbx_emit, k_tbx_nintv, k_tbx_linear, k_tbx_fill */
#define UZ_K_COUNT 26

typedef struct uz_ctx uz_ctx;

/* ---- context ---------------------------------------------------------- */
int uz_create(int device, uz_ctx **out);
void uz_destroy(uz_ctx *ctx);
const char *uz_last_error(const uz_ctx *ctx);
int uz_sync(uz_ctx *ctx);
/* thresholds: replaces the module globals the reference sets per call
 * (informative_site_finder.py:187-204, read_collector.py:361-370) */
int uz_set_params(uz_ctx *ctx, const uz_params *p);

/* ---- staging ---------------------------------------------------------- */
/* Sites file columns -> HBM.  Replaces cyvcf2.VCF(...) + per-DNM tabix queries
 * (informative_site_finder.py:213, :42; find_many :558-568). */
int uz_sites_upload(uz_ctx *ctx, const uz_sites_view *sites, int *sites_id);
/* Genotype columns of one trio -> HBM (gt_types / gt_ref_depths / gt_alt_depths /
 * gt_quals of informative_site_finder.py:257-260). */
int uz_family_upload(uz_ctx *ctx, int sites_id, const uz_family_view *fam, int *fam_id);
/* Both at once, asynchronously: the copies are queued on the library's copy stream (behind whatever uz_reads_upload_packed
 * queued before) and the call returns; the first call that uses the family or the sites makes the compute stream wait for
 * them.  The host arrays (pinned memory for link speed, uz_pinned_alloc) must stay untouched until such a call has returned.
 * This is how a batch is streamed in sub-batches: the site stage of sub-batch k + 1 rides the link between the record
 * tables of sub-batches k - 1 and k instead of stopping it. */
int uz_sites_family_upload_async(uz_ctx *ctx, const uz_sites_view *sites, const uz_family_view *fam, int *sites_id, int *fam_id);
/* Cohort form of the genotype columns (one multi-sample sites VCF, many trios, README.md:208): the columns of every sample
 * named by a batch's trios -> HBM ONCE, sample-major (uz_samples_view), and the trios made from them on the device.  Replaces the same
 * gt_types / gt_ref_depths / gt_alt_depths / gt_quals reads (informative_site_finder.py:257-260) and the per-family `vcf(region)` loop
 * around them (:42, :213, :558-568), which hands every sample's genotypes out again for every family it belongs to.
 * uz_samples_upload: one pooled block; the copies are queued on the copy stream (pinned host memory for link speed, uz_pinned_alloc)
 * and the call returns -- the host arrays must stay untouched until a uz_families_from_samples on the table has returned, which
 * makes the compute stream wait for the copies' event. */
int uz_samples_upload(uz_ctx *ctx, int sites_id, const uz_samples_view *samples, int *samples_id);
/* n trios of a sample table in ONE launch sequence: kid / dad / mom [n] are sample indices of the table.  A family's nine 16-bit
 * columns ARE the three samples' rows (no copy); it owns its packed genotype byte -- kid | dad << 2 | mom << 4 with the site's complex
 * flag already in bit 6 (k_family_gt_pack) -- its class bytes and the 32-bit depths of its three members at the table's wide sites.
 * The families are those of uz_family_upload to every later call (uz_site_scan*, uz_find, uz_phase*, uz_phase_cnv) and live until
 * uz_sites_free.  UZ_E_ARG: an index outside [0, n_samples), n < 0, a samples_id that names no live table of this context. */
int uz_families_from_samples(uz_ctx *ctx, int samples_id, int32_t n, const int32_t *kid, const int32_t *dad, const int32_t *mom, int *fam_ids /* [n] */);
/* Any family's device columns back on the host, whatever route made it: gt [S] (complex bit included), cols [9][S] = ref depth of
 * kid, dad, mom, alt depth of the three, GQ of the three.  For parity tests of the two routes. */
int uz_family_fetch(uz_ctx *ctx, int fam_id, uint8_t *gt, uint16_t *cols /* [9][S] */);
/* Any sites table's four device columns back on the host, S entries each: a table staged in the compact form (uz_sites_view.pos_d16 ...) is
 * expanded first if nothing has used it yet -- without its family, whose own first use then readies it.  For tests that hold the
 * expansion to the form's description; nothing on the product path calls it. */
int uz_sites_fetch(uz_ctx *ctx, int sites_id, int32_t *pos, uint8_t *sflags, uint8_t *ref_base, uint8_t *alt_base);
/* The same sample table WITHOUT the host parsing a sample cell: the record text of a lazily decoded text VCF (unfazed_io.h:
 * uz_vcf_decode_regions_lazy, uz_vcf_samples_text) goes up in bounded chunks cut at line ends -- chunk k + 1 copied while chunk k is parsed
 * -- and two kernels (csrc/k_vcf.hip) read GT, AD (or RO / AO) and GQ of the picked sample columns into rows [n_pick][S] of the layout
 * above.  Replaces gt_types / gt_ref_depths / gt_alt_depths / gt_quals of every sample at every record (informative_site_finder.py:257-260)
 * behind `vcf(region)` (:42, :213).  pick[r]: the file's sample column of row r, in any order.  text->n_records must equal the sites table's S.
 * The device settles only a plain grammar (csrc/vcf_cell.hpp); a record with any picked cell outside it -- or beyond a limit of the
 * kernels' formats: a FORMAT slot above 127, a sample region of 4 GiB -- is handed back: *n_unsettled of them, listed by
 * uz_samples_unsettled (site indices, ascending).  While there are any, the table answers uz_families_from_samples with UZ_E_STATE.
 * uz_samples_settle takes exactly those sites, in that order, and their cells as a sample table of n sites -- uz_samples_pack of
 * uz_vcf_record_samples: the host's own reader -- overwrites the rows there and builds the table's wide list from cells' wide list (whose
 * wide_site indexes the n sites).  A table with no unsettled site is ready at once (and has no wide site: a depth above 32767 is never
 * settled on the device).  The call returns when the rows are in place; the text may be freed then.
 * Chunks are 32 MiB of text; the environment variable UZ_VCF_CHUNK_BYTES, read per call, sets another size (a line longer than a
 * chunk gets a chunk of its own). */
int uz_samples_from_text(uz_ctx *ctx, int sites_id, const uz_vcf_text_view *text, int32_t n_pick, const int32_t *pick, int *samples_id, int64_t *n_unsettled);
/* The same from a BCF (unfazed_io.h: uz_vcf_decode_regions_lazy on a .bcf + .csi, uz_vcf_samples_bcf; informative_site_finder.py:41-43, :213):
 * a FORMAT field's values lie at a fixed stride per sample, so there is nothing to find -- only the value arrays of GT, AD, RO, AO and GQ go
 * up, gathered back to back (each on a 4-byte boundary) with five 32-bit offsets and five descriptors per record, in chunks cut at record
 * boundaries and bounded by UZ_VCF_CHUNK_BYTES (of gathered bytes; a record beyond it gets a chunk of its own), double buffered like the text's.
 * One kernel per chunk (csrc/k_bcf.hip: k_bcf_cells, the body of csrc/bcf_cell.hpp) writes the rows of the same table: same stride, same block,
 * the same uz_samples_unsettled / uz_samples_settle round trip and UZ_E_STATE until settled.  Handed back: a record with a picked cell whose
 * depth lies above 32767 or below 0, a record with one of the five fields in a type other than int8 / int16 / int32 (float for GQ), a record
 * whose five arrays exceed 4 GiB. */
int uz_samples_from_bcf(uz_ctx *ctx, int sites_id, const uz_vcf_bcf_view *bcf, int32_t n_pick, const int32_t *pick, int *samples_id, int64_t *n_unsettled);
int uz_samples_unsettled(uz_ctx *ctx, int samples_id, int64_t *site /* [n_unsettled] */);
int uz_samples_settle(uz_ctx *ctx, int samples_id, int64_t n, const int64_t *site, const uz_samples_view *cells);
/* A table is kept alive by the families made from it: UZ_E_STATE while one exists.  uz_sites_free frees a sites table's families
 * and then its sample tables. */
int uz_samples_free(uz_ctx *ctx, int samples_id);
/* Alignment records of one BAM -> HBM.  Replaces pysam.AlignmentFile + fetch +
 * mate (read_collector.py:372-385, :400, :167, :185).  Whatever form a table arrives in, HBM holds the packed
 * one (uz_reads_packed_view in uz_types.h).
 * uz_reads_upload: the ASCII form (bases as characters, one quality byte per base); the rows are packed on the
 * device and the qualities are kept, so the table serves any --min-gt-qual.  Returns when the copy is done. */
int uz_reads_upload(uz_ctx *ctx, const uz_reads_view *reads, int *reads_id);
/* uz_reads_upload_packed: the staged form a decoder emits directly (4-bit bases, the quality-below-threshold
 * plane, no offset columns) -- 2.8x fewer bytes over the host link.  ASYNCHRONOUS: the copies are queued on the
 * context's copy stream, the header build behind them on a stream of its own (neither the next table's copies
 * nor the kernels of the table before wait for it), and the call returns; the host buffers (pinned memory for
 * full link speed, uz_pinned_alloc) must stay untouched until uz_reads_wait or a uz_phase on the table has
 * returned.  uz_phase on the table waits for the build on the device, so the upload and the build of the next
 * table overlap the kernels of the current one.
 * The quality bits of listed bases (uz_reads_packed_view.bl_qlow, (n_bl + 7) / 8 bytes) travel with the other link columns; the column is
 * taken only with bl_pos / bl_code and the counts through the dictionary (tup_n_bl) -- UZ_E_ARG without them, with bl_n, or beside the quality
 * plane -- and a record whose set bits are not the number its count names fails the table (UZ_E_RANGE when the build has run). */
int uz_reads_upload_packed(uz_ctx *ctx, const uz_reads_packed_view *reads, int *reads_id);
int uz_reads_wait(uz_ctx *ctx, int reads_id);
/* what the device made of a table's fixed-width columns, whatever form they travelled in (plain, 16- / 8-bit differences, the pair
 * form; `end` derived from the CIGAR when it was left out): [n_segs] each, any pointer may be NULL.  For parity tests of the
 * upload forms; waits for the table like uz_reads_wait. */
int uz_reads_headers(uz_ctx *ctx, int reads_id, int32_t *start, int32_t *end, int32_t *tlen, int32_t *mate, uint32_t *qname);
/* parity / debug, like uz_reads_headers: the other columns of a table as the device holds them.  sizes [4] out: records, CIGAR words, base-row
 * units (16 bytes: 32 four-bit codes), quality-plane units (one 32-bit word: bit b = "base b of the unit lies below the table's threshold").  Every
 * other pointer may be NULL (call it once for the sizes): fm [n] = flag | mapq << 16 | aux << 24; l_seq, n_cigar, cigar_off (first word in the
 * CIGAR store), sq_off (first unit of the base row), qoff (first unit of the quality-plane row) [n]; cigar [sizes[1]]; seq4 [16 sizes[2]];
 * qlow [sizes[3]].  Nothing on the product path calls it. */
int uz_reads_columns(uz_ctx *ctx, int reads_id, int64_t sizes[4], uint32_t *fm, uint16_t *l_seq, uint16_t *n_cigar, uint32_t *cigar_off, uint32_t *sq_off,
                     uint32_t *qoff, uint32_t *cigar, uint8_t *seq4, uint32_t *qlow);
/* parity / debug, beside uz_reads_columns: the two per-record columns it leaves out, as the device holds them.  umask [n]: the staged 32-base units of
 * every record's rows (UZ_UMASK_ALL: every unit; UZ_UMASK_LISTED set when the record's bases came as a list); nlow [n]: the low-quality count that
 * travelled, saturated at 255.  Either pointer may be NULL.  Nothing on the product path calls it. */
int uz_reads_marks(uz_ctx *ctx, int reads_id, uint16_t *umask, uint8_t *nlow);
/* BGZF blocks inflated on the device (csrc/k_inflate.hip: one wavefront per block; fixed, dynamic and stored DEFLATE blocks).  This
 * entry is the measured form (repeat / kernel_ms) behind the parity tests; the session's path calls uz_bgzf_inflate_to_host below for
 * every staged batch (HipEngine.upload_reads_staged).  comp: the compressed bytes (host); in_off[k]: where the DEFLATE stream
 * of block k starts in them (behind its gzip header and BC field); out_off[k] .. out_off[k+1]: where its ISIZE bytes go in `out`
 * (host, [out_off[n_blocks]]).  repeat > 0: the kernel is run that many more times and *kernel_ms is their mean duration (HIP events).
 * A stream that does not decode to exactly its declared size fails the call (UZ_E_RANGE, the block named). */
int uz_bgzf_inflate(uz_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off,
                    uint8_t *out, int repeat, double *kernel_ms);
/* The working form: the same kernel on buffers the context keeps from call to call and on a stream of its own; comp and out in pinned
 * host memory for full link speed (uz_pinned_alloc).  This is what io_native.BamSource.select(inflate=...) calls between
 * uz_bam_stage_begin and uz_bam_stage_finish (unfazed_io.h): the blocks a batch's walk will read are gathered, inflated here, and handed
 * back; the host then copies records out of them instead of inflating (and still holds every block against its CRC-32). */
int uz_bgzf_inflate_to_host(uz_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off,
                            uint8_t *out);
/* ---- The record walk on the device (uz_bamwalk.h; the host half is uz_stage_walk_plan / uz_bam_stage_finish_desc / uz_stage_kept in unfazed_io.h).
 * What it replaces: `bamfile.fetch(chrom, lo, hi)` walking the records of a window (read_collector.py:385, :167) -- on the host until round 4, with
 * the inflated blocks crossing the link twice.
 * uz_bam_walk: the gathered BGZF blocks of a batch (uz_stage_gather_blocks: comp / in_off / out_off, blk_coff from uz_stage_walk_plan) go up, are
 * inflated in HBM and stay there; one wavefront per task of the plan walks them (every record inside a reach interval becomes a descriptor in HBM), and the
 * descriptors the batch-wide joins can need -- the records a fetch returns and those that share a name with one of them -- are counted.
 * -> *n_desc descriptors wait, *walk_id names the batch (four may be in flight).  Callable from a decoder's worker thread.
 * uz_bam_walk_fetch: those descriptors, task by task in file order: desc [n_desc], d_first [n_tasks + 1], d_flags / d_walked
 * [n_tasks] (UZ_WALK_TASK_*: a flagged task owns no descriptors -- the host walks it).
 * uz_reads_from_bam: the table of the kept records (uz_stage_kept), unpacked on the device from the bytes the walk left in HBM (and the aux bytes
 * of records only the host has seen) and built like an adopted table (uz_reads_adopt_device); releases the batch.  Owner's thread only.
 * uz_bam_walk_release: gives a walked batch up without building its table. */
int uz_bam_walk(uz_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, const int64_t *blk_coff,
                const uint32_t *blk_crc /* [n_blocks] the CRC-32 of every block's footer: held against the inflated bytes (k_bgzf_crc32); NULL: not checked */,
                int32_t n_tasks, const int32_t *task, int64_t n_spans, const int64_t *span, int64_t n_reach, const int32_t *reach, int64_t n_fetch,
                const int32_t *fetch, int *walk_id, int64_t *n_desc);
/* ---- The insert cutoff's input on the device: the template lengths of a file's first records and two order statistics of |tlen - 2 readlen|
 * (read_collector.py:11-25: estimate_concordant_insert_len reads the first insert_size_max_sample + 1 records of the alignment file and takes the
 * 99.5th percentile; the percentile's float arithmetic stays on the host, hostpath.cutoff_from_ranks).  Owner's thread only.
 * uz_head_walk (read_collector.py:11-25: the loop over the file's first records): the heads of n_files files, in rounds.  *head_id = -1 opens a
 *   head -- tlen columns of want[f] records per file -- and names it; a later call with that id appends to the same columns (its n_files and
 *   want are the first call's, have[f] what the calls so far have taken).  comp (page-locked host memory is fastest): the compressed bytes of
 *   this call's blocks; in_off[k]: where block k's DEFLATE stream starts in comp; isize[k]: its inflated size (<= 64 KiB); crc[k]: its footer's
 *   CRC-32; blk_first [n_files + 1]: file f's blocks are [blk_first[f], blk_first[f + 1]) -- consecutive blocks of the file, none for a file
 *   this call does not walk; start[f]: the first record's offset in the file's inflated bytes of this call.  The blocks are inflated in HBM,
 *   every block is held against its CRC-32, and k_head_walk (one wavefront per file) writes the records' tlen behind the have[f] it holds.
 *   -> per file: taken (records of this call), cursor (offset, in this call's inflated bytes of the file, of the first record not taken),
 *   state: UZ_HEAD_DONE (have + taken = want), UZ_HEAD_END (the bytes ended at a record boundary or inside a record: a record is taken only
 *   when its 4 + block_size bytes lie wholly inside the bytes given), UZ_HEAD_BAD (a block_size below 32, a block that does not inflate to its
 *   size, a CRC-32 mismatch: the FILE is bad, not the call), UZ_HEAD_NONE (no block of the file in this call).
 * uz_head_rank (read_collector.py:11-25: `np.percentile(insert_sizes, 99.5)` over abs(tlen - 2 readlen)): per file the keys |tlen - 2 readlen| at
 *   ranks k[f] and min(k[f] + 1, n - 1) of their ascending order, n = the records the file's column holds (k_head_rank: an exact radix select;
 *   64-bit arithmetic, 0 <= readlen < 2^30).  k[f] < 0: the file is skipped (a / b = 0).  k[f] >= n: UZ_E_ARG.
 * uz_head_fetch (read_collector.py:11-25, for the parity tests): file f's column, out [cap] -> *n records.
 * uz_head_free: gives the head's columns up. */
#define UZ_HEAD_NONE 0
#define UZ_HEAD_DONE 1
#define UZ_HEAD_END 2
#define UZ_HEAD_BAD 3
int uz_head_walk(uz_ctx *ctx, int *head_id, int32_t n_files, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off,
                 const int32_t *isize, const uint32_t *crc, const int64_t *blk_first, const int64_t *start, const int64_t *want, const int64_t *have,
                 int64_t *taken, int64_t *cursor, int32_t *state);
int uz_head_rank(uz_ctx *ctx, int head_id, int32_t readlen, const int64_t *k, uint32_t *a, uint32_t *b);
int uz_head_fetch(uz_ctx *ctx, int head_id, int32_t file, int32_t *out, int64_t cap, int64_t *n);
int uz_head_free(uz_ctx *ctx, int head_id);
/* k_bgzf_crc32 alone (the parity tests hold it against zlib): blocks data[off[k] .. off[k + 1]) of at most 64 KiB (host memory), want[k] their CRC-32;
 * *first_bad = -1, or a block whose checksum differs */
int uz_crc32_blocks(uz_ctx *ctx, const uint8_t *data, int64_t n_blocks, const int64_t *off, const uint32_t *want, int64_t *first_bad);
/* uz_bam_walk over the blocks of MANY files presented as one (unfazed_io.h: uz_bamsrc_open_many -- blk_coff, the spans and the tasks' references are
 * the set's).  file_base / ref_base [n_files + 1], salt1 / salt2 [n_files]: uz_bamsrc_files.  A task's file is the one its first block lies in; the
 * walk adds the file's ref_base to refID / next_refID of its records and mixes the salts into h1 / h2 (uz_bamwalk.h: uz_walk_file), so that the joins,
 * uz_reads_from_walk and uz_reads_names see one file.  Refused when a task's reference is not one of its file's. */
int uz_bam_walk_many(uz_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, const int64_t *blk_coff,
                     const uint32_t *blk_crc, int32_t n_tasks, const int32_t *task, int64_t n_spans, const int64_t *span, int64_t n_reach, const int32_t *reach,
                     int64_t n_fetch, const int32_t *fetch, int32_t n_files, const int64_t *file_base, const int32_t *ref_base, const uint64_t *salt1,
                     const uint32_t *salt2, int *walk_id, int64_t *n_desc);
/* A table built from such a batch (uz_reads_from_walk / uz_reads_from_bam): per file its first record and its first name id -- rec_first /
 * name_first [n_files + 1], from ref_base [n_files + 1].  A file's names must be one range of ids, the ranges in file order: UZ_E_STATE otherwise. */
int uz_reads_files(uz_ctx *ctx, int reads_id, int32_t n_files, const int32_t *ref_base, int64_t *rec_first, int64_t *name_first);
int uz_bam_walk_fetch(uz_ctx *ctx, int walk_id, uz_walk_desc *desc, int64_t *d_first, int32_t *d_flags, int64_t *d_walked);
int uz_bam_walk_release(uz_ctx *ctx, int walk_id);
/* ---- The batch-wide joins of a walked batch ON THE DEVICE (csrc/k_bamjoin.hip): mate() for every fetched record and every mate of a mate
 * (read_collector.py:400, :185), the names numbered by first appearance (the name-keyed tables of read_collector.py:226-234), file order, the
 * offsets of the record table -- through round 5 the host's uz_bam_stage_finish_desc over descriptors that crossed the link.  The descriptors stay
 * in the batch's slot; the host contributes only the records it has to walk itself (unfazed_io.h: uz_stage_walk_flagged, uz_stage_lookup), as
 * descriptors of its own (uz_walk_desc.task = UZ_WALK_TASK_JOIN | join task, .src = UZ_WALK_SRC_AUX | offset in the aux bytes).
 *   uz_bam_walk_flags   what the walk said of every walk task (d_flags, d_walked [n_tasks]) -> uz_stage_walk_flagged
 *   uz_bam_join         first call: n_host tasks of the stage, h_flags [n_host] (the tasks the host walked: their device descriptors are void),
 *                       n_ref references, all_bases; every call: xdesc [n_x] / xaux [xaux_bytes] = what the host walked SINCE the last call,
 *                       look_tid [n_look] = the reference of every look-up task so far, need_jtask = the answers to the last call's needs
 *                       (NULL on the first call).  -> *n_need > 0: the closure needs the index (uz_bam_join_needs -> uz_stage_lookup -> call again);
 *                       *n_need == 0: finished, totals = records, name ids, CIGAR words, row units, base-row units, name bytes
 *   uz_bam_join_fetch   parity / debug: the kept records in output order (any pointer may be NULL); contig_off [n_ref + 1], max_span [n_ref]
 *   uz_reads_from_walk  the record table, unpacked from the bytes in HBM through the kept list in HBM (releases the batch).  want_names: the read
 *                       names stay on the device with the table and uz_reads_names answers name ids (off [n + 1], the bytes in the context's page-locked memory)
 *   uz_walk_slot_stats  [0] device allocations the slots have made, [1] outgrown blocks parked, [2] their bytes, [4..7] the slots' inflated-bytes room */
int uz_bam_walk_flags(uz_ctx *ctx, int walk_id, int32_t *d_flags, int64_t *d_walked);
int uz_bam_join(uz_ctx *ctx, int walk_id, int32_t n_host, const int32_t *h_flags, int32_t n_ref, int all_bases, const uz_walk_desc *xdesc, int64_t n_x, const uint8_t *xaux,
                int64_t xaux_bytes, const int32_t *look_tid, int64_t n_look, const int32_t *need_jtask, int64_t *n_need, int64_t totals[8]);
int uz_bam_join_needs(uz_ctx *ctx, int walk_id, uz_need_rec *need);
int uz_bam_join_fetch(uz_ctx *ctx, int walk_id, uint64_t *voff, uint32_t *qname, int32_t *mate, uint8_t *bases, uz_kept_rec *kept, int64_t *contig_off, int32_t *max_span);
int uz_reads_from_walk(uz_ctx *ctx, int walk_id, int32_t min_base_qual, int want_names, int *reads_id, int64_t totals[8]);
int uz_reads_names(uz_ctx *ctx, int reads_id, const uint32_t *ids, int64_t n, int64_t *off /* [n + 1] */,
                   const uint8_t **bytes /* out: the names back to back in the context's page-locked memory, valid until the next call */);
int uz_walk_slot_stats(uz_ctx *ctx, int64_t out[8]);
/* every free slot among the first n_slots grown, now, to the largest sizes any batch of this context has asked for (a pipeline that will keep
 * n_slots batches in flight calls it once a first batch is through: no later batch's walk then pays for a slot's first gigabytes) */
int uz_walk_reserve(uz_ctx *ctx, int n_slots);
int uz_reads_from_bam(uz_ctx *ctx, int walk_id, const uz_kept_rec *kept, int64_t n, const uint8_t *aux, int64_t aux_bytes, const int64_t *contig_off,
                      const int32_t *max_span, int32_t n_contigs, int64_t n_cigar_total, int64_t n_row_units, int64_t n_seq_units, uint32_t n_qnames,
                      int32_t min_base_qual, uint8_t *names_out /* NULL, or [names_bytes]: the kept records' read names back to back (uz_kept_rec.name_off) */,
                      int64_t names_bytes, int *reads_id);
/* page-locked host memory for the staged columns (plain hipHostMalloc; no context needed) */
int uz_pinned_alloc(size_t bytes, void **out);
void uz_pinned_free(void *p);
/* The same for columns that already live in HBM (device pointers in the views; the library reads them in
 * place and never frees them). */
int uz_sites_adopt_device(uz_ctx *ctx, const uz_sites_view *sites, int *sites_id);
int uz_family_adopt_device(uz_ctx *ctx, int sites_id, const uz_family_view *fam, int *fam_id);
int uz_reads_adopt_device(uz_ctx *ctx, const uz_reads_packed_view *reads, int *reads_id);
/* Forget the derived columns (site classes of every family, per-record QC bits, the window lists of the last finds) so that
 * the next uz_find / uz_phase recomputes them: a timed "whole job" pass starts from the staged inputs only. */
int uz_drop_derived(uz_ctx *ctx);
int uz_sites_free(uz_ctx *ctx, int sites_id); /* also frees its families */
int uz_reads_free(uz_ctx *ctx, int reads_id);

/* ---- site stage ------------------------------------------------------- */
/* K1: one streaming pass over the family's columns -> one class byte per site
 * (UZ_CL_*).  Replaces is_high_quality_site (:46-73), get_kid_allele (:76-134) and
 * the DNM-independent part of find()'s per-variant body (:239-339 = :442-543). */
/* uz_site_scan / uz_site_classes compute every class bit; uz_find / uz_phase in SNV / breakpoint
 * mode run the variant without the DEL / DUP codes, which only whole_region=True reads (:286-291). */
int uz_site_scan(uz_ctx *ctx, int fam_id);
/* Cohort form (many kids / families in one sites VCF, README.md:208): classify n_fam
 * families of the SAME sites table in one launch.  Same result as n_fam calls of uz_site_scan. */
int uz_site_scan_many(uz_ctx *ctx, const int32_t *fam_ids, int32_t n_fam);
int uz_site_classes(uz_ctx *ctx, int fam_id, uint8_t *cls_out /* [n_sites] */);

/* K2: per-DNM window emit.  Replaces get_position (:10-43) / get_close_vars
 * (:399-420) and the list building of find (:262-343).  Runs uz_site_scan first
 * if the family's classes are stale.  Writes the CSR offsets; the lists stay in
 * HBM for uz_phase and can be copied out with uz_find_fetch. */
int uz_find(uz_ctx *ctx, int fam_id, const uz_dnms_view *dnms, int mode,
            int64_t *cand_off /* [n+1] */, int64_t *het_off /* [n+1] */);
int uz_find_fetch(uz_ctx *ctx, int32_t *cand_idx, uint8_t *cand_flags, int32_t *het_idx);
/* uz_find and uz_find_fetch in one call with ONE wait of the host, for a caller that reads the lists at once (a staged pass: the het lists of
 * a chunk tell its decoder what to stage): behind the fill pass one kernel writes the whole answer into `block` -- page-locked memory of this
 * library (uz_pinned_alloc), 256-byte aligned, block_bytes long -- and the call waits for the stream once.  The list lengths are read on the
 * device.  Layout of the block, every part starting at a multiple of 256 bytes, back to back in this order (csrc/find_answer.hpp):
 *     header     int64 [8]: n_cand, n_het, 1 (the answer is whole), the bytes this batch's answer takes, n, 0, 0, 0
 *     cand_off   int64 [n + 1]
 *     het_off    int64 [n + 1]
 *     cand_idx   int32 [n_cand]
 *     cand_flags uint8 [n_cand]
 *     het_idx    int32 [n_het]
 * out [4]: UZ_FA_* bits, the bytes a block for this batch needs, n_cand, n_het.  out[0] == 0: the block holds the answer.  Otherwise it holds
 * none -- the batch outgrew the room its lists had in HBM (UZ_FA_GREW_LISTS: they have been grown and filled again, as uz_find does) or the
 * block (UZ_FA_BLOCK_SMALL) -- and the caller calls again, same batch, with a block of out[1] bytes or more: that call finds the lists in
 * HBM and only writes the answer.  The lists stay in HBM for uz_phase under the same key as uz_find's. */
#define UZ_FA_GREW_LISTS 1
#define UZ_FA_BLOCK_SMALL 2
int uz_find_answer(uz_ctx *ctx, int fam_id, const uz_dnms_view *dnms, int mode, void *block, size_t block_bytes, int64_t out[4]);
/* test / debug: the last uz_find (with its uz_find_fetch) or uz_find_answer (with the call after a fall-back) of the context -- out [4]: stream
 * waits of the host, kernel launches of the find's own (site scan, DNM staging, window passes, scan, copies; not the kernels that finish an
 * asynchronous upload at its first use), UZ_FA_* bits of every call of it, the bytes its answer takes.  Only what these calls launch and
 * wait for is counted: other calls on the context in between (uz_phase_begin, uploads) leave the figures as they are. */
int uz_find_stats(uz_ctx *ctx, int64_t out[4]);
/* Cohort form: the window emit for the DNMs of many kids -- each group with its own trio columns -- in ONE launch sequence instead of one
 * uz_find per kid (the per-family loop of find, informative_site_finder.py:213, :558-568).  `groups` as in uz_phase_cohort, but only fam_id,
 * dnm_first and dnm_count count (reads_id and cutoff are ignored); `dnms` holds all groups' DNMs.  The groups must cover [0, dnms->n) exactly
 * once, in any order; empty groups are allowed and one family may serve several groups.  UZ_E_ARG: a gap, an overlap, a group outside the
 * batch, families of different sites tables.  Families whose classes are stale (for UZ_FIND_WHOLE_REGION: or lack the DEL / DUP codes) are
 * classified in one launch first.  Every mode of uz_find; the offsets and, through uz_find_fetch, the lists are those of one uz_find per
 * group laid end to end in DNM order.  The lists are kept under no key: a later uz_phase over the same DNMs computes its own. */
int uz_find_cohort(uz_ctx *ctx, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *dnms, int mode,
                   int64_t *cand_off /* [n+1] */, int64_t *het_off /* [n+1] */);
/* (The lists of the last THREE finds stay in HBM: a uz_phase / uz_phase_begin over a batch -- same family, DNMs, mode and parameters --
 * that one of them covered takes its lists instead of running the window emit again.  A staged pass calls uz_find for chunk k + 1,
 * whose het lists tell the decoder what to stage, before it queues the read stage of chunk k.) */

/* ---- read stage ------------------------------------------------------- */
/* Everything multithread_read_phasing does after get_refalt (snv_phaser.py:131-203):
 * collect_reads_snv (+ group_reads_by_haplotype / connect_reads), match_informative_sites,
 * phase_by_reads, the unique-name / unique-site tally and summarize_record's integer
 * read-backed decision (unfazed.py:193-234).  Runs the window emit for the batch first
 * (find_mode: UZ_FIND_SECOND_WINDOW for find, 0 for find_many; never WHOLE_REGION),
 * whose lists can be read back with uz_find_fetch afterwards.
 * counts = dad_reads, mom_reads, dad_sites, mom_sites per DNM. */
int uz_phase(uz_ctx *ctx, int fam_id, int reads_id, const uz_dnms_view *dnms, int find_mode,
             int32_t *status /* [n] UZ_ST_* */, int32_t *counts /* [4n] */,
             int32_t *origin /* [n] UZ_OR_* */, int32_t *evidence /* [n] */);
/* uz_phase in two halves, for a caller that has the next batch's work ready: uz_phase_begin queues the window emit and the read
 * stage and returns without waiting (a first batch, whose sizes nothing predicts yet, runs to its end instead); uz_phase_end -- same
 * batch, same arguments -- waits and hands out the results of uz_phase.  Between the two the caller may upload tables and run
 * uz_site_scan / uz_find / uz_phase_cnv for OTHER batches (they queue up behind the read stage: the device does not idle through the
 * host's round trips); not another uz_phase / uz_phase_begin / uz_phase_cohort, and not uz_find_fetch / uz_phase_votes of this batch
 * before uz_phase_end has returned.  After an
 * intervening uz_find the window lists of the context are that batch's: uz_find_fetch then returns those. */
int uz_phase_begin(uz_ctx *ctx, int fam_id, int reads_id, const uz_dnms_view *dnms, int find_mode);
int uz_phase_end(uz_ctx *ctx, int fam_id, int reads_id, const uz_dnms_view *dnms, int find_mode,
                 int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence);
/* Cohort form (603 samples in one run, README.md:208; one alignment file per kid, unfazed.py:574-575): the
 * DNMs of many kids -- each with its own trio columns, its own alignment records and its own insert cutoff -- in ONE
 * launch sequence instead of one per kid.  `dnms` holds all groups' DNMs back to back; `rcontig` refers to the group's
 * own reads table and dnms->cutoff is ignored.  The groups must cover [0, dnms->n) exactly once, in any order; empty groups
 * are allowed and one family (with its reads table) may serve several groups.  UZ_E_ARG, as from uz_find_cohort and before
 * anything of the context is touched: a gap, an overlap, a group outside the batch, families of different sites tables.
 * Families whose classes are stale are classified in one launch first.  The kids' tables are laid
 * end to end in HBM as one table (virtual contigs = kid x contig; rebuilt only when the list of reads_ids changes), the
 * window emit reads every DNM's own family column, the read stage every DNM's own cutoff.  Results as uz_phase, in DNM
 * order; uz_phase_votes / uz_phase_groups afterwards give query-name ids of the group's own table. */
int uz_phase_cohort(uz_ctx *ctx, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *dnms, int find_mode,
                    int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence);
/* The same run on a table that already IS the groups' tables end to end: one built over the groups' alignment files presented as one file
 * (uz_bam_walk_many ... uz_reads_from_walk).  group_ref_base [n_groups]: where each group's file starts among the table's contigs (its contigs
 * reach to the next larger base of any group, or to the table's end); `rcontig` of a DNM is the file's own number and becomes -1 outside the
 * file.  groups[g].reads_id is not looked at; the groups are held to uz_phase_cohort's rules (exact cover of [0, dnms->n), one sites table:
 * UZ_E_ARG otherwise) and their stale families classified in one launch.  Nothing is concatenated and nothing copied per group; uz_phase_votes / uz_phase_groups give the
 * TABLE's name ids (uz_reads_files: where each file's begin). */
int uz_phase_cohort_joined(uz_ctx *ctx, int reads_id, const uz_cohort_group *groups, int32_t n_groups, const int32_t *group_ref_base, const uz_dnms_view *dnms,
                           int find_mode, int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence);
/* Vote lists of the last uz_phase (for --verbose and the records dict):
 * vote_off[4n+1] then vote_val: dad_reads (qname ids, ascending), mom_reads,
 * dad_sites (positions, ascending), mom_sites.  Call with vote_val == NULL to get
 * the offsets / total first. */
int uz_phase_votes(uz_ctx *ctx, int64_t *vote_off /* [4n+1] */, int32_t *vote_val);
/* Haplotype groups after connect_reads of the last uz_phase (diagnostics / tests):
 * grp_off[2n+1] then grp_q: "ref" set then "alt" set (qname ids, ascending). */
int uz_phase_groups(uz_ctx *ctx, int64_t *grp_off /* [2n+1] */, int32_t *grp_q);
/* Test hook: what the sizing pass left for the batch of the last uz_phase / uz_phase_end (n DNMs, n_het = het_off[n] het sites of its
 * window lists).  bounds: five numbers per DNM -- records of its own fetch, sum of the lengths of its het-site fetch ranges (capped at
 * 0x7FFFFFF0), het sites, candidates, most het sites within one record's reach.  pre_win: first / one-past-last record of the DNM's own
 * fetch (an SV's: of both breakpoint fetches).  pre_ha / pre_hl: first record and length of every het site's fetch range, in the order
 * of het_idx (0 for the sites of a DNM without candidates).  reduced: the batch's reduction of `bounds`, UZ_SIZING_REDUCED_WORDS 8-byte
 * words: [0] max bounds[0], [1] max bounds[1], [2] max bounds[2], [3] max bounds[3], [4] DNMs with candidates, [5] max of
 * M = b1 + 4 b0 (b4 + 1), [6] sum of min(M, 4096) + b3, [7 + k], k < 256: DNMs with candidates whose arena estimate
 * min(((37 b1) / 4 + 10 b0 + 3328 + 255) >> 8, 255) is k.  Any pointer may be NULL.  UZ_E_STATE: no batch has run on the context, or one is
 * open (uz_phase_begin). */
#define UZ_SIZING_REDUCED_WORDS 263
int uz_phase_sizing_fetch(uz_ctx *ctx, int32_t *bounds /* [5n] */, int32_t *pre_win /* [4n] */, int32_t *pre_ha /* [n_het] */,
                          int32_t *pre_hl /* [n_het] */, int64_t *reduced /* [UZ_SIZING_REDUCED_WORDS] */);

/* ---- BED rows as text -------------------------------------------------- */
/* The BED lines of rows of the LAST finished uz_phase / uz_phase_end / uz_phase_cohort / uz_phase_cohort_joined, written by kernels from the
 * batch's result where it lies (k_bed_size, a scan, k_bed_fill; csrc/bed_row.hpp is the body): the decision of summarize_record's read-backed
 * branches (unfazed.py:206-234) with the evidence_min_ratio of uz_set_params, the SEX-CHROM row of summarize_autophased, and the line of
 * write_bed_output -- nine tab-separated fields, thirteen when verbose, '\n'.  Row k is bytes[off[k] .. off[k + 1]); a row is EMPTY when its DNM's
 * status is not UZ_ST_OK, or when its origin is None or ambiguous and include_ambiguous is 0.  The host orders the rows and writes the header.
 * Verbose site lists are sorted as decimal strings (unfazed.py:302-303), read names stand in list order; a verbose row's reads_id names the table
 * whose names its ids are (a cohort batch hands ids back relative to the group's own table, as uz_phase_votes does).
 * The text lies in page-locked memory of the context, valid until the next call.
 * UZ_E_STATE: no finished batch, or an open one (uz_phase_begin); verbose with a table that holds no names on the device (only a table of
 * uz_reads_from_walk with names does) or a batch that kept no lists; a site list that is not ascending; a name id at or beyond the table's
 * names; a row whose written bytes differ from its sized length.  UZ_E_ARG: a DNM index, string id or reads id out of range.  UZ_E_RANGE: 4 GiB or
 * more of text.  A call that is not verbose reads no name and works with any table. */
int uz_bed_rows(uz_ctx *ctx, const uz_bed_view *rows, int verbose, int include_ambiguous, int64_t *off /* [n_rows + 1] */, const uint8_t **bytes);
/* Test hook (as uz_phase_sizing_fetch is one): the same kernels over lists the caller supplies, no read stage run -- status [n_dnms], list_off
 * [4 n_dnms + 1] + list_val in uz_phase_votes' layout, the names as a plain store (name_off [n_qnames + 1] + name_bytes; NULL: no names, as a
 * table without them), the ratio.  Rows' reads_id is ignored.  Refusals as above; UZ_E_ARG on offsets that descend. */
int uz_bed_rows_lists(uz_ctx *ctx, const uz_bed_view *rows, int verbose, int include_ambiguous, int32_t n_dnms, const int32_t *status,
                      const int64_t *list_off, const int32_t *list_val, uint32_t n_qnames, const uint32_t *name_off, const uint8_t *name_bytes,
                      int32_t evidence_min_ratio, int64_t *off /* [n_rows + 1] */, const uint8_t **bytes);

/* ---- annotated VCF rows as text ---------------------------------------- */
/* The record lines of the annotated VCF (unfazed.py: write_vcf_output), rewritten by kernels from the DNM file's own text (k_vcfout_size, a scan,
 * k_vcfout_fill per chunk; csrc/vcf_row.hpp is the body and states the rules): FORMAT gets ":UOPS:UET", every sample column is padded with ":."
 * to FORMAT's piece count and gets ":<uops>:<uet>" -- ":-1:-1" unless the column has an annotation and the cell's own genotype, read from its
 * text, is HET or HOM_ALT -- and an applied annotation with gt code 1 / 2 replaces the GT piece by "1|0" / "0|1".  '\n' ends every line.
 * text: the view of unfazed_io.h: uz_vcf_samples_text; line_at [n_records]: where every record's line starts.  The annotations are a sparse
 * table over the records: record k has ann_off[k] .. ann_off[k + 1], its columns (ann_col, indices of sample columns) strictly ascending;
 * ann_gt 0 none, 1 "1|0", 2 "0|1"; ann_uops -1 .. 999 999; ann_uet -1 .. 6.  The text goes up in chunks cut at line ends
 * (UZ_VCFOUT_CHUNK_BYTES, read per call, 32 MiB), chunk k + 1 copied while chunk k is worked on.
 * Record k is bytes[off[k] .. off[k + 1]).  A record the kernels will not vouch for is HANDED BACK: handed_back[k] = 1 and off[k + 1] == off[k];
 * the caller writes it with its own per-record code.  Handed back: a GT piece outside the genotype grammar (an empty one included), a count of
 * sample columns that differs from text->n_samples, a line without FORMAT, a FORMAT that names GT twice, an annotation outside the ranges above
 * or at a column >= n_samples, columns that do not ascend, a line that holds a '\r', a line of 4 GiB.
 * The text lies in page-locked memory of the context, valid until the next call.  No entry point runs the read stage: the annotations are all
 * the call knows of phasing.  UZ_E_ARG (nothing launched): offsets that descend, a NULL table with annotations, a line outside the text.
 * UZ_E_RANGE: 4 GiB or more of output from one chunk.  UZ_E_STATE: a record whose written bytes differ from its sized length. */
int uz_vcf_rows(uz_ctx *ctx, const uz_vcf_text_view *text, const int64_t *line_at /* [n_records] */, const int64_t *ann_off /* [n_records + 1] */,
                const int32_t *ann_col, const uint8_t *ann_gt, const int32_t *ann_uops, const int8_t *ann_uet, int64_t *off /* [n_records + 1] */,
                const uint8_t **bytes, uint8_t *handed_back /* [n_records] */);

/* The records of a BCF as VCF text lines (unfazed.py: write_vcf_output on a BCF of DNMs, UZ_BCF_ROUTE=device), written by kernels from the
 * records' own bytes (k_bcfout_size, a scan, k_bcfout_fill per chunk; csrc/bcf_row.hpp is the body and states the rules): CHROM from the
 * header's contigs by id, POS + 1, ID, REF, ALT, QUAL by C's "%g" where that prints fixed notation, FILTER and INFO through the dictionary,
 * FORMAT and one column per sample, GT as alleles joined by '/' or '|'; every line closed by '\n'.  The text is what uz_vcf_rows takes next.
 * records: unfazed_io.h: uz_vcf_bcf_lines of a decoded BCF, or the caller's own arrays (HOST pointers).  The kernels prove every bound
 * themselves, against l_shared / l_indiv and the data's end: the bytes need not have passed a decoder.
 * off [n_records + 1]: record k's line is bytes[off[k], off[k + 1]), empty when the record is handed back; samp_at [n_records]: the offset in
 * `bytes` of the first byte of column 10 (of the closing '\n' when the line has none; off[k] for a record handed back) -- uz_vcf_text_view's
 * samp_at, its line_end being off[k + 1] - 1; *bytes: page-locked memory of the context, valid until the next uz_bcf_rows.
 * handed_back [k] = 1: the kernels do not vouch for the record and the caller writes its line (unfazed_amd/bcf_text.py) -- a float "%g" prints
 * in exponent form, an infinity or NaN; a record without an allele; a contig or dictionary id without a name; a key that is no scalar
 * integer; a type outside {0, 1, 2, 3, 5, 7}; a byte outside 0x20 .. 0x7E in a copied string; a typed value, length or array that does not
 * lie inside its block, or a block outside the data; n_sample different from n_samples while the record has FORMAT fields; a negative GT
 * entry; a line of 4 GiB.
 * The record bytes go up in chunks of UZ_BCFOUT_CHUNK_BYTES (read per call, 32 MiB) cut at record ends, chunk k + 1 copied while chunk k is
 * worked on; a record longer than a chunk gets a chunk of its own.
 * UZ_E_ARG (nothing launched): a NULL table, name offsets that descend, a rec_at that descends or lies outside `data`.  UZ_E_RANGE: 4 GiB or
 * more of text from one chunk.  UZ_E_STATE: a record whose written bytes differ from its sized length. */
int uz_bcf_rows(uz_ctx *ctx, const uz_bcf_lines_view *records, int64_t *off /* [n_records + 1] */, uint64_t *samp_at /* [n_records] */,
                const uint8_t **bytes, uint8_t *handed_back /* [n_records] */);

/* A host buffer written as BGZF blocks on the device (k_deflate.hip; csrc/deflate_body.hpp states the rules): the mirror image of
 * uz_bgzf_inflate.  data [n_bytes] is cut into slices of 65 280 bytes (htslib's), the last one shorter; every slice becomes one block: the
 * 18-byte header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, "BC", 2, BSIZE = block length - 1), one raw DEFLATE stream -- LZ77 over the
 * slice alone, one fixed-Huffman block (BTYPE 01), or one stored block (BTYPE 00) where that is shorter -- CRC-32 and ISIZE.  No block is
 * longer than 65 311 bytes.  *n_blocks: the blocks; *bgzf [*bgzf_bytes]: the blocks back to back, page-locked memory of the context, valid
 * until the next uz_bgzf_deflate.  The blocks only: the caller writes the 28-byte end-of-file marker behind them.
 * n_bytes == 0: no block, nothing launched, *bgzf NULL.  The same input gives the same bytes in every call.
 * repeat / kernel_ms as in uz_bgzf_inflate: repeat > 0 launches k_bgzf_deflate that many more times and *kernel_ms is the mean time of one
 * pass over the whole input (summed over the chunks).
 * The input goes up in chunks of UZ_BGZF_CHUNK_BYTES (read per call, 32 MiB, rounded down to a multiple of 65 280: the slices do not depend
 * on it), chunk k + 1 copied while chunk k is worked on.
 * UZ_E_ARG (nothing launched): NULL data with n_bytes > 0, a NULL result.  UZ_E_STATE: a framed block whose written size differs from its
 * scanned size. */
int uz_bgzf_deflate(uz_ctx *ctx, const uint8_t *data /* host */, int64_t n_bytes, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes,
                    int repeat, double *kernel_ms);

/* The same call with the choice of the coder.  code = UZ_DF_CODE_FIXED: uz_bgzf_deflate, byte for byte.  code = UZ_DF_CODE_DYNAMIC
 * (k_bgzf_deflate_dyn; csrc/deflate_dyn.hpp states the rules): the same LZ77 parse, taken over the whole slice; then per slice the shortest, in
 * whole bytes, of one dynamic-Huffman block (BTYPE 10: optimal code lengths under the 15- and 7-bit limits, run-length coded header), the
 * fixed-Huffman block (taken unless the dynamic one is strictly shorter: then uz_bgzf_deflate's bytes) and the stored block of 5 + n bytes.  So
 * no block is longer than the fixed code's block of the same slice.  The tokens wait between the two passes in a device buffer of the context
 * of 65 280 words per slice of a chunk: 131 MB at the default chunk size, 4.3 GB at the 1 GiB cap of UZ_BGZF_CHUNK_BYTES.
 * kinds: NULL, or [3]: the blocks that came out stored / fixed / dynamic (read from the blocks' BTYPE).  repeat times the kernel of the
 * chosen code.  Everything else as in uz_bgzf_deflate; the two share *bgzf.
 * UZ_E_ARG (nothing launched): any other code, and what uz_bgzf_deflate refuses. */
#define UZ_DF_CODE_FIXED 0
#define UZ_DF_CODE_DYNAMIC 1
int uz_bgzf_deflate_coded(uz_ctx *ctx, const uint8_t *data /* host */, int64_t n_bytes, int code, int64_t *kinds /* NULL or [3] */, int64_t *n_blocks,
                          const uint8_t **bgzf, int64_t *bgzf_bytes, int repeat, double *kernel_ms);

/* uz_bgzf_deflate_coded, and the tables of a tabix index (.tbi) of the text it compresses, from the same upload (k_tbx.hip; csrc/tbx_key.hpp
 * states the rules of a line).  The blocks are byte for byte uz_bgzf_deflate_coded's.  preset: UZ_TBX_PRESET_VCF (CHROM, POS, len(REF) and
 * INFO/END) or UZ_TBX_PRESET_BED (columns 1 / 2 / 3); lines that begin with '#' are meta lines.  A record's virtual offset is
 * (offset of its block << 16 | offset in the block's 65 280 bytes); the last record ends at (*bgzf_bytes << 16), where the caller's
 * end-of-file marker goes.
 * view (page-locked memory of the context, valid until the next uz_bgzf_deflate* call):
 *   status    0, or why the text has no index (UZ_TBX_S_*): then n_refs = n_runs = n_linear = 0
 *   refs      per reference, in file order: its name's place in `data`, n_intv, the pseudo-bin's values (first record's start, last record's
 *             end, the record count)
 *   runs      maximal runs of consecutive records with one (tid, bin), in file order: a bin's chunks are its runs, in this order (grouping
 *             them by (tid, bin) is a stable sort of a table the index's own size: the caller's)
 *   linear    the references' 16 kb windows back to back (n_intv each): the smallest start offset of a record that overlaps the window,
 *             an empty window filled from the next one
 *   host_rows the rows the call's host code settled: a chunk's first line (its predecessor is not in the chunk) and a line whose key columns
 *             the chunk's end cut: at most two per chunk
 * A contig that comes back after another one is not looked for here: the caller sees it in the references' names.
 * UZ_E_ARG: any other preset, a NULL view, and what uz_bgzf_deflate_coded refuses. */
#define UZ_TBX_PRESET_VCF 0
#define UZ_TBX_PRESET_BED 1
#define UZ_TBX_S_ORDER 1u  /* a start below the previous record's on the same contig */
#define UZ_TBX_S_RANGE 2u  /* a begin or end beyond 2^29 */
#define UZ_TBX_S_META 4u   /* a meta line among the data rows */
#define UZ_TBX_S_EMPTY 8u  /* an empty line */
#define UZ_TBX_S_CR 16u    /* a '\r' */
#define UZ_TBX_S_POS 32u   /* a position that is not 1 to 10 digits */
#define UZ_TBX_S_CUT 64u   /* (internal) a cut row that nobody settled */
typedef struct uz_tbx_ref {
    uint64_t name_off; /* in `data` */
    uint32_t name_len, n_intv;
    uint64_t v0, v1, n_rows;
} uz_tbx_ref;
typedef struct uz_tbx_run {
    uint32_t tid, bin;
    uint64_t v0, v1;
} uz_tbx_run;
typedef struct uz_tbx_view {
    int64_t n_rows, n_refs, n_runs, n_linear, host_rows;
    uint32_t status, pad_;
    const uz_tbx_ref *refs;
    const uz_tbx_run *runs;
    const uint64_t *linear;
} uz_tbx_view;
int uz_bgzf_deflate_indexed(uz_ctx *ctx, const uint8_t *data /* host */, int64_t n_bytes, int code, int64_t *kinds /* NULL or [3] */, int64_t *n_blocks,
                            const uint8_t **bgzf, int64_t *bgzf_bytes, int repeat, double *kernel_ms, int preset, uz_tbx_view *view);

/* ---- allele-balance (CNV) stage ---------------------------------------- */
/* K6.  Everything run_cnv_phasing does after its find (sv_phaser.py:357-423: phase_by_snvs :71-85,
 * multithread_cnv_phasing :269-301) and the decision of summarize_record (unfazed.py:193-298): runs the window
 * emit for the batch in UZ_FIND_WHOLE_REGION mode (search_dist 0, whole_region=True, :375-389), lets every candidate
 * of a DEL / DUP vote for the parent its kid_allele names, and decides.
 * rb_counts: optional [4n] read-backed counts of the same DNMs (dad_reads, mom_reads, dad_sites, mom_sites, e.g. the
 * `counts` of uz_phase): merged as summarize_record merges them (READBACKED + ALLELE-BALANCE, AMBIGUOUS_BOTH, ...);
 * NULL = allele-balance evidence only.
 * cnv_counts [2n] = cnv_dad_sites, cnv_mom_sites; origin UZ_OR_* (AMBIGUOUS = "dad|mom"); evidence = evidence_count;
 * etype = UZ_ET_* mask. */
int uz_phase_cnv(uz_ctx *ctx, int fam_id, const uz_dnms_view *dnms, const int32_t *rb_counts, int32_t *cnv_counts /* [2n] */,
                 int32_t *origin /* [n] */, int32_t *evidence /* [n] */, int32_t *etype /* [n] */);
/* Cohort form: the DEL / DUP of many kids in ONE whole-region find (a family per DNM) and one K6 launch instead of one uz_phase_cnv per
 * kid (the per-kid loop of run_cnv_phasing, sv_phaser.py:357-423).  Groups as in uz_find_cohort; rb_counts and the results as in
 * uz_phase_cnv, in DNM order. */
int uz_phase_cnv_cohort(uz_ctx *ctx, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *dnms, const int32_t *rb_counts,
                        int32_t *cnv_counts /* [2n] */, int32_t *origin /* [n] */, int32_t *evidence /* [n] */, int32_t *etype /* [n] */);
/* Site lists of the last uz_phase_cnv / uz_phase_cnv_cohort: off[2n+1], then pos: cnv_dad_sites, cnv_mom_sites per DNM (positions in
 * candidate-list order).  pos == NULL: offsets only.  The lists lie back to back on the device (k_cnv_dense): off[2n] positions are
 * copied, not the batch's candidates. */
int uz_phase_cnv_sites(uz_ctx *ctx, int64_t *off /* [2n+1] */, int32_t *pos);

/* ---- measurement ------------------------------------------------------ */
/* HIP-event timing of the kernels launched on the context's stream since the
 * last reset: total milliseconds and launch count per UZ_K_* id.
 * on: 0 none, 1 every id, otherwise a set of ids -- (1 << (id + 1)) for each id
 * wanted (two event records per timed launch are host work in front of the
 * launch: a caller that times a whole pass keeps the set small). */
int uz_prof_enable(uz_ctx *ctx, int on);
int uz_prof_reset(uz_ctx *ctx);
int uz_prof_get(uz_ctx *ctx, int kernel, double *total_ms, int64_t *launches);
/* Units the last launch of a kernel processed (K3a ids: alignment records examined; 0 when unknown). */
int uz_prof_units(uz_ctx *ctx, int kernel, int64_t *units);

#ifdef __cplusplus
}
#endif
#endif /* UNFAZED_HIP_H */
