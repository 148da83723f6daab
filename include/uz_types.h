/* uz_types.h -- plain-C views of the decoded inputs of the per-DNM phasing path.
 *
 * Shared by the C ABI (include/unfazed_hip.h), the HIP sources and the CPU
 * oracle (oracle/).  All pointers in these views are HOST pointers owned by the
 * caller; the library copies what it needs into HBM at upload time.
 *
 * Column semantics follow the libraries the reference reads its inputs with
 * (cyvcf2 / pysam) -- see unfazed_amd/model.py.
 */
#ifndef UZ_TYPES_H
#define UZ_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* genotype codes: reference unfazed/utils.py:2-5 */
#define UZ_HOM_REF 0
#define UZ_HET 1
#define UZ_GT_UNKNOWN 2
#define UZ_HOM_ALT 3

#define UZ_U16_MISSING 0xFFFFu /* cyvcf2's -1 (missing depth / GQ) in the 16-bit columns, which hold 0..32767
                                * otherwise (the kernels read them as signed halfwords) */

/* site flags */
#define UZ_SF_COMPLEX 1u /* reference informative_site_finder.py:239-243 */

/* site class byte written by the site-scan kernel (one per site per family) */
#define UZ_CL_HET 0x01u       /* usable for extended read-backed phasing (:268-284) */
#define UZ_CL_CAND 0x02u      /* informative site, SNV / breakpoint mode (:292-320) */
#define UZ_CL_ALT_DAD 0x04u   /* alt_parent is dad (else mom) -- valid when a pattern matched */
#define UZ_CL_DEL_SHIFT 3     /* bits 3-4: candidate code for a DEL (0 none, 1 ref_parent, 2 alt_parent) */
#define UZ_CL_DUP_SHIFT 5     /* bits 5-6: same for a DUP (get_kid_allele, :76-134) */
#define UZ_KA_NONE 0
#define UZ_KA_REF_PARENT 1
#define UZ_KA_ALT_PARENT 2

/* DNM variant type */
#define UZ_VT_POINT 0 /* POINT / SNV / INDEL */
#define UZ_VT_DEL 1
#define UZ_VT_DUP 2
#define UZ_VT_OTHER_SV 3

/* DNM flags */
#define UZ_DF_FETCH_FALLBACK 1u /* contig resolved through the renamed-contig fallback: fetch [pos,pos+1) (read_collector.py:386-392) */

/* candidate flags in the find output */
#define UZ_CF_ALT_DAD 0x1u
#define UZ_CF_KA_SHIFT 1 /* bits 1-2: kid_allele code (CNV mode) */

/* segment aux bits */
#define UZ_AUX_MATE_SAME_TID 1u
#define UZ_AUX_HAS_SA 2u
#define UZ_AUX_DECODE_BAD 4u
#define UZ_AUX_SIMPLE_SHIFT 4 /* packed form with cigar_compact, two bits: 0 = the CIGAR words are in `cigar`; 1 / 2 / 3 = one M / = / X over l_seq bases */
#define UZ_AUX_SIMPLE_MASK 48u
#define UZ_AUX_NO_SEQ 8u /* packed form only: the record was staged WITHOUT its bases (reachable only as a mate: nothing ever
                          * reads them); it has a quality-plane row but no seq4 row.  A kernel that asks for its bases fails loudly. */

/* per-DNM status of the read stage */
#define UZ_ST_OK 0             /* a record exists */
#define UZ_ST_NO_CAND 1        /* "No usable informative sites" (snv_phaser.py:254-262) */
#define UZ_ST_NO_OVERLAP 2     /* "No reads overlap informative sites" (snv_phaser.py:158-166) */
#define UZ_ST_REF_EXCEPTION 3  /* the reference raises inside the worker (KeyError in connect_reads): no record */
#define UZ_ST_SKIPPED 4        /* not run (host filtered: autophase, no genotype, ...) */
#define UZ_ST_CAPACITY 5       /* a per-DNM size exceeds the device layout (>= 2^20 list entries): reported, never silently dropped */

/* origin codes of the integer decision rule (unfazed.py:206-234) */
#define UZ_OR_NONE 0
#define UZ_OR_DAD 1
#define UZ_OR_MOM 2
#define UZ_OR_AMBIGUOUS 3

/* evidence types of summarize_record (unfazed.py:190-334), as a bit mask in list order */
#define UZ_ET_READBACKED 1
#define UZ_ET_ALLELE_BALANCE 2
#define UZ_ET_AMBIGUOUS_READBACKED 4
#define UZ_ET_AMBIGUOUS_ALLELE_BALANCE 8
#define UZ_ET_AMBIGUOUS_BOTH 16
#define UZ_ET_AMBIG_FLAG 32 /* the `ambig` variable: the call is dropped unless --include-ambiguous */

typedef struct uz_params {
    int32_t search_dist;        /* --search-dist */
    int32_t min_gt_qual;        /* --min-gt-qual: GQ threshold AND base-quality threshold (read_collector.py:361-362) */
    int32_t min_depth;          /* --min-depth */
    int32_t min_map_qual;       /* --min-map-qual */
    int32_t readlen;            /* --readlen */
    int32_t split_error_margin; /* --split-error-margin */
    int32_t no_extended;        /* --no-extended */
    int32_t read_goal;          /* EXTENDED_RB_READ_GOAL = --insert-size-max-sample (read_collector.py:369-370) */
    int32_t evidence_min_ratio; /* --evidence-min-ratio */
    int32_t reserved0;
    double ab_homref[2];
    double ab_homalt[2];
    double ab_het[2];
} uz_params;

/* sites table: records of the sites VCF in file order, grouped by contig */
typedef struct uz_sites_view {
    int64_t n_sites;
    int32_t n_contigs;
    int32_t reserved0;
    const int64_t *contig_off; /* [n_contigs+1] */
    const int32_t *pos;        /* [S] Variant.start (0-based) */
    const uint8_t *sflags;     /* [S] UZ_SF_* */
    const uint8_t *ref_base;   /* [S] ASCII, 0 for complex records */
    const uint8_t *alt_base;   /* [S] */
    /* The compact link form (uz_sites_pack writes it; pos / sflags / ref_base / alt_base are then NULL): 4 bytes per site cross the link
     * instead of 7.  Sites are taken in spans of UZ_SITE_SPAN; span s starts at site s * UZ_SITE_SPAN.
     *   pos_d16[i]      pos[i] - pos[i - 1] where that lies in [0, UZ_POS_D16_LIMIT) (anything where site i starts a span or escapes)
     *   bases8[i]       UZ_BASE3 code of ref_base | code of alt_base << 3 | complex (UZ_SF_COMPLEX) << 6.  Both readers (k_sites_expand,
     *                   uz_sites_unpack) decode the codes 6 and 7 as 'N' and ignore bit 7; uz_sites_pack writes neither.
     *   span_pos[s]     pos of the span's first site
     *   pos_esc_*       the escapes, ascending by site index: every other site whose difference does not fit, and the first site of every
     *                   contig -- index and absolute pos; pos_esc_off[s] = first escape of span s (n_spans + 1 entries, the last n_pos_esc).
     *                   A span's first site is never an escape (span_pos holds its pos): both readers refuse a list that names one.
     * pos[i] is then the value of the last anchor at or before i within its span (the span's first site, or an escape) plus the pos_d16 of
     * the sites after that anchor up to i.  Only uz_sites_family_upload_async takes this form; the device expands it into the plain
     * columns at first use. */
    const uint16_t *pos_d16;
    const uint8_t *bases8;
    const int32_t *span_pos;    /* [n_spans] */
    int64_t n_pos_esc;
    const int32_t *pos_esc_idx; /* [n_pos_esc] */
    const int32_t *pos_esc_val; /* [n_pos_esc] */
    const int32_t *pos_esc_off; /* [n_spans + 1] */
} uz_sites_view;
#define UZ_SITE_SPAN 1024
#define UZ_POS_D16_LIMIT 32768
/* the bases of a plain site in three bits (bases8): 0 = none (complex records), 1 .. 5 = A C G T N */
#define UZ_BASE3_CODES "\0ACGTN"


/* genotype columns of one trio, member order kid, dad, mom */
typedef struct uz_family_view {
    const uint8_t *gt;            /* [S] kid | dad<<2 | mom<<4 (cyvcf2 gt_types codes) */
    const uint16_t *ref_depth[3]; /* [S] each; UZ_U16_MISSING = -1 */
    const uint16_t *alt_depth[3];
    const uint16_t *gq[3];        /* floor(GQ); UZ_U16_MISSING = -1 */
    /* Sites with an allele depth the 16-bit columns cannot hold (> 32767: the reference takes any depth,
     * informative_site_finder.py:46-73): listed apart with their depths in 32 bits, all three members, -1 = missing.  The 16-bit
     * columns may hold anything there; the class of such a site is computed from these (same rule, the same f64 division).
     * HOST pointers, also for uz_family_adopt_device; n_wide = 0 / NULL: none.  wide_site ascending. */
    int64_t n_wide;
    const int64_t *wide_site;        /* [n_wide] site index */
    const int32_t *wide_ref_depth[3]; /* [n_wide] each; values up to 2^30 */
    const int32_t *wide_alt_depth[3];
    /* The nine columns in EIGHT bits for the host link (set all nine; ref_depth / alt_depth / gq are then NULL): a trio sequenced to
     * 30x has depths of a few dozen and genotype qualities of at most 99.  A depth byte below 254 is the depth; UZ_U8_MISSING (254) =
     * missing; UZ_U8_SEE_WIDE (255) = the site stands in the wide list above with its exact depths (any member's depth of 254 or more puts
     * it there).  A quality byte below 255 is min(floor(GQ), 254); 255 = missing --
     * the site tests compare GQ with --min-gt-qual only, so the clamp is exact for thresholds up to 254 (a family staged this way refuses
     * a larger one, UZ_E_STATE).  The device widens the columns to the 16-bit ones its kernels read: 10 bytes per site cross the link
     * instead of 19. */
    const uint8_t *ref_depth8[3];
    const uint8_t *alt_depth8[3];
    const uint8_t *gq8[3];
    /* The het form (uz_family_pack_het writes it; all nine plain columns, 16- and 8-bit, are then NULL): the nine bytes travel for the
     * kid-het sites only -- (gt & 3) == UZ_HET on this view's own gt -- since the SNV / breakpoint classes of every other site follow from
     * gt alone (HET and CAND need a het kid, ALT_DAD is the parental pattern).  Sites in spans of UZ_SITE_SPAN, as the compact site form.
     *   het9[9 * e + q]   het site e in site order, q = rd kid, dad, mom, ad kid, dad, mom, gq kid, dad, mom, in the eight-bit encoding above
     *   het_span_off[s]   kid-het sites before span s (n_spans + 1 entries, the last n_het)
     * Only uz_sites_family_upload_async takes it, together with the compact site form; the device writes the 16-bit columns of the het
     * sites and zeros for all others.  What needs the other sites' columns refuses such a family (UZ_E_STATE): the DEL / DUP classes
     * (uz_phase_cnv, uz_phase_cnv_cohort, a whole-region find) and uz_family_fetch. */
    const uint8_t *het9;
    const int32_t *het_span_off;
    int64_t n_het;
} uz_family_view;
#define UZ_U8_MISSING 254u
#define UZ_U8_SEE_WIDE 255u

/* genotype columns of the samples of a cohort, sample-major: every sample's columns lie in HBM once, and a trio's nine 16-bit columns
 * are nine rows of this table (uz_families_from_samples).  The values mean what the columns of uz_family_view mean: UZ_U16_MISSING,
 * depths clamped at 32767, floor(GQ).  The wide list is the TABLE's: a site stands in it when any sample of the table has a depth
 * above 32767 there, with every sample's depths in 32 bits (-1 = missing).  HOST pointers; rows back to back (row s at s * n_sites,
 * s * n_wide for the wide depths). */
typedef struct uz_samples_view {
    int32_t n_samples;
    int32_t reserved0;
    const uint8_t *gt;             /* [n_samples][S] cyvcf2 gt_types codes (0 / 1 / 2 / 3) */
    const uint16_t *ref_depth;     /* [n_samples][S] */
    const uint16_t *alt_depth;     /* [n_samples][S] */
    const uint16_t *gq;            /* [n_samples][S] */
    int64_t n_wide;
    const int64_t *wide_site;      /* [n_wide] site index, ascending */
    const int32_t *wide_ref_depth; /* [n_samples][n_wide]; values up to 2^30 */
    const int32_t *wide_alt_depth; /* [n_samples][n_wide] */
} uz_samples_view;

/* The record text of a decoded text VCF and where every record's sample columns lie in it (unfazed_io.h: uz_vcf_samples_text; taken by
 * unfazed_hip.h: uz_samples_from_text, which parses the sample cells on the device).  HOST pointers into the decoder's table: they live
 * as long as it does. */
typedef struct uz_vcf_text_view {
    const uint8_t *text;
    int64_t text_bytes;
    int64_t n_records;
    int32_t n_samples;       /* sample columns the header names */
    int32_t reserved0;
    const uint64_t *samp_at;  /* [n_records] offset of the first byte of column 10 (the line end when the line has none) */
    const uint64_t *line_end; /* [n_records] offset of the record's '\n' (the text's end for a last line without one) */
    const int32_t *fmt_slot;  /* [n_records][5] FORMAT slots of GT, AD, RO, AO, GQ; -1: absent (all five on a line without a sample column) */
} uz_vcf_text_view;

/* The bytes of a decoded BCF and where the per-sample value arrays of GT, AD, RO, AO and GQ of every record lie in them (unfazed_io.h:
 * uz_vcf_samples_bcf; taken by unfazed_hip.h: uz_samples_from_bcf, which reads the values on the device).  A field's array holds, sample after
 * sample, `count` values of one BCF type: sample s starts at fld_at + s * count * size(type).  The decode has proven every array to lie inside
 * its record.  HOST pointers into the decoder's table: they live as long as it does. */
typedef struct uz_vcf_bcf_view {
    const uint8_t *data;
    int64_t data_bytes;
    int64_t n_records;
    int32_t n_samples;        /* samples the header names (= samples of every record that has FORMAT fields) */
    int32_t reserved0;
    const uint64_t *fld_at;   /* [n_records][5] offset of the value array of GT, AD, RO, AO, GQ in `data` */
    const uint32_t *fld_desc; /* [n_records][5] BCF type (1 int8, 2 int16, 3 int32, 5 float, 7 char) | values per sample << 4; 0: absent */
} uz_vcf_bcf_view;

/* The records of a decoded BCF and what their ids name (unfazed_io.h: uz_vcf_bcf_lines; taken by unfazed_hip.h: uz_bcf_rows, which turns every
 * record into its VCF text line on the device).  Names lie end to end in their byte block, name k at [off[k], off[k + 1]); an id the header
 * does not define is an empty name.  HOST pointers into the decoder's table: they live as long as it does. */
typedef struct uz_bcf_lines_view {
    const uint8_t *data;
    int64_t data_bytes;
    int64_t n_records;
    int32_t n_samples;           /* samples the header names */
    int32_t n_dict;              /* ids of the FILTER / INFO / FORMAT dictionary */
    const uint64_t *rec_at;      /* [n_records] offset of each record's l_shared word in `data`, ascending */
    const uint32_t *dict_off;    /* [n_dict + 1] */
    const uint8_t *dict_bytes;
    int32_t n_contigs;           /* the header's contigs, by id */
    int32_t reserved0;
    const uint32_t *contig_off;  /* [n_contigs + 1] */
    const uint8_t *contig_bytes;
} uz_bcf_lines_view;

/* alignment records of one BAM in file (coordinate) order */
typedef struct uz_reads_view {
    int64_t n_segs; /* < 2^31 */
    int32_t n_contigs;
    int32_t reserved0;
    const int64_t *contig_off; /* [n_contigs+1] */
    const int32_t *max_span;   /* [n_contigs] max(end-start) */
    const int32_t *start;      /* reference_start */
    const int32_t *end;        /* bam_endpos */
    const uint16_t *flag;
    const uint8_t *mapq;
    const uint8_t *aux;        /* UZ_AUX_* */
    const int32_t *tlen;
    const uint32_t *qname;     /* interned query-name id */
    const int32_t *mate;       /* record pysam's mate() returns, -1 = ValueError */
    const uint32_t *cigar_off;
    const uint16_t *n_cigar;
    const uint32_t *cigar;     /* BAM encoding len<<4|op */
    const uint16_t *l_seq;
    const uint32_t *sq_off16;  /* row offset into seq/qual in 16-byte units */
    const uint8_t *seq;        /* ASCII */
    const uint8_t *qual;
    int64_t n_cigar_total;
    int64_t n_sq_bytes;
    uint32_t n_qnames;
    uint32_t reserved1;
} uz_reads_view;

/* ---- packed alignment records: the STAGED ("pre-decoded") form, and the only form kept in HBM -------------
 *
 * What crosses the host link per record is what the path can ever look at:
 *   - bases stay in BAM's own 4-bit codes ("=ACMGRSVTWYHKDBN", high nibble first): the decoder does not expand
 *     them, and every use is an equality test against a REF / ALT character (read_collector.py:56-73, :98-141,
 *     snv_phaser.py:28-44);
 *   - base qualities are reduced to the one comparison the reference ever makes with them, `qual <
 *     MIN_BASE_QUAL` (= --min-gt-qual: goodread read_collector.py:43-46, connect_reads :123,
 *     indel_match_alleles :281-284): one bit per base, built by the decoder for the threshold of the run;
 *   - CIGAR words and rows lie back to back in record order, so their offsets are prefix sums the device
 *     computes itself (no offset columns on the link).
 * 132 bytes per 151-base record instead of 370 for the ASCII form (uz_reads_view).
 * Row geometry: a record of l_seq bases owns UZ_ROW_UNITS(l_seq) units of 32 bases = 16 bytes of seq4 and
 * 4 bytes of qlow per unit; bits / nibbles beyond l_seq are zero.  A record without SEQ / QUAL / CIGAR
 * (UZ_AUX_DECODE_BAD) has l_seq = 0 and n_cigar = 0. */
#define UZ_ROW_UNITS(l_seq) (((uint32_t)(l_seq) + 31u) >> 5)
#define UZ_SEQ4_UNIT_BYTES 16
#define UZ_SEQ2_UNIT_BYTES 8
#define UZ_QLOW_LIST_MAX 10 /* = the constant of goodread (read_collector.py:46) */
#define UZ_QLOW_UNIT_BYTES 4

typedef struct uz_reads_packed_view {
    int64_t n_segs; /* < 2^31 */
    int32_t n_contigs;
    int32_t min_base_qual;     /* threshold qlow was built with; uz_phase refuses a different --min-gt-qual */
    const int64_t *contig_off; /* [n_contigs+1] */
    const int32_t *max_span;   /* [n_contigs] */
    const int32_t *start;
    const int32_t *end;        /* may be NULL: the device then derives it as htslib's bam_endpos does -- start + 1 for an unmapped record or one
                                * without CIGAR, else start + max(1, reference bases of the CIGAR) -- which is what a BAM decoder fills in */
    const int32_t *tlen;
    const int32_t *mate;
    const uint32_t *qname;
    const uint16_t *flag;
    const uint16_t *l_seq;
    const uint16_t *n_cigar;
    const uint8_t *mapq;
    const uint8_t *aux;
    const uint32_t *cigar; /* [n_cigar_total] record i owns the next n_cigar[i] words */
    const uint8_t *seq4;   /* [n_seq_units * 16] rows of the records WITHOUT UZ_AUX_NO_SEQ, back to back; base k of a row: byte k>>1, high nibble when k is even */
    const uint8_t *qlow;   /* [n_row_units * 4]  rows of ALL records; base k of a row: bit k&7 of byte k>>3, set iff qual[k] < min_base_qual */
    int64_t n_cigar_total; /* = sum n_cigar, < 2^32 */
    int64_t n_row_units;   /* = sum UZ_ROW_UNITS(l_seq) over all records, < 2^32 */
    int64_t n_seq_units;   /* = the same sum over the records that carry bases (= n_row_units when none is UZ_AUX_NO_SEQ) */
    uint32_t n_qnames;
    uint32_t reserved1;
    /* The bases in TWO bits -- an alternative to seq4 for the host link (exactly one of seq4 / seq2 is non-null when
     * n_seq_units > 0).  Aligned reads are A/C/G/T but for the odd N: a row stores 2-bit codes (A 0, C 1, G 2, T 3; base k of
     * a row: byte k>>2, bits 7-6 for k&3 == 0 down to bits 1-0; 8 bytes per unit of 32 bases) and every base that is not one
     * of the four is listed apart with its BAM 4-bit code (its 2-bit field is 0).  The device expands the rows to seq4 and
     * patches the listed bases in: lossless, half the bytes of the largest column. */
    const uint8_t *seq2;      /* [n_seq_units * 8] rows of the records WITHOUT UZ_AUX_NO_SEQ, back to back */
    const uint32_t *exc_rec;  /* [n_exc] record index, ascending (ties: ascending exc_pos) */
    const uint16_t *exc_pos;  /* [n_exc] base index within the record */
    const uint8_t *exc_code;  /* [n_exc] BAM 4-bit code of that base ("=ACMGRSVTWYHKDBN") */
    int64_t n_exc;
    /* The quality plane as lists -- an alternative to qlow for the host link (exactly one of qlow / n_low is non-null).
     * The path asks two things of the base qualities: HOW MANY bases of a record lie below the threshold (goodread,
     * read_collector.py:43-46: more than 10 and the record is never "good"), and, for a good record that carries its bases,
     * WHETHER base k does (:123, :281-284).  So: the count of every record (saturated at 255), and the positions themselves
     * only for the records that carry bases (not UZ_AUX_NO_SEQ) and have at most UZ_QLOW_LIST_MAX of them -- ascending, back to
     * back in record order, one byte each (two, little-endian, when qlow_pos_wide: reads longer than 256 bases).  A 151-base
     * read costs 1 + ~5 bytes instead of 20.  The device rebuilds plane rows for the listed records; a kernel that asks for a
     * bit of any other record raises UZ_E_STATE (it would contradict goodread).
     * For tables that serve batches of POINT variants only: collect_reads_snv takes "good" records on both ends (:397-404), so
     * every pair the chaining can reach is good.  collect_reads_sv takes its evidence under goodread(read, True) (:503, :512),
     * which does not count qualities, and connect_reads may then test a base of such a record (:114-124): an SV batch needs the
     * plane (qlow). */
    const uint8_t *n_low;     /* [n_segs] */
    const uint8_t *qlow_pos;  /* [n_qlow_pos] (* 2 bytes when qlow_pos_wide) */
    int64_t n_qlow_pos;
    int32_t qlow_pos_wide;
    int32_t cigar_compact;    /* 1: a record whose CIGAR is one M / = / X operation spanning the read (98 % of a short-read file) carries the
                               * operation in its aux byte (UZ_AUX_SIMPLE_*) and owns NO word in `cigar`; n_cigar_total counts the words that
                               * are there, n_cigar_omitted the ones that are not; the device writes them back (len = l_seq) */
    /* Which 32-base units of a record's base row were staged (NULL: every unit of every record; needs the list form of the
     * qualities).  The read stage reads the bases of a record only at the fetch points it overlaps -- the DNM position (plus
     * the length of the longer allele) and the het sites of the window -- so a selection made from those fetches can leave the
     * other units of a 151-base read (usually four of its five) at home.  Bit u = unit u (bases 32u .. 32u+31) for a read of up
     * to 480 bases; UZ_UMASK_ALL (0xFFFF) = every unit (any length; what a record with a multi-operation CIGAR gets).  The base
     * row then holds the staged units back to back; n_seq_units counts staged units; exc_* entries in other units are ignored.
     * A kernel that asks for a base of a unit that stayed home raises UZ_E_STATE.
     * The quality lists follow the mask: of a listed record only the positions INSIDE its staged units need to travel (the
     * quality row the device rebuilds has no other units), and n_low of such a record may be the length of that shorter
     * list instead of the full count -- all the read filter asks of the count is "at most UZ_QLOW_LIST_MAX", which a
     * subset keeps true (uz_reads_select_* stages them so; a record with more than UZ_QLOW_LIST_MAX keeps its full,
     * saturated count and no list). */
    const uint16_t *umask;    /* [n_segs] */
    int64_t n_cigar_omitted;  /* cigar_compact: records with a simple code (each stands for one word) */
    /* The small columns as a dictionary (NULL: the plain columns).  flag, l_seq, n_cigar, mapq, aux and n_low take a few hundred
     * distinct combinations in a whole alignment file (four pairing flags x a handful of mapping qualities and low-quality
     * counts, one read length, one CIGAR operation): a record then carries a 16-bit index into a table of the combinations it
     * uses instead of the nine bytes (tup set => flag, l_seq, n_cigar, mapq, aux and n_low are NULL; tup_n_low is NULL when the
     * qualities travel as the plane).  At most 65536 combinations per table: a packer that meets more keeps the columns. */
    const uint16_t *tup;         /* [n_segs] */
    const uint16_t *tup_flag;    /* [n_tup] */
    const uint16_t *tup_l_seq;
    const uint16_t *tup_n_cigar;
    const uint8_t *tup_mapq;
    const uint8_t *tup_aux;
    const uint8_t *tup_n_low;
    int64_t n_tup;
    const uint16_t *tup_umask;   /* [n_tup] optional: the unit mask joins the combination too (umask is then NULL) */
    /* The four wide columns as 16-bit differences (NULL: the plain columns; set all four or none, and then start / tlen / mate / qname
     * are NULL).  In a coordinate-sorted table a record starts within a few bases of the one before it, its name id lies a few
     * hundred from its neighbour's, its mate a few hundred records away, and a template is a few hundred bases long:
     *   start_d[i] = start[i] - start[i-1], qname_d[i] = qname[i] - qname[i-1] (modulo 2^32; the values before record 0 are 0),
     *   mate_d[i] = mate[i] - i (UZ_D16_NONE: no mate), tlen_s[i] = tlen[i].
     * A value that does not fit is UZ_D16_ESC in the column and stands in the escape list: key = record << 2 | column (0 start,
     * 1 tlen, 2 mate, 3 qname), ascending; value = what the 16 bits could not hold (the same difference / tlen / mate index). */
    const int16_t *start_d;
    const int16_t *tlen_s;
    const int16_t *mate_d;
    const int16_t *qname_d;
    const uint64_t *esc16_key;   /* [n_esc16] */
    const int32_t *esc16_val;
    int64_t n_esc16;
    /* start_d in eight bits (then start_d is NULL; tlen_s / mate_d / qname_d as above): consecutive records of a pile-up start a
     * few bases apart, so the difference is 0 .. 254 for all but the first record of a region; UZ_D8_ESC (255) = in the escape
     * list (column 0), as for start_d. */
    const uint8_t *start_d8;
    /* mate_d and qname_d in eight bits (then mate_d / qname_d are NULL; set both or none, with start_d8): a selection keeps about a
     * third of a pile-up, so a mate lies within +-75 kept records and a name id within +-40 of the record's before it -- signed
     * bytes, UZ_D8S_ESC (-128) = in the escape list (columns 2 / 3, as for the 16-bit form), UZ_D8S_NONE (-127) = no mate. */
    const int8_t *mate_d8;
    const int8_t *qname_d8;
    /* tlen, mate and name id of a record in ONE byte -- the pair form (with start_d8; then tlen_s / mate_d / qname_d / mate_d8 /
     * qname_d8 are NULL).  Nearly every record of a short-read file is one of two mates that name each other, carry one query name
     * nobody before them carried, and a template length that is the span of the pair; and name ids are handed out by first
     * appearance, so a new name's id is the number of new names before it.  pair_d8[i]:
     *   1 .. UZ_P8_MAX_DIST  FIRST of such a pair: mate = i + pair_d8[i]; a new name; tlen = max(end[i], end[mate]) - start[i]
     *   UZ_P8_SECOND (0)     SECOND of such a pair: the record naming it as its mate is its mate; the same name id; tlen = -(its mate's)
     *   UZ_P8_SECOND_TLEN (253)  the same, of a pair whose template lengths are +-t for some other t (soft clips, another aligner's
     *                        convention): its own tlen stands in the escape list (column 1), its mate's is the negative
     *   UZ_P8_NEW (254)      any other record with a new name: tlen and mate stand in the escape list (columns 1 and 2; mate -1 = none)
     *   UZ_P8_OLD (255)      any other record: tlen, mate and name id stand in the escape list (columns 1, 2 and 3: the id itself)
     * A packer gives a pair the first two codes only when every one of those statements holds for it (both directions of the mate
     * link, the distance, both template lengths), so the form is lossless; the device checks that every SECOND is named by exactly one
     * FIRST (UZ_E_STATE otherwise).  A 151-base pair costs 2 bytes here instead of 8. */
    const uint8_t *pair_d8;
    /* The bases of a record as a LIST -- per record an alternative to its staged row units (needs umask or tup_umask, and seq2).
     * The read stage reads a record's bases at the fetch points it overlaps and nowhere else: the DNM position (plus the longer
     * allele) and the het sites of the window -- one or two bases of a 151-base read, where its staged 32-base unit is 8 bytes.
     * A record with bl_n[i] = k > 0 (tup_n_bl through the dictionary) sends those k bases instead: their query indices (bl_pos,
     * ascending within the record, records in order; one byte each, two little-endian when bl_wide) and their two-bit codes
     * (bl_code: entry e of the table in bits 2 (e & 3) .. 2 (e & 3) + 1 of byte e >> 2; A 0, C 1, G 2, T 3; a base that is none of
     * the four is 0 here and stands in exc_*).  Such a record owns NO units in seq2; its umask still names the units its bases lie
     * in, the device lays those units out behind the ones that travelled as rows and writes the listed bases into them
     * (n_bl_units = sum of popcount(umask) over the records with a list).  A packer lists a record only when every listed position
     * lies in a unit of its mask, every unit of the mask holds a listed position, and no listed base is '=' (BAM code 0): the device
     * marks the record, and a kernel that asks for a base of it that was not listed reads code 0 and raises UZ_E_STATE -- the
     * staging rule and the kernel cannot disagree silently.  k = 0: the record's units travel as rows, as before. */
    const uint8_t *bl_n;       /* [n_segs], or NULL with tup_n_bl */
    const uint8_t *tup_n_bl;   /* [n_tup] */
    const uint8_t *bl_pos;     /* [n_bl] (* 2 bytes when bl_wide) */
    const uint8_t *bl_code;    /* [(n_bl + 3) / 4] */
    /* The quality bits of the listed bases -- optional (NULL: the form above).  The read stage asks for a quality bit only where it asks for
     * a base, so a record with a base list needs its bits at the listed positions and nowhere else: entry e of the bl_* table is bit e & 7
     * of byte e >> 3, set iff that base's quality lies below min_base_qual.  With the column set, a record with listed bases (k > 0) owns NO
     * entries in qlow_pos (quantity 3 of its pk_sums share is 0), and the count that travels for it (n_low / tup_n_low) is the number of its
     * set bits when the whole read has at most UZ_QLOW_LIST_MAX low-quality bases -- a subset keeps "at most UZ_QLOW_LIST_MAX" true -- or the
     * read's own (saturated) count when it has more: all its bits are then 0 and it gets no quality row, as before.  The device writes the
     * quality words of such a record's units from the bits as it writes their base rows, and holds the bits against the count (UZ_E_RANGE).
     * Records without a base list keep their entries in qlow_pos.  Needs bl_pos / bl_code. */
    const uint8_t *bl_qlow;    /* [(n_bl + 7) / 8] */
    int64_t n_bl;
    int64_t n_bl_units;
    int32_t bl_wide;
    int32_t reserved2;
    /* Span sums -- optional (NULL: the device computes them itself, one more pass over the small columns and a scan).  The header build lays the
     * records' variable-length parts out by the running sums of UZ_PK_SUMS per-record quantities: 0 CIGAR words, 1 row units, 2 base-row units
     * that travelled as rows, 3 listed low-quality positions (none for a record with a base list when bl_qlow is set), 4 CIGAR words that travelled (cigar_compact), 5 start differences and 6 name-id
     * differences / new names (difference forms; modulo 2^32 where a column is), 7 row units and 8 listed bases of the records whose bases came as a
     * list, 9 FIRST and 10 SECOND records of the pair form.  A packer knows them as it packs: pk_sums[UZ_PK_SUMS * b + k] = quantity k summed over
     * the records in front of span b, spans of 1 << UZ_PK_SHIFT(n_segs) records, b = 0 .. n_pk_spans (the last row: the totals).
     * uz_packed_block_sums (unfazed_io.h) fills it for any view.  The device packs from these offsets and holds every span's own sums against the
     * next row as it goes (UZ_E_RANGE on a mismatch; no record is laid out beyond its span's share). */
    const uint64_t *pk_sums;
    int64_t n_pk_spans;
    /* The dictionary index in ONE byte -- optional, instead of `tup` (then NULL).  A few hundred of a table's thousands of combinations cover nearly
     * all of its records (bench workload: the 255 most frequent of 2 763 cover 98.2 %), so a record carries tup8[i] = k < 255: its combination is
     * tup_hot[k]; or 255: its combination is the next entry of tup_esc (the escaped records' indices in record order).  tup_esc_off[b] = escaped
     * records in front of span b, spans of UZ_TUP8_SPAN records, b = 0 .. ceil(n_segs / UZ_TUP8_SPAN) (the last entry: n_tup_esc).  The device
     * rebuilds the 16-bit column before the header build reads it and holds every span against its two offsets (UZ_E_RANGE on a mismatch, or on an
     * index beyond n_tup).  2 -> 1.04 bytes per record on the link. */
    const uint8_t *tup8;          /* [n_segs] */
    const uint16_t *tup_hot;      /* [256] (entries beyond the combinations in use: 0) */
    const uint16_t *tup_esc;      /* [n_tup_esc] */
    const uint32_t *tup_esc_off;  /* [ceil(n_segs / UZ_TUP8_SPAN) + 1] */
    int64_t n_tup_esc;
} uz_reads_packed_view;
#define UZ_TUP8_SPAN 1024
#define UZ_PK_SUMS 11
#define UZ_PK_SHIFT_LARGE 12
#define UZ_PK_SHIFT_SMALL 10
#define UZ_PK_SHIFT(n) ((((int64_t)(n)) >> UZ_PK_SHIFT_LARGE) >= 4096 ? UZ_PK_SHIFT_LARGE : UZ_PK_SHIFT_SMALL) /* records per span of the header build's passes: 1 << this */
#define UZ_UMASK_LISTED 0x8000u /* device only: set in a record's unit mask when its bases came as a list (masks name units 0 .. 14) */
#define UZ_P8_SECOND 0
#define UZ_P8_MAX_DIST 252
#define UZ_P8_SECOND_TLEN 253
#define UZ_P8_NEW 254
#define UZ_P8_OLD 255
#define UZ_D8S_ESC (-128)
#define UZ_D8S_NONE (-127)
#define UZ_D8_ESC 255
#define UZ_D16_ESC (-32768)
#define UZ_D16_NONE (-32767)
#define UZ_UMASK_ALL 0xFFFFu

/* one batch of DNMs of one kid (one family, one BAM) */
typedef struct uz_dnms_view {
    int32_t n;
    int32_t reserved0;
    const int32_t *contig;      /* sites-table contig id, -1 = contig absent from the sites file */
    const int32_t *rcontig;     /* reads-table contig id, -1 = absent */
    const int32_t *start;       /* 0-based */
    const int32_t *end;
    const uint8_t *vartype;     /* UZ_VT_* */
    const uint8_t *dflags;      /* UZ_DF_* */
    const uint8_t *mult;        /* list-entry multiplicity (1; >1 reproduces find_many's duplicate appends) */
    const uint32_t *allele_off; /* [2n+1]: REF of DNM d = alleles[off[2d]..off[2d+1]), ALT = [off[2d+1]..off[2d+2]) */
    const uint8_t *alleles;
    double cutoff;              /* concordant_upper_len of this kid (read_collector.py:11-25) */
} uz_dnms_view;

/* one kid of a cohort batch (uz_phase_cohort) */
typedef struct uz_cohort_group {
    int32_t fam_id;    /* the kid's trio columns (uz_family_upload) */
    int32_t reads_id;  /* the kid's alignment records */
    int32_t dnm_first; /* its DNMs: [dnm_first, dnm_first + dnm_count) of the batch */
    int32_t dnm_count;
    double cutoff;     /* concordant_upper_len of the kid (read_collector.py:11-25) */
} uz_cohort_group;

/* BED rows (uz_bed_rows): one row of the output per entry, in the caller's order.  Strings (chrom, vartype, kid, dad, mom) are ids into
 * the view's string table: string k is str_bytes[str_off[k] .. str_off[k + 1]). */
typedef struct uz_bed_row {
    int32_t dnm;        /* the DNM's index in the batch; -1: a SEX-CHROM row (summarize_autophased), which reads no batch */
    int32_t start, end; /* printed as Python's str(int) */
    uint32_t chrom, vartype, kid, dad, mom;
    int32_t reads_id;   /* the reads table the row's read ids name (verbose rows; a cohort batch: the group's own table); -1: none */
    int32_t sex_origin; /* SEX-CHROM rows: 0 = dad is origin_parent (chrY), 1 = mom */
} uz_bed_row;
typedef struct uz_bed_view {
    int64_t n_rows;
    const uz_bed_row *rows;
    int32_t n_strings;
    const uint32_t *str_off; /* [n_strings + 1], ascending */
    const uint8_t *str_bytes;
} uz_bed_view;

#ifdef __cplusplus
}
#endif
#endif /* UZ_TYPES_H */
