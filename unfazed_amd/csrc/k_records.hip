// k_records.hip -- the header build on gfx950: everything that turns the staged columns of a reads view into the table the read stage
// (k_reads.hip) searches -- record headers, search index, base and quality rows -- plus the host-side launches (uz_ctx.hpp: uz_build_records
// and its neighbours).
//
// Two kernels build the same headers from the same columns: k_pack_rec reads a record's parts where they lie in memory, k_pack_link (the form
// every packer of the product emits) from its span's slices in LDS.  Each rule of the link form is stated ONCE, as a pk_* function in front
// of the two, which takes the place its operands are read from as an accessor; both builds call every one of them.
#include "uz_ctx.hpp"
#include "phase_body.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {

__global__ void k_build_coarse(const RecA *ra, int64_t n, int32_t *coarse, int32_t *mid_idx, int32_t *mid8) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((k << 3) < n) {
        const int32_t st = ra[k << 3].start;
        mid8[k] = st;
        if ((k & 7) == 0) mid_idx[k >> 3] = st;
        if ((k & 511) == 0) coarse[k >> 9] = st;
    }
}

// ---- record headers from the staged columns -------------------------------------------------------------
// cigar_off / sq_off are the exclusive prefix sums of n_cigar / UZ_ROW_UNITS(l_seq) over the records: block
// sums, one scan of the block sums, then the pack kernel scans inside its block and writes the headers.
// A span of records is one workgroup's share of the two passes below.  4096 for a table that fills the chip with such spans (a chunk
// of the 100 k-DNM pass: 23 M records, 5.6 k spans; 1024 / 2048 measured slower there: more sums to scan), 1024 for a smaller one --
// the 5 M records of a config-5 chunk are 1.2 k spans of 4096, five 256-lane workgroups per CU, and the pack pass ran at a third of
// its rate per record.
static inline int uz_pk_shift(int64_t n) { return UZ_PK_SHIFT(n); } // (uz_types.h: the packers cut their span sums the same way)
// four running sums per record: CIGAR words, quality-plane units (every record), seq4 units (records with bases), listed
// low-quality positions (list form of the staged plane: records with bases and at most UZ_QLOW_LIST_MAX of them; nl < 0: plane form)
// ... and, fifth, the CIGAR words that travelled (cigar_compact: a record with a simple code owns none); sixth and seventh, the
// differences of start and of the name id to the record before (16-bit difference form: the columns are their running sums,
// modulo 2^32; pair form: the sixth counts the NEW names, a new name's id being the number of new names before it); eighth and
// ninth, the row units and the listed bases of the records whose bases came as a list (bl_*: their units are laid out behind the
// ones that travelled as rows); tenth and eleventh, the FIRST and SECOND records of the pair form (their totals must agree)
#define UZ_PK_SCANNED 9 // the running sums the header build needs per record (the last two are totals only)
// um: which units of the record's rows were staged (UZ_UMASK_ALL: all of them)
// blq: the quality bits of listed bases ride with them (uz_types.h bl_qlow): a record with a base list owns no listed positions
__device__ __forceinline__ void pk_vals(uint32_t nc, uint32_t ls, uint32_t aux, int nl, uint32_t um, uint32_t nb, bool blq, uint32_t (&v)[UZ_PK_SUMS]) {
    v[4] = (aux & UZ_AUX_SIMPLE_MASK) ? 0u : nc;
    v[5] = 0u; v[6] = 0u; v[9] = 0u; v[10] = 0u; // (set by the callers from the difference columns)
    const uint32_t staged = (aux & UZ_AUX_NO_SEQ) ? 0u : (um == UZ_UMASK_ALL ? UZ_ROW_UNITS(ls) : (uint32_t)__popc(um));
    v[0] = nc; v[1] = UZ_ROW_UNITS(ls);
    v[2] = nb ? 0u : staged; // units that travelled as rows
    v[7] = nb ? staged : 0u; // units of a record whose bases came as a list
    v[8] = nb;
    v[3] = (nl >= 0 && !(aux & UZ_AUX_NO_SEQ) && nl <= UZ_QLOW_LIST_MAX && !(blq && nb)) ? (uint32_t)nl : 0u;
}
// the small columns of record i, plain or through the dictionary (uz_reads_packed_view.tup)
struct RecSmall { uint32_t flag, ls, nc, mapq, aux, um; int nl; uint32_t nb; };
// ... of record i whose dictionary index is already at hand
__device__ __forceinline__ RecSmall rec_small_of(const RecColumns &c, int64_t i, uint32_t t) {
    RecSmall r;
    r.flag = c.tup_flag[t]; r.ls = c.tup_l_seq[t]; r.nc = c.tup_n_cigar[t]; r.mapq = c.tup_mapq[t]; r.aux = c.tup_aux[t];
    r.nl = c.lists ? (int)c.tup_n_low[t] : -1;
    r.um = c.tup_umask ? (uint32_t)c.tup_umask[t] : (c.umask ? (uint32_t)c.umask[i] : UZ_UMASK_ALL);
    r.nb = c.tup_n_bl ? (uint32_t)c.tup_n_bl[t] : (c.bl_n ? (uint32_t)c.bl_n[i] : 0u);
    return r;
}
__device__ __forceinline__ RecSmall rec_small(const RecColumns &c, int64_t i) {
    if (c.tup) return rec_small_of(c, i, c.tup[i]);
    RecSmall r;
    r.flag = c.flag[i]; r.ls = c.l_seq[i]; r.nc = c.n_cigar[i]; r.mapq = c.mapq[i]; r.aux = c.aux[i];
    r.nl = c.lists ? (int)c.n_low[i] : -1;
    r.um = c.umask ? (uint32_t)c.umask[i] : UZ_UMASK_ALL;
    r.nb = c.bl_n ? (uint32_t)c.bl_n[i] : 0u;
    return r;
}
// the escape list of the 16-bit difference columns: value of (record, column).  The list is sorted by record, and esc_off (one entry
// per span of records, k_esc_block_off) bounds the search to the handful of entries of the record's own span: a lane that meets
// an escape costs its wave two or three loads instead of a binary search over the whole list
__device__ __forceinline__ int32_t esc16_of(const RecColumns &c, int64_t i, int col) {
    const unsigned long long key = ((unsigned long long)i << 2) | (unsigned long long)col;
    int64_t lo = c.esc_lo, hi = c.esc_hi; // (the entries of the workgroup's own span: set by the kernels below)
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (c.esc16_key[mid] < key) lo = mid + 1; else hi = mid; }
    return (lo < c.n_esc16 && c.esc16_key[lo] == key) ? c.esc16_val[lo] : 0; // (a missing entry is caught by the totals / the mate check)
}
// first escape entry at or behind record `rec` (the list is sorted by record): every workgroup of the header build bounds the searches of
// its span with two of these, kept in LDS (a kernel of its own did that for all spans at once: one more small launch per table that had to
// wait for room beside the read stage's persistent workgroups)
__device__ __forceinline__ int64_t esc_lower_bound(const unsigned long long *__restrict__ key, int64_t n_esc, int64_t rec) {
    const unsigned long long want = (unsigned long long)rec << 2;
    int64_t lo = 0, hi = n_esc;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (key[mid] < want) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint32_t d16_val(const RecColumns &c, const int16_t *col, int64_t i, int k) {
    const int v = col[i];
    return (uint32_t)(v == UZ_D16_ESC ? esc16_of(c, i, k) : v);
}
// the pair byte of a record (uz_types.h UZ_P8_*): a SECOND takes mate, name and template length from the FIRST that names it; a FIRST names
// the SECOND p records on; every record but a SECOND or an OLD one brings a new name
__device__ __forceinline__ bool p8_second(uint32_t p) { return p == UZ_P8_SECOND || p == UZ_P8_SECOND_TLEN; }
__device__ __forceinline__ bool p8_first(uint32_t p) { return p >= 1u && p <= UZ_P8_MAX_DIST; }
__device__ __forceinline__ bool p8_new_name(uint32_t p) { return p != UZ_P8_SECOND && p != UZ_P8_SECOND_TLEN && p != UZ_P8_OLD; }
// the name-id difference of record i: sixteen bits, or eight (qname_d8); pair form: 1 for a record that brings a new name
__device__ __forceinline__ uint32_t qname_diff(const RecColumns &c, int64_t i) {
    if (c.pair_d8) return p8_new_name(c.pair_d8[i]) ? 1u : 0u;
    if (c.qname_d8) {
        const int v = c.qname_d8[i];
        return (uint32_t)(v == UZ_D8S_ESC ? esc16_of(c, i, 3) : v);
    }
    return d16_val(c, c.qname_d, i, 3);
}
// the start difference of record i: sixteen bits, or eight (start_d8)
__device__ __forceinline__ uint32_t start_diff(const RecColumns &c, int64_t i) {
    if (c.start_d8) {
        const uint32_t x = c.start_d8[i];
        return x == UZ_D8_ESC ? (uint32_t)esc16_of(c, i, 0) : x;
    }
    return d16_val(c, c.start_d, i, 0);
}
// The form every packer of the product emits (uz_bam_stage_*, uz_reads_select_* with its defaults): the small columns through the dictionary
// with unit masks and counts of low-quality bases, eight-bit start differences, the pair form, compact CIGARs, no `end`.  The header-build
// kernels are compiled once more for exactly that form: the pointers of every other form are known to be null there, their branches fall
// away, and what stays alive across the record loop fits the scalar registers (the general build of k_pack_rec spills 160 of them).
__host__ __device__ inline bool uz_link_form(const RecColumns &c) {
    return c.tup && c.tup_umask && c.tup_n_low && c.lists && c.start_d8 && c.pair_d8 && c.cigar_out && !c.end && !c.plane_in && !c.umask && !c.n_low && !c.bl_n &&
           !c.start && !c.start_d && !c.tlen_s && !c.mate_d8 && !c.qname_d8 && !c.flag;
}
template <bool LINK>
__device__ __forceinline__ RecColumns uz_columns_of(const RecColumns &in) {
    RecColumns c = in;
    if (LINK) {
        c.start = nullptr; c.end = nullptr; c.tlen = nullptr; c.mate = nullptr; c.qname = nullptr;
        c.flag = nullptr; c.l_seq = nullptr; c.n_cigar = nullptr; c.mapq = nullptr; c.aux = nullptr;
        c.umask = nullptr; c.start_d = nullptr; c.tlen_s = nullptr; c.mate_d = nullptr; c.qname_d = nullptr; c.mate_d8 = nullptr; c.qname_d8 = nullptr;
        c.plane_in = nullptr; c.n_low = nullptr; c.bl_n = nullptr; c.lists = 1;
        __builtin_assume(c.tup != nullptr); __builtin_assume(c.tup_umask != nullptr); __builtin_assume(c.tup_n_low != nullptr);
        __builtin_assume(c.start_d8 != nullptr); __builtin_assume(c.pair_d8 != nullptr); __builtin_assume(c.cigar_out != nullptr);
        __builtin_assume(c.cigar_in != nullptr);
    }
    return c;
}
// exclusive scan of the block sums in place by ONE workgroup of 256 lanes; the totals are checked against what the view declared
struct PkWant { unsigned long long cigar, units, seq, qpos, staged /* ~0: not compact */, bl_units, bl; };
// the totals of the span sums against what the view declared (by ONE lane of the table's build)
__device__ __forceinline__ void pk_totals_check(const unsigned long long (&tot)[UZ_PK_SUMS], const PkWant &want, int32_t *hflags) {
    if (tot[0] != want.cigar || tot[1] != want.units || tot[2] != want.seq || tot[3] != want.qpos || tot[0] > 0xFFFFFFFFULL || tot[1] > 0xFFFFFFFFULL ||
        (want.staged != ~0ULL && tot[4] != want.staged) || tot[7] != want.bl_units || tot[8] != want.bl || tot[1] + tot[7] > 0xFFFFFFFFULL)
        hflags[0] = 1;
    if (tot[9] != tot[10]) hflags[0] = 8; // pair form: as many SECOND records as FIRST ones (k_pair_link checks that they are each other's)
}
__device__ __forceinline__ void scan_block_sums(int64_t nb, unsigned long long *sums, const PkWant &want, int32_t *hflags) {
    __shared__ unsigned long long wpart[UZ_PK_SUMS][4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t chunk = (nb + 255) / 256;
    const int64_t lo = t * chunk < nb ? t * chunk : nb, hi = lo + chunk < nb ? lo + chunk : nb;
    unsigned long long v[UZ_PK_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, inc[UZ_PK_SUMS];
    for (int64_t i = lo; i < hi; i++)
        for (int k = 0; k < UZ_PK_SUMS; k++) v[k] += sums[UZ_PK_SUMS * i + k];
#pragma unroll
    for (int k = 0; k < UZ_PK_SUMS; k++) { // inclusive scan inside the wave, then across the four waves
        unsigned long long x = v[k];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(x, o, 64); if (lane >= o) x += u; }
        inc[k] = x;
        if (lane == 63) wpart[k][wv] = x;
    }
    __syncthreads();
    unsigned long long tot[UZ_PK_SUMS];
#pragma unroll
    for (int k = 0; k < UZ_PK_SUMS; k++) {
        unsigned long long pre = 0, all = 0;
        for (int w = 0; w < 4; w++) { const unsigned long long x = wpart[k][w]; if (w < wv) pre += x; all += x; }
        v[k] = pre + inc[k] - v[k]; // exclusive prefix of this thread's blocks
        tot[k] = all;
    }
    if (t == 0) pk_totals_check(tot, want, hflags);
    for (int64_t i = lo; i < hi; i++)
        for (int k = 0; k < UZ_PK_SUMS; k++) {
            const unsigned long long x = sums[UZ_PK_SUMS * i + k];
            sums[UZ_PK_SUMS * i + k] = v[k];
            v[k] += x;
        }
}
template <bool LINK>
__global__ __launch_bounds__(256) void k_off_block_sums(int64_t n, RecColumns c_in, unsigned long long *sums /* [UZ_PK_SUMS nb] */) {
    RecColumns c = uz_columns_of<LINK>(c_in);
    __shared__ unsigned long long part[UZ_PK_SUMS][4];
    __shared__ int64_t esc_span[2];
    const int t = threadIdx.x;
    if (c.n_esc16 > 0 && t < 2) esc_span[t] = esc_lower_bound(c.esc16_key, c.n_esc16, ((int64_t)blockIdx.x + t) << c.pk_shift);
    __syncthreads();
    c.esc_lo = c.n_esc16 > 0 ? esc_span[0] : 0; c.esc_hi = c.n_esc16 > 0 ? esc_span[1] : 0;
    unsigned long long acc[UZ_PK_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // four records per lane at a time: their column bytes are requested together, then their dictionary entries, then the sums --
    // three round trips to memory for four records instead of three for each
    constexpr int U = 4;
    static_assert(((1 << UZ_PK_SHIFT_SMALL) / 256) % U == 0, "a span is a multiple of 1024 records");
    const int rounds = (1 << c.pk_shift) / 256;
    for (int it = 0; it < rounds; it += U) {
        int64_t idx[U];
        bool in[U];
        RecSmall r[U];
        uint32_t sd[U], pd[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            idx[u] = ((int64_t)blockIdx.x << c.pk_shift) + (it + u) * 256 + t;
            in[u] = idx[u] < n;
            if (!in[u]) idx[u] = n - 1; // (n > 0: the kernel is not launched on an empty table)
        }
        uint32_t tp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            tp[u] = c.tup ? (uint32_t)c.tup[idx[u]] : 0u;
            sd[u] = c.start_d8 ? (uint32_t)c.start_d8[idx[u]] : 0u;
            pd[u] = c.pair_d8 ? (uint32_t)c.pair_d8[idx[u]] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; u++) r[u] = c.tup ? rec_small_of(c, idx[u], tp[u]) : rec_small(c, idx[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!in[u]) continue;
            const int64_t i = idx[u];
            uint32_t v[UZ_PK_SUMS];
            pk_vals(r[u].nc, r[u].ls, r[u].aux, r[u].nl, r[u].um, r[u].nb, c.bl_qlow != nullptr, v);
            if (c.diff_form()) {
                v[5] = c.start_d8 ? (sd[u] == UZ_D8_ESC ? (uint32_t)esc16_of(c, i, 0) : sd[u]) : start_diff(c, i);
                v[6] = c.pair_d8 ? (p8_new_name(pd[u]) ? 1u : 0u) : qname_diff(c, i);
            }
            if (c.pair_d8) { v[9] = p8_first(pd[u]) ? 1u : 0u; v[10] = p8_second(pd[u]) ? 1u : 0u; }
#pragma unroll
            for (int k = 0; k < UZ_PK_SUMS; k++) acc[k] += v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < UZ_PK_SUMS; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
        if ((t & 63) == 0) part[k][t >> 6] = acc[k];
    }
    __syncthreads();
    if (t == 0)
        for (int k = 0; k < UZ_PK_SUMS; k++) sums[UZ_PK_SUMS * (size_t)blockIdx.x + k] = part[k][0] + part[k][1] + part[k][2] + part[k][3];
}
// (One workgroup.  Tried in round 4 and dropped: the scan done by whichever workgroup of k_off_block_sums finishes last.  The sums then cross
// between XCDs inside a kernel: with a __threadfence per workgroup every kernel of the step ran 20 - 50 % slower -- two thousand L2
// write-backs per table -- and with agent-scope accesses instead the lone scanning workgroup sat through ~180 uncached round trips.)
__global__ __launch_bounds__(256) void k_off_scan_sums(int64_t nb, unsigned long long *sums, PkWant want, int32_t *hflags) { scan_block_sums(nb, sums, want, hflags); }
// SELF: `sums` holds the raw block sums (no scan kernel ran): every workgroup adds up the sums of the blocks before its own -- a table of a
// few thousand spans costs each workgroup a few microseconds of L2 reads, where the one-workgroup scan kernel between the two passes waited
// ~100 us for room beside the read stage's persistent workgroups; the last workgroup holds the totals against what the view declared.
// pair form: FIRST record i hands its mate j (the SECOND it names) the link back, the name id and the template length
__device__ __forceinline__ void uz_pair_link_one(int64_t i, int64_t j, const uint8_t *__restrict__ pair, const RecA *ra, RecB *rb, int32_t *hflags) {
    if (atomicExch(&rb[j].mate, (int32_t)i) != -2) { hflags[0] = 8; return; } // not a SECOND record, or named twice
    const RecA A = ra[i], M = ra[j];
    if (pair[j] == UZ_P8_SECOND_TLEN) rb[i].tlen = -rb[j].tlen; // (the SECOND brought its own)
    else {
        const int32_t tl = (A.end > M.end ? A.end : M.end) - A.start;
        rb[i].tlen = tl;
        rb[j].tlen = -tl;
    }
    rb[j].qname = rb[i].qname;
}

// diagnostic build only (-DUZ_PACK_TIMING): shader-clock ticks of lane 0 per section of the header build, summed over the workgroups
#ifdef UZ_PACK_TIMING
__device__ unsigned long long uz_pack_ticks[16];
#define PK_TICK(k) do { if (threadIdx.x == 0) { const unsigned long long now__ = __builtin_amdgcn_s_memtime(); ptk__[k] += now__ - ptl__; ptl__ = now__; } } while (0)
#else
#define PK_TICK(k) ((void)0)
#endif

// ---- the rules of a header, stated once for the two builds below (k_pack_rec: operands from memory; k_pack_link: from its span's LDS) ----
// pair form -> mate, name id, template length.  qn0 comes in as the id of a NEW name (the new names before the record), esc(col) is the
// record's value of column col in the escape list.  A FIRST record knows its mate and its (new) name id, and gets its template length once
// every `end` is there; a SECOND record gets all three from the FIRST that names it (mate -2 until then)
template <typename Esc>
__device__ __forceinline__ void pk_pair_decode(uint32_t p, int64_t i, int64_t n, Esc esc, int32_t &mt0, uint32_t &qn0, int32_t &tl0, int32_t *hflags) {
    tl0 = 0;
    if (p == UZ_P8_SECOND) { mt0 = -2; qn0 = 0u; }
    else if (p == UZ_P8_SECOND_TLEN) { mt0 = -2; qn0 = 0u; tl0 = esc(1); }
    else if (p <= UZ_P8_MAX_DIST) {
        mt0 = (int32_t)(i + p);
        if (mt0 >= n) { hflags[0] = 7; mt0 = -1; }
    } else {
        tl0 = esc(1);
        mt0 = esc(2);
        if (p == UZ_P8_OLD) qn0 = (uint32_t)esc(3);
        if (mt0 < -1 || mt0 >= n) { hflags[0] = 7; mt0 = -1; }
    }
}
// one CIGAR word of a record: its share of the reference length and of the two CIGAR counts of the QC word
__device__ __forceinline__ void pk_cigar_take(uint32_t w, uint32_t ax, int64_t &ref_len, int &cig_nonmatch, int &cig_none) {
    const uint32_t op = w & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int64_t)(w >> 4); // M D N = X
    if (!(ax & UZ_AUX_DECODE_BAD)) uz_cigar_op_counts(w, cig_nonmatch, cig_none);
}
// `end` of a record whose column was left out: as htslib's bam_endpos -- uz_bam_endpos in pack.hpp states it for the host
__device__ __forceinline__ int32_t pk_end(uint32_t flag, uint32_t nc, bool have_words, int32_t st0, int64_t ref_len) {
    return ((flag & 4u) || nc == 0 || !have_words) ? st0 + 1 : (int32_t)(st0 + (ref_len > 0 ? ref_len : 1));
}
// the search index: start of every 4096th record (coarse), of every 64th (mid) and of every 8th (mid8)
__device__ __forceinline__ void pk_index_store(int64_t i, int32_t st0, int32_t *coarse, int32_t *mid_idx, int32_t *mid8) {
    if ((i & 7) == 0) {
        mid8[i >> 3] = st0;
        if ((i & 63) == 0) {
            mid_idx[i >> 6] = st0;
            if ((i & 4095) == 0) coarse[i >> 12] = st0;
        }
    }
}
// the unit mask as the readers get it, held against the read's length
__device__ __forceinline__ void pk_umask_store(int64_t i, uint32_t um, uint32_t nb, uint32_t ls, uint16_t *umask_out, int32_t *hflags) {
    const int units = (int)UZ_ROW_UNITS(ls);
    umask_out[i] = (uint16_t)(nb ? (um | UZ_UMASK_LISTED) : um);
    if (um != UZ_UMASK_ALL && (units > 15 || (um >> units) != 0u)) hflags[0] = 5; // a unit beyond the read, or a read too long for a mask
}
// List form of the staged plane: which record gets a quality row (at its base-row position) -- one whose bits can be asked for.  with_bits:
// its quality words are written with its base rows, from the bits of its listed bases (blq: the view has bl_qlow); else from its listed
// positions, which it owns when v3, its share of them (pk_vals), is its count
struct QRow { bool listed, with_bits; };
__device__ __forceinline__ QRow pk_qrow_rule(bool blq, uint32_t nb, uint32_t v3, int nl, uint32_t ax) {
    QRow q;
    q.with_bits = blq && nb != 0u;
    q.listed = nl >= 0 && (q.with_bits || v3 == (uint32_t)nl) && !(ax & UZ_AUX_NO_SEQ) && nl <= UZ_QLOW_LIST_MAX;
    return q;
}
// The listed bases -> the record's rows from `sq` on (one 16-byte row per unit of its mask; bases that were not listed stay code 0, which
// the readers of a listed record refuse: phase_body.hpp uz_base).  Positions ascend, so the units come in row order.  pos(e), code(e), qbit(e):
// entry e of the record's list.  With bits, the quality word of a unit is gathered beside its base row and stored with it -- for a record
// that gets a quality row at all -- and the set bits are held against the count: as many as it says, none for a record without a row.
// (The record's values by reference: by value the general build of k_pack_rec took two registers more.)
template <typename Pos, typename Code, typename QBit>
__device__ __forceinline__ void pk_listed_rows(const uint32_t &nb, const uint32_t &ls, const uint32_t &um, const uint32_t &ax, const uint32_t &sq, const QRow &qr, const int &nl,
                                               Pos pos, Code code, QBit qbit, uint32_t *seq4_out, uint32_t *plane_out, int32_t *hflags) {
    if (um == UZ_UMASK_ALL || (ax & UZ_AUX_NO_SEQ)) { hflags[0] = 9; return; }
    uint32_t w4r[4] = {0u, 0u, 0u, 0u};
    int cur = -1, last = -1;
    uint32_t row = sq, seen = 0u;
    bool bad = false;
    uint32_t qw = 0u; // the unit's quality word
    int bl_low = 0;   // ... and the set bits of the record
    const bool qrow = qr.with_bits && qr.listed;
    for (uint32_t e = 0; e < nb; e++) {
        const int ps = pos(e);
        const uint32_t cd = code(e), qb = qr.with_bits ? qbit(e) : 0u;
        const int u = ps >> 5;
        bad |= ps <= last || ps >= (int)ls || u > 14 || !((um >> u) & 1u);
        last = ps;
        if (u != cur) {
            if (cur >= 0) {
                reinterpret_cast<uint4 *>(seq4_out)[row] = make_uint4(w4r[0], w4r[1], w4r[2], w4r[3]);
                w4r[0] = w4r[1] = w4r[2] = w4r[3] = 0u;
                if (qrow) plane_out[(size_t)row] = qw;
                qw = 0u;
                row++;
            }
            cur = u;
            seen |= 1u << (u & 15);
        }
        const int k32 = ps & 31; // byte k32 >> 1 of the row, high nibble when k32 is even
        w4r[k32 >> 3] |= (1u << cd) << (8 * ((k32 >> 1) & 3) + ((k32 & 1) ? 0 : 4));
        qw |= qb << k32;
        bl_low += (int)qb;
    }
    if (cur >= 0) {
        reinterpret_cast<uint4 *>(seq4_out)[row] = make_uint4(w4r[0], w4r[1], w4r[2], w4r[3]);
        if (qrow) plane_out[(size_t)row] = qw;
    }
    if (bad || seen != um) hflags[0] = 9; // a position outside the mask / not ascending, or a unit of the mask without a listed base
    if (qr.with_bits && nl >= 0 && bl_low != (qr.listed ? nl : 0)) hflags[0] = 4;
}
// f(e) for the entries e < n of a record's list: in a loop (NE = 0), or unrolled NE times for a caller that keeps the list in registers
template <int NE, typename F>
__device__ __forceinline__ void pk_each(int n, F f) {
    if constexpr (NE > 0) {
#pragma unroll
        for (int e = 0; e < NE; e++) if (e < n) f(e);
    } else
        for (int e = 0; e < n; e++) f(e);
}
// The quality list of a record -> its plane rows from `sq` on: the row holds the same units as the base row, the staged ones.  pos(e): listed
// position e of the record
template <int NE, typename Pos>
__device__ __forceinline__ void pk_qlist_rows(int nl, uint32_t ls, uint32_t um, uint32_t sq, Pos pos, uint32_t *plane_out, int32_t *hflags) {
    bool bad = false;
    int prev = -1;
    pk_each<NE>(nl, [&](int e) { const int ps = pos(e); bad |= ps >= (int)ls || ps <= prev; prev = ps; });
    if (bad) hflags[0] = 4;
    uint32_t at_row = sq;
    auto row_word = [&](int u) { // the bits of unit u
        uint32_t w = 0;
        pk_each<NE>(nl, [&](int e) { const int ps = pos(e); if ((ps >> 5) == u) w |= 1u << (ps & 31); });
        return w;
    };
    if (um != UZ_UMASK_ALL) { // one round per staged unit (usually one or two of a read's five)
        uint32_t m = um;
        while (m) { const int u = __ffs((int)m) - 1; m &= m - 1u; plane_out[(size_t)at_row++] = row_word(u); }
    } else
        for (int u = 0; u < (int)UZ_ROW_UNITS(ls); u++) plane_out[(size_t)at_row++] = row_word(u);
}
// The dictionary index in one byte (uz_types.h tup8) back to sixteen bits, for the span of UZ_TUP8_SPAN records of this workgroup: four records
// per lane, an escaped record's place in the escape list = the span's offset + the escapes in front of it inside the span (a block scan of the
// lanes' counts).  store(k, v): the index of the lane's k-th record.  A span whose escapes are not the number its two offsets name, an escape
// beyond the list, an index beyond the dictionary: hflags[0] (UZ_E_RANGE at the table's first use)
template <typename Store>
__device__ __forceinline__ void pk_tup8_expand(int64_t n, const uint8_t *__restrict__ tup8, const uint16_t *__restrict__ hot, const uint16_t *__restrict__ esc,
                                               const uint32_t *__restrict__ esc_off, int64_t n_esc, int32_t n_tup, int32_t *hflags, Store store) {
    __shared__ uint16_t s_hot[256];
    __shared__ uint32_t s_tsum[4];
    static_assert(UZ_TUP8_SPAN == 4 * 256, "four records per lane");
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    s_hot[t] = hot[t];
    const int64_t base = (int64_t)blockIdx.x * UZ_TUP8_SPAN + 4 * t;
    uint32_t w = 0;
    if (base + 4 <= n) w = *reinterpret_cast<const uint32_t *>(tup8 + base);
    else for (int k = 0; k < 4; k++) if (base + k < n) w |= (uint32_t)tup8[base + k] << (8 * k);
    uint32_t ne = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) ne += (base + k < n && ((w >> (8 * k)) & 0xFFu) == 255u) ? 1u : 0u;
    const uint32_t inc = wv_incl_scan(ne);
    if (lane == 63) s_tsum[wv] = inc;
    __syncthreads();
    uint32_t before = inc - ne;
    for (int k = 0; k < wv; k++) before += s_tsum[k];
    const uint32_t x0 = esc_off[blockIdx.x], x1 = esc_off[blockIdx.x + 1];
    if (t == 255 && before + ne != x1 - x0) hflags[0] = 1;
    uint32_t at = x0 + before;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b = (w >> (8 * k)) & 0xFFu;
        uint32_t val = s_hot[b];
        if (b == 255u && base + k < n) {
            if ((int64_t)at < n_esc && at < x1) val = esc[at];
            else { val = 0; hflags[0] = 1; }
            at++;
        }
        if (val >= (uint32_t)n_tup) { val = 0; if (base + k < n) hflags[0] = 1; }
        store(k, val);
    }
}

template <bool LINK, bool SELF>
__global__ __launch_bounds__(256) void k_pack_rec(int64_t n, RecColumns c_in, const unsigned long long *__restrict__ sums, PkWant want, RecA *ra, RecB *rb,
                                                  uint32_t *fm, uint32_t *qoff, uint8_t *nlow, uint16_t *umask_out, uint32_t *plane_out,
                                                  uint16_t *qs, int32_t *coarse, int32_t *mid_idx, int32_t *mid8, int32_t *hflags, int host_sums) {
    RecColumns c = uz_columns_of<LINK>(c_in);
    __shared__ uint32_t wsum[UZ_PK_SCANNED][4];
    __shared__ int64_t esc_span[2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#ifdef UZ_PACK_TIMING
    unsigned long long ptk__[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ptl__ = __builtin_amdgcn_s_memtime();
#endif
    if (c.n_esc16 > 0 && t < 2) esc_span[t] = esc_lower_bound(c.esc16_key, c.n_esc16, ((int64_t)blockIdx.x + t) << c.pk_shift);
    __syncthreads();
    c.esc_lo = c.n_esc16 > 0 ? esc_span[0] : 0; c.esc_hi = c.n_esc16 > 0 ? esc_span[1] : 0;
    unsigned long long run[UZ_PK_SCANNED];
    if constexpr (SELF) {
        __shared__ unsigned long long pre_s[UZ_PK_SUMS][4];
        unsigned long long acc[UZ_PK_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const bool last = blockIdx.x + 1 == gridDim.x;
        const int64_t nbk = (int64_t)blockIdx.x + (last ? 1 : 0); // (the last workgroup adds its own block too: the totals)
        for (int64_t b = t; b < nbk; b += 256) {
            unsigned long long row[UZ_PK_SUMS];
#pragma unroll
            for (int k = 0; k < UZ_PK_SUMS; k++) row[k] = sums[UZ_PK_SUMS * (size_t)b + k];
#pragma unroll
            for (int k = 0; k < UZ_PK_SUMS; k++) acc[k] += row[k];
        }
        // (the last workgroup's own block: part of the totals, not of its prefix)
        unsigned long long own[UZ_PK_SUMS];
#pragma unroll
        for (int k = 0; k < UZ_PK_SUMS; k++) own[k] = last ? sums[UZ_PK_SUMS * (size_t)blockIdx.x + k] : 0ULL;
#pragma unroll
        for (int k = 0; k < UZ_PK_SUMS; k++) {
            unsigned long long x = acc[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
            if (lane == 0) pre_s[k][wv] = x;
        }
        __syncthreads();
        unsigned long long tot[UZ_PK_SUMS];
#pragma unroll
        for (int k = 0; k < UZ_PK_SUMS; k++) tot[k] = pre_s[k][0] + pre_s[k][1] + pre_s[k][2] + pre_s[k][3];
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) run[k] = tot[k] - own[k];
        if (last && t == 0) pk_totals_check(tot, want, hflags);
    } else {
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) run[k] = sums[UZ_PK_SUMS * (size_t)blockIdx.x + k];
    }
    // host_sums: the offsets come from the packer (uz_types.h pk_sums; the host has checked that the rows ascend and end at the declared totals).
    // Every record's variable-length parts must then end in front of the NEXT span's offsets -- nothing is read or written beyond the span's share
    // -- and the span's own sums must add up to exactly that row: a packer that counted wrong is refused, whatever it counted.
    // (the next row sits in LDS: eighteen registers less across the record loop)
    __shared__ unsigned long long nxt[UZ_PK_SCANNED];
    if (t < UZ_PK_SCANNED) nxt[t] = host_sums ? sums[UZ_PK_SUMS * ((size_t)blockIdx.x + 1) + t] : ~0ULL;
    __syncthreads();
    // the dictionary index of the NEXT round's record is requested a round ahead: its table entries can then be fetched as soon as
    // the round begins, instead of after a round trip of their own
    uint32_t tp_next = 0;
    {
        const int64_t i0 = ((int64_t)blockIdx.x << c.pk_shift) + t;
        if (c.tup && i0 < n) tp_next = c.tup[i0];
    }
    const int rounds = (1 << c.pk_shift) / 256;
    PK_TICK(0); // set-up
    for (int it = 0; it < rounds; it++) {
        const int64_t i = ((int64_t)blockIdx.x << c.pk_shift) + it * 256 + t;
        const bool in = i < n;
        const uint32_t tp = tp_next;
        if (c.tup && it + 1 < rounds && i + 256 < n) tp_next = c.tup[i + 256];
        RecSmall rs = {0u, 0u, 0u, 0u, 0u, UZ_UMASK_ALL, c.lists ? 0 : -1, 0u};
        if (in) rs = c.tup ? rec_small_of(c, i, tp) : rec_small(c, i);
        const uint32_t nc = rs.nc, ls = rs.ls, ax = rs.aux;
        const int nl = rs.nl;
        const uint32_t um = rs.um, nb = rs.nb;
        uint32_t v[UZ_PK_SUMS], inc[UZ_PK_SCANNED];
        pk_vals(nc, ls, ax, nl, um, nb, c.bl_qlow != nullptr, v);
        if (c.diff_form() && in) { v[5] = start_diff(c, i); v[6] = qname_diff(c, i); }
        PK_TICK(1); // small columns + dictionary + differences
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) inc[k] = wv_incl_scan(v[k]); // (the last two sums are totals only; DPP scans: wg.hpp)
        __syncthreads(); // wsum of the previous round has been read
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < UZ_PK_SCANNED; k++) wsum[k][wv] = inc[k];
        }
        __syncthreads();
        uint32_t pre[UZ_PK_SCANNED], tot[UZ_PK_SCANNED];
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) {
            pre[k] = 0; tot[k] = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) { if (w < wv) pre[k] += wsum[k][w]; tot[k] += wsum[k][w]; }
        }
        PK_TICK(2); // scans
        bool fits = true;
        if (host_sums && in) {
#pragma unroll
            for (int k = 0; k < UZ_PK_SCANNED; k++)
                if (k != 5 && k != 6) fits &= run[k] + pre[k] + inc[k] <= nxt[k];
            if (!fits) hflags[0] = 1;
        }
        if (in && fits) {
            RecA A;
            RecB B;
            // base rows: the units that travelled as rows in link order, then the units of the records whose bases came as a list
            const uint32_t sq = (ax & UZ_AUX_NO_SEQ) ? UZ_NO_SEQ_OFF
                                : (nb ? (uint32_t)((unsigned long long)c.n_seq_link + run[7] + pre[7] + inc[7] - v[7]) : (uint32_t)(run[2] + pre[2] + inc[2] - v[2]));
            const uint32_t cg = (uint32_t)(run[0] + pre[0] + inc[0] - v[0]);
            // the four wide columns: plain, or from their 16-bit differences (start and name id: running sums, this record included)
            int32_t st0, tl0, mt0;
            uint32_t qn0;
            if (c.pair_d8) {
                // pair form (the template length of a pair: the joins below / k_pair_link)
                st0 = (int32_t)(uint32_t)(run[5] + pre[5] + inc[5]);
                qn0 = (uint32_t)(run[6] + pre[6] + inc[6]) - 1u; // a new name's id = new names before it
                pk_pair_decode(c.pair_d8[i], i, n, [&](int col) { return esc16_of(c, i, col); }, mt0, qn0, tl0, hflags);
            } else if (c.tlen_s) {
                st0 = (int32_t)(uint32_t)(run[5] + pre[5] + inc[5]);
                qn0 = (uint32_t)(run[6] + pre[6] + inc[6]);
                tl0 = (int32_t)d16_val(c, c.tlen_s, i, 1);
                if (c.mate_d8) {
                    const int md = c.mate_d8[i];
                    mt0 = md == UZ_D8S_NONE ? -1 : (md == UZ_D8S_ESC ? esc16_of(c, i, 2) : (int32_t)(i + md));
                } else {
                    const int md = c.mate_d[i];
                    mt0 = md == UZ_D16_NONE ? -1 : (md == UZ_D16_ESC ? esc16_of(c, i, 2) : (int32_t)(i + md));
                }
                if (mt0 < -1 || mt0 >= n) { hflags[0] = 7; mt0 = -1; }
            } else { st0 = c.start[i]; tl0 = c.tlen[i]; mt0 = c.mate[i]; qn0 = c.qname[i]; }
            PK_TICK(3); // wide columns (pair form / escapes)
            // The record's CIGAR words, fetched ONCE and all together (the first four in one round trip; a short read has one to
            // three): its end and the two counts of the QC word come from registers, and the device's store gets the words -- the
            // travelled ones, or the one a simple record's aux byte names (cigar_compact).
            const uint32_t code = c.cigar_out ? (ax & UZ_AUX_SIMPLE_MASK) >> UZ_AUX_SIMPLE_SHIFT : 0u;
            if (code && nc != 1) hflags[0] = 6;
            const uint32_t *src_w = c.cigar_out ? c.cigar_staged + (run[4] + pre[4] + inc[4] - v[4]) : c.cigar_in + cg;
            const bool have_words = c.cigar_in != nullptr; // (an ASCII upload lays the words out after this kernel: k_pack_ascii sets the two bits)
            uint32_t w4[4] = {0u, 0u, 0u, 0u};
            if (code) w4[0] = uz_cigar_simple_word(code, ls);
            else if (have_words) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) if (k < nc) w4[k] = src_w[k];
            }
            int64_t ref_len = 0;
            int cig_nonmatch = 0, cig_none = 0; // the two CIGAR counts of the QC word
            if (have_words) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) if (k < nc) { pk_cigar_take(w4[k], ax, ref_len, cig_nonmatch, cig_none); if (c.cigar_out) c.cigar_out[cg + k] = w4[k]; }
                for (uint32_t k = 4; k < nc; k++) { const uint32_t w = src_w[k]; pk_cigar_take(w, ax, ref_len, cig_nonmatch, cig_none); if (c.cigar_out) c.cigar_out[cg + k] = w; }
            }
            const int32_t en0 = c.end ? c.end[i] : pk_end(rs.flag, nc, have_words, st0, ref_len);
            PK_TICK(4); // CIGAR
            int low_for_qc = 0; // (an ASCII upload has no counts yet: uz_build_qlow sets the bit that depends on them)
            uz_pack_rec(A, B, st0, en0, cg, sq, mt0, qn0, (uint16_t)ls, (uint16_t)nc, tl0);
            pk_index_store(i, st0, coarse, mid_idx, mid8);
            ra[i] = A;
            rb[i] = B;
            fm[i] = uz_pack_fm(rs.flag, rs.mapq, ax);
            pk_umask_store(i, um, nb, ls, umask_out, hflags);
            PK_TICK(5); // header stores
            const QRow qr = pk_qrow_rule(c.bl_qlow != nullptr, nb, v[3], nl, ax);
            if (nb) {
                const unsigned long long at = run[8] + pre[8] + inc[8] - v[8];
                pk_listed_rows(nb, ls, um, ax, sq, qr, nl,
                               [&](uint32_t e) { const unsigned long long g = at + e; return c.bl_wide ? ((int)c.bl_pos[2 * g] | ((int)c.bl_pos[2 * g + 1] << 8)) : (int)c.bl_pos[g]; },
                               [&](uint32_t e) { const unsigned long long g = at + e; return ((uint32_t)c.bl_code[g >> 2] >> (2u * (uint32_t)(g & 3ULL))) & 3u; },
                               [&](uint32_t e) { const unsigned long long g = at + e; return ((uint32_t)c.bl_qlow[g >> 3] >> (uint32_t)(g & 7ULL)) & 1u; }, c.seq4_out, plane_out, hflags);
            }
            PK_TICK(6); // listed bases
            if (nl >= 0) {
                // list form of the staged plane: the count as it is, and the quality row of a record that gets one from its listed positions
                nlow[i] = (uint8_t)nl;
                low_for_qc = nl;
                qoff[i] = qr.listed ? sq : UZ_NO_QLOW_OFF;
                if (qr.listed && !qr.with_bits) { // (with bits: written and held against the count above, beside the base rows)
                    const unsigned long long at = run[3] + pre[3] + inc[3] - v[3];
                    // (all of them requested together, and kept in registers: NE = UZ_QLOW_LIST_MAX below unrolls the helper's loops, so that
                    // pos[] is indexed by constants only and never goes to scratch)
                    int pos[UZ_QLOW_LIST_MAX];
#pragma unroll
                    for (int e = 0; e < UZ_QLOW_LIST_MAX; e++) {
                        pos[e] = -1;
                        if (e < nl) pos[e] = c.qpos_wide ? ((int)c.qlow_pos[2 * (at + e)] | ((int)c.qlow_pos[2 * (at + e) + 1] << 8)) : (int)c.qlow_pos[at + e];
                    }
                    pk_qlist_rows<UZ_QLOW_LIST_MAX>(nl, ls, um, sq, [&](int e) { return pos[e]; }, plane_out, hflags);
                }
            } else {
                const uint32_t qo = (uint32_t)(run[1] + pre[1] + inc[1] - v[1]);
                qoff[i] = qo;
                if (c.plane_in) { // the plane itself was staged: count its bits once
                    int low = 0;
                    for (int u = 0; u < (int)UZ_ROW_UNITS(ls); u++) {
                        uint32_t w = c.plane_in[(size_t)qo + u];
                        const int valid = (int)ls - 32 * u;
                        if (valid < 32) w &= valid > 0 ? ((1u << valid) - 1u) : 0u;
                        low += __popc(w);
                    }
                    nlow[i] = (uint8_t)(low > 255 ? 255 : low);
                    low_for_qc = low;
                }
            }
            qs[i] = uz_qs_word(rs.flag, ax, rs.mapq, low_for_qc, (int)nc, cig_nonmatch, cig_none);
            PK_TICK(7); // quality list + QC word
        }
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) run[k] += tot[k];
    }
    PK_TICK(8);
    if (c.pair_d8) {
        // the pairs that lie inside this span are joined here, by the workgroup that has just written both headers (they sit in its L2 lines); a FIRST
        // whose SECOND belongs to the next span is left to k_pair_link, which then looks at the last 256 records of every span only
        __syncthreads();
        const int64_t s0 = (int64_t)blockIdx.x << c.pk_shift, s1 = s0 + ((int64_t)1 << c.pk_shift);
        for (int it = 0; it < rounds; it++) {
            const int64_t i = s0 + it * 256 + t;
            if (i >= n) break;
            const uint32_t p = c.pair_d8[i];
            if (!p8_first(p)) continue;
            const int64_t j = i + p;
            if (j >= n || j >= s1) continue; // (beyond the table: flagged above; in the next span: k_pair_link)
            uz_pair_link_one(i, j, c.pair_d8, ra, rb, hflags);
        }
    }
    PK_TICK(9); // pairs inside the span
#ifdef UZ_PACK_TIMING
    if (threadIdx.x == 0) for (int k = 0; k < 10; k++) atomicAdd(&uz_pack_ticks[k], ptk__[k]);
#endif
    if (host_sums && t == 0) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < UZ_PK_SCANNED; k++) same &= (k == 5 || k == 6) ? (uint32_t)run[k] == (uint32_t)nxt[k] : run[k] == nxt[k]; // (the two difference columns count modulo 2^32)
        if (!same) hflags[0] = 1;
    }
}

// ---- the header build of the link form, from LDS -----------------------------------------------------------------------------------------
// k_pack_rec reads a record's parts where they lie: per round of 256 records a dozen dependent trips to memory (dictionary entries, escape
// searches, CIGAR words, listed positions one at a time, quality lists, and a second pass over the span for its pairs) -- 30 k cycles per
// round, 1.0 ms per 9.9 M-record chunk of the staged pass against a streaming bound of 0.12 ms (profiles/r05: section timing).  The form
// every packer of the product emits comes with the span sums of the packer (pk_sums): a workgroup knows before it starts where every
// variable-length list of its span begins and ends.  So it stages ALL of its span's input -- the three byte columns, the dictionary, its
// share of the quality lists, listed bases, travelled CIGAR words and escapes, ~6 KB -- into LDS with one round of coalesced loads, and
// decodes from there; the pairs of a span are joined through LDS too (a FIRST record tells its SECOND how far back it stands), so a header is
// stored once, finished.  Only a FIRST whose SECOND lies in the next span is left to k_pair_link.
// Taken for: the link form (uz_link_form) with host sums, spans of 1024 records, byte positions.  The dictionary of the small columns (a few
// thousand combinations of eight values) is packed into one 16-byte entry per combination first (k_pack_dict): a record's small columns are one load.
// A list of a span that outgrows its LDS room is read from memory by that workgroup (slower, same result).
#define UZ_PL_SPAN 1024
#define UZ_PL_QP 4096   // staged quality-list bytes per span
#define UZ_PL_BL 4096   // staged listed-base positions per span
#define UZ_PL_CIG 256   // staged CIGAR words per span
#define UZ_PL_ESC 64    // staged escape entries per span
// a workgroup barrier that orders LDS traffic only: the round's stores to memory (nobody reads them here) stay in flight across it, where
// __syncthreads() would have every wave wait for their acknowledgement three times a round
#define PL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
__global__ __launch_bounds__(256) void k_pack_dict(RecColumns c, int32_t n_tup, uint4 *dict) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_tup) return;
    uint4 e; // flag | l_seq << 16, n_cigar | umask << 16, mapq | aux << 8 | n_low << 16 | n_bl << 24
    e.x = (uint32_t)c.tup_flag[k] | ((uint32_t)c.tup_l_seq[k] << 16);
    e.y = (uint32_t)c.tup_n_cigar[k] | ((uint32_t)c.tup_umask[k] << 16);
    e.z = (uint32_t)c.tup_mapq[k] | ((uint32_t)c.tup_aux[k] << 8) | ((uint32_t)c.tup_n_low[k] << 16) | ((c.tup_n_bl ? (uint32_t)c.tup_n_bl[k] : 0u) << 24);
    e.w = 0u;
    dict[k] = e;
}
// (30 KB of LDS and <= 96 VGPRs: five workgroups per CU)
__global__ __launch_bounds__(256, 5) void k_pack_link(int64_t n, RecColumns c_in, const unsigned long long *__restrict__ sums, int32_t n_tup, const uint4 *__restrict__ dict, RecA *ra, RecB *rb,
                                                     uint32_t *fm, uint32_t *qoff, uint8_t *nlow, uint16_t *umask_out, uint32_t *plane_out,
                                                     uint16_t *qs, int32_t *coarse, int32_t *mid_idx, int32_t *mid8, int32_t *hflags) {
    RecColumns c = uz_columns_of<true>(c_in);
    __shared__ uint16_t s_tup[UZ_PL_SPAN];
    __shared__ uint8_t s_sd[UZ_PL_SPAN], s_pd[UZ_PL_SPAN];
    __shared__ uint8_t s_qp[UZ_PL_QP], s_blp[UZ_PL_BL], s_blc[UZ_PL_BL / 4 + 8], s_blq[UZ_PL_BL / 8 + 8]; // (the span's slices of bl_code and bl_qlow, byte for byte)
    __shared__ uint32_t s_cig[UZ_PL_CIG];
    __shared__ unsigned long long s_esck[UZ_PL_ESC];
    __shared__ int32_t s_escv[UZ_PL_ESC];
    // A SECOND stands at most UZ_P8_MAX_DIST < 256 records behind its FIRST: in the same round of 256 records or in the round before.  So only
    // the last two rounds' headers are held here, in a ring of 512: a record's RecA is stored at once (nothing changes it), its RecB once the
    // round after its own has been joined (a SECOND writes its FIRST's template length) -- 12 KB of LDS where the whole span's headers took 32
    __shared__ int2 s_se[2 * 256];  // start, end: what a SECOND reads of its FIRST's RecA
    __shared__ RecB s_rb[2 * 256];
    __shared__ uint8_t s_back[UZ_PL_SPAN];        // how far back a SECOND's FIRST stands (0: not named inside the span)
    __shared__ uint32_t s_named[UZ_PL_SPAN / 4];  // how often a record was named (a byte each)
    __shared__ uint32_t wsum[UZ_PK_SCANNED][4];
    __shared__ unsigned long long s_run[UZ_PK_SUMS], s_nxt[UZ_PK_SUMS];
    __shared__ int64_t esc_span[2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#ifdef UZ_PACK_TIMING
    unsigned long long ptk__[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ptl__ = __builtin_amdgcn_s_memtime();
#endif
    const int64_t s0 = (int64_t)blockIdx.x * UZ_PL_SPAN;
    const int cnt = (int)(n - s0 < UZ_PL_SPAN ? n - s0 : UZ_PL_SPAN);
    if (t < UZ_PK_SUMS) { s_run[t] = sums[UZ_PK_SUMS * (size_t)blockIdx.x + t]; s_nxt[t] = sums[UZ_PK_SUMS * ((size_t)blockIdx.x + 1) + t]; }
    if (c.n_esc16 > 0 && t < 2) esc_span[t] = esc_lower_bound(c.esc16_key, c.n_esc16, s0 + (int64_t)t * UZ_PL_SPAN);
    // the byte columns of the span and the dictionary (independent of the sums: requested beside them)
    for (int k = t; k < cnt; k += 256) { s_sd[k] = c.start_d8[s0 + k]; s_pd[k] = c.pair_d8[s0 + k]; }
    for (int k = t; k < UZ_PL_SPAN; k += 256) s_back[k] = 0;
    for (int k = t; k < UZ_PL_SPAN / 4; k += 256) s_named[k] = 0u;
    if (c.tup8 == nullptr) {
        for (int k = t; k < cnt; k += 256) s_tup[k] = c.tup[s0 + k];
        __syncthreads();
    } else {
        // The dictionary index arrives in ONE byte (uz_types.h tup8: its place among the 255 most frequent combinations, or 255 and the 16-bit
        // index in an escape list whose offsets are given per span of 1 024 records -- this workgroup's span).  Rounds 5's k_tup_expand rebuilt the
        // 16-bit column in HBM in front of this kernel (1 byte read + 2 written per record, and this kernel read the 2 again: 0.35 ms of a staged
        // step's chip time, a launch per table); the span's indices are now rebuilt where they are used, in LDS, with the same checks.
        static_assert(UZ_PL_SPAN == UZ_TUP8_SPAN, "the spans of the escape offsets are this kernel's");
        pk_tup8_expand(n, c.tup8, c.tup_hot, c.tup_esc, c.tup_esc_off, c.n_tup_esc, n_tup, hflags, [&](int k, uint32_t val) { s_tup[4 * t + k] = (uint16_t)val; });
        __syncthreads();
    }
    PK_TICK(0); // columns + sums rows
    // the dictionary entry of a round's record (requested at the top of its round: five workgroups per CU hide the trip, where holding it a
    // round ahead cost the registers that keep the kernel at 96 VGPRs)
    auto dict_of = [&](int k) -> uint4 {
        uint32_t tp = k < cnt ? (uint32_t)s_tup[k] : 0u;
        if ((int)tp >= n_tup) { hflags[0] = 1; tp = 0u; } // (an index beyond the dictionary)
        return dict[tp];
    };
    // Everything below counts in 32 bits from the span's own base: the running offsets inside the span (rel), the span's share of every
    // quantity (len: next row - this row; the host has checked that the rows ascend and that the totals fit 32 bits), the bases of the five
    // quantities that become absolute offsets.  All of it uniform: read back through readfirstlane so that it lives in scalar registers.
    auto uni64 = [&](unsigned long long x) -> unsigned long long {
        return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    };
    uint32_t rel[UZ_PK_SCANNED], len[UZ_PK_SCANNED];
#pragma unroll
    for (int k = 0; k < UZ_PK_SCANNED; k++) { rel[k] = 0u; len[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(s_nxt[k] - s_run[k])); }
    const uint32_t base_cg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s_run[0]), base_sq = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s_run[2]);
    const uint32_t base_st = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s_run[5]), base_qn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s_run[6]);
    const uint32_t base_sql = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)c.n_seq_link + s_run[7]));
    bool len_ok = true; // (a span's share of anything is far below 2^32; a row pair that says otherwise is refused)
#pragma unroll
    for (int k = 0; k < UZ_PK_SCANNED; k++) if (k != 5 && k != 6) len_ok &= s_nxt[k] - s_run[k] <= 0xFFFFFFFFULL;
    if (!len_ok) hflags[0] = 1;
    // this span's share of the lists, where the packer's sums put it
    const unsigned long long q0 = uni64(s_run[3]), b0 = uni64(s_run[8]), g0 = uni64(s_run[4]);
    const uint32_t qn_ = len[3], bn_ = len[8], gn_ = len[4];
    const bool q_in = qn_ <= UZ_PL_QP, b_in = bn_ <= UZ_PL_BL, g_in = gn_ <= UZ_PL_CIG;
    const int64_t e0 = c.n_esc16 > 0 ? (int64_t)uni64((unsigned long long)esc_span[0]) : 0, e1 = c.n_esc16 > 0 ? (int64_t)uni64((unsigned long long)esc_span[1]) : 0;
    const bool e_in = e1 - e0 <= UZ_PL_ESC;
    // (four two-bit codes per byte of bl_code, eight quality bits per byte of bl_qlow: the span's first entry sits b0 & 3 codes / b0 & 7 bits
    // into the first byte of its slice; both slices are copied as they lie)
    const uint32_t b0lo = (uint32_t)(b0 & 7ULL);
    if (q_in) for (int k = t; k < (int)qn_; k += 256) s_qp[k] = c.qlow_pos[q0 + k];
    if (b_in) {
        for (int k = t; k < (int)bn_; k += 256) s_blp[k] = c.bl_pos[b0 + k];
        const int ncb = (int)(((b0lo & 3u) + bn_ + 3u) >> 2);
        for (int k = t; k < ncb; k += 256) s_blc[k] = c.bl_code[(b0 >> 2) + k];
        if (c.bl_qlow) {
            const int nqb = (int)((b0lo + bn_ + 7u) >> 3);
            for (int k = t; k < nqb; k += 256) s_blq[k] = c.bl_qlow[(b0 >> 3) + k];
        }
    }
    if (g_in) for (int k = t; k < (int)gn_; k += 256) s_cig[k] = c.cigar_staged[g0 + k];
    if (e_in) for (int k = t; k < (int)(e1 - e0); k += 256) { s_esck[k] = c.esc16_key[e0 + k]; s_escv[k] = c.esc16_val[e0 + k]; }
    __syncthreads();
    PK_TICK(1); // lists
    auto esc_of = [&](int64_t i, int col) -> int32_t { // value of (record, column) in the escape list, 0 when missing (caught by the totals / the mate check)
        const unsigned long long key = ((unsigned long long)i << 2) | (unsigned long long)col;
        if (e_in) {
            int lo = 0, hi = (int)(e1 - e0);
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_esck[mid] < key) lo = mid + 1; else hi = mid; }
            return (lo < (int)(e1 - e0) && s_esck[lo] == key) ? s_escv[lo] : 0;
        }
        int64_t lo = e0, hi = e1;
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (c.esc16_key[mid] < key) lo = mid + 1; else hi = mid; }
        return (lo < c.n_esc16 && c.esc16_key[lo] == key) ? c.esc16_val[lo] : 0;
    };
    // (r: place in the span's share of the list)
    auto qpos_at = [&](uint32_t r) -> int { return q_in ? (int)s_qp[r] : (int)c.qlow_pos[q0 + r]; };
    auto blpos_at = [&](uint32_t r) -> int { return b_in ? (int)s_blp[r] : (int)c.bl_pos[b0 + r]; };
    auto blcode_at = [&](uint32_t r) -> uint32_t {
        const uint32_t g = (b0lo & 3u) + r;
        const uint32_t byte = b_in ? (uint32_t)s_blc[g >> 2] : (uint32_t)c.bl_code[(b0 >> 2) + (g >> 2)];
        return (byte >> (2u * (g & 3u))) & 3u;
    };
    auto blq_at = [&](uint32_t r) -> uint32_t { // (only asked with the column)
        const uint32_t g = b0lo + r;
        const uint32_t byte = b_in ? (uint32_t)s_blq[g >> 3] : (uint32_t)c.bl_qlow[(b0 >> 3) + (g >> 3)];
        return (byte >> (g & 7u)) & 1u;
    };
    const bool blq = c.bl_qlow != nullptr;
    auto cig_at = [&](uint32_t r) -> uint32_t { return g_in ? s_cig[r] : c.cigar_staged[g0 + r]; };
    for (int it = 0; it < UZ_PL_SPAN / 256; it++) {
        const int k = it * 256 + t; // the record's place in the span
        const int64_t i = s0 + k;
        const bool in = k < cnt;
        uint4 de = make_uint4(0u, 0u, 0u, 0u);
        uint32_t p = UZ_P8_NEW, sd = 0;
        if (in) { de = dict_of(k); p = s_pd[k]; sd = s_sd[k]; }
        const uint32_t flag = de.x & 0xFFFFu, ls = de.x >> 16, nc = de.y & 0xFFFFu, um = in ? (de.y >> 16) : UZ_UMASK_ALL;
        const uint32_t mapq = de.z & 0xFFu, ax = (de.z >> 8) & 0xFFu, nb = de.z >> 24;
        const int nl = (int)((de.z >> 16) & 0xFFu);
        uint32_t v[UZ_PK_SUMS], inc[UZ_PK_SCANNED];
        pk_vals(nc, ls, ax, nl, um, nb, c.bl_qlow != nullptr, v);
        if (!in) {
#pragma unroll
            for (int q = 0; q < UZ_PK_SUMS; q++) v[q] = 0u;
        } else {
            v[5] = sd == UZ_D8_ESC ? (uint32_t)esc_of(i, 0) : sd;
            v[6] = p8_new_name(p) ? 1u : 0u;
        }
        PK_TICK(2); // dictionary entry + values
#pragma unroll
        for (int q = 0; q < UZ_PK_SCANNED; q++) inc[q] = wv_incl_scan(v[q]);
        PL_BARRIER(); // wsum of the previous round has been read
        if (lane == 63) {
#pragma unroll
            for (int q = 0; q < UZ_PK_SCANNED; q++) wsum[q][wv] = inc[q];
        }
        PL_BARRIER();
        // (every round before this one has been joined: the RecBs of the round before the last are final, and this round reuses their slots)
        if (it >= 2 && k - 512 < cnt) rb[s0 + k - 512] = s_rb[k & 511];
        // where the record's parts end, counted from the span's base: the rounds before, the waves before, the lanes before and the record
        // itself; the running offsets move on at once, so that only the eight offsets below live through the rest of the round.  Nothing
        // of a record may end beyond the span's share: nothing is read or written outside it.
        bool fits = in;
        uint32_t e32[UZ_PK_SCANNED];
#pragma unroll
        for (int q = 0; q < UZ_PK_SCANNED; q++) {
            uint32_t pre = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) { if (w < wv) pre += wsum[q][w]; tot += wsum[q][w]; }
            e32[q] = rel[q] + pre + inc[q];
            if (q != 5 && q != 6) fits &= e32[q] <= len[q] && e32[q] >= inc[q]; // (no wrap)
            rel[q] += (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
        }
        if (in && !fits) hflags[0] = 1;
        const uint32_t o_cg = base_cg + e32[0] - v[0], o_sq = base_sq + e32[2] - v[2], o_sql = base_sql + e32[7] - v[7];
        const uint32_t r_qp = e32[3] - v[3], r_gw = e32[4] - v[4], r_bl = e32[8] - v[8];
        const uint32_t o_st = base_st + e32[5], o_qn = base_qn + e32[6];
        const uint32_t v3 = v[3];
        PK_TICK(3); // scans
        // ---- first half: everything of the record that does not depend on its mate
        int32_t st0 = 0, en0 = 0, tl0 = 0, mt0 = -1;
        uint32_t qn0 = 0, sq = 0, cg = 0;
        int cig_nonmatch = 0, cig_none = 0;
        if (fits) {
            sq = (ax & UZ_AUX_NO_SEQ) ? UZ_NO_SEQ_OFF : (nb ? o_sql : o_sq);
            cg = o_cg;
            st0 = (int32_t)o_st;
            qn0 = o_qn - 1u; // a new name's id = new names before it
            pk_pair_decode(p, i, n, [&](int col) { return esc_of(i, col); }, mt0, qn0, tl0, hflags);
            // CIGAR: the word a simple record's aux byte names, or the words that travelled; `end` and the two counts of the QC word from them
            const uint32_t code = (ax & UZ_AUX_SIMPLE_MASK) >> UZ_AUX_SIMPLE_SHIFT;
            if (code && nc != 1) hflags[0] = 6;
            const uint32_t gw = r_gw;
            int64_t ref_len = 0;
            for (uint32_t q = 0; q < nc; q++) {
                const uint32_t w = code ? uz_cigar_simple_word(code, ls) : cig_at(gw + q);
                pk_cigar_take(w, ax, ref_len, cig_nonmatch, cig_none);
                c.cigar_out[cg + q] = w;
            }
            en0 = pk_end(flag, nc, true, st0, ref_len);
            {
                RecA A;
                RecB B;
                uz_pack_rec(A, B, st0, en0, cg, sq, mt0, qn0, (uint16_t)ls, (uint16_t)nc, tl0);
                ra[i] = A;
                s_se[k & 511] = make_int2(st0, en0);
                s_rb[k & 511] = B;
            }
            if (p8_first(p) && mt0 >= 0 && k + (int)p < UZ_PL_SPAN) { // a FIRST whose SECOND lies in this span: tell it
                const int j = k + (int)p;
                s_back[j] = (uint8_t)p;
                if ((atomicAdd(&s_named[j >> 2], 1u << (8 * (j & 3))) >> (8 * (j & 3))) & 0xFFu) hflags[0] = 8; // named twice
            }
        }
        PL_BARRIER();
        PK_TICK(4); // first half (wide columns, CIGAR)
        // ---- second half: the pair.  A FIRST and its SECOND share name id and template length (+-): tlen = max(end, mate's end) - start of
        // the FIRST, or the SECOND's own (UZ_P8_SECOND_TLEN).  The SECOND finishes both headers (its FIRST stands in front of it: written, and
        // behind a barrier).
        if (fits) {
            const uint32_t named = (s_named[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            if (p8_second(p)) {
                const int d = (int)s_back[k];
                if (d) { // its FIRST stands d records back, in this span
                    const int f = k - d, sf = f & 511, sk = k & 511;
                    const int2 FA = s_se[sf];
                    int32_t tlf; // the FIRST's template length
                    if (p == UZ_P8_SECOND_TLEN) tlf = -tl0;
                    else { tlf = (FA.y > en0 ? FA.y : en0) - FA.x; tl0 = -tlf; }
                    s_rb[sf].tlen = tlf;
                    s_rb[sk].mate = (int32_t)(s0 + f);
                    s_rb[sk].qname = s_rb[sf].qname;
                    s_rb[sk].tlen = tl0;
                }
                // (else: its FIRST lies in the span before this one -- k_pair_link -- or nowhere: the totals of the packer's sums tell)
            } else if (named) hflags[0] = 8; // named as a mate, but not a SECOND record
            // (a FIRST whose SECOND lies in the next span: k_pair_link)
            pk_index_store(i, st0, coarse, mid_idx, mid8);
            fm[i] = uz_pack_fm(flag, mapq, ax);
            pk_umask_store(i, um, nb, ls, umask_out, hflags);
            PK_TICK(5); // pair + header stores
            // The count and the QC word first: nothing below changes them, and their inputs need not live through the two list loops.
            // list form of the staged plane: the count as it is; a quality row (at the record's base-row position) only for a record whose
            // bits can be asked for -- written from its listed positions, or, with bl_qlow, from the bits of its listed bases beside their rows
            nlow[i] = (uint8_t)nl;
            qs[i] = uz_qs_word(flag, ax, mapq, nl, (int)nc, cig_nonmatch, cig_none);
            const QRow qr = pk_qrow_rule(blq, nb, v3, nl, ax);
            qoff[i] = qr.listed ? sq : UZ_NO_QLOW_OFF;
            if (nb)
                pk_listed_rows(nb, ls, um, ax, sq, qr, nl, [&](uint32_t e) { return blpos_at(r_bl + e); }, [&](uint32_t e) { return blcode_at(r_bl + e); },
                               [&](uint32_t e) { return blq_at(r_bl + e); }, c.seq4_out, plane_out, hflags);
            PK_TICK(6); // listed bases
            if (qr.listed && !qr.with_bits) pk_qlist_rows<0>(nl, ls, um, sq, [&](int e) { return qpos_at(r_qp + (uint32_t)e); }, plane_out, hflags);
            PK_TICK(7); // quality list
        }
    }
#ifdef UZ_PACK_TIMING
    if (threadIdx.x == 0) for (int q = 0; q < 10; q++) atomicAdd(&uz_pack_ticks[q], ptk__[q]);
#endif
    PL_BARRIER();
    for (int q = 512 + t; q < cnt; q += 256) rb[s0 + q] = s_rb[q & 511]; // (the last two rounds)
    if (t == 0) { // the span's own sums must add up to exactly the packer's next row (the two difference columns modulo 2^32)
        bool same = true;
#pragma unroll
        for (int q = 0; q < UZ_PK_SCANNED; q++) same &= rel[q] == len[q];
        if (!same) hflags[0] = 1;
    }
}

// pair form, across spans: a FIRST among the last 256 records of a span of the header build whose SECOND lies in the next span (the pairs inside a
// span were joined by k_pack_rec's own workgroups; a mate lies at most UZ_P8_MAX_DIST = 252 records on)
__global__ __launch_bounds__(256) void k_pair_link(int64_t n, int pk_shift, const uint8_t *__restrict__ pair, const RecA *__restrict__ ra, RecB *rb, int32_t *hflags) {
    const int64_t s1 = ((int64_t)blockIdx.x + 1) << pk_shift;
    const int64_t i = s1 - 256 + threadIdx.x;
    if (i < 0 || i >= n) return;
    const uint32_t p = pair[i];
    if (!p8_first(p)) return;
    const int64_t j = i + p;
    if (j >= n || j < s1) return; // (beyond the table: flagged by the header build; inside the span: done there)
    uz_pair_link_one(i, j, pair, ra, rb, hflags);
}

// ---- ASCII uploads (uz_reads_upload): rows re-laid in the packed geometry ---------------------------------
__global__ __launch_bounds__(256) void k_pack_ascii(int64_t n, const RecA *__restrict__ ra, const RecB *__restrict__ rb,
                                                    const uint32_t *__restrict__ cigar_in, const uint32_t *__restrict__ cigar_off_in,
                                                    const uint8_t *__restrict__ seq_in, const uint32_t *__restrict__ sq_off16_in,
                                                    uint32_t *cigar_out, uint8_t *seq4_out, uint16_t *qs, int32_t *hflags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RecA A = ra[i];
    const RecB B = rb[i];
    int nonmatch = 0, none = 0;
    for (int k = 0; k < (int)B.n_cigar; k++) {
        const uint32_t w = cigar_in[(size_t)cigar_off_in[i] + k];
        cigar_out[(size_t)A.cigar_off + k] = w;
        uz_cigar_op_counts(w, nonmatch, none);
    }
    { // the two CIGAR bits of the QC word (the header build ran before the words were here); a record without CIGAR / SEQ / QUAL keeps 0
        const uint32_t w = qs[i];
        if (w & 0xFF0Fu || B.n_cigar) // (uz_qs_word gave 0 for UZ_AUX_DECODE_BAD: such a record has no operations)
            qs[i] = (uint16_t)((w & ~(UZ_QC_NM5 | UZ_QC_NONE5)) | (nonmatch <= 5 ? UZ_QC_NM5 : 0u) | (none <= 5 ? UZ_QC_NONE5 : 0u));
    }
    const uint8_t *src = seq_in + ((size_t)sq_off16_in[i] << 4);
    uint8_t *dst = seq4_out + (size_t)A.sq_off * UZ_SEQ4_UNIT_BYTES;
    const int ls = B.l_seq, nb = (int)UZ_ROW_UNITS(ls) * UZ_SEQ4_UNIT_BYTES;
    bool bad = false;
    for (int b = 0; b < nb; b++) {
        uint32_t hi = 0, lo = 0;
        if (2 * b < ls) { hi = uz_ascii_nt16(src[2 * b]); bad |= hi == 0xFFu; }
        if (2 * b + 1 < ls) { lo = uz_ascii_nt16(src[2 * b + 1]); bad |= lo == 0xFFu; }
        dst[b] = (uint8_t)(((hi & 15u) << 4) | (lo & 15u));
    }
    if (bad) hflags[0] = 2;
}
__global__ __launch_bounds__(256) void k_build_qlow(int64_t n, const RecA *__restrict__ ra, const RecB *__restrict__ rb,
                                                    const uint32_t *__restrict__ qoff, const uint8_t *__restrict__ qual8,
                                                    const uint32_t *__restrict__ qual_off16, int thr, uint8_t *qlow, uint8_t *nlow, uint16_t *qs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ls = rb[i].l_seq;
    const uint8_t *src = qual8 + ((size_t)qual_off16[i] << 4);
    uint32_t *dst = reinterpret_cast<uint32_t *>(qlow) + (size_t)qoff[i];
    const int units = (int)UZ_ROW_UNITS(ls);
    int low = 0;
    for (int u = 0; u < units; u++) {
        uint32_t w = 0;
        for (int k = 0; k < 32 && 32 * u + k < ls; k++) w |= (uint32_t)((int)src[32 * u + k] < thr) << k;
        dst[u] = w;
        low += __popc(w);
    }
    nlow[i] = (uint8_t)(low > 255 ? 255 : low);
    // the one bit of the QC word that depends on the threshold: goodread's count of low-quality bases (:43-52)
    const uint32_t w = qs[i];
    qs[i] = (uint16_t)((w & ~UZ_QC_GOOD) | (((w & UZ_QC_GOOD_DISC) && low <= 10 && rb[i].n_cigar <= 10) ? UZ_QC_GOOD : 0u));
}

// cohort batches: the headers of one kid's table copied into the merged table with its bases added
__global__ __launch_bounds__(256) void k_concat_rec(int64_t n, const RecA *__restrict__ sa, const RecB *__restrict__ sb, const uint32_t *__restrict__ sfm,
                                                    const uint32_t *__restrict__ sqo, const uint8_t *__restrict__ snl,
                                                    const uint16_t *__restrict__ sum_, const uint16_t *__restrict__ sqs, RecA *da, RecB *db, uint32_t *dfm, uint32_t *dqo,
                                                    uint8_t *dnl, uint16_t *dum, uint16_t *dqs,
                                                    int32_t rec_base,
                                                    uint32_t cigar_base, uint32_t unit_base, uint32_t seq_base, uint32_t qname_base) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    RecA A = sa[i];
    RecB B = sb[i];
    A.cigar_off += cigar_base;
    if (A.sq_off != UZ_NO_SEQ_OFF) A.sq_off += seq_base;
    if (B.mate >= 0) B.mate += rec_base;
    B.qname += qname_base;
    da[i] = A; db[i] = B; dfm[i] = sfm[i]; dqo[i] = sqo[i] == UZ_NO_QLOW_OFF ? UZ_NO_QLOW_OFF : sqo[i] + unit_base; dnl[i] = snl[i]; dum[i] = sum_[i]; dqs[i] = sqs[i];
}

// two-bit base rows of the host link -> the four-bit rows the kernels read: one lane per 8 staged bytes (32 bases),
// a pure streaming map (8 B in, 16 B out); the padding of a record's last unit expands to code 1 and is never read
__global__ __launch_bounds__(256) void k_expand_seq2(const unsigned long long *__restrict__ in, uint4 *__restrict__ out, size_t n_units) {
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < n_units; u += (size_t)gridDim.x * 256) {
        const unsigned long long w = in[u]; // little-endian: byte b of the row = bits 8b..8b+7
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t lo = uz_seq2_expand_byte((uint32_t)(w >> (16 * q)) & 0xFFu), hi = uz_seq2_expand_byte((uint32_t)(w >> (16 * q + 8)) & 0xFFu);
            o[q] = lo | (hi << 16);
        }
        out[u] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
// the listed bases (not A/C/G/T): their BAM codes written over the expanded rows; every entry owns its nibble
__global__ __launch_bounds__(256) void k_patch_exc(int64_t n_exc, const uint32_t *__restrict__ rec, const uint16_t *__restrict__ pos,
                                                   const uint8_t *__restrict__ code, const RecA *__restrict__ ra, const RecB *__restrict__ rb,
                                                   const uint16_t *__restrict__ umask, int64_t n, uint32_t *seq4_words, int32_t *hflags) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_exc) return;
    const uint32_t i = rec[e];
    const uint32_t k = pos[e];
    if ((int64_t)i >= n || k >= rb[i].l_seq || ra[i].sq_off == UZ_NO_SEQ_OFF || code[e] > 15) { hflags[0] = 3; return; }
    uint32_t unit = k >> 5;
    const uint32_t um = umask[i];
    if (um != UZ_UMASK_ALL) {
        if (unit > 14u || !((um >> unit) & 1u)) return; // the unit stayed home: nothing to patch
        unit = (uint32_t)__popc(um & ((1u << unit) - 1u));
    }
    const size_t byte = ((size_t)ra[i].sq_off + unit) * UZ_SEQ4_UNIT_BYTES + ((k & 31u) >> 1);
    const int sh = (int)(8 * (byte & 3)) + ((k & 1) ? 0 : 4);
    uint32_t *wd = seq4_words + (byte >> 2);
    atomicAnd(wd, ~(15u << sh));
    atomicOr(wd, (uint32_t)code[e] << sh);
}
} // namespace

// (sized for the short spans whatever the table gets: 96 bytes per 1024 records; never less than the packed dictionary of UZ_PL_DICT_MIN
// combinations, so that a table of a few hundred records -- a chunk of a small batch: a combination of its own for every few records -- is
// built by k_pack_link as the large ones are)
#define UZ_PL_DICT_MIN 256
size_t uz_rec_scratch_bytes(int64_t n) {
    const size_t spans = (size_t)(((n + (1 << UZ_PK_SHIFT_SMALL) - 1) >> UZ_PK_SHIFT_SMALL) + 2) * (UZ_PK_SUMS + 1) * sizeof(unsigned long long);
    return std::max(spans, (size_t)UZ_PL_DICT_MIN * sizeof(uint4));
}

// tup8 back to the 16-bit column in HBM, for every build that reads it from memory (pk_tup8_expand: one 4-byte load and one 8-byte store per
// lane; 1 byte read + 2 written per record)
__global__ __launch_bounds__(256) void k_tup_expand(int64_t n, const uint8_t *__restrict__ tup8, const uint16_t *__restrict__ hot, const uint16_t *__restrict__ esc,
                                                    const uint32_t *__restrict__ esc_off, int64_t n_esc, int32_t n_tup, uint16_t *__restrict__ out, int32_t *hflags) {
    const int64_t base = (int64_t)blockIdx.x * UZ_TUP8_SPAN + 4 * threadIdx.x;
    uint16_t v4[4];
    pk_tup8_expand(n, tup8, hot, esc, esc_off, n_esc, n_tup, hflags, [&](int k, uint32_t val) { v4[k] = (uint16_t)val; });
    if (base + 4 <= n) *reinterpret_cast<uint2 *>(out + base) = make_uint2((uint32_t)v4[0] | ((uint32_t)v4[1] << 16), (uint32_t)v4[2] | ((uint32_t)v4[3] << 16));
    else for (int k = 0; k < 4; k++) if (base + k < n) out[base + k] = v4[k];
}

void uz_build_records(uz_ctx *c, hipStream_t st, ReadsDev &r, const RecColumns &col_in, void *off_scratch) {
    static_assert(sizeof(RecA) == 16 && sizeof(RecB) == 16, "record headers are two 16-byte words");
    if (r.n <= 0) return;
    RecColumns col = col_in;
    if (col.tup8) col.tup = col.tup_out; // the one-byte dictionary index: the 16-bit column is rebuilt below, in HBM (k_tup_expand) or in k_pack_link's LDS
    col.pk_shift = uz_pk_shift(r.n);
    const unsigned nb = (unsigned)((r.n + (1 << col.pk_shift) - 1) >> col.pk_shift);
    unsigned long long *sums = (unsigned long long *)off_scratch;
    // (the escape list is cut at the spans of the passes below by the workgroups themselves; the coarse search index is written by the second
    // pass: two launches gone from every table)
    PkWant want;
    want.cigar = (unsigned long long)r.n_cigar_total; want.units = (unsigned long long)r.n_row_units; want.seq = (unsigned long long)(r.n_seq_units - r.n_bl_units);
    want.qpos = (unsigned long long)r.n_qlow_pos; want.staged = col.cigar_out ? (unsigned long long)r.n_cigar_staged : ~0ULL;
    want.bl_units = (unsigned long long)r.n_bl_units; want.bl = (unsigned long long)r.n_bl;
    static const bool no_link_build = getenv("UZ_BUILD_GENERIC") != nullptr; // (development aid: the general build of the two kernels for every table)
    const bool link_form = uz_link_form(col) && col.cigar_in != nullptr && !no_link_build;
    // the span sums: from the packer (uz_types.h pk_sums: the two kernels below are not launched, k_pack_rec packs from the packer's offsets and holds
    // every span against them), or counted here
    static const bool no_host_sums = getenv("UZ_BUILD_OWN_SUMS") != nullptr; // (development aid: ignore the packer's)
    const bool host_sums = col.pk_sums != nullptr && !no_host_sums;
    static const bool no_lds_build = getenv("UZ_BUILD_FROM_MEMORY") != nullptr; // (development aid: k_pack_rec for every table)
    // (with host sums the scratch of the span sums is free: it holds the packed dictionary)
    const bool from_lds = link_form && host_sums && col.pk_shift == UZ_PK_SHIFT_SMALL && col.n_tup >= 1 && (size_t)col.n_tup * sizeof(uint4) <= uz_rec_scratch_bytes(r.n) &&
                          !col.qpos_wide && !col.bl_wide && (col.tup_n_bl == nullptr || col.bl_pos != nullptr) && !no_lds_build;
    static const bool expand_in_hbm = getenv("UZ_TUP8_IN_HBM") != nullptr; // (development aid: round 5's k_tup_expand in front of k_pack_link too)
    const bool fold_tup8 = col.tup8 != nullptr && from_lds && !expand_in_hbm && (1 << col.pk_shift) == UZ_TUP8_SPAN;
    if (col.tup8 && !fold_tup8) { // every other build reads the 16-bit column from memory: rebuilt there first
        hipLaunchKernelGGL(k_tup_expand, dim3((unsigned)((r.n + UZ_TUP8_SPAN - 1) / UZ_TUP8_SPAN)), dim3(256), 0, st, (int64_t)r.n, col.tup8, col.tup_hot, col.tup_esc,
                           col.tup_esc_off, col.n_tup_esc, (int32_t)col.n_tup, col.tup_out, c->hflags);
        col.tup8 = nullptr; // (the kernels below read col.tup)
    }
    if (host_sums) sums = const_cast<unsigned long long *>(col.pk_sums);
    else if (link_form) hipLaunchKernelGGL((k_off_block_sums<true>), dim3(nb), dim3(256), 0, st, (int64_t)r.n, col, sums);
    else hipLaunchKernelGGL((k_off_block_sums<false>), dim3(nb), dim3(256), 0, st, (int64_t)r.n, col, sums);
    // a table of up to 4096 spans (a chunk of a staged pass: ~2 k): no scan kernel, every workgroup of the second pass adds up the sums in front
    // of its own block; a larger table (the resident 187 M-record one: 46 k spans) gets the one-workgroup scan
    static const bool no_self = getenv("UZ_BUILD_SCAN_KERNEL") != nullptr; // (development aid)
    const bool self = nb <= 4096 && !no_self && !host_sums;
    if (!self && !host_sums) hipLaunchKernelGGL(k_off_scan_sums, dim3(1), dim3(256), 0, st, (int64_t)nb, sums, want, c->hflags);
#define UZ_PACK_LAUNCH(L, S)                                                                                                                              \
    hipLaunchKernelGGL((k_pack_rec<L, S>), dim3(nb), dim3(256), 0, st, (int64_t)r.n, col, (const unsigned long long *)sums, want, (RecA *)r.rec_a, \
                       (RecB *)r.rec_b, r.fm, r.qoff, r.nlow, r.umask, reinterpret_cast<uint32_t *>(r.qlow), r.qs, r.coarse, r.mid, r.mid8, c->hflags, host_sums ? 1 : 0)
    static const bool build_log = getenv("UZ_BUILD_LOG") != nullptr; // (development aid)
    if (build_log)
        fprintf(stderr, "[uz_build_records] n %lld link_form %d host_sums %d pk_shift %d n_tup %lld qpos_wide %d bl_wide %d tup8 %s -> from_lds %d\n", (long long)r.n,
                (int)link_form, (int)host_sums, (int)col.pk_shift, (long long)col.n_tup, (int)col.qpos_wide, (int)col.bl_wide,
                fold_tup8 ? "lds" : (col_in.tup8 ? "hbm" : "none"), (int)from_lds);
    if (from_lds) {
        hipLaunchKernelGGL(k_pack_dict, dim3((unsigned)((col.n_tup + 255) / 256)), dim3(256), 0, st, col, (int32_t)col.n_tup, (uint4 *)off_scratch);
        hipLaunchKernelGGL(k_pack_link, dim3(nb), dim3(256), 0, st, (int64_t)r.n, col, (const unsigned long long *)sums, (int32_t)col.n_tup, (const uint4 *)off_scratch, (RecA *)r.rec_a,
                           (RecB *)r.rec_b, r.fm, r.qoff, r.nlow, r.umask, reinterpret_cast<uint32_t *>(r.qlow), r.qs, r.coarse, r.mid, r.mid8, c->hflags);
    } else if (link_form) { if (self) UZ_PACK_LAUNCH(true, true); else UZ_PACK_LAUNCH(true, false); }
    else { if (self) UZ_PACK_LAUNCH(false, true); else UZ_PACK_LAUNCH(false, false); }
#undef UZ_PACK_LAUNCH
#ifdef UZ_PACK_TIMING
    {
        UZ_HIP(hipStreamSynchronize(st));
        unsigned long long tk[16];
        UZ_HIP(hipMemcpyFromSymbol(tk, HIP_SYMBOL(uz_pack_ticks), sizeof(tk)));
        const char *nm[10] = {"s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9"};
        unsigned long long tot = 0;
        for (int k = 0; k < 10; k++) tot += tk[k];
        fprintf(stderr, "[pack timing] n %lld wgs %u", (long long)r.n, nb);
        for (int k = 0; k < 10; k++) fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * (double)tk[k] / (double)(tot ? tot : 1));
        fprintf(stderr, " | ticks/wg %.0f\n", (double)tot / nb);
        unsigned long long z[16] = {0};
        UZ_HIP(hipMemcpyToSymbol(HIP_SYMBOL(uz_pack_ticks), z, sizeof(z)));
    }
#endif
    if (col.pair_d8)
        hipLaunchKernelGGL(k_pair_link, dim3(nb), dim3(256), 0, st, (int64_t)r.n, (int)col.pk_shift, col.pair_d8, (const RecA *)r.rec_a, (RecB *)r.rec_b,
                           c->hflags);
    // the table arrived with two-bit base rows: expand them into seq4 (the units of list-form records, behind them, were written by
    // k_pack_rec); then the listed bases that are not A/C/G/T, of either kind of record
    if (r.seq2_staged && r.n_seq_units - r.n_bl_units > 0) {
        const size_t nu = (size_t)(r.n_seq_units - r.n_bl_units);
        hipLaunchKernelGGL(k_expand_seq2, dim3((unsigned)std::min<size_t>((nu + 255) / 256, 16384)), dim3(256), 0, st,
                           (const unsigned long long *)r.seq2_staged, (uint4 *)const_cast<uint8_t *>(r.seq4), nu);
    }
    if (r.n_exc > 0 && r.exc_rec) {
        hipLaunchKernelGGL(k_patch_exc, dim3((unsigned)((r.n_exc + 255) / 256)), dim3(256), 0, st, r.n_exc, r.exc_rec, r.exc_pos, r.exc_code,
                           (const RecA *)r.rec_a, (const RecB *)r.rec_b, (const uint16_t *)r.umask, (int64_t)r.n,
                           (uint32_t *)const_cast<uint8_t *>(r.seq4), c->hflags);
        r.n_exc = 0;
    }
    r.seq2_staged = nullptr;
    UZ_HIP(hipGetLastError());
}

void uz_concat_table(uz_ctx *c, hipStream_t st, ReadsDev &dst, const ReadsDev &src, int64_t rec_base, int64_t cigar_base, int64_t unit_base,
                     int64_t seq_base, uint32_t qname_base) {
    if (src.n <= 0) return;
    hipLaunchKernelGGL(k_concat_rec, dim3((unsigned)((src.n + 255) / 256)), dim3(256), 0, st, (int64_t)src.n, (const RecA *)src.rec_a,
                       (const RecB *)src.rec_b, (const uint32_t *)src.fm, (const uint32_t *)src.qoff, (const uint8_t *)src.nlow,
                       (const uint16_t *)src.umask, (const uint16_t *)src.qs, (RecA *)dst.rec_a + rec_base, (RecB *)dst.rec_b + rec_base, dst.fm + rec_base,
                       dst.qoff + rec_base, dst.nlow + rec_base, dst.umask + rec_base, dst.qs + rec_base,
                       (int32_t)rec_base, (uint32_t)cigar_base,
                       (uint32_t)unit_base, (uint32_t)seq_base, qname_base);
    UZ_HIP(hipGetLastError());
    if (src.n_cigar_total)
        UZ_HIP(hipMemcpyAsync(const_cast<uint32_t *>(dst.cigar) + cigar_base, src.cigar, (size_t)src.n_cigar_total * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (src.n_seq_units)
        UZ_HIP(hipMemcpyAsync(const_cast<uint8_t *>(dst.seq4) + (size_t)seq_base * UZ_SEQ4_UNIT_BYTES, src.seq4, (size_t)src.n_seq_units * UZ_SEQ4_UNIT_BYTES,
                              hipMemcpyDeviceToDevice, st));
    if (src.n_plane_units) {
        UZ_HIP(hipMemcpyAsync(dst.qlow + (size_t)unit_base * UZ_QLOW_UNIT_BYTES, src.qlow, (size_t)src.n_plane_units * UZ_QLOW_UNIT_BYTES,
                              hipMemcpyDeviceToDevice, st));
    }
}

void uz_finish_table(uz_ctx *c, hipStream_t st, ReadsDev &r) {
    if (r.n <= 0) return;
    const int64_t nk = (r.n >> 3) + 2;
    hipLaunchKernelGGL(k_build_coarse, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, (const RecA *)r.rec_a, (int64_t)r.n, r.coarse, r.mid, r.mid8);
    UZ_HIP(hipGetLastError());
}

void uz_pack_ascii_rows(uz_ctx *c, hipStream_t st, ReadsDev &r, const uint32_t *cigar_in, const uint32_t *cigar_off_in,
                        const uint8_t *seq_in, const uint32_t *sq_off16_in, uint32_t *cigar_out, uint8_t *seq4_out) {
    if (r.n <= 0) return;
    hipLaunchKernelGGL(k_pack_ascii, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, st, (int64_t)r.n, (const RecA *)r.rec_a,
                       (const RecB *)r.rec_b, cigar_in, cigar_off_in, seq_in, sq_off16_in, cigar_out, seq4_out, r.qs, c->hflags);
    UZ_HIP(hipGetLastError());
}

void uz_build_qlow(uz_ctx *c, hipStream_t st, ReadsDev &r, int min_base_qual) {
    const int thr = min_base_qual < 0 ? 0 : (min_base_qual > 255 ? 256 : min_base_qual);
    if (r.n > 0) {
        hipLaunchKernelGGL(k_build_qlow, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, st, (int64_t)r.n, (const RecA *)r.rec_a,
                           (const RecB *)r.rec_b, (const uint32_t *)r.qoff, (const uint8_t *)r.qual8, (const uint32_t *)r.qual_off16, thr, r.qlow, r.nlow, r.qs);
        UZ_HIP(hipGetLastError());
    }
    r.qlow_thr = min_base_qual;
    r.qlow_valid = true;
}

void uz_check_upload_flag(uz_ctx *c) {
    if (c->hflags[0]) { // set by the header build of an upload (abi.hip) whose commands have now run
        const int f = c->hflags[0];
        c->hflags[0] = 0;
        throw UzError{UZ_E_RANGE, f == 2 ? "SEQ holds a character outside BAM's 16-code alphabet"
                                  : f == 3 ? "exc_* columns of the reads view: an entry names a record without bases, a base beyond l_seq or a code above 15"
                                  : f == 4 ? "qlow_pos / bl_qlow of the reads view: positions of a record are not ascending or lie beyond l_seq, or the set quality bits of its listed bases are not the number its count names"
                                  : f == 5 ? "umask of the reads view: a unit beyond the read's length, or a mask on a read longer than 480 bases"
                                  : f == 6 ? "aux of the reads view: a simple-CIGAR code on a record whose n_cigar is not 1"
                                  : f == 7 ? "mate_d / esc16_* of the reads view: a mate index outside the table"
                                  : f == 8 ? "pair_d8 of the reads view: a SECOND record that no FIRST record names, or one that two of them name"
                                  : f == 10 ? "het_span_off of the family view: a span whose kid-het sites (by gt) are not the number its offsets name"
                                  : f == 9 ? "bl_* of the reads view: a listed base outside the record's unit mask or its length, positions not ascending, a unit of the mask without a listed base, or a list on a record without a mask / without bases"
                                           : "n_cigar_total / n_row_units of the reads view do not match its columns"};
    }
}
