// k_bcfout.hip -- the records of a BCF turned into VCF text lines on the device (unfazed_hip.h: uz_bcf_rows).  bcf_row.hpp is the body: the rules of
// a line, the uniform walk of the shared block, the lanes over samples.  Here: the kernels that run it and the host side of a call; the wavefront,
// the loop over the chunks and the two passes of a chunk are text_out.hpp's.
//
// The record bytes go up in chunks cut at record ends (UZ_BCFOUT_CHUNK_BYTES, 32 MiB), chunk k + 1 copied on the copy stream while chunk k is worked
// on; the dictionary and the contig names ride in every chunk's image (a few KiB):
//   k_bcfout_size  one wavefront per record: the line's length, where column 10 starts in it, or the record handed back (length 0, its flag set)
//   uz_len_scan    exclusive scan of the lengths -> off [n + 1] (one workgroup)
//   k_bcfout_fill  one wavefront per record: the bytes; no atomics but the OR of a raised flag, no LDS
// The buffers are the call's own (uz_ctx::bo): the text it returns is the input of the uz_vcf_rows call behind it, which has its own (uz_ctx::vo).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bcf_row.hpp"
#include "text_out.hpp"

#define UZ_BO_PAD 256  /* zero bytes behind a chunk's records (the body reads none of them) */
#define UZ_BO_WAVES 4  /* records of a workgroup */

namespace {

struct BoArgs {
    int32_t n_rec, reserved0;
    UzBrTables T;
    const uint64_t *rec_at; // [n_rec] in T.data
    uint32_t *len;          // [n_rec]
    const int64_t *off;     // [n_rec + 1]
    uint32_t *flags;        // one word, behind off
    uint32_t *samp;         // [n_rec], behind the flag word
    uint8_t *hb;            // [n_rec], behind samp
    uint8_t *out;
};

__global__ __launch_bounds__(64 * UZ_BO_WAVES) void k_bcfout_size(BoArgs a) {
    const int32_t r = (int32_t)blockIdx.x * UZ_BO_WAVES + (int32_t)(threadIdx.x >> 6);
    if (r >= a.n_rec) return; // (the whole wavefront)
    RowWave w;
    bool hb = false;
    uint32_t samp = 0;
    const uint32_t n = uz_bcf_row_walk<false>(w, a.T, a.rec_at[r], nullptr, 0u, samp, hb);
    if (w.lane() == 0) { a.len[r] = hb ? 0u : n; a.samp[r] = hb ? 0u : samp; a.hb[r] = hb ? 1 : 0; }
}

__global__ __launch_bounds__(64 * UZ_BO_WAVES) void k_bcfout_fill(BoArgs a) {
    const int32_t r = (int32_t)blockIdx.x * UZ_BO_WAVES + (int32_t)(threadIdx.x >> 6);
    if (r >= a.n_rec) return;
    const int64_t o0 = a.off[r], o1 = a.off[r + 1];
    if (o1 <= o0) return; // a record handed back
    RowWave w;
    bool hb = false;
    uint32_t samp = 0;
    const uint32_t limit = (uint32_t)(o1 - o0);
    const uint32_t n = uz_bcf_row_walk<true>(w, a.T, a.rec_at[r], a.out + o0, limit, samp, hb);
    if ((hb || n != limit) && w.lane() == 0) atomicOr(a.flags, UZ_BR_F_SIZE);
}

struct Chunk {
    int64_t r0, r1;     // records
    uint64_t t0, bytes; // data [t0, t0 + bytes): from the first record's start (rounded down to 16) to the furthest end of its records
};

struct Image { // where a chunk's inputs lie in its image (the page-locked one and its mirror on the device)
    size_t rec_at, dict_off, dict_bytes, ctg_off, ctg_bytes, bytes;
};
Image image_of(const Chunk &ck, const uz_bcf_lines_view *v) {
    Image m;
    m.rec_at = up256((size_t)ck.bytes + UZ_BO_PAD);
    m.dict_off = up256(m.rec_at + (size_t)(ck.r1 - ck.r0) * 8);
    m.dict_bytes = up256(m.dict_off + ((size_t)v->n_dict + 1) * 4);
    m.ctg_off = up256(m.dict_bytes + (size_t)v->dict_off[v->n_dict] + 4);
    m.ctg_bytes = up256(m.ctg_off + ((size_t)v->n_contigs + 1) * 4);
    m.bytes = up256(m.ctg_bytes + (size_t)v->contig_off[v->n_contigs] + 4);
    return m;
}

} // namespace

int uz_bcf_rows_impl(uz_ctx *c, const uz_bcf_lines_view *v, int64_t *off, uint64_t *samp_at, const uint8_t **bytes, uint8_t *handed_back) {
    UZ_REQUIRE(v && off && bytes && v->n_records >= 0 && v->n_records < 0x7FFFFFF0 && v->n_samples >= 0 && v->n_samples < (1 << 24) && v->data_bytes >= 0, UZ_E_ARG,
               "BCF rows: bad arguments");
    const int64_t n = v->n_records;
    UZ_REQUIRE(n == 0 || (v->data && v->rec_at && samp_at && handed_back), UZ_E_ARG, "BCF rows: bad arguments");
    UZ_REQUIRE(v->n_dict >= 0 && v->n_contigs >= 0 && v->dict_off && v->contig_off && v->dict_off[0] == 0 && v->contig_off[0] == 0, UZ_E_ARG,
               "BCF rows: the dictionary or the contigs are missing");
    for (int32_t k = 0; k < v->n_dict; k++) UZ_REQUIRE(v->dict_off[k + 1] >= v->dict_off[k], UZ_E_ARG, "BCF rows: the dictionary's offsets descend");
    for (int32_t k = 0; k < v->n_contigs; k++) UZ_REQUIRE(v->contig_off[k + 1] >= v->contig_off[k], UZ_E_ARG, "BCF rows: the contigs' offsets descend");
    UZ_REQUIRE((v->dict_off[v->n_dict] == 0 || v->dict_bytes) && (v->contig_off[v->n_contigs] == 0 || v->contig_bytes), UZ_E_ARG, "BCF rows: names without their bytes");
    off[0] = 0;
    *bytes = nullptr;
    c->bo.res.room(64);
    if (n == 0) { *bytes = c->bo.res.p; return 0; }
    const uint64_t size = (uint64_t)v->data_bytes;
    for (int64_t k = 0; k < n; k++)
        UZ_REQUIRE(v->rec_at[k] <= size && (k == 0 || v->rec_at[k] >= v->rec_at[k - 1]), UZ_E_ARG, "BCF rows: a record's offset lies outside the data or before the record ahead of it");
    size_t chunk_bytes = (size_t)32 << 20;
    if (const char *e = getenv("UZ_BCFOUT_CHUNK_BYTES")) { // (read per call: the tests put chunk edges into small files with it)
        const long long x = atoll(e);
        if (x > 0) chunk_bytes = (size_t)x;
    }
    chunk_bytes = std::min<size_t>(chunk_bytes, (size_t)1 << 31);
    // where a record says it ends, held inside the data (a record that says more is handed back by the body, which sees the chunk's end)
    auto end_of = [&](int64_t k) -> uint64_t {
        const uint64_t a = v->rec_at[k];
        if (size - a < 8) return size;
        const uint64_t ls = uz_br_rd32(v->data + a), li = uz_br_rd32(v->data + a + 4);
        return std::min<uint64_t>(size, a + 8 + ls + li);
    };
    // the chunks: whole records; a record longer than a chunk gets a chunk of its own, one beyond the 32-bit sizes goes back to the host
    const uint64_t span_max = 0xFFFF0000ull;
    std::vector<Chunk> chunks;
    memset(handed_back, 0, (size_t)n);
    for (int64_t i = 0; i < n;) {
        const uint64_t t0 = v->rec_at[i] & ~(uint64_t)15;
        uint64_t end = end_of(i);
        if (end - t0 > span_max) { handed_back[i] = 1; i++; continue; }
        int64_t k = i + 1;
        while (k < n) {
            const uint64_t e = std::max(end, end_of(k));
            if (e - t0 > chunk_bytes) break;
            end = e;
            k++;
        }
        chunks.push_back(Chunk{i, k, t0, end - t0});
        i = k;
    }
    ChunkLoop L(c, c->bo, chunks.size());
    // a chunk's inputs into its page-locked image, and the image onto the copy stream
    auto stage = [&](size_t q) {
        const Chunk &ck = chunks[q];
        const Image m = image_of(ck, v);
        uint8_t *pin = L.image(q, m.bytes);
        memcpy(pin, v->data + ck.t0, (size_t)ck.bytes);
        memset(pin + ck.bytes, 0, m.rec_at - (size_t)ck.bytes);
        uint64_t *rec = reinterpret_cast<uint64_t *>(pin + m.rec_at);
        for (int64_t i = ck.r0; i < ck.r1; i++) rec[i - ck.r0] = v->rec_at[i] - ck.t0;
        memcpy(pin + m.dict_off, v->dict_off, ((size_t)v->n_dict + 1) * 4);
        if (v->dict_off[v->n_dict]) memcpy(pin + m.dict_bytes, v->dict_bytes, v->dict_off[v->n_dict]);
        memcpy(pin + m.ctg_off, v->contig_off, ((size_t)v->n_contigs + 1) * 4);
        if (v->contig_off[v->n_contigs]) memcpy(pin + m.ctg_bytes, v->contig_bytes, v->contig_off[v->n_contigs]);
        L.send(q, m.bytes);
    };
    const RowsPass P{"BCF rows", UZ_K_BCFOUT_SIZE, UZ_K_BCFOUT_FILL, UZ_BO_WAVES, UZ_BR_F_SIZE, 1.02};
    int64_t done = 0; // records placed
    auto skip_to = [&](int64_t r) { // records no chunk holds: handed back by the host side
        for (; done < r; done++) { off[done + 1] = L.total; samp_at[done] = (uint64_t)L.total; }
    };
    if (!chunks.empty()) stage(0);
    for (size_t q = 0; q < chunks.size(); q++) {
        const Chunk &ck = chunks[q];
        const Image m = image_of(ck, v);
        const uint8_t *img = c->bo.in[q & 1].p;
        skip_to(ck.r0);
        BoArgs a;
        a.n_rec = (int32_t)(ck.r1 - ck.r0); a.reserved0 = 0;
        a.T.data = img; a.T.data_bytes = ck.bytes;
        a.T.dict_off = reinterpret_cast<const uint32_t *>(img + m.dict_off); a.T.dict_bytes = img + m.dict_bytes;
        a.T.ctg_off = reinterpret_cast<const uint32_t *>(img + m.ctg_off); a.T.ctg_bytes = img + m.ctg_bytes;
        a.T.n_dict = (uint32_t)v->n_dict; a.T.n_ctg = (uint32_t)v->n_contigs;
        a.T.n_samples = (uint32_t)v->n_samples; a.T.reserved0 = 0;
        a.rec_at = reinterpret_cast<const uint64_t *>(img + m.rec_at);
        uz_rows_chunk<BoArgs, k_bcfout_size, k_bcfout_fill>(L, q, P, a, &a.samp, a.n_rec, (double)(size - chunks[0].t0), (double)std::max<uint64_t>(1, ck.bytes), stage, off + ck.r0,
                                                            samp_at + ck.r0, handed_back + ck.r0);
        done = ck.r1;
    }
    skip_to(n);
    *bytes = c->bo.res.p;
    return 0;
}
