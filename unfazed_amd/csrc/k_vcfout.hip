// k_vcfout.hip -- the record lines of the annotated VCF written on the device (unfazed_hip.h: uz_vcf_rows).  vcf_row.hpp is the body: the rules of
// a line, the three scans of a step, the lane-private walk.  Here: the kernels that run it and the host side of a call; the wavefront, the loop over
// the chunks and the two passes of a chunk are text_out.hpp's.
//
// The text goes up in chunks cut at line ends (UZ_VCFOUT_CHUNK_BYTES, 32 MiB), chunk k + 1 copied on the copy stream while chunk k is worked on:
//   k_vcfout_size  one wavefront per record: the line's output length, or the record handed back (length 0, its flag set)
//   uz_len_scan    exclusive scan of the lengths -> off [n + 1] (one workgroup)
//   k_vcfout_fill  one wavefront per record: the bytes, at in + shift (vcf_row.hpp); no atomics but the OR of a raised flag, no LDS
// FORMAT's piece count and GT slot are found by the host side of the call (uz_vr_format, some twenty bytes a record), not on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "text_out.hpp"
#include "vcf_row.hpp"

#define UZ_VO_PAD 2048 /* readable bytes behind a chunk's text: a step of the walk loads up to 1 KiB beyond the last line end */
#define UZ_VO_WAVES 4  /* records of a workgroup */

namespace {

struct VoArgs {
    int32_t n_rec, n_samples;
    const uint8_t *text;
    const UzVrRec *recs;
    UzVrAnn A;
    uint32_t *len;      // [n_rec]
    const int64_t *off; // [n_rec + 1]
    uint32_t *flags;    // one word, behind off
    uint8_t *hb;        // [n_rec], behind the flag word
    uint8_t *out;
};

__global__ __launch_bounds__(64 * UZ_VO_WAVES) void k_vcfout_size(VoArgs a) {
    const int32_t r = (int32_t)blockIdx.x * UZ_VO_WAVES + (int32_t)(threadIdx.x >> 6);
    if (r >= a.n_rec) return; // (the whole wavefront)
    RowWave w;
    bool hb = false;
    const UzVrRec R = a.recs[r];
    const uint32_t n = uz_vcf_row_walk<false>(w, a.text, R, a.A, a.n_samples, nullptr, 0u, hb);
    if (w.lane() == 0) { a.len[r] = hb ? 0u : n; a.hb[r] = hb ? 1 : 0; }
}

__global__ __launch_bounds__(64 * UZ_VO_WAVES) void k_vcfout_fill(VoArgs a) {
    const int32_t r = (int32_t)blockIdx.x * UZ_VO_WAVES + (int32_t)(threadIdx.x >> 6);
    if (r >= a.n_rec) return;
    const int64_t o0 = a.off[r], o1 = a.off[r + 1];
    if (o1 <= o0) return; // a record handed back
    RowWave w;
    bool hb = false;
    const UzVrRec R = a.recs[r];
    const uint32_t limit = (uint32_t)(o1 - o0);
    const uint32_t n = uz_vcf_row_walk<true>(w, a.text, R, a.A, a.n_samples, a.out + o0, limit, hb);
    if ((hb || n != limit) && w.lane() == 0) atomicOr(a.flags, UZ_VR_F_SIZE);
}

struct Chunk {
    int64_t r0, r1;     // records
    uint64_t t0, bytes; // text [t0, t0 + bytes): from the first line's start (rounded down to 16) to the last line's end
};

struct Image { // where a chunk's inputs lie in its image (the page-locked one and its mirror on the device)
    size_t recs, col, uops, uet, gt, bytes;
};
Image image_of(const Chunk &ck, int64_t n_ann) {
    Image m;
    m.recs = up256((size_t)ck.bytes + UZ_VO_PAD);
    m.col = up256(m.recs + (size_t)(ck.r1 - ck.r0) * sizeof(UzVrRec));
    m.uops = up256(m.col + (size_t)n_ann * 4 + 4);
    m.uet = up256(m.uops + (size_t)n_ann * 4 + 4);
    m.gt = up256(m.uet + (size_t)n_ann + 4);
    m.bytes = up256(m.gt + (size_t)n_ann + 4);
    return m;
}

} // namespace

int uz_vcf_rows_impl(uz_ctx *c, const uz_vcf_text_view *t, const int64_t *line_at, const int64_t *ann_off, const int32_t *ann_col, const uint8_t *ann_gt,
                     const int32_t *ann_uops, const int8_t *ann_uet, int64_t *off, const uint8_t **bytes, uint8_t *handed_back) {
    UZ_REQUIRE(t && off && bytes && t->n_records >= 0 && t->n_records < 0x7FFFFFF0 && t->n_samples >= 0, UZ_E_ARG, "VCF rows: bad arguments");
    const int64_t n = t->n_records;
    UZ_REQUIRE(n == 0 || (t->text && t->samp_at && t->line_end && line_at && ann_off && handed_back), UZ_E_ARG, "VCF rows: bad arguments");
    off[0] = 0;
    *bytes = nullptr;
    c->vo.res.room(64);
    if (n == 0) { *bytes = c->vo.res.p; return 0; }
    UZ_REQUIRE(ann_off[0] == 0, UZ_E_ARG, "VCF rows: the annotation offsets start at 0");
    for (int64_t k = 0; k < n; k++)
        UZ_REQUIRE(ann_off[k + 1] >= ann_off[k] && ann_off[k + 1] - ann_off[k] < ((int64_t)1 << 31), UZ_E_ARG, "VCF rows: the annotation offsets descend");
    UZ_REQUIRE(ann_off[n] == 0 || (ann_col && ann_gt && ann_uops && ann_uet), UZ_E_ARG, "VCF rows: annotations without their table");
    for (int64_t k = 0; k < n; k++) {
        const int64_t a = line_at[k], s = (int64_t)t->samp_at[k], e = (int64_t)t->line_end[k];
        UZ_REQUIRE(a >= 0 && a <= s && s <= e && e <= t->text_bytes && (k == 0 || a >= (int64_t)t->line_end[k - 1]), UZ_E_ARG,
                   "VCF rows: a record's line lies outside the text or before the record ahead of it");
    }
    size_t chunk_bytes = (size_t)32 << 20;
    if (const char *e = getenv("UZ_VCFOUT_CHUNK_BYTES")) { // (read per call: the tests put chunk edges into small files with it)
        const long long v = atoll(e);
        if (v > 0) chunk_bytes = (size_t)v;
    }
    chunk_bytes = std::min<size_t>(chunk_bytes, (size_t)1 << 31);
    // the chunks: whole lines; a line longer than a chunk gets a chunk of its own, one beyond the 32-bit offsets goes back to the host
    const uint64_t span_max = 0xFFFF0000ull;
    std::vector<Chunk> chunks;
    memset(handed_back, 0, (size_t)n);
    for (int64_t i = 0; i < n;) {
        const uint64_t t0 = (uint64_t)line_at[i] & ~(uint64_t)15;
        if (t->line_end[i] - t0 > span_max) { handed_back[i] = 1; i++; continue; }
        int64_t k = i + 1;
        while (k < n && t->line_end[k] - t0 <= chunk_bytes) k++;
        chunks.push_back(Chunk{i, k, t0, t->line_end[k - 1] - t0});
        i = k;
    }
    ChunkLoop L(c, c->vo, chunks.size());
    // a chunk's inputs into its page-locked image, and the image onto the copy stream
    auto stage = [&](size_t q) {
        const Chunk &ck = chunks[q];
        const int64_t a0 = ann_off[ck.r0], n_ann = ann_off[ck.r1] - a0;
        const Image m = image_of(ck, n_ann);
        uint8_t *pin = L.image(q, m.bytes);
        memcpy(pin, t->text + ck.t0, (size_t)ck.bytes);
        memset(pin + ck.bytes, 0, m.recs - (size_t)ck.bytes);
        UzVrRec *recs = reinterpret_cast<UzVrRec *>(pin + m.recs);
        for (int64_t i = ck.r0; i < ck.r1; i++) {
            UzVrRec &R = recs[i - ck.r0];
            R = uz_vr_rec(t->text, ck.t0, (uint64_t)line_at[i], t->samp_at[i], t->line_end[i]);
            R.ann0 = (uint32_t)(ann_off[i] - a0); R.ann1 = (uint32_t)(ann_off[i + 1] - a0);
        }
        if (n_ann) {
            memcpy(pin + m.col, ann_col + a0, (size_t)n_ann * 4);
            memcpy(pin + m.uops, ann_uops + a0, (size_t)n_ann * 4);
            memcpy(pin + m.uet, ann_uet + a0, (size_t)n_ann);
            memcpy(pin + m.gt, ann_gt + a0, (size_t)n_ann);
        }
        L.send(q, m.bytes);
    };
    const RowsPass P{"VCF rows", UZ_K_VCFOUT_SIZE, UZ_K_VCFOUT_FILL, UZ_VO_WAVES, UZ_VR_F_SIZE, 1.02};
    int64_t done = 0; // records placed
    auto skip_to = [&](int64_t r) { // records no chunk holds: handed back by the host side
        for (; done < r; done++) off[done + 1] = L.total;
    };
    if (!chunks.empty()) stage(0);
    for (size_t q = 0; q < chunks.size(); q++) {
        const Chunk &ck = chunks[q];
        const Image m = image_of(ck, ann_off[ck.r1] - ann_off[ck.r0]);
        const uint8_t *img = c->vo.in[q & 1].p;
        skip_to(ck.r0);
        VoArgs a;
        a.n_rec = (int32_t)(ck.r1 - ck.r0); a.n_samples = t->n_samples;
        a.text = img;
        a.recs = reinterpret_cast<const UzVrRec *>(img + m.recs);
        a.A.col = reinterpret_cast<const int32_t *>(img + m.col);
        a.A.uops = reinterpret_cast<const int32_t *>(img + m.uops);
        a.A.uet = reinterpret_cast<const int8_t *>(img + m.uet);
        a.A.gt = img + m.gt;
        uz_rows_chunk<VoArgs, k_vcfout_size, k_vcfout_fill>(L, q, P, a, nullptr, a.n_rec, (double)(t->line_end[n - 1] - chunks[0].t0), (double)std::max<uint64_t>(1, ck.bytes), stage,
                                                            off + ck.r0, nullptr, handed_back + ck.r0);
        done = ck.r1;
    }
    skip_to(n);
    *bytes = c->vo.res.p;
    return 0;
}
