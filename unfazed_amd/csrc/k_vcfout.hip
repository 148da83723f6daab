// k_vcfout.hip -- the record lines of the annotated VCF written on the device (unfazed_hip.h: uz_vcf_rows).  vcf_row.hpp is the body: the rules of
// a line, the three scans of a step, the lane-private walk.  Here: the wavefront that runs it, the launches of a chunk and the host side of a call.
//
// The text goes up in chunks cut at line ends (UZ_VCFOUT_CHUNK_BYTES, 32 MiB), chunk k + 1 copied on the copy stream while chunk k is worked on:
//   k_vcfout_size  one wavefront per record: the line's output length, or the record handed back (length 0, its flag set)
//   k_vcfout_scan  exclusive scan of the lengths -> off [n + 1] (one workgroup)
//   k_vcfout_fill  one wavefront per record: the bytes, at in + shift (vcf_row.hpp); no atomics but the OR of a raised flag, no LDS
// FORMAT's piece count and GT slot are found by the host side of the call (uz_vr_format, some twenty bytes a record), not on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "uz_ctx.hpp"
#include "vcf_row.hpp"

#define UZ_VO_PAD 2048 /* readable bytes behind a chunk's text: a step of the walk loads up to 1 KiB beyond the last line end */
#define UZ_VO_WAVES 4  /* records of a workgroup */

namespace {

struct VoWave { // the 64 lanes of a wavefront share a record
    static constexpr uint32_t LANES = 64;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x & 63u; }
    __device__ __forceinline__ uint32_t shfl_up(uint32_t v, uint32_t d) const { return (uint32_t)__shfl_up((int)v, d, 64); }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ bool any(bool v) const { return __any(v ? 1 : 0) != 0; }
};

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
    VoWave w;
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
    VoWave w;
    bool hb = false;
    const UzVrRec R = a.recs[r];
    const uint32_t limit = (uint32_t)(o1 - o0);
    const uint32_t n = uz_vcf_row_walk<true>(w, a.text, R, a.A, a.n_samples, a.out + o0, limit, hb);
    if ((hb || n != limit) && w.lane() == 0) atomicOr(a.flags, UZ_VR_F_SIZE);
}

// off[k] = sum of len[0 .. k), off[n] the total: one workgroup of 1024 lanes, a tile of 1024 lengths per round
__global__ __launch_bounds__(1024) void k_vcfout_scan(int32_t n, const uint32_t *__restrict__ len, int64_t *__restrict__ off) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry_s;
    const uint32_t t = threadIdx.x, l = t & 63u, wv = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int32_t base = 0; base < n; base += 1024) {
        const int32_t i = base + (int32_t)t;
        const unsigned long long v = i < n ? (unsigned long long)len[i] : 0ull;
        unsigned long long x = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long y = (unsigned long long)__shfl_up((long long)x, d, 64);
            if (l >= d) x += y;
        }
        if (l == 63) wave_sum[wv] = x;
        __syncthreads();
        unsigned long long before = carry_s;
        for (uint32_t k = 0; k < wv; k++) before += wave_sum[k];
        if (i < n) off[i] = (int64_t)(before + x - v);
        __syncthreads();
        if (t == 1023) carry_s = before + x;
        __syncthreads();
    }
    if (t == 0) off[n] = (int64_t)carry_s;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

void pin_room(uint8_t *&p, size_t &cap, size_t need, size_t keep) { // a page-locked block grown to `need`, its first `keep` bytes carried over
    if (cap >= need) return;
    const size_t want = need + need / 4 + 4096;
    uint8_t *q = nullptr;
    UZ_HIP(hipHostMalloc((void **)&q, want, hipHostMallocDefault));
    if (keep) memcpy(q, p, keep);
    if (p) (void)hipHostFree(p);
    p = q; cap = want;
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
    pin_room(c->vo_res, c->vo_res_cap, 64, 0);
    if (n == 0) { *bytes = c->vo_res; return 0; }
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
    hipEvent_t copied[2] = {nullptr, nullptr};
    auto cleanup = [&] {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
        for (int b = 0; b < 2; b++)
            if (copied[b]) (void)hipEventDestroy(copied[b]);
    };
    // a chunk's inputs into its page-locked image, and the image onto the copy stream
    auto stage = [&](size_t q) {
        const Chunk &ck = chunks[q];
        const int b = (int)(q & 1);
        const int64_t a0 = ann_off[ck.r0], n_ann = ann_off[ck.r1] - a0;
        const Image m = image_of(ck, n_ann);
        pin_room(c->vo_pin[b], c->vo_pin_cap[b], m.bytes, 0);
        c->vo_in[b].ensure(m.bytes + 64);
        uint8_t *pin = c->vo_pin[b];
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
        UZ_HIP(hipMemcpyAsync(c->vo_in[b].p, pin, m.bytes, hipMemcpyHostToDevice, c->copy_stream));
        UZ_HIP(hipEventRecord(copied[b], c->copy_stream));
    };
    try {
        for (int b = 0; b < 2 && b < (int)chunks.size(); b++) UZ_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
        hipStream_t st = c->stream;
        int64_t total = 0, done = 0; // bytes written, records placed
        auto skip_to = [&](int64_t r) { // records no chunk holds: handed back by the host side
            for (; done < r; done++) off[done + 1] = total;
        };
        if (!chunks.empty()) stage(0);
        for (size_t q = 0; q < chunks.size(); q++) {
            const Chunk &ck = chunks[q];
            const int b = (int)(q & 1);
            const int32_t nr = (int32_t)(ck.r1 - ck.r0);
            const Image m = image_of(ck, ann_off[ck.r1] - ann_off[ck.r0]);
            skip_to(ck.r0);
            const size_t o_flag = ((size_t)nr + 1) * 8, o_hb = o_flag + 8, res_bytes = (o_hb + (size_t)nr + 15) & ~(size_t)15;
            c->vo_len.ensure((size_t)nr + 16);
            c->vo_off.ensure(res_bytes + 64);
            pin_room(c->vo_small, c->vo_small_cap, res_bytes, 0);
            VoArgs a;
            a.n_rec = nr; a.n_samples = t->n_samples;
            a.text = c->vo_in[b].p;
            a.recs = reinterpret_cast<const UzVrRec *>(c->vo_in[b].p + m.recs);
            a.A.col = reinterpret_cast<const int32_t *>(c->vo_in[b].p + m.col);
            a.A.uops = reinterpret_cast<const int32_t *>(c->vo_in[b].p + m.uops);
            a.A.uet = reinterpret_cast<const int8_t *>(c->vo_in[b].p + m.uet);
            a.A.gt = c->vo_in[b].p + m.gt;
            a.len = c->vo_len.p;
            a.off = reinterpret_cast<const int64_t *>(c->vo_off.p);
            a.flags = reinterpret_cast<uint32_t *>(c->vo_off.p + o_flag);
            a.hb = c->vo_off.p + o_hb;
            a.out = nullptr;
            const unsigned grid = (unsigned)((nr + UZ_VO_WAVES - 1) / UZ_VO_WAVES);
            UZ_HIP(hipStreamWaitEvent(st, copied[b], 0));
            UZ_HIP(hipMemsetAsync(c->vo_off.p + o_flag, 0, 8, st));
            {
                ProfScope ps(c, UZ_K_VCFOUT_SIZE);
                hipLaunchKernelGGL(k_vcfout_size, dim3(grid), dim3(64 * UZ_VO_WAVES), 0, st, a);
                UZ_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_vcfout_scan, dim3(1), dim3(1024), 0, st, nr, (const uint32_t *)c->vo_len.p, reinterpret_cast<int64_t *>(c->vo_off.p));
                UZ_HIP(hipGetLastError());
            }
            uz_kcopy(c, c->vo_small, c->vo_off.p, res_bytes);
            if (q + 1 < chunks.size()) stage(q + 1); // (its image and its block were chunk q - 1's, which is done)
            UZ_HIP(hipStreamSynchronize(st));
            const int64_t *off_h = reinterpret_cast<const int64_t *>(c->vo_small);
            const int64_t len = off_h[nr];
            UZ_REQUIRE(len >= 0 && len < ((int64_t)1 << 32), UZ_E_RANGE, "VCF rows: 4 GiB or more of text from one chunk");
            for (int32_t r = 0; r < nr; r++) {
                off[ck.r0 + r + 1] = total + off_h[r + 1];
                handed_back[ck.r0 + r] = c->vo_small[o_hb + (size_t)r];
            }
            done = ck.r1;
            if (len) {
                const size_t text = ((size_t)len + 15) & ~(size_t)15;
                c->vo_out.ensure(text + 64);
                // (the first chunk sizes the block for the whole call at its own rate of growth, so that it is allocated once)
                const size_t guess = q == 0 ? (size_t)((double)text * 1.02 * (double)(t->line_end[n - 1] - chunks[0].t0) / (double)std::max<uint64_t>(1, ck.bytes)) : 0;
                pin_room(c->vo_res, c->vo_res_cap, std::max((size_t)total + text + 16, guess), (size_t)total);
                a.out = c->vo_out.p;
                {
                    ProfScope ps(c, UZ_K_VCFOUT_FILL);
                    hipLaunchKernelGGL(k_vcfout_fill, dim3(grid), dim3(64 * UZ_VO_WAVES), 0, st, a);
                    UZ_HIP(hipGetLastError());
                }
                UZ_HIP(hipMemcpyAsync(c->vo_res + total, c->vo_out.p, (size_t)len, hipMemcpyDeviceToHost, st));
                uz_kcopy(c, c->vo_small, a.flags, 8);
                UZ_HIP(hipStreamSynchronize(st));
                UZ_REQUIRE(!(*reinterpret_cast<const uint32_t *>(c->vo_small) & UZ_VR_F_SIZE), UZ_E_STATE, "VCF rows: a record's written bytes differ from its sized length");
                total += len;
            }
        }
        skip_to(n);
    } catch (...) { cleanup(); throw; }
    cleanup();
    *bytes = c->vo_res;
    return 0;
}
