// k_bcfout.hip -- the records of a BCF turned into VCF text lines on the device (unfazed_hip.h: uz_bcf_rows).  bcf_row.hpp is the body: the rules of
// a line, the uniform walk of the shared block, the lanes over samples.  Here: the wavefront that runs it, the launches of a chunk and the host side
// of a call.
//
// The record bytes go up in chunks cut at record ends (UZ_BCFOUT_CHUNK_BYTES, 32 MiB), chunk k + 1 copied on the copy stream while chunk k is worked
// on; the dictionary and the contig names ride in every chunk's image (a few KiB):
//   k_bcfout_size  one wavefront per record: the line's length, where column 10 starts in it, or the record handed back (length 0, its flag set)
//   k_bcfout_scan  exclusive scan of the lengths -> off [n + 1] (one workgroup)
//   k_bcfout_fill  one wavefront per record: the bytes; no atomics but the OR of a raised flag, no LDS
// The buffers are the call's own (bo_*): the text it returns is the input of the uz_vcf_rows call behind it, which has its own (vo_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bcf_row.hpp"
#include "uz_ctx.hpp"

#define UZ_BO_PAD 256  /* zero bytes behind a chunk's records (the body reads none of them) */
#define UZ_BO_WAVES 4  /* records of a workgroup */

namespace {

struct BoWave { // the 64 lanes of a wavefront share a record
    static constexpr uint32_t LANES = 64;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x & 63u; }
    __device__ __forceinline__ uint32_t shfl_up(uint32_t v, uint32_t d) const { return (uint32_t)__shfl_up((int)v, d, 64); }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ bool any(bool v) const { return __any(v ? 1 : 0) != 0; }
};

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
    BoWave w;
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
    BoWave w;
    bool hb = false;
    uint32_t samp = 0;
    const uint32_t limit = (uint32_t)(o1 - o0);
    const uint32_t n = uz_bcf_row_walk<true>(w, a.T, a.rec_at[r], a.out + o0, limit, samp, hb);
    if ((hb || n != limit) && w.lane() == 0) atomicOr(a.flags, UZ_BR_F_SIZE);
}

// off[k] = sum of len[0 .. k), off[n] the total: one workgroup of 1024 lanes, a tile of 1024 lengths per round (k_bed_scan's, k_vcfout_scan's)
__global__ __launch_bounds__(1024) void k_bcfout_scan(int32_t n, const uint32_t *__restrict__ len, int64_t *__restrict__ off) {
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
    pin_room(c->bo_res, c->bo_res_cap, 64, 0);
    if (n == 0) { *bytes = c->bo_res; return 0; }
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
        const Image m = image_of(ck, v);
        pin_room(c->bo_pin[b], c->bo_pin_cap[b], m.bytes, 0);
        c->bo_in[b].ensure(m.bytes + 64);
        uint8_t *pin = c->bo_pin[b];
        memcpy(pin, v->data + ck.t0, (size_t)ck.bytes);
        memset(pin + ck.bytes, 0, m.rec_at - (size_t)ck.bytes);
        uint64_t *rec = reinterpret_cast<uint64_t *>(pin + m.rec_at);
        for (int64_t i = ck.r0; i < ck.r1; i++) rec[i - ck.r0] = v->rec_at[i] - ck.t0;
        memcpy(pin + m.dict_off, v->dict_off, ((size_t)v->n_dict + 1) * 4);
        if (v->dict_off[v->n_dict]) memcpy(pin + m.dict_bytes, v->dict_bytes, v->dict_off[v->n_dict]);
        memcpy(pin + m.ctg_off, v->contig_off, ((size_t)v->n_contigs + 1) * 4);
        if (v->contig_off[v->n_contigs]) memcpy(pin + m.ctg_bytes, v->contig_bytes, v->contig_off[v->n_contigs]);
        UZ_HIP(hipMemcpyAsync(c->bo_in[b].p, pin, m.bytes, hipMemcpyHostToDevice, c->copy_stream));
        UZ_HIP(hipEventRecord(copied[b], c->copy_stream));
    };
    try {
        for (int b = 0; b < 2 && b < (int)chunks.size(); b++) UZ_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
        hipStream_t st = c->stream;
        int64_t total = 0, done = 0; // bytes written, records placed
        auto skip_to = [&](int64_t r) { // records no chunk holds: handed back by the host side
            for (; done < r; done++) { off[done + 1] = total; samp_at[done] = (uint64_t)total; }
        };
        if (!chunks.empty()) stage(0);
        for (size_t q = 0; q < chunks.size(); q++) {
            const Chunk &ck = chunks[q];
            const int b = (int)(q & 1);
            const int32_t nr = (int32_t)(ck.r1 - ck.r0);
            const Image m = image_of(ck, v);
            skip_to(ck.r0);
            const size_t o_flag = ((size_t)nr + 1) * 8, o_samp = o_flag + 8, o_hb = o_samp + (size_t)nr * 4, res_bytes = (o_hb + (size_t)nr + 15) & ~(size_t)15;
            c->bo_len.ensure((size_t)nr + 16);
            c->bo_off.ensure(res_bytes + 64);
            pin_room(c->bo_small, c->bo_small_cap, res_bytes, 0);
            const uint8_t *img = c->bo_in[b].p;
            BoArgs a;
            a.n_rec = nr; a.reserved0 = 0;
            a.T.data = img; a.T.data_bytes = ck.bytes;
            a.T.dict_off = reinterpret_cast<const uint32_t *>(img + m.dict_off); a.T.dict_bytes = img + m.dict_bytes;
            a.T.ctg_off = reinterpret_cast<const uint32_t *>(img + m.ctg_off); a.T.ctg_bytes = img + m.ctg_bytes;
            a.T.n_dict = (uint32_t)v->n_dict; a.T.n_ctg = (uint32_t)v->n_contigs;
            a.T.n_samples = (uint32_t)v->n_samples; a.T.reserved0 = 0;
            a.rec_at = reinterpret_cast<const uint64_t *>(img + m.rec_at);
            a.len = c->bo_len.p;
            a.off = reinterpret_cast<const int64_t *>(c->bo_off.p);
            a.flags = reinterpret_cast<uint32_t *>(c->bo_off.p + o_flag);
            a.samp = reinterpret_cast<uint32_t *>(c->bo_off.p + o_samp);
            a.hb = c->bo_off.p + o_hb;
            a.out = nullptr;
            const unsigned grid = (unsigned)((nr + UZ_BO_WAVES - 1) / UZ_BO_WAVES);
            UZ_HIP(hipStreamWaitEvent(st, copied[b], 0));
            UZ_HIP(hipMemsetAsync(c->bo_off.p + o_flag, 0, 8, st));
            {
                ProfScope ps(c, UZ_K_BCFOUT_SIZE);
                hipLaunchKernelGGL(k_bcfout_size, dim3(grid), dim3(64 * UZ_BO_WAVES), 0, st, a);
                UZ_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_bcfout_scan, dim3(1), dim3(1024), 0, st, nr, (const uint32_t *)c->bo_len.p, reinterpret_cast<int64_t *>(c->bo_off.p));
                UZ_HIP(hipGetLastError());
            }
            uz_kcopy(c, c->bo_small, c->bo_off.p, res_bytes);
            if (q + 1 < chunks.size()) stage(q + 1); // (its image and its block were chunk q - 1's, which is done)
            UZ_HIP(hipStreamSynchronize(st));
            const int64_t *off_h = reinterpret_cast<const int64_t *>(c->bo_small);
            const uint32_t *samp_h = reinterpret_cast<const uint32_t *>(c->bo_small + o_samp);
            const int64_t len = off_h[nr];
            UZ_REQUIRE(len >= 0 && len < ((int64_t)1 << 32), UZ_E_RANGE, "BCF rows: 4 GiB or more of text from one chunk");
            for (int32_t r = 0; r < nr; r++) {
                off[ck.r0 + r + 1] = total + off_h[r + 1];
                samp_at[ck.r0 + r] = (uint64_t)(total + off_h[r]) + samp_h[r];
                handed_back[ck.r0 + r] = c->bo_small[o_hb + (size_t)r];
            }
            done = ck.r1;
            if (len) {
                const size_t text = ((size_t)len + 15) & ~(size_t)15;
                c->bo_out.ensure(text + 64);
                // (the first chunk sizes the block for the whole call at its own rate of growth, so that it is allocated once)
                const size_t guess = q == 0 ? (size_t)((double)text * 1.02 * (double)(size - chunks[0].t0) / (double)std::max<uint64_t>(1, ck.bytes)) : 0;
                pin_room(c->bo_res, c->bo_res_cap, std::max((size_t)total + text + 16, guess), (size_t)total);
                a.out = c->bo_out.p;
                {
                    ProfScope ps(c, UZ_K_BCFOUT_FILL);
                    hipLaunchKernelGGL(k_bcfout_fill, dim3(grid), dim3(64 * UZ_BO_WAVES), 0, st, a);
                    UZ_HIP(hipGetLastError());
                }
                UZ_HIP(hipMemcpyAsync(c->bo_res + total, c->bo_out.p, (size_t)len, hipMemcpyDeviceToHost, st));
                uz_kcopy(c, c->bo_small, a.flags, 8);
                UZ_HIP(hipStreamSynchronize(st));
                UZ_REQUIRE(!(*reinterpret_cast<const uint32_t *>(c->bo_small) & UZ_BR_F_SIZE), UZ_E_STATE, "BCF rows: a record's written bytes differ from its sized length");
                total += len;
            }
        }
        skip_to(n);
    } catch (...) { cleanup(); throw; }
    cleanup();
    *bytes = c->bo_res;
    return 0;
}
