// text_out.hpp -- what the calls that turn device results into a file's bytes share (k_bed.hip, k_vcfout.hip, k_bcfout.hip, k_deflate.hip): the
// wavefront of a row, the loop over a call's chunks, the two passes of a chunk of rows.  The length scan (uz_len_scan), the page-locked block (PinBuf)
// and a call's buffers (OutBufs) are in uz_ctx.hpp.
#pragma once
#include <algorithm>
#include <string>

#include "uz_ctx.hpp"

struct RowWave { // the 64 lanes of a wavefront share a row (what bed_row.hpp, vcf_row.hpp and bcf_row.hpp ask of a wave)
    static constexpr uint32_t LANES = 64;
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x & 63u; }
    __device__ __forceinline__ uint32_t shfl_up(uint32_t v, uint32_t d) const { return (uint32_t)__shfl_up((int)v, d, 64); }
    __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t src) const { return (uint32_t)__shfl((int)v, (int)src, 64); }
    __device__ __forceinline__ bool any(bool v) const { return __any(v ? 1 : 0) != 0; }
    __device__ __forceinline__ uint32_t excl_scan(uint32_t v, uint32_t &total) const {
        uint32_t x = v;
        const uint32_t l = lane();
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
            if (l >= d) x += y;
        }
        total = (uint32_t)__shfl((int)x, 63, 64);
        return x - v;
    }
    __device__ __forceinline__ const uint8_t *bcast_ptr(const uint8_t *p, uint32_t src) const {
        const uint64_t a = (uint64_t)(uintptr_t)p;
        const uint32_t lo = bcast((uint32_t)a, src), hi = bcast((uint32_t)(a >> 32), src);
        return (const uint8_t *)(uintptr_t)((uint64_t)hi << 32 | lo);
    }
};

// A call's chunks: chunk q goes up through image q & 1 on the copy stream while chunk q - 1 is worked on, and what it yields lands behind the
// `total` bytes of the call's result block.  How chunks are cut, what an image holds and which kernels run are the call's.  Both streams are
// drained when the loop goes, however it goes.
struct ChunkLoop {
    uz_ctx *c;
    OutBufs &B;
    size_t n_chunks;
    int64_t total = 0;
    hipEvent_t copied[2] = {nullptr, nullptr};
    ChunkLoop(uz_ctx *c_, OutBufs &B_, size_t n_chunks_) : c(c_), B(B_), n_chunks(n_chunks_) {}
    ChunkLoop(const ChunkLoop &) = delete;
    ~ChunkLoop() {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
        for (int b = 0; b < 2; b++)
            if (copied[b]) (void)hipEventDestroy(copied[b]);
    }
    uint8_t *image(size_t q, size_t bytes) { // the page-locked image of chunk q, for the call to fill
        B.pin[q & 1].room(bytes);
        B.in[q & 1].ensure(bytes + 64);
        return B.pin[q & 1].p;
    }
    void send(size_t q, size_t bytes) { // ... and the filled image onto the copy stream
        const int b = (int)(q & 1);
        if (!copied[b]) UZ_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
        UZ_HIP(hipMemcpyAsync(B.in[b].p, B.pin[b].p, bytes, hipMemcpyHostToDevice, c->copy_stream));
        UZ_HIP(hipEventRecord(copied[b], c->copy_stream));
    }
    void wait(size_t q) { UZ_HIP(hipStreamWaitEvent(c->stream, copied[q & 1], 0)); } // the compute stream behind chunk q's copy
    // behind chunk q's launches: the next chunk staged (its image and its block were chunk q - 1's, which is done), then the wait for chunk q
    template <typename Stage>
    void turn(size_t q, Stage &&stage) {
        if (q + 1 < n_chunks) stage(q + 1);
        UZ_HIP(hipStreamSynchronize(c->stream));
    }
    // room for `bytes` more of the result.  The first chunk sizes the block for the whole call at its own rate of growth (growth * full / part
    // + extra), so that it is allocated once
    void result_room(size_t q, size_t bytes, double growth, double full, double part, size_t extra = 0) {
        const size_t guess = q == 0 ? (size_t)((double)bytes * growth * full / part) + extra : 0;
        B.res.room(std::max((size_t)total + bytes + 16, guess), (size_t)total);
    }
    void fetch(const uint8_t *src, size_t len) { UZ_HIP(hipMemcpyAsync(B.res.p + total, src, len, hipMemcpyDeviceToHost, c->stream)); }
};

struct RowsPass { // what the two passes of a row writer are called and counted as
    const char *what;   // in the error texts
    int k_size, k_fill; // profiling slots
    unsigned waves;     // rows of a workgroup
    uint32_t f_size;    // the flag of the fill pass
    double growth;      // text out per byte in: the margin of the first chunk's guess
};

// Chunk q of a row writer, nr rows whose inputs `a` names already: the sizing pass, the scan, the small results back (off [nr + 1], the flag word,
// samp [nr] where the call has that column, the handed-back bytes), the fill pass, the text behind L.total.  off / samp_at / handed_back: the call's
// columns at the chunk's first row.  full / part: the call's input over the chunk's (ChunkLoop::result_room)
template <typename Args, void (*Size)(Args), void (*Fill)(Args), typename Stage>
void uz_rows_chunk(ChunkLoop &L, size_t q, const RowsPass &P, Args &a, uint32_t **samp, int32_t nr, double full, double part, Stage &&stage, int64_t *off,
                   uint64_t *samp_at, uint8_t *handed_back) {
    uz_ctx *c = L.c;
    OutBufs &B = L.B;
    hipStream_t st = c->stream;
    const size_t o_flag = ((size_t)nr + 1) * 8, o_samp = o_flag + 8, o_hb = o_samp + (samp ? (size_t)nr * 4 : 0), res_bytes = (o_hb + (size_t)nr + 15) & ~(size_t)15;
    B.len.ensure((size_t)nr + 16);
    B.small.ensure(res_bytes + 64);
    B.small_pin.room(res_bytes);
    a.len = B.len.p;
    a.off = reinterpret_cast<const int64_t *>(B.small.p);
    a.flags = reinterpret_cast<uint32_t *>(B.small.p + o_flag);
    if (samp) *samp = reinterpret_cast<uint32_t *>(B.small.p + o_samp);
    a.hb = B.small.p + o_hb;
    a.out = nullptr;
    const unsigned grid = ((unsigned)nr + P.waves - 1) / P.waves;
    L.wait(q);
    UZ_HIP(hipMemsetAsync(B.small.p + o_flag, 0, 8, st));
    {
        ProfScope ps(c, P.k_size);
        hipLaunchKernelGGL(Size, dim3(grid), dim3(64 * P.waves), 0, st, a);
        UZ_HIP(hipGetLastError());
        uz_len_scan(c, st, nr, B.len.p, 0, reinterpret_cast<int64_t *>(B.small.p));
    }
    uz_kcopy(c, B.small_pin.p, B.small.p, res_bytes);
    L.turn(q, stage);
    const int64_t *off_h = reinterpret_cast<const int64_t *>(B.small_pin.p);
    const uint32_t *samp_h = reinterpret_cast<const uint32_t *>(B.small_pin.p + o_samp);
    const int64_t len = off_h[nr];
    UZ_REQUIRE(len >= 0 && len < ((int64_t)1 << 32), UZ_E_RANGE, std::string(P.what) + ": 4 GiB or more of text from one chunk");
    for (int32_t r = 0; r < nr; r++) {
        off[r + 1] = L.total + off_h[r + 1];
        if (samp) samp_at[r] = (uint64_t)(L.total + off_h[r]) + samp_h[r];
        handed_back[r] = B.small_pin.p[o_hb + (size_t)r];
    }
    if (!len) return;
    const size_t text = ((size_t)len + 15) & ~(size_t)15;
    B.out.ensure(text + 64);
    L.result_room(q, text, P.growth, full, part);
    a.out = B.out.p;
    {
        ProfScope ps(c, P.k_fill);
        hipLaunchKernelGGL(Fill, dim3(grid), dim3(64 * P.waves), 0, st, a);
        UZ_HIP(hipGetLastError());
    }
    L.fetch(B.out.p, (size_t)len);
    uz_kcopy(c, B.small_pin.p, a.flags, 8);
    UZ_HIP(hipStreamSynchronize(st));
    UZ_REQUIRE(!(*reinterpret_cast<const uint32_t *>(B.small_pin.p) & P.f_size), UZ_E_STATE, std::string(P.what) + ": a record's written bytes differ from its sized length");
    L.total += len;
}
