// k_deflate.hip -- BGZF blocks written on the device (unfazed_hip.h: uz_bgzf_deflate, uz_bgzf_deflate_coded).  deflate_body.hpp is the body: the
// parse rule, the fixed-Huffman coder, the stored fallback; deflate_dyn.hpp the second coder over the same parse, which picks the shortest of a
// dynamic, a fixed and a stored block per slice.  Here: the wavefront that runs them, the launches of a chunk and the host side of a call.
//
// The input is cut into slices of 65 280 bytes, one BGZF block each, and goes up in chunks of UZ_BGZF_CHUNK_BYTES (32 MiB, rounded down to whole
// slices: a slice's edges do not depend on the chunk size), chunk k + 1 copied on the copy stream while chunk k is worked on:
//   k_bgzf_deflate    one wavefront per slice: its raw DEFLATE stream into a scratch slot of UZ_DF_SLOT bytes, and the stream's byte count
//   k_bgzf_deflate_dyn  (UZ_DF_CODE_DYNAMIC: in k_bgzf_deflate's place) the same through deflate_dyn.hpp: two passes over the slice, its tokens
//                     parked between them in a buffer of the context, 65 280 words a slice: 131 MB for a 32 MiB chunk, 4.3 GB at the 1 GiB cap
//   k_bgzf_crc32_out  one wavefront per slice: the CRC-32 of its bytes (crc32_wave.hpp, the code k_bgzf_crc32 compares with)
//   uz_len_scan       exclusive scan of the blocks' sizes (18 + stream + 8) -> off [n + 1] (one workgroup)
//   k_bgzf_frame      one workgroup per block: header, stream, CRC-32 and ISIZE, back to back at off; a block whose written bytes differ from its
//                     scanned size raises the flag
// No global atomics decide a byte: the only one is the OR of the raised flag.
// uz_bgzf_deflate_indexed hangs the index kernels of k_tbx.hip into the same loop (TbxCall, uz_ctx.hpp): the blocks do not change.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "crc32_wave.hpp"
#include "deflate_dyn.hpp"
#include "text_out.hpp"

#define UZ_DF_F_SIZE 1u /* a framed block's written bytes differ from its scanned size */

namespace {

struct DfWave { // the 64 lanes of a wavefront share a slice
    template <typename T>
    struct V {
        T x;
        __device__ __forceinline__ T &operator[](uint32_t) { return x; }
        __device__ __forceinline__ const T &operator[](uint32_t) const { return x; }
    };
    __device__ __forceinline__ uint32_t lane0() const { return threadIdx.x & 63u; }
    __device__ __forceinline__ uint32_t lane1() const { return (threadIdx.x & 63u) + 1u; }
    __device__ __forceinline__ void sync() const { __syncthreads(); } // (the workgroup is this wavefront)
    __device__ __forceinline__ void drain() const { __builtin_amdgcn_s_waitcnt(0x0F70); } // vmcnt(0): the stores issued so far have landed
    __device__ __forceinline__ uint64_t ballot(const V<uint32_t> &p) const { return (uint64_t)__ballot(p.x != 0 ? 1 : 0); }
    __device__ __forceinline__ void excl_scan(const V<uint32_t> &v, V<uint32_t> &out, uint32_t &total) const {
        const uint32_t l = threadIdx.x & 63u;
        uint32_t x = v.x;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
            if (l >= d) x += y;
        }
        out.x = x - v.x;
        total = (uint32_t)__shfl((int)x, 63, 64);
    }
    __device__ __forceinline__ uint32_t get(const V<uint32_t> &v, uint32_t src) const { return (uint32_t)__shfl((int)v.x, (int)src, 64); }
    // an entry is raised until no lane holds a higher position for it: the maximum, whichever lane a colliding store lets win
    __device__ __forceinline__ void insert_max(uint16_t *tab, const V<uint32_t> &h, const V<uint32_t> &val, const V<uint32_t> &ok) const {
        for (;;) {
            const bool need = ok.x && (uint32_t)tab[h.x] < val.x;
            if (!__any(need ? 1 : 0)) break;
            if (need) tab[h.x] = (uint16_t)val.x;
            __syncthreads();
        }
    }
    __device__ __forceinline__ void or_word(uint32_t *w, uint32_t v) const { atomicOr(w, v); } // (LDS)
    __device__ __forceinline__ void add_word(uint32_t *w, uint32_t v) const { atomicAdd(w, v); } // (LDS)
};

__global__ __launch_bounds__(64) void k_bgzf_deflate(int32_t n_slices, const uint8_t *__restrict__ in, int64_t in_bytes, uint8_t *__restrict__ slots,
                                                     uint32_t *__restrict__ count /* [n_slices] */) {
    __shared__ UzDfLds S;
    const int32_t s = (int32_t)blockIdx.x;
    if (s >= n_slices) return;
    const int64_t at = (int64_t)s * UZ_DF_SLICE;
    const uint32_t n = in_bytes - at < (int64_t)UZ_DF_SLICE ? (uint32_t)(in_bytes - at) : UZ_DF_SLICE;
    DfWave w;
    bool stored = false;
    const uint32_t bytes = uz_deflate_slice(w, S, in + at, n, slots + (size_t)s * UZ_DF_SLOT, UZ_DF_SLOT, stored);
    if ((threadIdx.x & 63u) == 0) count[s] = bytes;
}

__global__ __launch_bounds__(64) void k_bgzf_deflate_dyn(int32_t n_slices, const uint8_t *__restrict__ in, int64_t in_bytes, uint8_t *__restrict__ slots,
                                                         uint32_t *tokens /* [n_slices * UZ_DY_TOKENS] */, uint32_t *__restrict__ count /* [n_slices] */) {
    __shared__ UzDyLds S;
    const int32_t s = (int32_t)blockIdx.x;
    if (s >= n_slices) return;
    const int64_t at = (int64_t)s * UZ_DF_SLICE;
    const uint32_t n = in_bytes - at < (int64_t)UZ_DF_SLICE ? (uint32_t)(in_bytes - at) : UZ_DF_SLICE;
    DfWave w;
    uint32_t kind = 0;
    const uint32_t bytes = uz_deflate_slice_dyn(w, S, in + at, n, slots + (size_t)s * UZ_DF_SLOT, UZ_DF_SLOT, tokens + (size_t)s * UZ_DY_TOKENS, UZ_DY_TOKENS, kind);
    if ((threadIdx.x & 63u) == 0) count[s] = bytes;
}

__global__ __launch_bounds__(64) void k_bgzf_crc32_out(int32_t n_slices, const uint8_t *__restrict__ in, int64_t in_bytes, uint32_t *__restrict__ crc) {
    __shared__ UzCrcLds S;
    const int lane = threadIdx.x;
    uz_crc_setup(S, lane);
    for (int32_t s = (int32_t)blockIdx.x; s < n_slices; s += (int32_t)gridDim.x) {
        const int64_t at = (int64_t)s * UZ_DF_SLICE;
        const uint32_t n = in_bytes - at < (int64_t)UZ_DF_SLICE ? (uint32_t)(in_bytes - at) : UZ_DF_SLICE;
        const uint32_t c = uz_crc_wave(S, in + at, n, lane);
        if (lane == 0) crc[s] = c;
    }
}

#define UZ_DF_FRAME_LANES 256
__global__ __launch_bounds__(UZ_DF_FRAME_LANES) void k_bgzf_frame(int32_t n_slices, int64_t in_bytes, const uint8_t *__restrict__ slots, const uint32_t *__restrict__ count,
                                                                   const uint32_t *__restrict__ crc, const int64_t *__restrict__ off, int64_t out_cap,
                                                                   uint8_t *__restrict__ out, uint32_t *flags) {
    const int32_t s = (int32_t)blockIdx.x;
    if (s >= n_slices) return;
    const uint32_t t = threadIdx.x, cnt = count[s];
    const int64_t o0 = off[s], o1 = off[s + 1];
    const int64_t left = in_bytes - (int64_t)s * UZ_DF_SLICE;
    const uint32_t isize = left < (int64_t)UZ_DF_SLICE ? (uint32_t)left : UZ_DF_SLICE;
    const uint32_t block = UZ_BGZF_HEAD + cnt + UZ_BGZF_TAIL; // what this launch writes
    // (a stream is at most 5 + 65 280 bytes: deflate_body.hpp; held here again, with the block's place in the output)
    if (cnt == 0 || cnt > 5 + isize || o1 - o0 != (int64_t)block || o0 < 0 || o1 > out_cap) {
        if (t == 0) atomicOr(flags, UZ_DF_F_SIZE);
        return;
    }
    uint8_t *d = out + o0;
    if (t < UZ_BGZF_HEAD) {
        const uint32_t bsize = block - 1;
        const uint8_t head[UZ_BGZF_HEAD] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xFF), (uint8_t)(bsize >> 8)};
        d[t] = head[t];
    } else if (t < UZ_BGZF_HEAD + UZ_BGZF_TAIL) {
        const uint32_t k = t - UZ_BGZF_HEAD, v = k < 4 ? crc[s] : isize;
        d[UZ_BGZF_HEAD + cnt + k] = (uint8_t)(v >> (8 * (k & 3u)));
    }
    // the stream: bytes up to the destination's first whole word, whole words built from the slot's bytes, the bytes behind the last one
    const uint8_t *src = slots + (size_t)s * UZ_DF_SLOT;
    uint8_t *dst = d + UZ_BGZF_HEAD;
    const uint32_t a4 = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u), a = a4 < cnt ? a4 : cnt;
    if (t < a) dst[t] = src[t];
    const uint32_t words = (cnt - a) / 4;
    for (uint32_t k = t; k < words; k += UZ_DF_FRAME_LANES) {
        const uint32_t i = a + 4 * k;
        const uint32_t v = (uint32_t)src[i] | ((uint32_t)src[i + 1] << 8) | ((uint32_t)src[i + 2] << 16) | ((uint32_t)src[i + 3] << 24);
        *reinterpret_cast<uint32_t *>(dst + i) = v;
    }
    const uint32_t rest = a + 4 * words;
    if (rest + t < cnt && t < 4) dst[rest + t] = src[rest + t];
}

struct Timer { // the two events of the measured form
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Timer() {
        for (hipEvent_t e : {e0, e1})
            if (e) (void)hipEventDestroy(e);
    }
};

} // namespace

int uz_bgzf_deflate_impl(uz_ctx *c, const uint8_t *data, int64_t n_bytes, int code, int64_t *kinds, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes,
                         int repeat, double *kernel_ms, TbxCall *tbx) {
    UZ_REQUIRE(n_blocks && bgzf && bgzf_bytes && n_bytes >= 0, UZ_E_ARG, "BGZF deflate: bad arguments");
    UZ_REQUIRE(code == UZ_DF_CODE_FIXED || code == UZ_DF_CODE_DYNAMIC, UZ_E_ARG, "BGZF deflate: bad code argument (UZ_DF_CODE_FIXED or UZ_DF_CODE_DYNAMIC)");
    const bool dyn = code == UZ_DF_CODE_DYNAMIC;
    if (kinds) kinds[0] = kinds[1] = kinds[2] = 0;
    UZ_REQUIRE(data || n_bytes == 0, UZ_E_ARG, "BGZF deflate: no data");
    *n_blocks = 0; *bgzf = nullptr; *bgzf_bytes = 0;
    if (kernel_ms) *kernel_ms = 0;
    if (n_bytes == 0) return 0; // nothing is launched: no blocks (the caller's end-of-file marker is the whole file)
    size_t chunk_bytes = (size_t)32 << 20;
    if (const char *e = getenv("UZ_BGZF_CHUNK_BYTES")) { // (read per call: the tests put chunk edges into small inputs with it)
        const long long v = atoll(e);
        if (v > 0) chunk_bytes = (size_t)v;
    }
    chunk_bytes = std::min<size_t>(chunk_bytes, (size_t)1 << 30);
    chunk_bytes = std::max<size_t>(UZ_DF_SLICE, chunk_bytes / UZ_DF_SLICE * UZ_DF_SLICE); // whole slices
    const size_t n_chunks = ((size_t)n_bytes + chunk_bytes - 1) / chunk_bytes;
    const int64_t total_slices = (n_bytes + UZ_DF_SLICE - 1) / UZ_DF_SLICE;
    if (tbx) { tbx->data = data; tbx->n_bytes = n_bytes; tbx->chunk_bytes = chunk_bytes; tbx->n_chunks = n_chunks; }
    Timer T; // (goes behind the loop, which drains the streams)
    ChunkLoop L(c, c->df, n_chunks);
    auto bytes_of = [&](size_t q) { return std::min<size_t>(chunk_bytes, (size_t)n_bytes - q * chunk_bytes); };
    auto stage = [&](size_t q) { // a chunk into its page-locked image, and the image onto the copy stream
        const size_t nb = bytes_of(q);
        memcpy(L.image(q, nb), data + q * chunk_bytes, nb);
        L.send(q, nb);
    };
    if (repeat > 0) { UZ_HIP(hipEventCreate(&T.e0)); UZ_HIP(hipEventCreate(&T.e1)); }
    hipStream_t st = c->stream;
    double ms_sum = 0;
    stage(0);
    for (size_t q = 0; q < n_chunks; q++) {
        const size_t nb = bytes_of(q);
        const int32_t ns = (int32_t)((nb + UZ_DF_SLICE - 1) / UZ_DF_SLICE);
        // a chunk's small results in one block: off [ns + 1], the flag word (+ padding), count [ns], crc [ns]
        const size_t o_flag = ((size_t)ns + 1) * 8, o_count = o_flag + 8, o_crc = o_count + (size_t)ns * 4, small_bytes = up256(o_crc + (size_t)ns * 4);
        const size_t out_cap = nb + (size_t)ns * (UZ_BGZF_HEAD + UZ_BGZF_TAIL + 5); // every slice stored
        c->df_slots.ensure((size_t)ns * UZ_DF_SLOT + 64);
        if (dyn) c->df_tokens.ensure((size_t)ns * UZ_DY_TOKENS);
        c->df.small.ensure(small_bytes + 64);
        c->df.out.ensure(up256(out_cap) + 64);
        c->df.small_pin.room(64);
        int64_t *d_off = reinterpret_cast<int64_t *>(c->df.small.p);
        uint32_t *d_flag = reinterpret_cast<uint32_t *>(c->df.small.p + o_flag);
        uint32_t *d_count = reinterpret_cast<uint32_t *>(c->df.small.p + o_count);
        uint32_t *d_crc = reinterpret_cast<uint32_t *>(c->df.small.p + o_crc);
        const uint8_t *d_in = c->df.in[q & 1].p;
        auto deflate = [&] { // the kernel of the chosen code
            if (dyn) hipLaunchKernelGGL(k_bgzf_deflate_dyn, dim3((unsigned)ns), dim3(64), 0, st, ns, d_in, (int64_t)nb, c->df_slots.p, c->df_tokens.p, d_count);
            else hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)ns), dim3(64), 0, st, ns, d_in, (int64_t)nb, c->df_slots.p, d_count);
        };
        L.wait(q);
        UZ_HIP(hipMemsetAsync(d_flag, 0, 8, st));
        {
            ProfScope ps(c, UZ_K_DEFLATE);
            deflate();
            UZ_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_bgzf_crc32_out, dim3((unsigned)std::min<int32_t>(ns, 256 * 16)), dim3(64), 0, st, ns, d_in, (int64_t)nb, d_crc);
            UZ_HIP(hipGetLastError());
            uz_len_scan(c, st, ns, d_count, UZ_BGZF_HEAD + UZ_BGZF_TAIL, d_off);
        }
        {
            ProfScope ps(c, UZ_K_DEFLATE_FRAME);
            hipLaunchKernelGGL(k_bgzf_frame, dim3((unsigned)ns), dim3(UZ_DF_FRAME_LANES), 0, st, ns, (int64_t)nb, (const uint8_t *)c->df_slots.p, (const uint32_t *)d_count,
                               (const uint32_t *)d_crc, (const int64_t *)d_off, (int64_t)out_cap, c->df.out.p, d_flag);
            UZ_HIP(hipGetLastError());
        }
        uz_kcopy(c, c->df.small_pin.p, d_off + ns, 16); // the chunk's bytes, the flag word
        if (tbx) uz_tbx_mark(c, *tbx, q, d_in, nb);
        if (repeat > 0) { // the measured form: the same launch again, which writes the same bytes into the same slots
            UZ_HIP(hipEventRecord(T.e0, st));
            for (int r = 0; r < repeat; r++) deflate();
            UZ_HIP(hipGetLastError());
            UZ_HIP(hipEventRecord(T.e1, st));
        }
        L.turn(q, stage);
        if (repeat > 0) {
            float ms = 0;
            UZ_HIP(hipEventElapsedTime(&ms, T.e0, T.e1));
            ms_sum += (double)ms / repeat;
        }
        const int64_t len = *reinterpret_cast<const int64_t *>(c->df.small_pin.p);
        const uint32_t flag = *reinterpret_cast<const uint32_t *>(c->df.small_pin.p + 8);
        UZ_REQUIRE(!(flag & UZ_DF_F_SIZE) && len >= (int64_t)ns * (UZ_BGZF_HEAD + UZ_BGZF_TAIL) && len <= (int64_t)out_cap, UZ_E_STATE,
                   "BGZF deflate: a framed block's written bytes differ from its scanned size");
        if (tbx) uz_tbx_keys(c, *tbx, q, d_in, nb, d_off, L.total);
        L.result_room(q, (size_t)len, 1.05, (double)n_bytes, (double)nb, 65536);
        L.fetch(c->df.out.p, (size_t)len);
        UZ_HIP(hipStreamSynchronize(st));
        L.total += len;
    }
    if (kinds) { // each block's form is its stream's BTYPE: 00 stored, 01 fixed, 10 dynamic
        const uint8_t *p = c->df.res.p;
        for (int64_t at = 0; at + (int64_t)UZ_BGZF_HEAD < L.total;) {
            const uint32_t btype = (p[at + UZ_BGZF_HEAD] >> 1) & 3u;
            UZ_REQUIRE(btype < 3, UZ_E_STATE, "BGZF deflate: a block of no known form");
            kinds[btype]++;
            at += ((int64_t)p[at + 16] | ((int64_t)p[at + 17] << 8)) + 1;
        }
    }
    if (tbx) uz_tbx_tables(c, *tbx, L.total);
    *n_blocks = total_slices;
    *bgzf_bytes = L.total;
    if (kernel_ms) *kernel_ms = ms_sum;
    *bgzf = c->df.res.p;
    return 0;
}
