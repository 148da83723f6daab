// k_bamhead.hip -- the head of a cohort's alignment files on the device: the template lengths of every file's first records, and the two order
// statistics a kid's insert cutoff is made of (read_collector.py:11-25; the float arithmetic stays on the host: hostpath.cutoff_from_ranks).
//
// What it replaces: open_source's loop over the first insert_size_max_sample + 1 records of a file (csrc/io_stage.cpp), one host thread inflating
// block after block per file, and numpy's partition of the column.  The heads of a group of files are inflated in HBM by k_bgzf_inflate, held
// against their CRC-32s by k_bgzf_crc32, and stay there.
//
//   k_head_walk   one wavefront per file, as k_bam_walk: the file's bytes go through LDS in 16 KiB windows, lane 0 follows the chain of
//                 block_size fields inside the window, then the 64 lanes take one record each and write its tlen into the file's column.  The
//                 rules (what a window may load, when a record is taken, the three states) are headwalk.hpp's.
//   k_head_rank   one workgroup per file: a radix select over |tlen - 2 readlen| -- four passes over the column with a 256-bin histogram in LDS,
//                 the key at rank k and the one at min(k + 1, n - 1).  No floating point.
//
// Parity: tests/test_head_gpu.py holds the columns against the writer's list and the host's own head (BamSource.tlen_head), the ranks against
// numpy.sort; tests/headwalk_main.cpp runs headwalk.hpp on the CPU under AddressSanitizer.
#include <hip/hip_runtime.h>

#include "headwalk.hpp"
#include "uz_ctx.hpp"

namespace {

struct HeadWalkArgs {
    const uint8_t *buf;     // the inflated blocks of the call's files, back to back
    const int64_t *base;    // [n_files + 1]: where every file's bytes start in buf
    const int32_t *ok;      // [n_files]: 1 walk it, 0 no block of it in this call, -1 a block of it failed its inflate or its CRC-32
    const int64_t *start;   // [n_files]: the first record's offset in the file's bytes
    const int64_t *want, *have, *first; // records wanted in all / taken by earlier calls; where the file's column starts in tlen
    int32_t *tlen;
    int64_t *taken, *cursor;
    int32_t *state;
};

__global__ __launch_bounds__(64) void k_head_walk(HeadWalkArgs a) {
    __shared__ uint4 win[UZ_HW_WIN / 16];
    __shared__ uint16_t offs[UZ_HW_WIN_RECS];
    __shared__ int s_n, s_state;
    __shared__ long long s_next;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int32_t ok = a.ok[f];
    if (ok != 1) {
        if (lane == 0) { a.taken[f] = 0; a.cursor[f] = a.start[f]; a.state[f] = ok < 0 ? UZ_HEAD_BAD : UZ_HEAD_NONE; }
        return;
    }
    const uint8_t *bytes = a.buf + a.base[f];
    const int64_t len = a.base[f + 1] - a.base[f], room = a.want[f] - a.have[f];
    int32_t *col = a.tlen + a.first[f] + a.have[f];
    const uint8_t *win8 = reinterpret_cast<const uint8_t *>(win);
    int64_t cur = a.start[f], taken = 0;
    int state = UZ_HEAD_NONE;
    while (state == UZ_HEAD_NONE) {
        const int64_t w0 = cur - (int64_t)((uintptr_t)(bytes + cur) & 15u); // (16-byte loads want a 16-byte boundary of the memory, not of the file)
#pragma unroll 4
        for (int it = 0; it < UZ_HW_WIN / 16 / 64; it++) {
            const int idx = it * 64 + lane;
            const int64_t p = w0 + 16 * (int64_t)idx;
            uint4 v;
            if (uz_hw_piece_inside(p, len)) v = *reinterpret_cast<const uint4 *>(bytes + p);
            else {
                uint8_t t[16];
                uz_hw_piece_edge(bytes, len, p, t);
                v = make_uint4(uz_hw_ld32(t), uz_hw_ld32(t + 4), uz_hw_ld32(t + 8), uz_hw_ld32(t + 12));
            }
            win[idx] = v;
        }
        __syncthreads();
        if (lane == 0) {
            int st;
            int64_t nx;
            s_n = uz_hw_chain(win8, w0, cur, len, room - taken, offs, &st, &nx);
            s_state = st; s_next = nx;
        }
        __syncthreads();
        const int n = s_n;
        for (int j = lane; j < n; j += 64) col[taken + j] = uz_hw_tlen(win8, offs[j], bytes, w0);
        taken += n; cur = s_next; state = s_state;
        __syncthreads(); // the window is read to the end before the next one lands
    }
    if (lane == 0) { a.taken[f] = taken; a.cursor[f] = cur; a.state[f] = state; }
}

__global__ __launch_bounds__(256) void k_head_rank(const int32_t *__restrict__ tlen, const int64_t *__restrict__ first, const int64_t *__restrict__ n_of,
                                                   const int64_t *__restrict__ k_of, int32_t readlen, uint32_t *__restrict__ out_a, uint32_t *__restrict__ out_b) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_above;
    __shared__ unsigned long long s_rank;
    const int f = blockIdx.x, t = threadIdx.x;
    const int64_t n = n_of[f];
    if (n <= 0 || k_of[f] < 0 || k_of[f] >= n) { // (the host asks for no such rank: abi.hip uz_head_rank)
        if (t == 0) { out_a[f] = 0; out_b[f] = 0; }
        return;
    }
    const int32_t *col = tlen + first[f];
    if (t == 0) { s_prefix = 0; s_rank = (unsigned long long)k_of[f]; s_above = 0xFFFFFFFFu; }
    for (int pass = 0; pass < 4; pass++) {
        hist[t] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        uint32_t above = 0xFFFFFFFFu;
        for (int64_t i = t; i < n; i += 256) {
            const uint32_t key = uz_hw_key(col[i], readlen);
            if (uz_hw_sel_in(key, pass, prefix)) atomicAdd(&hist[uz_hw_sel_digit(key, pass)], 1u);
            else if (pass == 3 && (key >> 8) > prefix) above = min(above, key);
        }
        if (pass == 3 && above != 0xFFFFFFFFu) atomicMin(&s_above, above);
        __syncthreads();
        if (t == 0) {
            uint64_t r = s_rank;
            if (pass < 3) {
                const uint32_t b = uz_hw_sel_bin(hist, &r);
                s_prefix = (prefix << 8) | b; s_rank = r;
            } else {
                uint32_t ka, kb;
                uz_hw_sel_last(hist, r, prefix, k_of[f] + 1 <= n - 1, s_above, &ka, &kb);
                out_a[f] = ka; out_b[f] = kb;
            }
        }
        __syncthreads();
    }
}

} // namespace

// every pointer device memory (abi.hip: uz_head_walk checks the tables before they go up)
void uz_launch_head_walk(uz_ctx *c, hipStream_t st, int32_t n_files, const uint8_t *buf, const int64_t *base, const int32_t *ok, const int64_t *start,
                         const int64_t *want, const int64_t *have, const int64_t *first, int32_t *tlen, int64_t *taken, int64_t *cursor, int32_t *state) {
    if (n_files <= 0) return;
    HeadWalkArgs a{buf, base, ok, start, want, have, first, tlen, taken, cursor, state};
    hipLaunchKernelGGL(k_head_walk, dim3((unsigned)n_files), dim3(64), 0, st, a);
    UZ_HIP(hipGetLastError());
}
void uz_launch_head_rank(uz_ctx *c, hipStream_t st, int32_t n_files, const int32_t *tlen, const int64_t *first, const int64_t *n_of, const int64_t *k_of,
                         int32_t readlen, uint32_t *out_a, uint32_t *out_b) {
    if (n_files <= 0) return;
    hipLaunchKernelGGL(k_head_rank, dim3((unsigned)n_files), dim3(256), 0, st, tlen, first, n_of, k_of, readlen, out_a, out_b);
    UZ_HIP(hipGetLastError());
}
