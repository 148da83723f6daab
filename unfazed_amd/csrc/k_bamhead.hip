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

#include <algorithm>
#include <optional>

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

// ---- the entry points (abi.hip holds their guarded wrappers): the tables are checked here, before they go up -- the kernels check nothing
static uz_ctx::HeadDev &head_of(uz_ctx *c, int id) {
    UZ_REQUIRE(id >= 0 && id < (int)c->heads.size() && c->heads[(size_t)id].live, UZ_E_ARG, "unknown head id");
    return c->heads[(size_t)id];
}

void uz_head_walk_impl(uz_ctx *c, int *head_id, int32_t n_files, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off,
                      const int32_t *isize, const uint32_t *crc, const int64_t *blk_first, const int64_t *start, const int64_t *want, const int64_t *have,
                      int64_t *taken, int64_t *cursor, int32_t *state) {
    UZ_REQUIRE(head_id && n_files >= 1 && n_files < (1 << 24) && n_blocks >= 0 && n_blocks < ((int64_t)1 << 31) && comp_bytes >= 0 && blk_first && start && want && have &&
                   taken && cursor && state && (n_blocks == 0 || (comp && in_off && isize && crc)),
               UZ_E_ARG, "bad arguments");
    const size_t nf = (size_t)n_files, nb = (size_t)n_blocks;
    UZ_REQUIRE(blk_first[0] == 0 && blk_first[nf] == n_blocks, UZ_E_ARG, "bad block table (blk_first)");
    for (size_t f = 0; f < nf; f++) UZ_REQUIRE(blk_first[f] <= blk_first[f + 1], UZ_E_ARG, "bad block table (blk_first)");
    std::vector<int64_t> out_off(nb + 1, 0);
    for (size_t k = 0; k < nb; k++) out_off[k + 1] = out_off[k] + isize[k];
    UZ_REQUIRE(!uz_bgzf_check_tables(n_blocks, comp_bytes, in_off, out_off.data(), false), UZ_E_ARG, "bad block table (a BGZF block inflates to at most 64 KiB)");
    // the head: a new one is entered only when the whole call has gone through
    const bool fresh = *head_id < 0;
    uz_ctx::HeadDev made;
    uz_ctx::HeadDev *H = fresh ? &made : &head_of(c, *head_id);
    if (fresh) {
        made.n_files = n_files; made.want.assign(want, want + nf); made.have.assign(nf, 0); made.first.assign(nf + 1, 0);
        for (size_t f = 0; f < nf; f++) {
            UZ_REQUIRE(want[f] >= 0 && want[f] <= INT32_MAX, UZ_E_ARG, "bad record count wanted");
            made.first[f + 1] = made.first[f] + want[f];
        }
    } else {
        UZ_REQUIRE(H->n_files == n_files, UZ_E_ARG, "the head holds another number of files");
        for (size_t f = 0; f < nf; f++) UZ_REQUIRE(H->want[f] == want[f], UZ_E_ARG, "the head was opened with other record counts");
    }
    std::vector<int32_t> ok(nf, 0);
    for (size_t f = 0; f < nf; f++) {
        UZ_REQUIRE(have[f] == H->have[f], UZ_E_ARG, "have[] is not what the head's walks have taken so far");
        const int64_t len = out_off[(size_t)blk_first[f + 1]] - out_off[(size_t)blk_first[f]];
        ok[f] = blk_first[f + 1] > blk_first[f] ? 1 : 0;
        UZ_REQUIRE(!ok[f] || (start[f] >= 0 && start[f] <= len), UZ_E_ARG, "a file's start offset lies outside its bytes");
    }
    try {
        if (fresh) {
            made.tlen.ensure((size_t)made.first[nf] + 1);
            made.first_d.ensure(nf + 1);
            UZ_HIP(hipMemcpyAsync(made.first_d.p, made.first.data(), (nf + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
        // one table of 64-bit columns, one of 32-bit ones
        enum { I_IN = 0 };
        const size_t o_out = nb, o_base = o_out + nb + 1, o_start = o_base + nf + 1, o_want = o_start + nf, o_have = o_want + nf, o_taken = o_have + nf,
                     o_cursor = o_taken + nf, n64 = o_cursor + nf;
        std::vector<int64_t> t64(n64, 0);
        for (size_t k = 0; k < nb; k++) t64[I_IN + k] = in_off[k];
        std::copy(out_off.begin(), out_off.end(), t64.begin() + (ptrdiff_t)o_out);
        for (size_t f = 0; f <= nf; f++) t64[o_base + f] = out_off[(size_t)blk_first[f]];
        for (size_t f = 0; f < nf; f++) { t64[o_start + f] = ok[f] ? start[f] : 0; t64[o_want + f] = want[f]; t64[o_have + f] = have[f]; }
        const size_t o_ok = 0, o_state = nf, o_flags = 2 * nf, n32 = o_flags + 4 * (nf + 1); // flags: [cursor, err, crc err, -] for the group, then per file
        c->hd_comp.ensure((size_t)uz_bgzf_room(comp_bytes)); c->hd_out.ensure((size_t)out_off[nb] + 64);
        c->hd_i64.ensure(n64); c->hd_i32.ensure(n32); c->hd_u32.ensure(nb + 1);
        hipStream_t st = c->stream;
        int64_t *d64 = c->hd_i64.p;
        int32_t *d32 = c->hd_i32.p;
        UZ_HIP(hipMemcpyAsync(d64, t64.data(), n64 * 8, hipMemcpyHostToDevice, st));
        std::vector<int32_t> flags(4 * (nf + 1), 0);
        if (nb) {
            UZ_HIP(hipMemcpyAsync(c->hd_u32.p, crc, nb * 4, hipMemcpyHostToDevice, st));
            auto check = [&](size_t b0, size_t b1, size_t slot) {
                uz_launch_crc32(c, st, (int64_t)(b1 - b0), c->hd_out.p, d64 + o_out + b0, c->hd_u32.p + b0, d32 + o_flags + 4 * slot + 2);
            };
            // the group's blocks in one launch however many (the tables went up with t64), and their CRC-32s behind it
            InflateBatch b{comp, comp_bytes, n_blocks, in_off, out_off.data(), c->hd_comp.p, d64 + I_IN, d64 + o_out, c->hd_out.p, d32 + o_flags, {st, nullptr}, nullptr};
            b.tables_there = true;
            std::optional<ProfScope> ps; // (its span: the two kernels, not the bytes' way up)
            b.before = [&](size_t, hipStream_t) { ps.emplace(c, UZ_K_HEAD_INFLATE); };
            b.after = [&](size_t, hipStream_t) { check(0, nb, 0); ps.reset(); };
            uz_queue_inflate(c, b, {0, n_blocks});
            UZ_HIP(hipMemcpyAsync(flags.data(), d32 + o_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            UZ_HIP(hipStreamSynchronize(st));
            if (flags[1] || flags[2]) { // some block is bad: file by file, to know whose -- the FILE is marked, the call goes on
                for (size_t f = 0; f < nf; f++)
                    if (ok[f]) {
                        const size_t b0 = (size_t)blk_first[f], b1 = (size_t)blk_first[f + 1];
                        uz_launch_inflate(c, st, (int64_t)(b1 - b0), c->hd_comp.p, uz_bgzf_padded(comp_bytes), d64 + I_IN + b0, d64 + o_out + b0, c->hd_out.p, d32 + o_flags + 4 * (f + 1));
                        check(b0, b1, f + 1);
                    }
                UZ_HIP(hipMemcpyAsync(flags.data(), d32 + o_flags, flags.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                UZ_HIP(hipStreamSynchronize(st));
                for (size_t f = 0; f < nf; f++)
                    if (ok[f] && (flags[4 * (f + 1) + 1] || flags[4 * (f + 1) + 2])) ok[f] = -1;
            }
        }
        UZ_HIP(hipMemcpyAsync(d32 + o_ok, ok.data(), nf * 4, hipMemcpyHostToDevice, st));
        {
            ProfScope ps(c, UZ_K_HEAD_WALK);
            const HeadWalkArgs a{c->hd_out.p, d64 + o_base, d32 + o_ok, d64 + o_start, d64 + o_want, d64 + o_have, fresh ? made.first_d.p : H->first_d.p,
                                 fresh ? made.tlen.p : H->tlen.p, d64 + o_taken, d64 + o_cursor, d32 + o_state};
            hipLaunchKernelGGL(k_head_walk, dim3((unsigned)n_files), dim3(64), 0, st, a);
            UZ_HIP(hipGetLastError());
        }
        UZ_HIP(hipMemcpyAsync(taken, d64 + o_taken, nf * 8, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipMemcpyAsync(cursor, d64 + o_cursor, nf * 8, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipMemcpyAsync(state, d32 + o_state, nf * 4, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipStreamSynchronize(c->stream);
        if (fresh) { made.tlen.release(); made.first_d.release(); }
        throw;
    }
    for (size_t f = 0; f < nf; f++) {
        UZ_REQUIRE(taken[f] >= 0 && H->have[f] + taken[f] <= H->want[f], UZ_E_STATE, "the head walk took more records than wanted");
        H->have[f] += taken[f];
    }
    if (fresh) {
        made.live = true;
        const int k = new_slot(c->heads);
        c->heads[(size_t)k] = made;
        *head_id = k;
    }
}

void uz_head_rank_impl(uz_ctx *c, int head_id, int32_t readlen, const int64_t *k, uint32_t *a, uint32_t *b) {
    uz_ctx::HeadDev &H = head_of(c, head_id);
    UZ_REQUIRE(k && a && b && readlen >= 0 && readlen < (1 << 30), UZ_E_ARG, "bad arguments (0 <= readlen < 2^30)");
    const size_t nf = (size_t)H.n_files;
    std::vector<int64_t> t64(2 * nf);
    for (size_t f = 0; f < nf; f++) {
        UZ_REQUIRE(k[f] < H.have[f] || k[f] < 0, UZ_E_ARG, "a rank beyond the records the file's column holds");
        t64[f] = k[f] < 0 ? 0 : H.have[f]; // (a skipped file: no records as far as the kernel is concerned)
        t64[nf + f] = k[f];
    }
    c->hd_i64.ensure(2 * nf); c->hd_u32.ensure(2 * nf);
    hipStream_t st = c->stream;
    UZ_HIP(hipMemcpyAsync(c->hd_i64.p, t64.data(), 2 * nf * 8, hipMemcpyHostToDevice, st));
    {
        ProfScope ps(c, UZ_K_HEAD_RANK);
        hipLaunchKernelGGL(k_head_rank, dim3((unsigned)nf), dim3(256), 0, st, H.tlen.p, H.first_d.p, c->hd_i64.p, c->hd_i64.p + nf, readlen, c->hd_u32.p, c->hd_u32.p + nf);
        UZ_HIP(hipGetLastError());
    }
    UZ_HIP(hipMemcpyAsync(a, c->hd_u32.p, nf * 4, hipMemcpyDeviceToHost, st));
    UZ_HIP(hipMemcpyAsync(b, c->hd_u32.p + nf, nf * 4, hipMemcpyDeviceToHost, st));
    UZ_HIP(hipStreamSynchronize(st));
}

void uz_head_fetch_impl(uz_ctx *c, int head_id, int32_t file, int32_t *out, int64_t cap, int64_t *n) {
    uz_ctx::HeadDev &H = head_of(c, head_id);
    UZ_REQUIRE(file >= 0 && file < H.n_files && n && cap >= 0 && (cap == 0 || out), UZ_E_ARG, "bad arguments");
    *n = std::min<int64_t>(cap, H.have[(size_t)file]);
    if (*n) UZ_HIP(hipMemcpyAsync(out, H.tlen.p + H.first[(size_t)file], (size_t)*n * 4, hipMemcpyDeviceToHost, c->stream));
    UZ_HIP(hipStreamSynchronize(c->stream));
}

void uz_head_free_impl(uz_ctx *c, int head_id) {
    uz_ctx::HeadDev &H = head_of(c, head_id);
    UZ_HIP(hipStreamSynchronize(c->stream));
    H.tlen.release(); H.first_d.release();
    H = uz_ctx::HeadDev();
}
