// k_tbx.hip -- the tables of a tabix index, built beside the BGZF blocks of uz_bgzf_deflate_indexed from the chunk images the deflate kernels
// read (k_deflate.hip hangs the three calls below into its chunk loop).  tbx_key.hpp is the body: the rules that turn a line into its key.
//
// Per chunk of text (nb bytes in HBM; a TILE is 1 KiB of it):
//   k_tbx_mark    one wavefront per tile: 64 lanes x one 16-byte load, a compare against '\n', a popcount -> the tile's count of line starts.  A
//                 line starts behind every '\n' that is not the chunk's last byte, and at byte 0 when the host says so (it has the byte before)
//   uz_len_scan   the tiles' counts -> each tile's row base, and the chunk's row count (sent down with the chunk's other small results)
//   k_tbx_starts  the same loads again: every line's start, at its row                             (behind the chunk's host wait, which the
//   k_tbx_keys    one wavefront per line: the body, 64 bytes a step; the row appended to the row     deflate loop has anyway: the row count
//                 table: kind, beg, end, v0 = (base + d_off[t / 65280]) << 16 | t % 65280, the       sizes the table and the grid)
//                 name's place in the whole text, and same_as_prev: the name compared byte for byte, with its length, against the line before
//   The chunk's first line (the line before it is not in the chunk) and a last line whose key columns the chunk's end cut are settled by
//   uz_tbx_settle on the host, which has the whole text: the same body as a plain loop, at most two rows a chunk, patched in by k_tbx_patch.
// Once, behind the last chunk, over all N rows (the table stays in HBM across the chunks):
//   k_tbx_flags   per row: does it open a reference (a data row whose name differs from the row before, or that follows a meta line), does it
//                 open a run (a reference, or another bin than the row before); the status word: a bad row, a meta row behind data, a start
//                 below the one before on the same reference, a begin or end beyond 2^29
//   uz_len_scan   x 2: the two flags -> every row's tid and run
//   k_tbx_emit    per row: a run's (tid, bin, v0) from its first row and v1 from its last (v1 of a row = v0 of the next row, of the last row
//                 the end-of-file marker's place << 16); a reference's name, first v0, last v1 and row span; atomicMax of end per reference
//   k_tbx_nintv   per reference: n_intv = ((max end - 1) >> 14) + 1, the row count; uz_len_scan -> the linear table's offsets
//   k_tbx_linear  per row: 64-bit atomicMin of v0 over the windows beg >> 14 .. (end - 1) >> 14 (empty: all ones)
//   k_tbx_fill    one workgroup per reference: empty windows take the next window's value, going backwards (a suffix minimum: in a sorted file
//                 a window's first record never lies before an earlier window's)
// What comes down: the references, the runs in file order, the linear table, the status word.  Grouping the runs by (tid, bin) is a stable
// sort of a table the index's own size and is the caller's (engine.py: numpy.lexsort).  Global atomics: the OR of the status word, the max of
// end, the min of v0; every other store is one row's or one table entry's own.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "deflate_body.hpp"
#include "tbx_key.hpp"
#include "text_out.hpp"

#define UZ_TBX_TILE 1024u
#define UZ_TBX_WAVES 4u /* wavefronts of a workgroup */

namespace {

struct TbxDevWave { // the 64 bytes of a step are the wavefront's lanes
    __device__ __forceinline__ void step(const uint8_t *p, uint64_t pos, uint64_t lim, uint64_t &tabs, uint64_t &nls, uint64_t &crs, uint64_t &semis) const {
        const uint64_t i = pos + (threadIdx.x & 63u);
        const uint32_t ch = i < lim ? p[i] : 0u;
        tabs = (uint64_t)__ballot(ch == '\t' ? 1 : 0);
        nls = (uint64_t)__ballot(ch == '\n' ? 1 : 0);
        crs = (uint64_t)__ballot(ch == '\r' ? 1 : 0);
        semis = (uint64_t)__ballot(ch == ';' ? 1 : 0);
    }
};

// 0x80 in every byte of w that is '\n' (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t nl_bytes(uint32_t w) {
    const uint32_t y = w ^ 0x0A0A0A0Au;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}

// A lane's 16 bytes of tile `tile`: bit 8 k + 7 of m[k / 4 ...] -- one mask word per 4 bytes -- for every '\n' at a chunk offset j with j + 1 < nb
// (a line starts behind it, inside the chunk).  -> the lane's first byte's offset.  The load is whole and aligned (the image is a device
// allocation with 64 bytes of slack behind nb; a lane whose 16 bytes begin at or behind nb loads nothing)
__device__ __forceinline__ uint32_t lane_marks(const uint8_t *__restrict__ in, uint32_t nb, uint32_t tile, uint32_t m[4]) {
    const uint32_t at = tile * UZ_TBX_TILE + (threadIdx.x & 63u) * 16u;
    m[0] = m[1] = m[2] = m[3] = 0;
    if (at + 1 < nb) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t ok = nb - 1 - at; // bytes of the lane that may open a line behind them
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t have = ok > 4 * k ? ok - 4 * k : 0; // ... of this word
            const uint32_t keep = have >= 4 ? 0xFFFFFFFFu : have ? (1u << (8 * have)) - 1u : 0u;
            m[k] = nl_bytes(w[k]) & keep;
        }
    }
    return at;
}

__global__ __launch_bounds__(64 * UZ_TBX_WAVES) void k_tbx_mark(const uint8_t *__restrict__ in, uint32_t nb, uint32_t n_tiles, int carry, uint32_t *__restrict__ cnt) {
    const uint32_t tile = blockIdx.x * UZ_TBX_WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    uint32_t m[4];
    (void)lane_marks(in, nb, tile, m);
    RowWave w;
    uint32_t total = 0;
    (void)w.excl_scan((uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3])), total);
    if (w.lane() == 0) cnt[tile] = total + (tile == 0 && carry ? 1u : 0u);
}

__global__ __launch_bounds__(64 * UZ_TBX_WAVES) void k_tbx_starts(const uint8_t *__restrict__ in, uint32_t nb, uint32_t n_tiles, int carry, const int64_t *__restrict__ toff,
                                                                  int64_t nr, uint32_t *__restrict__ starts) {
    const uint32_t tile = blockIdx.x * UZ_TBX_WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    uint32_t m[4];
    const uint32_t at = lane_marks(in, nb, tile, m);
    RowWave w;
    uint32_t total = 0;
    const uint32_t before = w.excl_scan((uint32_t)(__popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3])), total);
    const bool first = tile == 0 && carry;
    int64_t r = toff[tile] + (first ? 1 : 0) + before;
    if (first && w.lane() == 0 && nr > 0) starts[0] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t bits = m[k]; bits; bits &= bits - 1, r++)
            if (r >= 0 && r < nr) starts[r] = at + 4 * k + ((uint32_t)__builtin_ctz(bits) >> 3) + 1; // (held against the table's size by itself)
}

__global__ __launch_bounds__(64 * UZ_TBX_WAVES) void k_tbx_keys(const uint8_t *__restrict__ in, uint32_t nb, int text_end, int preset, const uint32_t *__restrict__ starts,
                                                                int64_t nr, const int64_t *__restrict__ d_off, int32_t ns, int64_t base, uint64_t text_at,
                                                                TbxRow *__restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * UZ_TBX_WAVES + (threadIdx.x >> 6);
    if (r >= nr) return;
    const uint32_t s = starts[r], lane = threadIdx.x & 63u;
    TbxRow row;
    row.v0 = row.name_off = 0; row.beg = row.end = 0; row.name_len = 0; row.kind = UZ_TBX_CUT; // (a start outside the chunk: nobody settles it, the status word says so)
    if (s < nb && s / UZ_DF_SLICE < (uint32_t)ns) {
        TbxDevWave w;
        UzTbxKey k;
        uz_tbx_key(w, in, (uint64_t)s, (uint64_t)nb, text_end != 0, preset, k);
        uint32_t same = 0;
        if (r > 0 && k.kind != UZ_TBX_CUT) { // the line before: [ps, s - 1), its '\n' at s - 1
            const uint32_t ps = starts[r - 1], len = k.name_len;
            if (ps < s && len <= s - 1 - ps) {
                const uint32_t term = in[ps + len];
                uint32_t differ = 0;
                for (uint32_t i = lane; i < len; i += 64) differ |= in[ps + i] != in[s + i] ? 1u : 0u;
                same = (term == '\t' || term == '\n') && !__any((int)differ) ? 1u : 0u;
            }
        }
        row.v0 = (uint64_t)(base + d_off[s / UZ_DF_SLICE]) << 16 | (uint64_t)(s % UZ_DF_SLICE);
        row.name_off = text_at + s;
        row.beg = k.beg; row.end = k.end; row.name_len = k.name_len;
        row.kind = k.kind | k.why << 4 | same << 8;
    }
    if (lane == 0) rows[r] = row;
}

// the rows the host settled: kind, key and name length are the host's, v0 and the name's place stay the device's
__global__ __launch_bounds__(64) void k_tbx_patch(int32_t n, const int64_t *__restrict__ at, const TbxRow *__restrict__ from, int64_t n_rows, TbxRow *__restrict__ rows) {
    const int32_t i = (int32_t)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n || at[i] < 0 || at[i] >= n_rows) return;
    TbxRow row = rows[at[i]];
    row.beg = from[i].beg; row.end = from[i].end; row.name_len = from[i].name_len; row.kind = from[i].kind;
    rows[at[i]] = row;
}

__device__ __forceinline__ bool is_data(const TbxRow &r) { return (r.kind & 3u) == UZ_TBX_DATA; }

__global__ __launch_bounds__(256) void k_tbx_flags(int64_t n, const TbxRow *__restrict__ rows, uint32_t *__restrict__ is_new, uint32_t *__restrict__ is_run, uint32_t *status) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const TbxRow row = rows[r];
    const uint32_t kind = row.kind & 3u, why = row.kind >> 4 & 15u;
    const bool prev_data = r > 0 && is_data(rows[r - 1]);
    uint32_t st = 0, nw = 0, rn = 0;
    if (kind == UZ_TBX_BAD) st |= why == UZ_TBX_WHY_EMPTY ? UZ_TBX_S_EMPTY : why == UZ_TBX_WHY_CR ? UZ_TBX_S_CR : UZ_TBX_S_POS;
    if (kind == UZ_TBX_CUT) st |= UZ_TBX_S_CUT;
    if (kind == UZ_TBX_META && prev_data) st |= UZ_TBX_S_META;
    if (kind == UZ_TBX_DATA) {
        if (row.beg >= UZ_TBX_MAX_END || row.end > UZ_TBX_MAX_END) st |= UZ_TBX_S_RANGE;
        const bool same = prev_data && (row.kind >> 8 & 1u);
        nw = same ? 0u : 1u;
        rn = nw;
        if (same) {
            const TbxRow prev = rows[r - 1];
            if (row.beg < prev.beg) st |= UZ_TBX_S_ORDER;
            if (uz_tbx_reg2bin(row.beg, row.end) != uz_tbx_reg2bin(prev.beg, prev.end)) rn = 1;
        }
    }
    is_new[r] = nw;
    is_run[r] = rn;
    if (st) atomicOr(status, st);
}

struct TbxTables { // the device side of what comes down, and the work arrays of the passes (all of n_refs entries but runs)
    uz_tbx_ref *refs;
    uz_tbx_run *runs;
    uint32_t *max_end, *n_intv;
    int64_t *first, *last, *lin_off; // lin_off [n_refs + 1]
};

__global__ __launch_bounds__(256) void k_tbx_emit(int64_t n, const TbxRow *__restrict__ rows, const uint32_t *__restrict__ is_new, const int64_t *__restrict__ new_off,
                                                  const uint32_t *__restrict__ is_run, const int64_t *__restrict__ run_off, uint64_t eof_v, int64_t n_refs, int64_t n_runs,
                                                  TbxTables T) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const TbxRow row = rows[r];
    if (!is_data(row)) return;
    const int64_t tid = new_off[r] + is_new[r] - 1, run = run_off[r] + is_run[r] - 1;
    if (tid < 0 || tid >= n_refs || run < 0 || run >= n_runs) return;
    const uint64_t v1 = r + 1 < n ? rows[r + 1].v0 : eof_v;
    if (is_run[r]) { T.runs[run].tid = (uint32_t)tid; T.runs[run].bin = uz_tbx_reg2bin(row.beg, row.end); T.runs[run].v0 = row.v0; }
    if (r + 1 == n || is_run[r + 1]) T.runs[run].v1 = v1;
    if (is_new[r]) { T.refs[tid].name_off = row.name_off; T.refs[tid].name_len = row.name_len; T.refs[tid].v0 = row.v0; T.first[tid] = r; }
    if (r + 1 == n || is_new[r + 1]) { T.refs[tid].v1 = v1; T.last[tid] = r; }
    atomicMax(&T.max_end[tid], (uint32_t)row.end); // (1 <= end <= 2^29: k_tbx_flags)
}

__global__ __launch_bounds__(256) void k_tbx_nintv(int64_t n_refs, TbxTables T) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_refs) return;
    const uint32_t e = T.max_end[t], n_intv = e ? ((e - 1) >> 14) + 1 : 0;
    T.n_intv[t] = n_intv;
    T.refs[t].n_intv = n_intv;
    T.refs[t].n_rows = (uint64_t)(T.last[t] - T.first[t] + 1);
}

__global__ __launch_bounds__(256) void k_tbx_linear(int64_t n, const TbxRow *__restrict__ rows, const uint32_t *__restrict__ is_new, const int64_t *__restrict__ new_off,
                                                    int64_t n_refs, TbxTables T, unsigned long long *linear) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const TbxRow row = rows[r];
    if (!is_data(row)) return;
    const int64_t tid = new_off[r] + is_new[r] - 1;
    if (tid < 0 || tid >= n_refs) return;
    const int64_t lo = T.lin_off[tid], cnt = T.lin_off[tid + 1] - lo;
    for (int64_t w = row.beg >> 14; w <= (row.end - 1) >> 14 && w < cnt; w++) atomicMin(&linear[lo + w], (unsigned long long)row.v0);
}

__global__ __launch_bounds__(256) void k_tbx_fill(TbxTables T, unsigned long long *linear) {
    __shared__ unsigned long long sm[256];
    __shared__ unsigned long long carry_s;
    const uint32_t t = threadIdx.x;
    const int64_t lo = T.lin_off[blockIdx.x], n = T.lin_off[blockIdx.x + 1] - lo;
    if (t == 0) carry_s = ~0ull;
    __syncthreads();
    for (int64_t hi = n; hi > 0; hi -= 256) { // tiles of 256 windows, the last one first
        const int64_t base = hi > 256 ? hi - 256 : 0, cnt = hi - base;
        unsigned long long v = (int64_t)t < cnt ? linear[lo + base + t] : ~0ull;
        for (uint32_t d = 1; d < 256; d <<= 1) { // the minimum of this window and those behind it in the tile
            sm[t] = v;
            __syncthreads();
            if (t + d < 256 && sm[t + d] < v) v = sm[t + d];
            __syncthreads();
        }
        if (carry_s < v) v = carry_s;
        if ((int64_t)t < cnt) linear[lo + base + t] = v;
        __syncthreads();
        if (t == 0) carry_s = v;
        __syncthreads();
    }
}

// a line of the whole text settled on the host: the body as a plain loop, and the name held against the line before
TbxRow uz_tbx_settle(const TbxCall &t, uint64_t at) {
    UzTbxHostWave w;
    UzTbxKey k;
    uz_tbx_key(w, t.data, at, (uint64_t)t.n_bytes, true, t.preset, k);
    uint32_t same = 0;
    if (at > 0) {
        const uint8_t *nl = at > 1 ? (const uint8_t *)memrchr(t.data, '\n', at - 1) : nullptr;
        const uint64_t ps = nl ? (uint64_t)(nl - t.data) + 1 : 0, len = k.name_len;
        if (len <= at - 1 - ps && (t.data[ps + len] == '\t' || t.data[ps + len] == '\n') && memcmp(t.data + ps, t.data + at, len) == 0) same = 1;
    }
    TbxRow row;
    row.v0 = row.name_off = 0;
    row.beg = k.beg; row.end = k.end; row.name_len = k.name_len;
    row.kind = k.kind | k.why << 4 | same << 8;
    return row;
}

bool chunk_carry(const TbxCall &t, size_t q) { return q == 0 || t.data[q * t.chunk_bytes - 1] == '\n'; } // does the chunk's byte 0 open a line

// device memory grown with what it holds (the row table, across a call's chunks)
void grow_keep(uz_ctx *c, DevBuf<uint8_t> &b, size_t need, size_t used) {
    if (need <= b.cap) return;
    DevBuf<uint8_t> bigger;
    bigger.ensure(need + need / 2);
    if (used) UZ_HIP(hipMemcpyAsync(bigger.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
    UZ_HIP(hipStreamSynchronize(c->stream));
    b.release();
    b = bigger;
}

} // namespace

void uz_tbx_mark(uz_ctx *c, TbxCall &t, size_t q, const uint8_t *d_in, size_t nb) {
    const uint32_t n_tiles = (uint32_t)((nb + UZ_TBX_TILE - 1) / UZ_TBX_TILE);
    const size_t o_off = up256((size_t)n_tiles * 4);
    c->tbx_chunk.ensure(o_off + ((size_t)n_tiles + 1) * 8 + 64);
    c->tbx_pin.room(4096);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(c->tbx_chunk.p);
    int64_t *toff = reinterpret_cast<int64_t *>(c->tbx_chunk.p + o_off);
    {
        ProfScope ps(c, UZ_K_TBX_KEYS);
        hipLaunchKernelGGL(k_tbx_mark, dim3((n_tiles + UZ_TBX_WAVES - 1) / UZ_TBX_WAVES), dim3(64 * UZ_TBX_WAVES), 0, c->stream, d_in, (uint32_t)nb, n_tiles,
                           chunk_carry(t, q) ? 1 : 0, cnt);
        UZ_HIP(hipGetLastError());
        uz_len_scan(c, c->stream, n_tiles, cnt, 0, toff);
    }
    uz_kcopy(c, c->tbx_pin.p, toff + n_tiles, 8); // the chunk's rows
}

void uz_tbx_keys(uz_ctx *c, TbxCall &t, size_t q, const uint8_t *d_in, size_t nb, const int64_t *d_off, int64_t base) {
    const int64_t nr = *reinterpret_cast<const int64_t *>(c->tbx_pin.p);
    UZ_REQUIRE(nr >= 0 && nr <= (int64_t)nb, UZ_E_STATE, "BGZF index: a chunk's count of lines is not one");
    if (!nr) return;
    const uint32_t n_tiles = (uint32_t)((nb + UZ_TBX_TILE - 1) / UZ_TBX_TILE);
    const int64_t *toff = reinterpret_cast<const int64_t *>(c->tbx_chunk.p + up256((size_t)n_tiles * 4));
    const bool carry = chunk_carry(t, q), text_end = q + 1 == t.n_chunks;
    const uint64_t text_at = (uint64_t)q * t.chunk_bytes;
    grow_keep(c, c->tbx_rows, (size_t)(t.n_rows + nr) * sizeof(TbxRow) + 64, (size_t)t.n_rows * sizeof(TbxRow));
    c->tbx_work.ensure((size_t)nr * 4 + 64);
    uint32_t *starts = reinterpret_cast<uint32_t *>(c->tbx_work.p);
    TbxRow *rows = reinterpret_cast<TbxRow *>(c->tbx_rows.p) + t.n_rows;
    {
        ProfScope ps(c, UZ_K_TBX_KEYS);
        hipLaunchKernelGGL(k_tbx_starts, dim3((n_tiles + UZ_TBX_WAVES - 1) / UZ_TBX_WAVES), dim3(64 * UZ_TBX_WAVES), 0, c->stream, d_in, (uint32_t)nb, n_tiles, carry ? 1 : 0,
                           toff, nr, starts);
        UZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tbx_keys, dim3((unsigned)((nr + UZ_TBX_WAVES - 1) / UZ_TBX_WAVES)), dim3(64 * UZ_TBX_WAVES), 0, c->stream, d_in, (uint32_t)nb, text_end ? 1 : 0,
                           t.preset, (const uint32_t *)starts, nr, d_off, (int32_t)((nb + UZ_DF_SLICE - 1) / UZ_DF_SLICE), base, text_at, rows);
        UZ_HIP(hipGetLastError());
    }
    // the host's rows: the chunk's first line, and its last one where the chunk's end cuts its key columns
    const uint8_t *d = t.data + text_at;
    const uint8_t *nl0 = carry || nb < 2 ? nullptr : (const uint8_t *)memchr(d, '\n', nb - 1);
    const uint8_t *nl1 = nb < 2 ? nullptr : (const uint8_t *)memrchr(d, '\n', nb - 1);
    const int64_t first = carry ? 0 : nl0 ? (nl0 - d) + 1 : -1, last = nl1 ? (nl1 - d) + 1 : carry ? 0 : -1;
    UZ_REQUIRE(first >= 0 && last >= first, UZ_E_STATE, "BGZF index: the device counts lines in a chunk where the host finds none");
    t.settled.emplace_back(t.n_rows, uz_tbx_settle(t, text_at + (uint64_t)first));
    if (last != first) {
        UzTbxHostWave w;
        UzTbxKey k;
        uz_tbx_key(w, t.data, text_at + (uint64_t)last, text_at + nb, text_end, t.preset, k); // as the device sees it
        if (k.kind == UZ_TBX_CUT) t.settled.emplace_back(t.n_rows + nr - 1, uz_tbx_settle(t, text_at + (uint64_t)last));
    }
    t.n_rows += nr;
}

void uz_tbx_tables(uz_ctx *c, TbxCall &t, int64_t eof_at) {
    hipStream_t st = c->stream;
    uz_tbx_view &V = *t.view;
    const int64_t n = t.n_rows;
    V.n_rows = n;
    V.host_rows = (int64_t)t.settled.size();
    if (!n) return;
    TbxRow *rows = reinterpret_cast<TbxRow *>(c->tbx_rows.p);
    const size_t n_set = t.settled.size(), o_at = 4096, o_from = o_at + up256(n_set * 8);
    c->tbx_pin.room(o_from + n_set * sizeof(TbxRow) + 64);
    for (size_t i = 0; i < n_set; i++) {
        reinterpret_cast<int64_t *>(c->tbx_pin.p + o_at)[i] = t.settled[i].first;
        reinterpret_cast<TbxRow *>(c->tbx_pin.p + o_from)[i] = t.settled[i].second;
    }
    // the work arrays of the passes: is_new [n], is_run [n], new_off [n + 1], run_off [n + 1], the status word
    const size_t o_run = up256((size_t)n * 4), o_noff = o_run + up256((size_t)n * 4), o_roff = o_noff + up256(((size_t)n + 1) * 8), o_st = o_roff + up256(((size_t)n + 1) * 8);
    c->tbx_work.ensure(o_st + 256);
    uint32_t *is_new = reinterpret_cast<uint32_t *>(c->tbx_work.p), *is_run = reinterpret_cast<uint32_t *>(c->tbx_work.p + o_run);
    int64_t *new_off = reinterpret_cast<int64_t *>(c->tbx_work.p + o_noff), *run_off = reinterpret_cast<int64_t *>(c->tbx_work.p + o_roff);
    uint32_t *status = reinterpret_cast<uint32_t *>(c->tbx_work.p + o_st);
    const unsigned grid = (unsigned)((n + 255) / 256);
    UZ_HIP(hipMemsetAsync(status, 0, 8, st));
    {
        ProfScope ps(c, UZ_K_TBX_TABLE);
        hipLaunchKernelGGL(k_tbx_patch, dim3((unsigned)((n_set + 63) / 64)), dim3(64), 0, st, (int32_t)n_set, (const int64_t *)(c->tbx_pin.p + o_at),
                           (const TbxRow *)(c->tbx_pin.p + o_from), n, rows);
        UZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tbx_flags, dim3(grid), dim3(256), 0, st, n, (const TbxRow *)rows, is_new, is_run, status);
        UZ_HIP(hipGetLastError());
        uz_len_scan(c, st, n, is_new, 0, new_off);
        uz_len_scan(c, st, n, is_run, 0, run_off);
    }
    const KCopySeg down[3] = {{c->tbx_pin.p, new_off + n, 8}, {c->tbx_pin.p + 8, run_off + n, 8}, {c->tbx_pin.p + 16, status, 8}};
    uz_kcopy_many(c, down, 3);
    UZ_HIP(hipStreamSynchronize(st));
    const int64_t n_refs = reinterpret_cast<const int64_t *>(c->tbx_pin.p)[0], n_runs = reinterpret_cast<const int64_t *>(c->tbx_pin.p)[1];
    V.status = *reinterpret_cast<const uint32_t *>(c->tbx_pin.p + 16);
    UZ_REQUIRE(n_refs >= 0 && n_refs <= n_runs && n_runs <= n, UZ_E_STATE, "BGZF index: more references than runs, or more runs than rows");
    if (V.status || !n_refs) return;
    // the tables: refs [n_refs], runs [n_runs]; behind them the passes' own: max_end, n_intv, first, last, lin_off [n_refs + 1]
    const size_t refs_bytes = (size_t)n_refs * sizeof(uz_tbx_ref), runs_bytes = (size_t)n_runs * sizeof(uz_tbx_run);
    const size_t o_runs = up256(refs_bytes), o_max = o_runs + up256(runs_bytes), o_ni = o_max + up256((size_t)n_refs * 4), o_first = o_ni + up256((size_t)n_refs * 4),
                 o_last = o_first + up256((size_t)n_refs * 8), o_lin = o_last + up256((size_t)n_refs * 8), tab_bytes = o_lin + up256(((size_t)n_refs + 1) * 8);
    c->tbx_tab.ensure(tab_bytes + 64);
    uint8_t *tab = c->tbx_tab.p;
    TbxTables T{reinterpret_cast<uz_tbx_ref *>(tab), reinterpret_cast<uz_tbx_run *>(tab + o_runs), reinterpret_cast<uint32_t *>(tab + o_max),
                reinterpret_cast<uint32_t *>(tab + o_ni), reinterpret_cast<int64_t *>(tab + o_first), reinterpret_cast<int64_t *>(tab + o_last),
                reinterpret_cast<int64_t *>(tab + o_lin)};
    UZ_HIP(hipMemsetAsync(tab, 0, tab_bytes, st));
    {
        ProfScope ps(c, UZ_K_TBX_TABLE);
        hipLaunchKernelGGL(k_tbx_emit, dim3(grid), dim3(256), 0, st, n, (const TbxRow *)rows, (const uint32_t *)is_new, (const int64_t *)new_off, (const uint32_t *)is_run,
                           (const int64_t *)run_off, (uint64_t)eof_at << 16, n_refs, n_runs, T);
        UZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tbx_nintv, dim3((unsigned)((n_refs + 255) / 256)), dim3(256), 0, st, n_refs, T);
        UZ_HIP(hipGetLastError());
        uz_len_scan(c, st, n_refs, T.n_intv, 0, T.lin_off);
    }
    uz_kcopy(c, c->tbx_pin.p + 24, T.lin_off + n_refs, 8);
    UZ_HIP(hipStreamSynchronize(st));
    const int64_t n_lin = *reinterpret_cast<const int64_t *>(c->tbx_pin.p + 24);
    UZ_REQUIRE(n_lin >= n_refs && n_lin <= n_refs * ((UZ_TBX_MAX_END >> 14)), UZ_E_STATE, "BGZF index: a linear table out of its scheme's reach");
    const size_t lin_bytes = (size_t)n_lin * 8;
    c->tbx_chunk.ensure(lin_bytes + 64); // (the chunks are done: their block holds the linear table)
    unsigned long long *linear = reinterpret_cast<unsigned long long *>(c->tbx_chunk.p);
    UZ_HIP(hipMemsetAsync(linear, 0xFF, lin_bytes, st));
    {
        ProfScope ps(c, UZ_K_TBX_TABLE);
        hipLaunchKernelGGL(k_tbx_linear, dim3(grid), dim3(256), 0, st, n, (const TbxRow *)rows, (const uint32_t *)is_new, (const int64_t *)new_off, n_refs, T, linear);
        UZ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tbx_fill, dim3((unsigned)n_refs), dim3(256), 0, st, T, linear);
        UZ_HIP(hipGetLastError());
    }
    const size_t p_refs = 4096, p_runs = p_refs + up256(refs_bytes), p_lin = p_runs + up256(runs_bytes);
    c->tbx_pin.room(p_lin + lin_bytes + 64);
    const KCopySeg tables[3] = {{c->tbx_pin.p + p_refs, T.refs, refs_bytes}, {c->tbx_pin.p + p_runs, T.runs, runs_bytes}, {c->tbx_pin.p + p_lin, linear, lin_bytes}};
    uz_kcopy_many(c, tables, 3);
    UZ_HIP(hipStreamSynchronize(st));
    V.n_refs = n_refs; V.n_runs = n_runs; V.n_linear = n_lin;
    V.refs = reinterpret_cast<const uz_tbx_ref *>(c->tbx_pin.p + p_refs);
    V.runs = reinterpret_cast<const uz_tbx_run *>(c->tbx_pin.p + p_runs);
    V.linear = reinterpret_cast<const uint64_t *>(c->tbx_pin.p + p_lin);
}
