// k_vcf.hip -- the sample cells of a text VCF parsed on the device, straight into the rows of a sample table (uz_samples_from_text, tables.hip).
//
// The host has inflated the blocks, found the lines and parsed the eight fixed columns and FORMAT (io_vcf.cpp: uz_vcf_decode_regions_lazy); what
// is left is GT, AD (or RO / AO) and GQ of every picked sample at every record -- more than 99 % of a cohort file's decode time on the host, and
// 17 bytes per cell of host columns nobody reads on the cohort route (informative_site_finder.py:257-260 behind `vcf(region)`, :42, :213).
//
// The text goes up in bounded chunks cut at line ends, chunk k + 1 copied while chunk k is parsed, and two kernels run per chunk:
//   k_vcf_tabs   a wave per record scans the record's sample region 1 KiB at a time (one 16-byte load per lane), marks the tabs, numbers the
//                columns by a wave prefix sum and writes the field start of every PICKED column into starts[record][j] -- j runs over the picked
//                rows in the order of their file columns, so that neighbouring j are neighbouring text.
//   k_vcf_cells  a workgroup takes 64 consecutive records x 64 consecutive j.  A wave reads one record's 64 field starts in one coalesced load
//                and every lane parses one cell (vcf_cell.hpp: the body the CPU tests run); the values go through an LDS tile and leave
//                transposed, so that every row receives 64 consecutive sites in one 64- or 128-byte store.  The table is sample-major: a
//                workgroup per record that stores one byte into each of 1 800 rows is the design this avoids.
// A cell the parser will not vouch for marks its record in `unsettled`; the host's own reader settles those records afterwards (uz_samples_settle).
#include "uz_ctx.hpp"
#include "vcf_cell.hpp"

#include <algorithm>
#include <thread>

#define UZ_VCF_NO_FIELD 0xFFFFFFFFu // starts[][]: the line has no such column (it reads as "." -- every field at its default)
#define UZ_VCF_TILE 64
#define UZ_VCF_PAD 2048 // bytes behind a chunk's text the tab scan may load (and mask out)

namespace {

// 0x80 in every byte of w that equals '\t' (exact: no carry between bytes)
__device__ __forceinline__ uint32_t tab_bytes(uint32_t w) {
    const uint32_t x = w ^ 0x09090909u;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t tab_nibble(uint32_t w) {
    const uint32_t t = tab_bytes(w);
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// rec_beg / rec_end: the sample region of every record of the chunk, relative to `text` (16-byte aligned, UZ_VCF_PAD readable bytes behind the
// last region); slots: the five FORMAT slots as bytes (0xFF: absent) -- a record without any is skipped (its starts stay UZ_VCF_NO_FIELD);
// j_of_col [n_cols]: the first j whose picked column is c, or -1; col_of_j [n_pick] ascending (equal columns = a column picked twice).
__global__ __launch_bounds__(256) void k_vcf_tabs(int32_t n_rec, const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_beg,
                                                  const uint32_t *__restrict__ rec_end, const unsigned long long *__restrict__ slots, int32_t n_cols,
                                                  const int32_t *__restrict__ j_of_col, const int32_t *__restrict__ col_of_j, int32_t n_pick, int32_t last_col,
                                                  uint32_t *__restrict__ starts) {
    const int lane = threadIdx.x & 63;
    const int32_t rec = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
    if (rec >= n_rec) return;
    if ((slots[rec] & 0xFFFFFFFFFFull) == 0xFFFFFFFFFFull) return;
    const uint32_t beg = rec_beg[rec], end = rec_end[rec];
    uint32_t *__restrict__ out = starts + (size_t)rec * (size_t)n_pick;
    auto put = [&](int32_t col, uint32_t at) {
        if (col >= n_cols) return;
        int32_t j = j_of_col[col];
        if (j < 0) return;
        do { out[j] = at; j++; } while (j < n_pick && col_of_j[j] == col);
    };
    if (lane == 0) put(0, beg);
    int32_t seen = 0; // tabs before this step's kilobyte = the column its first byte lies in
    for (uint64_t base = beg & ~15u; base < end && seen < last_col; base += 1024) {
        const uint64_t at = base + (uint64_t)lane * 16;
        const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
        uint32_t m = tab_nibble(v.x) | tab_nibble(v.y) << 4 | tab_nibble(v.z) << 8 | tab_nibble(v.w) << 12;
        // the bytes of this lane that lie inside [beg, end)
        int64_t lo = (int64_t)beg - (int64_t)at, hi = (int64_t)end - (int64_t)at;
        lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
        hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
        m &= ((1u << (uint32_t)hi) - 1u) & ~((1u << (uint32_t)lo) - 1u);
        const int32_t cnt = __popc(m);
        int32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        int32_t col = seen + incl - cnt; // the column of this lane's first byte
        while (m) {
            const int k = __ffs(m) - 1;
            m &= m - 1;
            col++;
            put(col, (uint32_t)at + (uint32_t)k + 1u);
        }
        seen += __shfl(incl, 63, 64);
    }
}

// The tile of 64 records x 64 j.  LDS: three 16-bit planes [64 records][66] and one byte plane [64][68] -- a lane writes its cell at
// [record][j] (consecutive lanes, consecutive halfwords) and reads [record = lane][j] back at a stride of 33 (17) dwords: no bank is hit twice.
__global__ __launch_bounds__(256) void k_vcf_cells(int32_t n_rec, int64_t site0, const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_end,
                                                   const unsigned long long *__restrict__ slots, int32_t n_pick, const int32_t *__restrict__ row_of_j,
                                                   const uint32_t *__restrict__ starts, uint8_t *__restrict__ gt, uint16_t *__restrict__ rd,
                                                   uint16_t *__restrict__ ad, uint16_t *__restrict__ gq, size_t stride, uint8_t *__restrict__ unsettled) {
    __shared__ uint16_t t_rd[UZ_VCF_TILE][66], t_ad[UZ_VCF_TILE][66], t_gq[UZ_VCF_TILE][66];
    __shared__ uint8_t t_gt[UZ_VCF_TILE][68];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t rec0 = (int32_t)blockIdx.x * UZ_VCF_TILE, j0 = (int32_t)blockIdx.y * UZ_VCF_TILE;
    const int32_t j = j0 + lane;
    for (int r = wave; r < UZ_VCF_TILE; r += 4) {
        const int32_t rec = rec0 + r;
        if (rec >= n_rec) break;
        UzVcfCell c = uz_vcf_cell_default();
        if (j < n_pick) {
            const uint32_t at = starts[(size_t)rec * (size_t)n_pick + (size_t)j];
            if (at != UZ_VCF_NO_FIELD) {
                const uint32_t end = rec_end[rec];
                const uint8_t *__restrict__ p = text + at;
                uint32_t len = 0;
                while (at + len < end && p[len] != '\t') len++;
                const unsigned long long s = slots[rec];
                c = uz_vcf_cell(p, len, (int)(int8_t)(s & 0xFF), (int)(int8_t)(s >> 8 & 0xFF), (int)(int8_t)(s >> 16 & 0xFF), (int)(int8_t)(s >> 24 & 0xFF),
                                (int)(int8_t)(s >> 32 & 0xFF));
                if (!c.settled) unsettled[site0 + rec] = 1;
            }
        }
        t_gt[r][lane] = (uint8_t)c.gt;
        t_rd[r][lane] = (uint16_t)c.rd;
        t_ad[r][lane] = (uint16_t)c.ad;
        t_gq[r][lane] = (uint16_t)c.gq;
    }
    __syncthreads();
    const int32_t rec = rec0 + lane;
    if (rec >= n_rec) return;
    const size_t site = (size_t)(site0 + rec);
    for (int q = wave; q < UZ_VCF_TILE; q += 4) {
        if (j0 + q >= n_pick) break;
        const size_t o = (size_t)row_of_j[j0 + q] * stride + site;
        gt[o] = t_gt[lane][q];
        rd[o] = t_rd[lane][q];
        ad[o] = t_ad[lane][q];
        gq[o] = t_gq[lane][q];
    }
}

// the cells of the handed-back sites over those of the device's parse: in [n_rows][n] -> out[row][site[k]]
__global__ __launch_bounds__(256) void k_vcf_settle(int64_t n, int32_t n_rows, const int64_t *__restrict__ site, const uint8_t *__restrict__ gt_in,
                                                    const uint16_t *__restrict__ rd_in, const uint16_t *__restrict__ ad_in, const uint16_t *__restrict__ gq_in,
                                                    uint8_t *__restrict__ gt, uint16_t *__restrict__ rd, uint16_t *__restrict__ ad, uint16_t *__restrict__ gq, size_t stride) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;
    if (k >= n) return;
    const size_t i = row * (size_t)n + (size_t)k, o = row * stride + (size_t)site[k];
    gt[o] = gt_in[i]; rd[o] = rd_in[i]; ad[o] = ad_in[i]; gq[o] = gq_in[i];
}

struct Chunk {
    int64_t r0, r1;     // records
    uint64_t t0, bytes; // text
};

void gather(uint8_t *dst, const uint8_t *src, size_t n) { // pageable -> pinned, on a few threads when it is worth their start
    const int T = n >= ((size_t)8 << 20) ? 4 : 1;
    if (T == 1) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const size_t step = ((n + T - 1) / T + 4095) & ~(size_t)4095;
    for (size_t a = step; a < n; a += step) th.emplace_back([=] { memcpy(dst + a, src + a, std::min(step, n - a)); });
    memcpy(dst, src, std::min(step, n));
    for (auto &t : th) t.join();
}

} // namespace

void uz_launch_vcf_settle(uz_ctx *c, int64_t n, int32_t n_rows, const int64_t *site, const uint8_t *gt_in, const uint16_t *rd_in, const uint16_t *ad_in,
                          const uint16_t *gq_in, SamplesDev &m) {
    if (n <= 0 || n_rows <= 0) return;
    for (int32_t r0 = 0; r0 < n_rows; r0 += 65535) {
        const int32_t nr = std::min<int32_t>(65535, n_rows - r0);
        const size_t a = (size_t)r0 * (size_t)n, b = (size_t)r0 * m.stride;
        hipLaunchKernelGGL(k_vcf_settle, dim3((unsigned)((n + 255) / 256), (unsigned)nr), dim3(256), 0, c->stream, n, nr, site, gt_in + a, rd_in + a, ad_in + a,
                           gq_in + a, m.gt + b, m.rd + b, m.ad + b, m.gq + b, m.stride);
        UZ_HIP(hipGetLastError());
    }
}

// The rows of `m` (carved, m.stride set) from the text: streams the chunks, runs the two kernels per chunk, returns the records to hand back
// to the host (ascending).  Synchronous: the rows are in place when it returns.
void uz_vcf_parse_text(uz_ctx *c, const uz_vcf_text_view *t, int32_t n_pick, const int32_t *pick, SamplesDev &m, size_t chunk_bytes, std::vector<int64_t> &unsettled) {
    const int64_t S = t->n_records;
    unsettled.clear();
    if (S <= 0 || n_pick <= 0) return;
    const int32_t n_cols = t->n_samples;
    // the picked rows in the order of their file columns
    std::vector<int32_t> order((size_t)n_pick);
    for (int32_t r = 0; r < n_pick; r++) order[(size_t)r] = r;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pick[a] < pick[b]; });
    std::vector<int32_t> small((size_t)n_cols + 2 * (size_t)n_pick, -1); // j_of_col | col_of_j | row_of_j
    int32_t *j_of_col = small.data(), *col_of_j = j_of_col + n_cols, *row_of_j = col_of_j + n_pick;
    for (int32_t j = n_pick - 1; j >= 0; j--) {
        col_of_j[j] = pick[order[(size_t)j]];
        row_of_j[j] = order[(size_t)j];
        j_of_col[col_of_j[j]] = j;
    }
    const int32_t last_col = col_of_j[n_pick - 1];
    // the host's own share of "unsettled": limits of the kernels' formats, never silently wrong
    std::vector<uint8_t> flag((size_t)S, 0);
    auto slot_fits = [&](int64_t i) {
        for (int k = 0; k < 5; k++)
            if (t->fmt_slot[i * 5 + k] > 127) return false; // beyond what the slot byte holds
        return true;
    };
    const uint64_t span_max = 0xFFFF0000ull; // the kernels' offsets are 32 bits wide
    std::vector<Chunk> chunks;
    for (int64_t i = 0; i < S;) {
        UZ_REQUIRE(t->samp_at[i] <= t->line_end[i] && t->line_end[i] <= (uint64_t)t->text_bytes, UZ_E_ARG, "a record's sample region lies outside the text");
        if (t->line_end[i] - t->samp_at[i] > span_max) { flag[(size_t)i] = 1; i++; continue; }
        int64_t k = i + 1;
        while (k < S && t->line_end[k] >= t->samp_at[i] && t->line_end[k] - t->samp_at[i] <= chunk_bytes && t->samp_at[k] >= t->line_end[k - 1] &&
               t->samp_at[k] <= t->line_end[k])
            k++;
        chunks.push_back(Chunk{i, k, t->samp_at[i], t->line_end[k - 1] - t->samp_at[i]});
        i = k;
    }
    size_t max_text = 0, max_rec = 0;
    for (const Chunk &ck : chunks) { max_text = std::max<size_t>(max_text, ck.bytes); max_rec = std::max<size_t>(max_rec, (size_t)(ck.r1 - ck.r0)); }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // one staging image per chunk: [text + pad | rec_beg | rec_end | slots]; the device block mirrors it and holds the field starts behind
    const size_t o_beg = al(max_text + UZ_VCF_PAD), o_end = al(o_beg + 4 * max_rec), o_slot = al(o_end + 4 * max_rec), image = al(o_slot + 8 * max_rec);
    const size_t o_starts = image, dev_bytes = al(image + 4 * max_rec * (size_t)n_pick) + 256;
    DevBlock dev[2], aux = uz_block_get(c, al(small.size() * 4) + (size_t)S + 512);
    hipEvent_t copied[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    bool queued[2] = {false, false};
    auto cleanup = [&] {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
        for (int b = 0; b < 2; b++) {
            uz_block_put(c, dev[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
            if (done[b]) (void)hipEventDestroy(done[b]);
        }
        uz_block_put(c, aux);
    };
    try {
        int32_t *d_small = reinterpret_cast<int32_t *>(aux.p);
        uint8_t *d_flag = aux.p + al(small.size() * 4);
        UZ_HIP(hipMemcpyAsync(d_small, small.data(), small.size() * 4, hipMemcpyHostToDevice, c->stream));
        UZ_HIP(hipMemsetAsync(d_flag, 0, (size_t)S, c->stream));
        UZ_HIP(hipStreamSynchronize(c->stream)); // (`small` is pageable)
        for (int b = 0; b < 2 && b < (int)chunks.size(); b++) {
            dev[b] = uz_block_get(c, dev_bytes);
            if (c->vcf_pin_cap[b] < image) {
                if (c->vcf_pin[b]) (void)hipHostFree(c->vcf_pin[b]);
                c->vcf_pin[b] = nullptr; c->vcf_pin_cap[b] = 0;
                UZ_HIP(hipHostMalloc((void **)&c->vcf_pin[b], image, hipHostMallocDefault));
                c->vcf_pin_cap[b] = image;
            }
            UZ_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
            UZ_HIP(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        }
        const bool time_copy = (c->prof_mask >> UZ_K_VCF_COPY & 1u) != 0;
        for (size_t q = 0; q < chunks.size(); q++) {
            const Chunk &ck = chunks[q];
            const int b = (int)(q & 1);
            const int32_t nr = (int32_t)(ck.r1 - ck.r0);
            if (queued[b]) UZ_HIP(hipEventSynchronize(done[b])); // the chunk before last has been parsed: its image and its block are free
            uint8_t *pin = c->vcf_pin[b];
            gather(pin, t->text + ck.t0, (size_t)ck.bytes);
            uint32_t *h_beg = reinterpret_cast<uint32_t *>(pin + o_beg), *h_end = reinterpret_cast<uint32_t *>(pin + o_end);
            unsigned long long *h_slot = reinterpret_cast<unsigned long long *>(pin + o_slot);
            for (int32_t r = 0; r < nr; r++) {
                const int64_t i = ck.r0 + r;
                h_beg[r] = (uint32_t)(t->samp_at[i] - ck.t0);
                h_end[r] = (uint32_t)(t->line_end[i] - ck.t0);
                unsigned long long s = 0xFFFFFFFFFFull;
                if (!slot_fits(i)) flag[(size_t)i] = 1;
                else {
                    s = 0;
                    for (int k = 0; k < 5; k++) s |= (unsigned long long)(uint8_t)(int8_t)t->fmt_slot[i * 5 + k] << (8 * k);
                }
                h_slot[r] = s;
            }
            hipEvent_t ca = nullptr, cb = nullptr;
            if (time_copy) {
                for (hipEvent_t *e : {&ca, &cb}) {
                    if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); }
                    else UZ_HIP(hipEventCreate(e));
                }
                UZ_HIP(hipEventRecord(ca, c->copy_stream));
            }
            // the text and the record arrays in two copies (the gap between them is as large as the largest chunk's slack)
            UZ_HIP(hipMemcpyAsync(dev[b].p, pin, al((size_t)ck.bytes), hipMemcpyHostToDevice, c->copy_stream));
            UZ_HIP(hipMemcpyAsync(dev[b].p + o_beg, pin + o_beg, image - o_beg, hipMemcpyHostToDevice, c->copy_stream));
            if (time_copy) {
                UZ_HIP(hipEventRecord(cb, c->copy_stream));
                c->prof_pending.push_back(ProfPending{UZ_K_VCF_COPY, ca, cb});
                c->prof[UZ_K_VCF_COPY].last_units = (int64_t)ck.bytes;
            }
            UZ_HIP(hipEventRecord(copied[b], c->copy_stream));
            UZ_HIP(hipStreamWaitEvent(c->stream, copied[b], 0));
            uint32_t *starts = reinterpret_cast<uint32_t *>(dev[b].p + o_starts);
            UZ_HIP(hipMemsetAsync(starts, 0xFF, 4 * (size_t)nr * (size_t)n_pick, c->stream));
            {
                ProfScope ps(c, UZ_K_VCF_TABS);
                hipLaunchKernelGGL(k_vcf_tabs, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, c->stream, nr, (const uint8_t *)dev[b].p, (const uint32_t *)(dev[b].p + o_beg),
                                   (const uint32_t *)(dev[b].p + o_end), (const unsigned long long *)(dev[b].p + o_slot), n_cols, (const int32_t *)d_small,
                                   (const int32_t *)(d_small + n_cols), n_pick, last_col, starts);
                UZ_HIP(hipGetLastError());
            }
            {
                ProfScope ps(c, UZ_K_VCF_CELLS);
                hipLaunchKernelGGL(k_vcf_cells, dim3((unsigned)((nr + UZ_VCF_TILE - 1) / UZ_VCF_TILE), (unsigned)((n_pick + UZ_VCF_TILE - 1) / UZ_VCF_TILE)), dim3(256), 0,
                                   c->stream, nr, ck.r0, (const uint8_t *)dev[b].p, (const uint32_t *)(dev[b].p + o_end), (const unsigned long long *)(dev[b].p + o_slot),
                                   n_pick, (const int32_t *)(d_small + n_cols + n_pick), (const uint32_t *)starts, m.gt, m.rd, m.ad, m.gq, m.stride, d_flag);
                UZ_HIP(hipGetLastError());
            }
            UZ_HIP(hipEventRecord(done[b], c->stream));
            queued[b] = true;
        }
        UZ_HIP(hipStreamSynchronize(c->stream));
        std::vector<uint8_t> dflag((size_t)S);
        UZ_HIP(hipMemcpy(dflag.data(), d_flag, (size_t)S, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < S; i++)
            if (flag[(size_t)i] | dflag[(size_t)i]) unsettled.push_back(i);
    } catch (...) { cleanup(); throw; }
    cleanup();
}
