// k_bcf.hip -- the per-sample values of a BCF read on the device, straight into the rows of a sample table (uz_samples_from_bcf, tables.hip).
//
// The host has inflated the blocks, walked the records and proven every FORMAT array to lie inside its record (io_vcf.cpp:
// uz_vcf_decode_regions_lazy on a .bcf); what is left is GT, AD (or RO / AO) and GQ of every picked sample at every record -- the
// gt_types / gt_ref_depths / gt_alt_depths / gt_quals reads behind `vcf(region)` (informative_site_finder.py:257-260, :41-43, :213).  A field's
// values lie at a fixed stride per sample, so there is no field-start pass: the host gathers ONLY the value arrays of the five fields into a
// chunk's image, back to back, each on a 4-byte boundary (PL, DP and the rest of the record stay home), with five 32-bit offsets and five
// descriptors per record, and one kernel runs per chunk, chunk k + 1 copied while chunk k is read:
//   k_bcf_cells  a workgroup takes 64 consecutive records x 64 consecutive j -- j runs over the picked rows in the order of their file columns,
//                so a wave's 64 lanes read 64 neighbouring samples of one record at a constant stride, the record's offsets and descriptors
//                being wave-uniform (scalar loads).  Every lane runs uz_bcf_cell (bcf_cell.hpp: the body the CPU test runs); the values go
//                through the padded LDS tiles of k_vcf_cells and leave transposed, 64 consecutive sites per row and store.
// A cell the body will not vouch for marks its record in `unsettled`; the host's own reader settles those records (uz_samples_settle).
#include "uz_ctx.hpp"
#include "bcf_cell.hpp"

#include <algorithm>

#define UZ_BCF_TILE 64

namespace {

// off / desc [n_rec][5]: where the arrays of GT, AD, RO, AO, GQ of a record lie in `data` (multiples of 4) and their descriptors (0: absent --
// also every field of a record the host keeps to itself); col_of_j / row_of_j [n_pick]: the file column and the table row of j.
// LDS as in k_vcf_cells: three 16-bit planes [64 records][66] and one byte plane [64][68] -- a lane writes its cell at [record][j] (consecutive
// lanes, consecutive halfwords) and reads [record = lane][j] back at a stride of 33 (17) dwords: no bank is hit twice.
__global__ __launch_bounds__(256) void k_bcf_cells(int32_t n_rec, int64_t site0, const uint8_t *__restrict__ data, const uint32_t *__restrict__ off,
                                                   const uint32_t *__restrict__ desc, int32_t n_pick, const int32_t *__restrict__ col_of_j,
                                                   const int32_t *__restrict__ row_of_j, uint8_t *__restrict__ gt, uint16_t *__restrict__ rd,
                                                   uint16_t *__restrict__ ad, uint16_t *__restrict__ gq, size_t stride, uint8_t *__restrict__ unsettled) {
    __shared__ uint16_t t_rd[UZ_BCF_TILE][66], t_ad[UZ_BCF_TILE][66], t_gq[UZ_BCF_TILE][66];
    __shared__ uint8_t t_gt[UZ_BCF_TILE][68];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (uniform, and now provably so: the record's ten words load once per wave)
    const int32_t rec0 = (int32_t)blockIdx.x * UZ_BCF_TILE, j0 = (int32_t)blockIdx.y * UZ_BCF_TILE;
    const int32_t j = j0 + lane;
    const uint32_t col = j < n_pick ? (uint32_t)col_of_j[j] : 0u;
    for (int r = wave; r < UZ_BCF_TILE; r += 4) {
        const int32_t rec = rec0 + r;
        if (rec >= n_rec) break;
        const uint32_t *__restrict__ o = off + (size_t)rec * 5, *__restrict__ d = desc + (size_t)rec * 5;
        const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
        UzVcfCell c = uz_vcf_cell_default();
        if (j < n_pick && (d0 | d1 | d2 | d3 | d4)) {
            // this sample's values: array + column * values per sample * bytes per value (an absent field's pointer is never read)
            c = uz_bcf_cell(data + o[0] + (size_t)col * (d0 >> 4) * uz_bc_size(d0 & 15u), d0, data + o[1] + (size_t)col * (d1 >> 4) * uz_bc_size(d1 & 15u), d1,
                            data + o[2] + (size_t)col * (d2 >> 4) * uz_bc_size(d2 & 15u), d2, data + o[3] + (size_t)col * (d3 >> 4) * uz_bc_size(d3 & 15u), d3,
                            data + o[4] + (size_t)col * (d4 >> 4) * uz_bc_size(d4 & 15u), d4);
            if (!c.settled) unsettled[site0 + rec] = 1;
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
    for (int q = wave; q < UZ_BCF_TILE; q += 4) {
        if (j0 + q >= n_pick) break;
        const size_t at = (size_t)row_of_j[j0 + q] * stride + site;
        gt[at] = t_gt[lane][q];
        rd[at] = t_rd[lane][q];
        ad[at] = t_ad[lane][q];
        gq[at] = t_gq[lane][q];
    }
}

struct Chunk {
    int64_t r0, r1; // records
    size_t bytes;   // gathered values
};

inline size_t al4(size_t x) { return (x + 3) & ~(size_t)3; }

} // namespace

// The rows of `m` (carved, m.stride set) from the BCF's value arrays: streams the chunks, runs the kernel per chunk, returns the records to hand
// back to the host (ascending).  Synchronous: the rows are in place when it returns.
void uz_vcf_parse_bcf(uz_ctx *c, const uz_vcf_bcf_view *t, int32_t n_pick, const int32_t *pick, SamplesDev &m, size_t chunk_bytes, std::vector<int64_t> &unsettled) {
    const int64_t S = t->n_records;
    unsettled.clear();
    if (S <= 0 || n_pick <= 0) return;
    const size_t n_smp = (size_t)t->n_samples;
    // the picked rows in the order of their file columns
    std::vector<int32_t> order((size_t)n_pick);
    for (int32_t r = 0; r < n_pick; r++) order[(size_t)r] = r;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pick[a] < pick[b]; });
    std::vector<int32_t> small(2 * (size_t)n_pick); // col_of_j | row_of_j
    int32_t *col_of_j = small.data(), *row_of_j = col_of_j + n_pick;
    for (int32_t j = 0; j < n_pick; j++) { col_of_j[j] = pick[order[(size_t)j]]; row_of_j[j] = order[(size_t)j]; }
    // Per record: the bytes its five arrays take in an image, or "the host keeps it" -- the host's own share of "unsettled": a type the kernel
    // does not take, or arrays beyond what an image's 32-bit offsets hold; never silently wrong.  The view is checked here once more: the
    // device is only ever given arrays that lie inside the data.
    const uint64_t span_max = 0xFFFF0000ull;
    std::vector<uint8_t> flag((size_t)S, 0);
    std::vector<uint64_t> need((size_t)S, 0);
    auto field_bytes = [&](uint32_t d) { return (uint64_t)(d >> 4) * uz_bc_size(d & 15u) * n_smp; };
    for (int64_t i = 0; i < S; i++) {
        uint64_t sum = 0;
        bool ok = true;
        for (int k = 0; k < 5; k++) {
            const uint32_t d = t->fld_desc[i * 5 + k];
            if (!d) continue;
            const uint32_t ty = d & 15u;
            if (!(uz_bc_is_int(ty) || (k == 4 && ty == UZ_BC_FLOAT))) { ok = false; continue; }
            const uint64_t b = field_bytes(d);
            UZ_REQUIRE(t->fld_at[i * 5 + k] <= (uint64_t)t->data_bytes && b <= (uint64_t)t->data_bytes - t->fld_at[i * 5 + k], UZ_E_ARG,
                       "a record's FORMAT values lie outside the data");
            sum += al4(b);
        }
        if (!ok || sum > span_max) { flag[(size_t)i] = 1; sum = 0; }
        need[(size_t)i] = sum;
    }
    std::vector<Chunk> chunks;
    for (int64_t i = 0; i < S;) {
        size_t bytes = (size_t)need[(size_t)i];
        int64_t k = i + 1;
        while (k < S && bytes + need[(size_t)k] <= chunk_bytes) { bytes += (size_t)need[(size_t)k]; k++; }
        chunks.push_back(Chunk{i, k, bytes});
        i = k;
    }
    size_t max_bytes = 0, max_rec = 0;
    for (const Chunk &ck : chunks) { max_bytes = std::max(max_bytes, ck.bytes); max_rec = std::max<size_t>(max_rec, (size_t)(ck.r1 - ck.r0)); }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // one image per chunk, the device block its mirror: [values | off [records][5] | desc [records][5]]
    const size_t o_off = al(max_bytes + 16), o_desc = al(o_off + 20 * max_rec), image = al(o_desc + 20 * max_rec);
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
            dev[b] = uz_block_get(c, image + 256);
            if (c->vcf_pin_cap[b] < image) {
                if (c->vcf_pin[b]) (void)hipHostFree(c->vcf_pin[b]);
                c->vcf_pin[b] = nullptr; c->vcf_pin_cap[b] = 0;
                UZ_HIP(hipHostMalloc((void **)&c->vcf_pin[b], image, hipHostMallocDefault));
                c->vcf_pin_cap[b] = image;
            }
            UZ_HIP(hipEventCreateWithFlags(&copied[b], hipEventDisableTiming));
            UZ_HIP(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        }
        const bool time_copy = (c->prof_mask >> UZ_K_BCF_COPY & 1u) != 0;
        for (size_t q = 0; q < chunks.size(); q++) {
            const Chunk &ck = chunks[q];
            const int b = (int)(q & 1);
            const int32_t nr = (int32_t)(ck.r1 - ck.r0);
            if (queued[b]) UZ_HIP(hipEventSynchronize(done[b])); // the chunk before last has been read: its image and its block are free
            uint8_t *pin = c->vcf_pin[b];
            uint32_t *h_off = reinterpret_cast<uint32_t *>(pin + o_off), *h_desc = reinterpret_cast<uint32_t *>(pin + o_desc);
            size_t at = 0;
            for (int32_t r = 0; r < nr; r++) {
                const int64_t i = ck.r0 + r;
                for (int k = 0; k < 5; k++) {
                    const uint32_t d = flag[(size_t)i] ? 0u : t->fld_desc[i * 5 + k];
                    h_off[r * 5 + k] = (uint32_t)at;
                    h_desc[r * 5 + k] = d;
                    if (!d) continue;
                    const size_t nb = (size_t)field_bytes(d);
                    memcpy(pin + at, t->data + t->fld_at[i * 5 + k], nb);
                    at += al4(nb);
                }
            }
            UZ_REQUIRE(at == ck.bytes, UZ_E_STATE, "a chunk's gathered bytes are not the bytes it was cut for");
            hipEvent_t ca = nullptr, cb = nullptr;
            if (time_copy) {
                for (hipEvent_t *e : {&ca, &cb}) {
                    if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); }
                    else UZ_HIP(hipEventCreate(e));
                }
                UZ_HIP(hipEventRecord(ca, c->copy_stream));
            }
            // the values and the record arrays in two copies (the gap between them is as large as the largest chunk's slack)
            if (ck.bytes) UZ_HIP(hipMemcpyAsync(dev[b].p, pin, al4(ck.bytes), hipMemcpyHostToDevice, c->copy_stream));
            UZ_HIP(hipMemcpyAsync(dev[b].p + o_off, pin + o_off, image - o_off, hipMemcpyHostToDevice, c->copy_stream));
            if (time_copy) {
                UZ_HIP(hipEventRecord(cb, c->copy_stream));
                c->prof_pending.push_back(ProfPending{UZ_K_BCF_COPY, ca, cb});
                c->prof[UZ_K_BCF_COPY].last_units = (int64_t)ck.bytes;
            }
            UZ_HIP(hipEventRecord(copied[b], c->copy_stream));
            UZ_HIP(hipStreamWaitEvent(c->stream, copied[b], 0));
            {
                ProfScope ps(c, UZ_K_BCF_CELLS);
                hipLaunchKernelGGL(k_bcf_cells, dim3((unsigned)((nr + UZ_BCF_TILE - 1) / UZ_BCF_TILE), (unsigned)((n_pick + UZ_BCF_TILE - 1) / UZ_BCF_TILE)), dim3(256), 0,
                                   c->stream, nr, ck.r0, (const uint8_t *)dev[b].p, (const uint32_t *)(dev[b].p + o_off), (const uint32_t *)(dev[b].p + o_desc), n_pick,
                                   (const int32_t *)d_small, (const int32_t *)(d_small + n_pick), m.gt, m.rd, m.ad, m.gq, m.stride, d_flag);
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
