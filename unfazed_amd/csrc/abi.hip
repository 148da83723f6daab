// abi.hip -- the extern "C" entry points of include/unfazed_hip.h: context, staging of
// the decoded alignment columns into HBM, and the launch sequence of the stages (the site, family and sample tables: tables.hip).
#include "uz_stage.hpp"
#include "find_answer.hpp"

#include <chrono>
#include <algorithm>
#include <map>
#include <mutex>

bool uz_site_scan_fresh(const uz_ctx *c, const FamilyDev &f, bool need_cnv);

// the page-locked blocks this library handed out (uz_pinned_alloc), for the one-copy path of uz_stage.hpp
static std::mutex g_pinned_mu;
static std::map<uintptr_t, size_t> g_pinned;
bool inside_one_pinned_block(const uint8_t *lo, const uint8_t *hi) {
    std::lock_guard<std::mutex> g(g_pinned_mu);
    auto it = g_pinned.upper_bound((uintptr_t)lo);
    if (it == g_pinned.begin()) return false;
    --it;
    return (uintptr_t)lo >= it->first && (uintptr_t)hi <= it->first + it->second;
}

namespace {

ReadsDev &reads_of(uz_ctx *c, int id) {
    UZ_REQUIRE(id >= 0 && id < (int)c->reads.size() && c->reads[id].live, UZ_E_ARG, "unknown reads handle");
    return c->reads[id];
}

void free_reads(uz_ctx *c, ReadsDev &r) {
    if (r.built) { (void)hipEventSynchronize(r.built); (void)hipEventDestroy(r.built); } // (a table freed before its first use: its build may still run)
    if (r.ready) (void)hipEventDestroy(r.ready);
    uz_block_put(c, r.block);
    uz_block_put(c, r.mirror);
    r = ReadsDev();
}

} // namespace

// ---------------------------------------------------------------- copy kernel (see uz_ctx.hpp)
template <typename W>
__global__ __launch_bounds__(256) void k_copy(W *__restrict__ dst, const W *__restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
void uz_kcopy(uz_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!bytes) return;
    uz_find_launched(c, 1);
    const uintptr_t a = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)bytes;
    auto grid = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)); };
    if (a % 16 == 0) hipLaunchKernelGGL(k_copy<uint4>, grid(bytes / 16), dim3(256), 0, c->stream, (uint4 *)dst, (const uint4 *)src, bytes / 16);
    else if (a % 4 == 0) hipLaunchKernelGGL(k_copy<uint32_t>, grid(bytes / 4), dim3(256), 0, c->stream, (uint32_t *)dst, (const uint32_t *)src, bytes / 4);
    else hipLaunchKernelGGL(k_copy<uint8_t>, grid(bytes), dim3(256), 0, c->stream, (uint8_t *)dst, (const uint8_t *)src, bytes);
    UZ_HIP(hipGetLastError());
}
struct KCopySegs { KCopySeg s[UZ_KCOPY_SEGS]; };
template <typename W>
__device__ __forceinline__ void copy_seg(void *dst, const void *src, size_t n) {
    W *__restrict__ d = (W *)dst;
    const W *__restrict__ s = (const W *)src;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) d[i] = s[i];
}
__global__ __launch_bounds__(256) void k_copy_many(KCopySegs g) {
    const KCopySeg sg = g.s[blockIdx.y];
    const uintptr_t a = (uintptr_t)sg.dst | (uintptr_t)sg.src | (uintptr_t)sg.bytes; // (uniform over the workgroup)
    if (a % 16 == 0) copy_seg<uint4>(sg.dst, sg.src, sg.bytes / 16);
    else if (a % 4 == 0) copy_seg<uint32_t>(sg.dst, sg.src, sg.bytes / 4);
    else copy_seg<uint8_t>(sg.dst, sg.src, sg.bytes);
}
void uz_kcopy_many(uz_ctx *c, const KCopySeg *segs, int n_segs) {
    KCopySegs g;
    int m = 0;
    size_t units = 0; // of the segment with the most of them, in the width it is copied at
    for (int k = 0; k < n_segs; k++) {
        if (!segs[k].bytes) continue;
        UZ_REQUIRE(m < UZ_KCOPY_SEGS, UZ_E_ARG, "uz_kcopy_many: too many segments");
        g.s[m++] = segs[k];
        const uintptr_t a = (uintptr_t)segs[k].dst | (uintptr_t)segs[k].src | (uintptr_t)segs[k].bytes;
        units = std::max(units, segs[k].bytes / (a % 16 == 0 ? 16 : a % 4 == 0 ? 4 : 1));
    }
    if (!m) return;
    uz_find_launched(c, 1);
    for (int k = m; k < UZ_KCOPY_SEGS; k++) g.s[k] = KCopySeg{nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_copy_many, dim3((unsigned)std::min<size_t>((units + 255) / 256, 1024), (unsigned)m), dim3(256), 0, c->stream, g);
    UZ_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- length scan (see uz_ctx.hpp)
__global__ __launch_bounds__(1024) void k_scan_len(int64_t n, const uint32_t *__restrict__ len, uint32_t add, int64_t *__restrict__ off) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry_s;
    const uint32_t t = threadIdx.x, l = t & 63u, wv = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + t;
        const unsigned long long v = i < n ? (unsigned long long)len[i] + add : 0ull;
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
void uz_len_scan(uz_ctx *c, hipStream_t st, int64_t n, const uint32_t *len, uint32_t add, int64_t *off) {
    hipLaunchKernelGGL(k_scan_len, dim3(1), dim3(1024), 0, st, n, len, add, off);
    UZ_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- device block pool
DevBlock uz_block_get(uz_ctx *c, size_t bytes) {
    int best = -1;
    for (size_t i = 0; i < c->block_pool.size(); i++)
        if (c->block_pool[i].cap >= bytes && (best < 0 || c->block_pool[i].cap < c->block_pool[best].cap)) best = (int)i;
    if (best >= 0 && c->block_pool[best].cap <= 2 * bytes + (1 << 20)) {
        DevBlock b = c->block_pool[best];
        c->block_pool.erase(c->block_pool.begin() + best);
        return b;
    }
    DevBlock b;
    b.cap = bytes + bytes / 16 + 4096;
    UZ_HIP(hipMalloc((void **)&b.p, b.cap));
    return b;
}
void uz_block_put(uz_ctx *c, DevBlock b) {
    if (!b.p) return;
    c->block_pool.push_back(b);
    // keep the parked memory bounded: beyond 64 blocks the smallest ones are returned to the driver
    while (c->block_pool.size() > 64) {
        size_t k = 0;
        for (size_t i = 1; i < c->block_pool.size(); i++)
            if (c->block_pool[i].cap < c->block_pool[k].cap) k = i;
        (void)hipFree(c->block_pool[k].p);
        c->block_pool.erase(c->block_pool.begin() + k);
    }
}

// ---------------------------------------------------------------- profiling
void uz_prof_begin(uz_ctx *c, int kernel, hipEvent_t *a, hipEvent_t *b) {
    *a = *b = nullptr;
    if (!(c->prof_mask >> kernel & 1u)) return;
    for (hipEvent_t *e : {a, b}) {
        if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); }
        else UZ_HIP(hipEventCreate(e));
    }
    UZ_HIP(hipEventRecord(*a, c->stream));
}
void uz_prof_end(uz_ctx *c, int kernel, hipEvent_t a, hipEvent_t b) {
    if (!a) return;
    (void)hipEventRecord(b, c->stream);
    c->prof_pending.push_back(ProfPending{kernel, a, b});
}
void uz_prof_drain(uz_ctx *c) {
    for (auto &p : c->prof_pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->prof[p.kernel].total_ms += ms;
            c->prof[p.kernel].launches += 1;
        }
        c->event_pool.push_back(p.a);
        c->event_pool.push_back(p.b);
    }
    c->prof_pending.clear();
}

void uz_stage_dnms(uz_ctx *c, const uz_dnms_view *d) {
    UZ_REQUIRE(d != nullptr && d->n >= 0, UZ_E_ARG, "bad DNM view");
    const size_t n = (size_t)d->n;
    c->dn.n = d->n;
    UZ_REQUIRE(n == 0 || (d->contig && d->rcontig && d->start && d->end && d->vartype && d->dflags && d->mult && d->allele_off),
               UZ_E_ARG, "null DNM column pointer");
    const size_t nb = n ? (size_t)d->allele_off[2 * n] : 0;
    UZ_REQUIRE(nb == 0 || d->alleles != nullptr, UZ_E_ARG, "null DNM column pointer");
    // The nine small columns go through ONE pinned staging buffer: copies from pageable memory are staged
    // by the runtime one call at a time (~40 us each with the gaps between them, ~0.4 ms per batch).
    const size_t sizes[9] = {n * 4, n * 4, n * 4, n * 4, n, n, n, (2 * n + 1) * 4, nb};
    size_t off[10];
    off[0] = 0;
    for (int k = 0; k < 9; k++) off[k + 1] = (off[k] + sizes[k] + 63) & ~(size_t)63;
    // (an earlier batch's copies out of the buffer are usually long done -- every entry point but uz_phase_begin ends with a stream sync)
    if (c->dn_stage_done) UZ_HIP(hipEventSynchronize(c->dn_stage_done));
    if (c->dn_stage_cap < off[9]) {
        if (c->dn_stage) (void)hipHostFree(c->dn_stage);
        c->dn_stage = nullptr;
        c->dn_stage_cap = off[9] + off[9] / 4 + 4096;
        UZ_HIP(hipHostMalloc((void **)&c->dn_stage, c->dn_stage_cap, hipHostMallocDefault));
    }
    const void *src[9] = {d->contig, d->rcontig, d->start, d->end, d->vartype, d->dflags, d->mult, d->allele_off, d->alleles};
    for (int k = 0; k < 9; k++)
        if (sizes[k]) memcpy(c->dn_stage + off[k], src[k], sizes[k]);
    c->dn.block.ensure(off[9] + 64);
    uint8_t *const b = c->dn.block.p;
    c->dn.contig.p = (int32_t *)(b + off[0]); c->dn.rcontig.p = (int32_t *)(b + off[1]); c->dn.start.p = (int32_t *)(b + off[2]);
    c->dn.end.p = (int32_t *)(b + off[3]); c->dn.vartype.p = b + off[4]; c->dn.dflags.p = b + off[5]; c->dn.mult.p = b + off[6];
    c->dn.allele_off.p = (uint32_t *)(b + off[7]); c->dn.alleles.p = b + off[8];
    if (off[9]) uz_kcopy(c, b, c->dn_stage, off[9]); // out of the pinned staging buffer, by ONE kernel (the offsets are multiples of 64)
    if (!c->dn_stage_done) UZ_HIP(hipEventCreateWithFlags(&c->dn_stage_done, hipEventDisableTiming));
    UZ_HIP(hipEventRecord(c->dn_stage_done, c->stream));
    c->dn.cutoff = d->cutoff;
}

// ---------------------------------------------------------------- window lists of the last finds (uz_ctx.hpp: find_key, find_alt)
static FindKey find_key_of(const uz_ctx *c, int fam_id, int mode, const uz_dnms_view *d) {
    FindKey k;
    k.valid = d != nullptr && d->n >= 0;
    k.fam = fam_id; k.mode = mode; k.n = d ? d->n : -1; k.cohort = c->cohort_on;
    k.P = c->P;
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    // (four chains side by side over 32-byte steps, folded at the end of every column: one multiply chain over the 1.4 MB of a 100 k-DNM batch was
    // 0.21 ms of every read-stage call with the device idle; this is 0.04)
    auto mix = [&](const void *p, size_t bytes) {
        if (!p) return;
        const uint8_t *b = (const uint8_t *)p;
        uint64_t a0 = h ^ 0x243F6A8885A308D3ULL, a1 = h ^ 0x13198A2E03707344ULL, a2 = h ^ 0xA4093822299F31D0ULL, a3 = h ^ 0x082EFA98EC4E6C89ULL;
        size_t i = 0;
        for (; i + 32 <= bytes; i += 32) {
            uint64_t w[4];
            memcpy(w, b + i, 32);
            a0 = (a0 ^ w[0]) * 0x100000001B3ULL; a0 ^= a0 >> 29;
            a1 = (a1 ^ w[1]) * 0x100000001B3ULL; a1 ^= a1 >> 29;
            a2 = (a2 ^ w[2]) * 0x100000001B3ULL; a2 ^= a2 >> 29;
            a3 = (a3 ^ w[3]) * 0x100000001B3ULL; a3 ^= a3 >> 29;
        }
        h = (((a0 * 0x9E3779B97F4A7C15ULL) ^ a1) * 0x9E3779B97F4A7C15ULL ^ a2) * 0x9E3779B97F4A7C15ULL ^ a3;
        for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x100000001B3ULL; h ^= h >> 29; }
        for (; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ULL;
    };
    if (k.valid && d->n > 0) {
        const size_t n = (size_t)d->n;
        mix(d->contig, n * 4); mix(d->start, n * 4); mix(d->end, n * 4); mix(d->vartype, n); mix(d->mult, n);
    }
    k.hash = h;
    return k;
}
static bool find_key_eq(const FindKey &a, const FindKey &b) {
    return a.valid && b.valid && a.fam == b.fam && a.mode == b.mode && a.n == b.n && a.cohort == b.cohort && a.hash == b.hash &&
           memcmp(&a.P, &b.P, sizeof(uz_params)) == 0;
}
static void find_swap(uz_ctx *c, int which) { // a parked set becomes the context's, and the other way round (pointers only)
    FindSlot &a = c->find_alt[which];
    std::swap(c->cnt_c, a.cnt_c); std::swap(c->cnt_h, a.cnt_h); std::swap(c->win_range, a.win_range);
    std::swap(c->cand_off, a.cand_off); std::swap(c->het_off, a.het_off);
    std::swap(c->cand_idx, a.cand_idx); std::swap(c->het_idx, a.het_idx); std::swap(c->cand_flags, a.cand_flags);
    std::swap(c->n_cand, a.n_cand); std::swap(c->n_het, a.n_het);
    c->cand_off_h.swap(a.cand_off_h); c->het_off_h.swap(a.het_off_h);
    std::swap(c->find_key, a.key); std::swap(c->find_stamp, a.stamp);
}
// a new find overwrites the OLDEST set, or one that holds nothing (kernels still reading it are ahead of the new ones on the stream)
static void find_target(uz_ctx *c) {
    if (c->find_key.valid) {
        int best = -1;
        unsigned long long best_stamp = c->find_stamp;
        for (int k = 0; k < UZ_FIND_ALTS; k++) {
            const FindSlot &a = c->find_alt[k];
            if (!a.key.valid) { best = k; break; }
            if (a.stamp < best_stamp) { best = k; best_stamp = a.stamp; }
        }
        if (best >= 0) find_swap(c, best);
    }
    c->find_key.valid = false;
    c->find_valid = false;
}
static void find_done(uz_ctx *c, const FindKey &k) { c->find_key = k; c->find_stamp = ++c->find_counter; }
// the context's lists become those of batch `k` if one of the sets holds them; false: they must be computed
static bool find_recall(uz_ctx *c, const FindKey &k) {
    if (find_key_eq(c->find_key, k)) { c->find_valid = true; c->find_mode = k.mode; return true; }
    for (int a = 0; a < UZ_FIND_ALTS; a++)
        if (find_key_eq(c->find_alt[a].key, k)) { find_swap(c, a); c->find_valid = true; c->find_mode = k.mode; return true; }
    return false;
}
void find_forget(uz_ctx *c, int fam_id /* -1: everything */) {
    if (fam_id < 0 || c->find_key.fam == fam_id) { c->find_key.valid = false; c->find_valid = false; }
    for (int a = 0; a < UZ_FIND_ALTS; a++)
        if (fam_id < 0 || c->find_alt[a].key.fam == fam_id) c->find_alt[a].key.valid = false;
}

extern "C" {

int uz_create(int device, uz_ctx **out) {
    if (!out) return UZ_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UZ_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return UZ_E_HIP;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return UZ_E_NODEVICE; // code objects are gfx950 only
    uz_ctx *c = new uz_ctx();
    c->device = device;
    memset(&c->P, 0, sizeof(c->P));
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&c->hflags, 64, hipHostMallocMapped) != hipSuccess) {
        delete c;
        return UZ_E_HIP;
    }
    memset(c->hflags, 0, 64);
    *out = c;
    return 0;
}

void uz_destroy(uz_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    uz_prof_drain(c);
    uz_phase_state_free(c);
    for (auto &f : c->fams) if (f.live) free_family(c, f);
    for (auto &m : c->samples) if (m.live) free_samples(c, m);
    c->trio_idx.release();
    for (int b = 0; b < 2; b++) if (c->vcf_pin[b]) (void)hipHostFree(c->vcf_pin[b]);
    for (auto &s : c->sites) if (s.live) free_sites(c, s);
    for (auto &r : c->reads) if (r.live) free_reads(c, r);
    for (auto &b : c->block_pool) (void)hipFree(b.p);
    if (c->hflags) (void)hipHostFree(c->hflags);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->build_stream) (void)hipStreamDestroy(c->build_stream);
    c->dn.block.release();
    if (c->dn_stage_done) (void)hipEventDestroy(c->dn_stage_done);
    if (c->dn_stage) (void)hipHostFree(c->dn_stage);
    c->find_pin.release(); c->nm_pin.release(); c->bed_pin.release();
    c->bed_in.release(); c->bed_hook.release(); c->bed_out.release(); c->bed_len.release(); c->bed_off.release();
    c->vo.release(); c->bo.release(); c->df.release(); c->df_slots.release(); c->df_tokens.release();
    c->tbx_rows.release(); c->tbx_chunk.release(); c->tbx_work.release(); c->tbx_tab.release(); c->tbx_pin.release();
    c->nm_ids.release(); c->nm_len.release(); c->nm_off.release(); c->nm_out.release(); c->rf_first.release(); c->rf_mm.release();
    c->ab_lut.release(); c->win_range.release();
    c->dn_fam.release(); c->dn_cutoff.release(); c->fam_cls.release();
    c->cnv_counts.release(); c->cnv_pos.release(); c->cnv_origin.release(); c->cnv_evidence.release(); c->cnv_etype.release(); c->cnv_rb.release(); c->cnv_off.release(); c->cnv_dense.release();
    c->cnt_c.release(); c->cnt_h.release(); c->cand_off.release(); c->het_off.release();
    c->cand_idx.release(); c->het_idx.release(); c->cand_flags.release(); c->win_range.release();
    c->inf_comp.release(); c->inf_out.release(); c->inf_in.release(); c->inf_off.release(); c->inf_flags.release();
    if (c->inf_stream) (void)hipStreamDestroy(c->inf_stream);
    if (c->inf_stream2) (void)hipStreamDestroy(c->inf_stream2);
    if (c->inf_ready) (void)hipEventDestroy(c->inf_ready);
    for (auto &w : c->walk) {
        if (w.s0) (void)hipStreamDestroy(w.s0);
        if (w.s1) (void)hipStreamDestroy(w.s1);
        if (w.ev) (void)hipEventDestroy(w.ev);
#define UZ_X(T, name) w.name.release();
        UZ_WALK_BUFS(UZ_X)
#undef UZ_X
#define UZ_X(T, name) w.join.name.release();
        UZ_JOIN_BUFS(UZ_X)
#undef UZ_X
    }
    for (void *b : c->book.take_parked()) (void)hipFree(b);
    for (auto &h : c->heads) { h.tlen.release(); h.first_d.release(); }
    c->hd_comp.release(); c->hd_out.release(); c->hd_i64.release(); c->hd_i32.release(); c->hd_u32.release();
    for (FindSlot &a : c->find_alt) {
        a.cnt_c.release(); a.cnt_h.release(); a.win_range.release(); a.cand_off.release(); a.het_off.release();
        a.cand_idx.release(); a.het_idx.release(); a.cand_flags.release();
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *uz_last_error(const uz_ctx *c) {
    if (!c) return "null context";
    static thread_local std::string mine; // valid until this thread's next uz_last_error
    {
        std::lock_guard<std::mutex> lk(const_cast<uz_ctx *>(c)->err_mu);
        mine = c->err;
    }
    return mine.c_str();
}

int uz_sync(uz_ctx *c) {
    return guarded(c, [&] { UZ_HIP(hipStreamSynchronize(c->stream)); });
}

int uz_set_params(uz_ctx *c, const uz_params *p) {
    return guarded(c, [&] {
        UZ_REQUIRE(p != nullptr, UZ_E_ARG, "null params");
        c->P = *p;
    });
}

} // extern "C"

// ---- alignment records -> HBM ---------------------------------------------------------------------------
// Layout of a table's block: [record headers | flag word | QC word | coarse + mid search index | contig tables] then, for
// uploads, [cigar | seq4 | qlow] (+ the full qualities of an ASCII upload) and the staged fixed-width columns
// the headers are built from.
static void carve_common(Carver &cv, ReadsDev &r) {
    const size_t n = (size_t)r.n;
    r.rec_a = cv.take<uint8_t>(n * 16);
    r.rec_b = cv.take<uint8_t>(n * 16);
    r.fm = cv.take<uint32_t>(n);
    r.qoff = cv.take<uint32_t>(n);
    r.nlow = cv.take<uint8_t>(n);
    r.umask = cv.take<uint16_t>(n);
    r.qs = cv.take<uint16_t>(n);
    r.coarse = cv.take<int32_t>((n >> 12) + 2);
    r.mid = cv.take<int32_t>((n >> 6) + 2);
    r.mid8 = cv.take<int32_t>((n >> 3) + 16); // (read eight entries at a time: uz_mid8_refine)
    r.contig_off = cv.take<int64_t>((size_t)r.n_contigs + 1);
    r.max_span = cv.take<int32_t>((size_t)r.n_contigs + 1);
}

static void check_packed_view(const uz_reads_packed_view *v) {
    UZ_REQUIRE(v->n_segs >= 0 && v->n_segs < (int64_t)0x7FFFFFF0, UZ_E_RANGE, "more than 2^31 alignment records");
    UZ_REQUIRE(v->n_contigs >= 0, UZ_E_ARG, "bad reads view");
    UZ_REQUIRE(v->n_cigar_total >= 0 && v->n_cigar_total < ((int64_t)1 << 32), UZ_E_RANGE, "more than 2^32 CIGAR operations");
    UZ_REQUIRE(v->n_row_units >= 0 && v->n_row_units < ((int64_t)1 << 32), UZ_E_RANGE, "more than 2^32 row units (2^37 bases)");
    UZ_REQUIRE(v->n_seq_units >= 0 && v->n_seq_units <= v->n_row_units, UZ_E_ARG, "n_seq_units must lie in [0, n_row_units]");
    UZ_REQUIRE(!(v->seq2 && v->seq4), UZ_E_ARG, "a packed table has four-bit (seq4) OR two-bit (seq2) base rows, not both");
    UZ_REQUIRE(v->n_seq_units == 0 || v->seq2 || v->seq4, UZ_E_ARG, "n_seq_units > 0 but neither seq4 nor seq2 is set");
    if (v->seq2) UZ_REQUIRE(v->n_exc >= 0 && (v->n_exc == 0 || (v->exc_rec && v->exc_pos && v->exc_code)), UZ_E_ARG, "bad exc_* columns");
    UZ_REQUIRE(!(v->qlow && v->n_low), UZ_E_ARG, "a packed table has the quality plane (qlow) OR its list form (n_low / qlow_pos), not both");
    const bool v_dict = v->tup != nullptr || v->tup8 != nullptr;
    const bool v_lists = v->n_low != nullptr || (v_dict && v->tup_n_low);
    UZ_REQUIRE(v->n_segs == 0 || v->qlow || v_lists, UZ_E_ARG, "neither qlow nor n_low is set");
    UZ_REQUIRE(!(v->qlow && v_lists), UZ_E_ARG, "a packed table has the quality plane (qlow) OR its list form, not both");
    if (v_lists) UZ_REQUIRE(v->n_qlow_pos >= 0 && (v->n_qlow_pos == 0 || v->qlow_pos), UZ_E_ARG, "bad qlow_pos column");
    UZ_REQUIRE(!(v->umask || v->tup_umask) || v_lists, UZ_E_ARG, "umask (staged units) needs the list form of the qualities (n_low / qlow_pos)");
    UZ_REQUIRE(!v->tup_umask || (v_dict && !v->umask), UZ_E_ARG, "tup_umask needs tup, and umask NULL");
    if (v->start_d || v->start_d8) {
        UZ_REQUIRE(!(v->start_d && v->start_d8), UZ_E_ARG, "start_d and start_d8 are both set");
        const bool n8 = v->mate_d8 != nullptr || v->qname_d8 != nullptr;
        UZ_REQUIRE(!n8 || (v->start_d8 && v->mate_d8 && v->qname_d8 && !v->mate_d && !v->qname_d), UZ_E_ARG, "mate_d8 and qname_d8 come together, with start_d8, instead of mate_d / qname_d");
        if (v->pair_d8)
            UZ_REQUIRE(v->start_d8 && !v->tlen_s && !v->mate_d && !v->qname_d && !n8, UZ_E_ARG, "pair_d8 comes with start_d8, instead of tlen_s / mate_d* / qname_d*");
        UZ_REQUIRE((v->pair_d8 || (v->tlen_s && (n8 || (v->mate_d && v->qname_d)))) && v->n_esc16 >= 0 && (v->n_esc16 == 0 || (v->esc16_key && v->esc16_val)), UZ_E_ARG, "bad 16-bit difference columns");
        UZ_REQUIRE(!v->start && !v->tlen && !v->mate && !v->qname, UZ_E_ARG, "start_d / start_d8 is set: start / tlen / mate / qname must be NULL");
    }
    if (v->tup8) { // the index in one byte: hot table, escape list, escapes in front of every span (ascending from 0 to the total)
        UZ_REQUIRE(!v->tup && v->tup_hot && v->tup_esc_off && v->n_tup_esc >= 0 && v->n_tup_esc <= v->n_segs && (v->n_tup_esc == 0 || v->tup_esc), UZ_E_ARG, "bad tup8 form");
        const int64_t nsp = (v->n_segs + UZ_TUP8_SPAN - 1) / UZ_TUP8_SPAN;
        UZ_REQUIRE(v->tup_esc_off[0] == 0 && (int64_t)v->tup_esc_off[nsp] == v->n_tup_esc, UZ_E_RANGE, "tup_esc_off does not run from 0 to n_tup_esc");
        for (int64_t b = 0; b < nsp; b++) UZ_REQUIRE(v->tup_esc_off[b] <= v->tup_esc_off[b + 1], UZ_E_RANGE, "tup_esc_off does not ascend");
    }
    if (v_dict) {
        UZ_REQUIRE(v->n_tup >= 1 && v->n_tup <= 65536 && v->tup_flag && v->tup_l_seq && v->tup_n_cigar && v->tup_mapq && v->tup_aux, UZ_E_ARG, "bad tup_* table");
        UZ_REQUIRE(!v->flag && !v->l_seq && !v->n_cigar && !v->mapq && !v->aux && !v->n_low, UZ_E_ARG, "tup is set: flag / l_seq / n_cigar / mapq / aux / n_low must be NULL");
    }
    if (v->bl_n || v->tup_n_bl) {
        UZ_REQUIRE(!(v->bl_n && v->tup_n_bl) && (!v->tup_n_bl || v_dict), UZ_E_ARG, "bl_n OR tup_n_bl (the latter with tup)");
        UZ_REQUIRE((v->umask || v->tup_umask) && v_lists && (v->seq2 || v->n_seq_units == 0) && !v->seq4, UZ_E_ARG,
                   "the list form of the bases (bl_*) needs unit masks, the list form of the qualities and two-bit rows");
        UZ_REQUIRE(v->n_bl >= 0 && v->n_bl_units >= 0 && v->n_bl_units <= v->n_bl && (v->n_bl == 0 || (v->bl_pos && v->bl_code)), UZ_E_ARG, "bad bl_* columns");
        UZ_REQUIRE(v->n_seq_units + v->n_bl_units <= v->n_row_units, UZ_E_ARG, "n_seq_units + n_bl_units must not exceed n_row_units");
        // the quality bits of the listed bases: with the lists themselves, the counts through the dictionary (never beside the plane: the list
        // form of the bases has been held to the list form of the qualities above)
        UZ_REQUIRE(!v->bl_qlow || (v->bl_pos && v->bl_code && !v->bl_n), UZ_E_ARG, "bl_qlow needs bl_pos / bl_code and tup_n_bl, not bl_n");
    } else {
        UZ_REQUIRE(v->n_bl == 0 && v->n_bl_units == 0, UZ_E_ARG, "n_bl / n_bl_units without bl_n / tup_n_bl");
        UZ_REQUIRE(!v->bl_qlow, UZ_E_ARG, "bl_qlow without the list form of the bases (tup_n_bl, bl_pos, bl_code)");
    }
    UZ_REQUIRE(v->cigar_compact ? v->n_cigar_omitted >= 0 && v->n_cigar_omitted <= v->n_segs : v->n_cigar_omitted == 0, UZ_E_ARG, "bad n_cigar_omitted");
    UZ_REQUIRE(v->n_cigar_total + v->n_cigar_omitted < ((int64_t)1 << 32), UZ_E_RANGE, "more than 2^32 CIGAR operations");
    if (v->pk_sums) { // the packer's span sums: rows that ascend from zero to the totals the view declares (the device holds every span against its row)
        const int shift = UZ_PK_SHIFT(v->n_segs);
        const int64_t nb = (v->n_segs + ((int64_t)1 << shift) - 1) >> shift;
        UZ_REQUIRE(v->n_pk_spans == nb, UZ_E_ARG, "pk_sums: n_pk_spans is not the number of spans of n_segs records (UZ_PK_SHIFT)");
        const uint64_t *S = v->pk_sums, *T = S + (size_t)nb * UZ_PK_SUMS;
        bool ok = true;
        for (int k = 0; k < UZ_PK_SUMS; k++) ok &= S[k] == 0;
        for (int64_t b = 0; b < nb && ok; b++)
            for (int k = 0; k < UZ_PK_SUMS; k++)
                if (k != 5 && k != 6) ok &= S[(size_t)(b + 1) * UZ_PK_SUMS + k] >= S[(size_t)b * UZ_PK_SUMS + k];
        const bool lists_f = v->n_low != nullptr || (v_dict && v->tup_n_low);
        ok = ok && T[0] == (uint64_t)(v->n_cigar_total + v->n_cigar_omitted) && T[1] == (uint64_t)v->n_row_units && T[2] == (uint64_t)v->n_seq_units &&
             T[3] == (uint64_t)(lists_f ? v->n_qlow_pos : 0) && (!v->cigar_compact || T[4] == (uint64_t)v->n_cigar_total) && T[7] == (uint64_t)v->n_bl_units &&
             T[8] == (uint64_t)v->n_bl && T[9] == T[10];
        UZ_REQUIRE(ok, UZ_E_RANGE, "pk_sums: the span sums do not ascend from zero to the totals the view declares");
    }
}

// The columns of a table's block, each named ONCE by a staging routine that runs its body three times: pass 0 sizes the block, pass 1 plans
// the slab copy (h2d only looks at the host addresses), pass 2 places the columns and copies them (or points into the slab's image)
struct Stager {
    hipStream_t st;
    int pass;
    Carver cv;
    template <typename T>
    T *own(size_t n) { return cv.take<T>(n); } // an area that only the device writes
    template <typename T>
    const T *col(const T *host, size_t n, size_t room = 0) { // a column off the link (room: elements kept free behind it)
        T *d = cv.take<T>(n + room);
        return pass ? h2d(st, d, host, n) : d;
    }
};

// packed columns in HOST memory -> one block; every command goes to stream `st`.  The header build is left to the caller: r.cols and
// r.build_scratch are what uz_build_records takes
static void reads_from_packed_host(uz_ctx *c, hipStream_t st, const uz_reads_packed_view *v, ReadsDev &r) {
    check_packed_view(v);
    r.live = true;
    r.n = v->n_segs; r.n_contigs = v->n_contigs; r.n_qnames = v->n_qnames;
    r.n_cigar_total = v->n_cigar_total + v->n_cigar_omitted; // the device's store holds every record's words
    const bool blf = v->bl_n != nullptr || v->tup_n_bl != nullptr; // bases of some records as lists: their units exist on the device only, behind the rows that travelled
    r.n_bl = blf ? v->n_bl : 0; r.n_bl_units = blf ? v->n_bl_units : 0;
    r.n_row_units = v->n_row_units; r.n_seq_units = v->n_seq_units + r.n_bl_units;
    r.n_cigar_staged = v->n_cigar_total;
    const bool ccompact = v->cigar_compact != 0;
    const size_t n = (size_t)r.n, nc = (size_t)r.n_cigar_total, nu = (size_t)r.n_row_units, ns = (size_t)r.n_seq_units, ncs = (size_t)v->n_cigar_total;
    const size_t nsl = (size_t)v->n_seq_units; // units on the link
    const size_t nbl = (size_t)r.n_bl, nblp = nbl * (v->bl_wide ? 2 : 1), nblc = (nbl + 3) / 4, nblq = (nbl + 7) / 8;
    const bool two_bit = v->seq2 != nullptr;
    const size_t ne = two_bit ? (size_t)v->n_exc : 0;
    const bool t8 = v->tup8 != nullptr; // the dictionary index in one byte: rebuilt into the 16-bit column's place by the header build's first kernel
    const bool tupf = v->tup != nullptr || t8;
    const bool lists = v->n_low != nullptr || (tupf && v->tup_n_low); // quality rows only for the records with bases (at their base-row position), written by the header build
    const size_t nt = tupf ? (size_t)v->n_tup : 0;
    const size_t nte = t8 ? (size_t)v->n_tup_esc : 0, ntsp = t8 ? ((size_t)v->n_segs + UZ_TUP8_SPAN - 1) / UZ_TUP8_SPAN + 1 : 0;
    const size_t nql = lists ? (size_t)v->n_qlow_pos * (v->qlow_pos_wide ? 2 : 1) : 0;
    r.n_qlow_pos = lists ? v->n_qlow_pos : 0;
    r.n_plane_units = lists ? r.n_seq_units : v->n_row_units;
    const bool d8 = v->start_d8 != nullptr;
    const bool d16 = v->start_d != nullptr || d8;
    const size_t nes = d16 ? (size_t)v->n_esc16 : 0;
    const size_t npk = v->pk_sums ? ((size_t)v->n_pk_spans + 1) * UZ_PK_SUMS : 0; // the packer's span sums (checked by check_packed_view)
    RecColumns col;
    SlabPlan plan;
    SlabScope slab_scope(&plan);
    for (int pass = 0; pass < 3; pass++) {
        if (pass == 2) slab_commit(c, st, plan, r.mirror);
        Stager S{st, pass, Carver(pass ? r.block.p : nullptr)};
        col = RecColumns();
        carve_common(S.cv, r);
        if (pass) {
            r.contig_off = const_cast<int64_t *>(h2d(st, r.contig_off, v->contig_off, (size_t)v->n_contigs + 1));
            r.max_span = const_cast<int32_t *>(h2d(st, r.max_span, v->max_span, (size_t)v->n_contigs));
        }
        if (v->end) col.end = S.col(v->end, n);
        if (npk) col.pk_sums = S.col((const unsigned long long *)v->pk_sums, npk);
        if (d16) { // 16-bit differences + the escape list instead of four 32-bit columns
            if (d8) col.start_d8 = S.col(v->start_d8, n);
            else col.start_d = S.col(v->start_d, n);
            if (v->pair_d8) col.pair_d8 = S.col(v->pair_d8, n);
            else {
                col.tlen_s = S.col(v->tlen_s, n);
                if (v->mate_d8) { col.mate_d8 = S.col(v->mate_d8, n); col.qname_d8 = S.col(v->qname_d8, n); }
                else { col.mate_d = S.col(v->mate_d, n); col.qname_d = S.col(v->qname_d, n); }
            }
            col.esc16_key = S.col((const unsigned long long *)v->esc16_key, nes); col.esc16_val = S.col(v->esc16_val, nes);
            col.n_esc16 = (int64_t)nes;
        } else {
            col.start = S.col(v->start, n); col.tlen = S.col(v->tlen, n);
            col.mate = S.col(v->mate, n); col.qname = S.col(v->qname, n);
        }
        if (tupf) { // a 16-bit index per record + the table of combinations instead of nine bytes of small columns
            if (t8) {
                col.tup8 = S.col(v->tup8, n); col.tup_hot = S.col(v->tup_hot, (size_t)256);
                col.tup_esc = S.col(v->tup_esc, nte); col.tup_esc_off = S.col(v->tup_esc_off, ntsp);
                col.n_tup_esc = (int64_t)nte;
                col.tup_out = S.own<uint16_t>(n); col.tup = col.tup_out; // (k_tup_expand writes it before anything reads it)
            } else
                col.tup = S.col(v->tup, n);
            col.n_tup = (int64_t)nt;
            col.tup_flag = S.col(v->tup_flag, nt); col.tup_l_seq = S.col(v->tup_l_seq, nt); col.tup_n_cigar = S.col(v->tup_n_cigar, nt);
            col.tup_mapq = S.col(v->tup_mapq, nt); col.tup_aux = S.col(v->tup_aux, nt);
            if (v->tup_n_low) col.tup_n_low = S.col(v->tup_n_low, nt);
            if (v->tup_umask) col.tup_umask = S.col(v->tup_umask, nt);
            if (v->tup_n_bl) col.tup_n_bl = S.col(v->tup_n_bl, nt);
        } else {
            col.flag = S.col(v->flag, n);
            col.l_seq = S.col(v->l_seq, n); col.n_cigar = S.col(v->n_cigar, n);
            col.mapq = S.col(v->mapq, n); col.aux = S.col(v->aux, n);
        }
        col.lists = lists ? 1 : 0;
        if (ccompact) { // the travelled words land in a staging area; the header build writes the store
            col.cigar_out = S.own<uint32_t>(nc);
            col.cigar_staged = S.col(v->cigar, ncs);
            r.cigar = col.cigar_out;
        } else
            r.cigar = S.col(v->cigar, nc);
        col.cigar_in = r.cigar;
        if (two_bit) { // half the bytes over the link; the header build expands them into seq4
            r.seq4 = S.own<uint8_t>(ns * UZ_SEQ4_UNIT_BYTES);
            r.seq2_staged = S.col(v->seq2, nsl * UZ_SEQ2_UNIT_BYTES);
            r.n_exc = (int64_t)ne;
            r.exc_rec = S.col(v->exc_rec, ne); r.exc_pos = S.col(v->exc_pos, ne); r.exc_code = S.col(v->exc_code, ne);
        } else
            r.seq4 = S.col(v->seq4, ns * UZ_SEQ4_UNIT_BYTES);
        if (blf) {
            if (v->bl_n) col.bl_n = S.col(v->bl_n, n);
            col.bl_pos = S.col(v->bl_pos, nblp); col.bl_code = S.col(v->bl_code, nblc, 4);
            if (v->bl_qlow) col.bl_qlow = S.col(v->bl_qlow, nblq, 8);
            col.bl_wide = v->bl_wide;
            col.n_seq_link = (int64_t)nsl;
            col.seq4_out = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(r.seq4));
        }
        if (lists) {
            r.qlow = S.own<uint8_t>(ns * UZ_QLOW_UNIT_BYTES);
            if (!tupf) col.n_low = S.col(v->n_low, n);
            col.qlow_pos = S.col(v->qlow_pos, nql);
            col.qpos_wide = v->qlow_pos_wide;
            if (v->umask) col.umask = S.col(v->umask, n);
        } else {
            r.qlow = const_cast<uint8_t *>(S.col(v->qlow, nu * UZ_QLOW_UNIT_BYTES));
            col.plane_in = reinterpret_cast<const uint32_t *>(r.qlow);
        }
        r.build_scratch = S.own<uint8_t>(uz_rec_scratch_bytes(r.n));
        if (!pass) r.block = uz_block_get(c, S.cv.off + 256);
    }
    r.qlow_thr = v->min_base_qual;
    r.qlow_valid = true;
    r.cols = col;
}

void uz_reads_make_ready(uz_ctx *c, ReadsDev &r) {
    if (!r.pending) return;
    if (r.built) UZ_HIP(hipStreamWaitEvent(c->stream, r.built, 0)); // built beside whatever the compute stream was doing
    else { // no build queued with the upload (UZ_BUILD_LAZY): from the staged columns the upload left in the table's block
        UZ_HIP(hipStreamWaitEvent(c->stream, r.ready, 0));
        uz_build_records(c, c->stream, r, r.cols, r.build_scratch);
    }
    r.pending = false;
}

void uz_reads_ready_for_threshold(uz_ctx *c, ReadsDev &r, const char *what) {
    uz_reads_make_ready(c, r);
    if (r.qlow_valid && r.qlow_thr == c->P.min_gt_qual) return;
    UZ_REQUIRE(r.qual8 != nullptr, UZ_E_STATE,
               std::string(what) + " was packed for --min-gt-qual " + std::to_string(r.qlow_thr) + ", the parameters say " +
                   std::to_string(c->P.min_gt_qual) + ": decode it again for this threshold");
    uz_build_qlow(c, c->stream, r, c->P.min_gt_qual);
}

int uz_reads_upload_impl(uz_ctx *c, const uz_reads_view *v, ReadsDev &r) {
    // the ASCII form (uz_reads_view): the fixed-width columns are staged as they are, the CIGAR words and
    // the bases are re-laid in the packed geometry on the device, the qualities are kept for the plane
    UZ_REQUIRE(v->n_segs >= 0 && v->n_segs < (int64_t)0x7FFFFFF0, UZ_E_RANGE, "more than 2^31 alignment records");
    hipStream_t st = c->stream;
    r.live = true;
    r.n = v->n_segs; r.n_contigs = v->n_contigs; r.n_qnames = v->n_qnames;
    const size_t n = (size_t)r.n;
    // totals of the packed geometry from the host columns
    int64_t tot_c = 0, tot_u = 0;
    for (size_t i = 0; i < n; i++) { tot_c += v->n_cigar[i]; tot_u += UZ_ROW_UNITS(v->l_seq[i]); }
    r.n_cigar_total = tot_c; r.n_row_units = tot_u; r.n_seq_units = tot_u; // the ASCII form carries every record's bases
    r.n_plane_units = tot_u;
    UZ_REQUIRE(tot_c < ((int64_t)1 << 32) && tot_u < ((int64_t)1 << 32), UZ_E_RANGE, "table exceeds the 32-bit CIGAR / row offsets");
    const size_t nc = (size_t)tot_c, nu = (size_t)tot_u, nci = (size_t)v->n_cigar_total, nsq = (size_t)v->n_sq_bytes;
    uint32_t *cigar = nullptr, *cigar_in = nullptr, *cigar_off_in = nullptr; uint8_t *seq4 = nullptr, *qlow = nullptr, *seq_in = nullptr;
    int32_t *start, *end, *tlen, *mate; uint32_t *qname; uint16_t *flag, *l_seq, *n_cigar; uint8_t *mapq, *aux;
    void *scratch = nullptr;
    r.block = uz_carve(c, [&](Carver &cv) {
        carve_common(cv, r);
        cigar = cv.take<uint32_t>(nc);
        seq4 = cv.take<uint8_t>(nu * UZ_SEQ4_UNIT_BYTES);
        qlow = cv.take<uint8_t>(nu * UZ_QLOW_UNIT_BYTES);
        r.qual8 = cv.take<uint8_t>(nsq);
        r.qual_off16 = cv.take<uint32_t>(n);
        start = cv.take<int32_t>(n); end = cv.take<int32_t>(n); tlen = cv.take<int32_t>(n); mate = cv.take<int32_t>(n);
        qname = cv.take<uint32_t>(n); flag = cv.take<uint16_t>(n); l_seq = cv.take<uint16_t>(n); n_cigar = cv.take<uint16_t>(n);
        mapq = cv.take<uint8_t>(n); aux = cv.take<uint8_t>(n);
        cigar_in = cv.take<uint32_t>(nci); cigar_off_in = cv.take<uint32_t>(n); seq_in = cv.take<uint8_t>(nsq);
        scratch = cv.take<uint8_t>(uz_rec_scratch_bytes(r.n));
    });
    h2d(st, r.contig_off, v->contig_off, (size_t)v->n_contigs + 1);
    h2d(st, r.max_span, v->max_span, (size_t)v->n_contigs);
    RecColumns col;
    col.start = h2d(st, start, v->start, n); col.end = h2d(st, end, v->end, n); col.tlen = h2d(st, tlen, v->tlen, n);
    col.mate = h2d(st, mate, v->mate, n); col.qname = h2d(st, qname, v->qname, n); col.flag = h2d(st, flag, v->flag, n);
    col.l_seq = h2d(st, l_seq, v->l_seq, n); col.n_cigar = h2d(st, n_cigar, v->n_cigar, n);
    col.mapq = h2d(st, mapq, v->mapq, n); col.aux = h2d(st, aux, v->aux, n);
    h2d(st, cigar_in, v->cigar, nci); h2d(st, cigar_off_in, v->cigar_off, n);
    h2d(st, seq_in, v->seq, nsq); h2d(st, r.qual8, v->qual, nsq); h2d(st, r.qual_off16, v->sq_off16, n);
    r.cigar = cigar; r.seq4 = seq4; r.qlow = qlow;
    r.qlow_valid = false; // built for the threshold of the first uz_phase
    uz_build_records(c, st, r, col, scratch);
    uz_pack_ascii_rows(c, st, r, cigar_in, cigar_off_in, seq_in, r.qual_off16, cigar, seq4);
    UZ_HIP(hipStreamSynchronize(st));
    uz_check_upload_flag(c);
    return 0;
}

// A table over packed columns that lie in DEVICE memory: cigar, seq4 and the quality plane stay where they are and ARE the device's stores, the
// headers and the index are built into a block of the library's own (two-bit rows and the list form of the plane are expanded there).  None
// of the caller's other pointers is kept.  -> the table's id
static int adopt_device(uz_ctx *c, const uz_reads_packed_view *v) {
    check_packed_view(v);
    UZ_REQUIRE(!v->cigar_compact, UZ_E_ARG, "uz_reads_adopt_device takes every CIGAR word (cigar_compact = 0): the caller's column IS the device's store");
    UZ_REQUIRE(!v->bl_n && !v->tup_n_bl, UZ_E_ARG, "uz_reads_adopt_device takes base rows: the list form of the bases (bl_*) is a form of the host link");
    UZ_REQUIRE(!v->tup8, UZ_E_ARG, "uz_reads_adopt_device takes the 16-bit dictionary index: the one-byte form (tup8) is a form of the host link");
    UZ_REQUIRE(((uintptr_t)v->qlow | (uintptr_t)v->seq4 | (uintptr_t)v->seq2 | (uintptr_t)v->cigar) % 16 == 0, UZ_E_ARG, "device columns must be 16-byte aligned");
    ReadsDev r;
    r.live = true;
    r.n = v->n_segs; r.n_contigs = v->n_contigs; r.n_qnames = v->n_qnames;
    r.n_cigar_total = v->n_cigar_total; r.n_row_units = v->n_row_units; r.n_seq_units = v->n_seq_units;
    void *scratch = nullptr;
    uint8_t *seq4_own = nullptr; // two-bit rows are expanded into the library's own block
    uint8_t *qlow_own = nullptr; // the list form of the quality plane likewise
    const bool a_lists = v->n_low != nullptr || (v->tup && v->tup_n_low);
    r.n_qlow_pos = a_lists ? v->n_qlow_pos : 0;
    r.n_plane_units = a_lists ? v->n_seq_units : v->n_row_units;
    r.block = uz_carve(c, [&](Carver &cv) {
        carve_common(cv, r);
        if (v->seq2) seq4_own = cv.take<uint8_t>((size_t)r.n_seq_units * UZ_SEQ4_UNIT_BYTES);
        if (a_lists) qlow_own = cv.take<uint8_t>((size_t)r.n_seq_units * UZ_QLOW_UNIT_BYTES);
        scratch = cv.take<uint8_t>(uz_rec_scratch_bytes(r.n));
    });
    try {
        hipStream_t st = c->stream;
        UZ_HIP(hipMemcpyAsync(r.contig_off, v->contig_off, ((size_t)v->n_contigs + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        if (v->n_contigs) UZ_HIP(hipMemcpyAsync(r.max_span, v->max_span, (size_t)v->n_contigs * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        RecColumns col;
        col.start = v->start; col.end = v->end; col.tlen = v->tlen; col.mate = v->mate; col.qname = v->qname;
        if (v->start_d || v->start_d8) {
            col.start_d = v->start_d; col.start_d8 = v->start_d8; col.tlen_s = v->tlen_s; col.mate_d = v->mate_d; col.qname_d = v->qname_d;
            col.mate_d8 = v->mate_d8; col.qname_d8 = v->qname_d8; col.pair_d8 = v->pair_d8;
            col.esc16_key = (const unsigned long long *)v->esc16_key; col.esc16_val = v->esc16_val; col.n_esc16 = v->n_esc16;
        }
        col.flag = v->flag; col.l_seq = v->l_seq; col.n_cigar = v->n_cigar; col.mapq = v->mapq; col.aux = v->aux;
        r.cigar = v->cigar; r.seq4 = v->seq4; r.qlow = const_cast<uint8_t *>(v->qlow);
        col.cigar_in = v->cigar;
        if (v->seq2) {
            r.seq4 = seq4_own; r.seq2_staged = v->seq2;
            r.n_exc = v->n_exc; r.exc_rec = v->exc_rec; r.exc_pos = v->exc_pos; r.exc_code = v->exc_code;
        }
        if (v->tup) {
            col.tup = v->tup; col.tup_flag = v->tup_flag; col.tup_l_seq = v->tup_l_seq; col.tup_n_cigar = v->tup_n_cigar;
            col.tup_mapq = v->tup_mapq; col.tup_aux = v->tup_aux; col.tup_n_low = v->tup_n_low; col.tup_umask = v->tup_umask; col.n_tup = v->n_tup;
        }
        if (a_lists) { r.qlow = qlow_own; col.lists = 1; col.n_low = v->n_low; col.qlow_pos = v->qlow_pos; col.qpos_wide = v->qlow_pos_wide; col.umask = v->umask; }
        else col.plane_in = reinterpret_cast<const uint32_t *>(v->qlow);
        r.qlow_thr = v->min_base_qual;
        r.qlow_valid = true;
        uz_build_records(c, st, r, col, scratch);
        UZ_HIP(hipStreamSynchronize(st));
        r.exc_rec = nullptr; r.exc_pos = nullptr; r.exc_code = nullptr; r.n_exc = 0; // (the caller's memory: not kept)
        uz_check_upload_flag(c);
    } catch (...) { uz_block_put(c, r.block); throw; }
    const int k = new_slot(c->reads);
    c->reads[k] = r;
    return k;
}

// ---- the device slots of walked batches (uz_ctx::WalkSlot; which are held: uz_ctx::book, csrc/walk_book.hpp)
// the slot of a batch that is held: the look-up of every entry point that takes a walk id
uz_ctx::WalkSlot &walk_slot(uz_ctx *c, int walk_id) {
    UZ_REQUIRE(walk_id >= 0 && walk_id < uz_ctx::WALK_SLOTS && c->book.held(walk_id), UZ_E_ARG, "bad walk id");
    return c->walk[walk_id];
}

// A claimed slot, given back unless it is handed on (dismiss).  drain: copies into the claimer's locals and kernels on the slot's buffers may
// still be queued -- nothing of the slot is handed on, and the claimer's frame is not left, before both of its streams have drained.
struct SlotClaim {
    uz_ctx *c;
    int k;
    bool drain;
    SlotClaim(uz_ctx *c_, int k_, bool drain_) : c(c_), k(k_), drain(drain_) {}
    SlotClaim(const SlotClaim &) = delete;
    SlotClaim &operator=(const SlotClaim &) = delete;
    void dismiss() { k = -1; }
    ~SlotClaim() {
        if (k < 0) return;
        if (drain) {
            uz_ctx::WalkSlot &w = c->walk[k];
            if (w.s0) (void)hipStreamSynchronize(w.s0);
            if (w.s1) (void)hipStreamSynchronize(w.s1);
            (void)hipGetLastError();
        }
        c->book.release(k);
    }
};

// what uz_bam_walk is given, as its steps pass it on
struct WalkPlan {
    const uint8_t *comp; int64_t comp_bytes, n_blocks; const int64_t *in_off, *out_off, *blk_coff; const uint32_t *blk_crc;
    int32_t n_tasks; const int32_t *task; int64_t n_spans; const int64_t *span; int64_t n_reach; const int32_t *reach; int64_t n_fetch; const int32_t *fetch;
    int64_t out_bytes() const { return n_blocks ? out_off[n_blocks] : 0; }
    // a batch over many files (uz_bam_walk_many): the per-file table, NULL for one file
    int32_t n_files = 0; const int64_t *file_base = nullptr; const int32_t *ref_base = nullptr; const uint64_t *salt1 = nullptr; const uint32_t *salt2 = nullptr;
};

// the file of every walk task (uz_bamwalk.h: uz_walk_file): the one its first gathered block lies in -- whose references must hold the task's
std::vector<uz_walk_file> task_files(const WalkPlan &p) {
    UZ_REQUIRE(p.n_files >= 1 && p.file_base && p.ref_base && p.salt1 && p.salt2, UZ_E_ARG, "uz_bam_walk_many: null file table");
    UZ_REQUIRE(p.file_base[0] == 0 && p.ref_base[0] == 0, UZ_E_ARG, "uz_bam_walk_many: file_base and ref_base start at 0");
    for (int32_t f = 0; f < p.n_files; f++)
        UZ_REQUIRE(p.file_base[f + 1] >= p.file_base[f] && p.ref_base[f + 1] >= p.ref_base[f], UZ_E_ARG, "uz_bam_walk_many: file_base and ref_base are running sums");
    std::vector<uz_walk_file> out((size_t)p.n_tasks);
    for (int32_t t = 0; t < p.n_tasks; t++) {
        const int32_t *tc = p.task + UZ_WALK_TASK_COLS * (size_t)t;
        int32_t f = -1;
        for (int32_t sp = tc[2]; sp < tc[3] && f < 0; sp++) {
            const int64_t *sc = p.span + UZ_WALK_SPAN_COLS * (size_t)sp;
            if (sc[4] < sc[5]) f = (int32_t)(std::upper_bound(p.file_base, p.file_base + p.n_files + 1, p.blk_coff[sc[4]]) - p.file_base) - 1;
        }
        if (f < 0) f = (int32_t)(std::upper_bound(p.ref_base, p.ref_base + p.n_files + 1, tc[0]) - p.ref_base) - 1; // (no block: nothing is walked)
        UZ_REQUIRE(f >= 0 && f < p.n_files && tc[0] >= p.ref_base[f] && tc[0] < p.ref_base[f + 1], UZ_E_ARG,
                   "uz_bam_walk_many: a task's first block lies in another file than its reference");
        out[(size_t)t] = uz_walk_file{p.salt1[f], p.ref_base[f], p.ref_base[f + 1] - p.ref_base[f], p.salt2[f], 0u};
    }
    return out;
}

void check_walk_plan(const WalkPlan &p) {
    UZ_REQUIRE(p.n_blocks >= 0 && p.comp_bytes >= 0 && p.n_tasks >= 0 && p.n_spans >= 0 && p.n_reach >= 0 && p.n_fetch >= 0, UZ_E_ARG, "bad arguments");
    UZ_REQUIRE(p.n_blocks == 0 || (p.comp && p.in_off && p.out_off && p.blk_coff), UZ_E_ARG, "null block table");
    UZ_REQUIRE(p.n_tasks == 0 || (p.task && p.span && p.reach && p.fetch), UZ_E_ARG, "null walk plan");
    const int64_t *out_off = p.out_off;
    UZ_REQUIRE(!uz_bgzf_check_tables(p.n_blocks, p.comp_bytes, p.in_off, out_off, true), UZ_E_ARG,
               "bad block table (blocks in the order they lie in `comp`; a BGZF block inflates to at most 64 KiB)");
    // the plan is the kernel's only guard: every index it names must lie inside the arrays it names
    for (int32_t t = 0; t < p.n_tasks; t++) {
        const int32_t *tc = p.task + UZ_WALK_TASK_COLS * (size_t)t;
        UZ_REQUIRE(tc[2] >= 0 && tc[2] <= tc[3] && tc[3] <= p.n_spans && tc[4] >= 0 && tc[4] <= tc[5] && tc[5] <= p.n_reach && tc[6] >= 0 && tc[6] <= tc[7] && tc[7] <= p.n_fetch,
                   UZ_E_ARG, "walk plan: a task names spans, reach intervals or fetches outside the arrays");
        // column 9: the stage task a walk task belongs to -- its sub-tasks adjacent and in order (the hash sets of k_tab_insert / k_desc_filter and
        // the joins find a stage task's first sub-task by walking back over equal values)
        UZ_REQUIRE(tc[9] >= 0 && (t == 0 ? true : (tc[9] == tc[9 - UZ_WALK_TASK_COLS] || tc[9] == tc[9 - UZ_WALK_TASK_COLS] + 1)), UZ_E_ARG,
                   "walk plan: column 9 (the stage task of a walk task) must start at or above 0 and go up by at most one from task to task");
    }
    for (int64_t k = 0; k < p.n_spans; k++) {
        const int64_t *sc = p.span + UZ_WALK_SPAN_COLS * (size_t)k;
        UZ_REQUIRE(sc[4] >= 0 && sc[4] <= sc[5] && sc[5] <= p.n_blocks && (sc[4] == sc[5] || (sc[2] >= out_off[sc[4]] && sc[2] <= sc[3] && sc[3] == out_off[sc[5]])),
                   UZ_E_ARG, "walk plan: a span names blocks or bytes outside the block table");
    }
}

// one pass: every task writes its descriptors into a slice sized for the most records its bytes can hold (a record is at least 36 bytes)
std::vector<int64_t> desc_slices(const WalkPlan &p) {
    std::vector<int64_t> first((size_t)p.n_tasks + 1, 0);
    for (int32_t t = 0; t < p.n_tasks; t++) {
        const int32_t *tc = p.task + UZ_WALK_TASK_COLS * (size_t)t;
        int64_t cap = 0;
        for (int32_t sp = tc[2]; sp < tc[3]; sp++) cap += (p.span[UZ_WALK_SPAN_COLS * (size_t)sp + 3] - p.span[UZ_WALK_SPAN_COLS * (size_t)sp + 2]) / 36 + 1;
        first[(size_t)t + 1] = first[(size_t)t] + cap;
    }
    return first;
}

// The batch's blocks up and inflated in slices on the slot's two streams (uz_queue_inflate), which the first then waits for: the walk reads what
// both inflated; then every block against the CRC-32 of its footer.  w.iflags: two words per slice, then the CRC's
void queue_blocks(uz_ctx *c, uz_ctx::WalkSlot &w, const WalkPlan &p, const std::vector<int64_t> &cut) {
    const int64_t n_blocks = p.n_blocks;
    const size_t ns = cut.size() - 1;
    hipStream_t st = w.s0;
    UZ_WGROW(w, iflags, 2 * ns + 8); UZ_WGROW(w, blk_crc, (size_t)n_blocks + 1);
    if (n_blocks == 0) return;
    UZ_HIP(hipMemsetAsync(w.out.p + p.out_bytes(), 0, uz_bam_walk_pad(), st));
    UZ_HIP(hipMemcpyAsync(w.blk_coff.p, p.blk_coff, (size_t)n_blocks * 8, hipMemcpyHostToDevice, st));
    uz_queue_inflate(c, InflateBatch{p.comp, p.comp_bytes, n_blocks, p.in_off, p.out_off, w.comp.p, w.in_off.p, w.out_off.p, w.out.p, w.iflags.p, {w.s0, w.s1}, w.ev}, cut);
    if (ns > 1) {
        UZ_HIP(hipEventRecord(w.ev, w.s1));
        UZ_HIP(hipStreamWaitEvent(st, w.ev, 0));
    }
    if (p.blk_crc) { // as htslib's reader (and the host's walk) holds it
        UZ_HIP(hipMemcpyAsync(w.blk_crc.p, p.blk_crc, (size_t)n_blocks * 4, hipMemcpyHostToDevice, st));
        uz_launch_crc32(c, st, n_blocks, w.out.p, w.out_off.p, w.blk_crc.p, w.iflags.p + 2 * ns);
    }
}

// the plan up, the walk, and the count of the descriptors the host's joins can need at all (direct, or sharing a name hash with a direct record of
// the task).  The two counts come down by copies on the slot's stream: they belong to the caller, whose frame outlives the stream's drain (SlotClaim);
// *kept is valid after the caller's synchronise
void queue_walk(uz_ctx *c, uz_ctx::WalkSlot &w, const WalkPlan &p, const std::vector<int64_t> &first, const std::vector<uz_walk_file> &tfile, int64_t *tab_total_p,
                int64_t *kept) {
    const int32_t n_tasks = p.n_tasks;
    hipStream_t st = w.s0;
    int64_t &tab_total = *tab_total_p;
    w.n_desc_all = first.back();
    UZ_WGROW(w, desc, (size_t)first.back() + 1);
    UZ_HIP(hipMemcpyAsync(w.first.p, first.data(), ((size_t)n_tasks + 1) * 8, hipMemcpyHostToDevice, st));
    UZ_HIP(hipMemcpyAsync(w.task.p, p.task, (size_t)n_tasks * UZ_WALK_TASK_COLS * 4, hipMemcpyHostToDevice, st));
    if (p.n_spans) UZ_HIP(hipMemcpyAsync(w.span.p, p.span, (size_t)p.n_spans * UZ_WALK_SPAN_COLS * 8, hipMemcpyHostToDevice, st));
    if (p.n_reach) UZ_HIP(hipMemcpyAsync(w.reach.p, p.reach, (size_t)p.n_reach * 8, hipMemcpyHostToDevice, st));
    if (p.n_fetch) UZ_HIP(hipMemcpyAsync(w.fetch.p, p.fetch, (size_t)p.n_fetch * 12, hipMemcpyHostToDevice, st));
    if (!tfile.empty()) { // (pageable, as `first`: read by the time the synchronise below returns)
        UZ_WGROW(w, tfile, (size_t)n_tasks + 1);
        UZ_HIP(hipMemcpyAsync(w.tfile.p, tfile.data(), (size_t)n_tasks * sizeof(uz_walk_file), hipMemcpyHostToDevice, st));
    }
    uz_launch_bam_walk(c, st, n_tasks, w.out.p, w.out_off.p, w.blk_coff.p, w.task.p, w.span.p, w.reach.p, w.fetch.p, w.count.p, w.first.p, w.walked.p,
                       w.flags.p, w.desc.p, w.n_direct.p, w.tab_first.p, tfile.empty() ? nullptr : w.tfile.p);
    UZ_HIP(hipMemcpyAsync(&tab_total, w.tab_first.p + n_tasks, 8, hipMemcpyDeviceToHost, st));
    UZ_HIP(hipStreamSynchronize(st)); // (the pageable `first` has been read; the hash sets' size is known)
    UZ_WGROW(w, tab, (size_t)tab_total + 1);
    UZ_HIP(hipMemsetAsync(w.tab.p, 0, (size_t)tab_total * 8, st));
    uz_launch_desc_filter(c, st, false, n_tasks, w.desc.p, w.first.p, w.count.p, w.task.p, w.tab_first.p, w.tab.p, w.kcount.p, w.kfirst.p, nullptr);
    UZ_HIP(hipMemcpyAsync(kept, w.kfirst.p + n_tasks, 8, hipMemcpyDeviceToHost, st));
}

// what the inflate and the CRC check left in iflags (queue_blocks), as the call's error
void throw_block_errors(const WalkPlan &p, const std::vector<int64_t> &cut, const std::vector<int32_t> &iflags) {
    const size_t ns = cut.size() - 1;
    const UzBlockFault f = uz_bgzf_first_fault(cut, iflags.data());
    if (f.block >= 0) throw UzError{UZ_E_RANGE, uz_bgzf_fault_text(f, true)};
    if (p.blk_crc && p.n_blocks && iflags[2 * ns])
        throw UzError{UZ_E_RANGE, "CRC mismatch in BGZF block " + std::to_string(iflags[2 * ns] - 1) + " of the batch (file offset " +
                                      std::to_string((long long)p.blk_coff[iflags[2 * ns] - 1]) + ")"};
}

// What uz_reads_from_walk and uz_reads_from_bam share.  The records of a walked batch (they lie inflated in its slot) are unpacked into the columns of
// ONE block (uz_launch_bam_extract), the table adopts the columns where they lie (adopt_device) and keeps the block as its `mirror`; the slot is released.
struct ExtractJob {
    const char *who = "";              // the entry point: in front of the error texts
    const uz_kept_rec *kept = nullptr; // the kept list [n] and the aux bytes of records only the host has seen: device memory, or --
    const uint8_t *aux = nullptr;      // from_host -- the host's, which then travel into the block first
    int64_t aux_bytes = 0;
    bool from_host = false;
    const int64_t *contig_off = nullptr; // [n_contigs + 1], [n_contigs]: host memory
    const int32_t *max_span = nullptr;
    int32_t n_contigs = 0, min_base_qual = 0;
    int64_t n = 0, n_cigar_total = 0, n_row_units = 0, n_seq_units = 0, names_bytes = 0;
    uint32_t n_qnames = 0;
    bool names = false;                 // the read names are unpacked too, and then ...
    uint8_t *names_out = nullptr;       // ... copied to this host memory, or
    bool keep_names = false;            // ... kept in the block, with the kept list and ...
    const uint32_t *name_rec = nullptr; // ... this column (device, [n_qnames]): uz_reads_names answers ids from them
};
static int extract_and_adopt(uz_ctx *c, int walk_id, const ExtractJob &j) {
    uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
    const std::string who = std::string(j.who) + ": ";
    const size_t n = (size_t)j.n, nctg = (size_t)j.n_contigs;
    DevBlock blk;
    uz_kept_rec *d_kept = nullptr;
    uint8_t *d_aux = nullptr, *mapq = nullptr, *aux_col = nullptr, *seq4 = nullptr, *d_names = nullptr;
    int64_t *d_coff = nullptr;
    int32_t *d_span = nullptr, *start = nullptr, *tlen = nullptr, *mate = nullptr, *err = nullptr;
    uint32_t *qname = nullptr, *cigar = nullptr, *plane = nullptr, *name_rec = nullptr;
    uint16_t *flag = nullptr, *l_seq = nullptr, *n_cigar = nullptr;
    blk = uz_carve(c, [&](Carver &cv) {
        if (j.from_host) { d_kept = cv.take<uz_kept_rec>(n); d_aux = cv.take<uint8_t>((size_t)j.aux_bytes + 64); }
        d_coff = cv.take<int64_t>(nctg + 1); d_span = cv.take<int32_t>(nctg + 1); err = cv.take<int32_t>(4);
        start = cv.take<int32_t>(n); tlen = cv.take<int32_t>(n); mate = cv.take<int32_t>(n); qname = cv.take<uint32_t>(n);
        flag = cv.take<uint16_t>(n); l_seq = cv.take<uint16_t>(n); n_cigar = cv.take<uint16_t>(n);
        mapq = cv.take<uint8_t>(n); aux_col = cv.take<uint8_t>(n);
        cigar = cv.take<uint32_t>((size_t)j.n_cigar_total); seq4 = cv.take<uint8_t>((size_t)j.n_seq_units * UZ_SEQ4_UNIT_BYTES);
        plane = cv.take<uint32_t>((size_t)j.n_row_units);
        if (j.names) d_names = cv.take<uint8_t>((size_t)j.names_bytes);
        if (j.keep_names) { d_kept = cv.take<uz_kept_rec>(n); name_rec = cv.take<uint32_t>((size_t)j.n_qnames); }
    });
    int id = -1;
    try {
        hipStream_t st = c->stream;
        const uz_kept_rec *kept = j.kept;
        const uint8_t *aux = j.aux;
        if (j.from_host) {
            if (n) UZ_HIP(hipMemcpyAsync(d_kept, j.kept, n * sizeof(uz_kept_rec), hipMemcpyHostToDevice, st));
            if (j.aux_bytes) UZ_HIP(hipMemcpyAsync(d_aux, j.aux, (size_t)j.aux_bytes, hipMemcpyHostToDevice, st));
            kept = d_kept; aux = d_aux;
        }
        UZ_HIP(hipMemcpyAsync(d_coff, j.contig_off, (nctg + 1) * 8, hipMemcpyHostToDevice, st));
        if (nctg) UZ_HIP(hipMemcpyAsync(d_span, j.max_span, nctg * 4, hipMemcpyHostToDevice, st));
        UZ_HIP(hipMemsetAsync(err, 0, 16, st));
        uz_launch_bam_extract(c, st, j.n, w.out.p, w.out_bytes, aux, j.aux_bytes, kept, j.min_base_qual, start, tlen, mate, qname, flag, l_seq, n_cigar, mapq, aux_col,
                              cigar, seq4, plane, err, d_names, j.n_cigar_total, j.n_row_units, j.n_seq_units, j.names_bytes);
        if (j.names_out && j.names_bytes) UZ_HIP(hipMemcpyAsync(j.names_out, d_names, (size_t)j.names_bytes, hipMemcpyDeviceToHost, st));
        if (j.keep_names && n) {
            UZ_HIP(hipMemcpyAsync(d_kept, kept, n * sizeof(uz_kept_rec), hipMemcpyDeviceToDevice, st));
            if (j.n_qnames) UZ_HIP(hipMemcpyAsync(name_rec, j.name_rec, (size_t)j.n_qnames * 4, hipMemcpyDeviceToDevice, st));
        }
        int32_t e = 0;
        UZ_HIP(hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipStreamSynchronize(st));
        UZ_REQUIRE(e != 2, UZ_E_RANGE, who + "an offset of the kept list points beyond the stores its totals declare");
        UZ_REQUIRE(e == 0, UZ_E_RANGE, who + "a kept record lies outside the walked bytes, or overruns its block_size");
        uz_reads_packed_view v;
        memset(&v, 0, sizeof(v));
        v.n_segs = j.n; v.n_contigs = j.n_contigs; v.contig_off = d_coff; v.max_span = d_span;
        v.start = start; v.tlen = tlen; v.mate = mate; v.qname = qname; v.flag = flag; v.l_seq = l_seq; v.n_cigar = n_cigar; v.mapq = mapq; v.aux = aux_col;
        v.n_cigar_total = j.n_cigar_total; v.cigar = cigar; v.n_row_units = j.n_row_units; v.n_seq_units = j.n_seq_units; v.seq4 = seq4;
        v.qlow = reinterpret_cast<const uint8_t *>(plane); v.min_base_qual = j.min_base_qual; v.n_qnames = j.n_qnames;
        id = adopt_device(c, &v);
        ReadsDev &r = c->reads[(size_t)id];
        r.mirror = blk;
        if (j.keep_names) { r.kept_list = d_kept; r.name_rec = name_rec; r.names = d_names; r.names_bytes = j.names_bytes; }
    } catch (...) { uz_block_put(c, blk); throw; }
    c->book.release(walk_id); // (on success only: a failed batch stays the caller's until its uz_bam_walk_release)
    return id;
}

extern "C" {

int uz_reads_upload(uz_ctx *c, const uz_reads_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id, UZ_E_ARG, "bad reads view");
        ReadsDev r;
        try { uz_reads_upload_impl(c, v, r); } catch (...) { uz_block_put(c, r.block); throw; }
        const int k = new_slot(c->reads);
        c->reads[k] = r;
        *id = k;
    });
}

int uz_reads_upload_packed(uz_ctx *c, const uz_reads_packed_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id, UZ_E_ARG, "bad reads view");
        ReadsDev r;
        try {
            reads_from_packed_host(c, c->copy_stream, v, r);
            UZ_HIP(hipEventCreateWithFlags(&r.ready, hipEventDisableTiming));
            UZ_HIP(hipEventRecord(r.ready, c->copy_stream));
            r.pending = true;
            static const bool lazy = getenv("UZ_BUILD_LAZY") != nullptr; // development aid: the header build at first use, on the compute stream
            if (!lazy) {
                if (!c->build_stream) UZ_HIP(hipStreamCreateWithFlags(&c->build_stream, hipStreamNonBlocking));
                UZ_HIP(hipStreamWaitEvent(c->build_stream, r.ready, 0));
                uz_build_records(c, c->build_stream, r, r.cols, r.build_scratch);
                UZ_HIP(hipEventCreateWithFlags(&r.built, hipEventDisableTiming));
                UZ_HIP(hipEventRecord(r.built, c->build_stream));
            }
        } catch (...) {
            if (r.built) { (void)hipEventSynchronize(r.built); (void)hipEventDestroy(r.built); }
            if (r.ready) { (void)hipEventSynchronize(r.ready); (void)hipEventDestroy(r.ready); }
            uz_block_put(c, r.block); uz_block_put(c, r.mirror); throw;
        }
        const int k = new_slot(c->reads);
        c->reads[k] = r;
        *id = k;
    });
}

int uz_reads_wait(uz_ctx *c, int reads_id) {
    return guarded(c, [&] {
        ReadsDev &r = reads_of(c, reads_id);
        uz_reads_make_ready(c, r);
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_check_upload_flag(c);
    });
}

int uz_reads_headers(uz_ctx *c, int reads_id, int32_t *start, int32_t *end, int32_t *tlen, int32_t *mate, uint32_t *qname) {
    return guarded(c, [&] {
        ReadsDev &r = reads_of(c, reads_id);
        uz_reads_make_ready(c, r);
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_check_upload_flag(c);
        struct HA { int32_t start, end; uint32_t cigar_off, sq_off; }; // the record headers (RecA / RecB of phase_body.hpp)
        struct HB { int32_t mate; uint32_t qname; uint16_t l_seq, n_cigar; int32_t tlen; };
        const size_t n = (size_t)r.n;
        std::vector<HA> a(n);
        std::vector<HB> b(n);
        if (n) {
            UZ_HIP(hipMemcpy(a.data(), r.rec_a, n * sizeof(HA), hipMemcpyDeviceToHost));
            UZ_HIP(hipMemcpy(b.data(), r.rec_b, n * sizeof(HB), hipMemcpyDeviceToHost));
        }
        for (size_t i = 0; i < n; i++) {
            if (start) start[i] = a[i].start;
            if (end) end[i] = a[i].end;
            if (tlen) tlen[i] = b[i].tlen;
            if (mate) mate[i] = b[i].mate;
            if (qname) qname[i] = b[i].qname;
        }
    });
}

int uz_reads_columns(uz_ctx *c, int reads_id, int64_t sizes[4], uint32_t *fm, uint16_t *l_seq, uint16_t *n_cigar, uint32_t *cigar_off, uint32_t *sq_off,
                     uint32_t *qoff, uint32_t *cigar, uint8_t *seq4, uint32_t *qlow) {
    return guarded(c, [&] {
        UZ_REQUIRE(sizes, UZ_E_ARG, "uz_reads_columns: sizes is where the stores' sizes go");
        ReadsDev &r = reads_of(c, reads_id);
        uz_reads_make_ready(c, r);
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_check_upload_flag(c);
        sizes[0] = r.n; sizes[1] = r.n_cigar_total; sizes[2] = r.n_seq_units; sizes[3] = (r.qlow && r.qlow_valid) ? r.n_plane_units : 0;
        struct HA { int32_t start, end; uint32_t cigar_off, sq_off; }; // the record headers (RecA / RecB of phase_body.hpp)
        struct HB { int32_t mate; uint32_t qname; uint16_t l_seq, n_cigar; int32_t tlen; };
        const size_t n = (size_t)r.n;
        if (n && (l_seq || n_cigar || cigar_off || sq_off)) {
            std::vector<HA> a(n);
            std::vector<HB> b(n);
            UZ_HIP(hipMemcpy(a.data(), r.rec_a, n * sizeof(HA), hipMemcpyDeviceToHost));
            UZ_HIP(hipMemcpy(b.data(), r.rec_b, n * sizeof(HB), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) {
                if (l_seq) l_seq[i] = b[i].l_seq;
                if (n_cigar) n_cigar[i] = b[i].n_cigar;
                if (cigar_off) cigar_off[i] = a[i].cigar_off;
                if (sq_off) sq_off[i] = a[i].sq_off;
            }
        }
        if (n && fm) UZ_HIP(hipMemcpy(fm, r.fm, n * 4, hipMemcpyDeviceToHost));
        if (n && qoff) UZ_HIP(hipMemcpy(qoff, r.qoff, n * 4, hipMemcpyDeviceToHost));
        if (cigar && sizes[1]) UZ_HIP(hipMemcpy(cigar, r.cigar, (size_t)sizes[1] * 4, hipMemcpyDeviceToHost));
        if (seq4 && sizes[2]) UZ_HIP(hipMemcpy(seq4, r.seq4, (size_t)sizes[2] * UZ_SEQ4_UNIT_BYTES, hipMemcpyDeviceToHost));
        if (qlow && sizes[3]) UZ_HIP(hipMemcpy(qlow, r.qlow, (size_t)sizes[3] * UZ_QLOW_UNIT_BYTES, hipMemcpyDeviceToHost));
    });
}

int uz_reads_marks(uz_ctx *c, int reads_id, uint16_t *umask, uint8_t *nlow) {
    return guarded(c, [&] {
        ReadsDev &r = reads_of(c, reads_id);
        uz_reads_make_ready(c, r);
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_check_upload_flag(c);
        const size_t n = (size_t)r.n;
        if (n && umask) {
            UZ_REQUIRE(r.umask, UZ_E_STATE, "uz_reads_marks: the table holds no unit masks");
            UZ_HIP(hipMemcpy(umask, r.umask, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        }
        if (n && nlow) {
            UZ_REQUIRE(r.nlow, UZ_E_STATE, "uz_reads_marks: the table holds no low-quality counts");
            UZ_HIP(hipMemcpy(nlow, r.nlow, n, hipMemcpyDeviceToHost));
        }
    });
}

int uz_bgzf_inflate(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, uint8_t *out,
                    int repeat, double *kernel_ms) {
    return guarded(c, [&] { uz_bgzf_inflate_impl(c, comp, comp_bytes, n_blocks, in_off, out_off, out, repeat, kernel_ms); });
}
int uz_bgzf_inflate_to_host(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off,
                            uint8_t *out) {
    return guarded(c, [&] { uz_bgzf_inflate_to_host_impl(c, comp, comp_bytes, n_blocks, in_off, out_off, out); });
}

int uz_reads_adopt_device(uz_ctx *c, const uz_reads_packed_view *v, int *id) {
    return guarded(c, [&] {
        UZ_REQUIRE(v && id, UZ_E_ARG, "bad reads view");
        *id = adopt_device(c, v);
    });
}

int uz_pinned_alloc(size_t bytes, void **out) {
    if (!out) return UZ_E_ARG;
    *out = nullptr;
    if (hipHostMalloc(out, bytes ? bytes : 64, hipHostMallocDefault) != hipSuccess) return UZ_E_HIP;
    std::lock_guard<std::mutex> g(g_pinned_mu);
    g_pinned[(uintptr_t)*out] = bytes ? bytes : 64;
    return 0;
}
void uz_pinned_free(void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        g_pinned.erase((uintptr_t)p);
    }
    (void)hipHostFree(p);
}

int uz_drop_derived(uz_ctx *c) {
    return guarded(c, [&] {
        for (auto &f : c->fams) f.cls_valid = false;
        find_forget(c, -1);
    });
}

int uz_reads_free(uz_ctx *c, int reads_id) {
    return guarded(c, [&] {
        ReadsDev &r = reads_of(c, reads_id);
        // the block goes back to the pool: whatever still reads or fills it must have finished
        if (r.ready) UZ_HIP(hipEventSynchronize(r.ready));
        if (r.built) UZ_HIP(hipEventSynchronize(r.built));
        UZ_HIP(hipStreamSynchronize(c->stream));
        // a merged cohort table built from this table (or the merged table itself) is forgotten with it
        const bool member = std::find(c->cohort_ids.begin(), c->cohort_ids.end(), reads_id) != c->cohort_ids.end();
        if (reads_id == c->cohort_reads) { c->cohort_reads = -1; c->cohort_ids.clear(); }
        else if (member && c->cohort_reads >= 0) {
            free_reads(c, c->reads[(size_t)c->cohort_reads]);
            c->cohort_reads = -1;
            c->cohort_ids.clear();
        }
        free_reads(c, r);
    });
}

int uz_site_scan(uz_ctx *c, int fam_id) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        uz_launch_site_scan(c, f, sites_of(c, f.sites_id), !f.het_only); // (a het-form family has the SNV / breakpoint classes only)
    });
}

int uz_site_scan_many(uz_ctx *c, const int32_t *fam_ids, int32_t n_fam) {
    return guarded(c, [&] {
        UZ_REQUIRE(n_fam >= 0 && (n_fam == 0 || fam_ids != nullptr), UZ_E_ARG, "bad family list");
        if (n_fam == 0) return;
        std::vector<FamilyDev *> fams;
        for (int32_t k = 0; k < n_fam; k++) {
            FamilyDev &f = fam_of(c, fam_ids[k]);
            refuse_het_only(f, "uz_site_scan_many");
            UZ_REQUIRE(f.sites_id == fam_of(c, fam_ids[0]).sites_id, UZ_E_ARG, "the families of one cohort scan must share a sites table");
            for (int32_t j = 0; j < k; j++) UZ_REQUIRE(fam_ids[j] != fam_ids[k], UZ_E_ARG, "family listed twice");
            fams.push_back(&f);
        }
        uz_launch_site_scan_many(c, fams.data(), n_fam, sites_of(c, fams[0]->sites_id), true);
    });
}

int uz_site_classes(uz_ctx *c, int fam_id, uint8_t *out) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        SitesDev &s = sites_of(c, f.sites_id);
        UZ_REQUIRE(out != nullptr, UZ_E_ARG, "null output");
        const bool cnv = !f.het_only; // (a het-form family has the SNV / breakpoint classes only: bits 3-6 stay 0)
        if (!uz_site_scan_fresh(c, f, cnv)) uz_launch_site_scan(c, f, s, cnv);
        if (s.n) UZ_HIP(hipMemcpyAsync(out, f.cls, (size_t)s.n, hipMemcpyDeviceToHost, c->stream));
        UZ_HIP(hipStreamSynchronize(c->stream));
        if (f.het_only) uz_check_upload_flag(c); // (the expansion held every span's het count against het_span_off)
    });
}

int uz_find(uz_ctx *c, int fam_id, const uz_dnms_view *d, int mode, int64_t *cand_off, int64_t *het_off) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        SitesDev &s = sites_of(c, f.sites_id);
        UZ_REQUIRE(d != nullptr && d->n >= 0, UZ_E_ARG, "bad DNM view");
        c->phase_valid = false;
        FindCount counting(c);
        c->find_stat[0] = c->find_stat[1] = c->find_stat[2] = c->find_stat[3] = 0;
        c->find_answer_again = false;
        const bool cnv = (mode & UZ_FIND_WHOLE_REGION) != 0;
        if (cnv) refuse_het_only(f, "a whole-region find");
        if (!uz_site_scan_fresh(c, f, cnv)) uz_launch_site_scan(c, f, s, cnv); // (reads nothing of the batch: queued before the batch is staged)
        uz_stage_dnms(c, d);
        const FindKey key = find_key_of(c, fam_id, mode, d); // (behind the site scan's launch: host work beside the device's)
        find_target(c);
        uz_launch_find(c, f, s, mode);
        if (f.het_only) uz_check_upload_flag(c); // (the expansion held every span's het count against het_span_off; the find has waited for it)
        find_done(c, key);
        c->find_fam = fam_id;
        if (cand_off) memcpy(cand_off, c->cand_off_h.data(), ((size_t)d->n + 1) * sizeof(int64_t));
        if (het_off) memcpy(het_off, c->het_off_h.data(), ((size_t)d->n + 1) * sizeof(int64_t));
    });
}

int uz_find_answer(uz_ctx *c, int fam_id, const uz_dnms_view *d, int mode, void *block, size_t block_bytes, int64_t out[4]) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        SitesDev &s = sites_of(c, f.sites_id);
        UZ_REQUIRE(d != nullptr && d->n >= 0, UZ_E_ARG, "bad DNM view");
        FindCount counting(c);
        UZ_REQUIRE(block != nullptr && (uintptr_t)block % UZ_FA_ALIGN == 0 && inside_one_pinned_block((const uint8_t *)block, (const uint8_t *)block + block_bytes),
                   UZ_E_ARG, "uz_find_answer: the block must be page-locked memory of this library (uz_pinned_alloc), 256-byte aligned");
        c->phase_valid = false;
        const bool cnv = (mode & UZ_FIND_WHOLE_REGION) != 0;
        if (cnv) refuse_het_only(f, "a whole-region find");
        FindAnswer ans{(uint8_t *)block, block_bytes, 0, 0};
        const size_t n = (size_t)d->n;
        // the call after a fall-back, same batch with a block grown to what that call reported: the lists are in HBM, whole (grown and filled
        // again where they had to be) -- only the answer is written.  The counters go on from the first call's.
        // (the recall first: the totals the block is held against are then this batch's, whatever ran on the context in between; a block that
        // is still too small takes the whole find below, which reports the size again)
        if (c->find_answer_again && n > 0 && find_recall(c, find_key_of(c, fam_id, mode, d)) &&
            uz_find_answer_fits(uz_find_answer_layout(d->n, c->n_cand, c->n_het), block_bytes)) {
            c->dn_n_of_find = d->n;
            UZ_REQUIRE(uz_launch_find_answer(c, &ans, INT64_MAX, INT64_MAX), UZ_E_STATE, "uz_find_answer: the block reported as sufficient is not");
        } else {
            c->find_stat[0] = c->find_stat[1] = c->find_stat[2] = c->find_stat[3] = 0;
            if (!uz_site_scan_fresh(c, f, cnv)) uz_launch_site_scan(c, f, s, cnv); // (reads nothing of the batch: queued before the batch is staged)
            uz_stage_dnms(c, d);
            const FindKey key = find_key_of(c, fam_id, mode, d); // (behind the site scan's launch: host work beside the device's)
            find_target(c);
            uz_launch_find(c, f, s, mode, true, &ans);
            if (f.het_only) uz_check_upload_flag(c);
            find_done(c, key);
            c->find_fam = fam_id;
            if (n == 0) { // nothing was launched: the answer of an empty batch is written here
                const FindAnswerLayout L = uz_find_answer_layout(0, 0, 0);
                ans.need = L.total;
                if (!uz_find_answer_fits(L, block_bytes)) ans.code |= UZ_FA_BLOCK_SMALL;
                else {
                    memset(block, 0, (size_t)L.total);
                    int64_t *head = (int64_t *)block;
                    head[2] = 1; head[3] = (int64_t)L.total;
                }
            }
        }
        c->find_answer_again = ans.code != 0;
        c->find_stat[2] |= ans.code;
        c->find_stat[3] = (int64_t)ans.need;
        if (out) { out[0] = ans.code; out[1] = (int64_t)ans.need; out[2] = c->n_cand; out[3] = c->n_het; }
    });
}
int uz_find_stats(uz_ctx *c, int64_t out[4]) {
    if (!c || !out) return UZ_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = c->find_stat[k];
    return 0;
}

int uz_find_fetch(uz_ctx *c, int32_t *cand_idx, uint8_t *cand_flags, int32_t *het_idx) {
    return guarded(c, [&] {
        UZ_REQUIRE(c->find_valid, UZ_E_STATE, "uz_find_fetch before uz_find");
        FindCount counting(c);
        // destinations in page-locked memory of this library (uz_pinned_alloc): by copy kernels, past the DMA engine's queue (uz_launch_find)
        const bool pinned = (!cand_idx || !c->n_cand || inside_one_pinned_block((const uint8_t *)cand_idx, (const uint8_t *)(cand_idx + c->n_cand))) &&
                            (!cand_flags || !c->n_cand || inside_one_pinned_block(cand_flags, cand_flags + c->n_cand)) &&
                            (!het_idx || !c->n_het || inside_one_pinned_block((const uint8_t *)het_idx, (const uint8_t *)(het_idx + c->n_het)));
        if (pinned) {
            const KCopySeg lists[3] = {{cand_idx, c->cand_idx.p, cand_idx ? (size_t)c->n_cand * sizeof(int32_t) : 0},
                                       {cand_flags, c->cand_flags.p, cand_flags ? (size_t)c->n_cand : 0},
                                       {het_idx, c->het_idx.p, het_idx ? (size_t)c->n_het * sizeof(int32_t) : 0}};
            uz_kcopy_many(c, lists, 3); // ONE launch for the three lists
            UZ_HIP(hipStreamSynchronize(c->stream));
            uz_find_waited(c);
            return;
        }
        if (cand_idx && c->n_cand)
            UZ_HIP(hipMemcpyAsync(cand_idx, c->cand_idx.p, (size_t)c->n_cand * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (cand_flags && c->n_cand)
            UZ_HIP(hipMemcpyAsync(cand_flags, c->cand_flags.p, (size_t)c->n_cand, hipMemcpyDeviceToHost, c->stream));
        if (het_idx && c->n_het)
            UZ_HIP(hipMemcpyAsync(het_idx, c->het_idx.p, (size_t)c->n_het * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_find_waited(c);
    });
}

// uz_phase in two halves (unfazed_hip.h)
static void phase_whole(uz_ctx *c, int fam_id, int reads_id, const uz_dnms_view *d, int find_mode, int32_t *status, int32_t *counts, int32_t *origin,
                        int32_t *evidence, bool defer) {
    FamilyDev &f = fam_of(c, fam_id);
    SitesDev &s = sites_of(c, f.sites_id);
    ReadsDev &r = reads_of(c, reads_id);
    UZ_REQUIRE(d != nullptr, UZ_E_ARG, "null DNM view");
    UZ_REQUIRE(!(find_mode & UZ_FIND_WHOLE_REGION), UZ_E_ARG, "the read stage runs on SNV / breakpoint windows");
    c->phase_valid = false;
    c->phase_qbase.clear();
    static const bool trace = getenv("UZ_PHASE_HOST_TRACE") != nullptr; // development aid: where the HOST's time of a read-stage call goes (us)
    const auto t0 = std::chrono::steady_clock::now();
    auto us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    // the read stage consumes the window lists of this batch in SNV / breakpoint mode: those of the caller's own uz_find, if one of
    // the last two finds was over this batch; else computed here
    // (the batch goes up and the site scan is queued BEFORE the key of the batch is worked out: a hash over its columns, host work the device
    // need not wait for)
    // ... and the site scan, which reads nothing of the batch, before the batch's columns are copied into the staging buffer)
    if (!uz_site_scan_fresh(c, f, false)) uz_launch_site_scan(c, f, s, false);
    const double t_scan0 = us();
    uz_stage_dnms(c, d);
    const double t_stage0 = us() - t_scan0, t_scan = us();
    const FindKey key = find_key_of(c, fam_id, find_mode, d);
    const double t_key = us() - t_scan, t_stage = us();
    const bool have = find_recall(c, key);
    if (!have) find_target(c);
    if (!have) {
        uz_launch_find(c, f, s, find_mode, false);
        find_done(c, key);
    }
    const double t_find = us();
    c->find_fam = fam_id;
    uz_launch_phase(c, f, s, r, status, counts, origin, evidence, defer);
    if (trace) fprintf(stderr, "[uz] read-stage call, host us: site scan queued %.0f | stage dnms %.0f | key %.0f | find %.0f | phase (launches, waits, results) %.0f\n", t_scan0,
                       t_stage0, t_key, t_find - t_stage, us() - t_find);
}
int uz_phase(uz_ctx *c, int fam_id, int reads_id, const uz_dnms_view *d, int find_mode, int32_t *status,
             int32_t *counts, int32_t *origin, int32_t *evidence) {
    return guarded(c, [&] {
        UZ_REQUIRE(!c->phase_open, UZ_E_STATE, "uz_phase: a batch is still open (uz_phase_end)");
        phase_whole(c, fam_id, reads_id, d, find_mode, status, counts, origin, evidence, false);
    });
}
int uz_phase_begin(uz_ctx *c, int fam_id, int reads_id, const uz_dnms_view *d, int find_mode) {
    return guarded(c, [&] {
        UZ_REQUIRE(!c->phase_open, UZ_E_STATE, "uz_phase_begin: the batch before this one is still open (uz_phase_end)");
        phase_whole(c, fam_id, reads_id, d, find_mode, nullptr, nullptr, nullptr, nullptr, true);
        c->phase_open = true;
    });
}
int uz_phase_end(uz_ctx *c, int fam_id, int reads_id, const uz_dnms_view *d, int find_mode, int32_t *status, int32_t *counts, int32_t *origin,
                 int32_t *evidence) {
    return guarded(c, [&] {
        UZ_REQUIRE(c->phase_open, UZ_E_STATE, "uz_phase_end without uz_phase_begin");
        c->phase_open = false;
        if (uz_finish_phase(c, status, counts, origin, evidence)) return;
        // the batch outgrew the sizes it was run on: once more, whole, on its own sizes (the DNMs and the window lists of the
        // context may be another batch's by now)
        phase_whole(c, fam_id, reads_id, d, find_mode, status, counts, origin, evidence, false);
    });
}

// ---------------------------------------------------------------- cohort batches: description (cohort_batch), staging (cohort_stage), run
// cohort mode (a family per DNM: k_sites.hip uz_launch_find; a cutoff per DNM: k_reads.hip uz_launch_phase) for the launches of one scope.
// The only writer of cohort_on: outside such a scope it is false, whatever a launch threw.
struct CohortMode {
    uz_ctx *c;
    explicit CohortMode(uz_ctx *c_) : c(c_) { c->cohort_on = true; }
    ~CohortMode() { c->cohort_on = false; }
};
// search_dist = 0 for the find of an allele-balance stage: run_cnv_phasing calls find(..., search_dist=0, whole_region=True), sv_phaser.py:375-389
struct ZeroSearchDist {
    uz_ctx *c;
    const int32_t sd;
    explicit ZeroSearchDist(uz_ctx *c_) : c(c_), sd(c_->P.search_dist) { c->P.search_dist = 0; }
    ~ZeroSearchDist() { c->P.search_dist = sd; }
};

struct CohortBatch {
    const uz_cohort_group *groups = nullptr; int32_t n_groups = 0; // as the caller gave them
    const uz_dnms_view *d = nullptr; bool cnv = false;
    FamilyDev *f0 = nullptr; SitesDev *s = nullptr; // the family of group 0, and the sites table all families share
    std::vector<int32_t> fam;       // per DNM: its group
    std::vector<uint8_t *> cls;     // per group: the class column of its family
    std::vector<FamilyDev *> stale; // the families whose classes are not those of the parameters, each once (a family may serve several groups)
};

// The groups of a cohort call, checked: every group inside the batch, one sites table, the DNMs covered exactly once (empty groups are
// allowed), no het-form family when the whole-region classes are needed (cnv).  Everything that can refuse a batch for its groups is here,
// and nothing of the context is touched.
static CohortBatch cohort_batch(uz_ctx *c, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *d, bool cnv) {
    UZ_REQUIRE(groups && n_groups > 0 && d && d->n >= 0, UZ_E_ARG, "bad cohort batch");
    CohortBatch b;
    b.groups = groups; b.n_groups = n_groups; b.d = d; b.cnv = cnv;
    b.f0 = &fam_of(c, groups[0].fam_id);
    b.s = &sites_of(c, b.f0->sites_id);
    const int32_t n = d->n;
    b.fam.resize((size_t)n);
    b.cls.resize((size_t)n_groups);
    std::vector<std::pair<int32_t, int32_t>> spans;
    for (int32_t g = 0; g < n_groups; g++) {
        FamilyDev *f = &fam_of(c, groups[g].fam_id);
        UZ_REQUIRE(groups[g].dnm_first >= 0 && groups[g].dnm_count >= 0 && (int64_t)groups[g].dnm_first + groups[g].dnm_count <= n, UZ_E_ARG,
                   "cohort group outside the DNM batch");
        UZ_REQUIRE(f->sites_id == b.f0->sites_id, UZ_E_ARG, "the families of a cohort batch must share a sites table");
        if (cnv) refuse_het_only(*f, "a whole-region find / the allele-balance stage");
        if (groups[g].dnm_count) spans.push_back({groups[g].dnm_first, groups[g].dnm_count});
        b.cls[(size_t)g] = f->cls;
        for (int32_t k = 0; k < groups[g].dnm_count; k++) b.fam[(size_t)groups[g].dnm_first + (size_t)k] = g;
        if (!uz_site_scan_fresh(c, *f, cnv) && std::find(b.stale.begin(), b.stale.end(), f) == b.stale.end()) b.stale.push_back(f);
    }
    std::sort(spans.begin(), spans.end());
    int64_t next = 0;
    for (const auto &sp : spans) {
        UZ_REQUIRE(sp.first == next, UZ_E_ARG, "the groups of a cohort batch must cover its DNMs exactly once");
        next += sp.second;
    }
    UZ_REQUIRE(next == n, UZ_E_ARG, "the groups of a cohort batch must cover its DNMs exactly once");
    return b;
}

// A checked batch into the context: the stale families classified in ONE launch, the DNM columns `dv` (the batch's own, or a copy with the
// reads contigs renumbered), dn_fam = the DNM's group, fam_cls = the class column of every group, dn_cutoff when the read stage follows.
static void cohort_stage(uz_ctx *c, CohortBatch &b, const uz_dnms_view *dv, const double *cutoff_per_dnm /* may be null */) {
    const size_t n = (size_t)dv->n, ng = (size_t)b.n_groups;
    if (!b.stale.empty()) uz_launch_site_scan_many(c, b.stale.data(), (int)b.stale.size(), *b.s, b.cnv);
    find_target(c); c->phase_valid = false; // (the cohort's lists take the place of the oldest set, under no key)
    uz_stage_dnms(c, dv);
    c->dn_fam.ensure(n + 1); c->fam_cls.ensure(ng + 1);
    if (cutoff_per_dnm) c->dn_cutoff.ensure(n + 1);
    if (n) UZ_HIP(hipMemcpyAsync(c->dn_fam.p, b.fam.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (n && cutoff_per_dnm) UZ_HIP(hipMemcpyAsync(c->dn_cutoff.p, cutoff_per_dnm, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    UZ_HIP(hipMemcpyAsync(c->fam_cls.p, b.cls.data(), ng * sizeof(uint8_t *), hipMemcpyHostToDevice, c->stream));
    UZ_HIP(hipStreamSynchronize(c->stream)); // the host sides of these copies are the callers' locals
}

// The table a read-stage cohort batch runs on, its contigs "group x contig": contig_base[g] + the number of a contig in group g's file, for
// the nc[g] contigs of that file; q_base[g]: the first query-name id of group g (empty: the vote lists keep the table's own ids).
struct CohortTable {
    ReadsDev *R = nullptr;
    std::vector<int64_t> contig_base;
    std::vector<int32_t> nc;
    std::vector<uint32_t> q_base;
};

// The read stage of a cohort batch over its table: reads contigs renumbered into the table (-1 outside the contigs of the group's file),
// cutoff / name base per DNM, then find and the read stage.
static void cohort_run(uz_ctx *c, CohortBatch &b, const CohortTable &t, int find_mode, int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence) {
    const size_t n = (size_t)b.d->n;
    std::vector<int32_t> rc(n);
    std::vector<double> cut(n);
    std::vector<uint32_t> qb(n);
    for (size_t k = 0; k < n; k++) {
        const size_t g = (size_t)b.fam[k];
        const int32_t r = b.d->rcontig[k];
        rc[k] = (r >= 0 && r < t.nc[g]) ? (int32_t)(t.contig_base[g] + r) : -1;
        cut[k] = b.groups[g].cutoff;
        qb[k] = t.q_base.empty() ? 0u : t.q_base[g];
    }
    uz_dnms_view dv = *b.d;
    dv.rcontig = rc.data();
    cohort_stage(c, b, &dv, cut.data());
    c->phase_qbase = std::move(qb);
    CohortMode on(c);
    uz_launch_find(c, *b.f0, *b.s, find_mode, false);
    c->find_fam = b.groups[0].fam_id;
    uz_launch_phase(c, *b.f0, *b.s, *t.R, status, counts, origin, evidence);
}

// The members' tables end to end as ONE table: the merged table of the context when it was built from these members, else built here (the
// one before it is freed).  Every member is held to the threshold of the parameters before anything is built.
static CohortTable cohort_merged_table(uz_ctx *c, const uz_cohort_group *groups, int32_t n_groups) {
    const size_t ng = (size_t)n_groups;
    CohortTable t;
    t.contig_base.resize(ng); t.nc.resize(ng); t.q_base.resize(ng);
    std::vector<int64_t> rec_base(ng);
    std::vector<int> ids;
    int64_t tot_n = 0, tot_c = 0, tot_u = 0, tot_s = 0, tot_p = 0, tot_contigs = 0;
    uint64_t tot_q = 0;
    for (size_t g = 0; g < ng; g++) {
        ReadsDev &r = reads_of(c, groups[g].reads_id);
        UZ_REQUIRE(groups[g].reads_id != c->cohort_reads, UZ_E_ARG, "the merged cohort table cannot be a member of a cohort");
        uz_reads_ready_for_threshold(c, r, "a reads table of the cohort");
        ids.push_back(groups[g].reads_id);
        rec_base[g] = tot_n; t.contig_base[g] = tot_contigs; t.q_base[g] = (uint32_t)tot_q; t.nc[g] = r.n_contigs;
        tot_n += r.n; tot_c += r.n_cigar_total; tot_u += r.n_row_units; tot_s += r.n_seq_units; tot_p += r.n_plane_units;
        tot_contigs += r.n_contigs; tot_q += r.n_qnames;
    }
    UZ_REQUIRE(tot_n < (int64_t)0x7FFFFFF0 && tot_c < ((int64_t)1 << 32) && tot_u < ((int64_t)1 << 32) && tot_q < ((uint64_t)1 << 32), UZ_E_RANGE,
               "the cohort's alignment records exceed one table's index ranges");
    if (c->cohort_reads < 0 || !c->reads[(size_t)c->cohort_reads].live || c->cohort_ids != ids) {
        if (c->cohort_reads >= 0 && c->reads[(size_t)c->cohort_reads].live) {
            UZ_HIP(hipStreamSynchronize(c->stream));
            free_reads(c, c->reads[(size_t)c->cohort_reads]);
        }
        ReadsDev m;
        m.live = true;
        m.n = tot_n; m.n_contigs = (int32_t)tot_contigs; m.n_qnames = (uint32_t)tot_q; m.n_cigar_total = tot_c; m.n_row_units = tot_u;
        m.n_seq_units = tot_s; m.n_plane_units = tot_p;
        m.block = uz_carve(c, [&](Carver &cv) {
            carve_common(cv, m);
            m.cigar = cv.take<uint32_t>((size_t)tot_c);
            m.seq4 = cv.take<uint8_t>((size_t)tot_s * UZ_SEQ4_UNIT_BYTES);
            m.qlow = cv.take<uint8_t>((size_t)tot_p * UZ_QLOW_UNIT_BYTES);
        });
        m.qlow_thr = c->P.min_gt_qual; m.qlow_valid = true;
        try {
            std::vector<int64_t> co((size_t)tot_contigs + 1, 0);
            std::vector<int32_t> ms((size_t)tot_contigs + 1, 0);
            int64_t cg = 0, un = 0, sn = 0;
            for (size_t g = 0; g < ng; g++) {
                const ReadsDev &r = reads_of(c, groups[g].reads_id);
                std::vector<int64_t> rco((size_t)r.n_contigs + 1);
                std::vector<int32_t> rms((size_t)r.n_contigs + 1);
                UZ_HIP(hipMemcpyAsync(rco.data(), r.contig_off, rco.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
                if (r.n_contigs) UZ_HIP(hipMemcpyAsync(rms.data(), r.max_span, (size_t)r.n_contigs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
                UZ_HIP(hipStreamSynchronize(c->stream));
                for (int32_t k = 0; k < r.n_contigs; k++) {
                    co[(size_t)t.contig_base[g] + k] = rec_base[g] + rco[(size_t)k];
                    ms[(size_t)t.contig_base[g] + k] = rms[(size_t)k];
                }
                uz_concat_table(c, c->stream, m, r, rec_base[g], cg, un, sn, t.q_base[g]);
                cg += r.n_cigar_total; un += r.n_plane_units; sn += r.n_seq_units;
            }
            co[(size_t)tot_contigs] = tot_n;
            UZ_HIP(hipMemcpyAsync(m.contig_off, co.data(), co.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
            UZ_HIP(hipMemcpyAsync(m.max_span, ms.data(), ms.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            uz_finish_table(c, c->stream, m);
            UZ_HIP(hipStreamSynchronize(c->stream)); // co / ms are stack-local
        } catch (...) { uz_block_put(c, m.block); throw; }
        const int k = new_slot(c->reads);
        c->reads[(size_t)k] = m;
        c->cohort_reads = k;
        c->cohort_ids = ids;
    }
    t.R = &c->reads[(size_t)c->cohort_reads];
    return t;
}

int uz_phase_cohort(uz_ctx *c, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *d, int find_mode, int32_t *status,
                    int32_t *counts, int32_t *origin, int32_t *evidence) {
    return guarded(c, [&] {
        UZ_REQUIRE(!(find_mode & UZ_FIND_WHOLE_REGION), UZ_E_ARG, "the read stage runs on SNV / breakpoint windows");
        CohortBatch b = cohort_batch(c, groups, n_groups, d, false);
        const CohortTable t = cohort_merged_table(c, groups, n_groups);
        cohort_run(c, b, t, find_mode, status, counts, origin, evidence);
    });
}

// A table that already IS the groups' tables end to end: one built over the groups' files presented as one (uz_bam_walk_many ->
// uz_reads_from_walk).  group_ref_base [n_groups]: where each group's file starts among the table's contigs; the file's contigs reach to the
// next larger base of any group, or to the table's last.  No concatenation, no copy per group; the vote lists carry the table's own name ids
// (uz_reads_files says where each file's start).  groups[g].reads_id is not looked at.
static CohortTable cohort_joined_table(uz_ctx *c, int reads_id, const int32_t *group_ref_base, int32_t n_groups) {
    UZ_REQUIRE(group_ref_base != nullptr, UZ_E_ARG, "bad cohort batch");
    CohortTable t;
    t.R = &reads_of(c, reads_id);
    UZ_REQUIRE(reads_id != c->cohort_reads, UZ_E_ARG, "the merged cohort table of uz_phase_cohort is not a joined table");
    std::vector<int32_t> bases(group_ref_base, group_ref_base + n_groups);
    std::sort(bases.begin(), bases.end());
    t.contig_base.resize((size_t)n_groups); t.nc.resize((size_t)n_groups);
    for (int32_t g = 0; g < n_groups; g++) {
        UZ_REQUIRE(group_ref_base[g] >= 0 && group_ref_base[g] <= t.R->n_contigs, UZ_E_ARG, "a group's file starts outside the table's contigs");
        const auto nx = std::upper_bound(bases.begin(), bases.end(), group_ref_base[g]);
        t.contig_base[(size_t)g] = group_ref_base[g];
        t.nc[(size_t)g] = (nx == bases.end() ? t.R->n_contigs : *nx) - group_ref_base[g];
    }
    uz_reads_ready_for_threshold(c, *t.R, "the joined reads table");
    return t;
}

int uz_phase_cohort_joined(uz_ctx *c, int reads_id, const uz_cohort_group *groups, int32_t n_groups, const int32_t *group_ref_base, const uz_dnms_view *d,
                           int find_mode, int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence) {
    return guarded(c, [&] {
        UZ_REQUIRE(!(find_mode & UZ_FIND_WHOLE_REGION), UZ_E_ARG, "the read stage runs on SNV / breakpoint windows");
        CohortBatch b = cohort_batch(c, groups, n_groups, d, false);
        const CohortTable t = cohort_joined_table(c, reads_id, group_ref_base, n_groups);
        cohort_run(c, b, t, find_mode, status, counts, origin, evidence);
    });
}

int uz_find_cohort(uz_ctx *c, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *d, int mode, int64_t *cand_off, int64_t *het_off) {
    return guarded(c, [&] {
        CohortBatch b = cohort_batch(c, groups, n_groups, d, (mode & UZ_FIND_WHOLE_REGION) != 0);
        cohort_stage(c, b, d, nullptr);
        { CohortMode on(c); uz_launch_find(c, *b.f0, *b.s, mode); }
        c->find_fam = groups[0].fam_id;
        if (cand_off) memcpy(cand_off, c->cand_off_h.data(), ((size_t)d->n + 1) * sizeof(int64_t));
        if (het_off) memcpy(het_off, c->het_off_h.data(), ((size_t)d->n + 1) * sizeof(int64_t));
    });
}

// K6 over the whole-region lists of the context, the dense site lists behind it, the results back: the counts and the lists' offsets stay
// on the host for uz_phase_cnv_sites
static void cnv_after_find(uz_ctx *c, const SitesDev &s, size_t n, const int32_t *rb_counts, int32_t *cnv_counts, int32_t *origin, int32_t *evidence,
                           int32_t *etype) {
    c->cnv_n = (int32_t)n;
    c->cnv_counts.ensure(2 * n + 2); c->cnv_pos.ensure((size_t)c->n_cand + 1); c->cnv_origin.ensure(n + 1);
    c->cnv_evidence.ensure(n + 1); c->cnv_etype.ensure(n + 1);
    c->cnv_off.ensure(2 * n + 2); c->cnv_dense.ensure((size_t)c->n_cand + 1);
    const int32_t *rb = nullptr;
    if (rb_counts && n) {
        c->cnv_rb.ensure(4 * n);
        UZ_HIP(hipMemcpyAsync(c->cnv_rb.p, rb_counts, 4 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        rb = c->cnv_rb.p;
    }
    uz_launch_cnv(c, s, rb, c->cnv_counts.p, c->cnv_pos.p, c->cnv_origin.p, c->cnv_evidence.p, c->cnv_etype.p);
    uz_launch_cnv_dense(c, c->cnv_counts.p, c->cnv_pos.p, c->cnv_off.p, c->cnv_dense.p);
    c->cnv_counts_h.resize(2 * n + 2);
    c->cnv_off_h.assign(2 * n + 1, 0);
    if (n) {
        UZ_HIP(hipMemcpyAsync(c->cnv_counts_h.data(), c->cnv_counts.p, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        UZ_HIP(hipMemcpyAsync(c->cnv_off_h.data(), c->cnv_off.p, (2 * n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (origin) UZ_HIP(hipMemcpyAsync(origin, c->cnv_origin.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (evidence) UZ_HIP(hipMemcpyAsync(evidence, c->cnv_evidence.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (etype) UZ_HIP(hipMemcpyAsync(etype, c->cnv_etype.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    UZ_HIP(hipStreamSynchronize(c->stream));
    if (cnv_counts && n) memcpy(cnv_counts, c->cnv_counts_h.data(), 2 * n * sizeof(int32_t));
    c->cnv_valid = true;
}

int uz_phase_cnv(uz_ctx *c, int fam_id, const uz_dnms_view *d, const int32_t *rb_counts, int32_t *cnv_counts, int32_t *origin,
                 int32_t *evidence, int32_t *etype) {
    return guarded(c, [&] {
        FamilyDev &f = fam_of(c, fam_id);
        refuse_het_only(f, "uz_phase_cnv");
        SitesDev &s = sites_of(c, f.sites_id);
        UZ_REQUIRE(d != nullptr, UZ_E_ARG, "null DNM view");
        find_target(c); c->phase_valid = false; c->cnv_valid = false;
        uz_stage_dnms(c, d);
        if (!uz_site_scan_fresh(c, f, true)) uz_launch_site_scan(c, f, s, true);
        { ZeroSearchDist zero(c); uz_launch_find(c, f, s, UZ_FIND_WHOLE_REGION, false); }
        c->find_fam = fam_id;
        cnv_after_find(c, s, (size_t)d->n, rb_counts, cnv_counts, origin, evidence, etype);
    });
}

int uz_phase_cnv_cohort(uz_ctx *c, const uz_cohort_group *groups, int32_t n_groups, const uz_dnms_view *d, const int32_t *rb_counts, int32_t *cnv_counts,
                        int32_t *origin, int32_t *evidence, int32_t *etype) {
    return guarded(c, [&] {
        CohortBatch b = cohort_batch(c, groups, n_groups, d, true);
        cohort_stage(c, b, d, nullptr);
        c->cnv_valid = false;
        { ZeroSearchDist zero(c); CohortMode on(c); uz_launch_find(c, *b.f0, *b.s, UZ_FIND_WHOLE_REGION, false); }
        c->find_fam = groups[0].fam_id;
        cnv_after_find(c, *b.s, (size_t)d->n, rb_counts, cnv_counts, origin, evidence, etype);
    });
}

int uz_phase_cnv_sites(uz_ctx *c, int64_t *off, int32_t *pos) {
    return guarded(c, [&] {
        UZ_REQUIRE(c->cnv_valid && c->find_valid, UZ_E_STATE, "uz_phase_cnv_sites before uz_phase_cnv");
        UZ_REQUIRE(off != nullptr, UZ_E_ARG, "null output");
        const size_t n = (size_t)c->cnv_n;
        // dad's sites then mom's per DNM, back to back on the device (k_cnv_dense): their offsets came back with the counts
        memcpy(off, c->cnv_off_h.data(), (2 * n + 1) * sizeof(int64_t));
        const int64_t total = off[2 * n];
        if (!pos || total == 0) return;
        UZ_HIP(hipMemcpy(pos, c->cnv_dense.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    });
}

int uz_phase_votes(uz_ctx *c, int64_t *vote_off, int32_t *vote_val) {
    int rc = 0;
    int g = guarded(c, [&] {
        UZ_REQUIRE(c->phase_valid, UZ_E_STATE, "uz_phase_votes before uz_phase");
        rc = uz_phase_votes_impl(c, vote_off, vote_val);
    });
    return g ? g : rc;
}
int uz_phase_groups(uz_ctx *c, int64_t *grp_off, int32_t *grp_q) {
    int rc = 0;
    int g = guarded(c, [&] {
        UZ_REQUIRE(c->phase_valid, UZ_E_STATE, "uz_phase_groups before uz_phase");
        rc = uz_phase_groups_impl(c, grp_off, grp_q);
    });
    return g ? g : rc;
}
int uz_phase_sizing_fetch(uz_ctx *c, int32_t *bounds, int32_t *pre_win, int32_t *pre_ha, int32_t *pre_hl, int64_t *reduced) {
    int rc = 0;
    int g = guarded(c, [&] {
        UZ_REQUIRE(c->phase_valid && !c->phase_open, UZ_E_STATE, "uz_phase_sizing_fetch before uz_phase / uz_phase_end");
        rc = uz_phase_sizing_fetch_impl(c, bounds, pre_win, pre_ha, pre_hl, reduced);
    });
    return g ? g : rc;
}

int uz_bed_rows(uz_ctx *c, const uz_bed_view *rows, int verbose, int include_ambiguous, int64_t *off, const uint8_t **bytes) {
    return guarded(c, [&] { (void)uz_bed_rows_impl(c, rows, verbose, include_ambiguous, off, bytes); });
}
int uz_vcf_rows(uz_ctx *c, const uz_vcf_text_view *text, const int64_t *line_at, const int64_t *ann_off, const int32_t *ann_col, const uint8_t *ann_gt,
                const int32_t *ann_uops, const int8_t *ann_uet, int64_t *off, const uint8_t **bytes, uint8_t *handed_back) {
    return guarded(c, [&] { (void)uz_vcf_rows_impl(c, text, line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet, off, bytes, handed_back); });
}
int uz_bcf_rows(uz_ctx *c, const uz_bcf_lines_view *records, int64_t *off, uint64_t *samp_at, const uint8_t **bytes, uint8_t *handed_back) {
    return guarded(c, [&] { (void)uz_bcf_rows_impl(c, records, off, samp_at, bytes, handed_back); });
}

int uz_bgzf_deflate(uz_ctx *c, const uint8_t *data, int64_t n_bytes, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes, int repeat, double *kernel_ms) {
    return guarded(c, [&] { (void)uz_bgzf_deflate_impl(c, data, n_bytes, UZ_DF_CODE_FIXED, nullptr, n_blocks, bgzf, bgzf_bytes, repeat, kernel_ms); });
}
int uz_bgzf_deflate_coded(uz_ctx *c, const uint8_t *data, int64_t n_bytes, int code, int64_t *kinds, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes,
                          int repeat, double *kernel_ms) {
    return guarded(c, [&] { (void)uz_bgzf_deflate_impl(c, data, n_bytes, code, kinds, n_blocks, bgzf, bgzf_bytes, repeat, kernel_ms); });
}
int uz_bgzf_deflate_indexed(uz_ctx *c, const uint8_t *data, int64_t n_bytes, int code, int64_t *kinds, int64_t *n_blocks, const uint8_t **bgzf, int64_t *bgzf_bytes,
                            int repeat, double *kernel_ms, int preset, uz_tbx_view *view) {
    return guarded(c, [&] {
        UZ_REQUIRE(view && (preset == UZ_TBX_PRESET_VCF || preset == UZ_TBX_PRESET_BED), UZ_E_ARG, "BGZF deflate: bad index arguments (a view; UZ_TBX_PRESET_VCF or UZ_TBX_PRESET_BED)");
        *view = uz_tbx_view{};
        TbxCall t;
        t.preset = preset;
        t.view = view;
        (void)uz_bgzf_deflate_impl(c, data, n_bytes, code, kinds, n_blocks, bgzf, bgzf_bytes, repeat, kernel_ms, &t);
    });
}

int uz_bed_rows_lists(uz_ctx *c, const uz_bed_view *rows, int verbose, int include_ambiguous, int32_t n_dnms, const int32_t *status, const int64_t *list_off,
                      const int32_t *list_val, uint32_t n_qnames, const uint32_t *name_off, const uint8_t *name_bytes, int32_t evidence_min_ratio, int64_t *off,
                      const uint8_t **bytes) {
    return guarded(c, [&] {
        (void)uz_bed_rows_lists_impl(c, rows, verbose, include_ambiguous, n_dnms, status, list_off, list_val, n_qnames, name_off, name_bytes, evidence_min_ratio, off,
                                     bytes);
    });
}

int uz_prof_enable(uz_ctx *c, int on) {
    return guarded(c, [&] { c->prof_mask = on == 0 ? 0u : on == 1 ? ~0u : (uint32_t)on >> 1; });
}
int uz_prof_reset(uz_ctx *c) {
    return guarded(c, [&] {
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_prof_drain(c);
        for (auto &p : c->prof) p = ProfSlot();
    });
}
int uz_prof_get(uz_ctx *c, int kernel, double *total_ms, int64_t *launches) {
    return guarded(c, [&] {
        UZ_REQUIRE(kernel >= 0 && kernel < UZ_K_COUNT, UZ_E_ARG, "bad kernel id");
        uz_prof_drain(c);
        if (total_ms) *total_ms = c->prof[kernel].total_ms;
        if (launches) *launches = c->prof[kernel].launches;
    });
}
int uz_prof_units(uz_ctx *c, int kernel, int64_t *units) {
    return guarded(c, [&] {
        UZ_REQUIRE(kernel >= 0 && kernel < UZ_K_COUNT && units != nullptr, UZ_E_ARG, "bad kernel id");
        *units = c->prof[kernel].last_units;
    });
}

// ---- the record walk on the device (include/uz_bamwalk.h, csrc/k_bamwalk.hip)
static int bam_walk(uz_ctx *c, const WalkPlan &p, int *walk_id, int64_t *n_desc) {
    const int64_t n_blocks = p.n_blocks, comp_bytes = p.comp_bytes, n_spans = p.n_spans, n_reach = p.n_reach, n_fetch = p.n_fetch;
    const int32_t n_tasks = p.n_tasks;
    const int32_t *task = p.task;
    const uint32_t *blk_crc = p.blk_crc;
    return guarded(c, [&] {
        UZ_REQUIRE(walk_id && n_desc, UZ_E_ARG, "bad arguments");
        check_walk_plan(p);
        const std::vector<uz_walk_file> tfile = p.n_files ? task_files(p) : std::vector<uz_walk_file>();
        UZ_HIP(hipSetDevice(c->device));
        const std::vector<int64_t> first = desc_slices(p), cut = uz_bgzf_slices(n_blocks);
        const size_t ns = cut.size() - 1;
        std::vector<int32_t> iflags(2 * ns + 4, 0); // (what the slot's streams copy into is declared before the claim: it outlives their drain)
        int64_t tab_total = 0, kept = 0;
        // Nothing is freed while batches are in flight (hipFree waits for the whole device -- round 5: a process's second call, whose larger last
        // chunk met another slot than in the first call, stood still for 0.9 s): an outgrown block is parked, and the book hands the parked blocks
        // over only at a claim that finds no other batch in flight (WalkBook::claim).
        const size_t need_out = (size_t)p.out_bytes() + uz_bam_walk_pad(), need_comp = (size_t)uz_bgzf_room(comp_bytes), need_desc = (size_t)first.back() + 1;
        std::vector<void *> drained;
        const int k = c->book.claim([&](int i) { return WalkBook::Caps{c->walk[i].out.cap, c->walk[i].comp.cap, c->walk[i].desc.cap}; }, need_out, need_comp, need_desc, drained);
        for (void *b : drained) (void)hipFree(b);
        UZ_REQUIRE(k >= 0, UZ_E_STATE, "four walked batches are waiting for uz_reads_from_bam / uz_reads_from_walk / uz_bam_walk_release");
        SlotClaim claim(c, k, true);
        uz_ctx::WalkSlot &w = c->walk[k];
        // streams of the slot's own: the blocks of the next batch go up and are inflated while this one is still walked (two calls may run at once)
        if (!w.s0) {
            UZ_HIP(hipStreamCreateWithFlags(&w.s0, hipStreamNonBlocking));
            UZ_HIP(hipStreamCreateWithFlags(&w.s1, hipStreamNonBlocking));
            UZ_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
        }
        w.n_blocks = n_blocks; w.out_bytes = p.out_bytes(); w.n_tasks = n_tasks; w.n_desc = 0; w.n_reach = n_reach;
        w.max_host = n_tasks ? task[UZ_WALK_TASK_COLS * (size_t)(n_tasks - 1) + 9] : -1;
        w.join.started = false; w.join.done = false; w.join.n_need = 0; w.join.n_all = 0; w.join.n_dev = 0; w.join.aux_bytes = 0; w.join.n_look = 0;
        const size_t nb = (size_t)n_blocks + 1, nt = (size_t)n_tasks + 1;
        UZ_WGROW(w, comp, need_comp); UZ_WGROW(w, out, need_out);
        UZ_WGROW(w, in_off, nb); UZ_WGROW(w, out_off, nb); UZ_WGROW(w, blk_coff, nb);
        UZ_WGROW(w, task, (size_t)n_tasks * UZ_WALK_TASK_COLS + 1); UZ_WGROW(w, span, (size_t)n_spans * UZ_WALK_SPAN_COLS + 1);
        UZ_WGROW(w, reach, (size_t)n_reach * 2 + 1); UZ_WGROW(w, fetch, (size_t)n_fetch * 3 + 1);
        UZ_WGROW(w, count, nt); UZ_WGROW(w, first, nt + 1); UZ_WGROW(w, walked, nt); UZ_WGROW(w, flags, nt);
        UZ_WGROW(w, n_direct, nt); UZ_WGROW(w, tab_first, nt + 1); UZ_WGROW(w, kcount, nt); UZ_WGROW(w, kfirst, nt + 1);
        queue_blocks(c, w, p, cut);
        if (n_tasks) queue_walk(c, w, p, first, tfile, &tab_total, &kept);
        if (n_blocks) UZ_HIP(hipMemcpyAsync(iflags.data(), w.iflags.p, (2 * ns + (blk_crc ? 1 : 0)) * sizeof(int32_t), hipMemcpyDeviceToHost, w.s0));
        UZ_HIP(hipStreamSynchronize(w.s0));
        throw_block_errors(p, cut, iflags);
        w.n_desc = kept;
        *n_desc = kept;
        *walk_id = k;
        claim.dismiss();
    });
}

int uz_bam_walk(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, const int64_t *blk_coff,
                const uint32_t *blk_crc, int32_t n_tasks, const int32_t *task, int64_t n_spans, const int64_t *span, int64_t n_reach, const int32_t *reach, int64_t n_fetch,
                const int32_t *fetch, int *walk_id, int64_t *n_desc) {
    const WalkPlan p{comp, comp_bytes, n_blocks, in_off, out_off, blk_coff, blk_crc, n_tasks, task, n_spans, span, n_reach, reach, n_fetch, fetch};
    return bam_walk(c, p, walk_id, n_desc);
}

// the same over the blocks of many files laid end to end as one (unfazed_io.h: uz_bamsrc_open_many; uz_bamwalk.h: uz_walk_file)
int uz_bam_walk_many(uz_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off, const int64_t *out_off, const int64_t *blk_coff,
                     const uint32_t *blk_crc, int32_t n_tasks, const int32_t *task, int64_t n_spans, const int64_t *span, int64_t n_reach, const int32_t *reach, int64_t n_fetch,
                     const int32_t *fetch, int32_t n_files, const int64_t *file_base, const int32_t *ref_base, const uint64_t *salt1, const uint32_t *salt2, int *walk_id,
                     int64_t *n_desc) {
    WalkPlan p{comp, comp_bytes, n_blocks, in_off, out_off, blk_coff, blk_crc, n_tasks, task, n_spans, span, n_reach, reach, n_fetch, fetch};
    p.n_files = n_files < 1 ? -1 : n_files; p.file_base = file_base; p.ref_base = ref_base; p.salt1 = salt1; p.salt2 = salt2; // (-1: refused by task_files)
    return bam_walk(c, p, walk_id, n_desc);
}

int uz_bam_walk_fetch(uz_ctx *c, int walk_id, uz_walk_desc *desc, int64_t *d_first, int32_t *d_flags, int64_t *d_walked) {
    return guarded(c, [&] {
        uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
        UZ_REQUIRE(d_first && (w.n_desc == 0 || desc), UZ_E_ARG, "null output");
        UZ_HIP(hipSetDevice(c->device));
        hipStream_t st = w.s0;
        const int32_t nt = w.n_tasks;
        if (nt == 0) { d_first[0] = 0; return; }
        UZ_WGROW(w, desc_kept, (size_t)w.n_desc + 1);
        uz_launch_desc_filter(c, st, true, nt, w.desc.p, w.first.p, w.count.p, w.task.p, w.tab_first.p, w.tab.p, w.kcount.p, w.kfirst.p, w.desc_kept.p);
        if (w.n_desc) UZ_HIP(hipMemcpyAsync(desc, w.desc_kept.p, (size_t)w.n_desc * sizeof(uz_walk_desc), hipMemcpyDeviceToHost, st));
        UZ_HIP(hipMemcpyAsync(d_first, w.kfirst.p, (size_t)(nt + 1) * 8, hipMemcpyDeviceToHost, st));
        if (d_flags) UZ_HIP(hipMemcpyAsync(d_flags, w.flags.p, (size_t)nt * 4, hipMemcpyDeviceToHost, st));
        if (d_walked) UZ_HIP(hipMemcpyAsync(d_walked, w.walked.p, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipStreamSynchronize(st));
    });
}

int uz_bam_walk_release(uz_ctx *c, int walk_id) {
    return guarded(c, [&] {
        UZ_REQUIRE(walk_id >= 0 && walk_id < uz_ctx::WALK_SLOTS, UZ_E_ARG, "bad walk id"); // (a free slot may be released again)
        c->book.release(walk_id);
    });
}

// ---- the batch-wide joins on the device (csrc/k_bamjoin.hip)
int uz_bam_walk_flags(uz_ctx *c, int walk_id, int32_t *d_flags, int64_t *d_walked) {
    return guarded(c, [&] {
        uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
        if (w.n_tasks == 0) return;
        if (d_flags) UZ_HIP(hipMemcpyAsync(d_flags, w.flags.p, (size_t)w.n_tasks * 4, hipMemcpyDeviceToHost, w.s0));
        if (d_walked) UZ_HIP(hipMemcpyAsync(d_walked, w.walked.p, (size_t)w.n_tasks * 8, hipMemcpyDeviceToHost, w.s0));
        UZ_HIP(hipStreamSynchronize(w.s0));
    });
}

int uz_bam_join(uz_ctx *c, int walk_id, int32_t n_host, const int32_t *h_flags, int32_t n_ref, int all_bases, const uz_walk_desc *xdesc, int64_t n_x, const uint8_t *xaux,
                int64_t xaux_bytes, const int32_t *look_tid, int64_t n_look, const int32_t *need_jtask, int64_t *n_need, int64_t totals[8]) {
    return guarded(c, [&] {
        uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
        UZ_REQUIRE(n_need != nullptr, UZ_E_ARG, "null output");
        UZ_REQUIRE(n_host > w.max_host, UZ_E_ARG, "uz_bam_join: the plan names more tasks of the stage (column 9) than n_host");
        for (int64_t k = 0; k < n_x; k++)
            UZ_REQUIRE((xdesc[k].task & UZ_WALK_TASK_JOIN) && (xdesc[k].src & UZ_WALK_SRC_AUX), UZ_E_ARG, "uz_bam_join: a descriptor of the host without its join task or outside the aux bytes");
        JoinPlanHost P;
        P.n_host = n_host; P.n_ref = n_ref; P.h_flags = h_flags; P.all_bases = all_bases != 0;
        uz_join_run(c, w, P, xdesc, n_x, xaux, xaux_bytes, look_tid, n_look, need_jtask);
        *n_need = w.join.n_need;
        if (totals) for (int k = 0; k < 8; k++) totals[k] = w.join.done ? w.join.tot_h[k] : 0;
    });
}

int uz_bam_join_needs(uz_ctx *c, int walk_id, uz_need_rec *need) {
    return guarded(c, [&] {
        uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
        UZ_REQUIRE(need != nullptr, UZ_E_ARG, "bad walk id");
        uz_join_needs(c, w, need);
    });
}

int uz_bam_join_fetch(uz_ctx *c, int walk_id, uint64_t *voff, uint32_t *qname, int32_t *mate, uint8_t *bases, uz_kept_rec *kept, int64_t *contig_off, int32_t *max_span) {
    return guarded(c, [&] {
        uz_ctx::WalkSlot &w = walk_slot(c, walk_id);
        uz_join_fetch(c, w, voff, qname, mate, bases, kept);
        if (contig_off) for (size_t k = 0; k < w.join.contig_off_h.size(); k++) contig_off[k] = w.join.contig_off_h[k];
        if (max_span) for (int32_t k = 0; k < w.join.n_ref; k++) max_span[k] = w.join.max_span_h[(size_t)k];
    });
}

// Every free slot grown to the largest sizes any batch of this context has asked for, NOW -- by a caller that has just finished a batch and knows
// that more are coming (a staged pipeline keeps up to four in flight): a slot's first use otherwise pays for gigabytes of hipMalloc inside some later
// batch's walk (a pass of bench.py's feed leg that met a fresh slot took 0.7 s instead of 0.17).  n_slots: how many slots the caller will have in use.
int uz_walk_reserve(uz_ctx *c, int n_slots) {
    return guarded(c, [&] {
        UZ_HIP(hipSetDevice(c->device));
        for (int i = 0; i < uz_ctx::WALK_SLOTS && i < n_slots; i++) {
            if (!c->book.claim_slot(i)) continue;
            SlotClaim claim(c, i, false); // (nobody takes the slot while it grows)
            uz_ctx::WalkSlot &w = c->walk[i];
#define UZ_X(T, name) if (const size_t h = c->book.note(WK_##name, 0)) UZ_WGROW(w, name, h);
            UZ_WALK_BUFS(UZ_X)
#undef UZ_X
#define UZ_X(T, name) if (const size_t h = c->book.note(JK_##name, 0)) UZ_JGROW(w.join, name, h);
            UZ_JOIN_BUFS(UZ_X)
#undef UZ_X
        }
    });
}

int uz_walk_slot_stats(uz_ctx *c, int64_t out[8]) {
    return guarded(c, [&] {
        UZ_REQUIRE(out != nullptr, UZ_E_ARG, "null output");
        c->book.stats(&out[0], &out[1], &out[2]);
        out[3] = 0;
        for (int i = 0; i < uz_ctx::WALK_SLOTS && i < 4; i++) out[4 + i] = (int64_t)c->walk[i].out.cap;
    });
}

// The table of a batch whose joins ran on the device: the kept list lies in the slot (uz_bam_join), the records are unpacked where they lie.
int uz_reads_from_walk(uz_ctx *c, int walk_id, int32_t min_base_qual, int want_names, int *reads_id, int64_t totals[8]) {
    return guarded(c, [&] {
        auto &J = walk_slot(c, walk_id).join;
        UZ_REQUIRE(reads_id != nullptr, UZ_E_ARG, "bad walk id");
        UZ_REQUIRE(J.done, UZ_E_STATE, "uz_reads_from_walk: the joins of this batch are not finished (uz_bam_join until it needs nothing)");
        ExtractJob j;
        j.who = "uz_reads_from_walk";
        j.kept = J.kept.p; j.aux = J.aux.p; j.aux_bytes = J.aux_bytes; // (the joins ran on the slot's stream and were waited for: uz_bam_join returns behind them)
        j.contig_off = J.contig_off_h.data(); j.max_span = J.max_span_h.data(); j.n_contigs = J.n_ref; j.min_base_qual = min_base_qual;
        j.n = J.tot_h[JT_N]; j.n_cigar_total = J.tot_h[JT_CIGAR]; j.n_row_units = J.tot_h[JT_UNITS]; j.n_seq_units = J.tot_h[JT_SEQ_UNITS];
        j.names_bytes = J.tot_h[JT_NAME_BYTES]; j.n_qnames = (uint32_t)J.tot_h[JT_QNAMES];
        UZ_REQUIRE(j.n < (int64_t)0x7FFFFFF0 && j.n_cigar_total < ((int64_t)1 << 32) && j.n_row_units < ((int64_t)1 << 32) && j.names_bytes < ((int64_t)1 << 32), UZ_E_RANGE,
                   "uz_reads_from_walk: the batch does not fit the table's 32-bit offsets");
        if (totals) for (int k = 0; k < 8; k++) totals[k] = J.tot_h[k];
        j.names = j.keep_names = want_names != 0; j.name_rec = J.name_rec.p; // the names stay on the device
        *reads_id = extract_and_adopt(c, walk_id, j);
    });
}

// the read names of name ids of such a table: off [n + 1] (host) and the bytes back to back in page-locked memory of the CONTEXT (valid until the
// next call).  The context's own buffers, grown as needed, and copy kernels out of them: a first version made and freed four device blocks per call --
// hipFree waits for the whole device, the next chunk's read stage included: 8 ms per chunk on the calling thread, a tenth of the product's drop-in call.
int uz_reads_names(uz_ctx *c, int reads_id, const uint32_t *ids, int64_t n, int64_t *off, const uint8_t **bytes) {
    return guarded(c, [&] {
        UZ_REQUIRE(reads_id >= 0 && (size_t)reads_id < c->reads.size() && c->reads[(size_t)reads_id].live, UZ_E_ARG, "bad reads id");
        ReadsDev &r = c->reads[(size_t)reads_id];
        UZ_REQUIRE(r.kept_list && r.name_rec, UZ_E_STATE, "uz_reads_names: a table built by uz_reads_from_walk with names");
        UZ_REQUIRE(n >= 0 && off && bytes && (n == 0 || ids), UZ_E_ARG, "bad arguments");
        off[0] = 0;
        *bytes = nullptr;
        if (n == 0) return;
        for (int64_t k = 0; k < n; k++) UZ_REQUIRE(ids[k] < r.n_qnames, UZ_E_ARG, "uz_reads_names: a name id out of range");
        hipStream_t st = c->stream;
        c->nm_ids.ensure((size_t)n + 16); c->nm_len.ensure((size_t)n + 16); c->nm_off.ensure((size_t)n + 16);
        c->nm_pin.room((size_t)n * 4 + 64);
        memcpy(c->nm_pin.p, ids, (size_t)n * 4);
        uz_kcopy(c, c->nm_ids.p, c->nm_pin.p, (size_t)n * 4);
        uz_launch_name_lens(c, st, n, c->nm_ids.p, r.name_rec, r.kept_list, r.n, r.names_bytes, c->nm_len.p);
        UZ_HIP(hipStreamSynchronize(st)); // (the ids have left the staging block)
        uz_kcopy(c, c->nm_pin.p, c->nm_len.p, (size_t)n * 4);
        UZ_HIP(hipStreamSynchronize(st));
        const uint32_t *len = reinterpret_cast<const uint32_t *>(c->nm_pin.p);
        for (int64_t k = 0; k < n; k++) off[k + 1] = off[k] + (int64_t)len[k];
        const int64_t total = off[n];
        UZ_REQUIRE(total < ((int64_t)1 << 32), UZ_E_RANGE, "uz_reads_names: more than 4 GiB of names");
        if (total == 0) { *bytes = c->nm_pin.p; return; }
        std::vector<uint32_t> o32((size_t)n);
        for (int64_t k = 0; k < n; k++) o32[(size_t)k] = (uint32_t)off[k];
        c->nm_pin.room(std::max((size_t)n * 4, (size_t)total) + 64);
        memcpy(c->nm_pin.p, o32.data(), (size_t)n * 4);
        c->nm_out.ensure((size_t)total + 64);
        uz_kcopy(c, c->nm_off.p, c->nm_pin.p, (size_t)n * 4);
        uz_launch_name_gather(c, st, n, c->nm_ids.p, r.name_rec, r.kept_list, r.names, c->nm_len.p, c->nm_off.p, c->nm_out.p);
        UZ_HIP(hipStreamSynchronize(st)); // (the offsets have left the staging block before the names land in it)
        uz_kcopy(c, c->nm_pin.p, c->nm_out.p, ((size_t)total + 3) & ~(size_t)3);
        UZ_HIP(hipStreamSynchronize(st));
        *bytes = c->nm_pin.p;
    });
}

// A table built over many files presented as one (uz_bam_walk_many): per file its first record and its first name id.  ref_base [n_files + 1]: the
// files' references among the table's contigs.  rec_first follows from contig_off; name_first is the smallest name id of the file's records
// (k_reads_files), for a file without records the next file's.  The names of a file must be ONE range of ids, the ranges in file order and
// together every id of the table: that is what lets one name map serve every file, and a table that breaks it is refused.
int uz_reads_files(uz_ctx *c, int reads_id, int32_t n_files, const int32_t *ref_base, int64_t *rec_first, int64_t *name_first) {
    return guarded(c, [&] {
        ReadsDev &r = reads_of(c, reads_id);
        UZ_REQUIRE(n_files >= 1 && ref_base && rec_first && name_first, UZ_E_ARG, "uz_reads_files: bad arguments");
        UZ_REQUIRE(ref_base[0] == 0 && ref_base[n_files] == r.n_contigs, UZ_E_ARG, "uz_reads_files: ref_base must run from 0 to the table's contigs");
        for (int32_t f = 0; f < n_files; f++) UZ_REQUIRE(ref_base[f + 1] >= ref_base[f], UZ_E_ARG, "uz_reads_files: ref_base is a running sum");
        uz_reads_make_ready(c, r);
        hipStream_t st = c->stream;
        std::vector<int64_t> coff((size_t)r.n_contigs + 1);
        UZ_HIP(hipMemcpyAsync(coff.data(), r.contig_off, coff.size() * 8, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipStreamSynchronize(st));
        uz_check_upload_flag(c);
        for (int32_t f = 0; f <= n_files; f++) rec_first[f] = coff[(size_t)ref_base[f]];
        UZ_REQUIRE(rec_first[0] == 0 && rec_first[n_files] == r.n, UZ_E_STATE, "uz_reads_files: the table's contig offsets do not cover its records");
        for (int32_t f = 0; f < n_files; f++) UZ_REQUIRE(rec_first[f + 1] >= rec_first[f], UZ_E_STATE, "uz_reads_files: the table's contig offsets descend");
        c->rf_first.ensure((size_t)n_files + 1); c->rf_mm.ensure(2 * (size_t)n_files);
        std::vector<uint32_t> mm(2 * (size_t)n_files);
        UZ_HIP(hipMemcpyAsync(c->rf_first.p, rec_first, ((size_t)n_files + 1) * 8, hipMemcpyHostToDevice, st));
        uz_launch_reads_files(c, st, n_files, r.rec_b, c->rf_first.p, c->rf_mm.p, c->rf_mm.p + n_files);
        UZ_HIP(hipMemcpyAsync(mm.data(), c->rf_mm.p, mm.size() * 4, hipMemcpyDeviceToHost, st));
        UZ_HIP(hipStreamSynchronize(st));
        int64_t next = 0;
        for (int32_t f = 0; f < n_files; f++) {
            name_first[f] = next;
            if (rec_first[f + 1] == rec_first[f]) continue;
            UZ_REQUIRE((int64_t)mm[(size_t)f] == next && mm[(size_t)n_files + (size_t)f] >= mm[(size_t)f], UZ_E_STATE,
                       "uz_reads_files: the name ids of file " + std::to_string(f) + " do not start where those of the files before it end");
            next = (int64_t)mm[(size_t)n_files + (size_t)f] + 1;
        }
        name_first[n_files] = next;
        UZ_REQUIRE(next == (int64_t)r.n_qnames, UZ_E_STATE, "uz_reads_files: the files' name ids are not the table's");
    });
}

int uz_reads_from_bam(uz_ctx *c, int walk_id, const uz_kept_rec *kept, int64_t n, const uint8_t *aux, int64_t aux_bytes, const int64_t *contig_off,
                      const int32_t *max_span, int32_t n_contigs, int64_t n_cigar_total, int64_t n_row_units, int64_t n_seq_units, uint32_t n_qnames,
                      int32_t min_base_qual, uint8_t *names_out, int64_t names_bytes, int *reads_id) {
    return guarded(c, [&] {
        (void)walk_slot(c, walk_id);
        UZ_REQUIRE(names_bytes >= 0 && (names_out == nullptr || names_bytes < ((int64_t)1 << 32)), UZ_E_ARG, "bad name store size");
        UZ_REQUIRE(reads_id && n >= 0 && n < (int64_t)0x7FFFFFF0 && (n == 0 || kept) && aux_bytes >= 0 && (aux_bytes == 0 || aux) && contig_off && max_span && n_contigs >= 0 &&
                       n_cigar_total >= 0 && n_cigar_total < ((int64_t)1 << 32) && n_row_units >= 0 && n_row_units < ((int64_t)1 << 32) && n_seq_units >= 0 && n_seq_units <= n_row_units,
                   UZ_E_ARG, "bad arguments");
        ExtractJob j;
        j.who = "uz_reads_from_bam";
        j.kept = kept; j.aux = aux; j.aux_bytes = aux_bytes; j.from_host = true; // the host made the kept list: it travels into the table's block
        j.contig_off = contig_off; j.max_span = max_span; j.n_contigs = n_contigs; j.min_base_qual = min_base_qual;
        j.n = n; j.n_cigar_total = n_cigar_total; j.n_row_units = n_row_units; j.n_seq_units = n_seq_units; j.names_bytes = names_bytes; j.n_qnames = n_qnames;
        j.names = names_out != nullptr; j.names_out = names_out; // the names go back to the host, which keeps them
        *reads_id = extract_and_adopt(c, walk_id, j);
    });
}

int uz_crc32_blocks(uz_ctx *c, const uint8_t *data, int64_t n_blocks, const int64_t *off, const uint32_t *want, int64_t *first_bad) {
    return guarded(c, [&] { uz_crc32_blocks_impl(c, data, n_blocks, off, want, first_bad); });
}

// ---- the heads of a cohort's alignment files (csrc/k_bamhead.hip, csrc/headwalk.hpp)
int uz_head_walk(uz_ctx *c, int *head_id, int32_t n_files, const uint8_t *comp, int64_t comp_bytes, int64_t n_blocks, const int64_t *in_off,
                 const int32_t *isize, const uint32_t *crc, const int64_t *blk_first, const int64_t *start, const int64_t *want, const int64_t *have,
                 int64_t *taken, int64_t *cursor, int32_t *state) {
    return guarded(c, [&] { uz_head_walk_impl(c, head_id, n_files, comp, comp_bytes, n_blocks, in_off, isize, crc, blk_first, start, want, have, taken, cursor, state); });
}
int uz_head_rank(uz_ctx *c, int head_id, int32_t readlen, const int64_t *k, uint32_t *a, uint32_t *b) {
    return guarded(c, [&] { uz_head_rank_impl(c, head_id, readlen, k, a, b); });
}
int uz_head_fetch(uz_ctx *c, int head_id, int32_t file, int32_t *out, int64_t cap, int64_t *n) {
    return guarded(c, [&] { uz_head_fetch_impl(c, head_id, file, out, cap, n); });
}
int uz_head_free(uz_ctx *c, int head_id) {
    return guarded(c, [&] { uz_head_free_impl(c, head_id); });
}

} // extern "C"
