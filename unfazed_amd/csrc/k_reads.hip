// k_reads.hip -- read stage on gfx950: K3a per-segment QC pre-pass, the sizing pass and the
// per-DNM phase kernel (phase_body.hpp), plus the host-side launch sequence.  (The tables it reads are built in k_records.hip.)
//
// Launch shape: a persistent grid of 256-lane workgroups (a few per CU) pulls DNM indices from
// one device counter; each workgroup owns a scratch region in HBM sized from the sizing pass.
// The per-DNM working set (tens of KB) stays L2-resident; scans and small sorts go through LDS.
#include "uz_ctx.hpp"
#include "phase_body.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

// development aid: UZ_TRACE=1 in the environment names every kernel of the read stage before its launch (after a
// stream sync), so a device fault can be attributed
#define UZ_TRACE(name) do { if (getenv("UZ_TRACE")) { (void)hipStreamSynchronize(c->stream); fprintf(stderr, "[uz] before %s\n", name); fflush(stderr); } } while (0)

namespace {

// K3a (per-record QC bits) has no kernel of its own any more: with the count of low-quality bases a column of the table, a
// record's QC bits depend on nothing but the record -- the header build (k_pack_rec) writes them once, as a word that
// keeps the mapping quality beside the parameter-independent bits, and the readers apply --min-map-qual (uz_qc_of).

// The sizing pass: one UZ_BW_LANES-lane group per DNM (a DNM has about ten het sites, each costing two lower bounds over its contig's records;
// UZ_BW_SITES items per lane side by side).  What the pass pays for is (a) the length of a DNM's chain of dependent loads and (b) every probe of
// every lane -- about two cycles of its CU each, whether the line is in a cache or not.  So the lanes of a group do TOGETHER what every chain
// would do alike: the first steps of all of a DNM's searches run over the same entries of the index -- its ranges lie within a few thousand
// records of each other -- and take the group one 16-ary search over the coarse index (three steps instead of twelve, 48 probes instead of
// 264) and one over the mid entries under that coarse cell; the UZ_BW_STAGE mid entries from the DNM's lowest bound on go into LDS (coalesced
// loads), where every chain finds its 64-record cell without a probe; what is left per chain is one 32-byte load of the cell's eight mid8
// entries and three steps over the eight record headers under one of them -- ONE line.  A chain beyond the staged entries (a window of more than
// UZ_BW_STAGE x 64 records) takes the levels on its own (uz_lower_bounds_c).
// Round 6, per 100 k DNMs of the bench batch: 0.375 ms (a DNM's window first, its ranges inside it: 43 dependent loads, 120 registers) -> 0.30 (no
// window, mid index) -> 0.22 (32-bit chains: 62 registers, eight waves per SIMD instead of four) -> 0.22 (the group's shared steps: the set-up and
// the shared steps are 0.036 of it -- the rest was the last six steps over the record headers, ~4 lines of HBM traffic per chain) -> 0.150 (mid8).
#ifndef UZ_BW_LANES
#define UZ_BW_LANES 16
#endif
#ifndef UZ_BW_MIN_WAVES
#define UZ_BW_MIN_WAVES 1
#endif
#ifndef UZ_BW_STAGE
#define UZ_BW_STAGE 64
#endif
// first k of [a, b) with ld(k) >= v, else b -- by the GL lanes of a group together (a, b, v uniform over the group; gbase: the group's first lane
// in its wavefront).  Every step: GL probes spread evenly over the bracket, the number of probes below v is the bracket's next GL-th.
template <int GL, typename F>
__device__ __forceinline__ int32_t grp_lower_bound(F ld, int32_t a, int32_t b, int32_t v, int lane, int gbase) {
    constexpr int SH = GL == 64 ? 6 : GL == 32 ? 5 : GL == 16 ? 4 : GL == 8 ? 3 : GL == 4 ? 2 : GL == 2 ? 1 : 0;
    const unsigned long long gmask = GL == 64 ? ~0ull : ((1ull << GL) - 1ull);
    while (a < b) {
        const int32_t chunk = ((b - a) + GL - 1) >> SH;
        const int32_t q = a + lane * chunk;
        const bool below = q < b && ld(q) < v;
        const int cnt = __popcll((__ballot(below) >> gbase) & gmask); // (sorted: the probes below v are the first cnt)
        const int32_t a0 = a;
        if (cnt > 0) a = a0 + (cnt - 1) * chunk + 1;
        if (cnt < GL && a0 + cnt * chunk < b) b = a0 + cnt * chunk;
    }
    return a;
}
// The pass is the first kernel of a batch's read stage, so it also clears what the kernels behind it in stream order fill or count in -- the
// reduced record (k_bounds_reduce), the work cursors with both give-up counts and the list pool's fill level (k_phase): 1.8 KB by its first
// workgroup, where four hipMemsetAsync stood in the stream -- and writes the empty het ranges of the DNMs it does not search for.
struct PhaseClears { int32_t *red; int32_t *cursor; unsigned long long *pool_cursor; int red_words, cursor_words; long long n_het; };
__global__ __launch_bounds__(256, UZ_BW_MIN_WAVES) void k_phase_bounds(PhaseArgs a, int32_t *bounds /* [5n] */, PhaseClears z) {
    constexpr int GL = UZ_BW_LANES, NCH = 2 * UZ_BW_SITES;
    static_assert(GL == 1 || GL == 2 || GL == 4 || GL == 8 || GL == 16 || GL == 32 || GL == 64, "a group is a power of two inside a wavefront");
    __shared__ int32_t s_stage[256 / GL][UZ_BW_STAGE];
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < z.red_words; i += 256) z.red[i] = 0;
        for (int i = threadIdx.x; i < z.cursor_words; i += 256) z.cursor[i] = 0;
        if (threadIdx.x < 2) z.pool_cursor[threadIdx.x] = 0;
        if (threadIdx.x == 2) { a.pre_ha[z.n_het] = 0; a.pre_hl[z.n_het] = 0; } // (the slot behind each column)
    }
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / GL;
    const int lane = threadIdx.x & (GL - 1), gbase = (threadIdx.x & 63) & ~(GL - 1);
    const int d = g < a.n ? (int)g : a.n - 1; // whole groups stay converged for the shuffles below
    long long tp = 0;
    int mh = 0;
    int32_t *b = bounds + 5 * (size_t)d;
    if (g < a.n) {
        const int nc = (int)(a.cand_off[d + 1] - a.cand_off[d]), nh = (int)(a.het_off[d + 1] - a.het_off[d]);
        if (lane == 0) {
            b[0] = b[1] = b[4] = 0;
            b[2] = nh; b[3] = nc;
            for (int k = 0; k < 4; k++) a.pre_win[4 * d + k] = 0;
        }
        if (nc <= 0 || a.no_extended) { // no search writes this DNM's het ranges (uz_phase_bounds_w): they must read as empty
            const long long h0 = a.het_off[d];
            for (int h = lane; h < nh; h += GL) { a.pre_ha[h0 + h] = 0; a.pre_hl[h0 + h] = 0; }
        }
        const RD &R = a.R;
        const int tid = a.rcontig[d];
        const bool tid_ok = tid >= 0 && tid < R.n_contigs;
        const int32_t clo = tid_ok ? (int32_t)R.contig_off[tid] : 0, chi = tid_ok ? (int32_t)R.contig_off[tid + 1] : 0;
        if (nc > 0 && (!R.mid || !tid_ok || chi - clo <= 128)) { // no index to share: every chain on its own
            uz_phase_bounds_w(a, d, b, lane, GL, tp, mh,
                              [&R, clo, chi](const long long (&v)[NCH], const bool (&on)[NCH], long long (&r)[NCH]) { uz_lower_bounds_c<NCH>(R, clo, chi, v, on, r); });
        } else if (nc > 0) {
            // the DNM's lowest bound: of its own fetch (a point variant's) or of its first het site's (the list is sorted)
            const long long span = R.max_span[tid];
            const bool point = a.vartype[d] == UZ_VT_POINT;
            long long vmin_ = 0x7FFFFFFFLL;
            if (point) {
                const long long position = a.dstart[d];
                vmin_ = ((a.dflags[d] & UZ_DF_FETCH_FALLBACK) ? position : position - 1) - span;
            }
            if (!a.no_extended && nh > 0) {
                const long long v0 = (long long)a.spos[a.het_idx[a.het_off[d]]] - span;
                if (v0 < vmin_) vmin_ = v0;
            }
            const int32_t vmin = uz_clamp_i32(vmin_);
            int32_t lo0 = clo, hi0 = chi;
            if (R.coarse && chi - clo > 8192) {
                const int32_t kl = (clo + 4095) >> 12, kh = chi >> 12;
                const int32_t *cx = R.coarse;
                const int32_t a0 = grp_lower_bound<GL>([cx](int32_t k) { return cx[k]; }, kl, kh > kl ? kh : kl, vmin, lane, gbase);
                if (kh > kl) { lo0 = a0 > kl ? ((a0 - 1) << 12) : clo; hi0 = a0 < kh ? (a0 << 12) : chi; }
            }
            const int32_t *mx = R.mid;
            const int32_t kl_m = (clo + 63) >> 6, kh_m = chi >> 6; // the contig's mid entries
            const int32_t ml = (lo0 + 63) >> 6, mhi = hi0 >> 6;
            int32_t lo1 = lo0; // lower_bound(vmin) is not below lo1
            if (mhi > ml) {
                const int32_t m0 = grp_lower_bound<GL>([mx](int32_t k) { return mx[k]; }, ml, mhi, vmin, lane, gbase);
                if (m0 > ml) lo1 = (m0 - 1) << 6;
            }
            int32_t s0 = (lo1 + 63) >> 6;
            if (s0 < kl_m) s0 = kl_m;
            int32_t s_end = s0 + UZ_BW_STAGE < kh_m ? s0 + UZ_BW_STAGE : kh_m;
            if (s_end < s0) s_end = s0;
            const int32_t cnt = s_end - s0;
            int32_t *sm = s_stage[threadIdx.x / GL];
            for (int i = lane; i < cnt; i += GL) sm[i] = mx[s0 + i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (the group is inside one wavefront: its LDS accesses are in order; the fences are for the compiler)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const bool whole = s_end == kh_m; // the staged entries reach the contig's end
            uz_phase_bounds_w(a, d, b, lane, GL, tp, mh, [&R, clo, chi, sm, s0, cnt, lo1, whole](const long long (&v_)[NCH], const bool (&on)[NCH], long long (&r)[NCH]) {
                int32_t x[NCH], y[NCH], v[NCH];
                bool far[NCH], any_far = false;
#pragma unroll
                for (int s = 0; s < NCH; s++) { v[s] = uz_clamp_i32(v_[s]); x[s] = 0; y[s] = on[s] ? cnt : 0; }
                uz_lb_level<NCH>([sm](int32_t k) { return sm[k]; }, x, y, v, 0); // its 64-record cell, in LDS
#pragma unroll
                for (int s = 0; s < NCH; s++) {
                    const int32_t k = x[s];
                    far[s] = on[s] && k == cnt && !whole;
                    any_far |= far[s];
                    x[s] = k > 0 ? ((s0 + k - 1) << 6) : lo1;
                    y[s] = (on[s] && !far[s]) ? (k < cnt ? ((s0 + k) << 6) : chi) : x[s];
                    if (!on[s]) x[s] = y[s] = clo;
                }
                if (R.mid8) uz_mid8_refine<NCH>(R.mid8, x, y, v);
                const RecA *rx = R.ra;
                uz_lb_level<NCH>([rx](int32_t k) { return rx[k].start; }, x, y, v, clo);
#pragma unroll
                for (int s = 0; s < NCH; s++) r[s] = x[s];
                if (any_far) { // beyond the staged entries
                    long long rf[NCH];
                    uz_lower_bounds_c<NCH>(R, clo, chi, v_, far, rf);
#pragma unroll
                    for (int s = 0; s < NCH; s++) if (far[s]) r[s] = rf[s];
                }
            });
        }
    }
#pragma unroll
    for (int o = GL >> 1; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o, GL);
        const int m2 = __shfl_xor(mh, o, GL);
        mh = m2 > mh ? m2 : mh;
    }
    if (g < a.n && lane == 0) {
        b[1] = (int32_t)(tp > 0x7FFFFFF0LL ? 0x7FFFFFF0LL : tp);
        b[4] = mh;
    }
}

#ifndef UZ_PHASE_PARTS
#define UZ_PHASE_PARTS 8 // XCDs of an MI355X
#endif
#ifndef UZ_PHASE_MIN_WAVES
#define UZ_PHASE_MIN_WAVES 4 // LDS build: a workgroup is ONE wave (wg.hpp), so this is workgroups per SIMD: 4 -> up to 16 DNMs per CU, <= 128 VGPRs (what the LDS arenas leave room for anyway)
#endif
// Two builds of the per-DNM body (phase_body.hpp): k_phase<true> keeps the working arrays of a DNM in its workgroup's LDS
// arena and hands the DNMs that do not fit to k_phase<false>, launched right behind it, which keeps them in HBM scratch.
template <bool LDS>
__global__ __launch_bounds__(WG_NT, LDS ? UZ_PHASE_MIN_WAVES : 5) void k_phase(PhaseArgs a_by_value) {
    __shared__ WgSharedT<LDS ? 1 : WG_SORT_LDS_CAP> sh;
    extern __shared__ __attribute__((aligned(16))) uint8_t uz_lds_arena[];
    // the arguments are read where they lie, phase by phase (phase_body.hpp: uz_args_load); the by-value parameter only gives the kernarg
    // segment its layout (PhaseArgs is the kernel's first and only explicit argument: offset 0)
    (void)a_by_value;
    const PhaseArgsK ap = (PhaseArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    if constexpr (!LDS) {
        // the HBM build only ever runs over a list (what both arena launches gave up), and that list is usually empty: out before the cursor's
        // atomic -- 2 048 workgroups taking their turn on one word were the 27 us of this launch in every chunk of a staged pass
        if (*uz_g(ap->src_count) <= 0) return;
    }
    uint8_t *const scr_base = uz_g(ap->scratch) + (size_t)blockIdx.x * ap->scratch_per_wg;
#ifdef UZ_PHASE_TIMING
    if (threadIdx.x < 24) sh.tick[threadIdx.x] = 0;
    struct TickFlush { // on every way out of the kernel
        decltype(sh) *s; unsigned long long *t;
        __device__ ~TickFlush() { __syncthreads(); if (threadIdx.x < 24 && s->tick[threadIdx.x]) atomicAdd(&t[threadIdx.x], s->tick[threadIdx.x]); }
    } tick_flush{&sh, uz_g(ap->timing)};
#endif
    // Work distribution.  A launch over the whole batch: the batch is cut into UZ_PHASE_PARTS contiguous DNM ranges, one cursor each, and a
    // workgroup starts on the range of (blockIdx % PARTS) -- with the usual round-robin placement of workgroups over the 8 XCDs that is
    // "its XCD's range".  DNMs are sorted by position and neighbours share window sites and alignment records, so the lines one of them pulls
    // into the XCD's L2 serve the next (each XCD has its own L2).  A workgroup whose range is exhausted goes on to the other ranges; nothing
    // depends on where a workgroup really runs.  A launch over a list (the DNMs the launch before it gave up): one cursor.
    // (ONE call of the body for both: inlined twice, the kernel was twice the instruction cache's size)
    const bool from_list = ap->from_list != 0;
    int part = from_list ? ap->cursor_slot : (int)(blockIdx.x % UZ_PHASE_PARTS);
    int tried = 0;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const int k = atomicAdd(uz_g(ap->work_cursor) + 16 * part, 1); // cursors on separate cache lines
            if (from_list) sh.bcast[0] = k < *uz_g(ap->src_count) ? uz_g(ap->src_list)[k] : -1;
            else {
                const int n = ap->n;
                const int lo = (int)((long long)n * part / UZ_PHASE_PARTS), hi = (int)((long long)n * (part + 1) / UZ_PHASE_PARTS);
                sh.bcast[0] = lo + k < hi ? lo + k : -1;
            }
        }
        __syncthreads();
        const int d = sh.bcast[0];
        if (d < 0) {
            if (from_list || ++tried >= UZ_PHASE_PARTS) break;
            part = (part + 1) % UZ_PHASE_PARTS;
            continue;
        }
        if (uz_phase_dnm<LDS>(ap, scr_base, &sh, LDS ? uz_lds_arena : nullptr, d)) { // (uniform; the HBM build never gives a DNM up)
            if (threadIdx.x == 0) uz_g(ap->retry_list)[atomicAdd(uz_g(ap->retry_count), 1)] = d;
        }
    }
}

struct PhaseState {
    DevBuf<uint8_t> scratch;
    // res: the per-DNM results as they go back to the host in ONE copy -- status [n], counts [4n], origin [n], evidence [n], then (8-byte
    // aligned) the fill level of the list pool; pre_h: first record and length of every het-site fetch range, [2 (n_het + 1)]
    DevBuf<int32_t> bounds, bounds_red, res, cursor, pool, list_len, pre_win, pre_h, retry;
    DevBuf<long long> list_start;
    unsigned long long *pool_cursor = nullptr; // (inside res)
    DevBuf<unsigned int> need_count;
    int32_t *bounds_h = nullptr; // pinned: the copy back must not block the host, the marking kernels follow it
    size_t bounds_h_cap = 0;
    int32_t *res_h = nullptr;    // pinned staging of the per-DNM results
    size_t res_h_cap = 0;
    // the sizes of the batch before this one (with head room): what a batch is first run on (uz_launch_phase)
    bool spec_valid = false;
    Caps spec_caps = {0, 0, 0, 0, 0, 0};
    int spec_arena = 0, spec_arena2 = 0;
    double spec_sumP_per_dnm = 0.0;
    long long spec_runs = 0, spec_misses = 0;
    hipEvent_t bounds_ready = nullptr;
    int n_cus = 0;
    std::vector<long long> list_start_h;
    std::vector<int32_t> list_len_h;
    bool have_lists = false;
    int32_t n = 0;
    int64_t n_het = 0; // het sites of the batch the sizing pass last ran on (uz_phase_sizing_fetch)
    // uz_phase_begin left a speculative run in flight: what uz_finish_phase needs to judge it
    bool pending = false;
    Caps pend_caps = {0, 0, 0, 0, 0, 0};
    size_t pend_pool_cap = 0;
    int pend_want_lists = 0;
    bool force_exact = false; // the next run skips the speculative sizing (a batch that outgrew it is run again on its own sizes)
};

RD make_rd(const ReadsDev &r) {
    RD R;
    R.ra = (const RecA *)r.rec_a; R.rb = (const RecB *)r.rec_b; R.fm = r.fm;
    R.contig_off = r.contig_off; R.max_span = r.max_span; R.n_contigs = r.n_contigs;
    R.cigar = r.cigar; R.seq4 = r.seq4; R.qlow = r.qlow; R.qoff = r.qoff; R.nlow = r.nlow; R.umask = r.umask; R.qs = r.qs; R.min_map_qual = 0; R.coarse = r.coarse; R.mid = r.mid; R.mid8 = r.mid8;
    R.err = nullptr; // set by the launcher of the per-DNM kernel
    return R;
}

int next_pow2(long long v) {
    long long p = 1;
    while (p < v) p <<= 1;
    return (int)p;
}

} // namespace

void uz_phase_state_free(uz_ctx *c) {
    PhaseState *st = (PhaseState *)c->phase_state;
    if (!st) return;
    st->scratch.release(); st->bounds.release(); st->res.release();
    st->cursor.release(); st->pre_win.release(); st->pre_h.release(); st->pool.release(); st->list_len.release(); st->list_start.release();
    st->pool_cursor = nullptr; st->need_count.release();
    if (st->bounds_ready) (void)hipEventDestroy(st->bounds_ready);
    if (st->bounds_h) (void)hipHostFree(st->bounds_h);
    delete st;
    c->phase_state = nullptr;
}

int uz_want_lists = 1; // uz_phase always keeps the lists available for uz_phase_votes / uz_phase_groups

struct Sizes { Caps caps; int arena, arena2; long long sumP; };
static const int arena_env = [] { const char *e = getenv("UZ_PHASE_LDS_KB"); return e ? atoi(e) * 1024 : -1; }();
// the share of a batch's DNMs (per mille, by the estimate below) the arena is sized to hold; the rest take the HBM build behind it
// (1000 / 990 / 940 / 900 on the bench batch: 3.16 / 2.98 / 2.84 / 2.84 ms -- one more wave per CU is worth more than the 1.3 % of the DNMs redone)
static const int arena_permille = [] { const char *e = getenv("UZ_PHASE_ARENA_PERMILLE"); return e ? atoi(e) : 940; }();
// What the host needs of a batch's bounds (k_phase_bounds: five numbers per DNM) is a handful of maxima, one sum and a histogram: reduced on
// the device (k_bounds_reduce) behind the sizing pass, 1.1 KB come back instead of 20 bytes per DNM -- through round 5 the host walked the 2 MB
// of a 100 k-DNM batch twice between the device's last kernel and the call's return (0.24 ms of a 4.3 ms resident step with the device idle).
struct BoundsRed {
    int32_t mA, mT, mH, mC, active, pad;
    unsigned long long mM, sumP; // (mM by atomicMax on 64 bits)
    int32_t hist[256];           // arena estimate in units of 256 bytes, DNMs with candidate sites only
};
// (every workgroup ends with ~17 atomics on ONE 1 KB record, which the L2 takes one after the other -- ~5 ns each: 391 workgroups were 37 us for
// a pass over 2 MB; a few dozen workgroups walking more DNMs each are not)
#ifndef UZ_BR_BLOCKS
#define UZ_BR_BLOCKS 48
#endif
__global__ __launch_bounds__(256) void k_bounds_reduce(const int32_t *__restrict__ bounds, int32_t n, BoundsRed *out) {
    __shared__ int32_t hist[256];
    __shared__ unsigned long long part[4][8];
    hist[threadIdx.x] = 0;
    __syncthreads();
    long long mA = 0, mT = 0, mH = 0, mC = 0, mM = 0, sumP = 0, active = 0;
    int bin = -1;
    for (int64_t d0 = (int64_t)blockIdx.x * 256; d0 < n; d0 += (int64_t)gridDim.x * 256) { // (whole wavefronts stay in the loop: the ballots below)
        const int64_t d = d0 + threadIdx.x;
        const bool in = d < n;
        const int32_t *b = bounds + 5 * (in ? d : 0);
        const long long b0 = in ? b[0] : 0, b1 = in ? b[1] : 0, b2 = in ? b[2] : 0, b3 = in ? b[3] : 0, b4 = in ? b[4] : 0;
        mA = max(mA, b0); mT = max(mT, b1); mH = max(mH, b2); mC = max(mC, b3);
        const long long M = b1 + 4LL * b0 * (b4 + 1);
        mM = max(mM, M);
        sumP += min(M, 4096LL) + b3;
        if (b3 > 0) {
            const long long est = ((37LL * b1) / 4 + 10LL * b0 + 3328 + 255) >> 8;
            bin = (int)min(est, 255LL);
            active++;
        }
        // (a batch's estimates fall into a handful of bins: one LDS atomic per distinct bin of the wavefront, not 64 on the same word)
        unsigned long long left = __ballot(bin >= 0);
        while (left) {
            const int bb = __shfl(bin, __ffsll((long long)left) - 1, 64);
            const unsigned long long m = __ballot(bin == bb);
            if ((int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicAdd(&hist[bb], (int32_t)__popcll(m));
            left &= ~m;
        }
        bin = -1;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mA = max(mA, __shfl_xor(mA, o, 64)); mT = max(mT, __shfl_xor(mT, o, 64)); mH = max(mH, __shfl_xor(mH, o, 64)); mC = max(mC, __shfl_xor(mC, o, 64));
        mM = max(mM, __shfl_xor(mM, o, 64)); sumP += __shfl_xor(sumP, o, 64); active += __shfl_xor(active, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[w][0] = (unsigned long long)mA; part[w][1] = (unsigned long long)mT; part[w][2] = (unsigned long long)mH; part[w][3] = (unsigned long long)mC;
        part[w][4] = (unsigned long long)mM; part[w][5] = (unsigned long long)sumP; part[w][6] = (unsigned long long)active;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r[7];
        for (int k = 0; k < 7; k++) { r[k] = part[0][k]; for (int q = 1; q < 4; q++) r[k] = k < 5 ? max(r[k], part[q][k]) : r[k] + part[q][k]; }
        atomicMax(&out->mA, (int32_t)r[0]); atomicMax(&out->mT, (int32_t)r[1]); atomicMax(&out->mH, (int32_t)r[2]); atomicMax(&out->mC, (int32_t)r[3]);
        atomicMax(&out->mM, r[4]); atomicAdd(&out->sumP, r[5]); atomicAdd(&out->active, (int32_t)r[6]);
    }
    if (hist[threadIdx.x]) atomicAdd(&out->hist[threadIdx.x], hist[threadIdx.x]);
}
static Sizes phase_exact_sizes(const BoundsRed *br, int32_t n) {
    const long long mA = br->mA, mT = br->mT, mH = br->mH, mC = br->mC, mM = (long long)br->mM, sumP = (long long)br->sumP;
    Sizes z;
    z.caps.A = (int32_t)mA; z.caps.T = (int32_t)mT; z.caps.H = (int32_t)mH; z.caps.C = (int32_t)mC;
    z.caps.I = (int32_t)(4 * mA);
    z.caps.M = next_pow2(std::min<long long>(std::max<long long>(mM, 2), 1 << 20));
    z.sumP = sumP;
    // LDS arena of k_phase<true>, sized for THIS batch.  One wave works on a DNM, so the arena alone decides how many DNMs a CU has in
    // flight: a DNM needs about 9.2 bytes per record its het-site fetches return plus 3.2 KiB (fit over the bench workload by the CPU twin,
    // scripts/phase_sizes.py: residual p99 0.4 KiB).  The 94th percentile of that estimate over the batch decides how
    // many waves share a CU's 160 KiB (at most 4 x UZ_PHASE_MIN_WAVES: registers), and the arena is then the largest that this many leave
    // room for.  The bench batch runs 16 DNMs per CU on 9.25 KiB arenas; a deep-coverage batch gets larger arenas and fewer waves instead
    // of handing most of its DNMs to the slower HBM build.
    z.arena = arena_env;
    if (z.arena < 0) {
        // (k_bounds_reduce: est = ((37 b[1]) / 4 + 10 b[0] + 3328 + 255) >> 8 over the DNMs with candidate sites -- b[0]: records of the DNM's own
        // fetch, 33 of a point variant, hundreds around an SV's breakpoints: a class byte and two flags each)
        const int32_t *hist = br->hist;
        const int32_t active = br->active;
        int u = 16, seen = 0, umax = 16;
        for (int k = 0; k < 256; k++) if (hist[k]) umax = k;
        for (int k = 0; k < 256; k++) {
            seen += hist[k];
            if (hist[k]) u = std::max(u, k);
            if ((long long)seen * 1000 >= (long long)active * arena_permille) break;
        }
        z.arena = std::min(u * 256, 62 * 1024);
        z.arena2 = std::min(std::max(2 * z.arena, umax * 256 + 1024), 62 * 1024);
    } else
        z.arena2 = std::min(2 * z.arena, 62 * 1024);
    return z;
}

void uz_launch_phase(uz_ctx *c, FamilyDev &f, const SitesDev &s, ReadsDev &r, int32_t *status, int32_t *counts,
                     int32_t *origin, int32_t *evidence, bool defer) {
    if (!c->phase_state) c->phase_state = new PhaseState();
    PhaseState *st = (PhaseState *)c->phase_state;
    const int32_t n = c->dn.n;
    st->n = n;
    st->have_lists = false;
    st->pending = false;
    c->phase_n = n;
    if (n <= 0) { c->phase_valid = true; return; }
    static const bool host_trace = getenv("UZ_PHASE_HOST_TRACE") != nullptr; // development aid (abi.hip: phase_whole)
    const auto host_t0 = std::chrono::steady_clock::now();
    auto host_us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - host_t0).count(); };
    double t_queued = 0, t_synced = 0, t_sized = 0;
    uz_reads_ready_for_threshold(c, r, "the reads table");

    PhaseArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.min_gt_qual = c->P.min_gt_qual; a.readlen = c->P.readlen; a.no_extended = c->P.no_extended;
    a.read_goal = c->P.read_goal; a.evidence_min_ratio = c->P.evidence_min_ratio; a.split_error_margin = c->P.split_error_margin;
    a.cutoff = c->dn.cutoff;
    a.cutoff_d = c->cohort_on ? c->dn_cutoff.p : nullptr;
    a.spos = s.pos; a.sref = s.ref_base; a.salt = s.alt_base;
    a.cand_off = c->cand_off.p; a.het_off = c->het_off.p;
    a.cand_idx = c->cand_idx.p; a.het_idx = c->het_idx.p; a.cand_flags = c->cand_flags.p;
    a.rcontig = c->dn.rcontig.p; a.dstart = c->dn.start.p; a.dend = c->dn.end.p; a.dflags = c->dn.dflags.p; a.vartype = c->dn.vartype.p;
    a.allele_off = c->dn.allele_off.p; a.alleles = c->dn.alleles.p;
    a.R = make_rd(r);
    a.R.err = c->hflags + 1;
    a.R.min_map_qual = c->P.min_map_qual;

    // sizing pass -> scratch capacities (max over the batch)
    st->bounds.ensure((size_t)5 * n);
    st->pre_win.ensure((size_t)4 * n); st->pre_h.ensure(2 * ((size_t)c->n_het + 1));
    a.pre_win = st->pre_win.p; a.pre_ha = st->pre_h.p; a.pre_hl = st->pre_h.p + (size_t)c->n_het + 1;
    st->n_het = c->n_het;
    const size_t res_ints = (size_t)7 * n + ((7 * (size_t)n) & 1); // the results, padded to eight bytes; the pool's fill level behind them
    st->res.ensure(res_ints + 4);
    st->pool_cursor = (unsigned long long *)(st->res.p + res_ints);
    // the work cursors, and behind them the counts of the two lists of given-up DNMs: ONE block, cleared as one
    constexpr int cursor_words = 16 * (UZ_PHASE_PARTS + 2) + 32;
    st->cursor.ensure(cursor_words);
    st->bounds_red.ensure(sizeof(BoundsRed) / sizeof(int32_t) + 16);
    {
        const unsigned nb = (unsigned)(((int64_t)n * UZ_BW_LANES + 255) / 256);
        const PhaseClears z = {st->bounds_red.p, st->cursor.p, st->pool_cursor, (int)(sizeof(BoundsRed) / sizeof(int32_t)), cursor_words, (long long)c->n_het};
        ProfScope ps(c, UZ_K_SIZING);
        UZ_TRACE("k_phase_bounds");
        hipLaunchKernelGGL(k_phase_bounds, dim3(nb), dim3(256), 0, c->stream, a, st->bounds.p, z);
        UZ_HIP(hipGetLastError());
    }
    if (st->bounds_h_cap < sizeof(BoundsRed) / sizeof(int32_t)) {
        if (st->bounds_h) (void)hipHostFree(st->bounds_h);
        st->bounds_h = nullptr;
        st->bounds_h_cap = sizeof(BoundsRed) / sizeof(int32_t) + 64;
        UZ_HIP(hipHostMalloc((void **)&st->bounds_h, st->bounds_h_cap * sizeof(int32_t), hipHostMallocDefault));
    }
    hipLaunchKernelGGL(k_bounds_reduce, dim3((unsigned)std::max(1, std::min(UZ_BR_BLOCKS, (n + 255) / 256))), dim3(256), 0, c->stream, (const int32_t *)st->bounds.p, n,
                       reinterpret_cast<BoundsRed *>(st->bounds_red.p));
    UZ_HIP(hipGetLastError());
    // The sizes of the batch (k_phase_bounds) decide the scratch capacities, the LDS arena and the grid.  Waiting for them costs a
    // host round trip per batch -- a staged pass makes one per chunk.  So a batch is first run SPECULATIVELY on the capacities of the
    // batch before it (with head room): the kernels refuse what does not fit (UZ_ST_CAPACITY, never a write out of bounds), the
    // bounds come back with the results, and only when they exceed what was assumed is the batch run again on its own sizes.
    // (UZ_PHASE_NO_SPEC=1, the capacity / arena test hooks and the first batch of a context take the exact path.)
    const BoundsRed *const bh_own = reinterpret_cast<const BoundsRed *>(st->bounds_h); // (kept apart from the result staging below: both are read after the run)
    auto check_upload_flags = [&] { uz_check_upload_flag(c); };
    auto exact_sizes = [&](const BoundsRed *bh) { return phase_exact_sizes(bh, n); };
    if (st->n_cus <= 0) { // asked once: the query is not cheap
        hipDeviceProp_t prop;
        UZ_HIP(hipGetDeviceProperties(&prop, c->device));
        st->n_cus = prop.multiProcessorCount;
    }
    static const bool no_spec = getenv("UZ_PHASE_NO_SPEC") != nullptr;
    const bool hooks = getenv("UZ_TEST_CAP_T") || getenv("UZ_TEST_PHASE_ARENA");
    bool speculative = st->spec_valid && !no_spec && !hooks && !st->force_exact;
    st->force_exact = false;
    // An exact run waits for the reduced record in front of its launches: it comes back now, by a copy of its own.  A speculative run reads it
    // behind the run: it rides with the results (ONE copy launch at the end of the sequence).
    const bool bounds_early = !speculative;
    if (bounds_early) {
        uz_kcopy(c, st->bounds_h, st->bounds_red.p, sizeof(BoundsRed));
        if (!st->bounds_ready) UZ_HIP(hipEventCreateWithFlags(&st->bounds_ready, hipEventDisableTiming));
        UZ_HIP(hipEventRecord(st->bounds_ready, c->stream));
    }
    // two lists of given-up DNMs: what the first launch leaves for the second (larger arenas), what the second leaves for the HBM build
    st->retry.ensure(2 * ((size_t)n + 16));
    int32_t *const retry1_list = st->retry.p, *const retry2_list = st->retry.p + (size_t)n + 16;
    int32_t *const retry1 = st->cursor.p + 16 * (UZ_PHASE_PARTS + 2), *const retry2 = retry1 + 16;
    a.retry_count = retry1; a.retry_list = retry1_list;
    a.from_list = 0; a.cursor_slot = 0; a.src_count = nullptr; a.src_list = nullptr;
    a.status = st->res.p; a.counts = st->res.p + n; a.origin = st->res.p + (size_t)5 * n; a.evidence = st->res.p + (size_t)6 * n;
    a.work_cursor = st->cursor.p;
    a.want_lists = uz_want_lists;
    st->list_start.ensure(n); st->list_len.ensure((size_t)6 * n);
    a.pool_cursor = st->pool_cursor;
    a.list_start = st->list_start.p; a.list_len = st->list_len.p;
#ifdef UZ_PHASE_TIMING
    static DevBuf<unsigned long long> timing;
    timing.ensure(32);
    UZ_HIP(hipMemsetAsync(timing.p, 0, 32 * sizeof(unsigned long long), c->stream));
    a.timing = timing.p;
#endif
    // pinned staging of the per-DNM results (+ the list-pool fill level): everything comes back behind ONE sync
    {
        const size_t need = (size_t)7 * n + 16;
        if (st->res_h_cap < need) {
            if (st->res_h) (void)hipHostFree(st->res_h);
            st->res_h = nullptr;
            st->res_h_cap = need + (size_t)n;
            UZ_HIP(hipHostMalloc((void **)&st->res_h, st->res_h_cap * sizeof(int32_t), hipHostMallocDefault));
        }
    }
    int32_t *const hres = st->res_h;
    unsigned long long *const hused = (unsigned long long *)(hres + (size_t)7 * n + ((7 * (size_t)n) & 1)); // 8-byte aligned slot
    for (int round = 0; round < 2; round++) {
        Sizes z;
        if (speculative) {
            z.caps = st->spec_caps; z.arena = st->spec_arena; z.arena2 = st->spec_arena2;
            z.sumP = (long long)(st->spec_sumP_per_dnm * (double)n) + 4096;
        } else {
            if (bounds_early) UZ_HIP(hipEventSynchronize(st->bounds_ready)); // (else: the speculative run before this one brought the record back)
            check_upload_flags();
            z = exact_sizes(bh_own);
            if (const char *e = getenv("UZ_TEST_CAP_T")) { // test hook: a scratch too small for some DNMs -> they must come back as UZ_ST_CAPACITY
                const int32_t t = (int32_t)atoi(e);
                if (t < z.caps.T) z.caps.T = t;
            }
        }
        const Caps caps = z.caps;
        int arena_used = z.arena;
        // two layouts of a workgroup's scratch region: the arena build's (what that build keeps in HBM: little) for the two arena launches,
        // the HBM build's (every array) for the launch behind them; one buffer serves both, the launches run one after the other
        ScrOff so_hbm;
        const size_t per_wg = uz_scratch_layout(caps, a.so, true), per_wg_hbm = uz_scratch_layout(caps, so_hbm, false);
        if (const char *e = getenv("UZ_TEST_PHASE_ARENA")) { // test hook: an arena (bytes) too small for most DNMs -> they take the HBM build of k_phase
            const int t = atoi(e);
            if (t >= 0 && t < arena_used) arena_used = t;
        }
        int wgs_per_cu;
        {
            static const int wgs_env = [] { const char *e = getenv("UZ_PHASE_WGS_PER_CU"); return e ? atoi(e) : 0; }();
            const int by_lds = (160 * 1024) / (arena_used + (int)sizeof(WgSharedT<1>) + 512);
            const int by_regs = UZ_PHASE_MIN_WAVES * 4 / (WG_NT / 64); // waves per SIMD x four SIMDs / waves per workgroup
            wgs_per_cu = wgs_env > 0 ? wgs_env : std::max(1, std::min(by_lds, by_regs));
            if (arena_env < 0 && wgs_env <= 0) { // all the room this occupancy leaves
                const int room = ((160 * 1024) / wgs_per_cu - (int)sizeof(WgSharedT<1>) - 512) & ~255;
                if (room > arena_used && !getenv("UZ_TEST_PHASE_ARENA")) arena_used = std::min(room, 62 * 1024);
            }
        }
        a.lds_arena_bytes = arena_used;
        int grid = st->n_cus * wgs_per_cu;
        if (grid > n) grid = n;
        const size_t budget = (size_t)8 << 30; // keep the scratch under 8 GiB
        while (grid > 1 && (size_t)grid * per_wg > budget) grid /= 2;
        int grid_hbm = std::min(grid, 8 * st->n_cus); // (the DNMs the arena launches gave up: usually a handful -- eight waves per CU pull them from the list)
        while (grid_hbm > 1 && (size_t)grid_hbm * per_wg_hbm > budget) grid_hbm /= 2;
        st->scratch.ensure(std::max((size_t)grid * per_wg, (size_t)grid_hbm * per_wg_hbm));
        a.scratch = st->scratch.p; a.scratch_per_wg = per_wg; a.caps = caps;
        size_t pool_cap = (size_t)std::min<long long>(4 * z.sumP + 1024, (long long)1 << 31);
        st->pool.ensure(pool_cap);
        a.pool = st->pool.p; a.pool_cap = pool_cap;
        for (int attempt = 0; attempt < 4; attempt++) {
            if (round > 0 || attempt > 0) { // a batch run again (rare): the first run's counts are cleared here; the first run's by k_phase_bounds
                UZ_HIP(hipMemsetAsync(st->cursor.p, 0, cursor_words * sizeof(int32_t), c->stream)); // (cursors + both give-up counts)
                UZ_HIP(hipMemsetAsync(st->pool_cursor, 0, 2 * sizeof(unsigned long long), c->stream));
            }
            {
                // Three launches.  The arena is sized for most of the batch's DNMs, not all (the more DNMs a CU holds, the faster the batch);
                // the rest are redone by a second launch of the same build with arenas for the largest estimate -- a DNM's latency in the
                // arena build is ~100 us, in the HBM build ~450 us, and a list that is worked off behind the main launch costs the batch its
                // slowest DNM -- and only what that launch gives up too (a field width, a chaining level with more than 96 winners) goes to
                // the HBM build.
                ProfScope ps(c, UZ_K_PHASE);
                UZ_TRACE("k_phase");
                hipLaunchKernelGGL((k_phase<true>), dim3((unsigned)grid), dim3(WG_NT), (size_t)a.lds_arena_bytes, c->stream, a);
                UZ_HIP(hipGetLastError());
                PhaseArgs a2 = a;
                a2.from_list = 1; a2.cursor_slot = UZ_PHASE_PARTS; a2.src_count = retry1; a2.src_list = retry1_list;
                a2.retry_count = retry2; a2.retry_list = retry2_list;
                a2.lds_arena_bytes = getenv("UZ_TEST_PHASE_ARENA") ? arena_used /* test hook: the small arena again, so that the HBM build is what runs */
                                                                    : std::max(arena_used, std::min(z.arena2, 62 * 1024));
                const int per_cu2 = std::max(1, (160 * 1024) / (a2.lds_arena_bytes + (int)sizeof(WgSharedT<1>) + 512));
                hipLaunchKernelGGL((k_phase<true>), dim3((unsigned)std::min(grid, per_cu2 * st->n_cus)), dim3(WG_NT), (size_t)a2.lds_arena_bytes, c->stream, a2);
                UZ_HIP(hipGetLastError());
                PhaseArgs a3 = a2;
                a3.cursor_slot = UZ_PHASE_PARTS + 1; a3.src_count = retry2; a3.src_list = retry2_list;
                a3.so = so_hbm; a3.scratch_per_wg = per_wg_hbm;
                hipLaunchKernelGGL((k_phase<false>), dim3((unsigned)grid_hbm), dim3(WG_NT), 0, c->stream, a3);
                UZ_HIP(hipGetLastError());
            }
            UZ_TRACE("after k_phase");
            *hused = 0;
            int32_t *const hretry = (int32_t *)(hused + 1);
            *hretry = 0;
            // ONE copy launch: the results with the pool's fill level, the DNMs that took the HBM build, and (speculative run) the reduced record
            const KCopySeg back[3] = {{hres, st->res.p, res_ints * sizeof(int32_t) + sizeof(unsigned long long)},
                                      {hretry, retry2, sizeof(int32_t)},
                                      {st->bounds_h, st->bounds_red.p, speculative ? sizeof(BoundsRed) : 0}};
            uz_kcopy_many(c, back, 3);
            if (defer && speculative) { // uz_phase_begin: the run stays in flight; uz_finish_phase waits for it and judges it
                st->pending = true;
                st->pend_caps = caps; st->pend_pool_cap = a.pool_cap; st->pend_want_lists = a.want_lists;
                return;
            }
            if (host_trace) t_queued = host_us();
            UZ_HIP(hipStreamSynchronize(c->stream));
            if (host_trace) t_synced = host_us();
            if (speculative) check_upload_flags();
            if (c->hflags[1]) {
                const int f = c->hflags[1];
                c->hflags[1] = 0;
                throw UzError{UZ_E_STATE, f == 4 ? "the read stage asked for a base of a record whose bases were staged as a list (bl_*), and the list does not hold it: the fetch points that staged the table do not cover this batch"
                                        : f == 3 ? "the read stage asked for a base (or its quality bit) in a 32-base unit that was not staged (umask): the fetch points that staged the table do not cover this batch"
                                        : f == 2 ? "the read stage asked for a base-quality bit of a record staged without its quality row (more than 10 low-quality bases, or no bases): such a record can never pass goodread -- the staging rule and the kernel disagree"
                                                 : "the read stage asked for the bases of a record staged without them (UZ_AUX_NO_SEQ): the selection that staged the table does not cover this batch's fetches"};
            }
            const unsigned long long used = *hused;
            c->prof[UZ_K_PHASE].last_units = (int64_t)*(const int32_t *)(hused + 1); // DNMs that took the HBM build
            if (!a.want_lists || used <= a.pool_cap) break;
            // list pool too small: grow to the exact demand and run again
            pool_cap = (size_t)used + 1024;
            st->pool.ensure(pool_cap);
            a.pool = st->pool.p; a.pool_cap = pool_cap;
        }
        // what the batch really needed: the next batch's assumption -- and the verdict on this one's
        const Sizes real = exact_sizes(bh_own);
        if (host_trace) t_sized = host_us();
        // (head room costs scratch, and a scratch that outgrows its budget halves the grid: an eighth on the linear sizes, none on the
        // pair table -- its capacity is a power of two already)
        auto room = [](int32_t v) { return (int32_t)std::min<long long>((long long)v + v / 8 + 8, 0x3FFFFFFF); };
        st->spec_caps.A = room(real.caps.A); st->spec_caps.T = room(real.caps.T); st->spec_caps.H = room(real.caps.H); st->spec_caps.C = room(real.caps.C);
        st->spec_caps.I = 4 * st->spec_caps.A;
        st->spec_caps.M = real.caps.M;
        st->spec_arena = real.arena; st->spec_arena2 = real.arena2;
        st->spec_sumP_per_dnm = 1.25 * (double)real.sumP / (double)n;
        st->spec_valid = true;
        static const bool spec_log = getenv("UZ_PHASE_SPEC_LOG") != nullptr; // development aid
        if (spec_log)
            fprintf(stderr, "[uz_launch_phase] n %d speculative %d caps A %d T %d H %d C %d M %d arena %d grid %d per_wg %zu pool %zu | real A %d T %d H %d C %d M %d arena %d\n", n,
                    (int)speculative, caps.A, caps.T, caps.H, caps.C, caps.M, arena_used, grid, per_wg, pool_cap, real.caps.A, real.caps.T, real.caps.H, real.caps.C, real.caps.M, real.arena);
        if (!speculative) break;
        const bool fits = real.caps.A <= caps.A && real.caps.T <= caps.T && real.caps.H <= caps.H && real.caps.C <= caps.C && real.caps.M <= caps.M;
        st->spec_runs++;
        if (fits) break;
        st->spec_misses++;
        speculative = false; // the batch outgrew the assumption: once more, on its own sizes
    }
#ifdef UZ_PHASE_TIMING
    {
        unsigned long long t[32];
        UZ_HIP(hipMemcpy(t, timing.p, sizeof(t), hipMemcpyDeviceToHost));
        const char *nm[17] = {"A.classify", "A.lists+C", "-", "B.overlap", "B.finish", "S.keys", "S.sort", "P.count", "P.scatter", "P.pairs", "D.finder",
                              "E.setup", "E.expand", "E.winners", "E.frontier", "F.join", "F.count"};
        unsigned long long tot = 0;
        for (int k = 0; k < 17; k++) tot += t[k];
        fprintf(stderr, "[phase timing]");
        for (int k = 0; k < 17; k++) fprintf(stderr, " %s %.1f%%", nm[k], 100.0 * (double)t[k] / (double)(tot ? tot : 1));
        fprintf(stderr, " | ticks/DNM %.0f\n", (double)tot / n);
    }
#endif
    if (status) memcpy(status, hres, (size_t)n * sizeof(int32_t));
    if (counts) memcpy(counts, hres + n, (size_t)4 * n * sizeof(int32_t));
    if (origin) memcpy(origin, hres + (size_t)5 * n, (size_t)n * sizeof(int32_t));
    if (evidence) memcpy(evidence, hres + (size_t)6 * n, (size_t)n * sizeof(int32_t));
    st->have_lists = a.want_lists != 0;
    c->phase_valid = true;
    if (host_trace)
        fprintf(stderr, "[uz] uz_launch_phase, host us: everything queued %.0f | waited for the device %.0f | exact sizes %.0f | results copied out %.0f\n", t_queued, t_synced - t_queued,
                t_sized - t_synced, host_us() - t_sized);
}

// second half of uz_phase_begin / uz_phase_end: waits for the run uz_launch_phase(defer) left in flight (or finds the results of a run
// that had to be synchronous) and hands the results out.  false: the batch outgrew the sizes it was run on (or its list pool) and
// must be run again, whole -- the caller does that with PhaseState::force_exact set.
bool uz_finish_phase(uz_ctx *c, int32_t *status, int32_t *counts, int32_t *origin, int32_t *evidence) {
    PhaseState *st = (PhaseState *)c->phase_state;
    UZ_REQUIRE(st != nullptr, UZ_E_STATE, "uz_phase_end without uz_phase_begin");
    const int32_t n = st->n;
    if (n <= 0) { c->phase_valid = true; return true; }
    int32_t *const hres = st->res_h;
    if (st->pending) {
        st->pending = false;
        UZ_HIP(hipStreamSynchronize(c->stream));
        uz_check_upload_flag(c);
        if (c->hflags[1]) {
            c->hflags[1] = 0;
            st->force_exact = true; // (the whole run states the error in full)
            return false;
        }
        unsigned long long *const hused = (unsigned long long *)(hres + (size_t)7 * n + ((7 * (size_t)n) & 1));
        const unsigned long long used = *hused;
        c->prof[UZ_K_PHASE].last_units = (int64_t)*(const int32_t *)(hused + 1);
        const Sizes real = phase_exact_sizes(reinterpret_cast<const BoundsRed *>(st->bounds_h), n);
        auto room = [](int32_t v) { return (int32_t)std::min<long long>((long long)v + v / 8 + 8, 0x3FFFFFFF); };
        st->spec_caps.A = room(real.caps.A); st->spec_caps.T = room(real.caps.T); st->spec_caps.H = room(real.caps.H); st->spec_caps.C = room(real.caps.C);
        st->spec_caps.I = 4 * st->spec_caps.A;
        st->spec_caps.M = real.caps.M;
        st->spec_arena = real.arena; st->spec_arena2 = real.arena2;
        st->spec_sumP_per_dnm = 1.25 * (double)real.sumP / (double)n;
        const Caps &caps = st->pend_caps;
        const bool fits = real.caps.A <= caps.A && real.caps.T <= caps.T && real.caps.H <= caps.H && real.caps.C <= caps.C && real.caps.M <= caps.M;
        st->spec_runs++;
        if (!fits) st->spec_misses++;
        if (!fits || (st->pend_want_lists && used > st->pend_pool_cap)) { st->force_exact = true; return false; }
        st->have_lists = st->pend_want_lists != 0;
    }
    if (status) memcpy(status, hres, (size_t)n * sizeof(int32_t));
    if (counts) memcpy(counts, hres + n, (size_t)4 * n * sizeof(int32_t));
    if (origin) memcpy(origin, hres + (size_t)5 * n, (size_t)n * sizeof(int32_t));
    if (evidence) memcpy(evidence, hres + (size_t)6 * n, (size_t)n * sizeof(int32_t));
    c->phase_valid = true;
    return true;
}

static void fetch_list_index(uz_ctx *c, PhaseState *st) {
    const size_t n = (size_t)st->n;
    st->list_start_h.resize(n);
    st->list_len_h.resize(6 * n);
    if (!n) return;
    UZ_HIP(hipMemcpyAsync(st->list_start_h.data(), st->list_start.p, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    UZ_HIP(hipMemcpyAsync(st->list_len_h.data(), st->list_len.p, 6 * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    UZ_HIP(hipStreamSynchronize(c->stream));
}

// gathers lists [k0, k1) of every DNM (k in the 6-list layout) into CSR form
static int gather_lists(uz_ctx *c, int k0, int k1, int64_t *off, int32_t *val) {
    PhaseState *st = (PhaseState *)c->phase_state;
    UZ_REQUIRE(st && st->have_lists, UZ_E_STATE, "no lists kept by the last uz_phase");
    fetch_list_index(c, st);
    const int nk = k1 - k0;
    int64_t total = 0;
    for (int32_t d = 0; d < st->n; d++)
        for (int k = 0; k < nk; k++) {
            off[(size_t)nk * d + k] = total;
            if (st->list_start_h[d] >= 0) total += st->list_len_h[(size_t)6 * d + k0 + k];
        }
    off[(size_t)nk * st->n] = total;
    if (!val || total == 0) return 0;
    // copy the used part of the pool once, then slice on the host
    unsigned long long used = 0;
    UZ_HIP(hipMemcpy(&used, st->pool_cursor, sizeof(used), hipMemcpyDeviceToHost));
    std::vector<int32_t> pool((size_t)used);
    if (used) UZ_HIP(hipMemcpy(pool.data(), st->pool.p, (size_t)used * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t d = 0; d < st->n; d++) {
        if (st->list_start_h[d] < 0) continue;
        long long src = st->list_start_h[d];
        for (int k = 0; k < 6; k++) {
            const int len = st->list_len_h[(size_t)6 * d + k];
            if (k >= k0 && k < k1 && len) {
                int32_t *out = val + off[(size_t)nk * d + (k - k0)];
                memcpy(out, pool.data() + src, (size_t)len * sizeof(int32_t));
                // cohort batches: query-name ids (lists 0, 1, 4, 5) are handed back relative to the kid's own table
                if (k != 2 && k != 3 && !c->phase_qbase.empty())
                    for (int x = 0; x < len; x++) out[x] -= (int32_t)c->phase_qbase[(size_t)d];
            }
            src += len;
        }
    }
    return 0;
}

// test hook (unfazed_hip.h: uz_phase_sizing_fetch): what the sizing pass of the last batch left.  k_phase_bounds and k_bounds_reduce are the only
// writers of these buffers -- k_phase reads pre_win / pre_ha / pre_hl, the host reads the pinned copy of the reduced record -- so they still hold
// the pass's output when the batch's call has returned.
int uz_phase_sizing_fetch_impl(uz_ctx *c, int32_t *bounds, int32_t *pre_win, int32_t *pre_ha, int32_t *pre_hl, int64_t *reduced) {
    PhaseState *st = (PhaseState *)c->phase_state;
    UZ_REQUIRE(st != nullptr && !st->pending, UZ_E_STATE, "uz_phase_sizing_fetch: no finished batch on this context");
    const size_t n = (size_t)(st->n > 0 ? st->n : 0), nh = (size_t)st->n_het;
    if (reduced) memset(reduced, 0, UZ_SIZING_REDUCED_WORDS * sizeof(int64_t));
    if (!n) return 0;
    UZ_HIP(hipStreamSynchronize(c->stream));
    if (bounds) UZ_HIP(hipMemcpy(bounds, st->bounds.p, 5 * n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pre_win) UZ_HIP(hipMemcpy(pre_win, st->pre_win.p, 4 * n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pre_ha && nh) UZ_HIP(hipMemcpy(pre_ha, st->pre_h.p, nh * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pre_hl && nh) UZ_HIP(hipMemcpy(pre_hl, st->pre_h.p + nh + 1, nh * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (reduced) { // from the device's record, not the host's pinned copy of it
        BoundsRed br;
        UZ_HIP(hipMemcpy(&br, st->bounds_red.p, sizeof(br), hipMemcpyDeviceToHost));
        reduced[0] = br.mA; reduced[1] = br.mT; reduced[2] = br.mH; reduced[3] = br.mC; reduced[4] = br.active;
        reduced[5] = (int64_t)br.mM; reduced[6] = (int64_t)br.sumP;
        for (int k = 0; k < 256; k++) reduced[7 + k] = br.hist[k];
    }
    return 0;
}

// uz_bed_rows reads the batch's result where it lies: the per-DNM results in `res` (status [n], counts [4 n]) and, when the batch kept its lists,
// the pool with its index
void uz_phase_lists_dev(uz_ctx *c, int32_t *n, const int32_t **status, const int32_t **counts, const int32_t **pool, const long long **list_start,
                        const int32_t **list_len) {
    PhaseState *st = (PhaseState *)c->phase_state;
    UZ_REQUIRE(c->phase_valid && !c->phase_open && st != nullptr && !st->pending, UZ_E_STATE, "no finished batch on this context");
    *n = st->n > 0 ? st->n : 0;
    *status = st->res.p; *counts = st->res.p ? st->res.p + (size_t)*n : nullptr;
    *pool = st->have_lists ? st->pool.p : nullptr;
    *list_start = st->have_lists ? st->list_start.p : nullptr;
    *list_len = st->have_lists ? st->list_len.p : nullptr;
}

int uz_phase_votes_impl(uz_ctx *c, int64_t *vote_off, int32_t *vote_val) { return gather_lists(c, 0, 4, vote_off, vote_val); }
int uz_phase_groups_impl(uz_ctx *c, int64_t *grp_off, int32_t *grp_q) { return gather_lists(c, 4, 6, grp_off, grp_q); }
