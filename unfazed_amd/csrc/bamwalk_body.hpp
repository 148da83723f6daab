// bamwalk_body.hpp -- k_bam_walk's body (csrc/k_bamwalk.hip states what it does), included once per build of the kernel:
//   UZ_WALK_KERNEL k_bam_walk,      UZ_WALK_MANY 0   the walk of one file's blocks: the tokens below are then exactly the single-file kernel's
//   UZ_WALK_KERNEL k_bam_walk_many, UZ_WALK_MANY 1   the blocks of many files laid end to end as one (uz_bamwalk.h: uz_walk_file; unfazed_io.h:
//                                                    uz_bamsrc_open_many).  tf [n_tasks] names the file of every walk task: a record's refID and
//                                                    next_refID are moved into the set's numbering where they are read (one the file's header does
//                                                    not know becomes INT32_MAX: no reference of the set), its name hashes are salted where they
//                                                    are written.
// No include guard on purpose.
#if UZ_WALK_MANY
#define UZ_WALK_FILE_PARAM , const uz_walk_file *__restrict__ tf
#define UZ_WALK_REF(r) walk_set_ref((r), ref_base, n_ref_f)
#define UZ_WALK_SALT1 ^ salt1
#define UZ_WALK_SALT2 ^ salt2
#else
#define UZ_WALK_FILE_PARAM
#define UZ_WALK_REF(r) (r)
#define UZ_WALK_SALT1
#define UZ_WALK_SALT2
#endif
__global__ __launch_bounds__(64) void UZ_WALK_KERNEL(WalkArgs a UZ_WALK_FILE_PARAM) {
    constexpr bool FILL = true;
    __shared__ uint4 win[WIN / 16];
    __shared__ uint16_t offs[WIN_RECS];
    __shared__ int s_n, s_state;
    __shared__ long long s_next;
    // the task's fetches and reach intervals, searched once per record: in LDS when they fit (they do unless a task holds thousands of fetches)
    constexpr int FCAP = 1024, RCAP = 256;
    __shared__ int32_t f_lo[FCAP], f_hi[FCAP], r_a[RCAP], r_b[RCAP];
    const int t = blockIdx.x, lane = threadIdx.x;
    const int32_t *tc = a.task + UZ_WALK_TASK_COLS * (size_t)t;
    const int32_t tid = tc[0], tb = tc[1], sp0 = tc[2], sp1 = tc[3], r0 = tc[4], r1 = tc[5], f0 = tc[6], f1 = tc[7], max_len = tc[8];
    const uint8_t *win8 = reinterpret_cast<const uint8_t *>(win);
    const bool f_lds = f1 - f0 <= FCAP, r_lds = r1 - r0 <= RCAP;
#if UZ_WALK_MANY
    // the task's file: the same for the whole wavefront, read through the scalar cache and held in scalar registers
    const int32_t ref_base = __builtin_amdgcn_readfirstlane(tf[t].ref_base), n_ref_f = __builtin_amdgcn_readfirstlane(tf[t].n_ref);
    const uint32_t salt2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tf[t].salt2);
    const uint64_t salt1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tf[t].salt1 >> 32)) << 32) |
                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tf[t].salt1);
#endif
    if (f_lds) for (int i = lane; i < f1 - f0; i += 64) { f_lo[i] = a.fetch[3 * (f0 + i)]; f_hi[i] = a.fetch[3 * (f0 + i) + 1]; }
    if (r_lds) for (int i = lane; i < r1 - r0; i += 64) { r_a[i] = a.reach[2 * (r0 + i)]; r_b[i] = a.reach[2 * (r0 + i) + 1]; }
    __syncthreads();
    int64_t n_out = 0, walked = 0, n_dir = 0;
    int flag = 0;
    bool stop = false;
    for (int sp = sp0; sp < sp1 && !stop && !flag; sp++) {
        const int64_t *sc = a.span + UZ_WALK_SPAN_COLS * (size_t)sp;
        const uint64_t span_end = (uint64_t)sc[1];
        int64_t cur = sc[2];
        const int64_t bend = sc[3], blk0 = sc[4], blk1 = sc[5];
        if (blk0 >= blk1) { stop = true; break; } // no block at the span's start: the end of the file (the host's walk stops there too)
        bool span_done = false;
        int64_t bi_cur = blk0; // the block that holds `cur` (the cursor only moves forward: a step or none per window)
        while (!span_done) {
            while (bi_cur + 1 < blk1 && a.blk_at[bi_cur + 1] <= cur) bi_cur++;
            const int64_t w0 = cur & ~(int64_t)15;
#pragma unroll
            for (int it = 0; it < WIN / 16 / 64; it++) {
                const int idx = it * 64 + lane;
                win[idx] = *reinterpret_cast<const uint4 *>(a.buf + w0 + 16 * (int64_t)idx);
            }
            __syncthreads();
            if (lane == 0) { // the chain of block_size fields inside the window
                int k = 0, state = 0; // 0: the window is used up; 1: the gathered bytes end here; 2: ... in the middle of a record; 3: not a record
                int64_t c = cur;
                const int64_t wend = w0 + WIN;
                while (k < WIN_RECS) {
                    if (c + 4 > bend) { state = c >= bend ? 1 : 2; break; }
                    if (c + 4 > wend) break;
                    const int32_t bs = (int32_t)ld32(win8 + (c - w0));
                    if (bs < 32) { state = 3; break; }
                    if (c + 4 + (int64_t)bs > bend) { state = 2; break; }
                    offs[k++] = (uint16_t)(c - w0);
                    c += 4 + (int64_t)bs;
                }
                s_n = k; s_state = state; s_next = c;
            }
            __syncthreads();
            const int n = s_n, state = s_state;
            const int64_t next = s_next;
            int ended = 0; // the kind of the record that ended the walk of this span, 0: none did
            for (int b0 = 0; b0 < n && !ended; b0 += 64) {
                const int j = b0 + lane;
                const bool valid = j < n;
                int kind = K_SKIP;
                bool counted = false;
                int64_t c = 0;
                uint64_t voff = 0;
                int32_t pos = 0, end = 0;
                uint32_t l_name = 0, ncig = 0, fl = 0, lseq = 0, bs = 0;
                const uint8_t *p = a.buf;
                if (valid) {
                    c = w0 + offs[j];
                    bs = ld32(win8 + offs[j]);
                    // the record's own bytes: from the window in LDS when it lies inside it whole (all but the last record or two of a window),
                    // else from where it lies -- every field below is read byte by byte (BAM fields are unaligned)
                    p = (uint32_t)offs[j] + 4u + bs <= (uint32_t)WIN ? win8 + offs[j] + 4 : a.buf + c + 4;
                    // the block that holds the record's first byte: the first whose end lies behind it (an empty block holds nothing)
                    int64_t lo = bi_cur; // (a window reaches into the next block or two at most)
                    while (lo + 1 < blk1 && a.blk_at[lo + 1] <= c) lo++;
                    voff = ((uint64_t)a.blk_coff[lo] << 16) | (uint64_t)(c - a.blk_at[lo]);
                    if (voff >= span_end) kind = K_BREAK;
                    else {
                        const int32_t rt = UZ_WALK_REF((int32_t)ld32(p));
                        pos = (int32_t)ld32(p + 4);
                        if (rt != tid) kind = (rt < 0 || rt > tid) ? K_STOP : K_SKIP;
                        else if (pos >= tb) kind = K_STOP;
                        else {
                            l_name = p[8]; ncig = ld16(p + 12); fl = ld16(p + 14);
                            const int32_t ls = (int32_t)ld32(p + 16);
                            lseq = (uint32_t)ls;
                            if (ls < 0 || ls > 0xFFFF || l_name < 1 || 32 + (uint64_t)l_name + 4 * (uint64_t)ncig > (uint64_t)bs) kind = K_BAD;
                            else {
                                end = endpos_of(p, pos, fl, ncig, l_name);
                                counted = true;
                                // between two reach intervals nothing can be fetched (and a mate position there goes through the index)
                                bool gap;
                                if (r_lds) {
                                    int ri = 0;
                                    while (ri < r1 - r0 && pos >= r_b[ri]) ri++;
                                    gap = ri < r1 - r0 && end <= r_a[ri];
                                } else {
                                    int ri = r0;
                                    while (ri < r1 && pos >= a.reach[2 * ri + 1]) ri++;
                                    gap = ri < r1 && end <= a.reach[2 * ri];
                                }
                                if (gap) kind = K_SKIP;
                                else if (32 + (uint64_t)l_name + 4 * (uint64_t)ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > (uint64_t)bs) kind = K_BAD; // (the host's extract)
                                else kind = K_EMIT;
                            }
                        }
                    }
                }
                const unsigned long long term = __ballot(valid && kind >= K_BREAK);
                const int first = term ? __ffsll((long long)term) - 1 : 64;
                const bool live = valid && lane < first;
                walked += __popcll(__ballot(live && counted));
                const bool emit = live && kind == K_EMIT;
                const unsigned long long m = __ballot(emit);
                // does a fetch return it?  (start < hi and end > lo: read_collector.py:385, :167)
                bool direct = false;
                if (emit) {
                    const int64_t key = (int64_t)pos - max_len;
                    if (f_lds) {
                        int lo = 0, hi = f1 - f0;
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)f_lo[mid] < key) lo = mid + 1; else hi = mid; }
                        for (; lo < f1 - f0 && f_lo[lo] < end; lo++)
                            if (f_hi[lo] > pos) { direct = true; break; }
                    } else {
                        int lo = f0, hi = f1;
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)a.fetch[3 * mid] < key) lo = mid + 1; else hi = mid; }
                        for (; lo < f1 && a.fetch[3 * lo] < end; lo++)
                            if (a.fetch[3 * lo + 1] > pos) { direct = true; break; }
                    }
                }
                n_dir += __popcll(__ballot(direct));
                if (FILL && emit) {
                    const int rank = __popcll(m & ((1ULL << lane) - 1ULL));
                    uz_walk_desc d;
                    d.voff = voff; d.src = (uint64_t)(c + 4);
                    d.h1 = name_hash1(p + 32, l_name - 1) UZ_WALK_SALT1;
                    d.pos = pos; d.end = end; d.tlen = (int32_t)ld32(p + 28); d.mpos = (int32_t)ld32(p + 24); d.mtid = UZ_WALK_REF((int32_t)ld32(p + 20));
                    d.h2 = uz_name_hash2(p + 32, l_name - 1) UZ_WALK_SALT2;
                    d.task = (uint32_t)t;
                    d.flag = (uint16_t)fl; d.l_seq = (uint16_t)lseq; d.n_cigar = (uint16_t)ncig;
                    d.mapq = p[9]; d.l_name = (uint8_t)(l_name - 1); d.direct = direct ? 1 : 0; d.pad8 = 0; d.pad16 = 0;
                    a.out[a.first[t] + n_out + rank] = d;
                }
                n_out += __popcll(m);
                if (first < 64) ended = __shfl(kind, first, 64);
            }
            if (ended == K_BREAK) span_done = true;
            else if (ended == K_STOP) { stop = true; span_done = true; }
            else if (ended == K_BAD || state == 3) { flag |= UZ_WALK_TASK_BAD; span_done = true; }
            else if (state == 1 || state == 2) { flag |= UZ_WALK_TASK_INCOMPLETE; span_done = true; }
            cur = next;
            __syncthreads(); // the window is read to the end before the next one lands
        }
    }
    if (lane == 0) { // (a flagged task goes back to the host: what it wrote into its slice is never looked at)
        a.count[t] = flag ? 0 : n_out; a.n_direct[t] = flag ? 0 : n_dir; a.walked[t] = walked; a.flags[t] = flag;
    }
}
#undef UZ_WALK_FILE_PARAM
#undef UZ_WALK_REF
#undef UZ_WALK_SALT1
#undef UZ_WALK_SALT2
#undef UZ_WALK_KERNEL
#undef UZ_WALK_MANY
