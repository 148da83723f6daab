// walk_book.hpp -- the device slots of walked batches (uz_ctx::WalkSlot): the ONE table of their buffers, and the book that says which slot is
// held, how large every kind of buffer has been asked for and which outgrown blocks wait to be freed.  No HIP in here: the lists only name the
// buffers (uz_ctx.hpp declares them, abi.hip releases and reserves them, every grow site names one), and the book only keeps numbers and pointers
// -- tests/walk_book_main.cpp builds it with a host compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "uz_bamwalk.h"

// X(element type, name): the DevBuf members of uz_ctx::WalkSlot (uz_bam_walk, uz_bam_walk_fetch; desc_kept is also the joins' descriptor list)
#define UZ_WALK_BUFS(X)                                                                                                                               \
    X(uint8_t, comp) X(uint8_t, out) X(int64_t, in_off) X(int64_t, out_off) X(int64_t, blk_coff) X(int32_t, task) X(int64_t, span) X(int32_t, reach)  \
    X(int32_t, fetch) X(int64_t, count) X(int64_t, first) X(int64_t, walked) X(int32_t, flags) X(int64_t, n_direct) X(int64_t, tab_first)            \
    X(int64_t, kcount) X(int64_t, kfirst) X(int32_t, iflags) X(uint32_t, blk_crc) X(uz_walk_desc, desc) X(unsigned long long, tab)                   \
    X(uz_walk_desc, desc_kept) X(uz_walk_file, tfile)
// ... and of uz_ctx::WalkSlot::Join (k_bamjoin.hip: uz_join_run; look_tid is its scratch for the host's answers)
#define UZ_JOIN_BUFS(X)                                                                                                                               \
    X(uint8_t, tmp) X(int32_t, jtask) X(int32_t, keep) X(int32_t, mate) X(int32_t, target) X(unsigned long long, hkey_in) X(uint32_t, hval_in)       \
    X(unsigned long long, hkey) X(uint32_t, hperm) X(uint32_t, inv) X(uint32_t, front0) X(uint32_t, front1) X(uint32_t, need) X(int32_t, cnt)        \
    X(uint8_t, aux) X(int32_t, jt_tid) X(int64_t, reach_key) X(int32_t, reach_a) X(int32_t, reach_host) X(int32_t, h_flags) X(int32_t, look_tid)     \
    X(uz_need_rec, need_rec) X(unsigned long long, fkey_in) X(unsigned long long, fkey) X(uint32_t, fval_in) X(uint32_t, fidx) X(uint32_t, first)    \
    X(uint32_t, runid) X(uint32_t, pos_of_k) X(uint32_t, fo) X(int32_t, gidx) X(uint8_t, s5_in) X(uint8_t, s5_out) X(uz_kept_rec, kept)              \
    X(uint32_t, name_rec) X(unsigned long long, ccount) X(int32_t, cspan) X(int64_t, totals)

// which high-water mark of the book a buffer grows by: one per entry of the two lists
enum WalkKind : int {
#define UZ_X(T, name) WK_##name,
    UZ_WALK_BUFS(UZ_X)
#undef UZ_X
#define UZ_X(T, name) JK_##name,
    UZ_JOIN_BUFS(UZ_X)
#undef UZ_X
    WALK_KIND_COUNT
};

struct WalkBook {
    static constexpr int SLOTS = 4;
    static constexpr size_t DRAIN_ABOVE = (size_t)24 << 30; // parked bytes worth a device-wide wait (hipFree) at a moment no batch is in flight
    struct Caps { size_t out = 0, comp = 0, desc = 0; };    // the large buffers of a slot, in elements

    // The slot of a batch, among the free ones: one whose large buffers already hold it -- the smallest such (best fit) --, else the first that has
    // never been used, else the smallest (it is grown to the largest sizes ANY batch of the context has asked for: a slot grows once).  -1: all busy.
    static int choose(const bool busy[SLOTS], const Caps caps[SLOTS], size_t need_out, size_t need_comp, size_t need_desc) {
        int fit = -1, fresh = -1, small = -1;
        for (int i = 0; i < SLOTS; i++) {
            if (busy[i]) continue;
            const Caps &s = caps[i];
            if (s.out >= need_out && s.comp >= need_comp && s.desc >= need_desc) { if (fit < 0 || s.out < caps[fit].out) fit = i; }
            else if (s.out == 0) { if (fresh < 0) fresh = i; }
            else if (small < 0 || s.out < caps[small].out) small = i;
        }
        return fit >= 0 ? fit : fresh >= 0 ? fresh : small;
    }

    // Takes a slot (-1: none free).  caps_of(i) is asked for free slots only, under the lock: a slot's buffers belong to whoever holds it.
    // Nothing of an earlier batch in flight and a lot parked: the parked blocks are handed over in `to_free` (the caller frees them).
    template <typename F>
    int claim(F &&caps_of, size_t need_out, size_t need_comp, size_t need_desc, std::vector<void *> &to_free) {
        std::lock_guard<std::mutex> lk(mu);
        Caps caps[SLOTS];
        bool any_busy = false;
        for (int i = 0; i < SLOTS; i++) {
            if (busy[i]) any_busy = true;
            else caps[i] = caps_of(i);
        }
        const int k = choose(busy, caps, need_out, need_comp, need_desc);
        if (k < 0) return -1;
        busy[k] = true;
        if (!any_busy && parked_bytes() > DRAIN_ABOVE) {
            for (auto &b : park) to_free.push_back(b.first);
            park.clear();
        }
        return k;
    }
    bool claim_slot(int k) { // this very slot, if it is free (uz_walk_reserve)
        std::lock_guard<std::mutex> lk(mu);
        if (busy[k]) return false;
        return busy[k] = true;
    }
    void release(int k) { std::lock_guard<std::mutex> lk(mu); busy[k] = false; }
    bool held(int k) { std::lock_guard<std::mutex> lk(mu); return busy[k]; }
    // the largest request a kind of buffer has seen, this one included
    size_t note(int kind, size_t n) {
        std::lock_guard<std::mutex> lk(mu);
        if (n > hi[kind]) hi[kind] = n;
        return hi[kind];
    }
    // a buffer of a slot was allocated anew; `old` (null: none): the block it outgrew, kept until a drain or the context's end
    void grew(void *old, size_t old_bytes) {
        std::lock_guard<std::mutex> lk(mu);
        allocs++;
        if (old) park.push_back({old, old_bytes});
    }
    void stats(int64_t *n_allocs, int64_t *n_parked, int64_t *bytes_parked) { // (uz_walk_slot_stats)
        std::lock_guard<std::mutex> lk(mu);
        *n_allocs = allocs; *n_parked = (int64_t)park.size(); *bytes_parked = (int64_t)parked_bytes();
    }
    std::vector<void *> take_parked() { // every parked block, to be freed by the caller (uz_destroy)
        std::lock_guard<std::mutex> lk(mu);
        std::vector<void *> v;
        for (auto &b : park) v.push_back(b.first);
        park.clear();
        return v;
    }

    std::mutex mu; // guards everything below (walks and joins of different slots run on different decoder threads)
    bool busy[SLOTS] = {false, false, false, false};
    size_t hi[WALK_KIND_COUNT] = {0};
    std::vector<std::pair<void *, size_t>> park; // (block, bytes)
    int64_t allocs = 0; // device allocations the slots have made (a process whose batches stopped growing makes none)

private:
    size_t parked_bytes() const {
        size_t s = 0;
        for (auto &b : park) s += b.second;
        return s;
    }
};
