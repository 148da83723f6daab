// walk_book_main.cpp -- the book of the walk slots (unfazed_amd/csrc/walk_book.hpp) on the host, built and run by tests/test_walk_book.py under
// ThreadSanitizer and under AddressSanitizer + UBSan: the claim policy on a hand-written table, the drain signal, and four threads that claim, note
// and release.  Exit status 0: every check held.
#include "walk_book.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <type_traits>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

#define UZ_X(T, name) +1
constexpr int N_WALK = 0 UZ_WALK_BUFS(UZ_X), N_JOIN = 0 UZ_JOIN_BUFS(UZ_X);
#undef UZ_X
static_assert(WALK_KIND_COUNT == N_WALK + N_JOIN, "one kind per entry of the two lists");
static_assert(std::extent<decltype(WalkBook::hi)>::value == WALK_KIND_COUNT, "one high-water mark per kind");
static_assert(std::extent<decltype(WalkBook::busy)>::value == WalkBook::SLOTS, "one flag per slot");
static_assert(WK_comp == 0 && JK_tmp == N_WALK && JK_totals == WALK_KIND_COUNT - 1, "the kinds follow the lists in order");

using Caps = WalkBook::Caps;
static Caps mk(size_t out, size_t comp, size_t desc) { Caps c; c.out = out; c.comp = comp; c.desc = desc; return c; }

struct Table { // the slots' large buffers, as uz_bam_walk shows them to claim()
    Caps caps[WalkBook::SLOTS];
    int asked_busy = 0; // caps_of calls for a slot that was held
};

static int claim(WalkBook &b, Table &t, size_t out, size_t comp, size_t desc, std::vector<void *> *drained = nullptr) {
    std::vector<void *> d;
    const int k = b.claim([&](int i) { if (b.busy[i]) t.asked_busy++; return t.caps[i]; }, out, comp, desc, d); // (under the book's lock: busy[] may be read)
    if (drained) *drained = d;
    else CHECK(d.empty());
    return k;
}

static void policy() {
    WalkBook b;
    Table t;
    t.caps[0] = mk(1000, 1000, 100); t.caps[1] = mk(500, 500, 50); t.caps[2] = mk(0, 0, 0); t.caps[3] = mk(200, 200, 20);
    // fits two free slots: the smaller
    int k = claim(b, t, 400, 400, 40);
    CHECK(k == 1 && b.held(1) && !b.held(0));
    // release, then claim: the same slot
    b.release(1);
    CHECK(!b.held(1) && claim(b, t, 400, 400, 40) == 1);
    // a busy slot is never chosen: the next best fit
    CHECK(claim(b, t, 400, 400, 40) == 0);
    b.release(0); b.release(1);
    // all three buffers must fit: slot 1's descriptors do not hold this one
    CHECK(claim(b, t, 400, 400, 60) == 0);
    b.release(0);
    // fits none: a never-used slot before a used one
    CHECK(claim(b, t, 2000, 10, 10) == 2);
    // fits none and every free slot is used: the smallest
    CHECK(claim(b, t, 2000, 10, 10) == 3);
    CHECK(claim(b, t, 2000, 10, 10) == 1);
    CHECK(claim(b, t, 2000, 10, 10) == 0);
    // all busy
    CHECK(claim(b, t, 1, 1, 1) == -1 && claim(b, t, 2000, 10, 10) == -1);
    for (int i = 0; i < WalkBook::SLOTS; i++) b.release(i);
    t.caps[2] = mk(300, 300, 30);
    CHECK(claim(b, t, 2000, 10, 10) == 3); // (no fresh slot left: the smallest at once)
    b.release(3);
    b.release(3); // (releasing a free slot is legal)
    // every set of busy slots, a batch that fits some and one that fits none: never a busy slot, -1 only when all are busy
    for (int mask = 0; mask < 16; mask++)
        for (size_t need : {(size_t)250, (size_t)5000}) {
            for (int i = 0; i < 4; i++) if (mask >> i & 1) CHECK(b.claim_slot(i));
            k = claim(b, t, need, 1, 1);
            if (mask == 15) CHECK(k == -1);
            else CHECK(k >= 0 && !(mask >> k & 1) && b.held(k));
            bool busy[4]; // the pure function says the same
            for (int i = 0; i < 4; i++) busy[i] = mask >> i & 1;
            CHECK(WalkBook::choose(busy, t.caps, need, 1, 1) == k);
            for (int i = 0; i < 4; i++) b.release(i);
        }
    CHECK(t.asked_busy == 0); // (a held slot's buffers are its holder's: never looked at)
    CHECK(b.claim_slot(0));
    CHECK(!b.claim_slot(0)); // the second claim of one slot is refused
    b.release(0);
}

static void drain() {
    WalkBook b;
    Table t;
    for (auto &c : t.caps) c = mk(100, 100, 100);
    int64_t allocs = 0, blocks = 0, bytes = 0;
    char fake[4]; // (never dereferenced)
    b.grew(nullptr, 0); // a first allocation parks nothing
    b.grew(&fake[0], (size_t)12 << 30);
    b.grew(&fake[1], (size_t)12 << 30);
    b.stats(&allocs, &blocks, &bytes);
    CHECK(allocs == 3 && blocks == 2 && bytes == (int64_t)24 << 30);
    std::vector<void *> d;
    int k = claim(b, t, 1, 1, 1, &d);
    CHECK(k >= 0 && d.empty()); // exactly 24 GiB: not more than the bound
    b.grew(&fake[2], 1);
    int k2 = claim(b, t, 1, 1, 1, &d);
    CHECK(k2 >= 0 && k2 != k && d.empty()); // a slot is busy: never, however much is parked
    b.grew(&fake[3], (size_t)100 << 30);
    b.release(k2);
    k2 = claim(b, t, 1, 1, 1, &d);
    CHECK(k2 >= 0 && d.empty());
    b.release(k2); b.release(k);
    k = claim(b, t, 1, 1, 1, &d); // nothing in flight and more than 24 GiB parked
    CHECK(k >= 0 && d.size() == 4 && d[0] == &fake[0] && d[3] == &fake[3]);
    b.stats(&allocs, &blocks, &bytes);
    CHECK(allocs == 5 && blocks == 0 && bytes == 0);
    b.release(k);
    CHECK(claim(b, t, 1, 1, 1, &d) == k && d.empty()); // drained once
    b.release(k);
    b.grew(&fake[0], 7);
    CHECK(b.take_parked().size() == 1 && b.take_parked().empty());
    // all busy: no slot, and no drain
    b.grew(&fake[0], (size_t)30 << 30);
    for (int i = 0; i < 4; i++) CHECK(b.claim_slot(i));
    CHECK(claim(b, t, 1, 1, 1, &d) == -1 && d.empty());
}

static void marks() {
    WalkBook b;
    CHECK(b.note(WK_out, 0) == 0 && b.note(WK_out, 10) == 10 && b.note(WK_out, 3) == 10 && b.note(WK_out, 0) == 10 && b.note(WK_out, 11) == 11);
    CHECK(b.note(JK_totals, 5) == 5 && b.note(JK_need_rec, 0) == 0 && b.note(WK_comp, 0) == 0);
}

// four threads: claim, grow the slot that was won (its capacities are plain memory, as DevBuf's are), note, release
static constexpr int THREADS = 4, ROUNDS = 10000;
static void threads() {
    WalkBook b;
    Table t;
    std::atomic<int> owners[WalkBook::SLOTS]; // (relaxed: they order nothing -- what keeps two holders apart must be the book's lock)
    for (auto &o : owners) o.store(0);
    std::atomic<int> bad{0};
    static size_t top[THREADS][WALK_KIND_COUNT];
    std::vector<std::thread> th;
    for (int id = 0; id < THREADS; id++)
        th.emplace_back([&, id] {
            uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(id + 1);
            for (int r = 0; r < ROUNDS; r++) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                const size_t n = (size_t)(x >> 40), need = (size_t)(x >> 52);
                const int kind = (int)((x >> 20) % WALK_KIND_COUNT);
                std::vector<void *> d;
                const int k = b.claim([&](int i) { return t.caps[i]; }, need, need, need, d);
                if (k < 0) { bad++; continue; } // (four holders at most, one of them this thread: a slot is always free)
                if (owners[k].fetch_add(1, std::memory_order_relaxed) != 0) bad++;
                if (t.caps[k].out < need) t.caps[k] = mk(need, need, need);
                const size_t hi = b.note(kind, n);
                if (hi < n) bad++;
                if (n > top[id][kind]) top[id][kind] = n;
                if ((r & 1023) == 0) b.grew(&t, 64);
                if (owners[k].fetch_sub(1, std::memory_order_relaxed) != 1) bad++;
                b.release(k);
            }
        });
    for (auto &q : th) q.join();
    CHECK(bad.load() == 0);
    for (int kind = 0; kind < WALK_KIND_COUNT; kind++) {
        size_t want = 0;
        for (int id = 0; id < THREADS; id++) want = top[id][kind] > want ? top[id][kind] : want;
        CHECK(b.note(kind, 0) == want);
    }
    for (int i = 0; i < WalkBook::SLOTS; i++) CHECK(!b.held(i));
    int64_t allocs = 0, blocks = 0, bytes = 0;
    b.stats(&allocs, &blocks, &bytes);
    CHECK(allocs == THREADS * ((ROUNDS + 1023) / 1024) && blocks == allocs && bytes == 64 * allocs);
}

int main() {
    policy();
    drain();
    marks();
    threads();
    puts("walk book ok");
    return 0;
}
