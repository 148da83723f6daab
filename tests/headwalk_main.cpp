// headwalk_main.cpp -- unfazed_amd/csrc/headwalk.hpp (the bodies k_head_walk and k_head_rank run) on the CPU, as a program of its own:
// tests/test_headwalk.py builds it with g++ -fsanitize=address,undefined and runs it as a child process.  The walk is driven the way the
// kernel drives it -- window by window, 16-byte pieces, one "lane" per listed record -- over heap copies of EXACTLY the stream's size, so a load
// outside the file's bytes is the sanitizer's finding; expected values come from a plain sequential reader.  The selection runs the four passes
// the kernel runs and is held against std::nth_element.  Hand-built cases first, then a seeded fuzz of byte streams and key columns.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "headwalk.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                    \
    } while (0)

struct Walked { int64_t taken = 0, cursor = 0; int state = 0; std::vector<int32_t> tlen; };

static void put32(std::vector<uint8_t> &v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }
static void put_record(std::vector<uint8_t> &v, int32_t block_size, int32_t tlen, size_t body_bytes) { // body_bytes: what really follows the size field
    put32(v, (uint32_t)block_size);
    for (size_t i = 0; i < body_bytes; i++) v.push_back(i >= 28 && i < 32 ? (uint8_t)((uint32_t)tlen >> (8 * (i - 28))) : (uint8_t)(0xA0 + i % 7));
}

// the plain reader: record after record
static Walked reference(const std::vector<uint8_t> &s, int64_t start, int64_t room) {
    Walked w;
    const int64_t len = (int64_t)s.size();
    int64_t c = start;
    for (;;) {
        if (w.taken >= room) { w.state = UZ_HEAD_DONE; break; }
        if (c + 4 > len) { w.state = UZ_HEAD_END; break; }
        int32_t bs;
        memcpy(&bs, s.data() + c, 4);
        if (bs < 32) { w.state = UZ_HEAD_BAD; break; }
        if (c + 4 + (int64_t)bs > len) { w.state = UZ_HEAD_END; break; }
        int32_t t;
        memcpy(&t, s.data() + c + 32, 4);
        w.tlen.push_back(t);
        w.taken++;
        c += 4 + (int64_t)bs;
    }
    w.cursor = c;
    return w;
}

// the kernel's loop.  mis: the bytes' address modulo 16 on the device (the window starts on a 16-byte boundary of the memory)
static Walked windows(const std::vector<uint8_t> &s, int64_t start, int64_t room, unsigned mis) {
    Walked w;
    const int64_t len = (int64_t)s.size();
    uint8_t *bytes = (uint8_t *)malloc(s.size() ? s.size() : 1); // exactly the stream: the sanitizer guards both ends
    if (!s.empty()) memcpy(bytes, s.data(), s.size());
    std::vector<uint8_t> win(UZ_HW_WIN);
    std::vector<uint16_t> offs(UZ_HW_WIN_RECS);
    int64_t cur = start;
    int state = UZ_HEAD_NONE, guard = 0;
    while (state == UZ_HEAD_NONE) {
        const int64_t w0 = cur - (int64_t)(((uint64_t)mis + (uint64_t)cur) & 15u);
        for (int idx = 0; idx < UZ_HW_WIN / 16; idx++) {
            const int64_t p = w0 + 16 * (int64_t)idx;
            if (uz_hw_piece_inside(p, len)) memcpy(win.data() + 16 * idx, bytes + p, 16);
            else uz_hw_piece_edge(bytes, len, p, win.data() + 16 * idx);
        }
        int64_t next;
        const int n = uz_hw_chain(win.data(), w0, cur, len, room - w.taken, offs.data(), &state, &next);
        for (int j = 0; j < n; j++) w.tlen.push_back(uz_hw_tlen(win.data(), offs[(size_t)j], bytes, w0));
        CHECK(n > 0 || state != UZ_HEAD_NONE, "a window made no progress at %lld", (long long)cur);
        if (n == 0 && state == UZ_HEAD_NONE) break;
        w.taken += n; cur = next;
        if (++guard > 1000000) { CHECK(false, "the walk does not end"); break; }
    }
    w.cursor = cur; w.state = state;
    free(bytes);
    return w;
}

static void hold(const char *what, const std::vector<uint8_t> &s, int64_t start, int64_t room) {
    const Walked r = reference(s, start, room);
    for (unsigned mis : {0u, 1u, 7u, 15u}) {
        const Walked w = windows(s, start, room, mis);
        CHECK(w.taken == r.taken && w.cursor == r.cursor && w.state == r.state && w.tlen == r.tlen, "%s (start %lld, room %lld, mis %u): taken %lld / %lld, cursor %lld / %lld, state %d / %d",
              what, (long long)start, (long long)room, mis, (long long)w.taken, (long long)r.taken, (long long)w.cursor, (long long)r.cursor, w.state, r.state);
    }
}

static std::vector<uint8_t> stream_of(int n, std::mt19937_64 &rng, std::vector<int64_t> *starts = nullptr) {
    std::vector<uint8_t> s;
    for (int i = 0; i < n; i++) {
        if (starts) starts->push_back((int64_t)s.size());
        const int32_t bs = 32 + (int32_t)(rng() % 180);
        put_record(s, bs, (int32_t)rng(), (size_t)bs);
    }
    if (starts) starts->push_back((int64_t)s.size());
    return s;
}

static void walk_cases() {
    std::mt19937_64 rng(1);
    for (int R : {0, 1, 2, 200, 201, 5000}) {
        std::vector<int64_t> st;
        const std::vector<uint8_t> s = stream_of(R, rng, &st);
        for (int64_t want : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)R - 1, (int64_t)R, (int64_t)R + 1, (int64_t)R + 5})
            if (want >= 0) hold("whole stream", s, 0, want);
        if (R >= 200) { // the bytes end at a record boundary, inside a block_size field, inside a record's body; and a later round's start
            for (int64_t cut : {st[150], st[150] + 2, st[150] + 4, st[150] + 20, st[151] - 1}) {
                std::vector<uint8_t> t(s.begin(), s.begin() + cut);
                hold("cut stream", t, 0, R);
                hold("cut stream from a later record", t, st[40], R);
            }
            hold("start at the end", s, (int64_t)s.size(), 5);
        }
    }
    { // a block_size below 32 stops the walk where it stands; a negative one too
        for (int32_t bad : {16, 31, 0, -1, INT32_MIN}) {
            std::vector<uint8_t> s = stream_of(30, rng);
            put_record(s, bad, 7, 40);
            std::vector<uint8_t> more = stream_of(5, rng);
            s.insert(s.end(), more.begin(), more.end());
            hold("bad block_size", s, 0, 100);
            hold("bad block_size behind the wanted count", s, 0, 30);
        }
    }
    { // records that straddle the window's end: one longer than the window, one whose tlen straddles it, one whose size field ends with it
        for (int64_t lead : {UZ_HW_WIN - 40, UZ_HW_WIN - 36, UZ_HW_WIN - 33, UZ_HW_WIN - 30, UZ_HW_WIN - 4, UZ_HW_WIN - 3, UZ_HW_WIN - 1, UZ_HW_WIN}) {
            std::vector<uint8_t> s;
            put_record(s, (int32_t)(lead - 4), 11, (size_t)(lead - 4)); // one record up to `lead`
            put_record(s, 3 * UZ_HW_WIN, -22, 3 * UZ_HW_WIN);
            put_record(s, 32, 33, 32);
            hold("straddling records", s, 0, 10);
            s.resize(s.size() - 1);
            hold("straddling records, last byte missing", s, 0, 10);
        }
    }
    { // INT32_MAX as a size: far beyond the bytes
        std::vector<uint8_t> s = stream_of(3, rng);
        put_record(s, INT32_MAX, 1, 64);
        hold("a size beyond the bytes", s, 0, 10);
    }
}

static void walk_fuzz(int rounds) {
    std::mt19937_64 rng(20240611);
    for (int r = 0; r < rounds; r++) {
        std::vector<uint8_t> s;
        std::vector<int64_t> st;
        const int n = (int)(rng() % 400);
        for (int i = 0; i < n; i++) {
            st.push_back((int64_t)s.size());
            const uint64_t kind = rng() % 200;
            if (kind == 0) put_record(s, (int32_t)(rng() % 32) - (rng() % 2 ? 40 : 0), (int32_t)rng(), 40);  // a bad size
            else if (kind == 1) { const int32_t bs = 32 + (int32_t)(rng() % 40000); put_record(s, bs, (int32_t)rng(), (size_t)bs); } // a long record
            else if (kind == 2) put_record(s, 32 + (int32_t)(rng() % 100000), (int32_t)rng(), 32 + rng() % 50); // a size that lies
            else { const int32_t bs = 32 + (int32_t)(rng() % 250); put_record(s, bs, (int32_t)rng(), (size_t)bs); }
        }
        if (rng() % 3 == 0 && !s.empty()) s.resize((size_t)(rng() % s.size()));
        int64_t start = 0;
        if (!st.empty() && rng() % 2) { start = st[(size_t)(rng() % st.size())]; if (start > (int64_t)s.size()) start = (int64_t)s.size(); }
        const int64_t room = (int64_t)(rng() % 500);
        const Walked ref = reference(s, start, room);
        const Walked w = windows(s, start, room, (unsigned)(rng() % 16));
        CHECK(w.taken == ref.taken && w.cursor == ref.cursor && w.state == ref.state && w.tlen == ref.tlen, "walk fuzz %d", r);
    }
}

// the kernel's four passes, one thread
static void select_seq(const std::vector<int32_t> &col, int32_t readlen, int64_t k, uint32_t *a, uint32_t *b) {
    const int64_t n = (int64_t)col.size();
    uint32_t hist[256], prefix = 0, above = 0xFFFFFFFFu;
    uint64_t rank = (uint64_t)k;
    for (int pass = 0; pass < 4; pass++) {
        memset(hist, 0, sizeof(hist));
        for (int64_t i = 0; i < n; i++) {
            const uint32_t key = uz_hw_key(col[(size_t)i], readlen);
            if (uz_hw_sel_in(key, pass, prefix)) hist[uz_hw_sel_digit(key, pass)]++;
            else if (pass == 3 && (key >> 8) > prefix) above = std::min(above, key);
        }
        if (pass < 3) prefix = (prefix << 8) | uz_hw_sel_bin(hist, &rank);
        else uz_hw_sel_last(hist, rank, prefix, k + 1 <= n - 1, above, a, b);
    }
}

static void hold_select(const char *what, const std::vector<int32_t> &col, int32_t readlen) {
    const int64_t n = (int64_t)col.size();
    std::vector<uint64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t d = (int64_t)col[(size_t)i] - 2 * (int64_t)readlen;
        keys[(size_t)i] = (uint64_t)(d < 0 ? -d : d);
        CHECK(keys[(size_t)i] <= 0xFFFFFFFFull && (uint32_t)keys[(size_t)i] == uz_hw_key(col[(size_t)i], readlen), "%s: key %lld", what, (long long)i);
    }
    std::vector<int64_t> ks = {0, n / 2, n - 2, n - 1, (int64_t)((double)(n - 1) * 0.995)};
    for (int64_t k : ks) {
        if (k < 0 || k >= n) continue;
        const int64_t k2 = std::min(k + 1, n - 1);
        std::vector<uint64_t> t = keys;
        std::nth_element(t.begin(), t.begin() + k, t.end());
        const uint64_t wa = t[(size_t)k];
        std::nth_element(t.begin(), t.begin() + k2, t.end());
        const uint64_t wb = t[(size_t)k2];
        uint32_t a = 1, b = 2;
        select_seq(col, readlen, k, &a, &b);
        CHECK(a == wa && b == wb, "%s: n %lld k %lld readlen %d: (%u, %u), expected (%llu, %llu)", what, (long long)n, (long long)k, readlen, a, b,
              (unsigned long long)wa, (unsigned long long)wb);
    }
}

static void select_cases() {
    std::mt19937_64 rng(3);
    for (int n : {1, 2, 3, 201, 202, 5000})
        for (int32_t readlen : {0, 100, 150, (1 << 30) - 1}) {
            std::vector<int32_t> c((size_t)n);
            for (auto &x : c) x = 417;
            hold_select("all equal", c, readlen);
            for (auto &x : c) x = rng() % 2 ? 250 : 9000;
            hold_select("two values", c, readlen);
            for (int i = 0; i < n; i++) c[(size_t)i] = 7 * i - 300;
            hold_select("ascending", c, readlen);
            std::reverse(c.begin(), c.end());
            hold_select("descending", c, readlen);
            for (auto &x : c) x = (int32_t)rng();
            hold_select("random", c, readlen);
            for (auto &x : c) { const uint64_t r = rng() % 3; x = r == 0 ? INT32_MIN : r == 1 ? INT32_MAX : 0; }
            hold_select("extremes", c, readlen);
            for (int i = 0; i < n; i++) c[(size_t)i] = 256 * i + 255; // every key the last of its prefix: the next rank lies above it
            hold_select("one key per prefix", c, 0);
        }
}

static void select_fuzz(int rounds) {
    std::mt19937_64 rng(99);
    for (int r = 0; r < rounds; r++) {
        const int n = 1 + (int)(rng() % 700);
        const int spread = (int)(rng() % 33);
        std::vector<int32_t> c((size_t)n);
        for (auto &x : c) x = (int32_t)((spread == 32 ? rng() : rng() & ((1ull << spread) - 1)) - (rng() % 2 ? (1ull << (spread ? spread - 1 : 0)) : 0));
        hold_select("fuzz", c, (int32_t)(rng() % 400));
    }
}

int main() {
    walk_cases();
    walk_fuzz(3000);
    select_cases();
    select_fuzz(3000);
    if (g_fail) { printf("headwalk: %d failures\n", g_fail); return 1; }
    printf("headwalk ok\n");
    return 0;
}
