// find_answer_main.cpp -- the layout of a uz_find_answer block (unfazed_amd/csrc/find_answer.hpp: what k_find_answer, its launcher and the
// engine work from) on the CPU, as a program of its own, against a plain recomputation: every size 0 .. 3 of each list, and sizes that put a
// part's payload at 255 / 256 / 257 bytes; offsets, alignment, "fits / does not fit".  Built with -fsanitize=address,undefined by
// tests/test_find_answer_layout.py.
#include <cstdio>
#include <vector>

#include "find_answer.hpp"

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) fprintf(stderr, "line %d: %s (n %lld nc %lld nh %lld)\n", __LINE__, #c, (long long)n, (long long)nc, (long long)nh); } } while (0)

int main() {
    std::vector<long long> ns, lens;
    for (long long v = 0; v <= 3; v++) { ns.push_back(v); lens.push_back(v); }
    for (long long v : {30LL, 31LL, 32LL, 33LL}) ns.push_back(v);                               // 8 (n + 1) = 248, 256, 264, 272
    for (long long v : {63LL, 64LL, 65LL, 255LL, 256LL, 257LL, 1023LL, 1024LL, 1025LL}) lens.push_back(v); // 4 v and v around 256 and 1024
    long long cases = 0;
    for (long long n : ns) for (long long nc : lens) for (long long nh : lens) {
        const FindAnswerLayout L = uz_find_answer_layout(n, nc, nh);
        const unsigned long long payload[6] = {64ull, 8ull * (unsigned long long)(n + 1), 8ull * (unsigned long long)(n + 1), 4ull * (unsigned long long)nc,
                                               (unsigned long long)nc, 4ull * (unsigned long long)nh};
        unsigned long long at = 0;
        for (int k = 0; k < 6; k++) {
            CHECK(L.off[k] == at);
            CHECK(L.off[k] % 256 == 0);
            CHECK(L.bytes[k] == payload[k]);
            unsigned long long room = 0;
            while (room < payload[k]) room += 256; // the plain way up
            at += room;
            CHECK(L.off[k] + L.bytes[k] <= at && at - (L.off[k] + L.bytes[k]) < 256);
        }
        CHECK(L.total == at);
        CHECK(uz_find_answer_fits(L, at) && uz_find_answer_fits(L, at + 1) && !uz_find_answer_fits(L, at - 1) && !uz_find_answer_fits(L, 0));
        for (int k = 0; k < 6; k++) { // a block that ends inside part k or one byte in front of its end holds no whole answer
            if (L.bytes[k]) CHECK(!uz_find_answer_fits(L, L.off[k] + L.bytes[k] - 1));
            if (k < 5) CHECK(uz_find_answer_fits(L, L.off[k + 1]) == (L.off[k + 1] == L.total));
        }
        CHECK(uz_find_answer_fits_offsets(L, L.off[3]) && !uz_find_answer_fits_offsets(L, L.off[3] - 1));
        CHECK(uz_find_answer_layout(n, 0, 0).off[3] == L.off[3]); // what the host knows before the find has run
        cases++;
    }
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    printf("find answer layout ok: %lld cases\n", cases);
    return 0;
}
