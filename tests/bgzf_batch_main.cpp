// bgzf_batch_main.cpp -- the rules of a batch of gathered BGZF blocks (unfazed_amd/csrc/bgzf_batch.hpp) on the host, built and run by
// tests/test_bgzf_batch.py under AddressSanitizer + UBSan: the slicer on the block counts around its two thresholds, the bytes a slice carries,
// the table check with and without the in-order rule, and what is read out of the kernel's flag words.  The tables are heap copies of exactly
// their size: a look past one is the sanitizer's finding.  Exit status 0: every check held.
#include "bgzf_batch.hpp"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

using Vec = std::vector<int64_t>;

static void slicer() {
    // a cut at b when b - cut.back() >= 8192 and n - b >= 4096
    for (int64_t n : {0, 1, 8192, 12287}) CHECK((uz_bgzf_slices(n) == Vec{0, n}));
    CHECK((uz_bgzf_slices(12288) == Vec{0, 8192, 12288}));
    CHECK((uz_bgzf_slices(16384 + 4095) == Vec{0, 8192, 16384 + 4095}));
    CHECK((uz_bgzf_slices(20480) == Vec{0, 8192, 16384, 20480}));
}

static void slice_bytes() {
    {   // streams at 5, 10 and 40 of 64 bytes, a slice each: the framing of block 1 would start below 0
        const Vec in_off{5, 10, 40}, cut{0, 1, 2, 3};
        const UzByteRange r0 = uz_bgzf_slice_bytes(cut, 0, in_off.data(), 64), r1 = uz_bgzf_slice_bytes(cut, 1, in_off.data(), 64),
                          r2 = uz_bgzf_slice_bytes(cut, 2, in_off.data(), 64);
        CHECK(r0.c0 == 0 && r0.c1 == 0);
        CHECK(r1.c0 == 0 && r1.c1 == 22);
        CHECK(r2.c0 == 22 && r2.c1 == 64);
    }
    {   // frames of 30 bytes, as the slicer cuts 20 480 of them: the ranges tile [0, comp_bytes)
        const int64_t n = 20480, comp_bytes = 30 * n;
        Vec in_off((size_t)n);
        for (int64_t k = 0; k < n; k++) in_off[(size_t)k] = 30 * k + 18;
        const Vec cut = uz_bgzf_slices(n);
        const UzByteRange r0 = uz_bgzf_slice_bytes(cut, 0, in_off.data(), comp_bytes), r1 = uz_bgzf_slice_bytes(cut, 1, in_off.data(), comp_bytes),
                          r2 = uz_bgzf_slice_bytes(cut, 2, in_off.data(), comp_bytes);
        CHECK(r0.c0 == 0 && r0.c1 == 30 * 8192 && r1.c0 == r0.c1 && r1.c1 == 30 * 16384 && r2.c0 == r1.c1 && r2.c1 == comp_bytes);
    }
    {   // one slice, whatever the table: everything (the table is not looked at -- a null one here)
        const UzByteRange r = uz_bgzf_slice_bytes(Vec{0, 7}, 0, nullptr, 1000);
        CHECK(r.c0 == 0 && r.c1 == 1000);
    }
}

static int check(const Vec &in_off, const Vec &out_off, int64_t comp_bytes, bool in_order) {
    CHECK(out_off.size() == in_off.size() + 1);
    return uz_bgzf_check_tables((int64_t)in_off.size(), comp_bytes, in_off.data(), out_off.data(), in_order);
}

static void tables() {
    for (bool ord : {false, true}) {
        CHECK(check({18, 60, 90}, {0, 65536, 65536, 65540}, 100, ord) == 0); // a 65536-byte block, a 0-byte block
        CHECK(check({0}, {7, 8}, 1, ord) == 0);
        CHECK(uz_bgzf_check_tables(0, 0, nullptr, nullptr, ord) == 0);
        CHECK(check({-1, 60}, {0, 4, 8}, 100, ord) == UZ_TABLE_BLOCK);
        CHECK(check({18, 100}, {0, 4, 8}, 100, ord) == UZ_TABLE_BLOCK); // in_off == comp_bytes
        CHECK(check({18, 60}, {0, 8, 4}, 100, ord) == UZ_TABLE_BLOCK);  // out_off descends
        CHECK(check({18, 60}, {0, 4, 4 + 65537}, 100, ord) == UZ_TABLE_BLOCK);
        CHECK(check({18, 60}, {-1, 4, 8}, 100, ord) == UZ_TABLE_FIRST);
        CHECK(check({60, 18}, {0, 4, 8}, 100, ord) == (ord ? UZ_TABLE_BLOCK : 0)); // out of file order
        CHECK(check({18, 18}, {0, 4, 8}, 100, ord) == (ord ? UZ_TABLE_BLOCK : 0)); // ... or twice the same
    }
}

static void flags() {
    const Vec cut{0, 8192, 16384, 20480};
    {
        const int32_t f[6] = {5, 0, 9, 0, 3, 0}; // (the cursors say nothing)
        CHECK(uz_bgzf_first_fault(cut, f).block < 0);
    }
    {   // refused blocks in the second and the third slice: the second's, rebased by its first block
        const int32_t f[6] = {0, 0, 0, (7 << 4) | 2, 0, (0 << 4) | 5};
        const UzBlockFault b = uz_bgzf_first_fault(cut, f);
        CHECK(b.block == 8199 && b.code == 2);
        CHECK(uz_bgzf_fault_text(b, true) == "BGZF block 8199 of the batch: not a valid DEFLATE stream of the declared size (code 2)");
        CHECK(uz_bgzf_fault_text(b, false) == "BGZF block 8199: not a valid DEFLATE stream of the declared size (code 2)");
    }
    {   // one launch over the batch: the kernel's own number
        const int32_t f[2] = {0, (12287 << 4) | 15};
        const UzBlockFault b = uz_bgzf_first_fault(Vec{0, 12288}, f);
        CHECK(b.block == 12287 && b.code == 15);
    }
}

int main() {
    static_assert(UZ_BGZF_PAD == 1024 && uz_bgzf_room(10) == 1034, "1 KiB of zeros behind the batch");
    static_assert(uz_bgzf_padded(0) == 1024 && uz_bgzf_padded(1) == 1024 && uz_bgzf_padded(3) == 1024 && uz_bgzf_padded(4) == 1028, "whole dwords, inside the pad");
    slicer();
    slice_bytes();
    tables();
    flags();
    printf("bgzf_batch ok\n");
    return 0;
}
