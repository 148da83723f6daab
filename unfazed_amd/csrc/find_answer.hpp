// find_answer.hpp -- layout of the block uz_find_answer fills (unfazed_hip.h): ONE statement of it for the kernel that writes the block
// (k_sites.hip: k_find_answer), the host that sizes and reads it, and the stand-alone check (tests/find_answer_main.cpp).  Plain C++: no HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define UZ_FA_HD __host__ __device__
#else
#define UZ_FA_HD
#endif

#define UZ_FA_PARTS 6  // header, cand_off, het_off, cand_idx, cand_flags, het_idx
#define UZ_FA_ALIGN 256
#define UZ_FA_HEAD_WORDS 8 // int64: n_cand, n_het, fits, bytes needed, n; the rest 0

struct FindAnswerLayout {
    uint64_t off[UZ_FA_PARTS];   // where each part starts in the block (multiples of UZ_FA_ALIGN)
    uint64_t bytes[UZ_FA_PARTS]; // its payload
    uint64_t total;              // the block's bytes: the last part's end, rounded up like every part
};

UZ_FA_HD inline uint64_t uz_fa_up(uint64_t v) { return (v + (UZ_FA_ALIGN - 1)) & ~(uint64_t)(UZ_FA_ALIGN - 1); }

// n DNMs, n_cand candidate sites, n_het het sites (all >= 0)
UZ_FA_HD inline FindAnswerLayout uz_find_answer_layout(int64_t n, int64_t n_cand, int64_t n_het) {
    FindAnswerLayout L;
    L.bytes[0] = UZ_FA_HEAD_WORDS * sizeof(int64_t);
    L.bytes[1] = L.bytes[2] = ((uint64_t)n + 1) * sizeof(int64_t);
    L.bytes[3] = (uint64_t)n_cand * sizeof(int32_t);
    L.bytes[4] = (uint64_t)n_cand;
    L.bytes[5] = (uint64_t)n_het * sizeof(int32_t);
    uint64_t at = 0;
    for (int k = 0; k < UZ_FA_PARTS; k++) { L.off[k] = at; at += uz_fa_up(L.bytes[k]); }
    L.total = at;
    return L;
}
// the block holds the whole answer
UZ_FA_HD inline bool uz_find_answer_fits(const FindAnswerLayout &L, uint64_t block_bytes) { return L.total <= block_bytes; }
// the block holds the parts whose size the host knows before the find has run: the header and the two offset columns
UZ_FA_HD inline bool uz_find_answer_fits_offsets(const FindAnswerLayout &L, uint64_t block_bytes) { return L.off[3] <= block_bytes; }
