// bgzf_batch.hpp -- a batch of gathered BGZF blocks on its way to k_bgzf_inflate: the ONE statement of what its tables must hold, how it is cut
// into slices, which bytes of `comp` a slice carries, how far `comp` is padded on the device and what the kernel's flag words say.  Every route
// that takes blocks up goes by it: uz_bgzf_inflate, uz_bgzf_inflate_to_host (k_inflate.hip), uz_bam_walk (abi.hip), uz_head_walk (k_bamhead.hip),
// all through uz_queue_inflate (k_inflate.hip).  No HIP in here -- tests/bgzf_batch_main.cpp builds it with a host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

// `comp` on the device: the batch's bytes and 1 KiB of zeros behind them (a wave loads the stream 64 dwords at a time, ahead of the bits it
// decodes: its tail reads end in the pad); the kernel is told the padded length, a whole number of dwords
constexpr int64_t uz_bgzf_room(int64_t comp_bytes) { return comp_bytes + 1024; }
constexpr int64_t UZ_BGZF_PAD = uz_bgzf_room(0);
constexpr int64_t uz_bgzf_padded(int64_t comp_bytes) { return uz_bgzf_room(comp_bytes) & ~(int64_t)3; }

// The tables of n_blocks blocks: block k's DEFLATE stream starts at comp[in_off[k]] and inflates to out[out_off[k] .. out_off[k + 1]).
// -> 0, or the rule that is broken: UZ_TABLE_FIRST out_off[0] < 0; UZ_TABLE_BLOCK some block's in_off outside [0, comp_bytes), out_off descending,
// more than 64 KiB of output, or -- in_order: the blocks lie in `comp` in the order of the table (a slice is then one piece of it) -- an in_off
// not above the one before.  The caller words the refusal.
enum { UZ_TABLE_FIRST = 1, UZ_TABLE_BLOCK = 2 };
inline int uz_bgzf_check_tables(int64_t n_blocks, int64_t comp_bytes, const int64_t *in_off, const int64_t *out_off, bool in_order) {
    if (n_blocks <= 0) return 0;
    if (out_off[0] < 0) return UZ_TABLE_FIRST;
    for (int64_t k = 0; k < n_blocks; k++)
        if (!(in_off[k] >= 0 && in_off[k] < comp_bytes && (!in_order || k == 0 || in_off[k] > in_off[k - 1]) && out_off[k] <= out_off[k + 1] &&
              out_off[k + 1] - out_off[k] <= 65536))
            return UZ_TABLE_BLOCK;
    return 0;
}

// A large batch goes up and is inflated in slices, alternating between two streams: slice i + 1 goes up while slice i is inflated (and, on the
// staged route, while its bytes come down: the two directions of the link and the kernel overlap).  -> the first block of every slice and
// n_blocks behind them.  A cut after at least SLICE blocks, while at least half a slice remains.
inline std::vector<int64_t> uz_bgzf_slices(int64_t n_blocks) {
    const int64_t SLICE = 8192; // blocks: a wave is one block's decoder, and the chip holds 6 000 ... 8 000 waves -- a smaller launch leaves slots idle
    std::vector<int64_t> cut{0};
    for (int64_t b = 1; b < n_blocks; b++)
        if (b - cut.back() >= SLICE && n_blocks - b >= SLICE / 2) cut.push_back(b);
    cut.push_back(n_blocks);
    return cut;
}

// The bytes [c0, c1) of `comp` that slice i of `cut` carries (in_order tables).  Whole blocks travel: from the framing of the slice's first block
// -- 18 bytes in front of its stream -- to the framing of the next slice's; the first slice from 0, the last to comp_bytes.
struct UzByteRange { int64_t c0, c1; };
inline UzByteRange uz_bgzf_slice_bytes(const std::vector<int64_t> &cut, size_t i, const int64_t *in_off, int64_t comp_bytes) {
    auto framing = [&](int64_t b) { return std::max<int64_t>(in_off[b] - 18, 0); };
    const int64_t c0 = i == 0 ? 0 : framing(cut[i]);
    return {c0, i + 2 == cut.size() ? comp_bytes : std::max(framing(cut[i + 1]), c0)};
}

// The kernel leaves two words per launch: a cursor, and 0 or (block of the launch << 4 | code of the rule it broke) for one refused block.
// flags: two words per slice of `cut` -> the refused block of the lowest slice that has one, as a block of the batch (block < 0: none)
struct UzBlockFault { int64_t block = -1; int code = 0; };
inline UzBlockFault uz_bgzf_first_fault(const std::vector<int64_t> &cut, const int32_t *flags) {
    for (size_t i = 0; i + 1 < cut.size(); i++)
        if (const int32_t f = flags[2 * i + 1]) return {cut[i] + (f >> 4), f & 15};
    return {};
}
inline std::string uz_bgzf_fault_text(const UzBlockFault &f, bool of_the_batch) {
    return "BGZF block " + std::to_string(f.block) + (of_the_batch ? " of the batch" : "") + ": not a valid DEFLATE stream of the declared size (code " +
           std::to_string(f.code) + ")";
}
