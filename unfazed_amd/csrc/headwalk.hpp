// headwalk.hpp -- the rules of the head walk and of the rank selection behind a kid's insert cutoff (read_collector.py:11-25: the first
// insert_size_max_sample + 1 records of the alignment file, |tlen - 2 readlen|, its 99.5th percentile).  __host__ __device__: k_head_walk and
// k_head_rank (k_bamhead.hip) and tests/headwalk_main.cpp run these very bodies.
//
// The walk.  A file's inflated bytes are bytes[0 .. len).  A window of UZ_HW_WIN bytes starting at w0 (w0 <= cursor, cursor - w0 < 16; w0 may
// lie before the bytes when they start off a 16-byte boundary) is staged 16 bytes at a time: a piece that lies wholly inside [0, len) is one
// 16-byte load, any other piece is read byte by byte and only the bytes inside the range are touched (uz_hw_piece_inside / uz_hw_piece_edge).
// uz_hw_chain then follows the block_size fields inside the window: a record is taken only when its 4 + block_size bytes lie wholly inside
// [0, len).  Its tlen (offset 28 of the fixed part) comes from the window, or -- the record straddles the window's end -- from the bytes
// themselves, which hold the whole record (uz_hw_tlen).
//   UZ_HEAD_DONE  the wanted count was reached
//   UZ_HEAD_END   the bytes ended at a record boundary or inside a record (the cursor stays at that record's start)
//   UZ_HEAD_BAD   a block_size below 32
//
// The selection.  Keys are |tlen - 2 readlen| in 64-bit arithmetic: 32 unsigned bits hold it for every int32 tlen and 0 <= readlen < 2^30.
// A radix select over them, most significant byte first, four passes: pass p counts byte 3 - p of the keys whose higher bytes equal the prefix
// found so far into 256 bins (uz_hw_sel_in / uz_hw_sel_digit), uz_hw_sel_bin picks the bin that holds the rank.  The last pass also keeps the
// smallest key ABOVE the prefix's range, so that the key at the next rank is settled without a fifth pass (uz_hw_sel_last): it is the next
// key of the last histogram, or -- the rank was the last of its prefix -- that smallest key above.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UZ_HW_HD __host__ __device__ __forceinline__
#else
#define UZ_HW_HD inline
#endif

#define UZ_HW_WIN 16384     /* bytes of the stream staged at a time */
#define UZ_HW_WIN_RECS 512  /* record starts listed per window (a record is at least 36 bytes: at most 456 fit) */

#ifndef UZ_HEAD_DONE /* (unfazed_hip.h states them too) */
#define UZ_HEAD_NONE 0 /* of a call: the file had no block in it */
#define UZ_HEAD_DONE 1
#define UZ_HEAD_END 2
#define UZ_HEAD_BAD 3
#endif

UZ_HW_HD uint32_t uz_hw_ld32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the 16-byte piece at offset p of the file's bytes: inside the range whole?
UZ_HW_HD bool uz_hw_piece_inside(int64_t p, int64_t len) { return p >= 0 && p + 16 <= len; }
// ... else: its bytes one by one, zero where the range does not reach
UZ_HW_HD void uz_hw_piece_edge(const uint8_t *bytes, int64_t len, int64_t p, uint8_t out[16]) {
    for (int b = 0; b < 16; b++) {
        const int64_t q = p + b;
        out[b] = (q >= 0 && q < len) ? bytes[q] : (uint8_t)0;
    }
}

// The chain of block_size fields inside the window win[0 .. UZ_HW_WIN) = bytes[w0 .. w0 + UZ_HW_WIN), from the cursor on.  room: records still
// wanted.  -> the records listed (offs[k]: where record k's block_size field starts in the window), *state (UZ_HEAD_NONE: the window is used up,
// go on from *next), *next: the first record not taken.  Every window examines at least one record, for the cursor lies in its first 16 bytes.
UZ_HW_HD int uz_hw_chain(const uint8_t *win, int64_t w0, int64_t cur, int64_t len, int64_t room, uint16_t *offs, int *state, int64_t *next) {
    int k = 0, st = UZ_HEAD_NONE;
    int64_t c = cur;
    const int64_t wend = w0 + UZ_HW_WIN;
    for (;;) {
        if ((int64_t)k >= room) { st = UZ_HEAD_DONE; break; }
        if (c + 4 > len) { st = UZ_HEAD_END; break; }
        if (c + 4 > wend || k >= UZ_HW_WIN_RECS) break;
        const int32_t bs = (int32_t)uz_hw_ld32(win + (c - w0));
        if (bs < 32) { st = UZ_HEAD_BAD; break; }
        if (c + 4 + (int64_t)bs > len) { st = UZ_HEAD_END; break; }
        offs[k++] = (uint16_t)(c - w0);
        c += 4 + (int64_t)bs;
    }
    *state = st; *next = c;
    return k;
}

// tlen of a listed record (the chain has seen that the record lies inside the bytes whole)
UZ_HW_HD int32_t uz_hw_tlen(const uint8_t *win, uint32_t off, const uint8_t *bytes, int64_t w0) {
    return (int32_t)uz_hw_ld32(off + 36u <= (uint32_t)UZ_HW_WIN ? win + off + 32 : bytes + (w0 + (int64_t)off + 32));
}

UZ_HW_HD uint32_t uz_hw_key(int32_t tlen, int32_t readlen) {
    int64_t d = (int64_t)tlen - 2 * (int64_t)readlen;
    if (d < 0) d = -d;
    return (uint32_t)d;
}
UZ_HW_HD bool uz_hw_sel_in(uint32_t key, int pass, uint32_t prefix) { return pass == 0 || (key >> (32 - 8 * pass)) == prefix; }
UZ_HW_HD uint32_t uz_hw_sel_digit(uint32_t key, int pass) { return (key >> (24 - 8 * pass)) & 255u; }
// the bin that holds rank *rank of the keys counted in hist; *rank becomes the rank inside that bin
UZ_HW_HD uint32_t uz_hw_sel_bin(const uint32_t *hist, uint64_t *rank) {
    uint64_t below = 0;
    uint32_t b = 0;
    for (; b < 255u; b++) {
        if (below + hist[b] > *rank) break;
        below += hist[b];
    }
    *rank -= below;
    return b;
}
// after the last pass: hist counts the low byte of the keys under `prefix` (their higher 24 bits), rank is the wanted rank among them,
// min_above the smallest key above them (any value when there is none).  next: the key one rank further is wanted too (else *b = *a).
UZ_HW_HD void uz_hw_sel_last(const uint32_t *hist, uint64_t rank, uint32_t prefix, bool next, uint32_t min_above, uint32_t *a, uint32_t *b) {
    uint64_t total = 0;
    for (int i = 0; i < 256; i++) total += hist[i];
    uint64_t r = rank;
    *a = (prefix << 8) | uz_hw_sel_bin(hist, &r);
    if (!next) { *b = *a; return; }
    r = rank + 1;
    *b = r < total ? ((prefix << 8) | uz_hw_sel_bin(hist, &r)) : min_above;
}
