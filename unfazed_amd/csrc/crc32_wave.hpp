// crc32_wave.hpp -- CRC-32 of a run of bytes by one wavefront: the slice-and-combine code of k_bgzf_crc32 (k_inflate.hip: compares the value with
// a BGZF footer's) and k_bgzf_crc32_out (k_deflate.hip: returns it).  The run is cut into 64 consecutive slices, lane l runs the table CRC over slice
// l (slicing by four, 16-byte loads; tables in LDS; lane 0 starts from 0xFFFFFFFF, the others from 0 -- the register is linear in its start value),
// and the slices are joined the way zlib's crc32_combine joins two: the CRC register after m more zero bytes is a 32 x 32 matrix over GF(2) applied
// to it, the matrices for 2^j zero bytes (j = 0 .. 16) are squared up once per wave in LDS, and lane l applies those its distance from the run's end
// names.  XOR over the lanes, final inversion.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct UzCrcLds {
    uint32_t tab[4][256]; // slicing by four: tab[k][b] = the register after byte b and k more zero bytes
    uint32_t mat[19][32]; // [0]: one zero bit, [1]: two, [2]: four; [3 + j]: 2^j zero bytes
};

__device__ __forceinline__ uint32_t uz_gf2_times(const uint32_t *mat, uint32_t vec) {
    uint32_t sum = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) sum ^= ((vec >> i) & 1u) ? mat[i] : 0u;
    return sum;
}

// the tables of a wave (a workgroup of 64 lanes), once per kernel
__device__ __forceinline__ void uz_crc_setup(UzCrcLds &S, int lane) {
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        S.tab[0][i] = c;
    }
    if (lane < 32) S.mat[0][lane] = lane == 0 ? 0xEDB88320u : 1u << (lane - 1);
    __syncthreads();
    for (int k = 1; k < 4; k++) {
        for (int i = lane; i < 256; i += 64) { const uint32_t c = S.tab[k - 1][i]; S.tab[k][i] = S.tab[0][c & 0xFFu] ^ (c >> 8); }
        __syncthreads();
    }
    for (int j = 1; j < 19; j++) { // each squared from the one before
        if (lane < 32) S.mat[j][lane] = uz_gf2_times(S.mat[j - 1], S.mat[j - 1][lane]);
        __syncthreads();
    }
}

// CRC-32 of p[0 .. n), in every lane
__device__ __forceinline__ uint32_t uz_crc_wave(const UzCrcLds &S, const uint8_t *p, uint32_t n, int lane) {
    auto step4 = [&](uint32_t c, uint32_t w) {
        c ^= w;
        return S.tab[3][c & 0xFFu] ^ S.tab[2][(c >> 8) & 0xFFu] ^ S.tab[1][(c >> 16) & 0xFFu] ^ S.tab[0][c >> 24];
    };
    // slices whose first byte is 16-byte aligned in memory (all but lane 0's): a lane reads its slice with 16-byte loads, eight of them to a
    // cache line, instead of byte loads 1 KiB apart in every lane
    const uint32_t a0 = (uint32_t)((uintptr_t)p & 15u);
    const uint32_t S_ = ((((n + 15u) + 63u) / 64u) + 15u) & ~15u;
    uint32_t lo = lane == 0 ? 0u : min(n, (uint32_t)lane * S_ - a0);
    const uint32_t hi = min(n, ((uint32_t)lane + 1u) * S_ - a0);
    uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u;
    while (lo < hi && (((uintptr_t)(p + lo)) & 15u)) { c = S.tab[0][(c ^ p[lo]) & 0xFFu] ^ (c >> 8); lo++; }
    for (; lo + 16u <= hi; lo += 16u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + lo);
        c = step4(c, v.x); c = step4(c, v.y); c = step4(c, v.z); c = step4(c, v.w);
    }
    for (; lo < hi; lo++) c = S.tab[0][(c ^ p[lo]) & 0xFFu] ^ (c >> 8);
    uint32_t m = n - hi; // zero bytes behind this slice
    for (int j = 0; m; j++, m >>= 1)
        if (m & 1u) c = uz_gf2_times(S.mat[3 + j], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
    return c ^ 0xFFFFFFFFu;
}
