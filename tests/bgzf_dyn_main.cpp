// bgzf_dyn_main.cpp -- unfazed_amd/csrc/deflate_dyn.hpp (what k_bgzf_deflate_dyn runs) as a host program: one "wave" whose 64 lanes are a plain
// loop.  Built by tests/dyncases.py with g++ -fsanitize=address,undefined and run as a child process.
//
//   bgzf_dyn cases.bin out.bin    every payload of cases.bin as BGZF blocks (no end-of-file marker), framed as k_bgzf_frame frames them
//   bgzf_dyn --code vectors.txt   per line "LIMIT COUNT COUNT ...": the code lengths uz_dy_build gives the counts, one line each
//
// cases.bin: u32 count, then per case u64 n + n bytes.  out.bin: per case u32 blocks, u64 bytes, the bytes, then one byte per block: 0 stored,
// 1 fixed, 2 dynamic.  Every slice's input is a heap block of exactly its size, every slot one of exactly UZ_DF_SLOT bytes and every token
// buffer one of exactly one word per input byte, so that a read or a store outside any of them stops the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "deflate_dyn.hpp"

static uint32_t crc32_of(const uint8_t *p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

static void put32(std::vector<uint8_t> &v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }
static void put64(std::vector<uint8_t> &v, uint64_t x) { for (int k = 0; k < 8; k++) v.push_back((uint8_t)(x >> (8 * k))); }

static int code_mode(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    std::string text;
    char buf[1 << 12];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    fclose(f);
    std::istringstream lines(text);
    std::string line;
    std::unique_ptr<UzDyBuild> B(new UzDyBuild);
    while (std::getline(lines, line)) {
        std::istringstream in(line);
        uint32_t limit = 0;
        if (!(in >> limit)) continue;
        std::vector<uint32_t> cnt;
        for (uint32_t v; in >> v;) cnt.push_back(v);
        if (limit < 1 || limit > 15 || cnt.size() > 288) { fprintf(stderr, "a limit of %u, %zu counts\n", limit, cnt.size()); return 2; }
        const uint32_t n = (uint32_t)cnt.size();
        if (limit < 9 && n > (1u << limit)) { fprintf(stderr, "%u symbols cannot have codes of %u bits\n", n, limit); return 2; }
        std::unique_ptr<uint32_t[]> c(new uint32_t[n]), code(new uint32_t[n]);
        std::unique_ptr<uint8_t[]> len(new uint8_t[n]);
        for (uint32_t i = 0; i < n; i++) c[i] = cnt[i];
        UzDfHostWave w;
        uz_dy_build(w, *B, c.get(), n, limit, len.get(), code.get());
        for (uint32_t i = 0; i < n; i++) {
            if ((code[i] & 31u) != len[i] || (code[i] >> 5) >> len[i]) { fprintf(stderr, "symbol %u: code %x for length %u\n", i, code[i], len[i]); return 1; }
            printf(i ? " %u" : "%u", len[i]);
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "--code")) return code_mode(argv[2]);
    if (argc != 3) { fprintf(stderr, "usage: bgzf_dyn cases.bin out.bin | --code vectors.txt\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    auto rd = [&](size_t at, int bytes) { uint64_t v = 0; for (int k = 0; k < bytes; k++) v |= (uint64_t)file.at(at + k) << (8 * k); return v; };
    const uint32_t n_cases = (uint32_t)rd(0, 4);
    size_t at = 4;
    std::vector<uint8_t> out;
    std::unique_ptr<UzDyLds> lds(new UzDyLds);
    size_t slices = 0;
    for (uint32_t ci = 0; ci < n_cases; ci++) {
        const uint64_t n = rd(at, 8);
        at += 8;
        if (at + n > file.size()) { fprintf(stderr, "case %u overruns the file\n", ci); return 2; }
        std::vector<uint8_t> blocks, how;
        for (uint64_t s0 = 0; s0 < n; s0 += UZ_DF_SLICE) {
            const uint32_t len = (uint32_t)(n - s0 < UZ_DF_SLICE ? n - s0 : UZ_DF_SLICE);
            std::unique_ptr<uint8_t[]> in(new uint8_t[len]);
            memcpy(in.get(), file.data() + at + s0, len);
            std::unique_ptr<uint32_t[]> slot(new uint32_t[UZ_DF_SLOT / 4]), tok(new uint32_t[len]);
            memset(slot.get(), 0xA5, UZ_DF_SLOT);
            uint8_t *sp = reinterpret_cast<uint8_t *>(slot.get());
            UzDfHostWave w;
            uint32_t kind = 99;
            const uint32_t cnt = uz_deflate_slice_dyn(w, *lds, in.get(), len, sp, UZ_DF_SLOT, tok.get(), len, kind);
            if (cnt == 0 || cnt > 5 + len || kind > 2) { fprintf(stderr, "case %u: a stream of %u bytes from %u, kind %u\n", ci, cnt, len, kind); return 1; }
            for (uint32_t k = (cnt + 3) & ~3u; k < UZ_DF_SLOT; k++)
                if (sp[k] != 0xA5) { fprintf(stderr, "case %u: a store behind the stream's last word (byte %u of the slot)\n", ci, k); return 1; }
            const uint32_t bsize = UZ_BGZF_HEAD + cnt + UZ_BGZF_TAIL - 1;
            const uint8_t head[UZ_BGZF_HEAD] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 0xFF), (uint8_t)(bsize >> 8)};
            blocks.insert(blocks.end(), head, head + UZ_BGZF_HEAD);
            blocks.insert(blocks.end(), sp, sp + cnt);
            put32(blocks, crc32_of(in.get(), len));
            put32(blocks, len);
            how.push_back((uint8_t)kind);
            slices++;
        }
        at += n;
        put32(out, (uint32_t)how.size());
        put64(out, blocks.size());
        out.insert(out.end(), blocks.begin(), blocks.end());
        out.insert(out.end(), how.begin(), how.end());
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
    printf("bgzf dyn ok: %u cases, %zu slices\n", n_cases, slices);
    return 0;
}
