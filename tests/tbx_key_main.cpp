// tbx_key_main.cpp -- unfazed_amd/csrc/tbx_key.hpp (what k_tbx_keys runs) as a host program: the 64 bytes of a step are a plain loop.  Built by
// tests/test_tbx_body.py with g++ -fsanitize=address,undefined and run as a child process.
//
//   tbx_key cases.bin out.bin CHUNK    every line of every payload as the body states it when the text goes up in chunks of CHUNK bytes
//                                      (0: one chunk): a line sees its chunk's bytes only, and the text's end in the last chunk
//
// cases.bin: u32 count, then per case u32 preset, u64 n + n bytes.  out.bin: per case u32 rows, then per row u64 start, u32 kind, u32 why,
// u32 name_len, u32 bin, i64 beg, i64 end.  Every chunk is a heap block of exactly its size, so that a read outside it stops the program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "tbx_key.hpp"

template <typename T>
static void put(std::vector<uint8_t> &v, T x) {
    uint8_t b[sizeof(T)];
    memcpy(b, &x, sizeof(T));
    v.insert(v.end(), b, b + sizeof(T));
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: tbx_key cases.bin out.bin CHUNK\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    const uint64_t chunk_arg = strtoull(argv[3], nullptr, 10);
    auto rd = [&](size_t at, int bytes) { uint64_t v = 0; for (int k = 0; k < bytes; k++) v |= (uint64_t)file.at(at + k) << (8 * k); return v; };
    const uint32_t n_cases = (uint32_t)rd(0, 4);
    size_t at = 4, lines = 0;
    std::vector<uint8_t> out;
    for (uint32_t ci = 0; ci < n_cases; ci++) {
        const int preset = (int)rd(at, 4);
        const uint64_t n = rd(at + 4, 8);
        at += 12;
        if (at + n > file.size()) { fprintf(stderr, "case %u overruns the file\n", ci); return 2; }
        const uint8_t *text = file.data() + at;
        const uint64_t chunk = chunk_arg ? chunk_arg : (n ? n : 1);
        std::vector<uint8_t> rows;
        uint32_t n_rows = 0;
        for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
            const uint64_t nb = n - c0 < chunk ? n - c0 : chunk;
            std::unique_ptr<uint8_t[]> in(new uint8_t[nb]);
            memcpy(in.get(), text + c0, nb);
            for (uint64_t s = 0; s < nb; s++) {
                if (!(c0 + s == 0 || text[c0 + s - 1] == '\n')) continue; // not a line's first byte
                UzTbxHostWave w;
                UzTbxKey k;
                uz_tbx_key(w, in.get(), s, nb, c0 + nb == n, preset, k);
                put<uint64_t>(rows, c0 + s);
                put<uint32_t>(rows, k.kind);
                put<uint32_t>(rows, k.why);
                put<uint32_t>(rows, k.name_len);
                put<uint32_t>(rows, k.kind == UZ_TBX_DATA ? uz_tbx_reg2bin(k.beg, k.end) : 0u);
                put<int64_t>(rows, k.beg);
                put<int64_t>(rows, k.end);
                n_rows++;
                lines++;
            }
        }
        at += n;
        put<uint32_t>(out, n_rows);
        out.insert(out.end(), rows.begin(), rows.end());
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) { perror(argv[2]); return 2; }
    printf("tbx key ok: %u cases, %zu lines\n", n_cases, lines);
    return 0;
}
