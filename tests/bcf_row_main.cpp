// bcf_row_main.cpp -- the device's BCF-record-to-line body (unfazed_amd/csrc/bcf_row.hpp, __host__ __device__: what k_bcfout_size / k_bcfout_fill
// run) on the host with a one-lane group, as a program of its own: built by tests/test_bcf_row.py with g++ under AddressSanitizer + UBSan and run as
// a child process.  argv[1]: cases with their expected lines (tests/bcfrowcases.py: dump).  Every array lies in storage of exactly its size, so the
// sanitizer holds every load inside the data and the names; every record is sized, then filled into a buffer of exactly the sized bytes; sized must
// equal written, the bytes must equal the expected line, samp_at the stated one, and the records handed back must be the stated ones.
// Then the float rule against snprintf("%g"): every bit pattern at a stride of 1021, every pattern within 2 ulps of the printed range's edges and
// of the panel's values, and 10^5 seeded ties at the sixth digit with their neighbours -- the same characters where the body prints, and handed
// back exactly where "%g" takes exponent form or the value is not finite.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bcf_row.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    static uint8_t tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
    fclose(f);
    return b;
}

struct Reader {
    const std::vector<uint8_t> &b;
    size_t at = 0;
    int64_t i64() {
        if (at + 8 > b.size()) { fprintf(stderr, "short file\n"); exit(2); }
        int64_t v;
        memcpy(&v, b.data() + at, 8);
        at += 8;
        return v;
    }
    template <typename T>
    std::vector<T> arr() { // an array as it lies in the file, copied into storage of its own: the sanitizer sees its true size
        const int64_t bytes = i64();
        if (bytes < 0 || at + (size_t)bytes > b.size() || (size_t)bytes % sizeof(T)) { fprintf(stderr, "bad array\n"); exit(2); }
        std::vector<T> v((size_t)bytes / sizeof(T));
        if (bytes) memcpy(v.data(), b.data() + at, (size_t)bytes);
        at += ((size_t)bytes + 7) & ~(size_t)7;
        return v;
    }
};

// the body's float against "%g" -> 0 agree, 1 disagree
static int float_holds(uint32_t bits, long long &printed, long long &back) {
    float f;
    memcpy(&f, &bits, 4);
    char want[64];
    snprintf(want, sizeof want, "%g", (double)f);
    const bool fixed = std::isfinite(f) && !strchr(want, 'e');
    UzBrOut<false> S{nullptr, 0u, 0, true};
    const bool ok = uz_br_float<false>(S, bits);
    if (ok != fixed) { fprintf(stderr, "float %08x: \"%%g\" gives %s, the body %s\n", bits, want, ok ? "prints" : "hands back"); return 1; }
    if (!ok) { back++; return 0; }
    std::vector<uint8_t> out((size_t)S.o);
    UzBrOut<true> F{out.data(), (uint32_t)S.o, 0, true};
    if (!uz_br_float<true>(F, bits) || F.o != S.o || strlen(want) != S.o || memcmp(out.data(), want, (size_t)S.o) != 0) {
        fprintf(stderr, "float %08x: \"%%g\" gives %s, the body %.*s (sized %llu, written %llu)\n", bits, want, (int)S.o, (const char *)out.data(),
                (unsigned long long)S.o, (unsigned long long)F.o);
        return 1;
    }
    printed++;
    return 0;
}

static long long floats(long long &printed, long long &back) {
    long long bad = 0;
    for (uint64_t b = 0; b <= 0xFFFFFFFFull; b += 1021) bad += float_holds((uint32_t)b, printed, back);
    const float edges[] = {0.0f, 0.0001f, 9.99995e-5f, 999999.0f, 999999.5f, 1e6f, 50.0f, 0.1f, 9.999995f, 99999.95f, 100000.5f, 125000.5f, 1024.125f, 1e-5f, 1048576.0f,
                           6.103515625e-5f, 1.0f, 10.0f, 100.0f, 1000.0f, 10000.0f, 100000.0f, 0.001f, 0.01f};
    for (float e : edges) {
        uint32_t bits;
        memcpy(&bits, &e, 4);
        for (int d = -2; d <= 2; d++)
            for (uint32_t sign = 0; sign < 2; sign++) bad += float_holds((bits + (uint32_t)d) | sign << 31, printed, back);
    }
    for (uint32_t special : {0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F800001u, 0x7F800002u, 0x00000001u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x80000000u})
        bad += float_holds(special, printed, back);
    // ties at the sixth digit: N / 2^s with N odd has the finite decimal expansion N * 5^s / 10^s, which ends in 5; where N * 5^s has seven digits
    // the value is an exact tie at the sixth (s = 1: d.5; s = 3: 1024.125; s = 10: 1 / 1024).  N < 2^21: a float holds it exactly.
    uint64_t x = 88172645463325252ull; // xorshift64, seeded
    for (int i = 0; i < 100000; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const int s = 1 + (int)(x % 10);
        uint64_t p5 = 1;
        for (int k = 0; k < s; k++) p5 *= 5;
        const uint64_t lo = (1000000 + p5 - 1) / p5, hi = (10000000 - 1) / p5; // N in [lo, hi]
        uint64_t N = lo + (x >> 20) % (hi - lo + 1);
        if (!(N & 1)) N = N + 1 <= hi ? N + 1 : N - 1;
        if (N < lo || N > hi || !(N & 1)) continue; // (s = 10 has N = 1 alone)
        const float f = ldexpf((float)N, -s);
        uint32_t bits;
        memcpy(&bits, &f, 4);
        for (int dd = -1; dd <= 1; dd++)
            for (uint32_t sign = 0; sign < 2; sign++) bad += float_holds((bits + (uint32_t)dd) | sign << 31, printed, back);
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bcf_row cases.bin\n"); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]);
    Reader rd{file};
    const int64_t n_cases = rd.i64();
    long long run = 0, back = 0, bad = 0;
    for (int64_t ci = 0; ci < n_cases; ci++) {
        const int64_t n = rd.i64(), n_samples = rd.i64();
        const std::vector<uint8_t> data = rd.arr<uint8_t>();
        const std::vector<int64_t> rec_at = rd.arr<int64_t>();
        const std::vector<uint32_t> dict_off = rd.arr<uint32_t>();
        const std::vector<uint8_t> dict_bytes = rd.arr<uint8_t>();
        const std::vector<uint32_t> ctg_off = rd.arr<uint32_t>();
        const std::vector<uint8_t> ctg_bytes = rd.arr<uint8_t>();
        const std::vector<int64_t> exp_off = rd.arr<int64_t>();
        const std::vector<uint8_t> exp = rd.arr<uint8_t>(), exp_hb = rd.arr<uint8_t>();
        const std::vector<int64_t> exp_samp = rd.arr<int64_t>();
        if ((int64_t)rec_at.size() != n || (int64_t)exp_off.size() != n + 1 || (int64_t)exp_hb.size() != n || (int64_t)exp_samp.size() != n || dict_off.empty() ||
            ctg_off.empty() || dict_off.back() != dict_bytes.size() || ctg_off.back() != ctg_bytes.size()) {
            fprintf(stderr, "case %lld: the arrays do not fit the header\n", (long long)ci);
            return 2;
        }
        UzBrTables T;
        T.data = data.data(); T.data_bytes = data.size();
        T.dict_off = dict_off.data(); T.dict_bytes = dict_bytes.data(); T.n_dict = (uint32_t)dict_off.size() - 1u;
        T.ctg_off = ctg_off.data(); T.ctg_bytes = ctg_bytes.data(); T.n_ctg = (uint32_t)ctg_off.size() - 1u;
        T.n_samples = (uint32_t)n_samples; T.reserved0 = 0;
        const UzBrLane1 w;
        for (int64_t k = 0; k < n; k++) {
            bool hb = false;
            uint32_t samp = 0;
            const uint32_t sized = uz_bcf_row_walk<false>(w, T, (uint64_t)rec_at[(size_t)k], nullptr, 0u, samp, hb);
            run++;
            if (hb != (exp_hb[(size_t)k] != 0)) {
                fprintf(stderr, "case %lld record %lld: handed back %d, stated %d\n", (long long)ci, (long long)k, (int)hb, (int)exp_hb[(size_t)k]);
                bad++;
                continue;
            }
            if (hb) {
                back++;
                if (sized != 0) { fprintf(stderr, "case %lld record %lld: handed back with %u bytes\n", (long long)ci, (long long)k, sized); bad++; }
                continue;
            }
            std::vector<uint8_t> out((size_t)sized);
            bool hb2 = false;
            uint32_t samp2 = 0;
            const uint32_t written = uz_bcf_row_walk<true>(w, T, (uint64_t)rec_at[(size_t)k], out.data(), sized, samp2, hb2);
            const size_t e0 = (size_t)exp_off[(size_t)k], e1 = (size_t)exp_off[(size_t)k + 1];
            if (hb2 || written != sized || e1 - e0 != sized || memcmp(out.data(), exp.data() + e0, sized) != 0 || samp != (uint32_t)exp_samp[(size_t)k] || samp2 != samp) {
                fprintf(stderr, "case %lld record %lld: sized %u written %u expected %zu, samp_at %u / %u stated %lld\n  got  %.*s  want %.*s", (long long)ci, (long long)k,
                        sized, written, e1 - e0, samp, samp2, (long long)exp_samp[(size_t)k], (int)(sized > 400 ? 400 : sized), (const char *)out.data(),
                        (int)(e1 - e0 > 400 ? 400 : e1 - e0), (const char *)exp.data() + e0);
                bad++;
            }
        }
    }
    long long f_printed = 0, f_back = 0;
    const long long f_bad = floats(f_printed, f_back);
    printf("bcf row %s: %lld records, %lld handed back, %lld bad; floats: %lld printed, %lld handed back, %lld bad\n", bad || f_bad ? "FAILED" : "ok", run, back, bad,
           f_printed, f_back, f_bad);
    return bad || f_bad ? 1 : 0;
}
