// vcf_row_main.cpp -- the device's annotated-VCF line body (unfazed_amd/csrc/vcf_row.hpp, __host__ __device__: what k_vcfout_size / k_vcfout_fill run)
// on the host with a one-lane group, as a program of its own: built by tests/test_vcf_row.py with g++ under AddressSanitizer + UBSan and run as a
// child process.  argv[1]: cases with their expected lines (tests/vcfrowcases.py: dump).  Every record is sized, then filled into a buffer of
// exactly the sized bytes (the sanitizer holds every store inside it); sized must equal written, the bytes must equal the expected line, and the
// records handed back must be the stated ones.  The text lies in a buffer of its own with the 16 bytes behind it that a one-lane step may load.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcf_row.hpp"

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
    // an array as it lies in the file, copied into storage of its own (alignment, and the sanitizer sees its true size) + `pad` zero bytes
    template <typename T>
    std::vector<T> arr(size_t pad = 0) {
        const int64_t bytes = i64();
        if (bytes < 0 || at + (size_t)bytes > b.size() || (size_t)bytes % sizeof(T)) { fprintf(stderr, "bad array\n"); exit(2); }
        std::vector<T> v((size_t)bytes / sizeof(T) + pad);
        if (bytes) memcpy(v.data(), b.data() + at, (size_t)bytes);
        at += ((size_t)bytes + 7) & ~(size_t)7;
        return v;
    }
};

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: vcf_row cases.bin\n"); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]);
    Reader rd{file};
    const int64_t n_cases = rd.i64();
    long long run = 0, back = 0, bad = 0;
    for (int64_t ci = 0; ci < n_cases; ci++) {
        const int64_t n = rd.i64(), n_samples = rd.i64();
        const size_t pad = 32;
        const std::vector<uint8_t> text = rd.arr<uint8_t>(pad);
        const std::vector<int64_t> line_at = rd.arr<int64_t>(), samp_at = rd.arr<int64_t>(), line_end = rd.arr<int64_t>(), ann_off = rd.arr<int64_t>();
        const std::vector<int32_t> ann_col = rd.arr<int32_t>();
        const std::vector<uint8_t> ann_gt = rd.arr<uint8_t>();
        const std::vector<int32_t> ann_uops = rd.arr<int32_t>();
        const std::vector<int8_t> ann_uet = rd.arr<int8_t>();
        const std::vector<int64_t> exp_off = rd.arr<int64_t>();
        const std::vector<uint8_t> exp = rd.arr<uint8_t>(), exp_hb = rd.arr<uint8_t>();
        if ((int64_t)line_at.size() != n || (int64_t)samp_at.size() != n || (int64_t)line_end.size() != n || (int64_t)ann_off.size() != n + 1 ||
            (int64_t)exp_off.size() != n + 1 || (int64_t)exp_hb.size() != n || ann_col.size() != ann_gt.size() || ann_col.size() != ann_uops.size() ||
            ann_col.size() != ann_uet.size() || (n && (int64_t)ann_col.size() != ann_off[(size_t)n])) {
            fprintf(stderr, "case %lld: the arrays do not fit the header\n", (long long)ci);
            return 2;
        }
        UzVrAnn A;
        A.col = ann_col.data(); A.gt = ann_gt.data(); A.uops = ann_uops.data(); A.uet = ann_uet.data();
        const UzVrLane1 w;
        for (int64_t k = 0; k < n; k++) {
            // the text a record sees starts at its line's start rounded down to 16, as a chunk's does; the buffer itself is 16-byte aligned or not
            const uint64_t t0 = (uint64_t)line_at[(size_t)k] & ~(uint64_t)15;
            UzVrRec R = uz_vr_rec(text.data(), 0, (uint64_t)line_at[(size_t)k], (uint64_t)samp_at[(size_t)k], (uint64_t)line_end[(size_t)k]);
            (void)t0;
            R.ann0 = (uint32_t)ann_off[(size_t)k]; R.ann1 = (uint32_t)ann_off[(size_t)k + 1];
            bool hb = false;
            const uint32_t sized = uz_vcf_row_walk<false>(w, text.data(), R, A, (int32_t)n_samples, nullptr, 0u, hb);
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
            const uint32_t written = uz_vcf_row_walk<true>(w, text.data(), R, A, (int32_t)n_samples, out.data(), sized, hb2);
            const size_t e0 = (size_t)exp_off[(size_t)k], e1 = (size_t)exp_off[(size_t)k + 1];
            if (hb2 || written != sized || e1 - e0 != sized || memcmp(out.data(), exp.data() + e0, sized) != 0) {
                fprintf(stderr, "case %lld record %lld: sized %u written %u expected %zu\n  got  %.*s  want %.*s", (long long)ci, (long long)k, sized, written, e1 - e0,
                        (int)(sized > 400 ? 400 : sized), (const char *)out.data(), (int)(e1 - e0 > 400 ? 400 : e1 - e0), (const char *)exp.data() + e0);
                bad++;
            }
        }
    }
    printf("vcf row %s: %lld records, %lld handed back, %lld bad\n", bad ? "FAILED" : "ok", run, back, bad);
    return bad ? 1 : 0;
}
