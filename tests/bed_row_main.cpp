// bed_row_main.cpp -- the device's BED row body (unfazed_amd/csrc/bed_row.hpp, __host__ __device__: what k_bed_size / k_bed_fill run) on the host, as
// a program of its own: built by tests/test_bed_row.py with g++ under AddressSanitizer + UBSan and run as a child process.
// argv[1]: cases with their expected text (tests/bedcases.py: dump).  Every row is sized, then filled into a buffer of exactly the sized bytes
// (the sanitizer holds every store inside it); sized must equal written, and the bytes must equal the expected line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bed_row.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t tmp[1 << 16];
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
    // an array as it lies in the file, copied into storage of its own (alignment, and the sanitizer sees its true size)
    template <typename T>
    std::vector<T> arr() {
        const int64_t bytes = i64();
        if (bytes < 0 || at + (size_t)bytes > b.size() || (size_t)bytes % sizeof(T)) { fprintf(stderr, "bad array\n"); exit(2); }
        std::vector<T> v((size_t)bytes / sizeof(T));
        if (bytes) memcpy(v.data(), b.data() + at, (size_t)bytes);
        at += ((size_t)bytes + 7) & ~(size_t)7;
        return v;
    }
};

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bed_row cases.bin\n"); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]);
    Reader rd{file};
    const int64_t n_cases = rd.i64();
    long long rows_run = 0, rows_kept = 0, bad = 0;
    for (int64_t ci = 0; ci < n_cases; ci++) {
        const int64_t ratio = rd.i64(), verbose = rd.i64(), amb = rd.i64(), n_rows = rd.i64(), n_dnms = rd.i64(), n_strings = rd.i64(), n_names = rd.i64(), n_val = rd.i64();
        struct Row { int32_t dnm, start, end; uint32_t chrom, vartype, kid, dad, mom; int32_t reads_id, sex_origin; };
        const std::vector<Row> rows = rd.arr<Row>();
        const std::vector<uint32_t> str_off = rd.arr<uint32_t>();
        const std::vector<uint8_t> str_bytes = rd.arr<uint8_t>();
        const std::vector<int32_t> status = rd.arr<int32_t>();
        const std::vector<int64_t> list_off = rd.arr<int64_t>();
        const std::vector<int32_t> list_val = rd.arr<int32_t>();
        const std::vector<uint32_t> name_off = rd.arr<uint32_t>();
        const std::vector<uint8_t> name_bytes = rd.arr<uint8_t>();
        const std::vector<int64_t> exp_off = rd.arr<int64_t>();
        const std::vector<uint8_t> exp = rd.arr<uint8_t>();
        if ((int64_t)rows.size() != n_rows || (int64_t)status.size() != n_dnms || (int64_t)str_off.size() != n_strings + 1 || (int64_t)name_off.size() != n_names + 1 ||
            (int64_t)list_val.size() != n_val || (int64_t)list_off.size() != 4 * n_dnms + 1 || (int64_t)exp_off.size() != n_rows + 1) {
            fprintf(stderr, "case %lld: the arrays do not fit the header\n", (long long)ci);
            return 2;
        }
        UzBedLists L;
        memset(&L, 0, sizeof L);
        L.status = status.data(); L.off4 = list_off.data(); L.pool = list_val.data();
        UzBedNames T;
        memset(&T, 0, sizeof T);
        T.plain_off = name_off.data(); T.plain_bytes = name_bytes.data(); T.n_qnames = (uint32_t)n_names; T.has_names = 1;
        UzBedStrings S;
        S.off = str_off.data(); S.bytes = str_bytes.data();
        const UzBedLane1 w;
        for (int64_t k = 0; k < n_rows; k++) {
            UzBedRowDev R;
            R.dnm = rows[k].dnm; R.start = rows[k].start; R.end = rows[k].end;
            R.chrom = rows[k].chrom; R.vartype = rows[k].vartype; R.kid = rows[k].kid; R.dad = rows[k].dad; R.mom = rows[k].mom;
            R.table = 0; R.qbase = 0; R.sex_origin = rows[k].sex_origin;
            uint32_t flags = 0;
            const uint32_t sized = uz_bed_row_walk<false>(w, R, L, &T, S, ratio, (int)verbose, (int)amb, nullptr, 0u, flags);
            std::vector<uint8_t> out(sized); // exactly the sized bytes
            const uint32_t written = uz_bed_row_walk<true>(w, R, L, &T, S, ratio, (int)verbose, (int)amb, out.data(), sized, flags);
            const int64_t a = exp_off[k], b = exp_off[k + 1];
            rows_run++;
            rows_kept += sized ? 1 : 0;
            if (flags || sized != written || (int64_t)sized != b - a || (sized && memcmp(out.data(), exp.data() + a, sized) != 0)) {
                if (bad++ < 10)
                    fprintf(stderr, "case %lld row %lld: flags %u sized %u written %u expected %lld\n  got  %.200s\n  want %.200s\n", (long long)ci, (long long)k, flags, sized, written,
                            (long long)(b - a), std::string(out.begin(), out.end()).c_str(), std::string(exp.begin() + a, exp.begin() + b).c_str());
            }
        }
    }
    // what the walk must refuse: a site list that is not ascending, a name id beyond the store
    {
        const int32_t status[1] = {UZ_ST_OK};
        const int64_t off4[5] = {0, 1, 1, 3, 3};
        const int32_t vals[3] = {5, 10, 9};
        const uint32_t noff[2] = {0, 2}, soff[2] = {0, 1};
        const uint8_t nbytes[2] = {'a', 'b'}, sbytes[1] = {'c'};
        UzBedLists L;
        memset(&L, 0, sizeof L);
        L.status = status; L.off4 = off4; L.pool = vals;
        UzBedNames T;
        memset(&T, 0, sizeof T);
        T.plain_off = noff; T.plain_bytes = nbytes; T.n_qnames = 1; T.has_names = 1;
        UzBedStrings S;
        S.off = soff; S.bytes = sbytes;
        UzBedRowDev R;
        memset(&R, 0, sizeof R);
        uint32_t flags = 0;
        (void)uz_bed_row_walk<false>(UzBedLane1(), R, L, &T, S, 10, 1, 0, nullptr, 0u, flags);
        if (flags != (UZ_BED_F_ORDER | UZ_BED_F_NAME)) { fprintf(stderr, "refusals: flags %u\n", flags); bad++; }
    }
    if (bad) { fprintf(stderr, "%lld rows differ\n", bad); return 1; }
    printf("bed row ok: %lld rows, %lld kept\n", rows_run, rows_kept);
    return 0;
}
