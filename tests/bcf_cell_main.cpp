// bcf_cell_main.cpp -- the device's BCF value body (unfazed_amd/csrc/bcf_cell.hpp, the body k_bcf_cells runs) held on the CPU against a plain
// restatement of the host's reader (io_vcf.cpp: bcf_sample_cell) followed by the pack rules of uz_samples_pack.  A program of its own:
// tests/test_bcf_cell.py builds it with g++ under AddressSanitizer + UBSan and runs it as a child process.
//   bcf_cell_main CASES   CASES: one cell per line, fields separated by \x1f: label (plain / unsettled), five "descriptor:hex bytes of this
//                         sample's values" (GT, AD, RO, AO, GQ; descriptor 0 = absent), and for a plain cell "gt,rd,ad,gq" in the 16-bit
//                         encoding as the table states it by hand (tests/bcfcases.py).  Then a seeded fuzz of 2 * 10^5 cells.
// Every settled cell must equal the restatement (and the table); every cell the table calls unsettled must be unsettled; of the fuzzed cells at
// least 90 % must settle (the share is printed).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "bcf_cell.hpp"

namespace {

struct Field {
    uint32_t desc = 0;
    std::vector<uint8_t> bytes; // this sample's values, exactly: a read past them is the sanitizer's to find
    uint32_t type() const { return desc & 15u; }
    uint32_t n() const { return desc >> 4; }
};

struct Packed { // a cell in the sample table's encoding, or the reasons it has none
    uint32_t gt = 2, rd = 0xFFFF, ad = 0xFFFF, gq = 0xFFFF;
    bool range = false, wide = false;
};

// ---- the restatement: BCF2's typed integers as the decoder reads them, then the cell, then the pack
enum { OK = 0, MISSING = 1, EOV = 2 };
int read_int(const Field &f, uint32_t k, long long &out) {
    const uint8_t *p = f.bytes.data();
    if (f.type() == 1) { int8_t x; memcpy(&x, p + k, 1); if (x == INT8_MIN) return MISSING; if (x == INT8_MIN + 1) return EOV; out = x; return OK; }
    if (f.type() == 2) { int16_t x; memcpy(&x, p + 2 * k, 2); if (x == INT16_MIN) return MISSING; if (x == INT16_MIN + 1) return EOV; out = x; return OK; }
    if (f.type() == 3) { int32_t x; memcpy(&x, p + 4 * k, 4); if (x == INT32_MIN) return MISSING; if (x == INT32_MIN + 1) return EOV; out = x; return OK; }
    return MISSING; // any other type: nothing an integer can be read from
}

uint32_t depth16(long long d, Packed &p) {
    if (d < -1 || d > (1 << 30)) p.range = true; // uz_samples_pack refuses the table
    if (d > 32767) p.wide = true;                // the site goes to the wide list
    return d < 0 ? 0xFFFFu : d > 32767 ? 32767u : (uint32_t)d;
}

Packed host_cell(const Field f[5]) {
    Packed p;
    int gt = 2;
    long long rd = -1, ad = -1;
    double gq = -1.0;
    if (f[0].n()) {
        long long al[2] = {-1, -1};
        int na = 0;
        for (uint32_t k = 0; k < f[0].n(); k++) {
            long long x = 0;
            const int st = read_int(f[0], k, x);
            if (st == EOV) break;
            if (na < 2) al[na] = st == OK ? (x >> 1) - 1 : -1;
            na++;
        }
        if (na == 1) gt = al[0] < 0 ? 2 : (al[0] == 0 ? 0 : 3);
        else if (na >= 2) {
            const long long a = al[0], b = al[1];
            if (a < 0 && b < 0) gt = 2;
            else if (a < 0 || b < 0) gt = (b < 0 ? a : b) == 0 ? 0 : 1;
            else if (a != b) gt = 1;
            else gt = a == 0 ? 0 : 3;
        }
    }
    bool ad_done = false;
    if (f[1].n()) {
        long long x0 = -1, x1 = -1;
        const int s0 = read_int(f[1], 0, x0);
        const int s1 = f[1].n() > 1 ? read_int(f[1], 1, x1) : EOV;
        if (!(s0 != OK && s1 == EOV)) { rd = s0 == OK ? x0 : -1; ad = s1 == OK ? x1 : -1; ad_done = true; }
    }
    if (!ad_done && f[2].n() && f[3].n()) {
        long long x = 0;
        rd = read_int(f[2], 0, x) == OK ? x : -1;
        ad = read_int(f[3], 0, x) == OK ? x : -1;
    }
    if (f[4].n()) {
        if (f[4].type() == 5) {
            uint32_t bits;
            memcpy(&bits, f[4].bytes.data(), 4);
            float fl;
            memcpy(&fl, &bits, 4);
            gq = (bits == 0x7F800001u || bits == 0x7F800002u) ? -1.0 : (double)fl;
        } else {
            long long x = 0;
            gq = read_int(f[4], 0, x) == OK ? (double)x : -1.0;
        }
    }
    p.gt = (uint32_t)gt;
    p.rd = depth16(rd, p);
    p.ad = depth16(ad, p);
    const double g = std::floor(gq);
    p.gq = !(g >= 0.0) ? 0xFFFFu : g > 32767.0 ? 32767u : (uint32_t)(int)g;
    return p;
}

UzVcfCell device_cell(const Field f[5]) {
    return uz_bcf_cell(f[0].bytes.data(), f[0].desc, f[1].bytes.data(), f[1].desc, f[2].bytes.data(), f[2].desc, f[3].bytes.data(), f[3].desc, f[4].bytes.data(),
                       f[4].desc);
}

bool taken(const Field f[5]) { // the types the kernel takes (the host keeps every other record to itself, whether the cell reads the field or not)
    for (int k = 0; k < 5; k++)
        if (f[k].desc && !(uz_bc_is_int(f[k].type()) || (k == 4 && f[k].type() == UZ_BC_FLOAT))) return false;
    return true;
}

// -> "" or what is wrong
std::string check(const Field f[5], bool *settled) {
    const Packed h = host_cell(f);
    const UzVcfCell d = device_cell(f);
    *settled = d.settled;
    if (!d.settled) return "";
    if (h.range || h.wide) return "settled a depth the 16-bit rows cannot hold";
    if (d.gt != h.gt || d.rd != h.rd || d.ad != h.ad || d.gq != h.gq) {
        char b[160];
        snprintf(b, sizeof b, "device %u %u %u %u, host %u %u %u %u", d.gt, d.rd, d.ad, d.gq, h.gt, h.rd, h.ad, h.gq);
        return b;
    }
    return "";
}

std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> f;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find(sep, a);
        f.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    return f;
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bcf_cell_main CASES\n"); return 2; }
    int bad = 0;
    long n_cases = 0, n_plain = 0;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(in, line, '\n')) {
        const std::vector<std::string> f = split(line, '\x1f');
        if (f.size() != 8) { fprintf(stderr, "bad case line\n"); return 2; }
        const bool plain = f[1] == "plain";
        Field fld[5];
        for (int k = 0; k < 5; k++) {
            const std::vector<std::string> dh = split(f[2 + (size_t)k], ':');
            if (dh.size() != 2 || dh[1].size() % 2) { fprintf(stderr, "bad field\n"); return 2; }
            fld[k].desc = (uint32_t)strtoul(dh[0].c_str(), nullptr, 10);
            for (size_t i = 0; i < dh[1].size(); i += 2) fld[k].bytes.push_back((uint8_t)strtoul(dh[1].substr(i, 2).c_str(), nullptr, 16));
            if (fld[k].bytes.size() != (size_t)fld[k].n() * (fld[k].type() == 7 ? 1u : uz_bc_size(fld[k].type()))) { fprintf(stderr, "field bytes do not match the descriptor\n"); return 2; }
        }
        bool settled = false;
        const std::string err = check(fld, &settled);
        n_cases++;
        n_plain += plain;
        const char *name = f[0].c_str();
        if (!err.empty()) { bad++; printf("case %s: %s\n", name, err.c_str()); }
        if (plain != settled) { bad++; printf("case %s: labelled %s, the body %s it\n", name, f[1].c_str(), settled ? "settled" : "handed back"); }
        if (plain) { // the table's own statement of the packed values
            unsigned w[4] = {0, 0, 0, 0};
            if (sscanf(f[7].c_str(), "%u,%u,%u,%u", &w[0], &w[1], &w[2], &w[3]) != 4) { fprintf(stderr, "bad expected values\n"); return 2; }
            const UzVcfCell d = device_cell(fld);
            const Packed h = host_cell(fld);
            if (d.gt != w[0] || d.rd != w[1] || d.ad != w[2] || d.gq != w[3]) { bad++; printf("case %s: the body gives %u %u %u %u, the table says %s\n", name, d.gt, d.rd, d.ad, d.gq, f[7].c_str()); }
            if (h.gt != w[0] || h.rd != w[1] || h.ad != w[2] || h.gq != w[3]) { bad++; printf("case %s: the restatement gives %u %u %u %u, the table says %s\n", name, h.gt, h.rd, h.ad, h.gq, f[7].c_str()); }
        }
    }
    if (n_cases < 100 || n_plain < 80) { printf("only %ld cases read, %ld of them plain\n", n_cases, n_plain); return 1; }

    // fuzz: random descriptors and values -- mostly small numbers, markers now and then, a depth out of range or a foreign type rarely
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    auto put = [](Field &f, uint32_t type, long long v) {
        const uint32_t sz = uz_bc_size(type);
        for (uint32_t b = 0; b < sz; b++) f.bytes.push_back((uint8_t)((uint64_t)v >> (8 * b)));
    };
    auto int_entry = [&](uint32_t type, bool genotype) -> long long {
        const long long lowest = type == 1 ? -128 : type == 2 ? -32768 : (long long)INT32_MIN;
        const uint64_t r = rnd() % 1000;
        if (r < 60) return lowest;     // missing
        if (r < 110) return lowest + 1; // end-of-vector
        if (genotype) return (long long)(rnd() % 8);
        if (r < 116) return type == 1 ? -(long long)(rnd() % 100) - 1 : type == 2 ? -(long long)(rnd() % 30000) - 1 : (rnd() & 1 ? 32768 + (long long)(rnd() % 100000) : -(long long)(rnd() % 70000) - 1);
        if (r < 160) return type == 1 ? 127 : 32767 - (long long)(rnd() % 3);
        return (long long)(rnd() % (type == 1 ? 128 : 400));
    };
    auto int_field = [&](Field &f, bool genotype, uint32_t max_n) {
        const uint32_t type = 1 + (uint32_t)(rnd() % 3), n = 1 + (uint32_t)(rnd() % max_n);
        f.desc = type | n << 4;
        for (uint32_t k = 0; k < n; k++) put(f, type, int_entry(type, genotype));
    };
    static const float floats[] = {0.0f, 0.5f, 20.0f, 99.9f, 32767.0f, 32767.5f, 32768.0f, 40000.0f, -0.0f, -0.25f, -1.0f, 1e30f, -1e30f};
    long cells = 0, settled_n = 0;
    while (cells < 200000) {
        Field f[5];
        if (rnd() % 100 < 90) int_field(f[0], true, 3);
        if (rnd() % 100 < 75) int_field(f[1], false, 3);
        if (rnd() % 100 < 50) int_field(f[2], false, 1);
        if (rnd() % 100 < 50) int_field(f[3], false, 2);
        if (rnd() % 100 < 80) {
            if (rnd() & 1) int_field(f[4], false, 2);
            else {
                f[4].desc = UZ_BC_FLOAT | 1u << 4;
                const uint64_t r = rnd() % 100;
                uint32_t bits;
                if (r < 10) bits = 0x7F800001u + (uint32_t)(rnd() % 3);
                else if (r < 15) bits = 0x7FC00000u | (uint32_t)(rnd() & 0xFFFF);
                else if (r < 20) bits = rnd() & 1 ? 0x7F800000u : 0xFF800000u;
                else if (r < 60) { const float x = floats[rnd() % (sizeof(floats) / sizeof(floats[0]))]; memcpy(&bits, &x, 4); }
                else { const float x = (float)(rnd() % 1000000) / 1000.0f; memcpy(&bits, &x, 4); }
                put(f[4], UZ_BC_FLOAT, bits);
            }
        }
        if (rnd() % 100 < 2) { // a type the kernel does not take: characters, or floats where integers belong
            Field &g = f[rnd() % 5];
            if (g.desc) { const uint32_t n = g.n(); g.bytes.assign(n * (size_t)4, (uint8_t)'1'); g.desc = (rnd() & 1 ? 7u : 5u) | n << 4; if (g.type() == 7) g.bytes.resize(n); }
        }
        bool settled = false;
        const std::string err = check(f, &settled);
        cells++;
        settled_n += settled;
        if (!err.empty() && bad < 40) { bad++; printf("fuzz %u %u %u %u %u: %s\n", f[0].desc, f[1].desc, f[2].desc, f[3].desc, f[4].desc, err.c_str()); }
        if (!settled && taken(f)) { // the body may hand back only what the rows cannot hold
            const Packed h = host_cell(f);
            bool negative = false;
            long long x = 0;
            for (int k = 1; k < 4; k++)
                for (uint32_t e = 0; e < f[k].n() && e < 2; e++) negative |= read_int(f[k], e, x) == OK && x < 0;
            if (!h.wide && !h.range && !negative && bad < 40) { bad++; printf("fuzz %u %u %u %u %u: handed back a cell the rows can hold\n", f[0].desc, f[1].desc, f[2].desc, f[3].desc, f[4].desc); }
        }
    }
    const double share = (double)settled_n / (double)cells;
    printf("fuzz: %ld of %ld cells settled (%.1f %%)\n", settled_n, cells, 100.0 * share);
    if (share < 0.90) { bad++; printf("the fuzz settled less than 90 %% of its cells\n"); }
    if (bad) { printf("bcf cell FAILED: %d findings\n", bad); return 1; }
    printf("bcf cell ok: %ld cases, %ld fuzzed cells, %ld of them settled\n", n_cases, cells, settled_n);
    return 0;
}
