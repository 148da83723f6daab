// vcf_cell_main.cpp -- the device's cell parser (unfazed_amd/csrc/vcf_cell.hpp, the body k_vcf_cells runs) held against the host's reader
// (csrc/io_vcf_cell.hpp) and the pack rules of uz_samples_pack, on the CPU.  A program of its own: tests/test_vcf_cell.py builds it with
// g++ under AddressSanitizer + UBSan and runs it as a child process.
//   vcf_cell_main CASES   CASES: one cell per line, "label \x1f raises \x1f FORMAT \x1f cell" (tests/vcfcases.py); the cell "\x1e" is a
//                         column the line is too short to hold.  Then a seeded fuzz of 10^5 cells over the alphabet 0-9 . , : / | - + e \t.
// Every cell must either equal the host's value after the pack rules or be unsettled; a `plain` case must be settled, an `unsettled` one not.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "io_vcf_cell.hpp"
#include "vcf_cell.hpp"

namespace {

struct Packed { // a cell in the sample table's encoding, or the reasons it has none
    uint32_t gt = 2, rd = 0xFFFF, ad = 0xFFFF, gq = 0xFFFF;
    bool threw = false, range = false, wide = false;
};

uint32_t depth16(int32_t d, Packed &p) {
    if (d < -1 || d > (1 << 30)) p.range = true; // uz_samples_pack refuses the table
    if (d > 32767) p.wide = true;                // the site goes to the wide list
    return d < 0 ? 0xFFFFu : d > 32767 ? 32767u : (uint32_t)d;
}

Packed host_cell(const std::string &cell, bool missing, const int slot[5]) {
    Packed p;
    uint8_t gt = 2;
    int32_t rd = -1, ad = -1;
    double gq = -1.0;
    try {
        const std::string text = missing ? "." : cell;
        uzcell::sample_cell(uzcell::Str{text.data(), text.size()}, slot, gt, rd, ad, gq);
    } catch (const uzcell::BadAllele &) {
        p.threw = true;
        return p;
    }
    p.gt = gt;
    p.rd = depth16(rd, p);
    p.ad = depth16(ad, p);
    const double g = std::floor(gq);
    p.gq = !(g >= 0.0) ? 0xFFFFu : g > 32767.0 ? 32767u : (uint32_t)(int)g;
    return p;
}

UzVcfCell device_cell(const std::string &cell, bool missing, const int slot[5]) {
    if (missing || (slot[0] < 0 && slot[1] < 0 && slot[2] < 0 && slot[3] < 0 && slot[4] < 0)) return uz_vcf_cell_default();
    // the cell in a buffer of exactly its size: a read past its end is the sanitizer's to find
    std::vector<uint8_t> buf(cell.begin(), cell.end());
    return uz_vcf_cell(buf.data(), (uint32_t)buf.size(), slot[0], slot[1], slot[2], slot[3], slot[4]);
}

// -> "" or what is wrong
std::string check(const std::string &cell, bool missing, const int slot[5], bool *settled) {
    const Packed h = host_cell(cell, missing, slot);
    const UzVcfCell d = device_cell(cell, missing, slot);
    *settled = d.settled;
    if (!d.settled) return "";
    if (h.threw) return "settled a cell the host refuses";
    if (h.range || h.wide) return "settled a depth the 16-bit rows cannot hold";
    if (d.gt != h.gt || d.rd != h.rd || d.ad != h.ad || d.gq != h.gq) {
        char b[160];
        snprintf(b, sizeof b, "device %u %u %u %u, host %u %u %u %u", d.gt, d.rd, d.ad, d.gq, h.gt, h.rd, h.ad, h.gq);
        return b;
    }
    return "";
}

std::string show(const std::string &s) {
    std::string o;
    for (char ch : s) {
        if (ch == '\t') o += "\\t"; else if (ch == '\r') o += "\\r"; else o += ch;
    }
    return o;
}

} // namespace

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: vcf_cell_main CASES\n"); return 2; }
    int bad = 0;
    long n_cases = 0;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(in, line, '\n')) {
        std::vector<std::string> f;
        size_t a = 0;
        for (;;) {
            const size_t b = line.find('\x1f', a);
            f.push_back(line.substr(a, b == std::string::npos ? std::string::npos : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        if (f.size() != 4) { fprintf(stderr, "bad case line\n"); return 2; }
        const bool plain = f[0] == "plain", raises = f[1] == "1", missing = f[3] == "\x1e";
        int slot[5] = {-1, -1, -1, -1, -1};
        if (f[2] != "\x1e") uzcell::format_slots(uzcell::Str{f[2].data(), f[2].size()}, slot);
        bool settled = false;
        const std::string err = check(f[3], missing, slot, &settled);
        const Packed h = host_cell(f[3], missing, slot);
        n_cases++;
        if (!err.empty()) { bad++; printf("case %s | %s: %s\n", f[2].c_str(), show(f[3]).c_str(), err.c_str()); }
        if (plain != settled) { bad++; printf("case %s | %s: labelled %s, the parser %s it\n", f[2].c_str(), show(f[3]).c_str(), f[0].c_str(), settled ? "settled" : "handed back"); }
        if (raises != h.threw) { bad++; printf("case %s | %s: the host reader %s\n", f[2].c_str(), show(f[3]).c_str(), h.threw ? "refused it" : "did not refuse it"); }
    }
    if (n_cases < 50) { printf("only %ld cases read\n", n_cases); return 1; }

    // fuzz: random sample regions, split at tabs as the decoder splits a line, every column read by a random FORMAT
    static const char alphabet[] = "0123456789.,:/|-+e\t";
    static const char *formats[] = {"GT:AD:GQ", "GT:AD:RO:AO:GQ", "GQ:GT", "AD", "GT:RO:AO", "GT", "GT:GQ:AD", "RO:AO:AD:GT:GQ", "XX:GT:GT:AD"};
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    long cells = 0, settled_n = 0;
    while (cells < 100000) {
        const char *fmt = formats[rnd() % (sizeof(formats) / sizeof(formats[0]))];
        int slot[5];
        uzcell::format_slots(uzcell::Str{fmt, strlen(fmt)}, slot);
        std::string region;
        const int len = (int)(rnd() % 25);
        for (int i = 0; i < len; i++) {
            // digits and the separators a real cell is made of come up more often than the rest
            const uint64_t r = rnd() % 100;
            region += r < 45 ? (char)('0' + rnd() % 10) : r < 60 ? ':' : r < 70 ? ',' : r < 78 ? '/' : alphabet[rnd() % (sizeof(alphabet) - 1)];
        }
        size_t a = 0;
        for (;;) {
            const size_t b = region.find('\t', a);
            const std::string cell = region.substr(a, b == std::string::npos ? std::string::npos : b - a);
            bool settled = false;
            const std::string err = check(cell, false, slot, &settled);
            cells++;
            settled_n += settled;
            if (!err.empty() && bad < 40) { bad++; printf("fuzz %s | %s: %s\n", fmt, show(cell).c_str(), err.c_str()); }
            if (b == std::string::npos) break;
            a = b + 1;
        }
    }
    if (settled_n < cells / 20) { bad++; printf("the fuzz settled only %ld of %ld cells: it does not reach the parser's plain paths\n", settled_n, cells); }
    if (bad) { printf("vcf cell FAILED: %d findings\n", bad); return 1; }
    printf("vcf cell ok: %ld cases, %ld fuzzed cells, %ld of them settled\n", n_cases, cells, settled_n);
    return 0;
}
