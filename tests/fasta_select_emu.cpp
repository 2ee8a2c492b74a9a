// The two lane steps of k_fa_match_headers and the host's table builder (mbgc_amd/csrc/fasta_select.h) as plain C++: every header run
// tile by tile, every tile's 64 lanes one after the other (all the staging steps, then — the kernel's barrier — all the match steps),
// the header left at the first tile with a hit as the kernel leaves it, against a memmem loop written the obvious way. Built with
// AddressSanitizer by tests/test_fasta_select_kernel_cpu.py; every header is handed over in an allocation of its own that is
// exactly as long as the header, the patterns and the staging buffer are as long as declared, so a read past an end ends the run. No GPU.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
namespace fa {
#include "../mbgc_amd/csrc/fasta_select.h"
}
using namespace fa;

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 1500;
    std::mt19937_64 rng(11);
    uint64_t hits = 0, longHeaders = 0;
    for (int it = 0; it < iterations; it++) {
        // headers over a small alphabet, so that patterns drawn at random occur; lengths around the tile's and the gram's edges
        const char *alpha = it % 3 ? "ab" : "abcd|. ";
        const size_t na = strlen(alpha);
        const uint64_t lc[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 70, 71, 72, 127, 128, 129, rng() % 40, rng() % 400, rng() % 5000};
        const int nrec = 1 + (int) (rng() % 12);
        std::vector<uint64_t> off, len;
        std::string blob;
        for (int r = 0; r < nrec; r++) {
            const uint64_t n = lc[rng() % 18];
            off.push_back(blob.size()); len.push_back(n);
            for (uint64_t i = 0; i < n; i++) blob.push_back(alpha[rng() % na]);
            if (!(it % 5 == 0 && r + 1 == nrec)) blob.push_back('\n');   // (every fifth call: the last header ends with the blob)
        }
        // patterns: random ones, substrings of headers (at the head, at the tail, the whole header, one byte more than the header, across
        // the line feed into the next header), prefixes of other patterns, the same one twice, a long one
        const int npat = 1 + (int) (rng() % (it % 7 == 0 ? 300 : 6));
        const uint64_t minLen = 1 + rng() % 10;
        std::vector<std::string> pats;
        for (int k = 0; k < npat; k++) {
            std::string p;
            const int r = (int) (rng() % nrec);
            const unsigned kind = (unsigned) (rng() % 10);
            if (kind == 0 && len[r] >= minLen) p = blob.substr(off[r], minLen + rng() % (len[r] - minLen + 1));                    // the head
            else if (kind == 1 && len[r] >= minLen) { const uint64_t n = minLen + rng() % (len[r] - minLen + 1); p = blob.substr(off[r] + len[r] - n, n); }   // the tail
            else if (kind == 2 && len[r] >= minLen) p = blob.substr(off[r], len[r]);                                               // the whole header
            else if (kind == 3) p = blob.substr(off[r], len[r]) + alpha[rng() % na];                                              // one byte more
            else if (kind == 4 && r + 1 < nrec && len[r] >= 2 && len[r + 1] >= 2) {                                               // split over two headers
                const uint64_t a = 1 + rng() % std::min<uint64_t>(len[r], 12), b = 1 + rng() % std::min<uint64_t>(len[r + 1], 12);
                p = blob.substr(off[r] + len[r] - a, a) + blob.substr(off[r + 1], b);
            }
            else if (kind == 5 && !pats.empty()) { const std::string &q = pats[rng() % pats.size()]; p = q.substr(0, minLen + rng() % (q.size() - minLen + 1)); }   // a prefix of another
            else if (kind == 6 && !pats.empty()) p = pats[rng() % pats.size()];                                                   // the same again
            else if (kind == 7 && len[r] >= 300) p = blob.substr(off[r] + rng() % (len[r] - 299), 300);                           // a long one
            while (p.size() < minLen) p.push_back(alpha[rng() % na]);
            pats.push_back(p);
        }
        std::vector<uint64_t> patOff(1, 0);
        for (const std::string &p : pats) patOff.push_back(patOff.back() + p.size());
        // exactly as long as declared: operator new[] of that many bytes, so that ASan's red zone starts at the end
        uint8_t *headers = new uint8_t[blob.size() ? blob.size() : 1], *patBytes = new uint8_t[patOff.back()];
        memcpy(headers, blob.data(), blob.size());
        for (size_t k = 0; k < pats.size(); k++) memcpy(patBytes + patOff[k], pats[k].data(), pats[k].size());

        SelTable T;
        sel_build_table(patBytes, patOff.data(), pats.size(), T);
        uint64_t shortest = SEL_GRAM;
        for (const std::string &p : pats) shortest = std::min<uint64_t>(shortest, p.size());
        bool ok = T.m == shortest;
        for (int r = 0; r < nrec && ok; r++) {
            bool want = false;
            for (size_t k = 0; k < pats.size() && !want; k++)
                want = pats[k].size() <= len[r] && memmem(headers + off[r], len[r], pats[k].data(), pats[k].size()) != nullptr;
            bool got = false;
            uint8_t *hdr = new uint8_t[len[r] ? len[r] : 1];            // the record's own header and not a byte more: the step may read nothing else
            memcpy(hdr, headers + off[r], len[r]);
            if (len[r] > 64) longHeaders++;
            for (uint64_t base = 0; base + T.m <= len[r] && !got; base += SEL_TILE) {
                uint8_t *stage = new uint8_t[SEL_STAGE];
                memset(stage, 0xee, SEL_STAGE);
                for (uint32_t lane = 0; lane < SEL_TILE; lane++) sel_stage_step(hdr, len[r], base, lane, T.m, stage);
                for (uint32_t lane = 0; lane < SEL_TILE; lane++)
                    got |= sel_lane_step(hdr, len[r], base, lane, T.m, stage, T.slots.data(), T.bits, T.pats.data(), patBytes);
                delete[] stage;
            }
            hits += got;
            if (got != want) {
                printf("MISMATCH in call %d, record %d (%llu bytes): got %d, expected %d; m = %u, %zu patterns\n", it, r, (unsigned long long) len[r], got, want, T.m, pats.size());
                printf("  header: %.*s\n", (int) std::min<uint64_t>(len[r], 200), (const char *) hdr);
                for (const std::string &p : pats) printf("  pattern: %.200s\n", p.c_str());
                ok = false;
            }
            delete[] hdr;
        }
        delete[] headers; delete[] patBytes;
        if (!ok) return 1;
    }
    if (hits < (uint64_t) iterations / 4 || longHeaders < (uint64_t) iterations / 4) { printf("the inputs are too easy: %llu hits, %llu long headers\n", (unsigned long long) hits, (unsigned long long) longHeaders); return 1; }
    printf("ok: %d calls\n", iterations);
    return 0;
}
