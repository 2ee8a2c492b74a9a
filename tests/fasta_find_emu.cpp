// The lane steps of k_fa_find, the search of a tile's record and the host's table builder (mbgc_amd/csrc/fasta_find.h) as plain C++:
// every call cut into tiles as mbgc_fasta_find_dev cuts it, every tile staged vector by vector and then — the kernel's barrier — run
// lane by lane, the hits collected through the callback that is the kernel's atomic cursor, against a triple loop written the obvious
// way (records x patterns x positions, mismatches counted byte by byte). The whole table of hits must be equal, so a hit reported
// twice fails as a missing one does. Built with AddressSanitizer by tests/test_fasta_find_kernel_cpu.py: the text ends where its
// allocation ends (and, every other call, starts where it starts), the pattern blob, the table's arrays and the staging buffer are
// exactly as long as declared, so a read past an end ends the run. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <string>
#include <tuple>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define MBGC_FASTA_FIND_TILE 4096
namespace fa {
#include "../mbgc_amd/csrc/fasta_tiles.h"
#include "../mbgc_amd/csrc/fasta_find.h"
}
using namespace fa;

typedef std::tuple<uint32_t, uint64_t, uint32_t, uint32_t> Hit;      // rec, pos, pattern, mismatches

static uint8_t foldPlain(uint8_t b) { return ((b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z')) ? (uint8_t) (b & 0xDF) : b; }

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937_64 rng(29);
    uint64_t total = 0, withMismatch = 0, multiTile = 0, unaligned = 0, bigTables = 0;
    for (int it = 0; it < iterations; it++) {
        // text over a small alphabet in both cases, so that patterns drawn at random stand in it; now and then a byte that is no letter,
        // among them the ones next to the letters' ranges
        const char *alpha = it % 3 == 0 ? "aAcC" : (it % 3 == 1 ? "aA" : "acgtACGTnN");
        const size_t na = strlen(alpha);
        const char odd[] = {'@', '[', '`', '{', '-', '1', (char) 0xC1, (char) 0xE1};
        const bool big = it % 8 == 0;
        const uint64_t seqBytes = big ? 2 * FIND_TILE + rng() % (2 * FIND_TILE) : 1 + rng() % 700;
        const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;   // the buffer's first byte: any alignment
        uint8_t *alloc = new uint8_t[seqBytes + shift], *seq = alloc + shift;
        for (uint64_t i = 0; i < seqBytes; i++) seq[i] = rng() % 97 == 0 ? (uint8_t) odd[rng() % sizeof odd] : (uint8_t) alpha[rng() % na];
        if (it % 5 == 0) { const uint64_t a = rng() % seqBytes, n = std::min<uint64_t>(seqBytes - a, 1 + rng() % 300); memset(seq + a, 'a', n); }   // a run of one letter
        unaligned += ((uintptr_t) seq & 15) != 0;
        const uint32_t K = (uint32_t) (rng() % 4);
        // records: anywhere, of any length — empty ones, ones of a few bytes, the whole buffer, neighbours, the same one twice, unsorted
        std::vector<ScanRec> recs;
        const int nrec = 1 + (int) (rng() % 9);
        for (int r = 0; r < nrec; r++) {
            const uint64_t lc[] = {0, 1, 7, 8, 9, seqBytes, rng() % 40, rng() % (seqBytes + 1), rng() % (seqBytes + 1)};
            uint64_t len = std::min(lc[rng() % 9], seqBytes), off = rng() % (seqBytes - len + 1);
            if (r && rng() % 4 == 0) { off = recs[r - 1].off + recs[r - 1].len; len = std::min(len, seqBytes - off); }     // right behind the one before
            if (r && rng() % 6 == 0) { off = recs[r - 1].off; len = recs[r - 1].len; }                                     // the same again
            if (rng() % 5 == 0) { off = seqBytes - len; }                                                                 // ends with the buffer
            recs.push_back(ScanRec{off, len});
        }
        // patterns: pieces of the text with up to K + 1 substitutions, in the other case, random ones, prefixes of others, the same
        // one twice, one over a record's joint, long ones that span tiles
        const int npat = 1 + (int) (rng() % (it % 7 == 0 ? 200 : 8));
        const uint32_t minLen = FIND_GRAM * (K + 1);
        std::vector<std::string> pats;
        for (int q = 0; q < npat; q++) {
            std::string p;
            const unsigned kind = (unsigned) (rng() % 8);
            const ScanRec &rc = recs[rng() % recs.size()];
            uint32_t len = minLen + (uint32_t) (rng() % 4 == 0 ? rng() % 60 : rng() % 6);
            if (big && rng() % 9 == 0) len = FIND_TILE + (uint32_t) (rng() % (FIND_TILE + 9));
            if (kind <= 3 && rc.len >= len) {
                const uint64_t at = kind == 0 ? 0 : (kind == 1 ? rc.len - len : rng() % (rc.len - len + 1));
                p.assign((const char *) seq + rc.off + at, len);
                const uint32_t subs = (uint32_t) (rng() % (K + 2));
                for (uint32_t s = 0; s < subs; s++) {
                    const size_t j = rng() % 3 == 0 ? (rng() % 2 ? 0 : p.size() - 1) : rng() % p.size();
                    p[j] = alpha[rng() % na];
                }
            }
            else if (kind == 4 && seqBytes >= len) p.assign((const char *) seq + rng() % (seqBytes - len + 1), len);       // anywhere in the buffer: over joints
            else if (kind == 5 && !pats.empty()) { const std::string &o = pats[rng() % pats.size()]; p = o.substr(0, minLen + rng() % (o.size() - minLen + 1)); }
            else if (kind == 6 && !pats.empty()) p = pats[rng() % pats.size()];
            for (char &c : p) if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) c = alpha[rng() % na];             // (a pattern holds letters only)
            while (p.size() < minLen) p.push_back(alpha[rng() % na]);
            if (rng() % 2) for (char &c : p) c ^= 0x20;
            pats.push_back(p);
        }
        std::vector<uint64_t> patOff(1, 0);
        for (const std::string &p : pats) patOff.push_back(patOff.back() + p.size());
        uint8_t *patBytes = new uint8_t[patOff.back()];
        for (size_t q = 0; q < pats.size(); q++) memcpy(patBytes + patOff[q], pats[q].data(), pats[q].size());

        // ---- the obvious way
        std::vector<Hit> want;
        for (size_t r = 0; r < recs.size(); r++)
            for (size_t q = 0; q < pats.size(); q++)
                for (uint64_t p = 0; p + pats[q].size() <= recs[r].len; p++) {
                    uint32_t d = 0;
                    for (size_t j = 0; j < pats[q].size() && d <= K; j++) d += foldPlain(seq[recs[r].off + p + j]) != foldPlain((uint8_t) pats[q][j]);
                    if (d <= K) want.push_back(Hit((uint32_t) r, p, (uint32_t) q, d));
                }

        // ---- the kernel's way
        FindTable T;
        find_build_table(patBytes, patOff.data(), pats.size(), K, T);
        FindSlot *slots = exact(T.slots); FindSeed *seeds = exact(T.seeds); FindPat *ptab = exact(T.pats); uint8_t *folded = exact(T.bytes);
        bigTables += T.bits > 7;                                        // (more than 64 chains)
        std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
        for (size_t r = 0; r < recs.size(); r++) tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, find_positions(recs[r].len, T.shortest));
        uint64_t *tileStart = exact(tileStartV);
        ScanRec *recTab = exact(recs);
        std::vector<Hit> got;
        for (uint64_t tile = 0; tile < tileStartV.back(); tile++) {
            const ScanTile open = scan_tile(seq, recTab, tileStart, (uint32_t) recs.size(), tile);
            const uint32_t r = open.r;
            const ScanRec rec = open.rec;
            multiTile += tile != tileStart[r];
            const uintptr_t tileAddr = open.addr;
            uint8_t *stage = (uint8_t *) operator new[](FIND_STAGE, std::align_val_t(16));
            memset(stage, 0xee, FIND_STAGE);
            for (uint32_t lane = 0; lane < FIND_THREADS; lane++) find_stage_step(seq, seqBytes, tileAddr, lane, stage);
            find_stage_step(seq, seqBytes, tileAddr, FIND_VECS - 1, stage);
            for (uint32_t lane = 0; lane < FIND_THREADS; lane++)
                find_lane_step(seq, rec, tileAddr, lane, stage, slots, T.bits, seeds, ptab, folded, K,
                               [&](uint64_t pos, uint32_t pat, uint32_t d) { got.push_back(Hit(r, pos, pat, d)); });
            operator delete[](stage, std::align_val_t(16));
        }
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        total += want.size();
        for (const Hit &h : want) withMismatch += std::get<3>(h) != 0;
        const bool ok = got == want;
        if (!ok) {
            printf("MISMATCH in call %d: %zu hits, expected %zu; K = %u, %zu records, %zu patterns, %llu bytes\n", it, got.size(), want.size(), K, recs.size(), pats.size(),
                   (unsigned long long) seqBytes);
            std::vector<Hit> onlyGot, onlyWant;
            std::set_difference(got.begin(), got.end(), want.begin(), want.end(), std::back_inserter(onlyGot));
            std::set_difference(want.begin(), want.end(), got.begin(), got.end(), std::back_inserter(onlyWant));
            for (size_t i = 0; i < onlyGot.size() && i < 5; i++)
                printf("  not expected: rec %u pos %llu pattern %u mismatches %u\n", std::get<0>(onlyGot[i]), (unsigned long long) std::get<1>(onlyGot[i]), std::get<2>(onlyGot[i]), std::get<3>(onlyGot[i]));
            for (size_t i = 0; i < onlyWant.size() && i < 5; i++)
                printf("  missing: rec %u (off %llu len %llu) pos %llu pattern %u (%zu bytes) mismatches %u\n", std::get<0>(onlyWant[i]), (unsigned long long) recs[std::get<0>(onlyWant[i])].off,
                       (unsigned long long) recs[std::get<0>(onlyWant[i])].len, (unsigned long long) std::get<1>(onlyWant[i]), std::get<2>(onlyWant[i]), pats[std::get<2>(onlyWant[i])].size(), std::get<3>(onlyWant[i]));
        }
        delete[] alloc; delete[] patBytes; delete[] slots; delete[] seeds; delete[] ptab; delete[] folded; delete[] tileStart; delete[] recTab;
        if (!ok) return 1;
    }
    const uint64_t n = (uint64_t) iterations;
    if (total < 20 * n || withMismatch < 2 * n || multiTile < n / 8 || unaligned < n / 4 || bigTables < n / 16) {
        printf("the inputs are too easy: %llu hits, %llu with mismatches, %llu tiles behind a record's first, %llu unaligned buffers, %llu large tables\n",
               (unsigned long long) total, (unsigned long long) withMismatch, (unsigned long long) multiTile, (unsigned long long) unaligned, (unsigned long long) bigTables);
        return 1;
    }
    printf("ok: %d calls, %llu hits\n", iterations, (unsigned long long) total);
    return 0;
}
