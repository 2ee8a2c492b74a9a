// The lane step of k_fa_find_iupac and the host's table builder (mbgc_amd/csrc/fasta_find_iupac.h) as plain C++: every call cut into
// tiles as mbgc_fasta_find_iupac_dev cuts it, every tile staged vector by vector and then — the kernel's barrier — run lane by lane, the
// hits collected through the callback that is the kernel's atomic cursor, against a triple loop written from the rule alone (records x
// patterns x positions; a position matches iff the text byte is one of acgtuACGTU and its base is in the pattern letter's set, the sets
// spelled out as strings here). The whole table of hits must be equal, so a hit reported twice fails as a missing one does. Built with
// AddressSanitizer by tests/test_fasta_find_iupac_kernel_cpu.py: the text ends where its allocation ends (and, every other call, starts
// where it starts), the pattern blob, the table's arrays and the staging buffer are exactly as long as declared, so a read past an end
// ends the run. No GPU.
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
#include "../mbgc_amd/csrc/fasta_find_iupac.h"
}
using namespace fa;

typedef std::tuple<uint32_t, uint64_t, uint32_t, uint32_t> Hit;      // rec, pos, pattern, mismatches

// the rule, the obvious way: the set of a pattern letter as a string of bases, the base of a text byte as a character (0: none)
static const char *setOf(char c) {
    switch (c >= 'a' && c <= 'z' ? c - 32 : c) {
        case 'A': return "A"; case 'C': return "C"; case 'G': return "G"; case 'T': case 'U': return "T";
        case 'R': return "AG"; case 'Y': return "CT"; case 'S': return "CG"; case 'W': return "AT"; case 'K': return "GT"; case 'M': return "AC";
        case 'B': return "CGT"; case 'D': return "AGT"; case 'H': return "ACT"; case 'V': return "ACG"; case 'N': return "ACGT";
    }
    return nullptr;
}
static char baseOf(uint8_t b) {
    switch (b) {
        case 'a': case 'A': return 'A'; case 'c': case 'C': return 'C'; case 'g': case 'G': return 'G';
        case 't': case 'T': case 'u': case 'U': return 'T';
    }
    return 0;
}
static bool matches(char letter, uint8_t textByte) { const char b = baseOf(textByte); return b && strchr(setOf(letter), b); }
static uint32_t expansion(const std::string &p, size_t at) { uint32_t n = 1; for (size_t i = 0; i < 8; i++) n *= (uint32_t) strlen(setOf(p[at + i])); return n; }

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

static bool build(const std::vector<std::string> &pats, uint32_t K, IupacTable &T, uint64_t &badPat, uint32_t &badSeg, uint32_t &badGrams) {
    std::vector<uint64_t> patOff(1, 0);
    for (const std::string &p : pats) patOff.push_back(patOff.back() + p.size());
    uint8_t *patBytes = new uint8_t[patOff.back() ? patOff.back() : 1];
    for (size_t q = 0; q < pats.size(); q++) memcpy(patBytes + patOff[q], pats[q].data(), pats[q].size());
    const bool ok = iupac_build_table(patBytes, patOff.data(), pats.size(), K, T, badPat, badSeg, badGrams);
    delete[] patBytes;
    return ok;
}

// the builder's own cases: the window of a segment is the cheapest one, the leftmost on a tie; 256 grams are accepted, 1024 refused
static bool builderCases() {
    IupacTable T;
    uint64_t bp = 0; uint32_t bs = 0, bg = 0;
    // one segment of 12 letters, A C G N A C G T A R A C: the windows at 0..3 hold the N (4 grams and more), the one at 4 = ACGTARAC only
    // the R (2 grams): the best window is not the first
    if (!build({"ACGNACGTARAC"}, 0, T, bp, bs, bg) || T.pats[0].win[0] != 4 || T.rows.size() != 2) { printf("builder: the best window is not the first\n"); return false; }
    // a tie: ACGTACGTA has two windows of one gram each -> the leftmost
    if (!build({"ACGTACGTA"}, 0, T, bp, bs, bg) || T.pats[0].win[0] != 0 || T.rows.size() != 1) { printf("builder: a tie takes the leftmost window\n"); return false; }
    // four N in a row: exactly 256 grams, accepted, and every row a distinct gram
    if (!build({"ACNNNNGT"}, 0, T, bp, bs, bg) || T.rows.size() != 256) { printf("builder: 256 grams are accepted\n"); return false; }
    uint32_t set = 0;
    for (uint32_t w : T.bitmap) set += (uint32_t) __builtin_popcount(w);
    if (set != 256 || T.gramStart[IUPAC_GRAMS] != 256) { printf("builder: 256 distinct grams\n"); return false; }
    // five N: 1024, refused; as the second segment of the second pattern at K = 1
    if (build({"ACNNNNNT"}, 0, T, bp, bs, bg) || bp != 0 || bs != 0 || bg != 1024) { printf("builder: 1024 grams are refused\n"); return false; }
    if (build({"ACGTACGTACGTACGT", "ACGTACGTANNNNNCG"}, 1, T, bp, bs, bg) || bp != 1 || bs != 1 || bg != 1024) { printf("builder: the refusal names pattern and segment\n"); return false; }
    // ... but a longer segment that holds a cheaper window behind the run of N is accepted: window 5 = RACGTACG (x2)
    if (!build({"NNNNNRACGTACG"}, 0, T, bp, bs, bg) || T.pats[0].win[0] != 5 || T.rows.size() != 2) { printf("builder: a cheap window behind a run of N\n"); return false; }
    // every letter of the table, either case; anything else has no set
    const char *letters = "ACGTURYSWKMBDHVN";
    for (int c = 0; c < 256; c++) {
        const bool inTable = c && (strchr(letters, c) || (c >= 'a' && c <= 'z' && strchr(letters, c - 32)));
        uint32_t want = 0;
        if (inTable) for (const char *s = setOf((char) c); *s; s++) want |= 1u << (strchr("ACGT", *s) - "ACGT");
        if (iupac_mask((uint8_t) c) != want) { printf("builder: the mask of byte %d\n", c); return false; }
        const char b = baseOf((uint8_t) c);
        if (iupac_onehot((uint8_t) c) != (b ? 1u << (strchr("ACGT", b) - "ACGT") : 0u)) { printf("the base of byte %d\n", c); return false; }
    }
    return true;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 400;
    if (!builderCases()) return 1;
    std::mt19937_64 rng(31);
    uint64_t total = 0, withMismatch = 0, multiTile = 0, unaligned = 0, bigTables = 0, degenerateHits = 0, laterWindows = 0, firstLast = 0, wide = 0, walkedAll = 0;
    uint32_t offsetsSeen = 0, addressesSeen = 0;                       // bit m: a scanned record with off % 16 == m / whose first byte's address % 16 == m
    const std::string letters = "ACGTURYSWKMBDHVN";
    for (int it = 0; it < iterations; it++) {
        // text: mostly bases in both cases, so that patterns drawn at random stand in it, with the bytes that have no base sprinkled in
        const std::string textAlpha = it % 3 == 0 ? "aAcC" : (it % 3 == 1 ? "aAuUtT" : "ACGTacgtUu");
        const char odd[] = {'N', 'n', 'R', 'Y', '-', 0};
        const bool big = it % 8 == 0;
        const uint64_t seqBytes = big ? 2 * FIND_TILE + rng() % (2 * FIND_TILE) : 1 + rng() % 700;
        const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;   // the buffer's first byte: any alignment
        uint8_t *alloc = new uint8_t[seqBytes + shift], *seq = alloc + shift;
        const unsigned oddEvery = it % 4 == 0 ? 13 : 61;
        for (uint64_t i = 0; i < seqBytes; i++) seq[i] = rng() % oddEvery == 0 ? (uint8_t) odd[rng() % sizeof odd] : (uint8_t) textAlpha[rng() % textAlpha.size()];
        if (it % 5 == 0) { const uint64_t a = rng() % seqBytes, n = std::min<uint64_t>(seqBytes - a, 1 + rng() % 300); memset(seq + a, 'a', n); }   // a run of one base
        if (it % 5 == 1) { const uint64_t a = rng() % seqBytes, n = std::min<uint64_t>(seqBytes - a, 1 + rng() % 40); memset(seq + a, 'N', n); }    // a run of N
        unaligned += ((uintptr_t) seq & 15) != 0;
        const uint32_t K = (uint32_t) (rng() % 4);
        const uint32_t minLen = IUPAC_GRAM * (K + 1);
        // records: anywhere, of any length — empty ones, ones of a few bytes, of exactly the shortest pattern's length and one less, the
        // whole buffer, neighbours, overlapping ones, the same one twice, unsorted; every off % 16 comes by over the calls (r + it)
        std::vector<ScanRec> recs;
        const int nrec = 1 + (int) (rng() % 9);
        for (int r = 0; r < nrec; r++) {
            const uint64_t lc[] = {0, 1, 7, 8, minLen - 1, minLen, seqBytes, rng() % 40, rng() % (seqBytes + 1), rng() % (seqBytes + 1)};
            uint64_t len = std::min(lc[rng() % 10], seqBytes), off = rng() % (seqBytes - len + 1);
            if (rng() % 3 == 0 && seqBytes > 16 + len) off = (off & ~(uint64_t) 15) + (uint64_t) (r + it) % 16, off = std::min(off, seqBytes - len);
            if (r && rng() % 4 == 0) { off = recs[r - 1].off + recs[r - 1].len; len = std::min(len, seqBytes - off); }     // right behind the one before
            if (r && rng() % 6 == 0) { off = recs[r - 1].off; len = recs[r - 1].len; }                                     // the same again
            if (r && rng() % 6 == 0) { off = recs[r - 1].off + recs[r - 1].len / 2; len = std::min(len, seqBytes - off); } // over the one before
            if (rng() % 5 == 0) { off = seqBytes - len; }                                                                 // ends with the buffer
            recs.push_back(ScanRec{off, len});
        }
        // patterns: pieces of the text — from a record's first and last position, from anywhere —, bytes without a base replaced, letters
        // widened to codes that hold the base (a match) or exclude it (a mismatch), in both cases; random ones over the whole table;
        // prefixes of others; the same one twice; long ones that span tiles
        const int npat = 1 + (int) (rng() % (it % 7 == 0 ? 120 : 8));
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
            }
            else if (kind == 4 && seqBytes >= len) p.assign((const char *) seq + rng() % (seqBytes - len + 1), len);       // anywhere in the buffer: over joints
            else if (kind == 5 && !pats.empty()) { const std::string &o = pats[rng() % pats.size()]; p = o.substr(0, minLen + rng() % (o.size() - minLen + 1)); }
            else if (kind == 6 && !pats.empty()) p = pats[rng() % pats.size()];
            else if (kind == 7) for (uint32_t i = 0; i < len; i++) p.push_back(letters[rng() % letters.size()]);
            while (p.size() < minLen) p.push_back(textAlpha[rng() % textAlpha.size()]);
            if (kind <= 4) {
                for (char &c : p) if (!baseOf((uint8_t) c)) c = textAlpha[rng() % textAlpha.size()];
                // widen: every code that holds the letter's base keeps the match
                const uint32_t widen = (uint32_t) (rng() % 3 == 0 ? p.size() / 3 : rng() % 4);
                for (uint32_t s = 0; s < widen; s++) {
                    const size_t j = rng() % p.size();
                    const char b = baseOf((uint8_t) p[j]);
                    if (!b) continue;
                    char c;
                    do c = letters[rng() % letters.size()]; while (!strchr(setOf(c), b));
                    p[j] = c;
                }
                // ... and up to K + 1 letters that exclude it (or anything at all)
                const uint32_t subs = (uint32_t) (rng() % (K + 2));
                for (uint32_t s = 0; s < subs; s++) {
                    const size_t j = rng() % 3 == 0 ? (rng() % 2 ? 0 : p.size() - 1) : rng() % p.size();
                    p[j] = letters[rng() % letters.size()];
                }
            }
            if (rng() % 2) for (char &c : p) c = (char) (c >= 'A' && c <= 'Z' ? c + 32 : (c >= 'a' && c <= 'z' ? c - 32 : c));
            pats.push_back(p);
        }
        // (a window past the cap: narrow the offending segment until the builder takes the list)
        IupacTable T;
        uint64_t bp = 0; uint32_t bs = 0, bg = 0;
        while (!build(pats, K, T, bp, bs, bg)) {
            std::string &p = pats[bp];
            const uint32_t step = (uint32_t) p.size() / (K + 1);
            for (uint32_t i = 0; i < 4; i++) p[bs * step + rng() % step] = "ACGT"[rng() % 4];
        }
        for (size_t q = 0; q < pats.size(); q++)
            for (uint32_t j = 0; j <= K; j++) {
                const uint32_t step = (uint32_t) pats[q].size() / (K + 1);
                laterWindows += T.pats[q].win[j] != j * step;
                wide += expansion(pats[q], T.pats[q].win[j]) >= 64;
                // the window is the cheapest of its segment, the leftmost on a tie
                for (uint32_t w = 0; w + 8 <= step; w++) {
                    const uint32_t e = expansion(pats[q], j * step + w), mine = expansion(pats[q], T.pats[q].win[j]);
                    if (e < mine || (e == mine && j * step + w < T.pats[q].win[j])) { printf("call %d: pattern %zu segment %u: window %u is not the best\n", it, q, j, T.pats[q].win[j]); return 1; }
                }
            }

        // ---- the obvious way
        std::vector<Hit> want;
        for (size_t r = 0; r < recs.size(); r++)
            for (size_t q = 0; q < pats.size(); q++)
                for (uint64_t p = 0; p + pats[q].size() <= recs[r].len; p++) {
                    uint32_t d = 0;
                    bool degenerate = false;
                    for (size_t j = 0; j < pats[q].size() && d <= K; j++) {
                        d += !matches(pats[q][j], seq[recs[r].off + p + j]);
                        degenerate |= strlen(setOf(pats[q][j])) > 1;
                    }
                    if (d <= K) {
                        want.push_back(Hit((uint32_t) r, p, (uint32_t) q, d));
                        degenerateHits += degenerate;
                        firstLast += p == 0 || p + pats[q].size() == recs[r].len;
                    }
                }

        // ---- the kernel's way
        uint32_t *bitmap = exact(T.bitmap), *gramStart = exact(T.gramStart);
        IupacRow *rows = exact(T.rows); IupacPat *ptab = exact(T.pats); uint8_t *masks = exact(T.masks);
        bigTables += T.rows.size() > 256;
        std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
        for (size_t r = 0; r < recs.size(); r++) {
            tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, find_positions(recs[r].len, T.shortest));
            if (tileStartV[r + 1] != tileStartV[r]) { offsetsSeen |= 1u << (recs[r].off & 15); addressesSeen |= 1u << (((uintptr_t) seq + recs[r].off) & 15); }
        }
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
            memset(stage, 'A', FIND_STAGE);                              // (what an earlier tile may have left: bases, the worst case)
            for (uint32_t lane = 0; lane < FIND_THREADS; lane++) find_stage_step(seq, seqBytes, tileAddr, lane, stage);
            find_stage_step(seq, seqBytes, tileAddr, FIND_VECS - 1, stage);
            for (uint32_t lane = 0; lane < FIND_THREADS; lane++)
                walkedAll += iupac_lane_step(seq, rec, tileAddr, lane, stage, bitmap, gramStart, rows, ptab, masks, K,
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
                printf("  not expected: rec %u pos %llu pattern %u (%s) mismatches %u\n", std::get<0>(onlyGot[i]), (unsigned long long) std::get<1>(onlyGot[i]), std::get<2>(onlyGot[i]),
                       pats[std::get<2>(onlyGot[i])].substr(0, 80).c_str(), std::get<3>(onlyGot[i]));
            for (size_t i = 0; i < onlyWant.size() && i < 5; i++)
                printf("  missing: rec %u (off %llu len %llu) pos %llu pattern %u (%s) mismatches %u\n", std::get<0>(onlyWant[i]), (unsigned long long) recs[std::get<0>(onlyWant[i])].off,
                       (unsigned long long) recs[std::get<0>(onlyWant[i])].len, (unsigned long long) std::get<1>(onlyWant[i]), std::get<2>(onlyWant[i]),
                       pats[std::get<2>(onlyWant[i])].substr(0, 80).c_str(), std::get<3>(onlyWant[i]));
        }
        delete[] alloc; delete[] bitmap; delete[] gramStart; delete[] rows; delete[] ptab; delete[] masks; delete[] tileStart; delete[] recTab;
        if (!ok) return 1;
    }
    const uint64_t n = (uint64_t) iterations;
    if (total < 20 * n || withMismatch < 2 * n || multiTile < n / 8 || unaligned < n / 4 || bigTables < n / 16 || degenerateHits < 5 * n || laterWindows < n / 2 ||
        firstLast < n / 2 || wide < n / 8 || offsetsSeen != 0xffff || addressesSeen != 0xffff) {
        printf("the inputs are too easy: %llu hits, %llu with mismatches, %llu of degenerate patterns, %llu at a record's first or last position, %llu tiles behind a record's first, "
               "%llu unaligned buffers, %llu large tables, %llu windows that are not their segment's first, %llu of 64 grams and more; scanned records' off %% 16 seen: %04x, their addresses' %% 16: %04x\n",
               (unsigned long long) total, (unsigned long long) withMismatch, (unsigned long long) degenerateHits, (unsigned long long) firstLast, (unsigned long long) multiTile,
               (unsigned long long) unaligned, (unsigned long long) bigTables, (unsigned long long) laterWindows, (unsigned long long) wide, offsetsSeen, addressesSeen);
        return 1;
    }
    printf("ok: %d calls, %llu hits, %llu rows walked\n", iterations, (unsigned long long) total, (unsigned long long) walkedAll);
    return 0;
}
