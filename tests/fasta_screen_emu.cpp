// The lane steps of k_fa_screen (mbgc_amd/csrc/fasta_screen.h) as plain C++, with the host's builders of the filter and the table — the
// very functions the entry point calls: every call cut into tiles as mbgc_fasta_screen_dev cuts it, every tile run lane by lane — the
// wave's shuffles are arrays here, and the last two lanes of a wave pack the vectors behind the wave themselves, as the kernel does; a
// lane asks screen_first about all its valid positions, reads the keys behind the slots, then screen_confirm, in the kernel's order.
// Against a byte loop written the obvious way: every k-mer built from scratch out of the record's bytes, its reverse complement by
// reversing the string, the smaller of the two looked up in a std::set. The whole tables (record, position, key index) must be equal.
// The keys are k-mers of the text itself (so there are hits), their reverse complements' canonical forms with them by construction, and
// random words (so that filter bits are set that no text k-mer owns). Built with AddressSanitizer by
// tests/test_fasta_screen_kernel_cpu.py: the text, the keys, the filter and the table are allocations of exactly their sizes, so a read
// outside one ends the run. Records start at every offset mod 16, have 0, k - 1, k and k + 1 bytes, and end on the buffer's last byte, k
// around a tile's edge and k around a wave's edge. Per k the program prints the positions compared, the hits, the filter passes the
// table refuted, and the longest probe chain. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <tuple>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
namespace fa {
#include "../mbgc_amd/csrc/fasta_tiles.h"
#include "../mbgc_amd/csrc/fasta_sketch.h"
#include "../mbgc_amd/csrc/fasta_screen.h"
}
using namespace fa;

typedef std::tuple<uint32_t, uint64_t, uint32_t> Row;                // rec, position, key index

static int codeOf(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return -1;
    }
}
static uint64_t wordOf(const std::vector<int> &codes) {            // the first code in the highest pair
    uint64_t w = 0;
    for (const int c : codes) w = (w << 2) | (uint64_t) c;
    return w;
}
// the canonical word of the k bytes at p, false when one of them is invalid — the obvious way
static bool canonAt(const uint8_t *p, uint32_t k, uint64_t &canon) {
    std::vector<int> fwd, rev;
    for (uint32_t i = 0; i < k; i++) { const int c = codeOf(p[i]); if (c < 0) return false; fwd.push_back(c); }
    for (uint32_t i = 0; i < k; i++) rev.push_back(3 - fwd[k - 1 - i]);
    canon = std::min(wordOf(fwd), wordOf(rev));
    return true;
}

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 16;
    std::mt19937_64 rng(53);
    const char alpha[] = {'A', 'C', 'G', 'T', 'N', 'a', 'c', 'g', 't', 'n', 'R', 'Y', 'U', '>', '\0'};
    const char letters[] = {'A', 'C', 'G', 'T', 'a', 'c', 'g', 't', 'U'};
    const uint32_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    for (uint64_t n = 0; n < 70; n++) {                              // the slot count: the power of two >= 2 n
        const uint64_t s = screen_slots(n);
        if (s < 2 || s < 2 * n || (s & (s - 1)) || (s > 2 && s / 2 >= 2 * n)) { printf("MISMATCH: %llu keys get %llu slots\n", (unsigned long long) n, (unsigned long long) s); return 1; }
    }
    for (const uint32_t k : ks) {
        uint64_t compared = 0, hitsSeen = 0, refuted = 0, passed = 0, skipped = 0, atBufferEnd = 0;
        uint32_t longestChain = 0;
        for (int it = 0; it < iterations; it++) {
            const uint64_t seqBytes = 2 * SCAN_TILE + 100 + rng() % SCAN_TILE;
            const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;     // the buffer's first byte: any alignment
            uint8_t *alloc = new uint8_t[seqBytes + shift], *seq = alloc + shift;
            for (uint64_t i = 0; i < seqBytes; i++) seq[i] = (uint8_t) (rng() % 50 == 0 ? alpha[rng() % sizeof alpha] : letters[rng() % sizeof letters]);
            for (int s = 0; s < 6; s++) {
                const uint64_t at = rng() % seqBytes, n = std::min<uint64_t>(1 + rng() % 60, seqBytes - at);
                for (uint64_t i = 0; i < n; i++) seq[at + i] = (uint8_t) alpha[rng() % sizeof alpha];
            }
            if (k % 2 == 0)                                              // k-mers that are their own reverse complement
                for (int s = 0; s < 8; s++) {
                    const uint64_t at = rng() % (seqBytes - k);
                    for (uint32_t i = 0; i < k / 2; i++) {
                        const int c = (int) (rng() % 4);
                        seq[at + i] = (uint8_t) "ACGT"[c];
                        seq[at + k - 1 - i] = (uint8_t) "tgca"[c];
                    }
                }
            // ---- the keys: the k-mers of every third stretch of 200 positions, and random words of 2 k bits — many more of those at the
            // larger k, where a random word is no k-mer of the text: they set filter bits and fill slots that text k-mers run into
            std::set<uint64_t> keySet;
            for (uint64_t p = 0; p + k <= seqBytes; p++) {
                uint64_t c;
                if ((p / 200) % 3 == 0 && canonAt(seq + p, k, c)) keySet.insert(c);
            }
            const uint64_t extra = k >= 15 ? 20000 + rng() % 30000 : 3;
            for (uint64_t i = 0; i < extra; i++) {
                const uint64_t w = k == 32 ? rng() : rng() & (((uint64_t) 1 << (2 * k)) - 1);
                keySet.insert(screen_canon(w, k));
            }
            if (it == 0) { const uint64_t only = *keySet.begin(); keySet.clear(); keySet.insert(only); }     // a single key
            const std::vector<uint64_t> keyList(keySet.begin(), keySet.end());
            const uint64_t nkeys = keyList.size(), slots = screen_slots(nkeys);
            uint64_t *keys = exact(keyList);
            uint32_t *filter = new uint32_t[SCREEN_FILTER_WORDS], *table = new uint32_t[slots];
            const uint64_t bits = screen_build_filter(keys, nkeys, filter);
            longestChain = std::max(longestChain, screen_build_table(keys, nkeys, table, slots));
            uint64_t counted = 0, filled = 0;
            for (uint32_t w = 0; w < SCREEN_FILTER_WORDS; w++) counted += (uint64_t) __builtin_popcount(filter[w]);
            for (uint64_t s = 0; s < slots; s++) filled += table[s] != 0;
            if (counted != bits || bits > nkeys || filled != nkeys) { printf("MISMATCH: %llu keys set %llu filter bits (%llu counted) and fill %llu slots\n", (unsigned long long) nkeys, (unsigned long long) bits, (unsigned long long) counted, (unsigned long long) filled); return 1; }
            const uint32_t slotMask = (uint32_t) (slots - 1);

            // records: a start at every offset mod 16 of the buffer's addresses; the lengths and ends the header names
            std::vector<ScanRec> recs;
            for (uint32_t r = 0; r < 16; r++) {
                uint64_t off = rng() % 200;
                while (((uintptr_t) seq + off) % 16 != r) off++;
                const uint64_t grid = ((uintptr_t) seq + off) & 15;
                const uint64_t edges[] = {SCAN_TILE - grid, 1024 - grid, 2 * SCAN_TILE - grid};
                const uint64_t edge = edges[rng() % 3];
                const uint64_t lc[] = {0, k - 1, k, k + 1, seqBytes - off, edge - k, edge + k, edge - 1, edge, edge + 1, edge + k - 1, edge - k + 1, rng() % (seqBytes - off + 1)};
                const uint64_t len = std::min(lc[(it + r) % 13], seqBytes - off);
                recs.push_back(ScanRec{off, len});
                atBufferEnd += off + len == seqBytes && len >= k;
            }
            recs.push_back(ScanRec{seqBytes - k, k});                    // one k-mer, the buffer's last bytes
            recs.push_back(ScanRec{seqBytes, 0});
            recs.push_back(recs[rng() % 16]);                            // the same again
            atBufferEnd++;

            // ---- the obvious way
            std::vector<Row> want;
            uint64_t wantValid = 0;
            for (size_t r = 0; r < recs.size(); r++)
                for (uint64_t p = 0; p + k <= recs[r].len; p++) {
                    uint64_t c;
                    if (!canonAt(seq + recs[r].off + p, k, c)) { skipped++; continue; }
                    wantValid++;
                    if (keySet.count(c)) want.push_back(Row((uint32_t) r, p, (uint32_t) (std::lower_bound(keyList.begin(), keyList.end(), c) - keyList.begin())));     // (its place in the ascending list)
                }

            // ---- the kernel's way
            std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
            for (size_t r = 0; r < recs.size(); r++) tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, sketch_positions(recs[r].len, k));
            uint64_t *tileStart = exact(tileStartV);
            ScanRec *recTab = exact(recs);
            std::vector<Row> got;
            uint64_t gotValid = 0;
            for (uint64_t tile = 0; tile < tileStartV.back(); tile++) {
                const ScanTile open = scan_tile(seq, recTab, tileStart, (uint32_t) recs.size(), tile);
                const ScanRec rec = open.rec;
                uint64_t own[SCREEN_THREADS];
                for (uint32_t lane = 0; lane < SCREEN_THREADS; lane++) own[lane] = sketch_pack(seq, seqBytes, rec, open.addr + 16u * lane);
                for (uint32_t lane = 0; lane < SCREEN_THREADS; lane++) {
                    const uint32_t wl = lane & 63;
                    const uintptr_t v = open.addr + 16u * lane;
                    const uint64_t next1 = wl == 63 ? sketch_pack(seq, seqBytes, rec, v + 16) : own[lane + 1];
                    const uint64_t next2 = wl >= 62 ? sketch_pack(seq, seqBytes, rec, v + 32) : own[lane + 2];
                    uint64_t c[SCREEN_PER];
                    const uint32_t valid = screen_lane_canons(own[lane], next1, next2, k, c);
                    uint32_t e[SCREEN_PER], pass = 0;
                    for (uint32_t j = 0; j < SCREEN_PER; j++) {
                        e[j] = 0;
                        if (((valid >> j) & 1u) && screen_first(filter, table, slotMask, c[j], e[j])) pass |= 1u << j;
                    }
                    gotValid += (uint64_t) __builtin_popcount(valid);
                    passed += (uint64_t) __builtin_popcount(pass);
                    const int64_t t0 = (int64_t) v - (int64_t) ((uintptr_t) seq + rec.off);
                    for (uint32_t j = 0; j < SCREEN_PER; j++) {
                        if (!((pass >> j) & 1u)) continue;
                        uint32_t steps = 0;
                        const uint32_t hit = screen_confirm(table, slotMask, keys, c[j], e[j], e[j] ? keys[e[j] - 1] : 0, steps);
                        longestChain = std::max(longestChain, steps);
                        if (hit) got.push_back(Row(open.r, (uint64_t) (t0 + j), hit - 1)); else refuted++;
                    }
                }
            }
            std::sort(got.begin(), got.end());
            std::sort(want.begin(), want.end());
            compared += wantValid;
            hitsSeen += want.size();
            const bool ok = got == want && gotValid == wantValid;
            if (!ok) {
                printf("MISMATCH at k = %u in call %d: %zu hits, expected %zu; %llu valid positions, expected %llu; %llu keys\n", k, it, got.size(), want.size(),
                       (unsigned long long) gotValid, (unsigned long long) wantValid, (unsigned long long) nkeys);
                std::vector<Row> onlyGot, onlyWant;
                std::set_difference(got.begin(), got.end(), want.begin(), want.end(), std::back_inserter(onlyGot));
                std::set_difference(want.begin(), want.end(), got.begin(), got.end(), std::back_inserter(onlyWant));
                for (size_t i = 0; i < onlyGot.size() && i < 5; i++)
                    printf("  not expected: rec %u pos %llu key %u\n", std::get<0>(onlyGot[i]), (unsigned long long) std::get<1>(onlyGot[i]), std::get<2>(onlyGot[i]));
                for (size_t i = 0; i < onlyWant.size() && i < 5; i++)
                    printf("  missing: rec %u pos %llu key %u\n", std::get<0>(onlyWant[i]), (unsigned long long) std::get<1>(onlyWant[i]), std::get<2>(onlyWant[i]));
            }
            delete[] alloc; delete[] tileStart; delete[] recTab; delete[] keys; delete[] filter; delete[] table;
            if (!ok) return 1;
        }
        if (skipped < 100 || atBufferEnd < (uint64_t) iterations) {
            printf("the inputs are too easy at k = %u: %llu k-mers with an invalid byte, %llu records that end with the buffer\n", k, (unsigned long long) skipped, (unsigned long long) atBufferEnd);
            return 1;
        }
        printf("k %u: %llu positions compared, %llu hits, %llu filter passes, %llu refuted by the table, longest probe chain %u\n", k, (unsigned long long) compared,
               (unsigned long long) hitsSeen, (unsigned long long) passed, (unsigned long long) refuted, longestChain);
    }
    printf("ok\n");
    return 0;
}
