// The lane steps of k_fa_sketch (mbgc_amd/csrc/fasta_sketch.h) as plain C++: every call cut into tiles as mbgc_fasta_sketch_dev cuts it,
// every tile run lane by lane — the wave's shuffles are arrays here: a lane takes the packed words of the two lanes behind it out of the
// array of the lanes' words, and the last two lanes of a wave pack the vectors behind the wave themselves, as the kernel does. Against a
// byte loop written the obvious way: every k-mer built from scratch out of the record's bytes, its reverse complement by reversing the
// string, the hash from the two. The whole tables (record, position, hash) and the valid positions per record must be equal. Built with
// AddressSanitizer by tests/test_fasta_sketch_kernel_cpu.py: the text is exactly seqBytes long (and, every other call, starts where its
// allocation starts), so a read outside it ends the run. Records start at every offset mod 16, have 0, k - 1, k and k + 1 bytes, and end
// on the buffer's last byte, k around a tile's edge and k around a wave's edge (1024 positions). The program prints how many k-mers it
// compared per k and how many of them were their own reverse complement. Also: the pair index and the bisection of k_fa_sketch_pairs
// against loops. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
namespace fa {
#include "../mbgc_amd/csrc/fasta_tiles.h"
#include "../mbgc_amd/csrc/fasta_sketch.h"
}
using namespace fa;

typedef std::tuple<uint32_t, uint64_t, uint64_t> Row;                // rec, position, hash

static int codeOf(uint8_t b) {
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return -1;
    }
}
static uint64_t fmix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
static uint64_t wordOf(const std::vector<int> &codes) {            // the first code in the highest pair
    uint64_t w = 0;
    for (const int c : codes) w = (w << 2) | (uint64_t) c;
    return w;
}

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 16;
    std::mt19937_64 rng(47);
    const char alpha[] = {'A', 'C', 'G', 'T', 'N', 'a', 'c', 'g', 't', 'n', 'R', 'Y', 'U', '>', '\0'};
    const char letters[] = {'A', 'C', 'G', 'T', 'a', 'c', 'g', 't', 'U'};
    const uint32_t ks[] = {1, 2, 15, 16, 17, 31, 32};
    // ---- the pair index and the bisection
    for (uint32_t n = 2; n < 40; n++) {
        uint64_t q = 0;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++, q++) {
                uint32_t gi, gj;
                sketch_pair_of(q, n, gi, gj);
                if (gi != i || gj != j) { printf("MISMATCH: pair %llu of %u groups is (%u, %u), expected (%u, %u)\n", (unsigned long long) q, n, gi, gj, i, j); return 1; }
            }
    }
    for (uint64_t n = 0; n < 70; n++) {
        std::vector<uint64_t> list;
        for (uint64_t i = 0; i < n; i++) list.push_back(3 * i + 1);
        uint64_t *l = exact(list);
        for (uint64_t x = 0; x < 3 * n + 3; x++)
            if (sketch_holds(l, n, x) != (x % 3 == 1 && x < 3 * n)) { printf("MISMATCH: %llu in a list of %llu\n", (unsigned long long) x, (unsigned long long) n); return 1; }
        delete[] l;
    }
    // ---- the scan
    for (const uint32_t k : ks) {
        uint64_t compared = 0, palindromes = 0, skipped = 0, atBufferEnd = 0;
        for (int it = 0; it < iterations; it++) {
            const uint64_t seqBytes = 2 * SKETCH_TILE + 100 + rng() % SKETCH_TILE;
            const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;     // the buffer's first byte: any alignment
            uint8_t *alloc = new uint8_t[seqBytes + shift], *seq = alloc + shift;
            // letters, now and then a byte of the whole alphabet, now and then a stretch of them; k-mers that are their own reverse
            // complement planted (even k)
            for (uint64_t i = 0; i < seqBytes; i++) seq[i] = (uint8_t) (rng() % 50 == 0 ? alpha[rng() % sizeof alpha] : letters[rng() % sizeof letters]);
            for (int s = 0; s < 6; s++) {
                const uint64_t at = rng() % seqBytes, n = std::min<uint64_t>(1 + rng() % 60, seqBytes - at);
                for (uint64_t i = 0; i < n; i++) seq[at + i] = (uint8_t) alpha[rng() % sizeof alpha];
            }
            if (k % 2 == 0)
                for (int s = 0; s < 8; s++) {
                    const uint64_t at = rng() % (seqBytes - k);
                    for (uint32_t i = 0; i < k / 2; i++) {
                        const int c = (int) (rng() % 4);
                        seq[at + i] = (uint8_t) "ACGT"[c];
                        seq[at + k - 1 - i] = (uint8_t) "tgca"[c];
                    }
                }
            // records: a start at every offset mod 16 of the buffer's addresses; the lengths and ends the header names
            std::vector<ScanRec> recs;
            for (uint32_t r = 0; r < 16; r++) {
                uint64_t off = rng() % 200;
                while (((uintptr_t) seq + off) % 16 != r) off++;
                const uint64_t grid = ((uintptr_t) seq + off) & 15;     // the record's first position on its first tile
                const uint64_t edges[] = {SKETCH_TILE - grid, 1024 - grid, 2 * SKETCH_TILE - grid};
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
            std::vector<uint64_t> wantValid(recs.size(), 0);
            for (size_t r = 0; r < recs.size(); r++)
                for (uint64_t p = 0; p + k <= recs[r].len; p++) {
                    std::vector<int> fwd, rev;
                    bool ok = true;
                    for (uint32_t i = 0; i < k && ok; i++) { const int c = codeOf(seq[recs[r].off + p + i]); ok = c >= 0; fwd.push_back(c); }
                    if (!ok) { skipped++; continue; }
                    for (uint32_t i = 0; i < k; i++) rev.push_back(3 - fwd[k - 1 - i]);
                    const uint64_t fw = wordOf(fwd), rc = wordOf(rev);
                    palindromes += fw == rc;
                    want.push_back(Row((uint32_t) r, p, fmix(std::min(fw, rc) ^ 0x9E3779B97F4A7C15ull)));
                    wantValid[r]++;
                }

            // ---- the kernel's way
            std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
            for (size_t r = 0; r < recs.size(); r++) tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, sketch_positions(recs[r].len, k));
            uint64_t *tileStart = exact(tileStartV);
            ScanRec *recTab = exact(recs);
            std::vector<Row> got;
            std::vector<uint64_t> gotValid(recs.size(), 0);
            for (uint64_t tile = 0; tile < tileStartV.back(); tile++) {
                const ScanTile open = scan_tile(seq, recTab, tileStart, (uint32_t) recs.size(), tile);
                const uint32_t r = open.r;
                const ScanRec rec = open.rec;
                const uintptr_t tileAddr = open.addr;
                uint64_t own[SKETCH_THREADS];
                for (uint32_t lane = 0; lane < SKETCH_THREADS; lane++) own[lane] = sketch_pack(seq, seqBytes, rec, tileAddr + 16u * lane);
                for (uint32_t lane = 0; lane < SKETCH_THREADS; lane++) {
                    const uint32_t wl = lane & 63;
                    const uintptr_t v = tileAddr + 16u * lane;
                    const uint64_t next1 = wl == 63 ? sketch_pack(seq, seqBytes, rec, v + 16) : own[lane + 1];
                    const uint64_t next2 = wl >= 62 ? sketch_pack(seq, seqBytes, rec, v + 32) : own[lane + 2];
                    uint64_t h[SKETCH_PER];
                    const uint32_t valid = sketch_lane_hashes(own[lane], next1, next2, k, h);
                    const int64_t t0 = (int64_t) v - (int64_t) ((uintptr_t) seq + rec.off);
                    for (uint32_t j = 0; j < SKETCH_PER; j++)
                        if ((valid >> j) & 1u) { got.push_back(Row(r, (uint64_t) (t0 + j), h[j])); gotValid[r]++; }
                }
            }
            std::sort(got.begin(), got.end());
            std::sort(want.begin(), want.end());
            compared += want.size();
            const bool ok = got == want && gotValid == wantValid;
            if (!ok) {
                printf("MISMATCH at k = %u in call %d: %zu k-mers, expected %zu; %llu bytes\n", k, it, got.size(), want.size(), (unsigned long long) seqBytes);
                std::vector<Row> onlyGot, onlyWant;
                std::set_difference(got.begin(), got.end(), want.begin(), want.end(), std::back_inserter(onlyGot));
                std::set_difference(want.begin(), want.end(), got.begin(), got.end(), std::back_inserter(onlyWant));
                for (size_t i = 0; i < onlyGot.size() && i < 5; i++)
                    printf("  not expected: rec %u (off %llu len %llu) pos %llu hash %016llx\n", std::get<0>(onlyGot[i]), (unsigned long long) recs[std::get<0>(onlyGot[i])].off,
                           (unsigned long long) recs[std::get<0>(onlyGot[i])].len, (unsigned long long) std::get<1>(onlyGot[i]), (unsigned long long) std::get<2>(onlyGot[i]));
                for (size_t i = 0; i < onlyWant.size() && i < 5; i++)
                    printf("  missing: rec %u (off %llu len %llu) pos %llu hash %016llx\n", std::get<0>(onlyWant[i]), (unsigned long long) recs[std::get<0>(onlyWant[i])].off,
                           (unsigned long long) recs[std::get<0>(onlyWant[i])].len, (unsigned long long) std::get<1>(onlyWant[i]), (unsigned long long) std::get<2>(onlyWant[i]));
            }
            delete[] alloc; delete[] tileStart; delete[] recTab;
            if (!ok) return 1;
        }
        if (skipped < 100 || atBufferEnd < (uint64_t) iterations) {
            printf("the inputs are too easy at k = %u: %llu k-mers with an invalid byte, %llu records that end with the buffer\n", k, (unsigned long long) skipped, (unsigned long long) atBufferEnd);
            return 1;
        }
        printf("k %u: %llu k-mers compared, %llu palindromic, %llu skipped\n", k, (unsigned long long) compared, (unsigned long long) palindromes, (unsigned long long) skipped);
    }
    printf("ok\n");
    return 0;
}
