// The lane steps of k_fa_stats (mbgc_amd/csrc/fasta_stats.h) as plain C++: every call cut into tiles as mbgc_fasta_stats_dev cuts it, every
// tile run lane by lane — the wave's shuffles are arrays here: a lane takes the class bits of its neighbour's last and first position
// out of the array of the lanes' masks, and the first and last lane of a wave make their one guarded load —, the packed sums added up
// as the wave and the block add them, the edges collected through a cursor that counts as the kernel's atomic one does, then sorted and
// paired as the entry point pairs them. Against a byte loop written the obvious way: per record the seven counters, and the runs of
// each class by walking the record. The whole tables must be equal. Built with AddressSanitizer by
// tests/test_fasta_stats_kernel_cpu.py: the text is exactly seqBytes long (and, every other call, starts where its allocation
// starts), so a read outside it ends the run. The texts are biased towards long runs and runs that end on a record's last byte; the
// program prints how many runs of each class it compared. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <tuple>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
namespace fa {
#include "../mbgc_amd/csrc/fasta_tiles.h"
#include "../mbgc_amd/csrc/fasta_stats.h"
}
using namespace fa;

typedef std::tuple<uint32_t, uint32_t, uint64_t, uint64_t> Run;      // rec, cls, start, len
struct Counts { uint64_t v[7]; bool operator==(const Counts &o) const { return !memcmp(v, o.v, sizeof v); } };   // a, c, g, t, n, other, lower

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937_64 rng(31);
    const char alpha[] = {'A', 'C', 'G', 'T', 'N', 'a', 'c', 'g', 't', 'n', 'R', 'Y', 'U', '>', '\0'};
    uint64_t compared[2] = {0, 0}, atRecordEnd = 0, longRuns = 0, multiTile = 0, unaligned = 0, capped = 0;
    for (int it = 0; it < iterations; it++) {
        const bool big = it % 4 == 0;
        const uint64_t seqBytes = big ? 2 * STATS_TILE + rng() % (2 * STATS_TILE) : 1 + rng() % 900;
        const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;   // the buffer's first byte: any alignment
        uint8_t *alloc = new uint8_t[seqBytes + shift], *seq = alloc + shift;
        // stretches of one letter or of one case, of lengths from 1 to several tiles, between single random bytes
        for (uint64_t i = 0; i < seqBytes;) {
            const unsigned kind = (unsigned) (rng() % 6);
            uint64_t n = kind == 0 ? 1 : (rng() % 8 == 0 ? 1 + rng() % (big ? 3 * STATS_TILE : 300) : 1 + rng() % 40);
            n = std::min(n, seqBytes - i);
            for (uint64_t k = 0; k < n; k++) {
                const uint8_t any = (uint8_t) alpha[rng() % sizeof alpha];
                seq[i + k] = kind <= 1 ? any : kind == 2 ? 'N' : kind == 3 ? 'n' : kind == 4 ? (uint8_t) (any | 0x20) : (uint8_t) (rng() % 2 ? 'N' : 'n');
            }
            i += n;
        }
        unaligned += ((uintptr_t) seq & 15) != 0;
        // records: anywhere, of any length — empty ones, ones of a byte, the whole buffer, neighbours, the same one twice, overlapping
        std::vector<ScanRec> recs;
        const int nrec = 1 + (int) (rng() % 9);
        for (int r = 0; r < nrec; r++) {
            const uint64_t lc[] = {0, 1, 15, 16, 17, seqBytes, rng() % 40, rng() % (seqBytes + 1), rng() % (seqBytes + 1)};
            uint64_t len = std::min(lc[rng() % 9], seqBytes), off = rng() % (seqBytes - len + 1);
            if (r && rng() % 3 == 0) { off = recs[r - 1].off + recs[r - 1].len; len = std::min(len, seqBytes - off); }     // right behind the one before
            if (r && rng() % 6 == 0) { off = recs[r - 1].off; len = recs[r - 1].len; }                                     // the same again
            if (rng() % 5 == 0) { off = seqBytes - len; }                                                                 // ends with the buffer
            recs.push_back(ScanRec{off, len});
        }
        const uint32_t want = it % 7 == 0 ? STATS_CLS_N : (it % 7 == 1 ? STATS_CLS_LOWER : STATS_CLS_N | STATS_CLS_LOWER);

        // ---- the obvious way
        std::vector<Counts> wantCounts;
        std::vector<Run> wantRuns;
        for (size_t r = 0; r < recs.size(); r++) {
            Counts c = {{0, 0, 0, 0, 0, 0, 0}};
            const uint8_t *t = seq + recs[r].off;
            for (uint64_t p = 0; p < recs[r].len; p++) {
                const uint8_t b = t[p];
                if (b == 'A' || b == 'a') c.v[0]++;
                else if (b == 'C' || b == 'c') c.v[1]++;
                else if (b == 'G' || b == 'g') c.v[2]++;
                else if (b == 'T' || b == 't' || b == 'U' || b == 'u') c.v[3]++;
                else if (b == 'N' || b == 'n') c.v[4]++;
                else c.v[5]++;
                if (b >= 'a' && b <= 'z') c.v[6]++;
            }
            wantCounts.push_back(c);
            for (uint32_t cls = 0; cls < 2; cls++) {
                if (!(want & (1u << cls))) continue;
                for (uint64_t p = 0; p < recs[r].len;) {
                    const auto in = [&](uint64_t q) { return cls == 0 ? (t[q] == 'N' || t[q] == 'n') : (t[q] >= 'a' && t[q] <= 'z'); };
                    if (!in(p)) { p++; continue; }
                    uint64_t e = p;
                    while (e < recs[r].len && in(e)) e++;
                    wantRuns.push_back(Run((uint32_t) r, cls, p, e - p));
                    atRecordEnd += e == recs[r].len;
                    longRuns += e - p > STATS_TILE;
                    p = e;
                }
            }
        }

        // ---- the kernel's way
        std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
        for (size_t r = 0; r < recs.size(); r++) tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, recs[r].len);
        uint64_t *tileStart = exact(tileStartV);
        ScanRec *recTab = exact(recs);
        std::vector<Counts> gotCounts(recs.size(), Counts{{0, 0, 0, 0, 0, 0, 0}});
        // the edge buffer: exactly edgeCap rows, now and then too few — the cursor then counts on, and the pass is made again
        uint64_t edgeCap = it % 5 == 0 ? 3 : 1 << 16, cursor = 0;
        StatsEdge *edges = nullptr;
        for (;;) {
            edges = new StatsEdge[edgeCap ? edgeCap : 1];
            cursor = 0;
            for (Counts &c : gotCounts) c = Counts{{0, 0, 0, 0, 0, 0, 0}};
            for (uint64_t tile = 0; tile < tileStartV.back(); tile++) {
                const ScanTile open = scan_tile(seq, recTab, tileStart, (uint32_t) recs.size(), tile);
                const uint32_t r = open.r;
                const ScanRec rec = open.rec;
                multiTile += tile != tileStart[r];
                const uintptr_t tileAddr = open.addr;
                StatsLane L[STATS_THREADS];
                for (uint32_t lane = 0; lane < STATS_THREADS; lane++) L[lane] = stats_lane_step(seq, seqBytes, rec, tileAddr, lane);
                uint64_t a = 0, b = 0;                                   // the wave's and the block's sums
                for (uint32_t lane = 0; lane < STATS_THREADS; lane++) { a += L[lane].sumA; b += L[lane].sumB; }
                for (uint32_t i = 0; i < 7; i++) gotCounts[r].v[i] += stats_counter(a, b, i);
                for (uint32_t lane = 0; lane < STATS_THREADS; lane++) {
                    const uint32_t wl = lane & 63;
                    const int64_t t0 = (int64_t) (tileAddr + 16u * lane) - (int64_t) ((uintptr_t) seq + rec.off);
                    const uint32_t prevLast = wl == 0 ? stats_class_at(seq, rec, t0 - 1) : stats_last_of(L[lane - 1].masks);
                    const uint32_t nextFirst = wl == 63 ? stats_class_at(seq, rec, t0 + STATS_PER) : stats_first_of(L[lane + 1].masks);
                    const StatsEdges E = stats_edges(L[lane].masks, prevLast, nextFirst, want);
                    const uint32_t cnt = stats_edge_count(E);
                    if (cnt) { stats_edges_write(E, t0, r, cursor, edgeCap, edges); cursor += cnt; }
                }
            }
            if (cursor <= edgeCap) break;
            capped++;
            delete[] edges;
            edgeCap = cursor;
        }
        std::vector<StatsEdge> e(edges, edges + cursor);
        std::sort(e.begin(), e.end(), [](const StatsEdge &x, const StatsEdge &y) { return std::make_tuple(x.rec, x.kind & 1, x.kind, x.pos) < std::make_tuple(y.rec, y.kind & 1, y.kind, y.pos); });
        std::vector<Run> gotRuns;
        bool paired = true;
        for (size_t at = 0; at < e.size() && paired;) {
            size_t ends = at, next;
            while (ends < e.size() && e[ends].rec == e[at].rec && e[ends].kind == e[at].kind) ends++;
            for (next = ends; next < e.size() && e[next].rec == e[at].rec && e[next].kind == (e[at].kind | 2u); next++) {}
            paired = !(e[at].kind & 2u) && next - ends == ends - at;
            for (size_t i = 0; paired && i < ends - at; i++) gotRuns.push_back(Run(e[at].rec, e[at].kind & 1u, e[at + i].pos, e[ends + i].pos - e[at + i].pos + 1));
            at = next;
        }
        std::sort(wantRuns.begin(), wantRuns.end());
        for (const Run &r : wantRuns) compared[std::get<1>(r)]++;
        const bool ok = paired && gotRuns == wantRuns && gotCounts == wantCounts;
        if (!ok) {
            printf("MISMATCH in call %d: %zu runs, expected %zu (paired: %d); counts equal: %d; %zu records, %llu bytes, classes %u\n", it, gotRuns.size(), wantRuns.size(), (int) paired,
                   (int) (gotCounts == wantCounts), recs.size(), (unsigned long long) seqBytes, want);
            std::vector<Run> onlyGot, onlyWant;
            std::set_difference(gotRuns.begin(), gotRuns.end(), wantRuns.begin(), wantRuns.end(), std::back_inserter(onlyGot));
            std::set_difference(wantRuns.begin(), wantRuns.end(), gotRuns.begin(), gotRuns.end(), std::back_inserter(onlyWant));
            for (size_t i = 0; i < onlyGot.size() && i < 5; i++)
                printf("  not expected: rec %u cls %u start %llu len %llu\n", std::get<0>(onlyGot[i]), std::get<1>(onlyGot[i]), (unsigned long long) std::get<2>(onlyGot[i]), (unsigned long long) std::get<3>(onlyGot[i]));
            for (size_t i = 0; i < onlyWant.size() && i < 5; i++)
                printf("  missing: rec %u (off %llu len %llu) cls %u start %llu len %llu\n", std::get<0>(onlyWant[i]), (unsigned long long) recs[std::get<0>(onlyWant[i])].off,
                       (unsigned long long) recs[std::get<0>(onlyWant[i])].len, std::get<1>(onlyWant[i]), (unsigned long long) std::get<2>(onlyWant[i]), (unsigned long long) std::get<3>(onlyWant[i]));
            for (size_t r = 0; r < recs.size(); r++)
                if (!(gotCounts[r] == wantCounts[r])) {
                    printf("  counts of rec %zu (off %llu len %llu):", r, (unsigned long long) recs[r].off, (unsigned long long) recs[r].len);
                    for (int i = 0; i < 7; i++) printf(" %llu/%llu", (unsigned long long) gotCounts[r].v[i], (unsigned long long) wantCounts[r].v[i]);
                    printf("\n");
                    break;
                }
        }
        delete[] alloc; delete[] tileStart; delete[] recTab; delete[] edges;
        if (!ok) return 1;
    }
    const uint64_t n = (uint64_t) iterations;
    if (compared[0] < 1000 || compared[1] < 1000 || atRecordEnd < n / 2 || longRuns < n / 40 || multiTile < n / 8 || unaligned < n / 4 || capped < n / 10) {
        printf("the inputs are too easy: %llu / %llu runs, %llu at a record's end, %llu longer than a tile, %llu tiles behind a record's first, %llu unaligned buffers, %llu small edge buffers\n",
               (unsigned long long) compared[0], (unsigned long long) compared[1], (unsigned long long) atRecordEnd, (unsigned long long) longRuns, (unsigned long long) multiTile,
               (unsigned long long) unaligned, (unsigned long long) capped);
        return 1;
    }
    printf("ok: %d calls, runs compared: class 0 %llu, class 1 %llu (%llu end on a record's last byte, %llu longer than a tile)\n", iterations, (unsigned long long) compared[0],
           (unsigned long long) compared[1], (unsigned long long) atRecordEnd, (unsigned long long) longRuns);
    return 0;
}
