// The lane steps of k_fa_dups and k_fa_dups_verify (mbgc_amd/csrc/fasta_dups.h) as plain C++: every call cut into tiles as
// mbgc_fasta_dups_dev cuts it, every tile run lane by lane — the lane's eight residues times its own power, the wave's sum as the
// butterfly of shuffles it is on the device (arrays here), the four waves' sums, the tile's power as the first wave keeps it (by
// squaring when the block comes to a record, by the stride's power while it stays in it: the tiles are dealt to `grid` blocks), the
// terms added to the record's row, the row finished as the host finishes it. Against a byte loop written the obvious way: the forward
// fingerprint sum T[fold(s_j)] x^(len - 1 - j) and the reverse one sum T[comp(fold(s_j))] x^j modulo each prime, comp from a table
// written out here. Then every two records of equal length are compared by dups_verify_step, all lanes of all steps, forward and
// mirrored, against the byte loop's verdict. Built with AddressSanitizer by tests/test_fasta_dups_kernel_cpu.py: the text is exactly
// seqBytes long (and, every other call, starts where its allocation starts), so a read outside it ends the run. Copies, reverse
// complements and copies with one byte changed are planted; the program prints how many pairs it found equal on the reverse strand and
// how many it refuted. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
namespace fa {
#include "../mbgc_amd/csrc/fasta_tiles.h"
#include "../mbgc_amd/csrc/fasta_dups.h"
}
using namespace fa;

static uint8_t COMP[256];
static void make_comp() {
    for (int b = 0; b < 256; b++) COMP[b] = (uint8_t) b;
    const char *pairs[] = {"AT", "CG", "RY", "KM", "BV", "DH"};
    for (const char *p : pairs)
        for (int c = 0; c < 2; c++) {
            const uint8_t x = (uint8_t) p[c], y = (uint8_t) p[1 - c];
            COMP[x] = y; COMP[x | 0x20] = (uint8_t) (y | 0x20);
        }
}
static uint8_t fold_ref(uint8_t b, bool exact) { return !exact && b >= 'a' && b <= 'z' ? (uint8_t) (b - 32) : b; }

template <class T> static T *exact(const std::vector<T> &v) {       // a copy in an allocation of exactly that many elements
    T *p = new T[v.size() ? v.size() : 1];
    std::copy(v.begin(), v.end(), p);
    return p;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 200;
    make_comp();
    for (int b = 0; b < 256; b++)
        if (dups_comp((uint8_t) b) != COMP[b] || dups_comp(dups_comp((uint8_t) b)) != b) { printf("MISMATCH: comp(%d) = %d, the table says %d\n", b, dups_comp((uint8_t) b), COMP[b]); return 1; }
    const uint32_t P[4] = {dups_p(0), dups_p(1), dups_p(2), dups_p(3)}, X[4] = {dups_x(0), dups_x(1), dups_x(2), dups_x(3)};
    std::mt19937_64 rng(47);
    const uint8_t alpha[] = {'A', 'C', 'G', 'T', 'N', 'a', 'c', 'g', 't', 'R', 'Y', 'k', 'M', 'b', 'V', 'D', 'h', 'S', 'U', '>', 0, 0x80, 0xC1, 0xFF};
    uint64_t prints = 0, equalForward = 0, equalReverse = 0, refuted = 0, multiTile = 0, unaligned = 0;
    for (int it = 0; it < iterations; it++) {
        const bool big = it % 4 == 0, exactCase = it % 5 == 0;
        const uint32_t grid = it % 3 == 0 ? 1 : 1 + (uint32_t) (rng() % 5);
        // ---- the records' texts: fresh ones, copies, reverse complements, copies with one byte changed, case changed
        std::vector<std::vector<uint8_t>> texts;
        const int nrec = 2 + (int) (rng() % 9);
        for (int r = 0; r < nrec; r++) {
            const unsigned kind = r ? (unsigned) (rng() % 6) : 0;
            std::vector<uint8_t> t;
            if (kind <= 1) {
                const uint64_t lc[] = {0, 1, 15, 16, 17, 33, rng() % 300, big ? DUPS_TILE - 1 + rng() % 3 : rng() % 64, big ? 2 * DUPS_TILE + rng() % 40 : rng() % 700};
                t.resize(lc[rng() % 9]);
                for (uint8_t &b : t) b = alpha[rng() % (rng() % 4 ? 9 : sizeof alpha)];
            } else {
                t = texts[rng() % texts.size()];
                if (kind == 3 || kind == 5) { std::reverse(t.begin(), t.end()); for (uint8_t &b : t) b = COMP[b]; }
                if (kind >= 4 && !t.empty()) { const uint64_t at[] = {0, t.size() - 1, rng() % t.size()}; t[at[rng() % 3]] ^= (uint8_t) (1u << (rng() % 7)); }
                if (rng() % 4 == 0) for (uint8_t &b : t) if (rng() % 3 == 0 && ((b | 0x20) >= 'a' && (b | 0x20) <= 'z')) b ^= 0x20;
            }
            texts.push_back(t);
        }
        // ---- the buffer: the records at any offset, foreign bytes between them; exactly seqBytes long, at any alignment
        std::vector<uint8_t> buf;
        std::vector<ScanRec> recs;
        for (const std::vector<uint8_t> &t : texts) {
            for (uint64_t k = rng() % 18; k; k--) buf.push_back(alpha[rng() % sizeof alpha]);
            recs.push_back(ScanRec{buf.size(), t.size()});
            buf.insert(buf.end(), t.begin(), t.end());
        }
        if (it % 2) for (uint64_t k = rng() % 18; k; k--) buf.push_back('A');                    // (else the last record ends with the buffer)
        const uint64_t seqBytes = buf.size();
        const uint32_t shift = it % 2 ? (uint32_t) (rng() % 16) : 0;
        uint8_t *alloc = new uint8_t[seqBytes + shift + (seqBytes + shift ? 0 : 1)], *seq = alloc + shift;
        if (seqBytes) memcpy(seq, buf.data(), seqBytes);
        unaligned += ((uintptr_t) seq & 15) != 0;

        // ---- the kernel's way: the fingerprints
        std::vector<uint64_t> tileStartV(recs.size() + 1, 0);
        for (size_t r = 0; r < recs.size(); r++) tileStartV[r + 1] = tileStartV[r] + scan_tiles_of((uintptr_t) seq + recs[r].off, recs[r].len);
        uint64_t *tileStart = exact(tileStartV);
        ScanRec *recTab = exact(recs);
        std::vector<unsigned long long> rows(8 * recs.size(), 0);
        for (uint32_t block = 0; block < grid; block++) {
            uint32_t stride[8], pw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, powerOf = 0;
            bool powered = false;
            dups_pow8((uint64_t) DUPS_TILE * grid, stride);
            for (uint64_t tile = block; tile < tileStartV.back(); tile += grid) {
                const ScanTile open = scan_tile(seq, recTab, tileStart, (uint32_t) recs.size(), tile);
                const uint32_t r = open.r;
                const ScanRec rec = open.rec;
                multiTile += tile != tileStart[r];
                const uintptr_t first = (uintptr_t) seq + rec.off, tileAddr = open.addr;
                uint32_t v[DUPS_THREADS][8], lanePw[8];
                for (uint32_t lane = 0; lane < DUPS_THREADS; lane++) {
                    dups_lane_step(seq, seqBytes, rec, tileAddr, lane, exactCase, v[lane]);
                    dups_pow8(16ull * lane, lanePw);
                    dups_mul8(v[lane], lanePw);
                }
                for (uint32_t d = 32; d; d >>= 1) {                  // the butterfly: every lane adds its partner's value of before the step
                    uint32_t before[DUPS_THREADS][8];
                    memcpy(before, v, sizeof v);
                    for (uint32_t lane = 0; lane < DUPS_THREADS; lane++) dups_add8(v[lane], before[lane ^ d]);
                }
                if (powered && powerOf == r) dups_mul8(pw, stride); else dups_pow8(dups_tile_exp(first, tile - tileStart[r]), pw);
                powered = true; powerOf = r;
                for (uint32_t q = 0; q < 8; q++) {
                    uint64_t sum = 0;
                    for (uint32_t w = 0; w < DUPS_THREADS / 64; w++) sum += v[64 * w][q];
                    const uint32_t term = dups_tile_term(q, sum, pw);
                    if (term >= 0x80000000u) { printf("MISMATCH: a tile's term is not below 2^31\n"); return 1; }
                    rows[8 * r + q] += term;
                }
            }
        }
        // ---- the obvious way, and the two held together
        std::vector<DupsPrint> fw(recs.size()), rv(recs.size());
        for (size_t r = 0; r < recs.size(); r++) {
            dups_finish(&rows[8 * r], recs[r].len, fw[r], rv[r]);
            const std::vector<uint8_t> &t = texts[r];
            for (int i = 0; i < 4; i++) {
                uint64_t f = 0, b = 0;
                for (size_t j = 0; j < t.size(); j++) f = (f * X[i] + (uint64_t) fold_ref(t[j], exactCase) + 1) % P[i];                       // Horner: x^(len - 1 - j)
                for (size_t j = t.size(); j-- > 0;) b = (b * X[i] + (uint64_t) COMP[fold_ref(t[j], exactCase)] + 1) % P[i];                  // x^j
                if (f != fw[r].v[i] || b != rv[r].v[i]) {
                    printf("MISMATCH in call %d: record %zu (off %llu len %llu), prime %d: forward %u / %llu, reverse %u / %llu (grid %u)\n", it, r, (unsigned long long) recs[r].off,
                           (unsigned long long) recs[r].len, i, fw[r].v[i], (unsigned long long) f, rv[r].v[i], (unsigned long long) b, grid);
                    return 1;
                }
                prints += 2;
            }
        }
        // ---- the exactness step: every two records of equal length, both strands
        for (size_t a = 0; a < recs.size(); a++)
            for (size_t b = 0; b < recs.size(); b++) {
                if (a == b || recs[a].len != recs[b].len) continue;
                for (uint32_t strand = 0; strand < 2; strand++) {
                    const uint64_t len = recs[a].len;
                    bool want = false;
                    for (uint64_t i = 0; i < len; i++) {
                        const uint8_t x = fold_ref(texts[a][i], exactCase), y = strand ? COMP[fold_ref(texts[b][len - 1 - i], exactCase)] : fold_ref(texts[b][i], exactCase);
                        want |= x != y;
                    }
                    const uintptr_t first = (uintptr_t) seq + recs[a].off;
                    bool got = false;
                    for (uint64_t s = 0; s < scan_tiles_of(first, len); s++)
                        for (uint32_t lane = 0; lane < DUPS_THREADS; lane++)
                            got |= dups_verify_step(seq, recTab[a], recTab[b], strand, exactCase, (first & ~(uintptr_t) 15) + s * DUPS_TILE, lane);
                    if (got != want) { printf("MISMATCH in call %d: records %zu and %zu (len %llu), strand %u: differ %d, expected %d\n", it, a, b, (unsigned long long) len, strand, (int) got, (int) want); return 1; }
                    if (want) refuted++; else if (strand) equalReverse += len > 0; else equalForward += len > 0;
                    // equal bytes have equal fingerprints: forward with forward, forward with the other's reverse
                    if (!want && memcmp(&fw[a], strand ? &rv[b] : &fw[b], sizeof(DupsPrint))) { printf("MISMATCH in call %d: equal records %zu and %zu (strand %u) with different fingerprints\n", it, a, b, strand); return 1; }
                }
            }
        delete[] alloc; delete[] tileStart; delete[] recTab;
    }
    const uint64_t n = (uint64_t) iterations;
    if (equalForward < n / 2 || equalReverse < n / 2 || refuted < 5 * n || multiTile < n / 4 || unaligned < n / 4) {
        printf("the inputs are too easy: %llu / %llu equal pairs, %llu refuted, %llu tiles behind a record's first, %llu unaligned buffers\n", (unsigned long long) equalForward,
               (unsigned long long) equalReverse, (unsigned long long) refuted, (unsigned long long) multiTile, (unsigned long long) unaligned);
        return 1;
    }
    printf("ok: %d calls, %llu residues equal the byte loop's; pairs compared: %llu equal forward, %llu equal on the reverse strand, %llu refuted\n", iterations,
           (unsigned long long) prints, (unsigned long long) equalForward, (unsigned long long) equalReverse, (unsigned long long) refuted);
    return 0;
}
