// The lane steps of k_fa_crc and the host's table builder (mbgc_amd/csrc/fasta_crc.h) as plain C++: every row of the table run wave by
// wave, lane by lane, the groups' values folded as the kernel's shuffles fold them (XOR inside a group, the product of the lanes'
// factors for a cut range's piece, XOR into the range's word), with both table lookups, against a bitwise CRC loop written the
// obvious way. Built with AddressSanitizer by tests/test_fasta_crc_kernel_cpu.py; every range stands in an allocation of its own
// whose bytes in front of the range (they set its alignment) are poisoned and which ends with the range, so a read outside a range
// ends the run. No GPU.
#include <sanitizer/asan_interface.h>
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
struct uint4 { uint32_t x, y, z, w; };
namespace fa {
#include "../mbgc_amd/csrc/fasta_crc.h"
}
using namespace fa;

static uint32_t plain_crc(const uint8_t *p, uint64_t n) {
    uint32_t r = 0xffffffffu;
    for (uint64_t i = 0; i < n; i++) {
        r ^= p[i];
        for (int k = 0; k < 8; k++) r = r & 1u ? (r >> 1) ^ 0xEDB88320u : r >> 1;
    }
    return ~r;
}

template <uint32_t LOOKUP> static void fill(CrcShared<LOOKUP> &S, const CrcConsts &K) {
    memset(&S, 0xee, sizeof S);
    for (uint32_t tid = 0; tid < CRC_THREADS; tid++) crc_fill_shared(S, &K, tid, CRC_THREADS);
}

// what one launch computes: the ranges' words before the final XOR
template <uint32_t LOOKUP>
static void run_launch(const std::vector<uint8_t *> &base, const std::vector<CrcIn> &recs, const std::vector<CrcRow> &rows, const std::vector<uint64_t> &behind,
                       const CrcPlan &plan, uint64_t nwaves, const CrcShared<LOOKUP> &S, std::vector<uint32_t> &out) {
    out.assign(recs.size(), 0);
    for (uint64_t w = 0; w < nwaves; w++) {
        uint32_t c = 0;
        for (uint32_t k = 1; k < CRC_CLASSES; k++) if (w >= plan.wave0[k]) c = k;
        const uint32_t G = crc_class_lanes(c), rowEnd = plan.row0[c + 1];
        uint32_t v[CRC_LANES];
        CrcRow R[CRC_LANES];
        for (uint32_t lane = 0; lane < CRC_LANES; lane++) {
            const uint32_t row = plan.row0[c] + (uint32_t) (w - plan.wave0[c]) * (CRC_LANES / G) + lane / G;
            v[lane] = 0; R[lane] = CrcRow{0, 0, 0};
            if (row >= rowEnd) continue;
            R[lane] = rows[row];
            const uint32_t k = R[lane].rec & ~CRC_FIRST;
            // the range's own allocation stands where the caller's buffer would hold it: seq + recs[k].off is its first byte
            const uint8_t *seq = (const uint8_t *) ((uintptr_t) base[k] - (uintptr_t) recs[k].off);
            v[lane] = crc_lane_step<LOOKUP>(seq, R[lane], G, lane, S);
        }
        for (uint32_t g = 0; g < CRC_LANES; g += G) {
            const uint32_t row = plan.row0[c] + (uint32_t) (w - plan.wave0[c]) * (CRC_LANES / G) + g / G;
            if (row >= rowEnd) continue;
            uint32_t x = 0;
            for (uint32_t s = 0; s < G; s++) x ^= v[g + s];
            const uint32_t k = R[g].rec & ~CRC_FIRST;
            if (c + 1 < CRC_CLASSES) { out[k] = x; continue; }
            const uint64_t b = behind[row - plan.row0[c]];
            if (b) {
                uint32_t f = 0x80000000u;
                for (uint32_t lane = 0; lane < CRC_LANES; lane++) f = crc_mulmod(f, crc_pow_lane(b, lane, S));
                x = crc_mulmod(x, f);
            }
            out[k] ^= x;
        }
    }
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937_64 rng(17);
    CrcConsts K;
    crc_build_consts(K);
    static CrcShared<CRC_LOOKUP_NIBBLE> SN;
    static CrcShared<CRC_LOOKUP_BYTE> SB;
    fill(SN, K); fill(SB, K);
    uint64_t cut = 0, tiny = 0;
    for (int it = 0; it < iterations; it++) {
        // lengths around every class's threshold and the piece's, 0, and random ones of every class
        std::vector<uint64_t> lc = {0, 0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769,
                                    rng() % 41, rng() % 41, rng() % 300, rng() % 300, rng() % 2000, rng() % 6000, rng() % 20000, 49152 + rng() % 3, rng() % 70000};
        const int nrec = 1 + (int) (rng() % (it % 9 == 0 ? 300 : 20));
        const unsigned content = (unsigned) (it % 4);                      // random, all 0x00, all 0xff, four letters
        std::vector<CrcIn> recs;
        std::vector<uint8_t *> alloc, base;
        std::vector<uint32_t> want;
        uint64_t off = rng() % 100;
        for (int r = 0; r < nrec; r++) {
            const uint64_t len = lc[rng() % lc.size()], mis = rng() % 16;
            uint8_t *a = new uint8_t[mis + len ? mis + len : 1];            // 16-byte aligned: the range starts `mis` bytes behind a boundary
            for (uint64_t i = 0; i < len; i++)
                a[mis + i] = content == 0 ? (uint8_t) rng() : content == 1 ? 0 : content == 2 ? 0xff : "ACGT"[rng() & 3];
            if (mis) ASAN_POISON_MEMORY_REGION(a, mis);
            alloc.push_back(a); base.push_back(a + mis);
            // the offset the caller would name: congruent to the address mod 16, as in a buffer that starts on a boundary
            off = (off + 16) / 16 * 16 + mis;
            recs.push_back(CrcIn{off, len});
            off += len;
            want.push_back(len ? plain_crc(a + mis, len) : 0);
            if (len > CRC_PIECE) cut++;
            if (len <= CRC_SHARE) tiny++;
        }
        std::vector<CrcRow> rows;
        std::vector<uint64_t> behind;
        CrcPlan plan;
        const uint64_t nwaves = crc_build_table(recs.data(), recs.size(), rows, behind, plan);
        bool ok = true;
        for (int lookup = 0; lookup < 2 && ok; lookup++) {
            std::vector<uint32_t> out;
            if (lookup) run_launch(base, recs, rows, behind, plan, nwaves, SN, out);
            else run_launch(base, recs, rows, behind, plan, nwaves, SB, out);
            for (int r = 0; r < nrec && ok; r++) {
                const uint32_t got = recs[r].len ? ~out[r] : 0u;
                if (got != want[r]) {
                    printf("MISMATCH in call %d, lookup %d, range %d (%llu bytes, content %u): got %08x, expected %08x\n", it, lookup, r,
                           (unsigned long long) recs[r].len, content, got, want[r]);
                    ok = false;
                }
            }
        }
        // zlib's crc32_combine from the same arithmetic: the CRC of a range from those of its two halves
        for (int r = 0; r < nrec && ok; r++) {
            const uint64_t len = recs[r].len, a = len ? rng() % (len + 1) : 0;
            const uint32_t ca = a ? plain_crc(base[r], a) : 0, cb = len - a ? plain_crc(base[r] + a, len - a) : 0;
            const uint32_t got = crc_mulmod(crc_xpow8(len - a), ca) ^ cb;
            if (got != want[r]) { printf("COMBINE MISMATCH in call %d, range %d: %llu + %llu bytes\n", it, r, (unsigned long long) a, (unsigned long long) (len - a)); ok = false; }
        }
        for (size_t r = 0; r < alloc.size(); r++) {
            if (base[r] != alloc[r]) ASAN_UNPOISON_MEMORY_REGION(alloc[r], base[r] - alloc[r]);
            delete[] alloc[r];
        }
        if (!ok) return 1;
    }
    if (cut < (uint64_t) iterations || tiny < (uint64_t) iterations) { printf("the inputs are too easy: %llu cut ranges, %llu tiny ones\n", (unsigned long long) cut, (unsigned long long) tiny); return 1; }
    printf("ok: %d calls\n", iterations);
    return 0;
}
