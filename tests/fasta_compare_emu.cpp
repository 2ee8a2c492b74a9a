// The lane step of k_fa_compare and the host's table builders (mbgc_amd/csrc/fasta_compare.h) as plain C++: every lane step of every
// tile run one after the other on the CPU, the per-slot minimum taken the way the kernel's atomicMin takes it, against a byte loop
// written the obvious way. Built with AddressSanitizer by tests/test_fasta_compare_kernel_cpu.py; both buffers are allocated exactly
// as long as declared, so a read past either end ends the run. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
namespace fa {
constexpr int CHUNK = 4096, THREADS = 256, PER = CHUNK / THREADS;
#include "../mbgc_amd/csrc/fasta_compare.h"
}
using namespace fa;

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 1500;
    std::mt19937_64 rng(7);
    for (int it = 0; it < iterations; it++) {
        const int np = 1 + (int) (rng() % 10);
        const uint32_t nslots = 1 + (uint32_t) (rng() % 4);
        const uint64_t lc[] = {0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 3 * 4096 + 5, rng() % 300, rng() % 20000};
        std::vector<CmpIn> in;
        uint64_t aBytes = rng() % 3 ? rng() % 40 : 0, bBytes = rng() % 3 ? rng() % 40 : 0;       // bytes in front of the first piece
        for (int k = 0; k < np; k++) {
            const uint64_t len = lc[rng() % 14];
            in.push_back(CmpIn{aBytes, bBytes, len, (uint32_t) (rng() % nslots)});
            aBytes += len + (rng() % 2 ? rng() % 20 : 0);
            bBytes += len + (rng() % 2 ? rng() % 20 : 0);
        }
        if (rng() % 2) { aBytes = in.back().aOff + in.back().len; bBytes = in.back().bOff + in.back().len; }   // the last piece ends with the buffers
        // exactly as long as declared: operator new[] of that many bytes, so that ASan's red zone starts at the end
        uint8_t *a = new uint8_t[aBytes ? aBytes : 1], *b = new uint8_t[bBytes ? bBytes : 1];
        for (uint64_t i = 0; i < aBytes; i++) a[i] = (uint8_t) "ACGT"[rng() % 4];
        for (uint64_t i = 0; i < bBytes; i++) b[i] = (uint8_t) "acgt"[rng() % 4];                 // (outside the pieces everything differs)
        for (const CmpIn &x : in) memcpy(b + x.bOff, a + x.aOff, x.len);
        const int ndiff = (int) (rng() % 4);
        for (int d = 0; d < ndiff; d++) {
            const CmpIn &x = in[rng() % in.size()];
            if (!x.len) continue;
            const uint64_t at[] = {0, x.len - 1, x.len / 2, 15 % x.len, 16 % x.len, rng() % x.len};
            b[x.bOff + at[rng() % 6]] ^= 0x20;
        }
        std::vector<uint64_t> want(nslots, CMP_NONE), got(nslots, CMP_NONE);
        for (const CmpIn &x : in)
            for (uint64_t o = 0; o < x.len; o++)
                if (a[x.aOff + o] != b[x.bOff + o]) { want[x.slot] = std::min(want[x.slot], o); break; }
        std::vector<CmpPiece> table;
        const uint64_t total = cmp_build_table(in.data(), in.size(), (uint64_t) (uintptr_t) a, table);
        const uint32_t ntiles = (uint32_t) ((total + CHUNK - 1) / CHUNK);
        std::vector<uint32_t> owner;
        cmp_build_owner(table, ntiles, owner);
        uint64_t covered = 0;
        for (uint32_t t = 0; t < ntiles; t++)
            for (uint32_t lane = 0; lane < (uint32_t) THREADS; lane++) {
                uint32_t piece = ~0u;
                const uint64_t d = cmp_lane_step(a, b, table.data(), owner.data(), t, lane, total, &piece);
                if (piece != ~0u) covered++;
                if (d != CMP_NONE) got[table[piece].slot] = std::min(got[table[piece].slot], d);
            }
        bool ok = want == got && covered == total / PER;
        delete[] a; delete[] b;
        if (!ok) {
            printf("MISMATCH in call %d: %zu pieces, %u slots\n", it, in.size(), nslots);
            for (const CmpIn &x : in) printf("  piece: a %llu, b %llu, %llu bytes, slot %u\n", (unsigned long long) x.aOff, (unsigned long long) x.bOff, (unsigned long long) x.len, x.slot);
            for (uint32_t s = 0; s < nslots; s++) printf("  slot %u: %lld, expected %lld\n", s, (long long) got[s], (long long) want[s]);
            return 1;
        }
    }
    printf("ok: %d calls\n", iterations);
    return 0;
}
