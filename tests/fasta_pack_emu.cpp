// The lane step of k_fa_pack and the host's table builders (mbgc_amd/csrc/fasta_pack.h) as plain C++: every lane step of every tile
// run one after the other on the CPU, against a byte loop written the obvious way. Built with AddressSanitizer by
// tests/test_fasta_pack_kernel_cpu.py; both buffers are allocated exactly as long as declared, so a read or a write past either end
// ends the run, and the destination's bytes behind the total must stay as they were. No GPU.
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
inline uint8_t up(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t) (c - 32) : c; }   // (fasta_input.hip's, which the header takes from its includer)
#include "../mbgc_amd/csrc/fasta_pack.h"
}
using namespace fa;

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 1500;
    std::mt19937_64 rng(11);
    for (int it = 0; it < iterations; it++) {
        const int np = (int) (rng() % 5 == 0 ? rng() % 400 : rng() % 12);
        const uint64_t lc[] = {0, 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, rng() % 41, rng() % 300, rng() % 20000};
        std::vector<PackIn> in;
        uint64_t srcBytes = rng() % 3 ? rng() % 40 : 0;                                          // bytes in front of the first piece
        for (int k = 0; k < np; k++) {
            const uint64_t len = np > 12 ? rng() % 41 : lc[rng() % 19];
            in.push_back(PackIn{srcBytes, len});
            srcBytes += len + (rng() % 2 ? rng() % 20 : 0);
        }
        if (np && rng() % 2) srcBytes = in.back().srcOff + in.back().len;                        // the last piece ends with the source
        if (np > 2 && rng() % 4 == 0) std::swap(in[0], in[np - 1]);                              // (the pieces need not ascend in the source)
        uint64_t total = 0;
        for (const PackIn &x : in) total += x.len;
        const uint64_t slack = rng() % 3 ? 0 : rng() % 40, lead = rng() % 16;                    // dst at every alignment; capacity = the total, or more
        const bool fold = rng() % 2;
        // exactly as long as declared: operator new[] of that many bytes, so that ASan's red zone starts at the end
        uint8_t *src = new uint8_t[srcBytes ? srcBytes : 1], *dstAll = new uint8_t[lead + total + slack + 1];
        uint8_t *dst = dstAll + lead;
        for (uint64_t i = 0; i < srcBytes; i++) src[i] = (uint8_t) (rng() % 8 ? "ACGTacgtNn"[rng() % 10] : rng());
        memset(dstAll, 0xEE, lead + total + slack + 1);
        std::vector<uint8_t> want;
        std::vector<uint64_t> wantOff;
        for (const PackIn &x : in) {
            wantOff.push_back(want.size());
            for (uint64_t o = 0; o < x.len; o++) { const uint8_t c = src[x.srcOff + o]; want.push_back(fold && c >= 'a' && c <= 'z' ? (uint8_t) (c - 32) : c); }
        }
        wantOff.push_back(want.size());
        std::vector<PackPiece> table;
        std::vector<uint64_t> dstOff(in.size() + 1);
        const uint64_t got = pack_build_table(in.data(), in.size(), table, dstOff.data());
        bool ok = got == total && dstOff == wantOff;
        if (total) {
            const uint32_t mis = (uint32_t) ((uintptr_t) dst & (PER - 1));
            const uint32_t ntiles = (uint32_t) ((total + mis + CHUNK - 1) / CHUNK);
            std::vector<uint32_t> owner;
            pack_build_owner(table, mis, ntiles, owner);
            for (uint32_t t = 0; t < ntiles; t++)
                for (uint32_t lane = 0; lane < (uint32_t) THREADS; lane++) pack_lane_step(src, table.data(), owner.data(), t, lane, mis, total, fold, dst);
        }
        ok = ok && (total == 0 || memcmp(dst, want.data(), total) == 0);
        for (uint64_t i = 0; i < lead; i++) ok = ok && dstAll[i] == 0xEE;
        for (uint64_t i = lead + total; i < lead + total + slack + 1; i++) ok = ok && dstAll[i] == 0xEE;
        delete[] src; delete[] dstAll;
        if (!ok) {
            printf("MISMATCH in call %d: %zu pieces, %llu bytes, fold %d, dst %llu bytes behind a boundary\n", it, in.size(), (unsigned long long) total, (int) fold,
                   (unsigned long long) lead);
            for (size_t k = 0; k < in.size() && k < 40; k++) printf("  piece: src %llu, %llu bytes\n", (unsigned long long) in[k].srcOff, (unsigned long long) in[k].len);
            return 1;
        }
    }
    printf("ok: %d calls\n", iterations);
    return 0;
}
