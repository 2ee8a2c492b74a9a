// k_fa_format and the host's table builders (mbgc_amd/csrc/fasta_format.h) as plain C++: every lane step of every tile run one
// after the other on the CPU, against a formatter written the obvious way. Built with AddressSanitizer by
// tests/test_fasta_format_kernel_cpu.py: a read or a store outside the buffers ends the run. No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct uint4 { uint32_t x, y, z, w; };
static struct { uint32_t x; } threadIdx, blockIdx;
namespace fa {
constexpr int CHUNK = 4096, THREADS = 256, PER = CHUNK / THREADS;
#include "../mbgc_amd/csrc/fasta_format.h"
}
using namespace fa;

static std::string plain(const std::vector<uint8_t> &seq, const std::vector<uint8_t> &hdr, const std::vector<FmtIn> &R) {
    std::string o;
    for (const FmtIn &x : R) {
        o.push_back('>'); o.append((const char *) hdr.data() + x.headerOff, x.headerLen); o.push_back('\n');
        const uint64_t L = x.lineLen ? x.lineLen : std::max<uint64_t>(x.seqLen, 1);
        for (uint64_t i = 0; i < x.seqLen;) {
            const uint64_t n = std::min<uint64_t>(L, x.seqLen - i);
            o.append((const char *) seq.data() + x.seqOff + i, n); o.push_back('\n');
            i += n;
        }
    }
    return o;
}

int main(int argc, char **argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 1500;
    std::mt19937_64 rng(1);
    static const uint64_t lines[] = {0, 1, 7, 15, 16, 17, 60, 80, 4095, 4096, 4097, (1ull << 32) + 5, ~0ull};
    for (int it = 0; it < iterations; it++) {
        std::vector<uint8_t> seq, hdr;
        std::vector<FmtIn> R;
        const int nr = 1 + (int) (rng() % 12);
        for (int r = 0; r < nr; r++) {
            const uint64_t line = lines[rng() % 13], L = (line && line < 100000) ? line : 61;
            const uint64_t sc[] = {0, 1, L - 1, L, L + 1, 3 * L, 3 * L + 1, rng() % 200, rng() % 20000}, hc[] = {0, 1, 15, 16, 17, 5000, rng() % 40};
            const uint64_t sl = sc[rng() % 9], hl = hc[rng() % 7];
            R.push_back(FmtIn{seq.size(), sl, hdr.size(), hl, line});
            for (uint64_t i = 0; i < sl; i++) seq.push_back((uint8_t) "ACGT"[rng() % 4]);
            for (uint64_t i = 0; i < hl; i++) hdr.push_back((uint8_t) ('a' + rng() % 26));
        }
        const uint32_t mis = (uint32_t) (rng() % 16);
        std::vector<FmtRec> table;
        std::vector<uint64_t> textOff(R.size() + 1);
        const uint64_t total = fmt_build_table(R.data(), R.size(), table, textOff.data());
        const uint32_t ntiles = (uint32_t) ((total + mis + CHUNK - 1) / CHUNK);
        std::vector<uint32_t> owner;
        fmt_build_owner(table, R.size(), mis, ntiles, owner);
        std::vector<uint8_t> buf(total + mis + 80, 0xA5);
        uint8_t *text = buf.data();
        while (((uintptr_t) text & 15) != mis) text++;
        // exact-size copies: what lies behind the last contig and the last header is not the kernel's to read
        std::vector<uint8_t> seqExact(seq.begin(), seq.end()), hdrExact(hdr.begin(), hdr.end());
        seqExact.shrink_to_fit(); hdrExact.shrink_to_fit();
        for (uint32_t t = 0; t < ntiles; t++)
            for (uint32_t th = 0; th < (uint32_t) THREADS; th++) {
                blockIdx.x = t; threadIdx.x = th;
                k_fa_format(seqExact.data(), seqExact.size(), hdrExact.data(), table.data(), owner.data(), 0, ntiles, mis, total, text);
            }
        const std::string want = plain(seq, hdr, R);
        bool ok = want.size() == total && memcmp(want.data(), text, total) == 0;
        for (size_t k = 0; ok && k < R.size(); k++) ok = k == 0 ? textOff[0] == 0 : textOff[k] > textOff[k - 1];
        for (uint8_t *q = buf.data(); ok && q < text; q++) ok = *q == 0xA5;
        for (uint8_t *q = text + total; ok && q < buf.data() + buf.size(); q++) ok = *q == 0xA5;
        if (!ok) {
            printf("MISMATCH in batch %d: %llu bytes of text, %zu expected, buffer %u bytes behind a 16-byte boundary\n", it, (unsigned long long) total, want.size(), mis);
            for (const FmtIn &x : R) printf("  record: %llu bases, header of %llu, line length %llu\n", (unsigned long long) x.seqLen, (unsigned long long) x.headerLen, (unsigned long long) x.lineLen);
            return 1;
        }
    }
    printf("ok: %d batches\n", iterations);
    return 0;
}
