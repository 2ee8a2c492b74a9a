// The pairing of `mbgc-hip f --primers` (mbgc_amd/host/mbgc_find_amplicons.h) as a stand-alone program for
// tests/test_find_amplicons_cpu.py: cases on stdin — a line `min max n`, then n hits `rec pos len pair role mismatches` —, per case the
// products on stdout, one `rec pair start end strand leftMismatches rightMismatches` per line, and a line `end <n>`. Built with
// AddressSanitizer and UBSan. No GPU.
#include <cinttypes>
#include <cstdio>
#include "../mbgc_amd/host/mbgc_find_amplicons.h"

int main() {
    uint64_t minLen, maxLen, n;
    while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &minLen, &maxLen, &n) == 3) {
        std::vector<mbgc_amplicons::Hit> hits(n);
        for (mbgc_amplicons::Hit &h : hits)
            if (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &h.rec, &h.pos, &h.len, &h.pair, &h.role, &h.mismatches) != 6) return 2;
        const std::vector<mbgc_amplicons::Product> out = mbgc_amplicons::pairHits(hits, minLen, maxLen);
        for (const mbgc_amplicons::Product &p : out)
            printf("%" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %c %" PRIu32 " %" PRIu32 "\n", p.rec, p.pair, p.start, p.end, p.strand, p.leftMismatches, p.rightMismatches);
        printf("end %zu\n", out.size());
    }
    return 0;
}
