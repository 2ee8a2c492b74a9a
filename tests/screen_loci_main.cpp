// The keys and the chaining of `mbgc-hip m` (mbgc_amd/host/mbgc_screen_loci.h) as a stand-alone program for
// tests/test_screen_loci_cpu.py: cases on stdin — a line `k maxGap minHits flank queries hits`, then the queries, one per line, then
// the hits `rec pos key`, sorted by (rec, pos) —, per case on stdout a line `keys` with the key list in hex, a line `own` with the
// queries' key counts, a line `query rec start end hits distinct region` per locus (0-based, inclusive; region: the line of
// --regions-out for a record named r<rec>), and a line `end <n>`. Built with AddressSanitizer and UBSan. No GPU.
#include <cinttypes>
#include <cstdio>
#include "../mbgc_amd/host/mbgc_screen_loci.h"

int main() {
    uint32_t k;
    uint64_t maxGap, minHits, flank, nq, nh;
    while (scanf("%" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &k, &maxGap, &minHits, &flank, &nq, &nh) == 6) {
        std::vector<std::string> queries(nq);
        for (std::string &q : queries) {
            static char buf[1 << 20];
            if (scanf("%1048575s", buf) != 1) return 2;
            q = buf;
        }
        std::vector<mbgc_screen::Hit> hits(nh);
        for (mbgc_screen::Hit &h : hits)
            if (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32, &h.rec, &h.pos, &h.key) != 3) return 2;
        const mbgc_screen::KeySet S = mbgc_screen::buildKeys(queries, k);
        for (const mbgc_screen::Hit &h : hits) if (h.key >= S.keys.size()) return 3;
        printf("keys");
        for (const uint64_t key : S.keys) printf(" %" PRIx64, key);
        printf("\nown");
        for (const uint64_t n : S.queryKeys) printf(" %" PRIu64, n);
        printf("\n");
        const std::vector<mbgc_screen::Locus> out = mbgc_screen::chainLoci(hits, S, k, maxGap, minHits);
        for (const mbgc_screen::Locus &l : out)
            printf("%" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %s", l.query, l.rec, l.start, l.end, l.hits, l.distinct,
                   mbgc_screen::regionLine("r" + std::to_string(l.rec), l.start, l.end, flank).c_str());
        printf("end %zu\n", out.size());
    }
    return 0;
}
