/* The referee of the mutant corpus held in bounds: orc_decode_contig_bounded (oracle/decode_oracle.c) over every case
 * tests/_decmut.py writes, the rejected ones included. Built with AddressSanitizer and UBSan by tests/test_decode_mutants_cpu.py.
 * The reference buffer, the six streams and the destination are allocations of exactly their declared sizes, so a read or a
 * write past any of them ends the run; verdict, destLen, unmatchedChars and the sum of the bytes must be the corpus's. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oracle.h"

static int rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s corpus\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t nrows = 0, psize = 0;
    if (!rd(f, &nrows, 4) || !rd(f, &psize, 4) || psize != sizeof(orc_emit_params)) { fprintf(stderr, "corpus header\n"); return 2; }
    unsigned long long total = 0, failed = 0;
    for (uint32_t r = 0; r < nrows; r++) {
        orc_emit_params p;
        uint64_t refBytes = 0, lock = 0;
        uint32_t ncases = 0;
        if (!rd(f, &p, sizeof p) || !rd(f, &refBytes, 8) || !rd(f, &lock, 8) || !rd(f, &ncases, 4)) return 2;
        uint8_t *ref = malloc(refBytes);
        if (!ref || !rd(f, ref, refBytes)) return 2;
        for (uint32_t c = 0; c < ncases; c++, total++) {
            uint32_t accepted = 0;
            int64_t unmatched = 0;
            uint64_t destLen = 0, sum = 0, destCap = 0, sizes[ORC_NSTREAMS];
            if (!rd(f, &accepted, 4) || !rd(f, &unmatched, 8) || !rd(f, &destLen, 8) || !rd(f, &sum, 8) || !rd(f, &destCap, 8) || !rd(f, sizes, sizeof sizes)) return 2;
            uint8_t *s[ORC_NSTREAMS];
            const uint8_t *cs[ORC_NSTREAMS];
            for (int i = 0; i < ORC_NSTREAMS; i++) {
                s[i] = sizes[i] ? malloc(sizes[i]) : NULL;
                if (sizes[i] && (!s[i] || !rd(f, s[i], sizes[i]))) return 2;
                cs[i] = s[i];
            }
            uint8_t *dest = malloc(destCap ? destCap : 1);
            uint64_t got = 0;
            orc_decode_info info;
            memset(&info, 0, sizeof info);
            const int64_t un = orc_decode_contig_bounded(ref, refBytes, &p, cs, sizes, lock, dest, destCap, &got, &info);
            int ok = un >= 0;
            for (int i = 1; ok && i < ORC_NSTREAMS; i++) ok = info.cur[i] == sizes[i];
            int good = ok == (accepted != 0) && got <= destCap;
            if (good && ok) {
                uint64_t h = 0;
                for (uint64_t k = 0; k < got; k++) h += (uint64_t) dest[k] * (k % 65521 + 1);
                good = un == unmatched && got == destLen && h == sum;
            }
            if (!good) {
                printf("FAILED row %u case %u: verdict %d (%lld), expected %u (%lld); %llu bytes, expected %llu\n", r, c, ok, (long long) un, accepted,
                       (long long) unmatched, (unsigned long long) got, (unsigned long long) destLen);
                failed++;
            }
            free(dest);
            for (int i = 0; i < ORC_NSTREAMS; i++) free(s[i]);
        }
        free(ref);
    }
    fclose(f);
    if (failed) return 1;
    printf("ok: %llu cases\n", total);
    return 0;
}
