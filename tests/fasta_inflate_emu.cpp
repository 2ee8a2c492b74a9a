// The decoder of k_fa_inflate (mbgc_amd/csrc/fasta_inflate.h holds no HIP call) as plain C++: the 64 lanes of a wave run one after the
// other wherever the kernel lets them work side by side, everything else is the very text the kernel compiles — the bit reader, the
// table build, the symbol decode, every bounds and validity decision, the ring and the CRC fold. Reads the corpus that
// tests/_inflate_cases.py writes and holds every case to its expected status, length and bytes, at four alignments of the output.
// Built with AddressSanitizer and UBSan by tests/test_inflate_kernel_cpu.py; the input ends where its allocation ends and so does the
// output, so a read or a write past either end ends the run, and the bytes in front of the output are checked. No GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#define __device__
#define __forceinline__ inline
struct uint4 { uint32_t x, y, z, w; };
#define INF_CONST static
#define INF_LANES_DO(lane) for (uint32_t lane = 0; lane < INF_WAVE; lane++)
#define INF_LANE0 true
#define INF_SYNC() ((void) 0)
#define INF_UNI(x) ((uint32_t) (x))
namespace fa {
#include "../mbgc_amd/csrc/fasta_inflate.h"
}
using namespace fa;

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s corpus\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 2;
    InfShared *S = new InfShared();
    int bad = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        struct __attribute__((packed)) { uint32_t nameLen; uint64_t inLen, outCap; int32_t status; uint64_t wantLen; } h;
        if (fread(&h, sizeof h, 1, f) != 1) return 2;
        std::string name(h.nameLen, '\0');
        std::vector<uint8_t> gz(h.inLen), want(h.wantLen);
        if ((h.nameLen && fread(&name[0], h.nameLen, 1, f) != 1) || (h.inLen && fread(gz.data(), h.inLen, 1, f) != 1) || (h.wantLen && fread(want.data(), h.wantLen, 1, f) != 1)) return 2;
        for (uint32_t shift : {0u, 1u, 7u, 15u}) {
            // the input's last byte is its allocation's last byte; so is the output's; `shift` bytes of a pattern stand in front of both
            uint8_t *inAlloc = new uint8_t[shift + h.inLen + (shift + h.inLen ? 0 : 1)], *outAlloc = new uint8_t[shift + h.outCap + (shift + h.outCap ? 0 : 1)];
            memset(inAlloc, 0x5a, shift);
            if (h.inLen) memcpy(inAlloc + shift, gz.data(), h.inLen);
            memset(outAlloc, 0xa5, shift + h.outCap);
            memset(S, 0xcc, sizeof *S);
            Inf I(*S, inAlloc + shift, h.inLen, outAlloc + shift, h.outCap);
            const InfResult r = I.run();
            bool ok = h.status < 0 ? r.status != INF_OK : r.status == h.status;
            if (ok && r.status == INF_OK)
                ok = r.outLen == h.wantLen && r.inUsed == h.inLen && r.members >= 1 && (h.wantLen == 0 || memcmp(outAlloc + shift, want.data(), h.wantLen) == 0);
            for (uint32_t k = 0; k < shift; k++) ok = ok && outAlloc[k] == 0xa5;
            if (r.status == INF_OK) for (uint64_t k = r.outLen; k < h.outCap; k++) ok = ok && outAlloc[shift + k] == 0xa5;   // nothing behind the text either
            if (!ok) {
                printf("FAILED %s (output shifted by %u): status %d, expected %d; %llu bytes, expected %llu; %llu of %llu input bytes; %u members\n", name.c_str(), shift, r.status,
                       h.status, (unsigned long long) r.outLen, (unsigned long long) h.wantLen, (unsigned long long) r.inUsed, (unsigned long long) h.inLen, r.members);
                bad++;
            }
            delete[] inAlloc; delete[] outAlloc;
        }
    }
    fclose(f);
    delete S;
    if (bad) return 1;
    printf("ok: %u cases\n", ncases);
    return 0;
}
