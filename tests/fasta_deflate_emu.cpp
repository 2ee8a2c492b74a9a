// The encoder of k_fa_deflate and the pack step of k_fa_deflate_pack (mbgc_amd/csrc/fasta_deflate.h holds no HIP call) as plain C++:
// the 64 lanes of a wave run one after the other wherever the kernels let them work side by side, everything else is the very text
// the kernels compile. Reads the corpus that tests/_deflate_cases.py writes; every call's slots, chunk tables and output buffer are
// allocated exactly as long as declared (AddressSanitizer ends the run at a byte past any of them; built by
// tests/test_deflate_kernel_cpu.py). Every gzip file is inflated with zlib, all members: the text must come back byte for byte, the
// trailer's CRC-32 and ISIZE must be those of the results, the size must keep mbgc_fasta_deflate_bound. code_lengths() is called on
// its own: Kraft sum exactly 1 and no length above the limit over Fibonacci, random, single-entry and all-zero histograms.
// Prints "name job inLen outLen chunks storedChunks" per job and, given a second argument, writes the gzip bytes there. No GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>
#define __device__
#define __forceinline__ inline
struct uint4 { uint32_t x, y, z, w; };
static uint32_t def_exscan_cpu(uint32_t *a) { uint32_t sum = 0; for (int i = 0; i < 64; i++) { const uint32_t t = a[i]; a[i] = sum; sum += t; } return sum; }
#define INF_CONST static
#define INF_LANES_DO(lane) for (uint32_t lane = 0; lane < 64; lane++)
#define INF_LANE0 true
#define INF_SYNC() ((void) 0)
#define INF_UNI(x) ((uint32_t) (x))
#define DEF_ATOMIC_ADD(p, v) (*(p) += (v))
#define DEF_ATOMIC_OR(p, v) (*(p) |= (v))
#define DEF_ATOMIC_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#define DEF_EXSCAN(arr) def_exscan_cpu(arr)
namespace fa {
#include "../mbgc_amd/csrc/fasta_deflate.h"
}
using namespace fa;

static uint64_t deflate_bound(uint64_t n) { return 18 + (n ? (n + DEF_CHUNK - 1) / DEF_CHUNK : 1) * 10 + n; }

// all members of gz -> text; false: zlib refuses it
static bool inflate_all(const uint8_t *gz, size_t n, std::vector<uint8_t> &text, unsigned &members) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 31) != Z_OK) return false;
    z.next_in = (Bytef *) gz; z.avail_in = (uInt) n;
    std::vector<uint8_t> buf(1 << 16);
    members = 0;
    bool ok = true;
    for (;;) {
        z.next_out = buf.data(); z.avail_out = (uInt) buf.size();
        const int r = inflate(&z, Z_NO_FLUSH);
        text.insert(text.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
        if (r == Z_STREAM_END) {
            members++;
            if (!z.avail_in) break;
            if (inflateReset(&z) != Z_OK) { ok = false; break; }
        } else if (r != Z_OK) { ok = false; break; }
    }
    inflateEnd(&z);
    return ok;
}

static int check_lengths(DefShared *S, const std::vector<uint32_t> &hist, uint32_t limit, const char *what) {
    Def D(*S, nullptr, 0, true, nullptr);
    std::vector<uint8_t> lens(hist.size(), 0xee);
    D.code_lengths(hist.data(), (uint32_t) hist.size(), limit, lens.data());
    uint64_t kraft = 0;
    uint32_t coded = 0;
    for (size_t s = 0; s < hist.size(); s++) {
        if (lens[s] > limit || (hist[s] && !lens[s])) { printf("FAILED lengths %s: symbol %zu of count %u has length %u (limit %u)\n", what, s, hist[s], lens[s], limit); return 1; }
        if (lens[s]) { kraft += (uint64_t) 1 << (limit - lens[s]); coded++; }
    }
    if (kraft != (uint64_t) 1 << limit || coded < 2) { printf("FAILED lengths %s: Kraft sum %llu / %llu over %u symbols\n", what, (unsigned long long) kraft, 1ull << limit, coded); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s corpus [gzip bytes out]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    FILE *o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !o) { perror(argv[2]); return 2; }
    DefShared *S = new DefShared();
    int bad = 0;

    // ---- the code-length function on its own
    {
        std::vector<uint32_t> fib = {1, 1};
        while (fib.size() < 30) fib.push_back(fib[fib.size() - 1] + fib[fib.size() - 2]);
        std::vector<uint32_t> h(DEF_NLIT, 0);
        for (size_t i = 0; i < fib.size(); i++) h[(i * 37) % DEF_NLIT] = fib[i];                // 30 Fibonacci counts: depth 29 without a limit
        bad += check_lengths(S, h, 15, "fibonacci at 15");
        bad += check_lengths(S, std::vector<uint32_t>(fib.begin(), fib.begin() + DEF_NCL), 7, "fibonacci at 7");
        uint64_t rng = 0x9e3779b97f4a7c15ull;
        auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        for (int k = 0; k < 2000; k++) {
            const uint32_t which = (uint32_t) (next() % 3), nsym = which == 0 ? DEF_NLIT : which == 1 ? DEF_NDIST : DEF_NCL, limit = which == 2 ? 7 : 15;
            std::vector<uint32_t> r(nsym, 0);
            const uint32_t fill = (uint32_t) (next() % 4);
            for (uint32_t s = 0; s < nsym; s++) {
                const uint64_t x = next();
                r[s] = fill == 0 ? (uint32_t) (x % 33000) : fill == 1 ? ((x & 7) ? 0 : (uint32_t) (x >> 8) % 100) : fill == 2 ? (uint32_t) 1 << (x % 15) : (uint32_t) (x % 3);
            }
            char what[64];
            snprintf(what, sizeof what, "random %d (%u symbols)", k, nsym);
            bad += check_lengths(S, r, limit, what);
        }
        for (uint32_t nsym : {DEF_NLIT, DEF_NDIST, DEF_NCL}) {
            const uint32_t limit = nsym == DEF_NCL ? 7 : 15;
            bad += check_lengths(S, std::vector<uint32_t>(nsym, 0), limit, "all zero");
            for (uint32_t s : {0u, 1u, nsym / 2, nsym - 1}) {
                std::vector<uint32_t> one(nsym, 0);
                one[s] = s == 1 ? 1 : 32768;
                bad += check_lengths(S, one, limit, "a single entry");
            }
        }
    }

    // ---- the corpus
    uint32_t ncalls = 0;
    if (fread(&ncalls, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < ncalls; c++) {
        struct __attribute__((packed)) { uint32_t nameLen; uint64_t bufLen; uint32_t njobs; } h;
        if (fread(&h, sizeof h, 1, f) != 1) return 2;
        std::string name(h.nameLen, '\0');
        uint8_t *text = new uint8_t[h.bufLen ? h.bufLen : 1];                                    // the buffer's last byte is its allocation's last byte
        std::vector<uint64_t> jobs(2 * (size_t) h.njobs);
        if (fread(&name[0], h.nameLen, 1, f) != 1 || (h.bufLen && fread(text, h.bufLen, 1, f) != 1) || fread(jobs.data(), 16, h.njobs, f) != h.njobs) return 2;
        // the tables of mbgc_fasta_deflate_dev
        std::vector<DefChunk> chunks;
        std::vector<DefJobIn> jtab;
        std::vector<DefPackIn> pack;
        for (uint32_t k = 0; k < h.njobs; k++) {
            const uint64_t off = jobs[2 * k], len = jobs[2 * k + 1];
            const uint32_t m = (uint32_t) (len ? (len + DEF_CHUNK - 1) / DEF_CHUNK : 1);
            jtab.push_back({len, (uint32_t) chunks.size(), m});
            for (uint32_t i = 0; i < m; i++) {
                const uint64_t at = (uint64_t) i * DEF_CHUNK;
                chunks.push_back({off + at, (uint32_t) (len - at < DEF_CHUNK ? len - at : DEF_CHUNK), i + 1 == m ? 1u : 0u});
                pack.push_back({0, k, (i == 0 ? 1u : 0u) | (i + 1 == m ? 2u : 0u)});
            }
        }
        const size_t nc = chunks.size();
        uint8_t *slots = (uint8_t *) aligned_alloc(16, nc * DEF_SLOT);
        std::vector<DefChunkOut> outs(nc);
        for (size_t k = 0; k < nc; k++) {
            memset(S, 0xcc, sizeof *S);
            Def D(*S, text + chunks[k].inOff, chunks[k].n, chunks[k].last != 0, slots + k * DEF_SLOT);
            outs[k] = D.run();
        }
        struct Res { uint64_t outOff, outLen; uint32_t chunks, stored; };
        std::vector<Res> res(h.njobs);
        uint64_t total = 0;
        for (uint32_t k = 0; k < h.njobs; k++) {
            res[k] = {total, 0, jtab[k].nchunks, 0};
            total += 10;
            for (uint32_t i = jtab[k].chunk0; i < jtab[k].chunk0 + jtab[k].nchunks; i++) {
                pack[i].dst = total;
                total += outs[i].bytes & ~DEF_STORED;
                res[k].stored += (outs[i].bytes & DEF_STORED) != 0;
            }
            total += 8;
            res[k].outLen = total - res[k].outOff;
        }
        for (uint32_t shift : {0u, 5u}) {                                                       // the output at two alignments: the same bytes
            uint8_t *gzAlloc = (uint8_t *) malloc(shift + total), *gz = gzAlloc + shift;        // its last byte is the allocation's last byte
            memset(gzAlloc, 0xa5, shift);
            std::vector<uint32_t> jobCrc(h.njobs, 0);
            uint32_t red[DEF_WAVE];
            for (size_t k = 0; k < nc; k++) def_pack_chunk(red, slots, outs.data(), pack.data(), jtab.data(), (uint32_t) k, gz, jobCrc.data());
            for (uint32_t k = 0; k < h.njobs; k++) {
                const uint64_t off = jobs[2 * k], len = jobs[2 * k + 1];
                const uint8_t *g = gz + res[k].outOff;
                std::vector<uint8_t> back;
                unsigned members = 0;
                bool ok = inflate_all(g, res[k].outLen, back, members) && members == 1 && back.size() == len && (len == 0 || memcmp(back.data(), text + off, len) == 0);
                uint32_t crc = 0, isize = 0;
                memcpy(&crc, g + res[k].outLen - 8, 4); memcpy(&isize, g + res[k].outLen - 4, 4);
                ok = ok && crc == jobCrc[k] && crc == (uint32_t) crc32(0, text + off, (uInt) len) && isize == (uint32_t) len && res[k].outLen <= deflate_bound(len);
                if (!ok) { printf("FAILED %s job %u (output shifted by %u): %llu bytes in, %llu out, %u members\n", name.c_str(), k, shift, (unsigned long long) len, (unsigned long long) res[k].outLen, members); bad++; }
                if (shift == 0) printf("%s %u %llu %llu %u %u\n", name.c_str(), k, (unsigned long long) len, (unsigned long long) res[k].outLen, res[k].chunks, res[k].stored);
            }
            if (shift == 0 && o) { fwrite(&total, 8, 1, o); fwrite(gz, 1, total, o); }
            for (uint32_t k = 0; k < shift; k++) if (gzAlloc[k] != 0xa5) { printf("FAILED %s: a byte in front of the output was written\n", name.c_str()); bad++; break; }
            free(gzAlloc);
        }
        free(slots);
        delete[] text;
    }
    fclose(f);
    if (o) fclose(o);
    delete S;
    if (bad) return 1;
    printf("ok: %u calls\n", ncalls);
    return 0;
}
