// The inverse of the `-m3` reverse-complement pass without a GPU: the item bodies of k_varint_decode and k_check and the lane of
// k_restore_fill (mbgc_amd/csrc/copmem_restore_lane.h, which holds no HIP call) compiled as plain C++ and run over the corpus of
// tests/_rcmut.py — item by item, lane by lane, tile by tile — against the verdicts and bytes of the referee
// (tests/_rcrestore.py, restore_bounded), which the corpus file carries. Built with AddressSanitizer and UBSan by
// tests/test_rcrestore_mutants_cpu.py, with and without -DMBGC_RC_RESTORE_BYTEWISE. Every buffer has the size the plan gives it
// and not a byte more: the cut stream its whole tiles and CUT_PAD zero bytes, len and cum M + 1 entries, d and src M, the
// destination the restored length, the maps their own lengths; an address formed from a map's value that leaves one of them ends
// the run. The marks, the numbering of the values and the running sums, which on the device are scans, are plain loops here; the
// sizes-only refusals are restated from plan(). No GPU.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
namespace cmr {
#include "../mbgc_amd/csrc/copmem_restore_lane.h"
}
using namespace cmr;

static FILE *in;
static uint64_t rd64() { uint64_t v; if (fread(&v, 8, 1, in) != 1) { printf("corpus file ends early\n"); exit(2); } return v; }
// exactly n bytes on the heap (one for n == 0, never read): AddressSanitizer's red zone starts where the blob ends
static uint8_t *rd_blob(uint64_t &n) {
    n = rd64();
    uint8_t *p = new uint8_t[n ? n : 1];
    if (n && fread(p, 1, n, in) != n) { printf("corpus file ends early\n"); exit(2); }
    return p;
}

struct Verdict { bool ok; uint64_t M, total, deepest, minLen, orgLen; std::string why; };

// plan() and fill() on the CPU -> accepted or not; the restored bytes into out (exactly orgLen)
static Verdict run(const uint8_t *lut, const uint8_t *seq, uint64_t n, const uint8_t *mapOff, uint64_t mapOffLen, const uint8_t *mapLen, uint64_t mapLenLen,
                   int offBytes, uint8_t *&out) {
    Verdict v{false, 0, 0, 0, 0, 0, ""};
    out = nullptr;
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    std::vector<uint64_t> markPos;
    for (uint64_t p = 0; p < n; p++)
        if (seq[p] == MARK) markPos.push_back(p);
    const uint64_t M = markPos.size();
    uint64_t nval = 0;
    for (uint64_t j = 0; j < mapLenLen; j++) nval += EndsValue()(mapLen[j]);
    if (M == 0 && mapOffLen) { v.why = "rcMapOff without a mark"; return v; }
    if (M && (mapOffLen % M || (mapOffLen / M != 4 && mapOffLen / M != 8))) { v.why = "rcMapOff's size"; return v; }
    const int width = M ? (int) (mapOffLen / M) : 0;
    if (M && width != offBytes) { v.why = "rcMapOff's width"; return v; }
    if (mapLenLen == 0 && M) { v.why = "rcMapLen empty"; return v; }
    if (mapLenLen && mapLen[mapLenLen - 1] >= 128) { v.why = "the last value does not end"; return v; }
    if (mapLenLen && nval != M + 1) { v.why = "the number of values"; return v; }
    uint8_t *cut = new uint8_t[ntiles * TILE + CUT_PAD]();
    memcpy(cut, seq, n);
    uint64_t *len = new uint64_t[M + 1], *cum = new uint64_t[M + 1], *d = new uint64_t[M], *src = new uint64_t[M];
    uint64_t total = 0, minLen = 0;
    bool refused = false;
    cum[0] = 0;
    if (mapLenLen) {
        uint64_t *val = new uint64_t[M + 1];
        bool anyLong = false;
        uint64_t at = 0;
        for (uint64_t j = 0; j < mapLenLen; j++) {                              // (at: the exclusive scan of EndsValue)
            if (value_starts_at(mapLen, j)) {
                bool tooLong;
                const uint64_t x = value_at(mapLen, mapLenLen, j, tooLong);
                anyLong |= tooLong;
                if (at < M + 1) val[at] = x;
            }
            at += EndsValue()(mapLen[j]);
        }
        for (uint64_t i = 0; i <= M; i++) len[i] = length_of(val, M, i);
        for (uint64_t i = 0; i < M; i++) cum[i + 1] = SatAdd()(cum[i], len[i]);
        bool badSource = false;
        for (uint64_t i = 0; i < M; i++) badSource |= !match_in_bounds(markPos.data(), mapOff, width, len, cum, i, d[i], src[i]);
        total = cum[M]; minLen = val[0];
        delete[] val;
        if (anyLong) { v.why = "a value of more than 10 bytes"; refused = true; }
        else if (minLen > UINT32_MAX) { v.why = "the minimal length"; refused = true; }
        else if (total == SAT) { v.why = "the sum of the lengths"; refused = true; }
        else if (badSource) { v.why = "a source"; refused = true; }
    }
    if (!refused) {
        const uint64_t org = n - M + total;
        Plan P = {cut, d, src, len, cum, M, n, org};
        out = new uint8_t[org ? org : 1];
        uint32_t deepest = 0;
        const uint64_t otiles = (org + TILE - 1) / TILE;
        for (uint64_t tile = 0; tile < otiles; tile++) {
            uint64_t lo, hi;
            matches_of_tile(P, tile, lo, hi);
            for (uint64_t lane = 0; lane < (uint64_t) TPB; lane++) {
                const uint64_t p0 = tile * TILE + lane * LANE;
                if (p0 >= org) continue;
                restore_lane(P, lut, out, p0, lo, hi, deepest);
            }
        }
        v.ok = true; v.M = M; v.total = total; v.deepest = deepest; v.minLen = minLen; v.orgLen = org;
    }
    delete[] cut; delete[] len; delete[] cum; delete[] d; delete[] src;
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2 || !(in = fopen(argv[1], "rb"))) { printf("usage: rcrestore_emu corpus-file\n"); return 2; }
    uint8_t head[8], lut[256];
    if (fread(head, 1, 8, in) != 8 || memcmp(head, "RCMUT1\0\0", 8) || fread(lut, 1, 256, in) != 256) { printf("not a corpus file\n"); return 2; }
    int failures = 0;
    // ---- the values of k_varint_decode's item body alone
    const uint64_t nstreams = rd64();
    uint64_t nvalues = 0;
    for (uint64_t s = 0; s < nstreams; s++) {
        uint64_t nb;
        uint8_t *bytes = rd_blob(nb);
        const uint64_t want = rd64();
        uint64_t at = 0;
        for (uint64_t j = 0; j < nb; j++) {
            if (!value_starts_at(bytes, j)) continue;
            bool tooLong;
            const uint64_t x = value_at(bytes, nb, j, tooLong);
            if (at >= want) { printf("FAIL varint stream %llu: more than %llu values\n", (unsigned long long) s, (unsigned long long) want); return 1; }
            const uint64_t wv = rd64(), wok = rd64();
            at++; nvalues++;
            if (tooLong != !wok || (wok && x != wv)) {
                printf("FAIL varint stream %llu, value %llu: %llu%s, expected %llu%s\n", (unsigned long long) s, (unsigned long long) (at - 1), (unsigned long long) x,
                       tooLong ? " (too long)" : "", (unsigned long long) wv, wok ? "" : " (too long)");
                failures++;
            }
        }
        if (at != want) { printf("FAIL varint stream %llu: %llu values, expected %llu\n", (unsigned long long) s, (unsigned long long) at, (unsigned long long) want); return 1; }
        delete[] bytes;
    }
    // ---- the cases
    const uint64_t ncases = rd64();
    uint64_t accepted = 0, deepestSeen = 0;
    double slowest = 0;
    std::string slowestName;
    for (uint64_t c = 0; c < ncases; c++) {
        uint64_t nameLen, n, mapOffLen, mapLenLen;
        uint8_t *nm = rd_blob(nameLen);
        const std::string name((const char *) nm, nameLen);
        delete[] nm;
        const int offBytes = (int) rd64();
        const bool wantOk = rd64() != 0;
        uint8_t *seq = rd_blob(n), *mapOff = rd_blob(mapOffLen), *mapLen = rd_blob(mapLenLen);
        uint64_t wM = 0, wTotal = 0, wDeep = 0, wMin = 0, wLen = 0;
        uint8_t *want = nullptr;
        if (wantOk) { wM = rd64(); wTotal = rd64(); wDeep = rd64(); wMin = rd64(); want = rd_blob(wLen); }
        uint8_t *got = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        const Verdict v = run(lut, seq, n, mapOff, mapOffLen, mapLen, mapLenLen, offBytes, got);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (sec > slowest) { slowest = sec; slowestName = name; }
        std::string why;
        char buf[200];
        if (v.ok != wantOk) why = v.ok ? "accepted what the referee refuses" : "refused (" + v.why + ") what the referee accepts";
        else if (v.ok) {
            if (v.M != wM || v.total != wTotal || v.minLen != wMin || v.orgLen != wLen) {
                snprintf(buf, sizeof buf, "marks %llu, from matches %llu, minimum %llu, length %llu; the referee: %llu, %llu, %llu, %llu", (unsigned long long) v.M,
                         (unsigned long long) v.total, (unsigned long long) v.minLen, (unsigned long long) v.orgLen, (unsigned long long) wM,
                         (unsigned long long) wTotal, (unsigned long long) wMin, (unsigned long long) wLen);
                why = buf;
            } else if (memcmp(got, want, wLen)) {
                uint64_t at = 0;
                while (got[at] == want[at]) at++;
                snprintf(buf, sizeof buf, "byte %llu of %llu is 0x%02x, the referee's 0x%02x", (unsigned long long) at, (unsigned long long) wLen, got[at], want[at]);
                why = buf;
            } else if (v.deepest != wDeep) {
                snprintf(buf, sizeof buf, "deepest chain %llu, the referee's %llu", (unsigned long long) v.deepest, (unsigned long long) wDeep);
                why = buf;
            }
            accepted++;
            if (v.deepest > deepestSeen) deepestSeen = v.deepest;
        }
        if (!why.empty()) { printf("FAIL %s: %s\n", name.c_str(), why.c_str()); failures++; }
        delete[] seq; delete[] mapOff; delete[] mapLen; delete[] want; delete[] got;
    }
    printf("slowest: %.2f s, %s\n", slowest, slowestName.c_str());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok: %llu values, %llu cases, %llu accepted, %llu refused, deepest chain %llu\n", (unsigned long long) nvalues, (unsigned long long) ncases,
           (unsigned long long) accepted, (unsigned long long) (ncases - accepted), (unsigned long long) deepestSeen);
    return 0;
}
