// The scan of `mbgc-hip f` (included by fasta_input.hip, inside namespace fa): the gram table mbgc_fasta_find_dev makes on the host, the
// search of a tile's record and the two steps of one lane. Kept free of HIP calls so that the same text compiles as plain C++:
// tests/fasta_find_emu.cpp runs the steps tile by tile and lane by lane on the CPU under AddressSanitizer. The staging buffer in LDS,
// the table's copy there, the barrier and the atomic cursor of the hit buffer stay in fasta_input.hip (k_fa_find).
// ---- a hit is (record r, pattern q, position p, mismatches d): p + len(q) <= the record's length, d = the positions j with
// fold(text[p + j]) != fold(q[j]), d <= K. What a text byte costs does not grow with the number of patterns: a pattern of L bytes is cut
// into K + 1 disjoint seeds, seed j at offset j * (L / (K + 1)) — each of them at least FIND_GRAM bytes, as L >= FIND_GRAM (K + 1) — and an
// alignment with at most K mismatches leaves one seed exact (pigeonhole), so the first FIND_GRAM folded bytes of that seed, its gram,
// stand in the text as they are. The host keys an open-addressing table by the grams; the (pattern, seed) rows that share a key are one
// chain. Every text position t with t + FIND_GRAM <= the record's length is looked at exactly once, by the lane that owns it: it packs
// the folded gram at t from LDS, probes the table (half empty at most) and, on a hit, walks the chain. Row (q, j) proposes the start
// t - seedOff_j; the lane counts the mismatches of the whole pattern there and reports the alignment only if no gram j' < j of q is
// exact at its own place start + seedOff_j' — the lane that owns that place reports it. So every hit is reported exactly once, by the
// smallest exact gram, and no pass removes duplicates afterwards.
// ---- tiles: the shared grid of fasta_tiles.h (ScanRec, ScanVec, scan_tile); a record's start positions are those of its grams, none
// when no pattern fits into it (find_positions). Every tile is staged with aligned 16-byte loads. A staged byte outside the record is
// never looked at: a position counts only when its whole gram lies inside the record, and a proposed start only when the whole
// pattern does.
constexpr uint32_t FIND_TILE = SCAN_TILE, FIND_GRAM = 8, FIND_THREADS = SCAN_THREADS, FIND_PER = SCAN_PER;   // 16 positions per lane
constexpr uint32_t FIND_VECS = FIND_TILE / 16 + 1, FIND_STAGE = FIND_VECS * 16;    // the tile and the 16 bytes behind it (FIND_GRAM - 1 are needed)
constexpr uint32_t FIND_LDS_BITS = 11;                                             // the table lives in LDS up to 2048 slots (32 KiB)
constexpr uint32_t FIND_MAX_K = 3, FIND_MAX_LEN = 65535;
static_assert(MBGC_FASTA_FIND_TILE == FIND_TILE, "the tile the public header states");

struct FindSlot {
    uint64_t key;             // the folded gram, byte j in bits [8 j, 8 j + 8)
    uint32_t first, count;    // the chain: rows [first, first + count) of the seed table; count == 0: an empty slot
};
struct FindSeed { uint32_t pat; uint16_t off, j; };                   // seed j of the caller's pattern `pat`, `off` bytes into it
struct FindPat { uint64_t off; uint32_t len, step; };                 // folded bytes [off, off + len) of the table's blob; seed j at j * step

__host__ __device__ __forceinline__ uint32_t find_hash(uint64_t key, uint32_t bits) { return (uint32_t) ((key * 0x9E3779B97F4A7C15ull) >> (64 - bits)); }
__host__ __device__ __forceinline__ uint8_t find_fold(uint8_t b) { return (uint8_t) ((uint8_t) ((b | 0x20) - 'a') < 26 ? b & 0xDF : b); }

// the start positions of a record of `len` bytes (scan_tiles_of): its grams, none when no pattern fits into it
__host__ __device__ __forceinline__ uint64_t find_positions(uint64_t len, uint32_t shortest) {
    return len < shortest || len < FIND_GRAM ? 0 : len - FIND_GRAM + 1;
}

// the first step: vector `vec` (of FIND_VECS) of the tile whose first byte has address `tileAddr` (a multiple of 16) goes to
// stage[16 vec, 16 vec + 16) — one aligned 16-byte load when the vector lies inside seq[0, seqBytes), else its bytes inside, one by one
__device__ __forceinline__ void find_stage_step(const uint8_t *__restrict__ seq, uint64_t seqBytes, uintptr_t tileAddr, uint32_t vec, uint8_t *stage) {
    const uintptr_t lo = (uintptr_t) seq, hi = lo + seqBytes, v = tileAddr + 16u * vec;
    if (v >= lo && v + 16 <= hi) { *(ScanVec *) (stage + 16u * vec) = *(const ScanVec *) v; return; }
    for (uint32_t k = 0; k < 16; k++)
        if (v + k >= lo && v + k < hi) stage[16u * vec + k] = *(const uint8_t *) (v + k);
}

// does pattern P stand at txt with at most K mismatches? -> the mismatches, K + 1 when there are more
__device__ __forceinline__ uint32_t find_count(const uint8_t *__restrict__ txt, const uint8_t *__restrict__ pb, uint32_t len, uint32_t K) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < len && d <= K; i++) d += find_fold(txt[i]) != pb[i];
    return d;
}

// the second step, behind a barrier: lane `lane` (of FIND_THREADS) owns the FIND_PER positions from address tileAddr + 16 lane on;
// emit(pos, pattern, mismatches) is called once per hit of record `rec` this lane reports
template <class Emit>
__device__ __forceinline__ void find_lane_step(const uint8_t *__restrict__ seq, const ScanRec rec, uintptr_t tileAddr, uint32_t lane, const uint8_t *stage,
                                               const FindSlot *slots, uint32_t bits, const FindSeed *__restrict__ seeds, const FindPat *__restrict__ pats,
                                               const uint8_t *__restrict__ patBytes, uint32_t K, Emit &&emit) {
    const uint8_t *text = seq + rec.off;
    // the lane's first position in the record; in front of the record in its first tile only
    const int64_t t0 = (int64_t) (tileAddr + 16u * lane) - (int64_t) (uintptr_t) text;
    if (t0 + (int64_t) FIND_PER <= 0 || t0 + (int64_t) FIND_GRAM > (int64_t) rec.len) return;
    const ScanVec a = *(const ScanVec *) (stage + 16u * lane), b = *(const ScanVec *) (stage + 16u * lane + 16);
    const uint32_t w[8] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]};
    uint64_t key = 0;
#pragma unroll
    for (uint32_t i = 0; i < FIND_GRAM - 1; i++) key |= (uint64_t) find_fold((uint8_t) (w[i >> 2] >> (8 * (i & 3)))) << (8 * (i + 1));
    const uint32_t mask = (1u << bits) - 1u;
#pragma unroll
    for (uint32_t k = 0; k < FIND_PER; k++) {
        const uint32_t i = k + FIND_GRAM - 1;
        key = (key >> 8) | ((uint64_t) find_fold((uint8_t) (w[i >> 2] >> (8 * (i & 3)))) << 56);
        const int64_t t = t0 + k;
        if (t < 0 || t + (int64_t) FIND_GRAM > (int64_t) rec.len) continue;
        for (uint32_t s = find_hash(key, bits);; s = (s + 1) & mask) {
            const FindSlot e = slots[s];
            if (e.count == 0) break;
            if (e.key != key) continue;
            for (uint32_t c = e.first; c < e.first + e.count; c++) {
                const FindSeed sd = seeds[c];
                const FindPat P = pats[sd.pat];
                if (t < (int64_t) sd.off || (uint64_t) (t - sd.off) + P.len > rec.len) continue;      // the pattern would not lie inside the record
                const uint64_t start = (uint64_t) (t - sd.off);
                const uint8_t *txt = text + start, *pb = patBytes + P.off;
                const uint32_t d = find_count(txt, pb, P.len, K);
                if (d > K) continue;
                bool earlier = false;                                // an exact gram in front of this one: its own lane reports the alignment
                for (uint32_t j = 0; j < sd.j && !earlier; j++) earlier = find_count(txt + j * P.step, pb + j * P.step, FIND_GRAM, 0) == 0;
                if (!earlier) emit(start, sd.pat, d);
            }
            break;
        }
    }
}

// The host's half: the caller's patterns (back to back, patOff[npat + 1], letters only, FIND_GRAM (K + 1) <= length <= FIND_MAX_LEN) ->
// their folded bytes, the seed rows in chains and the slots (1 << bits of them, at least twice the chains). The same pattern given
// twice is two rows of one chain: every index is reported.
struct FindTable { uint32_t bits = 0, shortest = 0; std::vector<FindSlot> slots; std::vector<FindSeed> seeds; std::vector<FindPat> pats; std::vector<uint8_t> bytes; };
inline void find_build_table(const uint8_t *patterns, const uint64_t *patOff, uint64_t npat, uint32_t K, FindTable &T) {
    T.slots.clear(); T.seeds.clear(); T.pats.clear(); T.bytes.clear();
    T.shortest = FIND_MAX_LEN;
    T.bytes.resize(patOff[npat] - patOff[0]);
    struct Row { uint64_t key; FindSeed seed; };
    std::vector<Row> rows;
    for (uint64_t q = 0; q < npat; q++) {
        const uint32_t len = (uint32_t) (patOff[q + 1] - patOff[q]), step = len / (K + 1);
        const uint64_t at = patOff[q] - patOff[0];
        for (uint32_t i = 0; i < len; i++) T.bytes[at + i] = find_fold(patterns[patOff[q] + i]);
        T.pats.push_back(FindPat{at, len, step});
        T.shortest = std::min(T.shortest, len);
        for (uint32_t j = 0; j <= K; j++) {
            Row r = {0, FindSeed{(uint32_t) q, (uint16_t) (j * step), (uint16_t) j}};
            for (uint32_t i = 0; i < FIND_GRAM; i++) r.key |= (uint64_t) T.bytes[at + j * step + i] << (8 * i);
            rows.push_back(r);
        }
    }
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.seed.pat != b.seed.pat) return a.seed.pat < b.seed.pat;
        return a.seed.j < b.seed.j;
    });
    uint64_t chains = 0;
    for (size_t k = 0; k < rows.size(); k++) chains += k == 0 || rows[k].key != rows[k - 1].key;
    T.bits = 6;
    while ((1ull << T.bits) < 2 * chains) T.bits++;
    T.slots.assign((size_t) 1 << T.bits, FindSlot{0, 0, 0});
    const uint32_t mask = (1u << T.bits) - 1u;
    for (size_t c = 0; c < rows.size();) {
        size_t e = c + 1;
        while (e < rows.size() && rows[e].key == rows[c].key) e++;
        uint32_t s = find_hash(rows[c].key, T.bits);
        while (T.slots[s].count) s = (s + 1) & mask;
        T.slots[s] = FindSlot{rows[c].key, (uint32_t) c, (uint32_t) (e - c)};
        c = e;
    }
    T.seeds.reserve(rows.size());
    for (const Row &r : rows) T.seeds.push_back(r.seed);
}
