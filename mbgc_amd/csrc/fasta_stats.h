// The scan of `mbgc-hip s` (included by fasta_input.hip, inside namespace fa, behind fasta_tiles.h, whose grid it
// scans): the classes of a byte and the steps of one lane. Kept free of HIP calls so that the
// same text compiles as plain C++: tests/fasta_stats_emu.cpp runs the steps tile by tile and lane by lane on the CPU under
// AddressSanitizer, the wave's shuffles emulated by arrays. The shuffles, the block's sum in LDS, the atomic adds to a record's row and
// the atomic cursor of the edge buffer stay in fasta_input.hip (k_fa_stats).
// ---- counts: per record a, c, g, t (with u), n without case, `other` = every other byte, `lower` = the bytes in 'a'..'z' whatever the
// letter. A lane classifies its 16 positions and packs its seven sums (a, c, g, t | n, lower, valid — `other` is valid less the five
// letters) into two 64-bit words of 16-bit fields: a tile holds 4096 positions, so the fields cannot carry into each other when the
// words of a whole block are added.
// ---- runs: class 0 is N / n, class 1 is 'a'..'z'. A run is a maximal stretch of one class inside one record, found by its two EDGES
// and never walked: position p is a start when byte p is in the class and p == 0 or byte p - 1 is not, an end when byte p is in the
// class and p == len - 1 or byte p + 1 is not. A lane holds the class of its 16 positions as a 16-bit mask per class, in which a
// position outside the record is 0 whatever memory holds there; the bit in front of the mask and the bit behind it are the
// neighbouring lane's (a shuffle) or, for the first and last lane of a wave, one guarded byte load (stats_class_at). The edges of a
// record and class pair up when sorted: the i-th start with the i-th end.
// ---- tiles: the shared grid of fasta_tiles.h; a record's start positions are its bytes, so every record with a byte has tiles. A
// lane reads its 16 positions as one aligned vector; a vector that does not lie inside seq[0, seqBytes) whole is read byte by byte,
// the bytes inside only (find_stage_step's rule), and a lane none of whose positions lie in the record reads nothing.
constexpr uint32_t STATS_TILE = SCAN_TILE, STATS_THREADS = SCAN_THREADS, STATS_PER = SCAN_PER;   // 16 positions per lane: a class is a 16-bit mask
constexpr uint64_t STATS_EDGES_FIRST = 65536;                         // rows of the entry point's first edge buffer; it grows to the cursor's count
constexpr uint32_t STATS_CLS_N = 1u, STATS_CLS_LOWER = 2u;            // the class bits of a byte

struct StatsEdge { uint64_t pos; uint32_t rec, kind; };               // kind: the class (0, 1), + 2 for an end
struct StatsLane {
    uint64_t sumA, sumB;      // a | c << 16 | g << 32 | t << 48,  n | lower << 16 | valid << 32
    uint32_t masks;           // bit k: position k is in class 0; bit 16 + k: in class 1 (positions outside the record: 0)
};
struct StatsEdges { uint32_t startN, endN, startL, endL; };          // 16-bit masks over the lane's positions

__host__ __device__ __forceinline__ uint32_t stats_class(uint8_t b) {
    return ((b | 0x20) == 'n' ? STATS_CLS_N : 0u) | ((uint8_t) (b - 'a') < 26 ? STATS_CLS_LOWER : 0u);
}

// the class bits of position t of the record, 0 for a position outside it: the one guarded load of a wave's first and last lane
__device__ __forceinline__ uint32_t stats_class_at(const uint8_t *__restrict__ seq, const ScanRec rec, int64_t t) {
    return t >= 0 && (uint64_t) t < rec.len ? stats_class(seq[rec.off + (uint64_t) t]) : 0u;
}

// the first step: lane `lane` (of STATS_THREADS) owns the STATS_PER positions from address tileAddr + 16 lane on
__device__ __forceinline__ StatsLane stats_lane_step(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec rec, uintptr_t tileAddr, uint32_t lane) {
    StatsLane L = {0, 0, 0};
    const uintptr_t lo = (uintptr_t) seq, hi = lo + seqBytes, v = tileAddr + 16u * lane;
    // the lane's first position in the record; in front of the record in its first tile only
    const int64_t t0 = (int64_t) v - (int64_t) (lo + rec.off);
    if (t0 + (int64_t) STATS_PER <= 0 || t0 >= (int64_t) rec.len) return L;
    ScanVec x = {{0, 0, 0, 0}};
    if (v >= lo && v + 16 <= hi) x = *(const ScanVec *) v;
    else
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (v + k >= lo && v + k < hi) x.w[k >> 2] |= (uint32_t) *(const uint8_t *) (v + k) << (8 * (k & 3));
    uint32_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};                         // a, c, g, t, n, lower, valid
#pragma unroll
    for (uint32_t k = 0; k < STATS_PER; k++) {
        const int64_t t = t0 + k;
        if (t < 0 || t >= (int64_t) rec.len) continue;
        const uint8_t b = (uint8_t) (x.w[k >> 2] >> (8 * (k & 3))), f = b | 0x20;
        const uint32_t lower = (uint8_t) (b - 'a') < 26, isN = f == 'n';
        cnt[0] += f == 'a'; cnt[1] += f == 'c'; cnt[2] += f == 'g'; cnt[3] += (f == 't') | (f == 'u');
        cnt[4] += isN; cnt[5] += lower; cnt[6] += 1;
        L.masks |= (isN << k) | (lower << (16 + k));
    }
    L.sumA = (uint64_t) cnt[0] | (uint64_t) cnt[1] << 16 | (uint64_t) cnt[2] << 32 | (uint64_t) cnt[3] << 48;
    L.sumB = (uint64_t) cnt[4] | (uint64_t) cnt[5] << 16 | (uint64_t) cnt[6] << 32;
    return L;
}

// counter i (of 7: a, c, g, t, n, other, lower — the order of mbgc_fasta_counts_t) out of the two words summed over a tile
__host__ __device__ __forceinline__ uint64_t stats_counter(uint64_t sumA, uint64_t sumB, uint32_t i) {
    const uint64_t a = sumA & 0xffff, c = (sumA >> 16) & 0xffff, g = (sumA >> 32) & 0xffff, t = sumA >> 48;
    const uint64_t n = sumB & 0xffff, lower = (sumB >> 16) & 0xffff, valid = (sumB >> 32) & 0xffff;
    return i == 0 ? a : i == 1 ? c : i == 2 ? g : i == 3 ? t : i == 4 ? n : i == 5 ? valid - a - c - g - t - n : lower;
}

// the second step: the lane's masks, the masks of the lane in front of it and of the lane behind it (the class bits of one position
// each is all that is taken from them: prev's last, next's first) -> the edges among the lane's positions, of the classes in `want`
// (STATS_CLS_*)
__host__ __device__ __forceinline__ StatsEdges stats_edges(uint32_t masks, uint32_t prevLast, uint32_t nextFirst, uint32_t want) {
    const uint32_t n = want & STATS_CLS_N ? masks & 0xffff : 0u, l = want & STATS_CLS_LOWER ? masks >> 16 : 0u;
    const uint32_t pn = prevLast & STATS_CLS_N ? 1u : 0u, pl = prevLast & STATS_CLS_LOWER ? 1u : 0u;
    const uint32_t nn = nextFirst & STATS_CLS_N ? 0x8000u : 0u, nl = nextFirst & STATS_CLS_LOWER ? 0x8000u : 0u;
    StatsEdges E;
    E.startN = n & ~((n << 1) | pn) & 0xffff; E.endN = n & ~((n >> 1) | nn);
    E.startL = l & ~((l << 1) | pl) & 0xffff; E.endL = l & ~((l >> 1) | nl);
    return E;
}
__host__ __device__ __forceinline__ uint32_t stats_edge_count(const StatsEdges E) {
    return (uint32_t) (__builtin_popcount(E.startN) + __builtin_popcount(E.endN) + __builtin_popcount(E.startL) + __builtin_popcount(E.endL));
}
// the class bits a neighbour hands over: of its last position (to the lane behind it) and of its first (to the lane in front of it)
__host__ __device__ __forceinline__ uint32_t stats_last_of(uint32_t masks) { return ((masks >> 15) & 1u) | ((masks >> 31) & 1u) << 1; }
__host__ __device__ __forceinline__ uint32_t stats_first_of(uint32_t masks) { return (masks & 1u) | ((masks >> 16) & 1u) << 1; }

// the lane's edges to rows [base, base + stats_edge_count(E)) of the edge buffer, the rows below cap only; t0 = the lane's first position
__device__ __forceinline__ void stats_edges_write(const StatsEdges E, int64_t t0, uint32_t rec, uint64_t base, uint64_t cap, StatsEdge *__restrict__ out) {
    const uint32_t m[4] = {E.startN, E.startL, E.endN, E.endL};      // kinds 0, 1, 2, 3
#pragma unroll
    for (uint32_t kind = 0; kind < 4; kind++)
        for (uint32_t rest = m[kind]; rest; rest &= rest - 1, base++)
            if (base < cap) out[base] = StatsEdge{(uint64_t) (t0 + __builtin_ctz(rest)), rec, kind};
}
