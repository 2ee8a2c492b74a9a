// The scan of `mbgc-hip k` (included by fasta_input.hip, inside namespace fa, behind fasta_tiles.h, whose grid it
// scans): the start positions of a record, the packing of a vector and the k-mer hashes of one lane. Kept free of HIP calls so
// that the same text compiles as plain C++: tests/fasta_sketch_emu.cpp runs the steps tile by tile and lane by lane on the CPU under
// AddressSanitizer, the wave's shuffles emulated by arrays. The shuffles, the ballot, the atomic cursor of the row buffer, the groups'
// k-mer counters, the sort and the pair search stay in fasta_input.hip (k_fa_sketch, k_fa_sketch_flag, k_fa_sketch_compact,
// k_fa_sketch_pairs).
// ---- the hash (the contract of include/mbgc_fasta.h): codes A/a 0, C/c 1, G/g 2, T/t/U/u 3, every other byte invalid; a k-mer is k
// bytes of ONE record, skipped when one of them is invalid; fw = the codes as a number, the first base in the highest pair of 2 k
// bits; rc = the same of the reverse complement; h = fmix64(min(fw, rc) ^ SKETCH_SEED). Not the hash of Mash or sourmash.
// ---- packing: a lane owns one aligned 16-byte vector and packs it into a 32-bit code word — position j of the vector in bits
// [30 - 2 j, 32 - 2 j), so that positions read from the top — and a 16-bit invalid mask, bit j for position j. A position OUTSIDE THE
// RECORD is invalid whatever memory holds there (and a vector none of whose positions lie in the record is not read at all), so a k-mer
// that would reach over the record's end, or start in front of it, holds an invalid position and drops out by the one test that also
// drops N: no byte outside the record, and so none outside the buffer, can reach a result. Both words travel as one 64-bit value
// (codes | bad << 32). A k-mer that starts at the lane's position j reads k - 1 <= 31 further positions: the words of the TWO following
// vectors, by shuffle inside the wave, by sketch_pack on the vector's address for the wave's last two lanes.
// ---- a position: the 32 positions from j on are one 64-bit window W (position j on top); fw = W >> (64 - 2 k), never a shift by 64
// as k >= 1. rc comes from fw with no second state: complement, reverse the 2-bit pairs, shift right by 64 - 2 k (0 at k = 32).
// ---- tiles: the shared grid of fasta_tiles.h; a record's start positions are its len - k + 1 k-mer starts, none when it is shorter
// than k (sketch_positions).
constexpr uint32_t SKETCH_TILE = SCAN_TILE, SKETCH_THREADS = SCAN_THREADS, SKETCH_PER = SCAN_PER;   // 16 positions per lane: a 32-bit code word, a 16-bit invalid mask
constexpr uint64_t SKETCH_ROWS_FIRST = 65536;                        // rows of the entry point's first row buffer; it grows to the cursor's count
constexpr uint64_t SKETCH_SEED = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t sketch_positions(uint64_t len, uint32_t k) { return len >= k ? len - k + 1 : 0; }

// MurmurHash3's 64-bit finaliser
__host__ __device__ __forceinline__ uint64_t sketch_fmix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// the 32 two-bit pairs of x in reverse order
__host__ __device__ __forceinline__ uint64_t sketch_reverse_pairs(uint64_t x) {
    x = __builtin_bswap64(x);
    x = ((x & 0x0f0f0f0f0f0f0f0full) << 4) | ((x >> 4) & 0x0f0f0f0f0f0f0f0full);
    return ((x & 0x3333333333333333ull) << 2) | ((x >> 2) & 0x3333333333333333ull);
}

// fw (2 k bits, the first base on top) -> the hash of the canonical k-mer
__host__ __device__ __forceinline__ uint64_t sketch_hash(uint64_t fw, uint32_t k) {
    const uint64_t rc = sketch_reverse_pairs(~fw) >> (64 - 2 * k);  // (the complement's 64 - 2 k high pairs — all ones — leave at the bottom)
    return sketch_fmix64((fw < rc ? fw : rc) ^ SKETCH_SEED);
}

// the code of a byte, 4 for an invalid one
__host__ __device__ __forceinline__ uint32_t sketch_code(uint8_t b) {
    const uint8_t f = b | 0x20;
    return f == 'a' ? 0u : f == 'c' ? 1u : f == 'g' ? 2u : (f == 't' || f == 'u') ? 3u : 4u;
}

// the first step: the vector at address v (a multiple of 16, anywhere) -> codes | bad << 32 for record `rec`. 0xffff << 32 — all
// invalid, nothing read — when none of its positions lies in the record
__device__ __forceinline__ uint64_t sketch_pack(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec rec, uintptr_t v) {
    const uintptr_t lo = (uintptr_t) seq, hi = lo + seqBytes;
    const int64_t t0 = (int64_t) v - (int64_t) (lo + rec.off);     // the vector's first position in the record
    if (t0 + (int64_t) SKETCH_PER <= 0 || t0 >= (int64_t) rec.len) return (uint64_t) 0xffff << 32;
    ScanVec x = {{0, 0, 0, 0}};
    if (v >= lo && v + 16 <= hi) x = *(const ScanVec *) v;
    else
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (v + j >= lo && v + j < hi) x.w[j >> 2] |= (uint32_t) *(const uint8_t *) (v + j) << (8 * (j & 3));
    uint32_t codes = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < SKETCH_PER; j++) {
        const int64_t t = t0 + j;
        const uint32_t c = sketch_code((uint8_t) (x.w[j >> 2] >> (8 * (j & 3))));
        if (t < 0 || t >= (int64_t) rec.len || c > 3) bad |= 1u << j;
        else codes |= c << (30 - 2 * j);
    }
    return (uint64_t) codes | (uint64_t) bad << 32;
}

// the second step: the lane's packed word and those of the two vectors behind it -> the hashes of the k-mers that start at the lane's
// 16 positions; bit j of the result: position j starts a valid k-mer (h[j] is set for those alone)
__host__ __device__ __forceinline__ uint32_t sketch_lane_hashes(uint64_t own, uint64_t next1, uint64_t next2, uint32_t k, uint64_t h[SKETCH_PER]) {
    const uint64_t top = (own & 0xffffffffull) << 32 | (next1 & 0xffffffffull);                 // positions 0..31, position 0 on top
    const uint32_t behind = (uint32_t) next2;                                                    // positions 32..47
    const uint64_t bad = (own >> 32 & 0xffff) | (next1 >> 32 & 0xffff) << 16 | (next2 >> 32 & 0xffff) << 32;
    const uint64_t span = ((uint64_t) 1 << k) - 1;                                               // k <= 32: the k positions from j on
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t j = 0; j < SKETCH_PER; j++) {
        if ((bad >> j) & span) continue;
        const uint64_t W = j ? (top << (2 * j)) | (uint64_t) (behind >> (32 - 2 * j)) : top;
        h[j] = sketch_hash(W >> (64 - 2 * k), k);
        valid |= 1u << j;
    }
    return valid;
}

// ---- pairs: pair q of all i < j of n groups in row-major order — row i holds n - 1 - i pairs and starts at i (2 n - i - 1) / 2
__host__ __device__ __forceinline__ uint64_t sketch_pair_row_start(uint64_t i, uint64_t n) { return i * (2 * n - i - 1) / 2; }
__host__ __device__ __forceinline__ void sketch_pair_of(uint64_t q, uint32_t n, uint32_t &i, uint32_t &j) {
    uint32_t lo = 0, hi = n - 1;                                     // rowStart(lo) <= q < rowStart(hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sketch_pair_row_start(mid, n) <= q) lo = mid; else hi = mid;
    }
    i = lo;
    j = lo + 1 + (uint32_t) (q - sketch_pair_row_start(lo, n));
}

// is x in the strictly ascending list[0, n)?
__host__ __device__ __forceinline__ bool sketch_holds(const uint64_t *__restrict__ list, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;                                         // the first element >= x lies in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (list[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && list[lo] == x;
}
