// The scan of `mbgc-hip m` (included by fasta_input.hip, inside namespace fa, behind fasta_sketch.h, whose grid, packing and three-lane
// window it uses): is the canonical k-mer at a text position a member of the queries' key set? Kept free of HIP calls so that the same
// text compiles as plain C++: tests/fasta_screen_emu.cpp runs the steps tile by tile and lane by lane on the CPU under AddressSanitizer,
// the wave's shuffles emulated by arrays. The shuffles, the ballot, the atomic cursor of the row buffer, the sorts and the compaction
// stay in fasta_input.hip (k_fa_screen, k_fa_screen_flag, k_fa_screen_compact).
// ---- the key of a k-mer (the contract of include/mbgc_fasta.h): canon = min(fw, rc) of mbgc_fasta_sketch_dev, the 2-bit packed word
// itself. No hash enters a result; h = fmix64(canon ^ SKETCH_SEED) only says WHERE to look.
// ---- two levels. (1) A filter of 2^17 bits, 16 KiB, a copy in every block's LDS: bit h >> 47. (2) A table in global memory, open
// addressing, linear probing, a power-of-two slot count >= 2 nkeys (at most 2^25): slot h & (slots - 1) on. A slot holds a key INDEX + 1,
// 0 when free — so no key value is a sentinel and k = 32, whose keys use all 64 bits, is no special case —, and a find is confirmed
// against keys[]. The filter takes the hash's top 17 bits, the slot at most its low 25: keys that crowd one stretch of the table do not
// share a filter bit for that reason. 16 KiB keeps LDS out of the occupancy question: the registers bind (114 VGPRs: four blocks of four
// waves per CU, 64 KiB of the CU's 160 KiB), and LDS would not bind at eight blocks either; 32 KiB would fit today's four blocks too, but
// would become the limit at five, and all it buys is 0.6 % instead of 1.1 % of the positions sent to the table for one gene. n keys set
// 2^17 (1 - exp(-n / 2^17)) bits: 1.1 % at 1 500 keys, 53 % at 100 000, 99.97 % at 2^20 — from about a million keys on everything goes
// through the table. The lanes of a wave read the filter at unrelated words: the conflicts are those of 64 random
// addresses over 32 banks, and no layout changes that.
// ---- a lane: its 16 positions' canonical words (screen_lane_canons: sketch_lane_hashes's window without the hash), then per position
// screen_first — the filter, and on a set bit the table's first slot —, and screen_confirm — the key behind that slot compared, the
// probe walked on when it is another's. The kernel calls screen_first for all 16 positions before it looks at one answer, so that the
// table's loads travel together.
constexpr uint32_t SCREEN_THREADS = SCAN_THREADS, SCREEN_PER = SCAN_PER;
constexpr uint32_t SCREEN_FILTER_LOG = 17, SCREEN_FILTER_WORDS = 1u << (SCREEN_FILTER_LOG - 5);     // 4096 words of 32 bits
constexpr uint32_t SCREEN_KEYS_LOG = 24;                             // at most 2^24 keys in one call: at most 2^25 slots
constexpr uint64_t SCREEN_MAX_KEYS = (uint64_t) 1 << SCREEN_KEYS_LOG;
constexpr uint64_t SCREEN_ROWS_FIRST = 65536;                        // rows of the entry point's first row buffer; it grows to the cursor's count
static_assert(SCREEN_FILTER_LOG + SCREEN_KEYS_LOG + 1 <= 64, "the filter's bits and the slot's bits are different bits of the hash");
static_assert(SCREEN_FILTER_WORDS % 4 == 0, "the filter is copied to LDS in 16-byte vectors");

__host__ __device__ __forceinline__ uint64_t screen_hash(uint64_t canon) { return sketch_fmix64(canon ^ SKETCH_SEED); }

// the slots of a table of nkeys keys: the power of two >= 2 nkeys, 2 at least
__host__ __device__ __forceinline__ uint64_t screen_slots(uint64_t nkeys) {
    uint64_t s = 2;
    while (s < 2 * nkeys) s <<= 1;
    return s;
}

// fw (2 k bits, the first base on top) -> the canonical word
__host__ __device__ __forceinline__ uint64_t screen_canon(uint64_t fw, uint32_t k) {
    const uint64_t rc = sketch_reverse_pairs(~fw) >> (64 - 2 * k);
    return fw < rc ? fw : rc;
}

// is the filter's bit of hash h set?
__host__ __device__ __forceinline__ bool screen_filter_holds(const uint32_t *__restrict__ filter, uint64_t h) {
    const uint32_t bit = (uint32_t) (h >> (64 - SCREEN_FILTER_LOG));
    return (filter[bit >> 5] >> (bit & 31)) & 1u;
}

// the lane's packed word and those of the two vectors behind it -> the canonical words of the k-mers that start at the lane's 16
// positions; bit j of the result: position j starts a valid k-mer (c[j] is set for those alone). The window is sketch_lane_hashes's
__host__ __device__ __forceinline__ uint32_t screen_lane_canons(uint64_t own, uint64_t next1, uint64_t next2, uint32_t k, uint64_t c[SCREEN_PER]) {
    const uint64_t top = (own & 0xffffffffull) << 32 | (next1 & 0xffffffffull);
    const uint32_t behind = (uint32_t) next2;
    const uint64_t bad = (own >> 32 & 0xffff) | (next1 >> 32 & 0xffff) << 16 | (next2 >> 32 & 0xffff) << 32;
    const uint64_t span = ((uint64_t) 1 << k) - 1;
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCREEN_PER; j++) {
        if ((bad >> j) & span) continue;
        const uint64_t W = j ? (top << (2 * j)) | (uint64_t) (behind >> (32 - 2 * j)) : top;
        c[j] = screen_canon(W >> (64 - 2 * k), k);
        valid |= 1u << j;
    }
    return valid;
}

// the first step of a position: false when the filter says the word is no key; else passed, and e = what the word's first slot holds
__host__ __device__ __forceinline__ bool screen_first(const uint32_t *__restrict__ filter, const uint32_t *__restrict__ table, uint32_t slotMask, uint64_t canon, uint32_t &e) {
    const uint64_t h = screen_hash(canon);
    if (!screen_filter_holds(filter, h)) return false;
    e = table[(uint32_t) h & slotMask];
    return true;
}

// the probe from `slot` on: the index + 1 of the key that equals canon, 0 at the first free slot; steps: the slots looked at
__host__ __device__ __forceinline__ uint32_t screen_probe(const uint32_t *__restrict__ table, uint32_t slotMask, const uint64_t *__restrict__ keys, uint64_t canon, uint32_t slot,
                                                          uint32_t &steps) {
    for (;;) {                                                       // (half of the slots are free: the walk ends)
        const uint32_t e = table[slot];
        steps++;
        if (e == 0 || keys[e - 1] == canon) return e;
        slot = (slot + 1) & slotMask;
    }
}

// the second step: e is the first slot's entry, behind is the key it names (read by the caller, unused when e is 0) -> the index + 1 of
// canon among the keys, 0 when it is none; steps counts the first slot too
__host__ __device__ __forceinline__ uint32_t screen_confirm(const uint32_t *__restrict__ table, uint32_t slotMask, const uint64_t *__restrict__ keys, uint64_t canon, uint32_t e,
                                                            uint64_t behind, uint32_t &steps) {
    steps++;
    if (e == 0 || behind == canon) return e;
    return screen_probe(table, slotMask, keys, canon, ((uint32_t) screen_hash(canon) + 1) & slotMask, steps);
}

// ---- the host's builders (the entry point and the emulation use these very functions)
// the filter of keys[0, nkeys) into filter[0, SCREEN_FILTER_WORDS) -> the bits set
__host__ inline uint64_t screen_build_filter(const uint64_t *keys, uint64_t nkeys, uint32_t *filter) {
    for (uint32_t w = 0; w < SCREEN_FILTER_WORDS; w++) filter[w] = 0;
    uint64_t set = 0;
    for (uint64_t i = 0; i < nkeys; i++) {
        const uint32_t bit = (uint32_t) (screen_hash(keys[i]) >> (64 - SCREEN_FILTER_LOG));
        set += !((filter[bit >> 5] >> (bit & 31)) & 1u);
        filter[bit >> 5] |= 1u << (bit & 31);
    }
    return set;
}

// the table of the DISTINCT keys[0, nkeys) into table[0, slots), slots = screen_slots(nkeys) -> the longest walk of an insertion, in slots
__host__ inline uint32_t screen_build_table(const uint64_t *keys, uint64_t nkeys, uint32_t *table, uint64_t slots) {
    const uint32_t mask = (uint32_t) (slots - 1);
    for (uint64_t s = 0; s < slots; s++) table[s] = 0;
    uint32_t longest = 0;
    for (uint64_t i = 0; i < nkeys; i++) {
        uint32_t slot = (uint32_t) screen_hash(keys[i]) & mask, walked = 1;
        while (table[slot]) { slot = (slot + 1) & mask; walked++; }
        table[slot] = (uint32_t) i + 1;
        if (walked > longest) longest = walked;
    }
    return longest;
}
