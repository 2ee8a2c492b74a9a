// The header match of `mbgc-hip d --select-seq` (included by fasta_input.hip, inside namespace fa): the pattern table
// mbgc_fasta_match_headers_dev makes on the host, and the two steps of one lane. Kept free of HIP calls so that the same text compiles
// as plain C++: tests/fasta_select_emu.cpp runs the steps lane by lane on the CPU under AddressSanitizer. The staging buffer in LDS,
// the barrier, the ballot and the atomic of a wave stay in fasta_input.hip (k_fa_match_headers).
// ---- record r is chosen iff its header contains a pattern as a byte substring. What a header byte costs does not grow with the
// number of patterns: every pattern is at least m = min(8, the shortest pattern) bytes long, so a match at position p shows in the m
// bytes at p — the gram. The host keys an open-addressing table by the patterns' first m bytes; the distinct patterns that share a key
// are one chain (shortest first). A wave takes one header, SEL_TILE positions at a time: the tile's bytes and the m - 1 behind them
// are staged in LDS, each lane packs the gram at its position, probes the table (half empty at most: a miss ends at once, almost
// always at the first slot) and, on a hit, walks the key's chain, comparing what lies behind the gram with the header in memory.
// Only positions p with p + m <= the header's length are looked at, and a pattern is compared only where it ends inside the header:
// no byte outside the record's own header is read, neither the line feed behind it nor the next header.
struct SelSlot {
    uint64_t key;             // the first m bytes of the chain's patterns, byte j in bits [8 j, 8 j + 8)
    uint32_t first, count;    // the chain: rows [first, first + count) of the pattern table; count == 0: an empty slot
};
struct SelPat { uint64_t off, len; };                                // a distinct pattern: bytes [off, off + len) of the caller's patterns
constexpr uint32_t SEL_TILE = 64, SEL_GRAM = 8, SEL_STAGE = SEL_TILE + SEL_GRAM - 1;

__host__ __device__ __forceinline__ uint32_t sel_hash(uint64_t key, uint32_t bits) { return (uint32_t) ((key * 0x9E3779B97F4A7C15ull) >> (64 - bits)); }

// the first step of lane `lane` of the tile that starts at position `base` of a header hdr[0, len): its share of the bytes
// [base, min(len, base + SEL_STAGE)) goes to stage[0, ...)
__device__ __forceinline__ void sel_stage_step(const uint8_t *__restrict__ hdr, uint64_t len, uint64_t base, uint32_t lane, uint32_t m, uint8_t *stage) {
    if (base + lane < len) stage[lane] = hdr[base + lane];
    if (lane + 1 < m && base + SEL_TILE + lane < len) stage[SEL_TILE + lane] = hdr[base + SEL_TILE + lane];
}

// the second step, behind a barrier: does a pattern start at position base + lane of the header?
__device__ __forceinline__ bool sel_lane_step(const uint8_t *__restrict__ hdr, uint64_t len, uint64_t base, uint32_t lane, uint32_t m, const uint8_t *stage,
                                              const SelSlot *__restrict__ slots, uint32_t bits, const SelPat *__restrict__ pats,
                                              const uint8_t *__restrict__ patBytes) {
    const uint64_t p = base + lane;
    if (p + m > len) return false;
    uint64_t key = 0;
    for (uint32_t j = 0; j < m; j++) key |= (uint64_t) stage[lane + j] << (8 * j);
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t s = sel_hash(key, bits);; s = (s + 1) & mask) {
        const SelSlot e = slots[s];
        if (e.count == 0) return false;
        if (e.key != key) continue;
        const uint64_t room = len - p;
        for (uint32_t c = e.first; c < e.first + e.count; c++) {
            const SelPat pt = pats[c];
            if (pt.len > room) return false;                          // (shortest first: the rest of the chain is longer still)
            uint64_t j = m;                                          // the first m bytes are the key's
            while (j < pt.len && hdr[p + j] == patBytes[pt.off + j]) j++;
            if (j == pt.len) return true;
        }
        return false;
    }
}

// The host's half: the caller's patterns (back to back, patOff[npat + 1], each of them non-empty) -> m, the distinct patterns in
// chains and the slots (1 << bits of them, at least twice the chains).
struct SelTable { uint32_t m = 0, bits = 0; std::vector<SelSlot> slots; std::vector<SelPat> pats; };
inline void sel_build_table(const uint8_t *patterns, const uint64_t *patOff, uint64_t npat, SelTable &T) {
    T.slots.clear(); T.pats.clear();
    uint64_t shortest = SEL_GRAM;
    for (uint64_t k = 0; k < npat; k++) shortest = std::min(shortest, patOff[k + 1] - patOff[k]);
    T.m = (uint32_t) shortest;
    struct Row { uint64_t key, off, len; };
    std::vector<Row> rows(npat);
    for (uint64_t k = 0; k < npat; k++) {
        rows[k] = Row{0, patOff[k], patOff[k + 1] - patOff[k]};
        for (uint32_t j = 0; j < T.m; j++) rows[k].key |= (uint64_t) patterns[patOff[k] + j] << (8 * j);
    }
    const auto cmp = [patterns](const Row &a, const Row &b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.len != b.len) return a.len < b.len;
        return memcmp(patterns + a.off, patterns + b.off, a.len) < 0;
    };
    std::sort(rows.begin(), rows.end(), cmp);
    std::vector<uint64_t> keys;                                      // per distinct pattern
    uint64_t chains = 0;
    for (uint64_t k = 0; k < npat; k++) {
        if (k && !cmp(rows[k - 1], rows[k])) continue;               // the same pattern again
        if (keys.empty() || rows[k].key != keys.back()) chains++;
        T.pats.push_back(SelPat{rows[k].off, rows[k].len});
        keys.push_back(rows[k].key);
    }
    T.bits = 6;
    while ((1ull << T.bits) < 2 * chains) T.bits++;
    T.slots.assign((size_t) 1 << T.bits, SelSlot{0, 0, 0});
    const uint32_t mask = (1u << T.bits) - 1u;
    for (size_t c = 0; c < T.pats.size();) {
        size_t e = c + 1;
        while (e < T.pats.size() && keys[e] == keys[c]) e++;
        uint32_t s = sel_hash(keys[c], T.bits);
        while (T.slots[s].count) s = (s + 1) & mask;
        T.slots[s] = SelSlot{keys[c], (uint32_t) c, (uint32_t) (e - c)};
        c = e;
    }
}
