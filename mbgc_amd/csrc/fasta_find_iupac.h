// The scan of `mbgc-hip f --iupac` (included by fasta_input.hip, inside namespace fa, behind fasta_find.h whose staging step it shares):
// the tables mbgc_fasta_find_iupac_dev makes on the host and the step of one lane. Kept free of HIP calls so that the same text
// compiles as plain C++: tests/fasta_find_iupac_emu.cpp runs it tile by tile and lane by lane on the CPU under AddressSanitizer. The
// staging buffer in LDS, the bitmap's copy there, the barrier and the atomic cursor of the hit buffer stay in fasta_input.hip
// (k_fa_find_iupac).
// ---- the rule (include/mbgc_fasta.h): a pattern letter is a SET of bases, a 4-bit mask (A 1, C 2, G 4, T 8; R = A | G, ..., N = 15); a
// text byte has a base only if it is one of acgtuACGTU (u as T) and is then the one-hot mask of that base, every other byte — N and the
// ambiguity letters in the text included — is 0. Position j matches iff (mask_j & onehot(text_j)) != 0. A hit is (record r, pattern q,
// position p, mismatches d): p + len(q) <= the record's length, d = the positions that do not match, d <= K.
// ---- seeds: a pattern of L letters is cut into K + 1 disjoint segments, segment j at j * (L / (K + 1)), L / (K + 1) >= IUPAC_GRAM
// letters each, and an alignment with at most K mismatches leaves one segment free of them (pigeonhole). A segment's seed is its WINDOW:
// the IUPAC_GRAM letters inside it whose expansion — the product of the letters' set sizes — is smallest, the leftmost on a tie. The host
// expands the window into every concrete ACGT gram it stands for (IUPAC_MAX_EXPAND at most: a pattern with a segment whose best window
// is wider is refused) and packs each into 16 bits, base i in bits [2 i, 2 i + 2). Every (pattern, segment, expansion) is a row; the rows
// that share a gram are one chain, gramStart[g] .. gramStart[g + 1] of the row table, and the grams that have a chain are the set bits
// of a bitmap of 65536 bits — 8 KiB, in LDS whatever the number of patterns and expansions.
// ---- exactly once: every text position t with t + IUPAC_GRAM <= the record's length is looked at once, by the lane that owns it. A
// text gram that holds a byte without a base is no gram at all and matches no window, as such a byte matches no letter. Otherwise the
// lane tests the gram's bit and only on a set bit reads the chain. Row (q, j) proposes the start t - windowOff_j; the lane counts the
// mismatches of the whole pattern there and reports the alignment only if no segment j' < j of q has its window matching, by the rule
// above, at its own place start + windowOff_j'. The text gram under a matching window is one of that window's expansions and equals
// exactly one of them (the expansions of a window are distinct grams), so the lane that owns that place finds exactly one row (q, j')
// in its chain and reports the alignment there. So every hit is reported exactly once, by the first segment whose window matches —
// there is one, the segment without a mismatch has it — and no pass removes duplicates afterwards.
// ---- tiles: the shared grid of fasta_tiles.h, staged by find_stage_step; the start positions of a record are those of its grams
// (find_positions). A staged byte outside the record is never looked at: a position counts only when its whole gram lies inside the
// record, and a proposed start only when the whole pattern does.
constexpr uint32_t IUPAC_GRAM = FIND_GRAM, IUPAC_MAX_EXPAND = 256, IUPAC_GRAMS = 1u << (2 * IUPAC_GRAM), IUPAC_BITMAP_WORDS = IUPAC_GRAMS / 32;
constexpr uint32_t IUPAC_WALKED = 16;                                 // the rows-walked counter's word behind the hit cursor: 128 bytes on, another cache line
static_assert(IUPAC_GRAM == 8 && FIND_PER + IUPAC_GRAM - 1 <= 32, "a gram is 16 bits; a lane's positions and the grams' tails are two vectors");

struct IupacRow { uint32_t pat; uint16_t off, j; };                   // segment j of the caller's pattern `pat`, its window `off` letters into the pattern
struct IupacPat { uint64_t off; uint32_t len; uint16_t win[FIND_MAX_K + 1]; };     // masks [off, off + len) of the table's blob; win[j]: segment j's window

// the set of a pattern letter, either case, as a mask; 0: not a letter of the table
__host__ __device__ __forceinline__ uint8_t iupac_mask(uint8_t c) {
    switch (c | 0x20) {
        case 'a': return 1; case 'c': return 2; case 'g': return 4; case 't': case 'u': return 8;
        case 'r': return 1 | 4; case 'y': return 2 | 8; case 's': return 2 | 4; case 'w': return 1 | 8; case 'k': return 4 | 8; case 'm': return 1 | 2;
        case 'b': return 2 | 4 | 8; case 'd': return 1 | 4 | 8; case 'h': return 1 | 2 | 8; case 'v': return 1 | 2 | 4; case 'n': return 15;
    }
    return 0;
}

// a text byte -> its base's code (A 0, C 1, G 2, T and U 3) in bits 0..1 and bit 2 set, or 0 for a byte without a base: two constants
// indexed by the letter (bit 0x20 is the case; 0x41 and 0x61 alone become 'a')
__host__ __device__ __forceinline__ uint32_t iupac_code(uint8_t b) {
    const uint32_t i = (uint32_t) (b | 0x20) - 'a';
    constexpr uint32_t HAS = 1u << ('a' - 'a') | 1u << ('c' - 'a') | 1u << ('g' - 'a') | 1u << ('t' - 'a') | 1u << ('u' - 'a');
    constexpr uint64_t CODE = 1ull << 2 * ('c' - 'a') | 2ull << 2 * ('g' - 'a') | 3ull << 2 * ('t' - 'a') | 3ull << 2 * ('u' - 'a');
    const uint32_t s = i < 26 ? i : 25;                              // ('z' has no base)
    return ((HAS >> s) & 1u) << 2 | (uint32_t) ((CODE >> (2 * s)) & 3u);
}
__host__ __device__ __forceinline__ uint32_t iupac_onehot(uint8_t b) { const uint32_t c = iupac_code(b); return (c >> 2) << (c & 3u); }

// does the pattern of masks pm stand at txt with at most K positions that do not match? -> their number, K + 1 when there are more
__device__ __forceinline__ uint32_t iupac_count(const uint8_t *__restrict__ txt, const uint8_t *__restrict__ pm, uint32_t len, uint32_t K) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < len && d <= K; i++) d += (pm[i] & iupac_onehot(txt[i])) == 0;
    return d;
}

// the lane's step, behind the barrier: lane `lane` (of FIND_THREADS) owns the FIND_PER positions from address tileAddr + 16 lane on;
// emit(pos, pattern, mismatches) is called once per hit of record `rec` this lane reports. -> the rows the lane walked
template <class Emit>
__device__ __forceinline__ uint32_t iupac_lane_step(const uint8_t *__restrict__ seq, const ScanRec rec, uintptr_t tileAddr, uint32_t lane, const uint8_t *stage,
                                                    const uint32_t *bitmap, const uint32_t *__restrict__ gramStart, const IupacRow *__restrict__ rows,
                                                    const IupacPat *__restrict__ pats, const uint8_t *__restrict__ masks, uint32_t K, Emit &&emit) {
    const uint8_t *text = seq + rec.off;
    // the lane's first position in the record; in front of the record in its first tile only
    const int64_t t0 = (int64_t) (tileAddr + 16u * lane) - (int64_t) (uintptr_t) text;
    if (t0 + (int64_t) FIND_PER <= 0 || t0 + (int64_t) IUPAC_GRAM > (int64_t) rec.len) return 0;
    const ScanVec a = *(const ScanVec *) (stage + 16u * lane), b = *(const ScanVec *) (stage + 16u * lane + 16);
    const uint32_t w[8] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]};
    // the codes of the lane's 16 + 7 bytes, byte i in bits [2 i, 2 i + 2), and the bytes without a base, bit i
    uint64_t codes = 0;
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t i = 0; i < FIND_PER + IUPAC_GRAM - 1; i++) {
        const uint32_t c = iupac_code((uint8_t) (w[i >> 2] >> (8 * (i & 3))));
        codes |= (uint64_t) (c & 3u) << (2 * i);
        bad |= ((c >> 2) ^ 1u) << i;
    }
    uint32_t walked = 0;
#pragma unroll
    for (uint32_t k = 0; k < FIND_PER; k++) {
        const int64_t t = t0 + k;
        if (t < 0 || t + (int64_t) IUPAC_GRAM > (int64_t) rec.len || ((bad >> k) & 0xffu)) continue;
        const uint32_t g = (uint32_t) (codes >> (2 * k)) & (IUPAC_GRAMS - 1u);
        if (!((bitmap[g >> 5] >> (g & 31u)) & 1u)) continue;
        const uint32_t first = gramStart[g], end = gramStart[g + 1];
        walked += end - first;
        for (uint32_t c = first; c < end; c++) {
            const IupacRow row = rows[c];
            const IupacPat P = pats[row.pat];
            if (t < (int64_t) row.off || (uint64_t) (t - row.off) + P.len > rec.len) continue;        // the pattern would not lie inside the record
            const uint64_t start = (uint64_t) (t - row.off);
            const uint8_t *txt = text + start, *pm = masks + P.off;
            const uint32_t d = iupac_count(txt, pm, P.len, K);
            if (d > K) continue;
            bool earlier = false;                                    // a matching window in front of this one: its own lane reports the alignment
            for (uint32_t j = 0; j < row.j && !earlier; j++) earlier = iupac_count(txt + P.win[j], pm + P.win[j], IUPAC_GRAM, 0) == 0;
            if (!earlier) emit(start, row.pat, d);
        }
    }
    return walked;
}

// The host's half: the caller's patterns (back to back, patOff[npat + 1], letters of the table only, IUPAC_GRAM (K + 1) <= length <=
// FIND_MAX_LEN) -> their masks, the windows, the rows in chains by gram and the bitmap. The same pattern given twice is two rows of
// every chain it is in: every index is reported. -> true, or false with the first pattern and segment whose best window expands to
// badGrams > IUPAC_MAX_EXPAND grams (T is then unfinished)
struct IupacTable {
    uint32_t shortest = 0;
    std::vector<uint32_t> bitmap, gramStart;                          // IUPAC_BITMAP_WORDS words; IUPAC_GRAMS + 1 prefix sums
    std::vector<IupacRow> rows; std::vector<IupacPat> pats; std::vector<uint8_t> masks;
};
inline bool iupac_build_table(const uint8_t *patterns, const uint64_t *patOff, uint64_t npat, uint32_t K, IupacTable &T, uint64_t &badPat, uint32_t &badSeg, uint32_t &badGrams) {
    T.rows.clear(); T.pats.clear();
    T.shortest = FIND_MAX_LEN;
    T.masks.resize(patOff[npat] - patOff[0]);
    struct Row { uint32_t gram; IupacRow row; };
    std::vector<Row> rows;
    for (uint64_t q = 0; q < npat; q++) {
        const uint32_t len = (uint32_t) (patOff[q + 1] - patOff[q]), step = len / (K + 1);
        const uint64_t at = patOff[q] - patOff[0];
        for (uint32_t i = 0; i < len; i++) T.masks[at + i] = iupac_mask(patterns[patOff[q] + i]);
        IupacPat P = {at, len, {0, 0, 0, 0}};
        T.shortest = std::min(T.shortest, len);
        for (uint32_t j = 0; j <= K; j++) {
            const uint8_t *seg = T.masks.data() + at + j * step;
            uint32_t best = 0, bestGrams = 0;
            for (uint32_t wnd = 0; wnd + IUPAC_GRAM <= step; wnd++) {
                uint32_t grams = 1;
                for (uint32_t i = 0; i < IUPAC_GRAM; i++) grams *= (uint32_t) __builtin_popcount(seg[wnd + i]);
                if (wnd == 0 || grams < bestGrams) { best = wnd; bestGrams = grams; }
            }
            if (bestGrams > IUPAC_MAX_EXPAND) { badPat = q; badSeg = j; badGrams = bestGrams; return false; }
            P.win[j] = (uint16_t) (j * step + best);
            // every choice of one base per letter: an odometer over the window's letters
            const uint8_t *wm = seg + best;
            uint32_t pick[IUPAC_GRAM];
            for (uint32_t i = 0; i < IUPAC_GRAM; i++) pick[i] = (uint32_t) __builtin_ctz(wm[i]);
            for (;;) {
                uint32_t gram = 0;
                for (uint32_t i = 0; i < IUPAC_GRAM; i++) gram |= pick[i] << (2 * i);
                rows.push_back(Row{gram, IupacRow{(uint32_t) q, P.win[j], (uint16_t) j}});
                uint32_t i = 0;
                for (; i < IUPAC_GRAM; i++) {
                    uint32_t next = pick[i] + 1;
                    while (next < 4 && !((wm[i] >> next) & 1)) next++;
                    if (next < 4) { pick[i] = next; break; }
                    pick[i] = (uint32_t) __builtin_ctz(wm[i]);
                }
                if (i == IUPAC_GRAM) break;
            }
        }
        T.pats.push_back(P);
    }
    std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
        if (a.gram != b.gram) return a.gram < b.gram;
        if (a.row.pat != b.row.pat) return a.row.pat < b.row.pat;
        return a.row.j < b.row.j;
    });
    T.bitmap.assign(IUPAC_BITMAP_WORDS, 0);
    T.gramStart.assign(IUPAC_GRAMS + 1, 0);
    T.rows.reserve(rows.size());
    for (const Row &r : rows) { T.bitmap[r.gram >> 5] |= 1u << (r.gram & 31u); T.gramStart[r.gram + 1]++; T.rows.push_back(r.row); }
    for (uint32_t g = 0; g < IUPAC_GRAMS; g++) T.gramStart[g + 1] += T.gramStart[g];
    return true;
}
