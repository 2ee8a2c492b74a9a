// The comparison of the validate command (included by fasta_input.hip, inside namespace fa, after CHUNK / THREADS / PER): the piece
// table and the owner table mbgc_fasta_compare_dev makes on the host, and the step of one lane. Kept free of HIP calls so that the
// same text compiles as plain C++: tests/fasta_compare_emu.cpp runs the step lane by lane on the CPU under AddressSanitizer. The
// ballot and the atomic of a wave stay in fasta_input.hip (k_fa_compare).
// ---- mbgc_fasta_compare_dev: pieces a[aOff, aOff + len) against b[bOff, bOff + len), the first differing offset of each. The work
// unit is a tile of 4096 bytes, 16 per lane step, laid over the pieces back to back — every piece led in by the bytes its a side
// stands behind a 16-byte boundary and padded to whole steps, so that a step belongs to one piece, every whole step reads its a
// side with one aligned 16-byte vector load, and the b side is the one that goes unaligned. The first and the last step of a
// piece, where they are partial, walk byte by byte. A tile finds its pieces through an owner table (tile -> first piece that touches
// it) made on the host; a lane searches only between its tile's owner and the next tile's. Pieces of no bytes have no row.
struct CmpPiece {
    uint64_t vOff;            // where the piece's steps start in the tiled range (a multiple of 16)
    uint64_t aOff, bOff, len; // len > 0
    uint32_t mis;             // bytes a + aOff stands behind a 16-byte boundary: step s covers the piece's bytes [16 s - mis, 16 s - mis + 16)
    uint32_t slot;
};
constexpr uint64_t CMP_NONE = ~0ull;

__device__ __forceinline__ uint32_t cmp_find(const CmpPiece *__restrict__ P, uint32_t lo, uint32_t hi, uint64_t v) {   // the last piece of [lo, hi] that starts at or before v
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (P[mid].vOff <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the step of lane `lane` of tile `tile`: the smallest offset in the step's piece at which a and b differ, among the step's bytes,
// or CMP_NONE; *piece = the piece's row (also when nothing differs; untouched when the step lies behind the last piece)
__device__ __forceinline__ uint64_t cmp_lane_step(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const CmpPiece *__restrict__ P,
                                                  const uint32_t *__restrict__ owner, uint32_t tile, uint32_t lane, uint64_t total, uint32_t *piece) {
    const uint64_t vs = (uint64_t) tile * CHUNK + (uint64_t) lane * PER;
    if (vs >= total) return CMP_NONE;
    const uint32_t r = cmp_find(P, owner[tile], owner[tile + 1], vs);
    *piece = r;
    const CmpPiece pc = P[r];
    const uint64_t s = vs - pc.vOff;                                  // the step's first byte, counted from the piece's 16-byte boundary
    if (s >= pc.mis && s - pc.mis + PER <= pc.len) {
        const uint64_t o = s - pc.mis;
        uint4 va, vb;
        va = *(const uint4 *) (a + pc.aOff + o);                      // 16-byte aligned by the table's construction
        memcpy(&vb, b + pc.bOff + o, PER);
        // all four words are XORed before anything is tested: both sides' 16 bytes are loaded whole, in one round trip each, not the
        // second half behind a branch on the first
        const uint32_t x[4] = {va.x ^ vb.x, va.y ^ vb.y, va.z ^ vb.z, va.w ^ vb.w};
        if (!(x[0] | x[1] | x[2] | x[3])) return CMP_NONE;
        const uint64_t x0 = x[0] | (uint64_t) x[1] << 32, x1 = x[2] | (uint64_t) x[3] << 32;
        return x0 ? o + (uint64_t) (__builtin_ctzll(x0) >> 3) : o + 8 + (uint64_t) (__builtin_ctzll(x1) >> 3);
    }
    const uint64_t from = s >= pc.mis ? s - pc.mis : 0;               // the piece's head and tail
    const uint64_t to = s + PER - pc.mis < pc.len ? s + PER - pc.mis : pc.len;
    for (uint64_t o = from; o < to; o++)
        if (a[pc.aOff + o] != b[pc.bOff + o]) return o;
    return CMP_NONE;
}

// The host's half: the caller's pieces -> table (the pieces that hold bytes, in order, then a sentinel at the tiled range's end) and
// the tiles' owners (ntiles + 1 entries). aBase: the address of a's first byte (its low four bits are what matters). Returns the
// tiled range's size.
struct CmpIn { uint64_t aOff, bOff, len; uint32_t slot; };
inline uint64_t cmp_build_table(const CmpIn *pieces, uint64_t npieces, uint64_t aBase, std::vector<CmpPiece> &table) {
    table.clear();
    uint64_t total = 0;
    for (uint64_t k = 0; k < npieces; k++) {
        const CmpIn &x = pieces[k];
        if (x.len == 0) continue;
        const uint32_t mis = (uint32_t) ((aBase + x.aOff) & (uint64_t) (PER - 1));
        table.push_back(CmpPiece{total, x.aOff, x.bOff, x.len, mis, x.slot});
        total += (mis + x.len + PER - 1) / PER * PER;
    }
    table.push_back(CmpPiece{total, 0, 0, 0, 0, 0});
    return total;
}
inline void cmp_build_owner(const std::vector<CmpPiece> &table, uint32_t ntiles, std::vector<uint32_t> &owner) {
    owner.resize((size_t) ntiles + 1);
    uint32_t r = 0;
    for (uint32_t t = 0; t < ntiles; t++) {
        while (table[r + 1].vOff <= (uint64_t) t * CHUNK) r++;
        owner[t] = r;
    }
    owner[ntiles] = (uint32_t) table.size() - 2;                      // the last piece that holds bytes
}
