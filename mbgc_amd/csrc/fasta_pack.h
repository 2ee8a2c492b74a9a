// The packing of `mbgc-hip r` (included by fasta_input.hip, inside namespace fa, after CHUNK / THREADS / PER and up()): the piece
// table and the owner table mbgc_fasta_pack_dev makes on the host, and the step of one lane. Kept free of HIP calls so that the same
// text compiles as plain C++: tests/fasta_pack_emu.cpp runs the step lane by lane on the CPU under AddressSanitizer.
// ---- mbgc_fasta_pack_dev: pieces src[srcOff, srcOff + len) back to back in dst, optionally folded to upper case. It is a copy, and
// the work unit is a tile of the OUTPUT: 4096 bytes of dst, 16 per lane step, laid over the 16-byte boundaries of dst's address — so
// the output bytes are divided evenly over the waves whatever the pieces look like (one of tens of Mbp spans thousands of tiles,
// hundreds of empty or tiny ones share one), every whole step is one aligned 16-byte vector store, and the load is the side that
// goes unaligned. A tile finds its pieces through an owner table (tile -> the piece that holds its first byte) made on the host; a
// lane searches only between its tile's owner and the next tile's. A step that holds a piece boundary, and the first and last
// step of the output where they are partial, walk byte by byte. Pieces of no bytes have no row.
struct PackPiece { uint64_t dOff, sOff; };   // where the piece starts in dst and in src; it ends where the next row starts (last row: the total)

__device__ __forceinline__ uint32_t pack_find(const PackPiece *__restrict__ P, uint32_t lo, uint32_t hi, uint64_t o) {   // the last piece of [lo, hi] that starts at or before o
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (P[mid].dOff <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the step of lane `lane` of tile `tile`. dst stands `mis` bytes behind a 16-byte boundary: the step covers the output offsets
// [tile * 4096 + lane * 16 - mis, ... + 16) that lie in [0, total). No byte outside dst[0, total) is written, none outside a piece read.
__device__ __forceinline__ void pack_lane_step(const uint8_t *__restrict__ src, const PackPiece *__restrict__ P, const uint32_t *__restrict__ owner,
                                               uint32_t tile, uint32_t lane, uint32_t mis, uint64_t total, bool fold, uint8_t *__restrict__ dst) {
    const uint64_t vs = (uint64_t) tile * CHUNK + (uint64_t) lane * PER, ve = vs + PER;
    if (ve <= mis || vs >= mis + total) return;
    const uint64_t a = vs > mis ? vs - mis : 0, b = ve - mis < total ? ve - mis : total;
    uint32_t r = pack_find(P, owner[tile], owner[tile + 1], a);
    if (b - a == PER && P[r + 1].dOff >= b) {                         // a whole step inside one piece
        uint4 v;
        memcpy(&v, src + P[r].sOff + (a - P[r].dOff), PER);
        if (fold) {
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 4; j++)
                w[j] = (uint32_t) up((uint8_t) w[j]) | (uint32_t) up((uint8_t) (w[j] >> 8)) << 8 | (uint32_t) up((uint8_t) (w[j] >> 16)) << 16 |
                       (uint32_t) up((uint8_t) (w[j] >> 24)) << 24;
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *(uint4 *) (dst + a) = v;                                     // 16-byte aligned: dst + a = the boundary the step lies on
        return;
    }
    for (uint64_t o = a; o < b; o++) {
        while (P[r + 1].dOff <= o) r++;                               // (the sentinel starts at the total: never passed)
        const uint8_t c = src[P[r].sOff + (o - P[r].dOff)];
        dst[o] = fold ? up(c) : c;
    }
}

// The host's half: the caller's pieces -> dstOff (n + 1 entries) and the table (the pieces that hold bytes, in order, then a sentinel
// at the total); the tiles' owners (ntiles + 1 entries). Returns the total.
struct PackIn { uint64_t srcOff, len; };
inline uint64_t pack_build_table(const PackIn *pieces, uint64_t n, std::vector<PackPiece> &table, uint64_t *dstOff) {
    table.clear();
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        dstOff[k] = total;
        if (pieces[k].len == 0) continue;
        table.push_back(PackPiece{total, pieces[k].srcOff});
        total += pieces[k].len;
    }
    dstOff[n] = total;
    table.push_back(PackPiece{total, 0});
    return total;
}
inline void pack_build_owner(const std::vector<PackPiece> &table, uint32_t mis, uint32_t ntiles, std::vector<uint32_t> &owner) {
    owner.resize((size_t) ntiles + 1);
    uint32_t r = 0;
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint64_t vs = (uint64_t) t * CHUNK, first = vs > mis ? vs - mis : 0;
        while (table[r + 1].dOff <= first) r++;
        owner[t] = r;
    }
    owner[ntiles] = (uint32_t) table.size() - 2;                      // the last piece that holds bytes
}
