// The one grid the record scans share — `mbgc-hip f`, `s`, `k` and `u` (included by fasta_input.hip, inside namespace fa, in front of
// fasta_find.h, fasta_stats.h, fasta_sketch.h and fasta_dups.h). Kept free of HIP calls so that the same text compiles as plain C++: the
// four emulations under tests/ include it in front of the lane steps they run.
// ---- tiles: the records are cut on the 16-byte grid of the buffer's ADDRESSES, so that every tile is read with aligned 16-byte loads
// whatever the record's offset is: record r's tiles start at the address of its first byte rounded down to 16, SCAN_TILE positions
// each; the positions of the first tile that lie in front of the record are nobody's. A scan says how many START positions a record
// has (its bytes, its grams, its k-mers); a record without one has no tile. tileStart[] is the prefix sum of the records' tile counts,
// one flat list over all records; a block finds its tile's record by bisection. A byte outside the buffer is never read: a vector that
// does not lie inside it whole is read byte by byte, the bytes inside only (the lane steps).
constexpr uint32_t SCAN_TILE = 4096, SCAN_THREADS = 256, SCAN_PER = SCAN_TILE / SCAN_THREADS;
static_assert(SCAN_PER == 16 && SCAN_THREADS % 64 == 0, "a lane reads its 16 positions as one aligned vector; a block is whole waves");

struct alignas(16) ScanVec { uint32_t w[4]; };
struct ScanRec { uint64_t off, len; };                                // the ABI's mbgc_fasta_crc_rec_t
struct ScanTile { uint32_t r; ScanRec rec; uintptr_t addr; };         // the record's index, the record, the address of the tile's first byte

// the tiles of a record whose first byte has address `first` and which holds `positions` start positions
__host__ __device__ __forceinline__ uint64_t scan_tiles_of(uintptr_t first, uint64_t positions) {
    return positions ? ((first & 15) + positions + SCAN_TILE - 1) / SCAN_TILE : 0;
}

// the record of tile `tile`: the last r of [0, n) with tileStart[r] <= tile (records without a tile are passed over)
__host__ __device__ __forceinline__ uint32_t scan_tile_record(const uint64_t *__restrict__ tileStart, uint32_t n, uint64_t tile) {
    uint32_t lo = 0, hi = n;                                         // tileStart[lo] <= tile < tileStart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tileStart[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// how every scan opens a tile of the flat list; scan_tile_of for a scan that reads a word of its own by the record's index before
// the record (k_fa_sketch's group: the loads go out together, none waits for another)
__host__ __device__ __forceinline__ ScanTile scan_tile_of(const uint8_t *__restrict__ seq, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                           uint32_t r, uint64_t tile) {
    const ScanRec rec = recs[r];
    return ScanTile{r, rec, (((uintptr_t) seq + rec.off) & ~(uintptr_t) 15) + (tile - tileStart[r]) * SCAN_TILE};
}
__host__ __device__ __forceinline__ ScanTile scan_tile(const uint8_t *__restrict__ seq, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                        uint32_t nrec, uint64_t tile) {
    return scan_tile_of(seq, recs, tileStart, scan_tile_record(tileStart, nrec, tile), tile);
}
