// The inverse of the `-m3` reverse-complement pass, what one work item does (included by copmem_restore.h inside namespace cmr):
// the item bodies of k_varint_decode and k_check, a tile's range of matches and the 16 output bytes of one lane of k_restore_fill,
// with both vector paths. Kept free of HIP calls so that the same text compiles as plain C++: tests/rcrestore_emu.cpp runs it item
// by item, lane by lane on the CPU under AddressSanitizer against exactly sized buffers. Shared-memory staging, the loops over
// tiles, the block scan and the atomics stay in copmem_restore.h.
constexpr uint8_t MARK = (uint8_t) ('$' + 128);      // MBGC_Params::RC_MATCH_MARK, MBGC_Params.h:48
constexpr int LANE = 16;                             // output bytes per lane
constexpr int TPB = 256;
constexpr uint64_t TILE = (uint64_t) TPB * LANE;     // output (or input) bytes per workgroup step
constexpr uint64_t SAT = ~0ull, CAP = 1ull << 62;    // sums beyond CAP saturate: an overflow is seen, never wrapped
constexpr int MAX_VARINT = 10;                       // bytes of a 64-bit value
constexpr uint64_t CUT_PAD = 64;                     // zero bytes the plan allocates behind the cut stream's last whole tile
enum { E_VARINT_LONG = 1, E_SOURCE = 2 };

struct SatAdd {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return (a > CAP || b > CAP || a + b > CAP) ? SAT : a + b; }
};
struct EndsValue {
    __host__ __device__ uint64_t operator()(uint8_t b) const { return b < 128 ? 1u : 0u; }
};

struct Plan {                                        // what the fill reads
    const uint8_t *cut;                              // n bytes (+ zero bytes up to a whole tile, + CUT_PAD)
    const uint64_t *d, *src, *len, *cum;             // per match; cum has M + 1 entries
    uint64_t M, n, orgLen;
};

// ---- plan ----------------------------------------------------------------------------------------------------------------
// byte j of rcMapLen is the first of a value
__device__ __forceinline__ bool value_starts_at(const uint8_t *__restrict__ bytes, uint64_t j) { return !j || bytes[j - 1] < 128; }
// the value whose first byte is byte j (little-endian base 128, the last byte below 128), SAT beyond CAP; tooLong: it does not end
// within MAX_VARINT bytes (or within the stream)
__device__ __forceinline__ uint64_t value_at(const uint8_t *__restrict__ bytes, uint64_t nbytes, uint64_t j, bool &tooLong) {
    uint64_t v = 0;
    tooLong = true;
    for (int k = 0; k < MAX_VARINT && j + k < nbytes; k++) {
        const uint8_t b = bytes[j + k];
        const uint64_t digit = b & 127u;
        if (k == MAX_VARINT - 1) { if (digit) v = SAT; }                   // 128^9 = 2^63: beyond CAP
        else if (v != SAT) v |= digit << (7 * k);
        if (b < 128) { tooLong = false; break; }
    }
    if (v > CAP) v = SAT;
    return v;
}
// the length of match i from the decoded values: val[0] is minMatchLength
__device__ __forceinline__ uint64_t length_of(const uint64_t *__restrict__ val, uint64_t M, uint64_t i) { return i < M ? SatAdd()(val[i + 1], val[0]) : 0; }
// match i: where it starts in restored coordinates and its source -> false if the source does not end before the match starts
// (src[i] + len[i] <= d[i] is what makes the fill's walk end inside the text)
__device__ __forceinline__ bool match_in_bounds(const uint64_t *__restrict__ markPos, const uint8_t *__restrict__ mapOff, int offBytes,
                                                const uint64_t *__restrict__ len, const uint64_t *__restrict__ cum, uint64_t i, uint64_t &di, uint64_t &s) {
    const uint64_t L = len[i], c = cum[i];
    di = 0; s = 0;
    if (L == SAT || c == SAT) return true;                                 // (a saturated sum is reported from cum[M])
    di = markPos[i] - i + c;
    if (offBytes == 4) { uint32_t v; __builtin_memcpy(&v, mapOff + 4 * i, 4); s = v; }
    else __builtin_memcpy(&s, mapOff + 8 * i, 8);
    return !(s > di || L > di - s);
}

// ---- fill ----------------------------------------------------------------------------------------------------------------
// the number k in [lo, hi] with d[j] <= p for every j < k and d[j] > p for every j >= k (true of lo and hi on entry)
__device__ __forceinline__ uint64_t matches_at_or_before(const uint64_t *__restrict__ d, uint64_t lo, uint64_t hi, uint64_t p) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (d[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the matches that start inside tile `tile` (tile * TILE < orgLen): [lo, hi)
__device__ __forceinline__ void matches_of_tile(const Plan &P, uint64_t tile, uint64_t &lo, uint64_t &hi) {
    const uint64_t last = tile * TILE + TILE < P.orgLen ? tile * TILE + TILE - 1 : P.orgLen - 1;
    lo = matches_at_or_before(P.d, 0, P.M, tile * TILE);
    hi = matches_at_or_before(P.d, lo, P.M, last);
}
__device__ __forceinline__ uint8_t complemented(const uint8_t *sl, uint8_t x, uint32_t hops) {
    if (hops == 0) return x;
    x = sl[x];
    return (hops & 1) ? x : sl[x];
}
// restored position p, k = matches_at_or_before(p) -> its byte; every hop lands below the match it leaves (the plan's check)
__device__ __forceinline__ uint8_t restored_byte(const Plan &P, const uint8_t *sl, uint64_t p, uint64_t k, uint32_t &maxHops) {
    uint32_t hops = 0;
    while (k) {
        const uint64_t i = k - 1, di = P.d[i], L = P.len[i];
        if (p - di >= L) break;
        p = P.src[i] + L - 1 - (p - di);
        hops++;
        k = matches_at_or_before(P.d, 0, i, p);
    }
    if (hops > maxHops) maxHops = hops;
    return complemented(sl, P.cut[p - P.cum[k] + k], hops);
}
// [p, p + 16) lies in one literal run: where it starts in the cut stream, else SAT
__device__ __forceinline__ uint64_t literal_run_of_16(const Plan &P, uint64_t p, uint64_t k) {
    if (k && p - P.d[k - 1] < P.len[k - 1]) return SAT;
    const uint64_t runEnd = k < P.M ? P.d[k] : P.orgLen;
    return p + LANE <= runEnd ? p - P.cum[k] + k : SAT;
}
// the lane that owns dst[p0, p0 + 16) (p0 < orgLen, a multiple of 16 inside a tile whose matches are [sLo, sHi)): writes the bytes
// of it that lie below orgLen, nothing else; sl is the complement table
__device__ __forceinline__ void restore_lane(const Plan &P, const uint8_t *sl, uint8_t *__restrict__ dst, uint64_t p0, uint64_t sLo, uint64_t sHi,
                                             uint32_t &maxHops) {
    uint64_t k = matches_at_or_before(P.d, sLo, sHi, p0);
    const bool whole = p0 + LANE <= P.orgLen;
#ifndef MBGC_RC_RESTORE_BYTEWISE                                          /* (defined for the measurement of what the vector path buys) */
    if (whole) {
        uint64_t at = literal_run_of_16(P, p0, k);
        if (at != SAT) {                                                   // 16 literals
            uint4 v;
            __builtin_memcpy(&v, P.cut + at, 16);
            __builtin_memcpy(dst + p0, &v, 16);
            return;
        }
        const uint64_t i = k - 1;                                          // (k != 0: p0 is inside match i, or the run ends within 16 bytes)
        if (k && p0 - P.d[i] < P.len[i] && p0 + LANE <= P.d[i] + P.len[i]) {
            const uint64_t s0 = P.src[i] + P.len[i] - 1 - (p0 + LANE - 1 - P.d[i]);   // the source of the lane's last byte
            at = literal_run_of_16(P, s0, matches_at_or_before(P.d, 0, i, s0));
            if (at != SAT) {                                               // 16 bytes of one match over 16 literals
                uint4 v;
                __builtin_memcpy(&v, P.cut + at, 16);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
                for (int b = 0; b < LANE; b++) {
                    const int f = LANE - 1 - b;
                    o[b >> 2] |= (uint32_t) sl[(w[f >> 2] >> (8 * (f & 3))) & 0xFFu] << (8 * (b & 3));
                }
                v = make_uint4(o[0], o[1], o[2], o[3]);
                __builtin_memcpy(dst + p0, &v, 16);
                if (maxHops < 1) maxHops = 1;
                return;
            }
        }
    }
#endif
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < LANE; b++) {
        const uint64_t p = p0 + b;
        if (p < P.orgLen) {
            while (k < sHi && P.d[k] <= p) k++;
            o[b >> 2] |= (uint32_t) restored_byte(P, sl, p, k, maxHops) << (8 * (b & 3));
        }
    }
    if (whole) {
        const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
        __builtin_memcpy(dst + p0, &v, 16);
    } else {
#pragma unroll
        for (int b = 0; b < LANE; b++)
            if (p0 + b < P.orgLen) dst[p0 + b] = (uint8_t) (o[b >> 2] >> (8 * (b & 3)));
    }
}
