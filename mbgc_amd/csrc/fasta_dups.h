// The two scans of `mbgc-hip u` (included by fasta_input.hip, inside namespace fa, behind fasta_tiles.h, whose grid they scan — a
// record's start positions are its bytes, as for fasta_stats.h): fold and comp of a byte, the arithmetic of the two strand fingerprints, the step of
// one lane of k_fa_dups, the step of one lane of k_fa_dups_verify and the host's last step. Kept free of HIP calls so that the same text
// compiles as plain C++: tests/fasta_dups_emu.cpp runs the steps tile by tile and lane by lane on the CPU under AddressSanitizer, the
// wave's shuffles emulated by arrays. The shuffles, the block's sum in LDS, the atomic adds to a record's row, the ballot and the
// atomic of a refuted pair stay in fasta_input.hip (k_fa_dups, k_fa_dups_verify).
// ---- comp is stated ONCE, in dups_comp_upper: the six pairs on upper case. The device does not look a byte up in a table: the pairs
// keep the case, so comp(b) = b ^ delta(b & 31) for a letter, and the 32 deltas are four 64-bit constants derived from that one
// function at compile time (dups_delta_word). The 256-entry table of the header's comment is dups_comp over 0..255.
// ---- the fingerprints: with T[b] = b + 1, the device sums per record, for q = 0..3, A_q = sum T[fold(s_j)] y_q^(j + 16) and B_q = sum
// T[comp(fold(s_j))] x_q^(j + 16) modulo the prime p_q, y_q being the inverse of x_q; the host (dups_finish) turns them into
//     forward_q = A_q x_q^(len + 15) = sum T[fold(s_j)] x_q^(len - 1 - j),        reverse_q = B_q y_q^16 = sum T[comp(fold(s_j))] x_q^j,
// the forward fingerprint of the record and the forward fingerprint of its reverse complement (comp being an involution). Both sums
// ascend in j, so a position outside the record is a term of 0 and nothing depends on where the record ends; the + 16 keeps the
// exponent of a lane's first position, which lies up to 15 in front of the record in its first tile, above 0. Four primes just below
// 2^31: 124 bits per strand, and every product is 32 x 32 -> 64.
// A lane multiplies its 16 terms with the constants z^0..z^15 and adds them up unreduced (below 2^44), reduces once, and multiplies with
// z^(16 lane), which it computed once per launch; the wave adds modulo p by shuffles; lanes 0..7 of the block add the four waves' sums
// and multiply with the tile's power z^(16 - (address & 15) + 4096 tile), which the first wave keeps: by squaring when the block
// comes to a record, by one multiplication with z^(4096 gridDim) while it stays in it.
constexpr uint32_t DUPS_TILE = SCAN_TILE, DUPS_THREADS = SCAN_THREADS, DUPS_PER = SCAN_PER;   // 16 positions per lane
constexpr uint32_t DUPS_FORWARD_ONLY = 1u, DUPS_EXACT_CASE = 2u, DUPS_WEAK_HASH = 4u;            // MBGC_FASTA_DUPS_*

struct DupsPair { uint32_t rec, rep, strand, reserved; };             // is record rec the same as record rep read forward (0) / as its reverse complement (1)?
struct DupsPrint { uint32_t v[4]; };                                  // a strand's fingerprint: the residue modulo each prime
struct DupsTab { uint32_t v[17]; };

// ---- the bytes
constexpr uint8_t dups_comp_upper(uint8_t u) {
    switch (u) {
        case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'R': return 'Y'; case 'Y': return 'R'; case 'K': return 'M'; case 'M': return 'K';
        case 'B': return 'V'; case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D';
        default: return u;
    }
}
constexpr uint64_t dups_delta_word(uint32_t w) {                     // byte i: 'letter' ^ comp('letter') of letter number 8 w + i ('A' = 1)
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; i++) {
        const uint8_t u = (uint8_t) (0x40u | (8 * w + i));
        v |= (uint64_t) (uint8_t) (u ^ dups_comp_upper(u)) << (8 * i);
    }
    return v;
}
__host__ __device__ __forceinline__ bool dups_is_letter(uint8_t b) { return (uint8_t) ((b | 0x20) - 'a') < 26; }
__host__ __device__ __forceinline__ uint8_t dups_fold(uint8_t b, bool exactCase) { return (uint8_t) (!exactCase && dups_is_letter(b) ? b & 0xDF : b); }
__host__ __device__ __forceinline__ uint8_t dups_comp(uint8_t b) {
    constexpr uint64_t W0 = dups_delta_word(0), W1 = dups_delta_word(1), W2 = dups_delta_word(2), W3 = dups_delta_word(3);
    const uint32_t i = b & 31u, w = i >> 3;
    const uint64_t word = w == 0 ? W0 : w == 1 ? W1 : w == 2 ? W2 : W3;
    return (uint8_t) (dups_is_letter(b) ? b ^ (uint8_t) (word >> (8 * (i & 7))) : b);
}
__host__ __device__ __forceinline__ uint32_t dups_T(uint8_t b) { return (uint32_t) b + 1u; }

// ---- the arithmetic: q = 0..3 is the forward sum (z = y_q), q = 4..7 the reverse one (z = x_(q - 4)), modulo p_(q & 3)
constexpr uint32_t dups_p(uint32_t q) { return (q & 3) == 0 ? 2147483647u : (q & 3) == 1 ? 2147483629u : (q & 3) == 2 ? 2147483587u : 2147483579u; }
constexpr uint32_t dups_x(uint32_t q) { return (q & 3) == 0 ? 1709817893u : (q & 3) == 1 ? 1363361858u : (q & 3) == 2 ? 1783135819u : 560104786u; }
constexpr uint32_t dups_y(uint32_t q) { return (q & 3) == 0 ? 673830337u : (q & 3) == 1 ? 351693872u : (q & 3) == 2 ? 1833976688u : 1470025292u; }
constexpr uint32_t dups_z(uint32_t q) { return q < 4 ? dups_y(q) : dups_x(q); }
constexpr uint32_t dups_mulmod_c(uint32_t a, uint32_t b, uint32_t p) { return (uint32_t) ((uint64_t) a * b % p); }
constexpr uint32_t dups_pow_c(uint32_t base, uint64_t e, uint32_t p) {
    uint32_t r = 1;
    for (; e; e >>= 1, base = dups_mulmod_c(base, base, p)) if (e & 1) r = dups_mulmod_c(r, base, p);
    return r;
}
constexpr DupsTab dups_tab(uint32_t q) {                              // z^0 .. z^16
    DupsTab t = {};
    uint32_t pw = 1;
    for (uint32_t k = 0; k < 17; k++) { t.v[k] = pw; pw = dups_mulmod_c(pw, dups_z(q), dups_p(q)); }
    return t;
}
static_assert(dups_mulmod_c(dups_x(0), dups_y(0), dups_p(0)) == 1 && dups_mulmod_c(dups_x(1), dups_y(1), dups_p(1)) == 1 &&
              dups_mulmod_c(dups_x(2), dups_y(2), dups_p(2)) == 1 && dups_mulmod_c(dups_x(3), dups_y(3), dups_p(3)) == 1, "y is the inverse of x modulo p");
static_assert(dups_comp_upper(dups_comp_upper('R')) == 'R' && dups_delta_word(0) == 0x0400000c04141500ull, "comp is an involution; the deltas of @, A .. G");

template <uint32_t Q> __host__ __device__ __forceinline__ uint32_t dups_mod(uint64_t v) { return (uint32_t) (v % dups_p(Q)); }
template <uint32_t Q> __host__ __device__ __forceinline__ uint32_t dups_mulmod(uint32_t a, uint32_t b) { return dups_mod<Q>((uint64_t) a * b); }
template <uint32_t Q> __host__ __device__ __forceinline__ uint32_t dups_addmod(uint32_t a, uint32_t b) {     // a, b < p < 2^31
    const uint32_t s = a + b;
    return s >= dups_p(Q) ? s - dups_p(Q) : s;
}
template <uint32_t Q> __host__ __device__ __forceinline__ uint32_t dups_pow(uint64_t e) {
    uint32_t r = 1, base = dups_z(Q);
    for (; e; e >>= 1, base = dups_mulmod<Q>(base, base)) if (e & 1) r = dups_mulmod<Q>(r, base);
    return r;
}
// out[q] = z_q^e, all eight
__host__ __device__ __forceinline__ void dups_pow8(uint64_t e, uint32_t out[8]) {
    out[0] = dups_pow<0>(e); out[1] = dups_pow<1>(e); out[2] = dups_pow<2>(e); out[3] = dups_pow<3>(e);
    out[4] = dups_pow<4>(e); out[5] = dups_pow<5>(e); out[6] = dups_pow<6>(e); out[7] = dups_pow<7>(e);
}
// a[q] = a[q] b[q] mod p_q, all eight
__host__ __device__ __forceinline__ void dups_mul8(uint32_t a[8], const uint32_t b[8]) {
    a[0] = dups_mulmod<0>(a[0], b[0]); a[1] = dups_mulmod<1>(a[1], b[1]); a[2] = dups_mulmod<2>(a[2], b[2]); a[3] = dups_mulmod<3>(a[3], b[3]);
    a[4] = dups_mulmod<4>(a[4], b[4]); a[5] = dups_mulmod<5>(a[5], b[5]); a[6] = dups_mulmod<6>(a[6], b[6]); a[7] = dups_mulmod<7>(a[7], b[7]);
}
// a[q] = a[q] + b[q] mod p_q, all eight: a step of the wave's sum (b: the partner lane's)
__host__ __device__ __forceinline__ void dups_add8(uint32_t a[8], const uint32_t b[8]) {
    a[0] = dups_addmod<0>(a[0], b[0]); a[1] = dups_addmod<1>(a[1], b[1]); a[2] = dups_addmod<2>(a[2], b[2]); a[3] = dups_addmod<3>(a[3], b[3]);
    a[4] = dups_addmod<4>(a[4], b[4]); a[5] = dups_addmod<5>(a[5], b[5]); a[6] = dups_addmod<6>(a[6], b[6]); a[7] = dups_addmod<7>(a[7], b[7]);
}
// what lane q (of 0..7) adds to its counter of the record: (the block's sum of residue q, below 2^33) z_q^e, below 2^31
__host__ __device__ __forceinline__ uint32_t dups_tile_term(uint32_t q, uint64_t sum, const uint32_t pw[8]) {
    const uint32_t t[8] = {dups_mulmod<0>(dups_mod<0>(sum), pw[0]), dups_mulmod<1>(dups_mod<1>(sum), pw[1]), dups_mulmod<2>(dups_mod<2>(sum), pw[2]),
                           dups_mulmod<3>(dups_mod<3>(sum), pw[3]), dups_mulmod<4>(dups_mod<4>(sum), pw[4]), dups_mulmod<5>(dups_mod<5>(sum), pw[5]),
                           dups_mulmod<6>(dups_mod<6>(sum), pw[6]), dups_mulmod<7>(dups_mod<7>(sum), pw[7])};
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) v = k == q ? t[k] : v;
    return v;
}
// the exponent of the tile's power: tile `index` of the record whose first byte has address `first`
__host__ __device__ __forceinline__ uint64_t dups_tile_exp(uintptr_t first, uint64_t index) { return 16u - (uint32_t) (first & 15) + (uint64_t) DUPS_TILE * index; }

template <uint32_t Q> __host__ __device__ __forceinline__ uint32_t dups_lane_sum(const uint32_t t[DUPS_PER]) {
    constexpr DupsTab Z = dups_tab(Q);
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < DUPS_PER; k++) s += (uint64_t) t[k] * Z.v[k];      // (16 terms below 2^9 2^31)
    return dups_mod<Q>(s);
}

// the step of k_fa_dups: lane `lane` (of DUPS_THREADS) owns the DUPS_PER positions from address tileAddr + 16 lane on -> out[q] = the sum
// over its positions t0 + k inside the record of T[.] z_q^k, reduced; zeros for a lane without one. The vector is read as stats_lane_step
// reads it: aligned and whole where it lies inside seq[0, seqBytes), its bytes inside one by one otherwise
__device__ __forceinline__ void dups_lane_step(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec rec, uintptr_t tileAddr, uint32_t lane, bool exactCase,
                                               uint32_t out[8]) {
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) out[q] = 0;
    const uintptr_t lo = (uintptr_t) seq, hi = lo + seqBytes, v = tileAddr + 16u * lane;
    const int64_t t0 = (int64_t) v - (int64_t) (lo + rec.off);
    if (t0 + (int64_t) DUPS_PER <= 0 || t0 >= (int64_t) rec.len) return;
    ScanVec x = {{0, 0, 0, 0}};
    if (v >= lo && v + 16 <= hi) x = *(const ScanVec *) v;
    else
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (v + k >= lo && v + k < hi) x.w[k >> 2] |= (uint32_t) *(const uint8_t *) (v + k) << (8 * (k & 3));
    uint32_t fw[DUPS_PER], rc[DUPS_PER];
#pragma unroll
    for (uint32_t k = 0; k < DUPS_PER; k++) {
        const int64_t t = t0 + k;
        const bool in = t >= 0 && t < (int64_t) rec.len;
        const uint8_t f = dups_fold((uint8_t) (x.w[k >> 2] >> (8 * (k & 3))), exactCase);
        fw[k] = in ? dups_T(f) : 0u;
        rc[k] = in ? dups_T(dups_comp(f)) : 0u;
    }
    out[0] = dups_lane_sum<0>(fw); out[1] = dups_lane_sum<1>(fw); out[2] = dups_lane_sum<2>(fw); out[3] = dups_lane_sum<3>(fw);
    out[4] = dups_lane_sum<4>(rc); out[5] = dups_lane_sum<5>(rc); out[6] = dups_lane_sum<6>(rc); out[7] = dups_lane_sum<7>(rc);
}

// the step of k_fa_dups_verify: lane `lane` owns the 16 positions of record a from address tileAddr + 16 lane on (a's side is read on
// the 16-byte grid, aligned); b has a's length and is read where the same positions lie — forward — or mirrored, from its end, and
// complemented. -> does one of the lane's positions differ? A lane whose 16 positions all lie inside the record reads a vector on
// either side (b's at any address: the bytes are inside b, so inside the buffer); the others read the positions inside, byte by byte
__device__ __forceinline__ bool dups_verify_step(const uint8_t *__restrict__ seq, const ScanRec a, const ScanRec b, uint32_t strand, bool exactCase, uintptr_t tileAddr,
                                                 uint32_t lane) {
    const uintptr_t v = tileAddr + 16u * lane;
    const int64_t t0 = (int64_t) v - (int64_t) ((uintptr_t) seq + a.off), len = (int64_t) a.len;
    if (t0 + 16 <= 0 || t0 >= len) return false;
    bool differ = false;
    if (t0 >= 0 && t0 + 16 <= len) {
        const ScanVec x = *(const ScanVec *) v;
        ScanVec y;
        memcpy(&y, seq + b.off + (strand ? (uint64_t) (len - 16 - t0) : (uint64_t) t0), 16);
        if (strand) y = ScanVec{{__builtin_bswap32(y.w[3]), __builtin_bswap32(y.w[2]), __builtin_bswap32(y.w[1]), __builtin_bswap32(y.w[0])}};     // (mirrored)
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint8_t p = dups_fold((uint8_t) (x.w[k >> 2] >> (8 * (k & 3))), exactCase), q = dups_fold((uint8_t) (y.w[k >> 2] >> (8 * (k & 3))), exactCase);
            differ |= p != (strand ? dups_comp(q) : q);
        }
        return differ;
    }
    for (int64_t t = t0 < 0 ? 0 : t0; t < t0 + 16 && t < len; t++) {
        const uint8_t p = dups_fold(seq[a.off + (uint64_t) t], exactCase), q = dups_fold(seq[b.off + (uint64_t) (strand ? len - 1 - t : t)], exactCase);
        differ |= p != (strand ? dups_comp(q) : q);
    }
    return differ;
}

// The host's last step: a record's row of eight sums (any multiple of p added) and its length -> the two fingerprints
inline void dups_finish(const unsigned long long row[8], uint64_t len, DupsPrint &forward, DupsPrint &reverse) {
    const uint32_t f[4] = {dups_mulmod<0>(dups_mod<0>(row[0]), dups_pow_c(dups_x(0), len + 15, dups_p(0))), dups_mulmod<1>(dups_mod<1>(row[1]), dups_pow_c(dups_x(1), len + 15, dups_p(1))),
                           dups_mulmod<2>(dups_mod<2>(row[2]), dups_pow_c(dups_x(2), len + 15, dups_p(2))), dups_mulmod<3>(dups_mod<3>(row[3]), dups_pow_c(dups_x(3), len + 15, dups_p(3)))};
    const uint32_t r[4] = {dups_mulmod<0>(dups_mod<0>(row[4]), dups_pow_c(dups_y(0), 16, dups_p(0))), dups_mulmod<1>(dups_mod<1>(row[5]), dups_pow_c(dups_y(1), 16, dups_p(1))),
                           dups_mulmod<2>(dups_mod<2>(row[6]), dups_pow_c(dups_y(2), 16, dups_p(2))), dups_mulmod<3>(dups_mod<3>(row[7]), dups_pow_c(dups_y(3), 16, dups_p(3)))};
    for (int i = 0; i < 4; i++) { forward.v[i] = f[i]; reverse.v[i] = r[i]; }
}
