// Per-range CRC-32 for bytes in HBM (included by fasta_input.hip, inside namespace fa): the row table mbgc_fasta_crc_dev makes on
// the host, the constants it uploads once, and the steps of one lane. Kept free of HIP calls so that the same text compiles as plain
// C++: tests/fasta_crc_emu.cpp runs the steps row by row, lane by lane on the CPU under AddressSanitizer. The tables in LDS, the
// shuffles that fold a group of lanes and the atomic of a cut record stay in fasta_input.hip (k_fa_crc).
// ---- crc[k] = zlib's crc32(0, seq + off, len) for n ranges of any length, 0 bytes to a chromosome, in one launch. The CRC register
// is linear in (its start value, the data): a range cut into shares gives XOR over the shares of reg(share) * x^(8 * bytes of the
// range behind the share) mod P, where the share at the range's first byte starts from 0xffffffff and every other one from 0 — the
// raw registers, not finalised CRCs — and the final XOR with 0xffffffff is applied once per range, by the host.
//   share  CRC_SHARE = 256 bytes: what one lane walks.
//   row    what a group of G lanes takes, G = 1, 4, 16 or 64 by the row's length (<= 256, <= 1024, <= 4096, <= 16384 bytes); a wave
//          holds 64 / G rows of one class, so ranges shorter than a lane's share sit 64 to a wave and no wave serves one tiny range.
//          The shares of a row are laid from its END: lane s of nl = ceil(len / 256) takes [len - (nl - s) * 256, len - (nl - s - 1) *
//          256) clipped at 0, so the bytes behind a share inside its row are (nl - 1 - s) * 256 and the factor comes from a table of 64.
//   piece  a range longer than 16384 bytes is cut into rows of class 64 (the last one shorter); row j carries the bytes of the range
//          behind it, the wave's folded value is multiplied by x^(8 * behind) — the product of the squares x^(8 * 2^b) of its set
//          bits b, one per lane, folded by shuffles — and XORed into the range's word with one atomic. Rows of the other classes are
//          whole ranges and store their word.
// The host's table is O(n + bytes / 16384). A lane reads its share with aligned 16-byte and 4-byte loads where a whole vector lies in
// the share and byte by byte at its two ends: no byte outside [off, off + len) is read on a range's behalf.
// The byte-table lookup goes through LDS. LOOKUP_BYTE (the one in use): one 1 KiB table of 256 entries hit by 64 data-dependent
// indices, 4 dependent lookups per word (what fasta_deflate.h does for its 32 KiB chunk); two lanes of a 32-lane half that meet on a
// bank with different entries cost an LDS cycle each. LOOKUP_NIBBLE (MBGC_HIP_CRC_LOOKUP=nibble): the register is advanced 4 bytes at
// a time as the XOR of 8 lookups in 16-entry tables (one per nibble of reg ^ word: slicing-by-4 taken down to nibbles, which
// linearity allows), a single byte as 2 lookups; every table entry is stored 32 times, once per LDS bank, and a lane reads the copy
// in its own bank (lane & 31), so the lookups are conflict-free by construction and independent of each other — at twice the
// lookups, 20 KiB of LDS and a table fill of 5120 words per block. Measured (MEASUREMENTS.md §9, profiles/crc_bench.py): the two
// are within 3 % of each other on long ranges, where the kernel runs at HBM-class rates either way, and the byte table is 20 %
// faster on 2 000 000 short ranges. The simpler one is in use; the other stays as the alternative the choice was measured against.
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_SHARE = 256, CRC_LANES = 64, CRC_PIECE = CRC_SHARE * CRC_LANES, CRC_CLASSES = 4;
constexpr uint32_t CRC_THREADS = 256, CRC_WAVES = CRC_THREADS / CRC_LANES;
constexpr uint32_t CRC_BANKS = 32;                                     // ds_read_b32: bank = (address / 4) % 32, per 32-lane half
constexpr uint32_t CRC_LOOKUP_BYTE = 0, CRC_LOOKUP_NIBBLE = 1;
__host__ __device__ constexpr uint32_t crc_class_lanes(uint32_t c) { return 1u << (2 * c); }                       // 1, 4, 16, 64
__host__ __device__ constexpr uint32_t crc_class_max(uint32_t c) { return CRC_SHARE << (2 * c); }                  // 256, 1024, 4096, 16384

// (fasta_gzip_common.h holds the same two for the device alone; the host's table builder and mbgc_fasta_crc_combine need them too)
__host__ __device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {   // a * b mod P, bit-reflected (zlib's multmodp)
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
__host__ __device__ __forceinline__ uint32_t crc_xpow8(uint64_t nbytes) {           // x^(8 * nbytes) mod P
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) p = crc_mulmod(sq, p);
        sq = crc_mulmod(sq, sq);
    }
    return p;
}
__host__ __device__ __forceinline__ uint32_t crc_shift(uint32_t c, uint32_t bits) {  // the register c advanced over `bits` zero bits
    for (uint32_t k = 0; k < bits; k++) c = c & 1u ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}

// what the host uploads once per handle
struct CrcConsts {
    uint32_t nib4[8][16];        // nib4[t][v]: the register v << 4 t advanced over 4 bytes
    uint32_t nib1[2][16];        // nib1[t][v]: the register v << 4 t advanced over 1 byte
    uint32_t byteTab[256];       // the classic table: the register i advanced over 1 byte
    uint32_t pw[CRC_LANES];      // x^(8 * 256 * j) mod P
    uint32_t sq[64];             // x^(8 * 2^b) mod P
};
inline void crc_build_consts(CrcConsts &K) {
    for (uint32_t t = 0; t < 8; t++) for (uint32_t v = 0; v < 16; v++) K.nib4[t][v] = crc_shift(v << (4 * t), 32);
    for (uint32_t t = 0; t < 2; t++) for (uint32_t v = 0; v < 16; v++) K.nib1[t][v] = crc_shift(v << (4 * t), 8);
    for (uint32_t i = 0; i < 256; i++) K.byteTab[i] = crc_shift(i, 8);
    for (uint32_t j = 0; j < CRC_LANES; j++) K.pw[j] = crc_xpow8((uint64_t) CRC_SHARE * j);
    uint32_t s = 0x00800000u;                                           // x^8
    for (uint32_t b = 0; b < 64; b++) { K.sq[b] = s; s = crc_mulmod(s, s); }
}

// the tables as a block holds them in LDS
constexpr uint32_t CRC_NIB_WORDS = 10 * 16 * CRC_BANKS;                 // nib4 then nib1, every entry once per bank
template <uint32_t LOOKUP> struct CrcShared;
template <> struct CrcShared<CRC_LOOKUP_NIBBLE> { uint32_t tab[CRC_NIB_WORDS]; uint32_t pw[CRC_LANES], sq[64]; };
template <> struct CrcShared<CRC_LOOKUP_BYTE> { uint32_t tab[256]; uint32_t pw[CRC_LANES], sq[64]; };

// thread `tid` of `nthreads` fills its part of the block's tables (a barrier follows)
template <uint32_t LOOKUP> __device__ __forceinline__ void crc_fill_shared(CrcShared<LOOKUP> &S, const CrcConsts *__restrict__ K, uint32_t tid, uint32_t nthreads) {
    if (LOOKUP == CRC_LOOKUP_NIBBLE) {
        const uint32_t *flat = &K->nib4[0][0];                          // (nib1 lies right behind nib4)
        for (uint32_t i = tid; i < CRC_NIB_WORDS; i += nthreads) S.tab[i] = flat[i / CRC_BANKS];
    } else
        for (uint32_t i = tid; i < 256; i += nthreads) S.tab[i] = K->byteTab[i];
    for (uint32_t i = tid; i < CRC_LANES; i += nthreads) { S.pw[i] = K->pw[i]; S.sq[i] = K->sq[i]; }
}

template <uint32_t LOOKUP> __device__ __forceinline__ uint32_t crc_byte(const CrcShared<LOOKUP> &S, uint32_t bank, uint32_t r, uint32_t b) {
    if (LOOKUP == CRC_LOOKUP_NIBBLE) {
        const uint32_t x = (r ^ b) & 255u;
        return (r >> 8) ^ S.tab[(128 + (x & 15u)) * CRC_BANKS + bank] ^ S.tab[(144 + (x >> 4)) * CRC_BANKS + bank];
    }
    return S.tab[(r ^ b) & 255u] ^ (r >> 8);
}
template <uint32_t LOOKUP> __device__ __forceinline__ uint32_t crc_word(const CrcShared<LOOKUP> &S, uint32_t bank, uint32_t r, uint32_t w) {   // 4 bytes, little-endian
    if (LOOKUP == CRC_LOOKUP_NIBBLE) {
        const uint32_t x = r ^ w;
        uint32_t o = 0;
        for (uint32_t t = 0; t < 8; t++) o ^= S.tab[(16 * t + ((x >> (4 * t)) & 15u)) * CRC_BANKS + bank];
        return o;
    }
    for (uint32_t j = 0; j < 4; j++) r = S.tab[(r ^ (w >> (8 * j))) & 255u] ^ (r >> 8);
    return r;
}

// a row: a whole range, or one piece of a cut range (then `behind` of the same index holds the bytes of the range behind it)
struct CrcRow { uint64_t off; uint32_t len, rec; };                     // rec | CRC_FIRST: the row starts its range
constexpr uint32_t CRC_FIRST = 0x80000000u;
struct CrcPlan {                                                        // rows of class c: [row0[c], row0[c + 1]); their waves start at wave0[c]
    uint32_t row0[CRC_CLASSES + 1], wave0[CRC_CLASSES + 1];
};

// the step of lane `lane` of the wave that holds row `row` in the group of G lanes the lane belongs to: the register over the lane's
// share, moved to the row's end. Reads p[0, R.len) of the row's bytes and nothing else.
template <uint32_t LOOKUP> __device__ __forceinline__ uint32_t crc_lane_step(const uint8_t *__restrict__ seq, const CrcRow R, uint32_t G, uint32_t lane,
                                                                              const CrcShared<LOOKUP> &S) {
    const uint32_t s = lane & (G - 1), nl = (R.len + CRC_SHARE - 1) / CRC_SHARE;
    if (s >= nl) return 0;
    const uint32_t endAt = R.len - (nl - 1 - s) * CRC_SHARE, a = endAt > CRC_SHARE ? endAt - CRC_SHARE : 0, bank = lane & (CRC_BANKS - 1);
    const uint8_t *p = seq + R.off;
    uint32_t r = (a == 0 && (R.rec & CRC_FIRST)) ? 0xffffffffu : 0u, i = a;
    while (i < endAt && (((uintptr_t) (p + i)) & 3u)) r = crc_byte(S, bank, r, p[i++]);
    while (i + 4 <= endAt) {
        if ((((uintptr_t) (p + i)) & 15u) == 0 && i + 16 <= endAt) {
            const uint4 v = *(const uint4 *) (p + i);
            r = crc_word(S, bank, r, v.x); r = crc_word(S, bank, r, v.y); r = crc_word(S, bank, r, v.z); r = crc_word(S, bank, r, v.w);
            i += 16;
        } else {
            r = crc_word(S, bank, r, *(const uint32_t *) (p + i));
            i += 4;
        }
    }
    while (i < endAt) r = crc_byte(S, bank, r, p[i++]);
    return crc_mulmod(r, S.pw[nl - 1 - s]);
}
// lane b's factor of x^(8 * behind): the product over the 64 lanes is the power
template <uint32_t LOOKUP> __device__ __forceinline__ uint32_t crc_pow_lane(uint64_t behind, uint32_t lane, const CrcShared<LOOKUP> &S) {
    return (behind >> lane) & 1u ? S.sq[lane] : 0x80000000u;
}

// The host's half: the caller's ranges -> rows sorted by class (a stable order inside a class), the bytes behind every row of the
// last class, the plan. Ranges of no bytes have no row. Returns the number of waves.
struct CrcIn { uint64_t off, len; };
inline uint64_t crc_build_table(const CrcIn *recs, uint64_t n, std::vector<CrcRow> &rows, std::vector<uint64_t> &behind, CrcPlan &plan) {
    uint64_t count[CRC_CLASSES] = {0, 0, 0, 0};
    const auto cls = [](uint64_t len) { uint32_t c = 0; while (c + 1 < CRC_CLASSES && len > crc_class_max(c)) c++; return c; };
    for (uint64_t k = 0; k < n; k++)
        if (recs[k].len) { const uint32_t c = cls(recs[k].len); count[c] += c + 1 < CRC_CLASSES ? 1 : (recs[k].len + CRC_PIECE - 1) / CRC_PIECE; }
    uint64_t at[CRC_CLASSES], total = 0, waves = 0;
    for (uint32_t c = 0; c < CRC_CLASSES; c++) {
        plan.row0[c] = (uint32_t) total; plan.wave0[c] = (uint32_t) waves;
        at[c] = total; total += count[c];
        const uint64_t perWave = CRC_LANES / crc_class_lanes(c);
        waves += (count[c] + perWave - 1) / perWave;
    }
    plan.row0[CRC_CLASSES] = (uint32_t) total; plan.wave0[CRC_CLASSES] = (uint32_t) waves;
    rows.resize(total);
    behind.assign(count[CRC_CLASSES - 1], 0);
    const uint64_t cut0 = at[CRC_CLASSES - 1];
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t len = recs[k].len;
        if (!len) continue;
        const uint32_t c = cls(len);
        if (c + 1 < CRC_CLASSES) { rows[at[c]++] = CrcRow{recs[k].off, (uint32_t) len, (uint32_t) k | CRC_FIRST}; continue; }
        for (uint64_t o = 0; o < len; o += CRC_PIECE) {
            const uint64_t m = std::min<uint64_t>(CRC_PIECE, len - o);
            behind[at[c] - cut0] = len - o - m;
            rows[at[c]++] = CrcRow{recs[k].off + o, (uint32_t) m, (uint32_t) k | (o ? 0u : CRC_FIRST)};
        }
    }
    return waves;
}
