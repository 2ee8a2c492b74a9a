// gzip inflate for whole files in HBM (included by fasta_input.hip, inside namespace fa): mbgc_fasta_inflate_dev's decoder, one
// gzip file per wave. Kept free of HIP calls so that the same text compiles as plain C++: tests/fasta_inflate_emu.cpp runs it on
// the CPU under AddressSanitizer with buffers exactly as long as declared. The includer says how a wave is spelt:
//   INF_LANES_DO(lane)   the statement behind it runs once per lane (the device: this thread's lane; the CPU: a loop over 64 lanes)
//   INF_LANE0            true in the lane that writes what the whole wave decided
//   INF_SYNC()           orders the wave's LDS traffic between a section of lane work and what reads its results
//   INF_UNI(x)           x, known to be the same in every lane (the device: read from the first lane, so it lives in a scalar register)
//
// A DEFLATE stream is one chain of dependent decisions, so the decode state — bit buffer, input and output positions, the block's
// codes — is the same in all 64 lanes and every branch on it is uniform; the lanes differ only where there is width to use: the
// input window's refill, the code tables' build, a match's copy, a stored block's copy, the ring's flush and the CRC.
//   input   a 4 KiB window of the job's bytes in LDS, loaded 16 bytes per lane; bytes past the job's end read as zero IN LDS (no
//           byte outside [0, inLen) is loaded), and the bit position is held against 8 * inLen after every symbol — a stream that
//           runs off its end stops there.
//   output  the last 32 KiB in an LDS ring, indexed so that 16-byte boundaries of the ring are 16-byte boundaries of the output in
//           HBM. Back-references read the ring, never HBM. Half a ring behind the write position the ring is drained: whole
//           16 KiB pieces go through the CRC, and everything up to the last 16-byte boundary goes to HBM in aligned vector stores
//           (bytes in front of the first boundary and, at the job's end, behind the last one, singly).
//   codes   a fast table indexed by the next 10 (distances, code lengths: 8, 7) bits, and for longer codes the canonical walk over
//           the per-length counts and the symbols in code order; a table entry of 0 (a longer code, or none at all) takes the walk.
//           What zlib refuses is refused: over-subscribed sets; incomplete ones unless all there is is one code of one bit.
//   crc     lane i takes the raw CRC of 256 bytes by the byte table, multiplies it by x^(8 * 256 * (n - 1 - i)) mod P, the wave
//           folds: reg = reg * x^(8 * 256 * n) ^ XOR of those (zlib's crc32_combine arithmetic); tails shorter than 256 byte by byte.
// Every loop advances the input's bit position or the output position, or ends the job with a status.
// A job is ONE wave (a block of INF_WAVE threads). What one lane writes to LDS and another reads is separated by INF_SYNC() wherever
// lanes work side by side; the single values the first lane writes between two such sections (a literal's byte, a code length) and
// the whole wave reads back lean on that: a wave's LDS operations are carried out in the order it issues them.
#include "fasta_gzip_common.h"

constexpr uint32_t INF_WAVE = 64;
constexpr uint32_t INF_RING = 32768, INF_RMASK = INF_RING - 1;
constexpr uint32_t INF_INBUF = 4096;                 // the input window (a multiple of INF_WAVE * 16)
constexpr uint32_t INF_DRAIN = 16384;                // the ring is drained when this much of it is neither flushed nor summed
constexpr uint32_t INF_CL = 256;                     // bytes per lane and CRC step; INF_WAVE * INF_CL == INF_DRAIN
constexpr uint32_t INF_LFAST = 10, INF_DFAST = 8, INF_CFAST = 7;
constexpr int INF_OK = 0, INF_ESHORT = 1, INF_EDATA = 2, INF_ECHECK = 3;   // MBGC_INFLATE_*
// (after a drain less than INF_DRAIN bytes are pending, and one step adds at most INF_INBUF: nothing pending is overwritten)
static_assert(INF_WAVE * INF_CL == INF_DRAIN && INF_INBUF % (INF_WAVE * 16) == 0 && INF_DRAIN + INF_INBUF + 258 <= INF_RING, "ring arithmetic");

struct InfJob { uint64_t inOff, inLen, outOff, outCap; };
struct InfResult { int32_t status; uint32_t members; uint64_t outLen, inUsed; };

struct InfCode {
    uint16_t cnt[16];                                // codes per length
    uint16_t sorted[288];                            // the symbols in code order
    uint16_t tab[1u << INF_LFAST];                   // next bits -> symbol | length << 9; 0: take the walk
};

struct InfShared {
    alignas(16) uint8_t ring[INF_RING];
    alignas(16) uint8_t inbuf[INF_INBUF];
    InfCode lit, dist;                               // (the code-length code lives in dist until the block's lengths are read)
    uint8_t lens[320];
    uint32_t crcTab[256];
    uint32_t crcK[INF_WAVE + 1];                     // x^(8 * INF_CL * j) mod P
    uint32_t red[INF_WAVE];
};

INF_CONST const uint8_t INF_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Inf {
    InfShared &S;
    const uint8_t *in; uint64_t inLen;               // the job's input: in[0, inLen)
    uint8_t *out; uint64_t outCap;                   // the job's output: out[0, outCap)
    uint32_t bias;                                   // out's address modulo 16: ring slot of output byte p = (p + bias) & INF_RMASK
    uint64_t bb = 0; uint32_t bc = 0;                // bit buffer: bc valid bits, the next one lowest
    uint64_t wi = 0;                                 // the next input word (4 bytes) the bit buffer takes
    uint64_t ibase = 0;                              // the window holds in[ibase, ibase + INF_INBUF), a multiple of 4
    uint64_t pos = 0, flushed = 0, crcDone = 0, memberStart = 0;
    uint32_t crc = 0;

    __device__ __forceinline__ Inf(InfShared &s, const uint8_t *i, uint64_t il, uint8_t *o, uint64_t oc)
        : S(s), in(i), inLen(il), out(o), outCap(oc), bias((uint32_t) ((uintptr_t) o & 15u)) {}

    __device__ __forceinline__ uint32_t ridx(uint64_t p) const { return ((uint32_t) p + bias) & INF_RMASK; }

    // ---- input
    __device__ void load_window(uint64_t at) {
        ibase = at & ~(uint64_t) 3;
        INF_SYNC();
        for (uint32_t base = 0; base < INF_INBUF; base += INF_WAVE * 16)
            INF_LANES_DO(lane) {
                const uint32_t k = base + lane * 16;
                const uint64_t g = ibase + k;
                uint4 v = {0, 0, 0, 0};
                const bool whole = g < inLen && inLen - g >= 16;
                if (whole) memcpy(&v, in + g, 16);
                *(uint4 *) (S.inbuf + k) = v;
                if (!whole)
                    for (uint32_t j = 0; j < 16 && g + j < inLen; j++) S.inbuf[k + j] = in[g + j];
            }
        INF_SYNC();
    }
    __device__ __forceinline__ uint32_t next_word() {
        const uint64_t b = wi * 4;
        if (b - ibase >= INF_INBUF) load_window(b);
        const uint32_t w = *(const uint32_t *) (S.inbuf + (uint32_t) (b - ibase));
        wi++;
        return INF_UNI(w);
    }
    __device__ __forceinline__ void refill() {       // afterwards bc >= 33
        if (bc <= 32) { bb |= (uint64_t) next_word() << bc; bc += 32; }
    }
    __device__ __forceinline__ uint32_t take(uint32_t n) {    // n <= bc, n < 32
        const uint32_t v = (uint32_t) bb & ((1u << n) - 1u);
        bb >>= n; bc -= n;
        return v;
    }
    __device__ __forceinline__ uint64_t bitpos() const { return wi * 32 - bc; }       // bits of the input consumed
    __device__ __forceinline__ bool overrun() const { return bitpos() > inLen * 8; }
    __device__ __forceinline__ uint64_t byte_pos() {          // drops the rest of the current byte
        const uint32_t r = bc & 7u;
        bb >>= r; bc -= r;
        return bitpos() >> 3;
    }
    __device__ __forceinline__ void seek_byte(uint64_t bp) {
        wi = bp >> 2;
        const uint32_t sh = 8u * (uint32_t) (bp & 3u);
        bb = (uint64_t) (next_word() >> sh);
        bc = 32 - sh;
    }
    __device__ __forceinline__ uint32_t in_byte(uint64_t bp) {   // bp < inLen
        if (bp - ibase >= INF_INBUF) load_window(bp);
        return INF_UNI((uint32_t) S.inbuf[(uint32_t) (bp - ibase)]);
    }

    // ---- output
    __device__ __forceinline__ uint64_t low() const { return flushed < crcDone ? flushed : crcDone; }

    __device__ void crc_span(uint64_t from, uint64_t to) {       // the ring's bytes [from, to) into crc
        while (to - from >= INF_CL) {
            const uint64_t whole = (to - from) / INF_CL;
            const uint32_t n = whole < INF_WAVE ? (uint32_t) whole : INF_WAVE;
            INF_SYNC();
            INF_LANES_DO(lane) {
                if (lane < n) {
                    uint32_t r = 0;
                    const uint64_t q = from + (uint64_t) lane * INF_CL;
                    for (uint32_t k = 0; k < INF_CL; k++) r = S.crcTab[(r ^ S.ring[ridx(q + k)]) & 255u] ^ (r >> 8);
                    S.red[lane] = inf_mulmod(r, S.crcK[n - 1 - lane]);
                }
            }
            INF_SYNC();
            uint32_t acc = inf_mulmod(crc, INF_UNI(S.crcK[n]));
            for (uint32_t i = 0; i < n; i++) acc ^= INF_UNI(S.red[i]);
            crc = acc;
            from += (uint64_t) n * INF_CL;
        }
        INF_SYNC();                                              // (the tail's bytes were written by the first lane or by a copy's lanes)
        for (; from < to; from++) crc = INF_UNI(S.crcTab[(crc ^ S.ring[ridx(from)]) & 255u]) ^ (crc >> 8);
    }

    __device__ void flush(bool final) {                          // the ring's bytes [flushed, pos) to HBM; !final: up to the last 16-byte boundary
        const uint64_t A = flushed + bias, B = pos + bias;       // (positions counted from out's 16-byte boundary)
        const uint64_t up = (A + 15) & ~(uint64_t) 15, a1 = up < B ? up : B;
        uint64_t done = a1;
        INF_SYNC();
        INF_LANES_DO(lane) {
            const uint64_t i = A + lane;
            if (lane < 16 && i < a1) out[i - bias] = S.ring[(uint32_t) i & INF_RMASK];
        }
        if (a1 < B) {
            const uint64_t b0 = B & ~(uint64_t) 15;              // a1 is a boundary here, so a1 <= b0
            INF_LANES_DO(lane) {
                for (uint64_t v = a1 + (uint64_t) lane * 16; v < b0; v += INF_WAVE * 16)
                    *(uint4 *) (out + (v - bias)) = *(const uint4 *) (S.ring + ((uint32_t) v & INF_RMASK));
            }
            done = b0;
            if (final) {
                INF_LANES_DO(lane) {
                    const uint64_t i = b0 + lane;
                    if (lane < 16 && i < B) out[i - bias] = S.ring[(uint32_t) i & INF_RMASK];
                }
                done = B;
            }
        }
        flushed = done - bias;
        INF_SYNC();
    }

    __device__ __forceinline__ void drain() {        // afterwards pos - low() < INF_DRAIN
        while (pos - crcDone >= INF_DRAIN) { crc_span(crcDone, crcDone + INF_DRAIN); crcDone += INF_DRAIN; }
        flush(false);
    }

    // ---- codes
    // lens[0, n) -> C; fast: the table's index bits; codes: the code-length code, which may not be incomplete at all
    __device__ bool build(InfCode &C, const uint8_t *lens, uint32_t n, uint32_t fast, bool codes) {
        INF_SYNC();
        INF_LANES_DO(lane) {
            if (lane < 16) {
                uint32_t c = 0;
                if (lane) for (uint32_t s = 0; s < n; s++) c += lens[s] == lane;
                C.cnt[lane] = (uint16_t) c;
            }
            for (uint32_t j = lane; j < (1u << fast); j += INF_WAVE) C.tab[j] = 0;
        }
        INF_SYNC();
        int32_t left = 1;
        uint32_t max = 0;
        for (uint32_t l = 1; l <= 15; l++) {
            const uint32_t c = INF_UNI((uint32_t) C.cnt[l]);
            left = (left << 1) - (int32_t) c;
            if (left < 0) return false;                          // over-subscribed
            if (c) max = l;
        }
        if (left > 0 && max != 0 && (codes || max != 1)) return false;   // incomplete (zlib's inflate_table: max == 0 passes, and then no symbol decodes)
        INF_LANES_DO(lane) {
            if (lane >= 1 && lane <= 15) {
                uint32_t code = 0, off = 0;
                for (uint32_t k = 1; k < lane; k++) { code = (code + C.cnt[k]) << 1; off += C.cnt[k]; }
                for (uint32_t s = 0; s < n; s++) {
                    if (lens[s] != lane) continue;
                    C.sorted[off++] = (uint16_t) s;
                    if (lane <= fast) {
                        const uint16_t e = (uint16_t) (s | lane << 9);
                        for (uint32_t j = inf_bitrev(code, lane); j < (1u << fast); j += 1u << lane) C.tab[j] = e;
                    }
                    code++;
                }
            }
        }
        INF_SYNC();
        return true;
    }
    // the next symbol of C, or -1 when the bits are no code of it; takes at most 15 bits (bc >= 15)
    __device__ __forceinline__ int32_t decode(const InfCode &C, uint32_t fast) {
        const uint32_t e = INF_UNI((uint32_t) C.tab[(uint32_t) bb & ((1u << fast) - 1u)]);
        if (e) { const uint32_t l = e >> 9; bb >>= l; bc -= l; return (int32_t) (e & 511u); }
        int32_t code = 0, first = 0, index = 0;
        for (uint32_t len = 1; len <= 15; len++) {
            code |= (int32_t) take(1);
            const int32_t count = (int32_t) INF_UNI((uint32_t) C.cnt[len]);
            if (code - count < first) return (int32_t) INF_UNI((uint32_t) C.sorted[index + (code - first)]);
            index += count; first += count;
            first <<= 1; code <<= 1;
        }
        return -1;
    }

    // ---- blocks
    __device__ int stored() {
        uint64_t bp = byte_pos();
        if (bp > inLen || inLen - bp < 4) return INF_EDATA;
        const uint32_t len = in_byte(bp) | in_byte(bp + 1) << 8, nlen = in_byte(bp + 2) | in_byte(bp + 3) << 8;
        if ((len ^ nlen) != 0xffffu) return INF_EDATA;
        bp += 4;
        if (len > inLen - bp) return INF_EDATA;
        if (len > outCap - pos) return INF_ESHORT;
        uint32_t left = len;
        while (left) {
            if (bp - ibase >= INF_INBUF) load_window(bp);
            const uint32_t at = (uint32_t) (bp - ibase), room = INF_INBUF - at, n = left < room ? left : room;   // 1 <= n <= INF_INBUF
            if (pos - low() >= INF_DRAIN) drain();
            INF_SYNC();
            for (uint32_t base = 0; base < n; base += INF_WAVE)
                INF_LANES_DO(lane) {
                    const uint32_t i = base + lane;
                    if (i < n) S.ring[ridx(pos + i)] = S.inbuf[at + i];
                }
            INF_SYNC();
            pos += n; bp += n; left -= n;
        }
        seek_byte(bp);
        return INF_OK;
    }

    __device__ int dynamic_header() {
        refill();
        const uint32_t hlit = take(5) + 257, hdist = take(5) + 1, hclen = take(4) + 4;
        if (hlit > 286 || hdist > 30) return INF_EDATA;
        INF_SYNC();
        INF_LANES_DO(lane) { if (lane < 19) S.lens[lane] = 0; }
        INF_SYNC();
        for (uint32_t i = 0; i < hclen; i++) {
            refill();
            const uint32_t l = take(3);
            if (INF_LANE0) S.lens[INF_ORDER[i]] = (uint8_t) l;
        }
        if (overrun()) return INF_EDATA;
        if (!build(S.dist, S.lens, 19, INF_CFAST, true)) return INF_EDATA;
        const uint32_t total = hlit + hdist;
        uint32_t idx = 0;
        while (idx < total) {
            refill();
            const int32_t sym = decode(S.dist, INF_CFAST);
            if (sym < 0) return INF_EDATA;
            if (sym < 16) {
                if (INF_LANE0) S.lens[idx] = (uint8_t) sym;
                idx++;
            } else {
                uint32_t prev = 0, rep;
                if (sym == 16) {
                    if (idx == 0) return INF_EDATA;              // nothing to repeat
                    prev = INF_UNI((uint32_t) S.lens[idx - 1]);
                    rep = 3 + take(2);
                } else if (sym == 17) rep = 3 + take(3);
                else rep = 11 + take(7);
                if (rep > total - idx) return INF_EDATA;
                for (uint32_t base = 0; base < rep; base += INF_WAVE)
                    INF_LANES_DO(lane) { if (base + lane < rep) S.lens[idx + base + lane] = (uint8_t) prev; }
                INF_SYNC();                                      // (the next repeat reads the last of these from another lane)
                idx += rep;
            }
            if (overrun()) return INF_EDATA;
        }
        INF_SYNC();
        if (INF_UNI((uint32_t) S.lens[256]) == 0) return INF_EDATA;   // no end-of-block code
        if (!build(S.lit, S.lens, hlit, INF_LFAST, false)) return INF_EDATA;
        if (!build(S.dist, S.lens + hlit, hdist, INF_DFAST, false)) return INF_EDATA;
        return INF_OK;
    }

    __device__ void fixed_header() {
        INF_SYNC();
        INF_LANES_DO(lane) {
            for (uint32_t s = lane; s < 320; s += INF_WAVE) S.lens[s] = (uint8_t) (s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        }
        (void) build(S.lit, S.lens, 288, INF_LFAST, false);
        (void) build(S.dist, S.lens + 288, 32, INF_DFAST, false);   // (30 and 31 decode and are refused where they are met)
    }

    __device__ int symbols() {                                    // the block's symbols up to its end-of-block
        for (;;) {
            if (pos - low() >= INF_DRAIN) drain();
            refill();
            const int32_t sym = decode(S.lit, INF_LFAST);
            if (sym < 0) return INF_EDATA;
            if (sym < 256) {
                if (pos >= outCap) return INF_ESHORT;
                if (INF_LANE0) S.ring[ridx(pos)] = (uint8_t) sym;
                pos++;
            } else if (sym == 256) {
                return overrun() ? INF_EDATA : INF_OK;
            } else {
                if (sym > 285) return INF_EDATA;
                const uint32_t lc = (uint32_t) sym - 257;
                uint32_t len;
                if (lc < 8) len = 3 + lc;
                else if (lc == 28) len = 258;
                else { const uint32_t eb = (lc >> 2) - 1; len = 3 + ((4 + (lc & 3u)) << eb) + take(eb); }
                refill();
                const int32_t ds = decode(S.dist, INF_DFAST);
                if (ds < 0 || ds > 29) return INF_EDATA;
                uint32_t d;
                if (ds < 4) d = 1 + (uint32_t) ds;
                else { const uint32_t eb = ((uint32_t) ds >> 1) - 1; d = 1 + ((2 + ((uint32_t) ds & 1u)) << eb) + take(eb); }
                if (overrun()) return INF_EDATA;
                if (d > pos - memberStart) return INF_EDATA;     // reaches in front of the member
                if (len > outCap - pos) return INF_ESHORT;
                INF_SYNC();
                for (uint32_t base = 0; base < len; base += INF_WAVE)
                    INF_LANES_DO(lane) {
                        const uint32_t i = base + lane;
                        if (i < len) S.ring[ridx(pos + i)] = S.ring[ridx(pos - d + (d >= len ? i : d == 1 ? 0 : i % d))];
                    }
                INF_SYNC();
                pos += len;
            }
            if (overrun()) return INF_EDATA;
        }
    }

    __device__ int blocks() {
        for (;;) {
            refill();
            const uint32_t last = take(1), type = take(2);
            if (overrun()) return INF_EDATA;
            int st;
            if (type == 0) st = stored();
            else if (type == 1) { fixed_header(); st = symbols(); }
            else if (type == 2) { st = dynamic_header(); if (st == INF_OK) st = symbols(); }
            else st = INF_EDATA;
            if (st != INF_OK) return st;
            if (last) return INF_OK;
        }
    }

    // ---- members (RFC 1952)
    __device__ int member_header(uint64_t &bp) {
        if (inLen - bp < 18) return INF_EDATA;                   // ten bytes of header, eight of trailer
        const uint64_t start = bp;
        if (in_byte(bp) != 0x1f || in_byte(bp + 1) != 0x8b || in_byte(bp + 2) != 8) return INF_EDATA;
        const uint32_t flg = in_byte(bp + 3);
        if (flg & 0xe0u) return INF_EDATA;
        bp += 10;
        if (flg & 4u) {                                          // FEXTRA
            if (inLen - bp < 2) return INF_EDATA;
            const uint32_t xlen = in_byte(bp) | in_byte(bp + 1) << 8;
            bp += 2;
            if (xlen > inLen - bp) return INF_EDATA;
            bp += xlen;
        }
        for (uint32_t field = 8u; field <= 16u; field <<= 1) {   // FNAME, FCOMMENT
            if (!(flg & field)) continue;
            for (;;) {
                if (bp >= inLen) return INF_EDATA;
                if (in_byte(bp++) == 0) break;
            }
        }
        if (flg & 2u) {                                          // FHCRC
            if (inLen - bp < 2) return INF_EDATA;
            uint32_t r = 0xffffffffu;
            for (uint64_t q = start; q < bp; q++) r = INF_UNI(S.crcTab[(r ^ in_byte(q)) & 255u]) ^ (r >> 8);
            const uint32_t want = in_byte(bp) | in_byte(bp + 1) << 8;
            bp += 2;
            if ((~r & 0xffffu) != want) return INF_ECHECK;
        }
        return INF_OK;
    }

    __device__ InfResult run() {
        InfResult R = {INF_EDATA, 0, 0, 0};
        INF_LANES_DO(lane) {
            for (uint32_t j = lane; j < 256; j += INF_WAVE) {
                uint32_t c = j;
                for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ INF_POLY : c >> 1;
                S.crcTab[j] = c;
            }
            S.crcK[lane] = inf_xpow8(INF_CL * lane);
            if (lane == 0) S.crcK[INF_WAVE] = inf_xpow8(INF_CL * INF_WAVE);
        }
        load_window(0);
        uint64_t bp = 0;
        do {
            int st = member_header(bp);
            if (st == INF_OK) {
                memberStart = crcDone = pos;
                crc = 0xffffffffu;
                seek_byte(bp);
                st = blocks();
            }
            if (st == INF_OK) {
                bp = byte_pos();
                if (bp > inLen || inLen - bp < 8) st = INF_EDATA;
            }
            if (st != INF_OK) { R.status = st; R.inUsed = bp; return R; }
            crc_span(crcDone, pos);
            crcDone = pos;
            const uint32_t wantCrc = in_byte(bp) | in_byte(bp + 1) << 8 | in_byte(bp + 2) << 16 | in_byte(bp + 3) << 24;
            const uint32_t wantLen = in_byte(bp + 4) | in_byte(bp + 5) << 8 | in_byte(bp + 6) << 16 | in_byte(bp + 7) << 24;
            bp += 8;
            R.inUsed = bp;
            if (~crc != wantCrc || (uint32_t) (pos - memberStart) != wantLen) { R.status = INF_ECHECK; return R; }
            R.members++;
        } while (bp < inLen);
        flush(true);
        R.status = INF_OK; R.outLen = pos;
        return R;
    }
};
