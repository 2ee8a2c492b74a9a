// gzip deflate for text in HBM (included by fasta_input.hip, inside namespace fa): mbgc_fasta_deflate_dev's encoder, one chunk of
// DEF_CHUNK text bytes per wave, and its pack step. Kept free of HIP calls like fasta_inflate.h, so that the same text compiles as
// plain C++: tests/fasta_deflate_emu.cpp runs it on the CPU under AddressSanitizer. The includer spells the wave with the macros of
// fasta_inflate.h (INF_LANES_DO, INF_LANE0, INF_SYNC, INF_UNI, INF_CONST) and four more:
//   DEF_ATOMIC_ADD / _OR / _MAX(p, v)   on a 32-bit word of LDS (the CPU: the plain operation, the lanes run one after the other)
//   DEF_EXSCAN(arr)                     arr[0, 64) in LDS -> its exclusive prefix sums, in place; the value is the total (a wave scan)
//
// The encoder chooses its own block boundaries, so a chunk depends on nothing in front of it: no back-reference crosses its start,
// it ends on a byte boundary (an empty stored block, as a full flush of zlib ends; the job's last chunk sets BFINAL and pads), and
// the chunks of a job laid end to end are one DEFLATE stream. Per chunk, in this order:
//   text     loaded into LDS (16 bytes per lane where a whole vector lies inside the chunk), its CRC-32 by the lane-parallel fold
//   matches  one candidate per position: the most recent EARLIER TILE's position whose 8 bytes hash alike (LDS table of position and
//            16 check bits, updated by atomicMax tile by tile in position order, so that no lane scheduling shows), and the distance
//            of the last match taken (the period of a run locks in); extended byte by byte to 258; taken from DEF_MIN_MATCH.
//            The greedy parse is a walk over a 64-bit mask of the tile's candidates: one step per match TAKEN, none for a tile of
//            literals. A match is kept in the slot of the 8 bytes it starts in (matches are >= 8 long: one start per slot), the
//            positions where a token starts in a bitmap; tokens are never stored
//   counts   exact histograms of the 286 + 30 symbols, filled as the walk settles them
//   lengths  code_lengths(): symbols ranked by the wave, Moffat-Katajainen's in-place Huffman over the used ones in one lane, the
//            limit enforced on the per-length counts so that the Kraft sum stays exactly 1 (the rule zlib and miniz share), at least
//            two symbols coded. Canonical codes: one lane per length
//   block    dynamic (RFC 1951 3.2.7, the lengths run-length coded with 16/17/18) unless its bits are not fewer than the text's:
//            then stored. The text of no bytes: an empty fixed block
//   emit     the text is read from HBM a second time (LDS now stages the output): per tile every lane takes the bits of its token,
//            a wave prefix sum places them, they are ORed into the staging area; at the end that area goes to the chunk's slot in
//            16-byte vector stores between a head and a tail written singly
// LDS: text / staging 32 KiB, match slots 16 KiB, hash table 8 KiB (dead after the matches: the code builder's workspace), token
// bitmap 4 KiB, histograms, codes and the wave's exchange arrays: static_assert below holds it under 64 KiB.
#include "fasta_gzip_common.h"

#ifndef DEF_MIN_MATCH
#define DEF_MIN_MATCH 8                              // EXPERIMENTS.md: 8, 12 and 16 over the corpus of tests/_deflate_cases.py
#endif
constexpr uint32_t DEF_WAVE = 64;
constexpr uint32_t DEF_CHUNK = 32768;                // MBGC_DEFLATE_CHUNK
constexpr uint32_t DEF_SLOT = DEF_CHUNK + 64;        // a chunk's place in the staging buffer (stored form + flush block: DEF_CHUNK + 10)
constexpr uint32_t DEF_MAX_MATCH = 258;
constexpr uint32_t DEF_HBITS = 11;
constexpr uint32_t DEF_NLIT = 286, DEF_NDIST = 30, DEF_NCL = 19;
constexpr uint32_t DEF_CRC_PER = DEF_CHUNK / DEF_WAVE;   // bytes per lane of the CRC
constexpr uint32_t DEF_STORED = 0x80000000u;         // DefChunkOut::bytes: the chunk went out stored
static_assert(DEF_MIN_MATCH >= 8 && DEF_MIN_MATCH <= DEF_MAX_MATCH, "one match start per 8-byte slot");

struct DefChunk { uint64_t inOff; uint32_t n, last; };            // text[inOff, inOff + n); last: its job's last chunk
struct DefChunkOut { uint32_t bytes, crc; };                      // what the chunk wrote into its slot (| DEF_STORED); the CRC-32 of its text
struct DefPackIn { uint64_t dst; uint32_t job, flags; };          // where the chunk goes; flags 1: its job's first, 2: its last
struct DefJobIn { uint64_t inLen; uint32_t chunk0, nchunks; };

INF_CONST const uint8_t DEF_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
INF_CONST const uint8_t DEF_GZ_HEADER[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};

struct DefBuild {                                                 // the code builder's workspace
    uint32_t freq[288], A[288];
    uint16_t sym[288];
    uint32_t cnt[16];
    uint8_t seq[320];                                             // the two alphabets' lengths as the header carries them
    uint16_t hs[320];                                             // ... run-length coded: symbol | extra bits << 8
};

struct DefShared {
    alignas(16) uint8_t text[16 + DEF_CHUNK + 64];                // the text at its address modulo 16; then the output, likewise
    union {
        uint32_t hash[1u << DEF_HBITS];                           // (position + 1) << 16 | 16 more bits of the hash; 0: empty
        struct { uint32_t tab[256], red[DEF_WAVE]; } crc;
        DefBuild b;
    } u;
    uint32_t match[DEF_CHUNK / 8];                                // start & 7 | length << 3 | distance << 12; 0: none starts here
    uint32_t tok[DEF_CHUNK / 32];                                 // bit p: a token starts at p
    uint32_t litHist[288], distHist[32], clHist[20];
    uint16_t litCode[288], distCode[32], clCode[20];
    uint8_t litLen[288], distLen[32], clLen[20];
    uint64_t ev[DEF_WAVE];                                        // a tile's bits per lane
    uint32_t scan[DEF_WAVE], cand[DEF_WAVE];
    uint32_t mask[2], nused, hdr[4];
};
static_assert(sizeof(DefShared) <= 65536, "two chunks per CU");
static_assert(sizeof(DefBuild) <= sizeof(uint32_t) << DEF_HBITS, "the workspace lives where the hash table was");

__device__ __forceinline__ uint64_t def_low(uint32_t k) { return k >= 64 ? ~(uint64_t) 0 : ((uint64_t) 1 << k) - 1; }   // the k lowest bits
__device__ __forceinline__ uint32_t def_log2(uint32_t v) { return 31u - (uint32_t) __builtin_clz(v); }                 // v > 0
__device__ __forceinline__ uint32_t def_ctz64(uint64_t v) { return (uint32_t) __builtin_ctzll(v); }                    // v != 0
// a match length (3..258) -> its symbol's number behind 257, its extra bits and their count
__device__ __forceinline__ void def_len_sym(uint32_t len, uint32_t &lc, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - 3;
    if (len == DEF_MAX_MATCH) { lc = 28; eb = 0; ev = 0; }
    else if (l < 8) { lc = l; eb = 0; ev = 0; }
    else { eb = def_log2(l) - 2; lc = (eb + 1) * 4 + ((l >> eb) & 3u); ev = l & ((1u << eb) - 1u); }
}
__device__ __forceinline__ void def_dist_sym(uint32_t dist, uint32_t &ds, uint32_t &eb, uint32_t &ev) {      // 1..32768
    const uint32_t x = dist - 1;
    if (x < 4) { ds = x; eb = 0; ev = 0; }
    else { eb = def_log2(x) - 1; ds = 2 * (eb + 1) + ((x >> eb) & 1u); ev = x & ((1u << eb) - 1u); }
}
__device__ __forceinline__ uint32_t def_len_extra(uint32_t lc) { return lc < 8 || lc == 28 ? 0 : (lc >> 2) - 1; }
__device__ __forceinline__ uint32_t def_dist_extra(uint32_t ds) { return ds < 4 ? 0 : (ds >> 1) - 1; }
__device__ __forceinline__ uint32_t def_cl_extra(uint32_t s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }

struct Def {
    DefShared &S;
    const uint8_t *in; uint32_t n; bool last;        // the chunk's text: in[0, n)
    uint8_t *slot;                                   // its output: slot[0, DEF_SLOT)
    uint8_t *tx;                                     // in[i] in LDS: tx[i]
    uint32_t bitpos = 0;                             // the next output bit, counted from S.text
    uint32_t crc = 0;

    __device__ __forceinline__ Def(DefShared &s, const uint8_t *i, uint32_t len, bool l, uint8_t *o)
        : S(s), in(i), n(len), last(l), slot(o), tx(s.text + ((uintptr_t) i & 15u)) {}

    // ---- the text and its CRC-32
    __device__ void load_text() {
        const uint32_t bias = (uint32_t) (tx - S.text), span = bias + n;
        for (uint32_t base = 0; base < span; base += DEF_WAVE * 16)
            INF_LANES_DO(lane) {
                const uint32_t j = base + lane * 16;
                if (j >= bias && j + 16 <= span) *(uint4 *) (S.text + j) = *(const uint4 *) (in + (j - bias));
                else for (uint32_t k = j < bias ? bias : j; k < j + 16 && k < span; k++) S.text[k] = in[k - bias];
            }
        INF_SYNC();
    }
    __device__ void text_crc() {
        INF_LANES_DO(lane) {
            for (uint32_t j = lane; j < 256; j += DEF_WAVE) {
                uint32_t c = j;
                for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ INF_POLY : c >> 1;
                S.u.crc.tab[j] = c;
            }
        }
        INF_SYNC();
        INF_LANES_DO(lane) {
            const uint32_t a = lane * DEF_CRC_PER, e = a + DEF_CRC_PER < n ? a + DEF_CRC_PER : n;
            uint32_t r = 0;
            for (uint32_t k = a; k < e; k++) r = S.u.crc.tab[(r ^ tx[k]) & 255u] ^ (r >> 8);
            S.u.crc.red[lane] = a < e ? inf_mulmod(r, inf_xpow8(n - e)) : 0;
        }
        INF_SYNC();
        uint32_t acc = inf_mulmod(0xffffffffu, inf_xpow8(n));
        for (uint32_t i = 0; i < DEF_WAVE; i++) acc ^= INF_UNI(S.u.crc.red[i]);
        crc = ~acc;
        INF_SYNC();
    }

    // ---- matches
    __device__ __forceinline__ uint32_t hash_key(uint32_t p, uint32_t &idx) const {      // p + 8 <= n -> the entry's low half
        uint32_t a, b;
        memcpy(&a, tx + p, 4); memcpy(&b, tx + p + 4, 4);
        const uint32_t h = (a * 2654435761u + b) * 2246822519u;
        idx = h >> (32 - DEF_HBITS);
        return (h >> 4) & 0xffffu;
    }
    __device__ __forceinline__ uint32_t extend(uint32_t q, uint32_t p, uint32_t maxLen) const {   // q < p
        uint32_t l = 0;
        while (l < maxLen && tx[q + l] == tx[p + l]) l++;
        return l;
    }
    __device__ void clear() {
        INF_LANES_DO(lane) {
            for (uint32_t j = lane; j < (1u << DEF_HBITS); j += DEF_WAVE) S.u.hash[j] = 0;
            for (uint32_t j = lane; j < DEF_CHUNK / 8; j += DEF_WAVE) S.match[j] = 0;
            for (uint32_t j = lane; j < DEF_CHUNK / 32; j += DEF_WAVE) S.tok[j] = 0;
            for (uint32_t j = lane; j < 288; j += DEF_WAVE) S.litHist[j] = 0;
            if (lane < 32) S.distHist[lane] = 0;
            if (lane < 20) S.clHist[lane] = 0;
            if (lane < 2) S.mask[lane] = 0;
        }
        INF_SYNC();
    }
    __device__ void find_matches() {
        uint32_t cov = 0, rep = 0;                   // the parse has settled [0, cov); the last taken match's distance
        for (uint32_t base = 0; base < n; base += DEF_WAVE) {
            const uint32_t end = base + DEF_WAVE < n ? base + DEF_WAVE : n;
            if (cov < end) {
                INF_LANES_DO(lane) {
                    const uint32_t p = base + lane;
                    uint32_t bestLen = 0, bestDist = 0;
                    if (p >= cov && p < n && n - p >= DEF_MIN_MATCH) {
                        const uint32_t maxLen = n - p < DEF_MAX_MATCH ? n - p : DEF_MAX_MATCH;
                        if (rep && rep <= p) {
                            const uint32_t l = extend(p - rep, p, maxLen);
                            if (l >= DEF_MIN_MATCH) { bestLen = l; bestDist = rep; }
                        }
                        if (bestLen < maxLen) {
                            uint32_t idx;
                            const uint32_t tag = hash_key(p, idx), e = S.u.hash[idx];
                            if (e && (e & 0xffffu) == tag) {
                                const uint32_t q = (e >> 16) - 1, l = extend(q, p, maxLen);
                                if (l >= DEF_MIN_MATCH && l > bestLen) { bestLen = l; bestDist = p - q; }
                            }
                        }
                    }
                    S.cand[lane] = bestLen | bestDist << 16;
                    if (bestLen) DEF_ATOMIC_OR(&S.mask[lane >> 5], 1u << (lane & 31u));
                }
                INF_SYNC();
                // the greedy parse of this tile: the same in every lane
                const uint32_t at = cov > base ? cov - base : 0;                      // (< 64: cov < end)
                uint64_t covered = def_low(at), starts = 0;
                uint64_t m = ((uint64_t) INF_UNI(S.mask[0]) | (uint64_t) INF_UNI(S.mask[1]) << 32) & ~covered;
                while (m) {
                    const uint32_t i = def_ctz64(m), c = INF_UNI(S.cand[i]), len = c & 0xffffu, dist = c >> 16, s = base + i;
                    starts |= (uint64_t) 1 << i;
                    covered |= def_low(i + len) & ~def_low(i + 1);
                    if (INF_LANE0) {
                        uint32_t lc, ds, eb, ev;
                        def_len_sym(len, lc, eb, ev); def_dist_sym(dist, ds, eb, ev);
                        S.match[s >> 3] = (s & 7u) | len << 3 | dist << 12;
                        S.litHist[257 + lc]++; S.distHist[ds]++;
                    }
                    cov = s + len; rep = dist;
                    m &= ~def_low(i + len);
                }
                const uint64_t tokm = ~covered & def_low(end - base);
                if (INF_LANE0) {
                    S.tok[base >> 5] = (uint32_t) tokm; S.tok[(base >> 5) + 1] = (uint32_t) (tokm >> 32);
                    S.mask[0] = 0; S.mask[1] = 0;
                }
                INF_LANES_DO(lane) {
                    if ((tokm & ~starts) >> lane & 1u) DEF_ATOMIC_ADD(&S.litHist[tx[base + lane]], 1u);
                }
            }
            INF_SYNC();
            INF_LANES_DO(lane) {                                                       // this tile's positions are candidates from the next tile on
                const uint32_t p = base + lane;
                if (p < n && n - p >= 8) {
                    uint32_t idx;
                    const uint32_t tag = hash_key(p, idx);
                    DEF_ATOMIC_MAX(&S.u.hash[idx], (p + 1) << 16 | tag);
                }
            }
            INF_SYNC();
        }
    }

    // ---- code lengths
    // hist[0, nsym) -> lens[0, nsym): a complete prefix code (Kraft sum exactly 1) of at most `limit` bits over the symbols that
    // occur, and over at least two symbols whatever occurs. nsym <= 288, 2^limit >= nsym. Uses S.u.b.
    __device__ void code_lengths(const uint32_t *hist, uint32_t nsym, uint32_t limit, uint8_t *lens) {
        DefBuild &B = S.u.b;
        INF_SYNC();
        INF_LANES_DO(lane) {
            uint32_t c = 0;
            for (uint32_t s = lane; s < nsym; s += DEF_WAVE) { const uint32_t f = hist[s]; B.freq[s] = f; lens[s] = 0; c += f != 0; }
            S.scan[lane] = c;
            if (lane < 16) B.cnt[lane] = 0;
        }
        INF_SYNC();
        uint32_t m = DEF_EXSCAN(S.scan);
        INF_SYNC();
        if (m < 2) {                                                                   // zlib's rule: the lowest unused symbols join with count 1
            if (INF_LANE0) {
                uint32_t have = m;
                for (uint32_t s = 0; s < nsym && have < 2; s++) if (!B.freq[s]) { B.freq[s] = 1; have++; }
            }
            m = 2;
            INF_SYNC();
        }
        INF_LANES_DO(lane) {                                                           // rank by (count, symbol) among the used ones
            for (uint32_t s = lane; s < nsym; s += DEF_WAVE) {
                const uint32_t f = B.freq[s];
                if (!f) continue;
                uint32_t r = 0;
                for (uint32_t t = 0; t < nsym; t++) { const uint32_t g = B.freq[t]; r += g != 0 && (g < f || (g == f && t < s)); }
                B.A[r] = f; B.sym[r] = (uint16_t) s;
            }
        }
        INF_SYNC();
        if (INF_LANE0) {
            uint32_t *A = B.A;
            // Moffat & Katajainen, in place: A[0, m) ascending counts -> code lengths, descending
            A[0] += A[1];
            uint32_t root = 0, leaf = 2;
            for (uint32_t next = 1; next + 1 < m; next++) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
            }
            A[m - 2] = 0;
            for (uint32_t next = m - 2; next-- > 0;) A[next] = A[A[next]] + 1;
            {
                int32_t avbl = 1, used = 0, r = (int32_t) m - 2, nx = (int32_t) m - 1;
                uint32_t dpth = 0;
                while (avbl > 0) {
                    while (r >= 0 && A[r] == dpth) { used++; r--; }
                    while (avbl > used) { A[nx--] = dpth; avbl--; }
                    avbl = 2 * used; dpth++; used = 0;
                }
            }
            // the limit, on the per-length counts: every step takes one unit of 2^-limit off the Kraft sum and keeps the number of codes
            uint32_t total = 0;
            for (uint32_t i = 0; i < m; i++) B.cnt[A[i] < limit ? A[i] : limit]++;
            for (uint32_t l = 1; l <= limit; l++) total += B.cnt[l] << (limit - l);
            while (total != 1u << limit) {
                B.cnt[limit]--;
                for (uint32_t l = limit - 1; l > 0; l--)
                    if (B.cnt[l]) { B.cnt[l]--; B.cnt[l + 1] += 2; break; }
                total--;
            }
            uint32_t i = 0;                                                            // the rarest symbols take the longest codes
            for (uint32_t l = limit; l > 0; l--)
                for (uint32_t k = B.cnt[l]; k; k--) lens[B.sym[i++]] = (uint8_t) l;
        }
        INF_SYNC();
    }
    // the canonical codes of lens[0, nsym), bit-reversed (DEFLATE packs Huffman codes from their first bit): one lane per length
    __device__ void assign_codes(const uint8_t *lens, uint32_t nsym, uint16_t *codes) {
        DefBuild &B = S.u.b;
        INF_SYNC();
        INF_LANES_DO(lane) {
            if (lane < 16) {
                uint32_t c = 0;
                if (lane) for (uint32_t s = 0; s < nsym; s++) c += lens[s] == lane;
                B.cnt[lane] = c;
            }
        }
        INF_SYNC();
        INF_LANES_DO(lane) {
            if (lane >= 1 && lane <= 15) {
                uint32_t code = 0;
                for (uint32_t k = 1; k < lane; k++) code = (code + B.cnt[k]) << 1;
                for (uint32_t s = 0; s < nsym; s++)
                    if (lens[s] == lane) codes[s] = (uint16_t) inf_bitrev(code++, lane);
            }
        }
        INF_SYNC();
    }

    // ---- output bits
    __device__ __forceinline__ void or_bits(uint32_t bp, uint64_t v) {                 // v's bits from output bit bp on (v < 2^56)
        uint32_t *W = (uint32_t *) S.text;
        const uint32_t w = bp >> 5, s = bp & 31u, lo = (uint32_t) v, hi = (uint32_t) (v >> 32);
        const uint32_t x0 = lo << s, x1 = s ? lo >> (32 - s) | hi << s : hi, x2 = s ? hi >> (32 - s) : 0;
        if (x0) DEF_ATOMIC_OR(W + w, x0);
        if (x1) DEF_ATOMIC_OR(W + w + 1, x1);
        if (x2) DEF_ATOMIC_OR(W + w + 2, x2);
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t nbits) {                  // the whole wave's: one lane writes
        if (INF_LANE0) or_bits(bitpos, v);
        bitpos += nbits;
    }
    __device__ __forceinline__ void pad_to_byte() { bitpos = (bitpos + 7u) & ~7u; }
    __device__ void place_tile() {                                                    // S.ev / S.scan of every lane -> the output
        INF_SYNC();
        const uint32_t total = DEF_EXSCAN(S.scan);
        INF_SYNC();
        INF_LANES_DO(lane) {
            const uint64_t v = S.ev[lane];
            if (v) or_bits(bitpos + S.scan[lane], v);
        }
        INF_SYNC();
        bitpos += total;
    }

    // ---- the block
    __device__ bool build_dynamic(uint32_t &hlit, uint32_t &hdist, uint32_t &hclen, uint32_t &nh) {   // false: stored is no larger
        DefBuild &B = S.u.b;
        if (INF_LANE0) S.litHist[256] = 1;
        code_lengths(S.litHist, DEF_NLIT, 15, S.litLen);
        assign_codes(S.litLen, DEF_NLIT, S.litCode);
        code_lengths(S.distHist, DEF_NDIST, 15, S.distLen);
        assign_codes(S.distLen, DEF_NDIST, S.distCode);
        if (INF_LANE0) {                                                               // the header's lengths, run-length coded
            uint32_t hl = DEF_NLIT, hd = DEF_NDIST, k = 0;
            while (hl > 257 && !S.litLen[hl - 1]) hl--;
            while (hd > 1 && !S.distLen[hd - 1]) hd--;
            for (uint32_t i = 0; i < hl; i++) B.seq[i] = S.litLen[i];
            for (uint32_t i = 0; i < hd; i++) B.seq[hl + i] = S.distLen[i];
            const uint32_t all = hl + hd;
            for (uint32_t i = 0; i < all;) {
                const uint32_t v = B.seq[i];
                uint32_t run = 1;
                while (i + run < all && B.seq[i + run] == v) run++;
                i += run;
                if (v == 0) {
                    while (run >= 11) { const uint32_t r = run < 138 ? run : 138; B.hs[k++] = (uint16_t) (18 | (r - 11) << 8); S.clHist[18]++; run -= r; }
                    if (run >= 3) { B.hs[k++] = (uint16_t) (17 | (run - 3) << 8); S.clHist[17]++; run = 0; }
                } else {
                    B.hs[k++] = (uint16_t) v; S.clHist[v]++; run--;
                    while (run >= 3) { const uint32_t r = run < 6 ? run : 6; B.hs[k++] = (uint16_t) (16 | (r - 3) << 8); S.clHist[16]++; run -= r; }
                }
                for (; run; run--) { B.hs[k++] = (uint16_t) v; S.clHist[v]++; }
            }
            S.hdr[0] = hl; S.hdr[1] = hd; S.hdr[2] = k;
        }
        INF_SYNC();
        code_lengths(S.clHist, DEF_NCL, 7, S.clLen);
        assign_codes(S.clLen, DEF_NCL, S.clCode);
        INF_LANES_DO(lane) {                                                           // the block's bits
            uint32_t bits = 0;
            for (uint32_t s = lane; s < DEF_NLIT; s += DEF_WAVE) bits += S.litHist[s] * (S.litLen[s] + (s > 256 ? def_len_extra(s - 257) : 0));
            if (lane < DEF_NDIST) bits += S.distHist[lane] * (S.distLen[lane] + def_dist_extra(lane));
            if (lane < DEF_NCL) bits += S.clHist[lane] * (S.clLen[lane] + def_cl_extra(lane));
            S.scan[lane] = bits;
        }
        INF_SYNC();
        uint32_t bits = DEF_EXSCAN(S.scan);
        INF_SYNC();
        if (INF_LANE0) {
            uint32_t h = DEF_NCL;
            while (h > 4 && !S.clLen[DEF_ORDER[h - 1]]) h--;
            S.hdr[3] = h;
        }
        INF_SYNC();
        hlit = INF_UNI(S.hdr[0]); hdist = INF_UNI(S.hdr[1]); nh = INF_UNI(S.hdr[2]); hclen = INF_UNI(S.hdr[3]);
        bits += 3 + 14 + 3 * hclen;
        return bits < 8 * n;
    }
    __device__ void zero_staging() {
        INF_SYNC();
        INF_LANES_DO(lane) {
            const uint4 z = {0, 0, 0, 0};
            for (uint32_t j = lane * 16; j < sizeof S.text; j += DEF_WAVE * 16) *(uint4 *) (S.text + j) = z;
        }
        INF_SYNC();
    }
    __device__ void emit_dynamic(uint32_t hlit, uint32_t hdist, uint32_t hclen, uint32_t nh) {
        DefBuild &B = S.u.b;
        put((last ? 1u : 0u) | 2u << 1, 3);
        put(hlit - 257, 5); put(hdist - 1, 5); put(hclen - 4, 4);
        for (uint32_t i = 0; i < hclen; i++) put(INF_UNI((uint32_t) S.clLen[DEF_ORDER[i]]), 3);
        for (uint32_t base = 0; base < nh; base += DEF_WAVE) {
            INF_LANES_DO(lane) {
                uint64_t v = 0; uint32_t nb = 0;
                if (base + lane < nh) {
                    const uint32_t e = B.hs[base + lane], s = e & 255u, l = S.clLen[s];
                    v = (uint64_t) S.clCode[s] | (uint64_t) (e >> 8) << l; nb = l + def_cl_extra(s);
                }
                S.ev[lane] = v; S.scan[lane] = nb;
            }
            place_tile();
        }
        for (uint32_t base = 0; base < n; base += DEF_WAVE) {
            const uint64_t tw = (uint64_t) INF_UNI(S.tok[base >> 5]) | (uint64_t) INF_UNI(S.tok[(base >> 5) + 1]) << 32;
            if (!tw) continue;
            INF_LANES_DO(lane) {
                uint64_t v = 0; uint32_t nb = 0;
                const uint32_t p = base + lane;
                if (tw >> lane & 1u) {
                    const uint32_t e = S.match[p >> 3];
                    if (e && (e & 7u) == (p & 7u)) {
                        uint32_t lc, leb, lev, ds, deb, dev;
                        def_len_sym(e >> 3 & 511u, lc, leb, lev); def_dist_sym(e >> 12, ds, deb, dev);
                        const uint32_t ll = S.litLen[257 + lc], dl = S.distLen[ds];
                        v = (uint64_t) S.litCode[257 + lc] | (uint64_t) lev << ll | (uint64_t) S.distCode[ds] << (ll + leb) | (uint64_t) dev << (ll + leb + dl);
                        nb = ll + leb + dl + deb;
                    } else {
                        const uint32_t b = in[p];
                        v = S.litCode[b]; nb = S.litLen[b];
                    }
                }
                S.ev[lane] = v; S.scan[lane] = nb;
            }
            place_tile();
        }
        put(INF_UNI((uint32_t) S.litCode[256]), INF_UNI((uint32_t) S.litLen[256]));
    }
    __device__ void emit_stored() {
        put(last ? 1u : 0u, 3);
        pad_to_byte();
        put(n | (~n & 0xffffu) << 16, 32);
        const uint32_t at = bitpos >> 3;
        INF_SYNC();
        for (uint32_t base = 0; base < n; base += DEF_WAVE)
            INF_LANES_DO(lane) { if (base + lane < n) S.text[at + base + lane] = in[base + lane]; }
        INF_SYNC();
        bitpos += 8 * n;
    }
    __device__ void flush(uint32_t sb, uint32_t bytes) {                               // S.text[sb, sb + bytes) -> slot[0, bytes): 16-byte boundaries coincide
        const uint32_t A = sb, B = sb + bytes, up = (A + 15u) & ~15u, a1 = up < B ? up : B;
        INF_SYNC();
        INF_LANES_DO(lane) { if (lane < 16 && A + lane < a1) slot[lane] = S.text[A + lane]; }
        if (a1 < B) {
            const uint32_t b0 = B & ~15u;
            INF_LANES_DO(lane) {
                for (uint32_t v = a1 + lane * 16; v < b0; v += DEF_WAVE * 16) *(uint4 *) (slot + (v - sb)) = *(const uint4 *) (S.text + v);
                if (lane < 16 && b0 + lane < B) slot[b0 + lane - sb] = S.text[b0 + lane];
            }
        }
        INF_SYNC();
    }

    __device__ DefChunkOut run() {
        load_text();
        text_crc();
        clear();
        find_matches();
        uint32_t hlit = 0, hdist = 0, hclen = 0, nh = 0;
        const bool dynamic = n != 0 && build_dynamic(hlit, hdist, hclen, nh);
        const uint32_t sb = (uint32_t) ((uintptr_t) slot & 15u);
        zero_staging();
        bitpos = 8 * sb;
        if (dynamic) emit_dynamic(hlit, hdist, hclen, nh);
        else if (n) emit_stored();
        else { put((last ? 1u : 0u) | 1u << 1, 3); put(0, 7); }                        // no text: an empty fixed block
        if (!last) { put(0, 3); pad_to_byte(); put(0xffff0000u, 32); }                 // the chunk ends on a byte: an empty stored block
        pad_to_byte();
        const uint32_t bytes = (bitpos >> 3) - sb;
        flush(sb, bytes);
        DefChunkOut R = {bytes | (dynamic || !n ? 0u : DEF_STORED), crc};
        return R;
    }
};

// ---- pack: chunk c from its slot to its place in the caller's buffer; its job's first chunk writes the gzip header in front of
// it, the last one folds the job's CRC-32 from its chunks' (crc32_combine: XOR of crc_k * x^(8 * bytes behind chunk k)) and writes
// the trailer. red: DEF_WAVE words of LDS.
__device__ void def_pack_chunk(uint32_t *red, const uint8_t *slots, const DefChunkOut *outs, const DefPackIn *pk, const DefJobIn *jobs, uint32_t c, uint8_t *gz,
                               uint32_t *jobCrc) {
    const DefPackIn P = pk[c];
    const uint32_t bytes = outs[c].bytes & ~DEF_STORED;
    const uint8_t *src = slots + (uint64_t) c * DEF_SLOT;
    uint8_t *dst = gz + P.dst;
    const uint32_t head = (16u - (uint32_t) ((uintptr_t) dst & 15u)) & 15u, h1 = head < bytes ? head : bytes, b0 = h1 + ((bytes - h1) & ~15u);
    INF_LANES_DO(lane) {
        if (lane < h1) dst[lane] = src[lane];
        for (uint32_t v = h1 + lane * 16; v < b0; v += DEF_WAVE * 16) {
            uint4 x;
            memcpy(&x, src + v, 16);
            *(uint4 *) (dst + v) = x;
        }
        if (lane < 16 && b0 + lane < bytes) dst[b0 + lane] = src[b0 + lane];
        if ((P.flags & 1u) && lane < 10) dst[(int64_t) lane - 10] = DEF_GZ_HEADER[lane];
    }
    if (!(P.flags & 2u)) return;
    const DefJobIn J = jobs[P.job];
    INF_LANES_DO(lane) {
        uint32_t acc = 0;
        for (uint32_t k = lane; k < J.nchunks; k += DEF_WAVE) {
            const uint64_t behind = k + 1 < J.nchunks ? J.inLen - (uint64_t) (k + 1) * DEF_CHUNK : 0;
            acc ^= inf_mulmod(outs[J.chunk0 + k].crc, inf_xpow8(behind));
        }
        red[lane] = acc;
    }
    INF_SYNC();
    uint32_t crc = 0;
    for (uint32_t i = 0; i < DEF_WAVE; i++) crc ^= INF_UNI(red[i]);
    const uint32_t isize = (uint32_t) J.inLen;
    INF_LANES_DO(lane) {
        if (lane < 4) dst[bytes + lane] = (uint8_t) (crc >> (8 * lane));
        else if (lane < 8) dst[bytes + lane] = (uint8_t) (isize >> (8 * (lane - 4)));
    }
    if (INF_LANE0) jobCrc[P.job] = crc;
}
