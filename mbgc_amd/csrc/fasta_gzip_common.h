// What the gzip inflate (fasta_inflate.h) and the gzip deflate (fasta_deflate.h) of the input stage share: the CRC-32 arithmetic of
// zlib's crc32_combine (polynomials modulo P, bit-reflected) and the bit reversal of a canonical code. Included inside namespace fa by
// either of them, whichever comes first; free of HIP calls like they are.
#ifndef MBGC_FASTA_GZIP_COMMON_H
#define MBGC_FASTA_GZIP_COMMON_H
constexpr uint32_t INF_POLY = 0xEDB88320u;

__device__ __forceinline__ uint32_t inf_mulmod(uint32_t a, uint32_t b) {          // a * b mod P, bit-reflected (zlib's multmodp)
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ INF_POLY : b >> 1;
    }
    return p;
}
template <class N> __device__ __forceinline__ uint32_t inf_xpow8(N nbytes) {      // x^(8 * nbytes) mod P (N: uint32_t or uint64_t)
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) p = inf_mulmod(sq, p);
        sq = inf_mulmod(sq, sq);
    }
    return p;
}
__device__ __forceinline__ uint32_t inf_bitrev(uint32_t v, uint32_t bits) {       // the low `bits` bits of v, reversed (1 <= bits <= 15)
    v = (v & 0x5555u) << 1 | (v >> 1 & 0x5555u);
    v = (v & 0x3333u) << 2 | (v >> 2 & 0x3333u);
    v = (v & 0x0f0fu) << 4 | (v >> 4 & 0x0f0fu);
    v = (v & 0x00ffu) << 8 | (v >> 8 & 0x00ffu);
    return v >> (16 - bits);
}
#endif
