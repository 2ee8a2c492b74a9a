// Input stage on the device (include/mbgc_fasta.h): kseq_read_lossless_fasta (utils/kseq.h:233-274) for whole files
// resident in HBM. The reader is a byte-serial state machine, but its state at a byte is tiny — "is the line
// this byte belongs to a header line" and where that line started — and it is decided by the nearest '\n'
// before the byte. So: (1) every 4096-byte chunk summarises itself independently of what comes before
// (its first/last newline, what it keeps after its first newline, its header starts), (2) one wave per file
// scans the chunk summaries (a chunk with a newline fixes the state for what follows, one without passes it
// on), (3) every chunk, now knowing the state it starts in and how many bytes / records precede it, writes its
// sequence bytes and its records and votes on the line-length rule. Streaming work: the file is read twice,
// the sequences are written once.
//
// The lossy rule (kseq_read_lossy, utils/kseq.h:282-333; MBGC_FASTA_LOSSY) is a compile-time variant of the same three
// passes. What it adds to the state: the file starts at its first '>' or '@' (k_fa_first_marker moves the file's start
// there, so that byte 0 is a header line's marker as in a well-formed file); a line's last CR goes (ks_getuntil2, :147)
// unless it is the record's first sequence byte — a CR alone on its line stays exactly when only empty lines lie between
// it and the record's header line, so the scan also carries "the record has no sequence byte yet" across chunks that are
// nothing but newlines; the line-length vote is one maximum over the stripped lines. At most one CR per chunk cannot be
// decided inside the chunk (the one behind the chunk's leading run of newlines): the summary names what it depends on,
// the scan counts it, the emit pass keeps or drops it by the same two flags.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <sys/mman.h>

#include "../../include/mbgc_fasta.h"

namespace fa {

constexpr int CHUNK = 4096, THREADS = 256, PER = CHUNK / THREADS;    // 16 bytes per thread
constexpr int WAVE = 64;

struct FileDesc {
    uint64_t off, n;          // bytes of the file in the input buffer
    uint32_t chunk0, nchunks;
};

struct ChunkSum {             // what a chunk knows on its own
    int32_t firstNL, lastNL;  // offsets inside the chunk, -1: none
    uint32_t keepAfter;       // bytes kept among those after firstNL (their lines start inside the chunk)
    uint32_t hdrStarts;       // header lines starting in the chunk (a '>' on the file's last byte is not one, kseq.h:243)
    uint8_t fresh;            // the chunk's first byte starts a line (file start, or the byte before it is '\n')
    uint8_t firstGt;          // the chunk's first byte is '>'
    uint8_t openHdr;          // the line open at the chunk's end is a header line (valid when lastNL >= 0 and it is not the last byte)
    uint8_t aux;              // lossy rule only (AUX_*), else 0
};

struct ChunkIn {              // what the scan adds
    uint64_t lineStart;       // file offset where the line open at the chunk's first byte started
    uint64_t keptBefore;      // sequence bytes of the file before the chunk
    uint32_t recBefore;       // records of the file before the chunk
    uint32_t inHdr;           // that open line is a header line (lossy rule: bit 0; bit 1: the record has no sequence byte where that line starts)
};

struct FileOut {              // per file, written by the scan and the emit kernels
    uint64_t kept, recs;
    unsigned long long minLine, maxLine, maxLast;   // lengths of the non-last lines of all records / of their last lines
    uint32_t emptyLine, firstNotGt;                 // (lossy rule: maxLine = the longest stripped line, firstNotGt = a '+' starts a line)
};

__device__ __forceinline__ uint8_t up(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t) (c - 32) : c; }

// stage the chunk in LDS; returns its length
__device__ __forceinline__ uint32_t stage(const uint8_t *__restrict__ f, const FileDesc &fd, uint32_t c, uint8_t *lds) {
    const uint64_t cs = (uint64_t) c * CHUNK;
    const uint32_t len = (uint32_t) (fd.n - cs < CHUNK ? fd.n - cs : CHUNK);
    const uint8_t *src = f + fd.off + cs;
    const uint32_t o = threadIdx.x * PER;
    if (o + PER <= len) {
        uint4 t;
        memcpy(&t, src + o, PER);
        *(uint4 *) (lds + o) = t;
    } else
        for (uint32_t k = o; k < len && k < o + PER; k++) lds[k] = src[k];
    __syncthreads();
    return len;
}

// ---- lossy rule
__device__ __forceinline__ bool marker(uint8_t c) { return c == '>' || c == '@'; }

// ChunkSum::aux. A verdict of two bits: 0 no, 1 yes, 2 = yes iff the record has no sequence byte where the chunk's open line
// starts (ChunkIn bit 1), 3 = yes iff the chunk's open line is a header line (ChunkIn bit 0).
constexpr uint32_t AUX_COND = 3;          // verdict on the chunk's one lone CR that the chunk cannot decide (2, 3), 0: there is none
constexpr uint32_t AUX_PREFIX_CR = 4;     // the open line's last byte lies in the chunk and is a CR that goes if that line is sequence
constexpr uint32_t AUX_PLUS = 8;          // a '+' starts a line: FASTQ
constexpr int AUX_TAIL = 4;               // verdict "the record has no sequence byte behind the chunk" (read when the chunk ends with '\n')
constexpr uint32_t NO_MARKER = 0xffffffffu;

// the lossy chunk: an empty one when the file, cut at its first marker, ends before it; ch[len] = the byte behind the chunk,
// '\n' at the end of the file (a line's last byte is the one in front of either)
__device__ __forceinline__ uint32_t stage_lossy(const uint8_t *__restrict__ f, const FileDesc &fd, uint32_t c, uint8_t *lds) {
    const uint64_t cs = (uint64_t) c * CHUNK;
    const uint32_t len = cs < fd.n ? (uint32_t) (fd.n - cs < CHUNK ? fd.n - cs : CHUNK) : 0u;
    const uint8_t *src = f + fd.off + cs;
    const uint32_t o = threadIdx.x * PER;
    if (o + PER <= len) {
        uint4 t;
        memcpy(&t, src + o, PER);
        *(uint4 *) (lds + o) = t;
    } else
        for (uint32_t k = o; k < len && k < o + PER; k++) lds[k] = src[k];
    if (threadIdx.x == THREADS - 1) lds[len] = cs + len < fd.n ? src[len] : (uint8_t) '\n';
    __syncthreads();
    return len;
}

// Is the line that holds ch[j] a header line? nl: what prev_newline() leaves behind (thread t: the last '\n' at or before its
// segment's end). -> verdict 0, 1 or 3.
__device__ __forceinline__ uint32_t line_is_header(const uint8_t *ch, const int32_t *nl, int32_t j, bool fresh) {
    const int32_t t0 = j / PER * PER;
    int32_t q = j - 1;
    while (q >= t0 && ch[q] != '\n') q--;
    if (q < t0) q = t0 ? nl[t0 / PER - 1] : -1;
    if (q < 0) return fresh ? (marker(ch[0]) ? 1u : 0u) : 3u;        // the chunk's open line
    return marker(ch[q + 1]) ? 1u : 0u;
}

// ch[k] is a CR alone on its line and a '\n' follows: does the byte stay (kseq.h:147 with seq.l == 1)? -> verdict
__device__ __forceinline__ uint32_t lone_cr_stays(const uint8_t *ch, const int32_t *nl, int32_t k, bool fresh) {
    int32_t j = k - 2;                                              // (ch[k - 1] is the '\n' that makes k a line start)
    while (j >= 0 && ch[j] == '\n') j--;
    if (j < 0) return fresh ? 2u : 3u;                               // empty lines back to the chunk's first byte
    return line_is_header(ch, nl, j, fresh);
}

// last '\n' at or before every thread's segment start (exclusive of the segment), as an offset in the chunk, -1: none.
// `mine` = the thread's own last newline offset or -1. lds2: THREADS ints.
__device__ __forceinline__ int32_t prev_newline(int32_t mine, int32_t *lds2) {
    lds2[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {                           // inclusive max-scan (Hillis-Steele)
        const int32_t other = threadIdx.x >= (unsigned) d ? lds2[threadIdx.x - d] : -1;
        __syncthreads();
        if (other > lds2[threadIdx.x]) lds2[threadIdx.x] = other;
        __syncthreads();
    }
    const int32_t r = threadIdx.x ? lds2[threadIdx.x - 1] : -1;
    __syncthreads();
    return r;
}

template <int NT>
__device__ uint32_t block_sum_scan(uint32_t x, uint32_t *lds, uint32_t *total) {     // exclusive scan over the block
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t inc = x;
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t y = (uint32_t) __shfl_up((int) inc, d);
        if ((int) lane >= d) inc += y;
    }
    __syncthreads();
    if (lane == WAVE - 1) lds[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < NT / WAVE; i++) { const uint32_t t = lds[i]; lds[i] = run; run += t; }
        lds[NT / WAVE] = run;
    }
    __syncthreads();
    *total = lds[NT / WAVE];
    const uint32_t r = lds[w] + inc - x;
    __syncthreads();
    return r;
}

// (1) per chunk
template <bool LOSSY>
__global__ void __launch_bounds__(THREADS) k_fa_summary(const uint8_t *__restrict__ f, const FileDesc *__restrict__ files,
                                                        const uint32_t *__restrict__ owner, ChunkSum *__restrict__ sums) {
    __shared__ uint8_t ch[CHUNK + 16];
    __shared__ int32_t nl[THREADS];
    __shared__ uint32_t red[THREADS / WAVE + 2];
    __shared__ int32_t firstNL, lastNL;
    __shared__ uint32_t sAux;
    const FileDesc fd = files[owner[blockIdx.x]];
    const uint32_t c = blockIdx.x - fd.chunk0;
    const uint32_t len = LOSSY ? stage_lossy(f, fd, c, ch) : stage(f, fd, c, ch);
    const uint64_t cs = (uint64_t) c * CHUNK;
    if (threadIdx.x == 0) { firstNL = 0x7fffffff; lastNL = -1; if (LOSSY) sAux = 0; }
    __syncthreads();
    const uint32_t o = threadIdx.x * PER;
    int32_t myFirst = 0x7fffffff, myLast = -1;
    for (uint32_t k = o; k < o + PER && k < len; k++)
        if (ch[k] == '\n') { if (myFirst == 0x7fffffff) myFirst = (int32_t) k; myLast = (int32_t) k; }
    if (myLast >= 0) { atomicMin(&firstNL, myFirst); atomicMax(&lastNL, myLast); }
    const int32_t prevNL = prev_newline(myLast, nl);
    __syncthreads();
    const int32_t fNL = firstNL == 0x7fffffff ? -1 : firstNL;
    // walk the segment: bytes after the chunk's first newline know their line start
    uint32_t keep = 0, hdr = 0;
    int32_t ls = prevNL >= 0 ? prevNL + 1 : -1;                       // start of the open line if it lies in the chunk
    if constexpr (LOSSY) {
        bool isHdr = ls >= 0 && ls < (int32_t) len && marker(ch[ls]);
        const bool fresh = len && (cs == 0 || f[fd.off + cs - 1] == '\n');
        uint32_t aux = 0;
        for (uint32_t k = o; k < o + PER && k < len; k++) {
            const uint8_t b = ch[k];
            const bool lineStart = k == 0 ? fresh : ch[k - 1] == '\n';
            if (lineStart) { isHdr = marker(b); if (isHdr && cs + k + 1 < fd.n) hdr++; if (b == '+') aux |= AUX_PLUS; }
            const bool after = fNL >= 0 && (int32_t) k > fNL;
            bool stays = b != '\n';
            if (b == '\r' && ch[k + 1] == '\n') {                    // the line's last byte (ch[len]: the byte behind the chunk)
                uint32_t v = 0;
                if (lineStart) v = cs + k + 1 == fd.n ? 1u : lone_cr_stays(ch, nl, (int32_t) k, fresh);   // (nothing behind it: -1 at kseq.h:143, before the strip)
                if (v >= 2) { aux |= v; v = 0; }                     // the scan decides, and counts it
                stays = v == 1;
                if (!after && !stays) aux |= AUX_PREFIX_CR;
            }
            if (after && !isHdr && stays) keep++;
        }
        if (aux) atomicOr(&sAux, aux);
        uint32_t tk, th;
        block_sum_scan<THREADS>(keep, red, &tk);
        block_sum_scan<THREADS>(hdr, red, &th);
        if (threadIdx.x == 0) {
            uint32_t tail = 0;
            if (len && lastNL == (int32_t) len - 1) {                // what a chunk that starts a line behind this one needs to know
                int32_t j = (int32_t) len - 2;
                while (j >= 0 && ch[j] == '\n') j--;
                tail = j < 0 ? (fresh ? 2u : 3u) : line_is_header(ch, nl, j, fresh);
            }
            ChunkSum s;
            s.firstNL = fNL; s.lastNL = lastNL; s.keepAfter = tk; s.hdrStarts = th;
            s.fresh = fresh; s.firstGt = len && marker(ch[0]);
            s.openHdr = lastNL >= 0 && lastNL + 1 < (int32_t) len && marker(ch[lastNL + 1]);
            s.aux = (uint8_t) (sAux | (tail << AUX_TAIL));
            sums[blockIdx.x] = s;
        }
    } else {
    bool isHdr = ls >= 0 && ls < (int32_t) len && ch[ls] == '>';
    const bool fresh = cs == 0 || f[fd.off + cs - 1] == '\n';
    for (uint32_t k = o; k < o + PER && k < len; k++) {
        const uint8_t b = ch[k];
        const bool lineStart = k == 0 ? fresh : ch[k - 1] == '\n';
        if (lineStart) { ls = (int32_t) k; isHdr = b == '>'; if (isHdr && cs + k + 1 < fd.n) hdr++; }
        if (fNL >= 0 && (int32_t) k > fNL && !isHdr && b != '\n') keep++;
    }
    uint32_t tk, th;
    block_sum_scan<THREADS>(keep, red, &tk);
    block_sum_scan<THREADS>(hdr, red, &th);
    if (threadIdx.x == 0) {
        ChunkSum s;
        s.firstNL = fNL; s.lastNL = lastNL; s.keepAfter = tk; s.hdrStarts = th;
        s.fresh = fresh; s.firstGt = len && ch[0] == '>';
        s.openHdr = lastNL >= 0 && lastNL + 1 < (int32_t) len && ch[lastNL + 1] == '>';
        s.aux = 0;
        sums[blockIdx.x] = s;
    }
    }
}

// (2) one wave per file
template <bool LOSSY>
__global__ void __launch_bounds__(WAVE) k_fa_scan(const uint8_t *__restrict__ f, const FileDesc *__restrict__ files,
                                                  const ChunkSum *__restrict__ sums, ChunkIn *__restrict__ ins, FileOut *__restrict__ fout) {
    const FileDesc fd = files[blockIdx.x];
    const int lane = threadIdx.x;
    // state carried across groups of 64 chunks
    bool carryHdr = fd.n && (LOSSY ? marker(f[fd.off]) : f[fd.off] == '>');   // the file's first line (no newline seen yet)
    uint64_t carryLS = 0, kept = 0;
    uint32_t recs = 0;
    int carryE = 0;                                                   // lossy: the record has no sequence byte behind the chunks so far
    bool plus = false;
    for (uint32_t g0 = 0; g0 < fd.nchunks; g0 += WAVE) {
        const uint32_t c = g0 + lane;
        const bool live = c < fd.nchunks;
        ChunkSum s;
        s.firstNL = -1; s.lastNL = -1; s.keepAfter = 0; s.hdrStarts = 0; s.fresh = 0; s.firstGt = 0; s.openHdr = 0; s.aux = 0;
        if (live) s = sums[fd.chunk0 + c];
        const uint64_t cs = (uint64_t) c * CHUNK;
        const uint32_t len = live && (!LOSSY || cs < fd.n) ? (uint32_t) (fd.n - cs < CHUNK ? fd.n - cs : CHUNK) : 0;
        // nearest earlier chunk of the group that fixes the state of what follows: one with a newline (the line open
        // at its end), or one whose first byte starts a line and that has no newline (that very line)
        int idx = (live && (s.lastNL >= 0 || s.fresh)) ? lane : -1;
        for (int d = 1; d < WAVE; d <<= 1) {
            const int y = __shfl_up(idx, d);
            if (lane >= d && y > idx) idx = y;
        }
        const int prev = __shfl_up(idx, 1);
        const int pidx = lane ? prev : -1;
        // state a chunk with a newline leaves behind: header flag and start of its open line
        // (a chunk that ends with its newline leaves a line that starts with the next chunk: that chunk is "fresh" and
        // never asks)
        const uint64_t myLS = s.lastNL >= 0 ? cs + (uint64_t) (s.lastNL + 1) : cs;
        const int myHdr = s.lastNL >= 0 ? (int) s.openHdr : (int) s.firstGt;
        const int srcLane = pidx >= 0 ? pidx : 0;
        const int pHdr = __shfl(myHdr, srcLane);
        const uint64_t pLS = ((uint64_t) (uint32_t) __shfl((int) (myLS >> 32), srcLane) << 32) | (uint32_t) __shfl((int) (uint32_t) myLS, srcLane);
        bool inHdr; uint64_t inLS;
        if (s.fresh) { inHdr = s.firstGt; inLS = cs; }
        else if (pidx >= 0) { inHdr = pHdr; inLS = pLS; }
        else { inHdr = carryHdr; inLS = carryLS; }
        const uint32_t prefix = s.firstNL >= 0 ? (uint32_t) s.firstNL : len;        // bytes of the open line inside the chunk (no newline among them)
        uint32_t mine = live ? s.keepAfter + (inHdr ? 0u : prefix) : 0u;
        int inE = 0;
        if constexpr (LOSSY) {
            // "no sequence byte yet" behind every chunk: its own verdict, or what it starts with when it is nothing but newlines
            const uint32_t tail = (s.aux >> AUX_TAIL) & 3u;
            const int ev = tail == 2 ? -1 : tail == 3 ? (int) inHdr : (int) tail;
            int eidx = ev >= 0 ? lane : -1;
            for (int d = 1; d < WAVE; d <<= 1) {
                const int y = __shfl_up(eidx, d);
                if (lane >= d && y > eidx) eidx = y;
            }
            const int evAt = __shfl(ev, eidx >= 0 ? eidx : 0);
            const int outE = eidx >= 0 ? evAt : carryE;
            const int before = __shfl_up(outE, 1);
            inE = lane ? before : carryE;
            carryE = __shfl(outE, WAVE - 1);
            const uint32_t cond = s.aux & AUX_COND;
            if (live) {
                if (!inHdr && (s.aux & AUX_PREFIX_CR)) mine -= 1;
                if ((cond == 2 && inE) || (cond == 3 && inHdr)) mine += 1;
            }
            plus = plus || __ballot(live && (s.aux & AUX_PLUS)) != 0;
        }
        uint32_t incK = mine, incR = live ? s.hdrStarts : 0u;
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t a = (uint32_t) __shfl_up((int) incK, d), b = (uint32_t) __shfl_up((int) incR, d);
            if (lane >= d) { incK += a; incR += b; }
        }
        if (live) {
            ChunkIn in;
            in.lineStart = inLS; in.keptBefore = kept + incK - mine; in.recBefore = recs + incR - s.hdrStarts; in.inHdr = (uint32_t) inHdr | (uint32_t) (inE << 1);
            ins[fd.chunk0 + c] = in;
        }
        // carry out of the group: the last chunk with a newline (or the old carry), totals
        const int lastIdx = __shfl(idx, WAVE - 1);
        if (lastIdx >= 0) {
            const int lh = __shfl(myHdr, lastIdx);
            const uint64_t ll = ((uint64_t) (uint32_t) __shfl((int) (myLS >> 32), lastIdx) << 32) | (uint32_t) __shfl((int) (uint32_t) myLS, lastIdx);
            carryHdr = lh; carryLS = ll;
        }
        kept += (uint64_t) (uint32_t) __shfl((int) incK, WAVE - 1);
        recs += (uint32_t) __shfl((int) incR, WAVE - 1);
    }
    if (lane == 0) {
        FileOut o;
        o.kept = kept; o.recs = recs; o.minLine = ~0ull; o.maxLine = 0; o.maxLast = 0; o.emptyLine = 0;
        o.firstNotGt = LOSSY ? (uint32_t) plus : (uint32_t) (fd.n && f[fd.off] != '>');
        fout[blockIdx.x] = o;
    }
}

// (3) per chunk again. shift (lossy rule): what k_fa_first_marker cut off every file's front — record headers are offsets in the whole file
template <bool LOSSY>
__global__ void __launch_bounds__(THREADS) k_fa_emit(const uint8_t *__restrict__ f, const FileDesc *__restrict__ files,
                                                     const uint32_t *__restrict__ owner, const ChunkSum *__restrict__ sums,
                                                     const ChunkIn *__restrict__ ins, const uint64_t *__restrict__ seqBase,
                                                     const uint64_t *__restrict__ recBase, int uppercase, uint8_t *__restrict__ out,
                                                     mbgc_fasta_record_t *__restrict__ recs, FileOut *__restrict__ fout,
                                                     const uint64_t *__restrict__ shift) {
    __shared__ uint8_t ch[CHUNK + 16];
    __shared__ int32_t nl[THREADS];
    __shared__ uint32_t red[THREADS / WAVE + 2];
    const uint32_t fi = owner[blockIdx.x];
    const FileDesc fd = files[fi];
    const uint32_t c = blockIdx.x - fd.chunk0;
    const uint32_t len = LOSSY ? stage_lossy(f, fd, c, ch) : stage(f, fd, c, ch);
    const uint64_t cs = (uint64_t) c * CHUNK;
    const ChunkIn in = ins[blockIdx.x];
    const ChunkSum sm = sums[blockIdx.x];
    const uint32_t o = threadIdx.x * PER;
    int32_t myLast = -1;
    for (uint32_t k = o; k < o + PER && k < len; k++) if (ch[k] == '\n') myLast = (int32_t) k;
    const int32_t prevNL = prev_newline(myLast, nl);
    // state at the thread's first byte
    uint64_t ls = prevNL >= 0 ? cs + (uint64_t) prevNL + 1 : in.lineStart;        // file offset of the open line's start
    if constexpr (LOSSY) {
        const bool inHdr = in.inHdr & 1u, inE = in.inHdr & 2u;
        bool isHdr = prevNL >= 0 ? (prevNL + 1 < (int32_t) len ? marker(ch[prevNL + 1]) : false) : inHdr;
        // pass A: the CRs that go (bit i: byte o + i), what the thread keeps, its header starts
        uint32_t keep = 0, hdr = 0, goes = 0;
        {
            bool h2 = isHdr;
            for (uint32_t k = o; k < o + PER && k < len; k++) {
                const uint8_t b = ch[k];
                const bool lineStart = k == 0 ? sm.fresh : ch[k - 1] == '\n';
                if (lineStart) { h2 = marker(b); if (h2 && cs + k + 1 < fd.n) hdr++; }
                if (b == '\r' && ch[k + 1] == '\n') {                // the line's last byte: as in k_fa_summary
                    uint32_t v = 0;
                    if (lineStart) v = cs + k + 1 == fd.n ? 1u : lone_cr_stays(ch, nl, (int32_t) k, sm.fresh);
                    const bool stays = v == 1 || (v == 2 && inE) || (v == 3 && inHdr);
                    if (!stays) goes |= 1u << (k - o);
                }
                if (!h2 && b != '\n' && !((goes >> (k - o)) & 1u)) keep++;
            }
        }
        uint32_t tk, th;
        const uint32_t keepEx = block_sum_scan<THREADS>(keep, red, &tk);
        const uint32_t hdrEx = block_sum_scan<THREADS>(hdr, red, &th);
        __shared__ uint8_t packed[CHUNK];
        __shared__ unsigned long long sMax;
        if (threadIdx.x == 0) sMax = 0;
        __syncthreads();
        uint8_t *dst = packed + keepEx;
        mbgc_fasta_record_t *R = recs + recBase[fi];
        const uint64_t cut = shift[fi];
        uint32_t kk = 0, hh = in.recBefore + hdrEx;                 // hh: records started before the current byte
        unsigned long long mx = 0;
        for (uint32_t k = o; k < o + PER && k < len; k++) {
            const uint8_t b = ch[k];
            const uint64_t p = cs + k;
            const bool lineStart = k == 0 ? sm.fresh : ch[k - 1] == '\n';
            if (lineStart) {
                ls = p; isHdr = marker(b);
                if (isHdr && p + 1 < fd.n) {                        // a record starts here
                    R[hh].headerOff = cut + p + 1;
                    R[hh].seqOff = in.keptBefore + keepEx + kk;
                    hh++;
                }
            }
            const bool gone = (goes >> (k - o)) & 1u;
            if (b != '\n' && ch[k + 1] == '\n') {                    // the line's last byte ('\n' or the file's end follows)
                if (isHdr) {
                    if (ls + 1 < fd.n && hh > 0) {                  // the record whose header line ends here; its CR goes when more than the CR is there (:147)
                        const uint64_t hl = p - ls;
                        R[hh - 1].headerLen = hl > 1 && b == '\r' ? hl - 1 : hl;
                    }
                } else {
                    const unsigned long long d = p + 1 - ls - (gone ? 1 : 0);       // maxLastDnaLineLen (:301-312) counts what the strip left
                    if (d > mx) mx = d;
                }
            }
            if (!isHdr && b != '\n' && !gone) dst[kk++] = uppercase ? up(b) : b;
        }
        if (mx) atomicMax(&sMax, mx);
        __syncthreads();
        if (threadIdx.x == 0 && sMax) atomicMax(&fout[fi].maxLine, sMax);
        uint8_t *g = out + seqBase[fi] + in.keptBefore;
        for (uint32_t k = threadIdx.x * 16; k < tk; k += THREADS * 16) {
            if (k + 16 <= tk) {
                uint4 t = *(const uint4 *) (packed + k);
                memcpy(g + k, &t, 16);
            } else
                for (uint32_t j = k; j < tk; j++) g[j] = packed[j];
        }
    } else {
    bool isHdr = prevNL >= 0 ? (prevNL + 1 < (int32_t) len ? ch[prevNL + 1] == '>' : false) : in.inHdr != 0;
    // pass A: count what the thread keeps and the header starts before each byte
    uint32_t keep = 0, hdr = 0;
    {
        uint64_t l2 = ls; bool h2 = isHdr;
        for (uint32_t k = o; k < o + PER && k < len; k++) {
            const uint8_t b = ch[k];
            const bool lineStart = k == 0 ? sm.fresh : ch[k - 1] == '\n';
            if (lineStart) { l2 = cs + k; h2 = b == '>'; if (h2 && cs + k + 1 < fd.n) hdr++; }
            if (!h2 && b != '\n') keep++;
        }
    }
    uint32_t tk, th;
    const uint32_t keepEx = block_sum_scan<THREADS>(keep, red, &tk);
    const uint32_t hdrEx = block_sum_scan<THREADS>(hdr, red, &th);
    // pass B: the kept bytes are compacted in LDS first (then stored coalesced), records and line lengths on the way
    __shared__ uint8_t packed[CHUNK];
    __shared__ unsigned long long sMin, sMax, sLast;
    __shared__ uint32_t sEmpty;
    if (threadIdx.x == 0) { sMin = ~0ull; sMax = 0; sLast = 0; sEmpty = 0; }
    __syncthreads();
    uint8_t *dst = packed + keepEx;
    mbgc_fasta_record_t *R = recs + recBase[fi];
    uint32_t kk = 0, hh = in.recBefore + hdrEx;                     // hh: records started before the current byte
    unsigned long long mn = ~0ull, mx = 0, mxLast = 0;
    uint32_t empty = 0;
    for (uint32_t k = o; k < o + PER && k < len; k++) {
        const uint8_t b = ch[k];
        const uint64_t p = cs + k;
        const bool lineStart = k == 0 ? sm.fresh : ch[k - 1] == '\n';
        if (lineStart) {
            ls = p; isHdr = b == '>';
            if (isHdr && p + 1 < fd.n) {                            // a record starts here
                R[hh].headerOff = p + 1;
                R[hh].seqOff = in.keptBefore + keepEx + kk;
                hh++;
            }
        }
        const bool term = b == '\n';
        const bool eofTerm = !term && p + 1 == fd.n;                // the file's last line has no newline
        if (term || eofTerm) {
            const uint64_t end = term ? p : p + 1;
            if (isHdr) {
                if (ls + 1 < fd.n && hh > 0) R[hh - 1].headerLen = end - (ls + 1);  // the record whose header line ends here
            } else {
                const unsigned long long d = end - ls;
                const bool lastOfRecord = end + 1 >= fd.n || (term && f[fd.off + p + 1] == '>') || eofTerm;
                if (d == 0) empty = 1;                               // an empty line (kseq.h:251)
                else if (lastOfRecord) { if (d > mxLast) mxLast = d; }
                else { if (d < mn) mn = d; if (d > mx) mx = d; }
            }
        }
        if (!isHdr && !term) dst[kk++] = uppercase ? up(b) : b;
    }
    // one vote per chunk on the line-length rule (a million lines voting one by one serialise on the file's counters)
    if (mn != ~0ull) { atomicMin(&sMin, mn); atomicMax(&sMax, mx); }
    if (mxLast) atomicMax(&sLast, mxLast);
    if (empty) atomicOr(&sEmpty, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sMin != ~0ull) { atomicMin(&fout[fi].minLine, sMin); atomicMax(&fout[fi].maxLine, sMax); }
        if (sLast) atomicMax(&fout[fi].maxLast, sLast);
        if (sEmpty) atomicOr(&fout[fi].emptyLine, 1u);
    }
    uint8_t *g = out + seqBase[fi] + in.keptBefore;
    for (uint32_t k = threadIdx.x * 16; k < tk; k += THREADS * 16) {
        if (k + 16 <= tk) {
            uint4 t = *(const uint4 *) (packed + k);
            memcpy(g + k, &t, 16);
        } else
            for (uint32_t j = k; j < tk; j++) g[j] = packed[j];
    }
    }
}

// the lossy rule's first step (kseq.h:288): everything in front of the file's first '>' or '@' is skipped, wherever in a line that
// byte stands. One workgroup per file reads chunks until it meets one (the first chunk, in a file that is not damaged) and moves
// the file's start there; a file without one becomes empty. shift: how far.
__global__ void __launch_bounds__(THREADS) k_fa_first_marker(const uint8_t *__restrict__ f, FileDesc *__restrict__ files, uint64_t *__restrict__ shift) {
    __shared__ uint32_t first;
    const FileDesc fd = files[blockIdx.x];
    const uint32_t o = threadIdx.x * PER;
    uint64_t at = fd.n;
    for (uint64_t cs = 0; cs < fd.n; cs += CHUNK) {                  // (every branch on `first` is taken by the whole workgroup)
        if (threadIdx.x == 0) first = NO_MARKER;
        __syncthreads();
        const uint32_t len = (uint32_t) (fd.n - cs < CHUNK ? fd.n - cs : CHUNK);
        const uint8_t *src = f + fd.off + cs;
        uint8_t t[PER];
        if (o + PER <= len) memcpy(t, src + o, PER);
        else for (uint32_t k = 0; k < PER; k++) t[k] = o + k < len ? src[o + k] : 0;
        uint32_t mine = NO_MARKER;
#pragma unroll
        for (int k = PER - 1; k >= 0; k--) if (marker(t[k])) mine = o + (uint32_t) k;
        if (mine != NO_MARKER) atomicMin(&first, mine);
        __syncthreads();
        const uint32_t r = first;
        __syncthreads();
        if (r != NO_MARKER) { at = cs + r; break; }
    }
    if (threadIdx.x == 0) {
        files[blockIdx.x].off = fd.off + at; files[blockIdx.x].n = fd.n - at;
        shift[blockIdx.x] = at;
    }
}

// ---- single-FASTA input: mgmpInSplit_next (matching/input_with_libdeflate_wrapper.cpp:150-171) on a window in HBM.
// An element ends at the first '>' at or behind its start + minSplitSize, whatever line that '>' stands in. (1) a streaming
// pass leaves every 4096-byte tile's first '>' (one wave per tile, 16 bytes per lane and load, all four loads of a tile in
// flight before the first compare; no LDS); (2) one wave walks the chain of elements: the rest of the threshold's own tile
// byte by byte, then the tile array 64 tiles per ballot.
constexpr uint32_t NO_GT = 0xffffffffu;
constexpr int TILE_LOADS = CHUNK / (WAVE * PER);                     // 4 loads of 1 KiB per wave and tile

// index of the first byte of w equal to '>' (0..3), 4: none
__device__ __forceinline__ uint32_t first_gt_in_word(uint32_t w) {
    const uint32_t x = w ^ 0x3e3e3e3eu;
    const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;       // the lowest set bit marks the first zero byte of x
    return z ? (uint32_t) (__builtin_ctz(z) >> 3) : 4u;
}

// the split's marks under the flags of mbgc_fasta_split_buf_dev2; F = 0: any '>', the code as it was
constexpr uint32_t SPLIT_LS = MBGC_FASTA_SPLIT_LINE_START, SPLIT_AT = MBGC_FASTA_SPLIT_AT;

// 0x80 in every byte of w that equals the byte repeated in pat, and nowhere else (first_gt_in_word's cheaper form lets a borrow
// run into the bytes above the first hit: good for a first hit, not for a mask that is shifted and ANDed)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

template <uint32_t F>
__global__ void __launch_bounds__(THREADS) k_fa_first_gt(const uint8_t *__restrict__ f, uint64_t n, uint32_t tile0, uint32_t ntiles,
                                                         uint32_t *__restrict__ tileFirst) {       // tiles [tile0, ntiles)
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t tile = tile0 + blockIdx.x * (THREADS / WAVE) + threadIdx.x / WAVE;
    if (tile >= ntiles) return;                                     // (whole waves: a wave has one tile)
    const uint64_t ts = (uint64_t) tile * CHUNK;
    const uint32_t len = (uint32_t) (n - ts < CHUNK ? n - ts : CHUNK);
    const uint8_t *src = f + ts;
    uint4 v[TILE_LOADS];
#pragma unroll
    for (int i = 0; i < TILE_LOADS; i++) {
        const uint32_t o = (uint32_t) i * (WAVE * PER) + lane * PER;
        v[i] = make_uint4(0, 0, 0, 0);
        if (o + PER <= len) memcpy(&v[i], src + o, PER);
        else if (o < len) {                                        // the window's last, partial 16 bytes
            uint8_t t[PER] = {};
            for (uint32_t k = 0; o + k < len; k++) t[k] = src[o + k];
            memcpy(&v[i], t, PER);
        }
    }
    // the byte in front of the tile: across the tile edge, and, for a scan that is resumed, across the seam of the kept tile
    // array (the bytes before it have not changed); offset 0 of the buffer is a line start
    uint32_t behind = '\n';
    if constexpr ((F & SPLIT_LS) != 0) if (ts) behind = src[-1];
    uint32_t first = NO_GT;
    if constexpr (F == 0) {
#pragma unroll
        for (int i = 0; i < TILE_LOADS; i++) {
            const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            uint32_t mine = NO_GT;
#pragma unroll
            for (int k = 3; k >= 0; k--) {
                const uint32_t b = first_gt_in_word(w[k]);
                if (b < 4) mine = (uint32_t) k * 4 + b;
            }
            const unsigned long long m = __ballot(mine != NO_GT);
            if (m && first == NO_GT) {
                const int l = __builtin_ctzll(m);
                first = (uint32_t) i * (WAVE * PER) + (uint32_t) l * PER + (uint32_t) __shfl((int) mine, l);
            }
        }
    } else {
        // "the byte before is '\n'" is the LF mask moved up one byte: inside a dword a shift, from dword to dword a carried bit, from
        // lane to lane one shuffle of the four loads' last-byte bits, from load to load lane 63's bits — bit i of `before` says it
        // of the first byte of this lane's load i
        uint32_t before = 0;
        if constexpr ((F & SPLIT_LS) != 0) {
            uint32_t last = 0;
#pragma unroll
            for (int i = 0; i < TILE_LOADS; i++) last |= (uint32_t) ((v[i].w >> 24) == '\n') << i;
            const uint32_t up = (uint32_t) __shfl_up((int) last, 1), end = (uint32_t) __shfl((int) last, WAVE - 1);
            before = lane ? up : (end << 1) | (uint32_t) (behind == '\n');
        }
#pragma unroll
        for (int i = 0; i < TILE_LOADS; i++) {
            const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            uint32_t carry = ((before >> i) & 1u) << 7, hit[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t marks = eq_bytes(w[k], 0x3e3e3e3eu);
                if constexpr ((F & SPLIT_AT) != 0) marks |= eq_bytes(w[k], 0x40404040u);
                if constexpr ((F & SPLIT_LS) != 0) {
                    const uint32_t lf = eq_bytes(w[k], 0x0a0a0a0au);
                    marks &= (lf << 8) | carry;
                    carry = lf >> 24;
                }
                hit[k] = marks;
            }
            uint32_t mine = NO_GT;
#pragma unroll
            for (int k = 3; k >= 0; k--) if (hit[k]) mine = (uint32_t) k * 4 + (uint32_t) (__builtin_ctz(hit[k]) >> 3);
            const unsigned long long m = __ballot(mine != NO_GT);
            if (m && first == NO_GT) {
                const int l = __builtin_ctzll(m);
                first = (uint32_t) i * (WAVE * PER) + (uint32_t) l * PER + (uint32_t) __shfl((int) mine, l);
            }
        }
    }
    if (lane == 0) tileFirst[tile] = first;
}

template <uint32_t F>
__global__ void __launch_bounds__(WAVE) k_fa_split_chain(const uint8_t *__restrict__ f, uint64_t n, const uint32_t *__restrict__ tileFirst,
                                                         uint32_t ntiles, uint64_t start, int isFileEnd, uint64_t firstMin, uint64_t nextMin,
                                                         int maxElems, uint64_t *__restrict__ res) {   // res[0] = elements found, res[1 + j] = end of element j
    const uint32_t lane = threadIdx.x;
    const uint64_t NONE = ~0ull;
    uint64_t s = start;
    int j = 0;
    for (; j < maxElems && s != n; j++) {                           // (every branch below is taken by the whole wave)
        const uint64_t mn = j ? nextMin : firstMin;
        uint64_t e = NONE;
        if (mn < n - s) {
            const uint64_t thr = s + mn;
            const uint32_t t = (uint32_t) (thr / CHUNK);
            const uint64_t tbase = (uint64_t) t * CHUNK;
            const uint32_t tf = tileFirst[t];
            if (tf != NO_GT && tbase + tf >= thr) e = tbase + tf;
            else if (tf != NO_GT) {                                // the tile's first mark stands before the threshold: the rest of the tile
                const uint64_t tend = tbase + CHUNK < n ? tbase + CHUNK : n;
                for (uint64_t b = thr; b < tend && e == NONE; b += WAVE) {
                    const uint64_t p = b + lane;
                    bool mark = false;
                    if constexpr (F == 0) mark = p < tend && f[p] == '>';
                    else if (p < tend) {                           // (p >= thr > 0: the byte before p is in the buffer)
                        const uint8_t c = f[p];
                        mark = c == '>' || ((F & SPLIT_AT) != 0 && c == '@');
                        if constexpr ((F & SPLIT_LS) != 0) mark = mark && f[p - 1] == '\n';
                    }
                    const unsigned long long m = __ballot(mark);
                    if (m) e = b + (uint64_t) __builtin_ctzll(m);
                }
            }
            for (uint32_t tb = t + 1; tb < ntiles && e == NONE; tb += WAVE) {
                const uint32_t ti = tb + lane;
                const uint32_t v = ti < ntiles ? tileFirst[ti] : NO_GT;
                const unsigned long long m = __ballot(v != NO_GT);
                if (m) {
                    const int l = __builtin_ctzll(m);
                    e = (uint64_t) (tb + (uint32_t) l) * CHUNK + (uint32_t) __shfl((int) v, l);
                }
            }
        }
        if (e == NONE) {                                            // the threshold or the search ran off the window
            if (!isFileEnd) break;
            e = n;
        }
        if (lane == 0) res[1 + j] = e;
        s = e;
    }
    if (lane == 0) res[0] = (uint64_t) j;
}

// the two kernels of a split under F: one instantiation per rule, and the one without flags is the code as it was
template <uint32_t F>
static void launch_split(hipStream_t stream, const uint8_t *buf_dev, uint64_t start, uint64_t n, uint32_t tile0, uint32_t ntiles, int isFileEnd,
                         uint64_t firstMin, uint64_t nextMin, int maxElems, uint32_t *tileFirst, uint64_t *res) {
    if (tile0 < ntiles)
        k_fa_first_gt<F><<<dim3((ntiles - tile0 + THREADS / WAVE - 1) / (THREADS / WAVE)), dim3(THREADS), 0, stream>>>(buf_dev, n, tile0, ntiles, tileFirst);
    k_fa_split_chain<F><<<dim3(1), dim3(WAVE), 0, stream>>>(buf_dev, n, tileFirst, ntiles, start, isFileEnd, firstMin, nextMin, maxElems, res);
}

#include "fasta_format.h"
#include "fasta_compare.h"
#include "fasta_pack.h"
#include "fasta_select.h"
#include "fasta_tiles.h"
#include "fasta_find.h"
#include "fasta_find_iupac.h"
#include "fasta_stats.h"
#include "fasta_sketch.h"
#include "fasta_screen.h"
#include "fasta_dups.h"
#include "fasta_crc.h"

#define INF_CONST static __device__
#define INF_LANES_DO(lane) for (uint32_t lane = threadIdx.x, once_ = 1; once_; once_ = 0)
#define INF_LANE0 (threadIdx.x == 0)
#define INF_SYNC() __syncthreads()
#define INF_UNI(x) ((uint32_t) __builtin_amdgcn_readfirstlane((int) (x)))
#include "fasta_inflate.h"

// mbgc_fasta_inflate_dev: one gzip file per block of one wave (the decoder, the ring and the tables: fasta_inflate.h). gz and out may
// be one buffer (the round's file buffer holds both): no restrict on them; a job's input that another job's output runs over is refused
__global__ void __launch_bounds__(INF_WAVE) k_fa_inflate(const uint8_t *gz, uint8_t *out, const InfJob *__restrict__ jobs,
                                                         uint32_t job0, uint32_t njobs, InfResult *__restrict__ results) {
    __shared__ InfShared S;
    const uint32_t j = job0 + blockIdx.x;
    if (j >= njobs) return;
    const InfJob job = jobs[j];
    Inf I(S, gz + job.inOff, job.inLen, out + job.outOff, job.outCap);
    const InfResult r = I.run();
    if (threadIdx.x == 0) results[j] = r;
}

#define DEF_ATOMIC_ADD(p, v) atomicAdd(p, v)
#define DEF_ATOMIC_OR(p, v) atomicOr(p, v)
#define DEF_ATOMIC_MAX(p, v) atomicMax(p, v)
// arr[0, 64) in LDS -> its exclusive prefix sums; the total (the callers put a barrier on either side)
__device__ __forceinline__ uint32_t def_wave_exscan(uint32_t *arr) {
    const uint32_t lane = threadIdx.x, v = arr[lane];
    uint32_t x = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t) __shfl_up((int) x, d);
        if (lane >= d) x += y;
    }
    arr[lane] = x - v;
    return (uint32_t) __shfl((int) x, 63);
}
#define DEF_EXSCAN(arr) def_wave_exscan(arr)
#include "fasta_deflate.h"

// mbgc_fasta_deflate_dev: one chunk of DEF_CHUNK text bytes per block of one wave (the encoder: fasta_deflate.h) into its slot of the
// handle's staging buffer, then one block per chunk from the slot to its place between its job's gzip header and trailer
__global__ void __launch_bounds__(DEF_WAVE) k_fa_deflate(const uint8_t *__restrict__ text, const DefChunk *__restrict__ chunks, uint32_t chunk0, uint32_t nchunks,
                                                         uint8_t *__restrict__ slots, DefChunkOut *__restrict__ outs) {
    __shared__ DefShared S;
    const uint32_t c = chunk0 + blockIdx.x;
    if (c >= nchunks) return;
    const DefChunk ch = chunks[c];
    Def D(S, text + ch.inOff, ch.n, ch.last != 0, slots + (uint64_t) c * DEF_SLOT);
    const DefChunkOut r = D.run();
    if (threadIdx.x == 0) outs[c] = r;
}

__global__ void __launch_bounds__(DEF_WAVE) k_fa_deflate_pack(const uint8_t *__restrict__ slots, const DefChunkOut *__restrict__ outs, const DefPackIn *__restrict__ pk,
                                                              const DefJobIn *__restrict__ jobs, uint32_t chunk0, uint32_t nchunks, uint8_t *__restrict__ gz,
                                                              uint32_t *__restrict__ jobCrc) {
    __shared__ uint32_t red[DEF_WAVE];
    const uint32_t c = chunk0 + blockIdx.x;
    if (c >= nchunks) return;
    def_pack_chunk(red, slots, outs, pk, jobs, c, gz, jobCrc);
}

// mbgc_fasta_compare_dev: a wave's steps, then — only when a lane found a difference — one 64-bit atomicMin per piece the wave
// touches, from the lowest differing lane of that piece (its offset is the smallest: the steps of a piece ascend with the lanes).
// Equal data issues no atomic.
__global__ void __launch_bounds__(THREADS) k_fa_compare(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, const CmpPiece *__restrict__ P,
                                                        const uint32_t *__restrict__ owner, uint32_t tile0, uint32_t ntiles, uint64_t total,
                                                        unsigned long long *__restrict__ firstDiff) {
    const uint32_t tile = tile0 + blockIdx.x;
    if (tile >= ntiles) return;
    uint32_t piece = 0;
    const uint64_t d = cmp_lane_step(a, b, P, owner, tile, threadIdx.x, total, &piece);
    unsigned long long m = __ballot(d != CMP_NONE);
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    while (m) {                                                      // (uniform over the wave)
        const int leader = __ffsll(m) - 1;
        const uint32_t leaderPiece = (uint32_t) __shfl((int) piece, leader);
        if (lane == (uint32_t) leader) atomicMin(firstDiff + P[piece].slot, (unsigned long long) d);
        m &= ~__ballot(piece == leaderPiece);
    }
}

// mbgc_fasta_pack_dev: one lane step per thread (fasta_pack.h); nothing passes between the lanes
__global__ void __launch_bounds__(THREADS) k_fa_pack(const uint8_t *__restrict__ src, const PackPiece *__restrict__ P, const uint32_t *__restrict__ owner,
                                                     uint32_t tile0, uint32_t ntiles, uint32_t mis, uint64_t total, int fold, uint8_t *__restrict__ dst) {
    const uint32_t tile = tile0 + blockIdx.x;
    if (tile >= ntiles) return;
    pack_lane_step(src, P, owner, tile, threadIdx.x, mis, total, fold != 0, dst);
}

// mbgc_fasta_match_headers_dev: one wave per header, SEL_TILE positions at a time (the two lane steps: fasta_select.h). A block is one
// wave, so the barrier between the steps stands in a loop whose trip count differs from header to header. The wave leaves its header
// at the first tile with a hit, and one lane sets the record's bit: records share words, hence the atomic; no hit, no atomic.
__global__ void __launch_bounds__(WAVE) k_fa_match_headers(const uint8_t *__restrict__ headers, const uint64_t *__restrict__ hdrOff, const uint64_t *__restrict__ hdrLen,
                                                           uint64_t nrec, uint32_t m, const SelSlot *__restrict__ slots, uint32_t bits,
                                                           const SelPat *__restrict__ pats, const uint8_t *__restrict__ patBytes, uint32_t *__restrict__ chosen) {
    __shared__ uint8_t stage[SEL_STAGE + 1];
    const uint32_t lane = threadIdx.x;
    for (uint64_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        const uint8_t *hdr = headers + hdrOff[r];
        const uint64_t len = hdrLen[r];
        for (uint64_t base = 0; base + m <= len; base += SEL_TILE) {     // (uniform over the wave)
            sel_stage_step(hdr, len, base, lane, m, stage);
            __syncthreads();
            const bool hit = sel_lane_step(hdr, len, base, lane, m, stage, slots, bits, pats, patBytes);
            const unsigned long long any = __ballot(hit);
            __syncthreads();                                             // (the next tile's stores wait for this tile's reads)
            if (any) {
                if (lane == 0) atomicOr(chosen + (r >> 5), 1u << (r & 31));
                break;
            }
        }
    }
}

// mbgc_fasta_find_dev: a block takes tile after tile of the flat list over all records (the record by bisection of the tiles' prefix sum,
// the two lane steps: fasta_find.h). The table is copied to LDS once per block when it fits (LDS_TABLE), and read where it lies in
// global memory — from L2 — otherwise. A hit takes a row of the buffer through the one cursor; rows at or past the capacity are
// counted and not written, so the cursor ends as the exact count.
template <bool LDS_TABLE>
__global__ void __launch_bounds__(FIND_THREADS) k_fa_find(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                          uint32_t nrec, uint64_t ntiles, const FindSlot *__restrict__ slotsGlobal, uint32_t bits,
                                                          const FindSeed *__restrict__ seeds, const FindPat *__restrict__ pats, const uint8_t *__restrict__ patBytes, uint32_t K,
                                                          mbgc_fasta_hit_t *__restrict__ hits, uint64_t hitCap, unsigned long long *__restrict__ cursor) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FIND_STAGE];
    __shared__ FindSlot slotsLds[LDS_TABLE ? (1u << FIND_LDS_BITS) : 1];
    const uint32_t lane = threadIdx.x;
    if (LDS_TABLE) for (uint32_t s = lane; s < (1u << bits); s += FIND_THREADS) slotsLds[s] = slotsGlobal[s];   // (visible behind the first tile's barrier)
    const FindSlot *slots = LDS_TABLE ? slotsLds : slotsGlobal;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {     // (uniform over the block)
        const ScanTile T = scan_tile(seq, recs, tileStart, nrec, tile);
        const uint32_t r = T.r;
        const ScanRec rec = T.rec;
        const uintptr_t tileAddr = T.addr;
        find_stage_step(seq, seqBytes, tileAddr, lane, stage);
        if (lane == 0) find_stage_step(seq, seqBytes, tileAddr, FIND_VECS - 1, stage);
        __syncthreads();
        find_lane_step(seq, rec, tileAddr, lane, stage, slots, bits, seeds, pats, patBytes, K, [&](uint64_t pos, uint32_t pat, uint32_t d) {
            const unsigned long long at = atomicAdd(cursor, 1ull);
            if (at < hitCap) hits[at] = mbgc_fasta_hit_t{pos, r, pat, d, 0u};
        });
        __syncthreads();                                                     // (the next tile's stores wait for this tile's reads)
    }
}

// mbgc_fasta_find_iupac_dev: k_fa_find's grid, staging, cursor and hit buffer with the matcher of fasta_find_iupac.h. The bitmap of the
// grams that have a chain — 8 KiB whatever the patterns are — is copied to LDS once per block; the chains' starts and the rows are read
// where they lie in global memory, from L2, and only behind a set bit. stats[0] is the cursor; stats[IUPAC_WALKED], a cache line of
// its own, the rows walked: summed over the wave by shuffles, one add per wave and tile that walked any.
__global__ void __launch_bounds__(FIND_THREADS) k_fa_find_iupac(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                                uint32_t nrec, uint64_t ntiles, const uint32_t *__restrict__ bitmapGlobal, const uint32_t *__restrict__ gramStart,
                                                                const IupacRow *__restrict__ rows, const IupacPat *__restrict__ pats, const uint8_t *__restrict__ masks, uint32_t K,
                                                                mbgc_fasta_hit_t *__restrict__ hits, uint64_t hitCap, unsigned long long *__restrict__ stats) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FIND_STAGE];
    __shared__ uint32_t bitmap[IUPAC_BITMAP_WORDS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t s = lane; s < IUPAC_BITMAP_WORDS; s += FIND_THREADS) bitmap[s] = bitmapGlobal[s];      // (visible behind the first tile's barrier)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {     // (uniform over the block)
        const ScanTile T = scan_tile(seq, recs, tileStart, nrec, tile);
        const uint32_t r = T.r;
        find_stage_step(seq, seqBytes, T.addr, lane, stage);
        if (lane == 0) find_stage_step(seq, seqBytes, T.addr, FIND_VECS - 1, stage);
        __syncthreads();
        const uint32_t walked = iupac_lane_step(seq, T.rec, T.addr, lane, stage, bitmap, gramStart, rows, pats, masks, K, [&](uint64_t pos, uint32_t pat, uint32_t d) {
            const unsigned long long at = atomicAdd(stats, 1ull);
            if (at < hitCap) hits[at] = mbgc_fasta_hit_t{pos, r, pat, d, 0u};
        });
        uint32_t waveWalked = walked;                                        // (every lane of the block is here: the tile loop is uniform)
#pragma unroll
        for (uint32_t d = WAVE / 2; d; d >>= 1) waveWalked += __shfl_xor(waveWalked, d);
        if (waveWalked && (lane & (WAVE - 1)) == 0) atomicAdd(stats + IUPAC_WALKED, (unsigned long long) waveWalked);
        __syncthreads();                                                     // (the next tile's stores wait for this tile's reads)
    }
}

// mbgc_fasta_stats_dev: a block takes tile after tile of the flat list over all records, as k_fa_find does (the lane steps: fasta_stats.h).
// Nothing is staged in LDS: every byte is looked at by one lane, which has it in its own vector, and the one bit a lane needs from each
// neighbour comes by a shuffle (the first and last lane of a wave: one guarded byte load). Counts: the lanes' two packed words are
// summed over the wave by shuffles and over the block through 64 bytes of LDS; lanes 0..6 keep one counter each in a register while
// the block's tiles stay in one record and add it to the record's row when the record changes — at most seven atomic adds per tile.
// Edges: a lane takes as many rows as it has edges through the one cursor; rows at or past the capacity are counted and not written.
__global__ void __launch_bounds__(STATS_THREADS) k_fa_stats(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                            uint32_t nrec, uint64_t ntiles, uint32_t counting, uint32_t want, unsigned long long *__restrict__ counts,
                                                            StatsEdge *__restrict__ edges, uint64_t edgeCap, unsigned long long *__restrict__ cursor) {
    __shared__ uint64_t sums[2][STATS_THREADS / WAVE][2];
    const uint32_t lane = threadIdx.x, wl = lane & (WAVE - 1), wave = lane / WAVE;
    uint64_t mine = 0;                                                       // lanes 0..6: counter `lane` of record `held`, not yet added to its row
    uint32_t held = 0, parity = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, parity ^= 1) {     // (uniform over the block)
        const ScanTile T = scan_tile(seq, recs, tileStart, nrec, tile);
        const uint32_t r = T.r;
        const ScanRec rec = T.rec;
        const uintptr_t tileAddr = T.addr;
        const StatsLane L = stats_lane_step(seq, seqBytes, rec, tileAddr, lane);
        const int64_t t0 = (int64_t) (tileAddr + 16u * lane) - (int64_t) ((uintptr_t) seq + rec.off);
        if (want) {
            uint32_t prevLast = stats_last_of(__shfl_up(L.masks, 1)), nextFirst = stats_first_of(__shfl_down(L.masks, 1));
            if (wl == 0) prevLast = stats_class_at(seq, rec, t0 - 1);
            if (wl == WAVE - 1) nextFirst = stats_class_at(seq, rec, t0 + STATS_PER);
            const StatsEdges E = stats_edges(L.masks, prevLast, nextFirst, want);
            const uint32_t cnt = stats_edge_count(E);
            if (cnt) stats_edges_write(E, t0, r, atomicAdd(cursor, (unsigned long long) cnt), edgeCap, edges);
        }
        if (counting) {
            uint64_t a = L.sumA, b = L.sumB;
#pragma unroll
            for (int d = WAVE / 2; d; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
            if (wl == 0) { sums[parity][wave][0] = a; sums[parity][wave][1] = b; }
            __syncthreads();                                                 // (the other buffer is the next tile's: one barrier per tile)
            if (lane < 7) {
                if (r != held) { if (mine) atomicAdd(counts + 8ull * held + lane, (unsigned long long) mine); mine = 0; held = r; }
                a = b = 0;
#pragma unroll
                for (uint32_t w = 0; w < STATS_THREADS / WAVE; w++) { a += sums[parity][w][0]; b += sums[parity][w][1]; }
                mine += stats_counter(a, b, lane);
            }
        }
    }
    if (counting && lane < 7 && mine) atomicAdd(counts + 8ull * held + lane, (unsigned long long) mine);
}

// mbgc_fasta_dups_dev, the first scan: a block takes tile after tile of the flat list over all records, as k_fa_stats does (the lane steps
// and the arithmetic: fasta_dups.h). One read of the text yields both strands' sums: a lane turns its own aligned vector into eight
// residues (four primes, forward and reverse), multiplies them with its own power z^(16 lane) — computed once per launch —, the wave
// adds them modulo the primes by shuffles, the block through 256 bytes of LDS; lanes 0..7 multiply one residue each with the tile's
// power, which the first wave keeps (by squaring when the block comes to a record, by one multiplication while it stays in it), and
// hold the sum in a register while the block's tiles stay in one record: at most eight 64-bit atomic adds per tile, of terms below
// 2^31. The host reduces a record's row modulo the primes (dups_finish).
__global__ void __launch_bounds__(DUPS_THREADS) k_fa_dups(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint64_t *__restrict__ tileStart,
                                                           uint32_t nrec, uint64_t ntiles, uint32_t exactCase, unsigned long long *__restrict__ rows) {
    __shared__ uint32_t sums[2][DUPS_THREADS / WAVE][8];
    const uint32_t lane = threadIdx.x, wl = lane & (WAVE - 1), wave = lane / WAVE;
    uint32_t lanePw[8], stride[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    dups_pow8(16ull * lane, lanePw);
    if (wave == 0) dups_pow8((uint64_t) DUPS_TILE * gridDim.x, stride);
    uint64_t mine = 0;                                                       // lanes 0..7: residue `lane` of record `held`, not yet added to its row
    uint32_t held = 0, parity = 0, powerOf = 0;
    bool powered = false;                                                    // pw is the power of record powerOf's tile gridDim.x in front of this one
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, parity ^= 1) {     // (uniform over the block)
        const ScanTile T = scan_tile(seq, recs, tileStart, nrec, tile);
        const uint32_t r = T.r;
        const ScanRec rec = T.rec;
        const uintptr_t first = (uintptr_t) seq + rec.off, tileAddr = T.addr;
        uint32_t v[8], other[8];
        dups_lane_step(seq, seqBytes, rec, tileAddr, lane, exactCase != 0, v);
        dups_mul8(v, lanePw);
#pragma unroll
        for (int d = WAVE / 2; d; d >>= 1) {
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) other[q] = __shfl_xor(v[q], d);
            dups_add8(v, other);
        }
        if (wl == 0)
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) sums[parity][wave][q] = v[q];
        if (wave == 0) {
            if (powered && powerOf == r) dups_mul8(pw, stride);
            else dups_pow8(dups_tile_exp(first, tile - tileStart[r]), pw);
            powered = true; powerOf = r;
        }
        __syncthreads();                                                     // (the other buffer is the next tile's: one barrier per tile)
        if (lane < 8) {
            if (r != held) { if (mine) atomicAdd(rows + 8ull * held + lane, (unsigned long long) mine); mine = 0; held = r; }
            uint64_t sum = 0;
#pragma unroll
            for (uint32_t w = 0; w < DUPS_THREADS / WAVE; w++) sum += sums[parity][w][lane];
            mine += dups_tile_term(lane, sum, pw);
        }
    }
    if (lane < 8 && mine) atomicAdd(rows + 8ull * held + lane, (unsigned long long) mine);
}

// mbgc_fasta_dups_dev, the exactness step: a block per pair of the list (record, candidate representative, strand), striding. The
// record's side is walked on the 16-byte grid with aligned vectors, the representative's side is read where the same positions lie,
// forward or mirrored and complemented (dups_verify_step). One ballot per step; a wave stops at its first difference. A pair that
// differs costs one atomic, a pair that is equal none.
__global__ void __launch_bounds__(DUPS_THREADS) k_fa_dups_verify(const uint8_t *__restrict__ seq, const ScanRec *__restrict__ recs, const DupsPair *__restrict__ pairs, uint32_t npairs,
                                                                  uint32_t exactCase, uint32_t *__restrict__ refuted) {
    __shared__ uint32_t differs[DUPS_THREADS / WAVE];
    const uint32_t lane = threadIdx.x, wl = lane & (WAVE - 1), wave = lane / WAVE;
    for (uint32_t pair = blockIdx.x; pair < npairs; pair += gridDim.x) {     // (uniform over the block)
        const DupsPair P = pairs[pair];
        const ScanRec a = recs[P.rec], b = recs[P.rep];
        const uintptr_t first = (uintptr_t) seq + a.off;
        const uint64_t steps = scan_tiles_of(first, a.len);
        bool differ = false;                                                 // (uniform over the wave)
        for (uint64_t s = 0; s < steps && !differ; s++)
            differ = __ballot(dups_verify_step(seq, a, b, P.strand, exactCase != 0, (first & ~(uintptr_t) 15) + s * DUPS_TILE, lane)) != 0;
        if (wl == 0) differs[wave] = differ;
        __syncthreads();
        if (lane == 0 && (differs[0] | differs[1] | differs[2] | differs[3])) atomicOr(refuted + pair, 1u);
        __syncthreads();                                                     // (the next pair's stores wait for this pair's read)
    }
}

// mbgc_fasta_sketch_dev: a block takes tile after tile of the flat list over all records, as k_fa_stats does (the lane steps:
// fasta_sketch.h). A lane packs its own aligned vector into a code word and an invalid mask and takes the same of the two vectors
// behind it by shuffles; the last two lanes of a wave pack what lies behind the wave themselves (guarded: a vector outside the record is
// not read). Rows: a lane keeps the hashes <= maxHash among its 16, the wave sums the lanes' counts by a scan of shuffles and takes its
// rows from the one cursor with ONE atomic add per wave and tile, none when the ballot says no lane keeps one; rows at or past the
// capacity are counted and not written. kmers: the valid positions summed over the wave, held in a register while the block's tiles
// stay in one group, one atomic add per wave when the group changes.
__global__ void __launch_bounds__(SKETCH_THREADS) k_fa_sketch(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint32_t *__restrict__ groups,
                                                              const uint64_t *__restrict__ tileStart, uint32_t nrec, uint64_t ntiles, uint32_t k, uint64_t maxHash,
                                                              unsigned long long *__restrict__ kmers, uint64_t *__restrict__ rowHash, uint32_t *__restrict__ rowGroup, uint64_t rowCap,
                                                              unsigned long long *__restrict__ cursor) {
    const uint32_t lane = threadIdx.x, wl = lane & (WAVE - 1);
    uint64_t mine = 0;                                                       // the wave's valid positions of group `held`, not yet added (the same in every lane)
    uint32_t held = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {     // (uniform over the block)
        const uint32_t r = scan_tile_record(tileStart, nrec, tile);
        const uint32_t g = groups[r];
        const ScanTile T = scan_tile_of(seq, recs, tileStart, r, tile);
        const ScanRec rec = T.rec;
        const uintptr_t v = T.addr + 16u * lane;
        const uint64_t own = sketch_pack(seq, seqBytes, rec, v);
        uint64_t next1 = __shfl_down(own, 1), next2 = __shfl_down(own, 2);
        if (wl == WAVE - 1) next1 = sketch_pack(seq, seqBytes, rec, v + 16);
        if (wl >= WAVE - 2) next2 = sketch_pack(seq, seqBytes, rec, v + 32);
        uint64_t h[SKETCH_PER];
        const uint32_t valid = sketch_lane_hashes(own, next1, next2, k, h);
        uint32_t keep = 0;
#pragma unroll
        for (uint32_t j = 0; j < SKETCH_PER; j++) if (((valid >> j) & 1u) && h[j] <= maxHash) keep |= 1u << j;
        uint32_t nv = (uint32_t) __builtin_popcount(valid);
#pragma unroll
        for (int d = WAVE / 2; d; d >>= 1) nv += __shfl_xor(nv, d);
        if (g != held) { if (wl == 0 && mine) atomicAdd(kmers + held, (unsigned long long) mine); mine = 0; held = g; }
        mine += nv;
        const uint32_t cnt = (uint32_t) __builtin_popcount(keep);
        if (__ballot(cnt != 0) == 0) continue;                               // (uniform over the wave)
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (wl >= (uint32_t) d) incl += up; }
        unsigned long long base = 0;
        if (wl == WAVE - 1) base = atomicAdd(cursor, (unsigned long long) incl);
        uint64_t at = __shfl(base, WAVE - 1) + incl - cnt;
#pragma unroll
        for (uint32_t j = 0; j < SKETCH_PER; j++)
            if ((keep >> j) & 1u) {
                if (at < rowCap) { rowHash[at] = h[j]; rowGroup[at] = g; }
                at++;
            }
    }
    if (wl == 0 && mine) atomicAdd(kmers + held, (unsigned long long) mine);
}

// the rows sorted by (group, hash): flag[i] = row i is the first of its (group, hash)
__global__ void __launch_bounds__(256) k_fa_sketch_flag(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ group, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        flag[i] = i == 0 || group[i] != group[i - 1] || hash[i] != hash[i - 1];
}

// pos = the exclusive sum of the flags: a flagged row goes to out[pos]; the first row of a group leaves its place in groupStart (the
// groups without a row keep the host's filling); the last row leaves the number of distinct rows
__global__ void __launch_bounds__(256) k_fa_sketch_compact(const uint64_t *__restrict__ hash, const uint32_t *__restrict__ group, const uint32_t *__restrict__ flag,
                                                           const uint32_t *__restrict__ pos, uint64_t n, uint64_t *__restrict__ out, unsigned long long *__restrict__ groupStart,
                                                           unsigned long long *__restrict__ total) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        if (flag[i]) {
            out[pos[i]] = hash[i];
            if (i == 0 || group[i] != group[i - 1]) groupStart[group[i]] = pos[i];
        }
        if (i == n - 1) *total = (unsigned long long) pos[i] + flag[i];
    }
}

// mbgc_fasta_screen_dev: k_fa_sketch's scan with another question (the lane steps: fasta_screen.h). The filter is copied into the block's
// LDS once, in front of the block's tiles. A lane forms the canonical words of its 16 positions, asks the filter about every valid one
// and, on a set bit, reads the word's first slot of the table — all 16 positions before one answer is looked at, then the keys behind the
// slots, so the loads of a lane travel together —; a key that is another's sends the lane down the probe. Rows: the sketch kernel's
// ballot, scan and ONE atomic add per wave and tile; a row is group << keyBits | key index for the found lists and, when the hits are
// asked for (rowPos != nullptr), the position and rec << 32 | key index; rows at or past the capacity are counted and not written.
// words[0]: the cursor; words[2]: the valid positions that passed the filter, one atomic add per wave at the end.
__global__ void __launch_bounds__(SCREEN_THREADS) k_fa_screen(const uint8_t *__restrict__ seq, uint64_t seqBytes, const ScanRec *__restrict__ recs, const uint32_t *__restrict__ groups,
                                                              const uint64_t *__restrict__ tileStart, uint32_t nrec, uint64_t ntiles, uint32_t k, const uint32_t *__restrict__ filterWords,
                                                              const uint32_t *__restrict__ table, uint32_t slotMask, const uint64_t *__restrict__ keys, uint32_t keyBits,
                                                              uint64_t *__restrict__ rowGroupKey, uint64_t *__restrict__ rowPos, uint64_t *__restrict__ rowRecKey, uint64_t rowCap,
                                                              unsigned long long *__restrict__ words) {
    __shared__ ScanVec filterVec[SCREEN_FILTER_WORDS / 4];
    for (uint32_t i = threadIdx.x; i < SCREEN_FILTER_WORDS / 4; i += SCREEN_THREADS) filterVec[i] = ((const ScanVec *) filterWords)[i];
    __syncthreads();
    const uint32_t *filter = (const uint32_t *) filterVec;
    const uint32_t lane = threadIdx.x, wl = lane & (WAVE - 1);
    uint32_t passed = 0;                                                     // the lane's own
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {     // (uniform over the block)
        const uint32_t r = scan_tile_record(tileStart, nrec, tile);
        const uint32_t g = groups[r];
        const ScanTile T = scan_tile_of(seq, recs, tileStart, r, tile);
        const ScanRec rec = T.rec;
        const uintptr_t v = T.addr + 16u * lane;
        const uint64_t own = sketch_pack(seq, seqBytes, rec, v);
        uint64_t next1 = __shfl_down(own, 1), next2 = __shfl_down(own, 2);
        if (wl == WAVE - 1) next1 = sketch_pack(seq, seqBytes, rec, v + 16);
        if (wl >= WAVE - 2) next2 = sketch_pack(seq, seqBytes, rec, v + 32);
        uint64_t c[SCREEN_PER];
        const uint32_t valid = screen_lane_canons(own, next1, next2, k, c);
        uint32_t e[SCREEN_PER], pass = 0;
#pragma unroll
        for (uint32_t j = 0; j < SCREEN_PER; j++) {
            e[j] = 0;
            if (((valid >> j) & 1u) && screen_first(filter, table, slotMask, c[j], e[j])) pass |= 1u << j;
        }
        passed += (uint32_t) __builtin_popcount(pass);
        uint64_t behind[SCREEN_PER];
#pragma unroll
        for (uint32_t j = 0; j < SCREEN_PER; j++) behind[j] = e[j] ? keys[e[j] - 1] : 0;
        uint32_t keep = 0;
#pragma unroll
        for (uint32_t j = 0; j < SCREEN_PER; j++) {
            uint32_t steps = 0;
            if (e[j]) e[j] = screen_confirm(table, slotMask, keys, c[j], e[j], behind[j], steps);
            if (e[j]) keep |= 1u << j;
        }
        const uint32_t cnt = (uint32_t) __builtin_popcount(keep);
        if (__ballot(cnt != 0) == 0) continue;                               // (uniform over the wave)
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (wl >= (uint32_t) d) incl += up; }
        unsigned long long base = 0;
        if (wl == WAVE - 1) base = atomicAdd(words, (unsigned long long) incl);
        uint64_t at = __shfl(base, WAVE - 1) + incl - cnt;
        const uint64_t t0 = (uint64_t) ((int64_t) v - (int64_t) ((uintptr_t) seq + rec.off));    // the lane's first position in the record (a kept position is inside it)
#pragma unroll
        for (uint32_t j = 0; j < SCREEN_PER; j++)
            if ((keep >> j) & 1u) {
                if (at < rowCap) {
                    rowGroupKey[at] = (uint64_t) g << keyBits | (uint64_t) (e[j] - 1);
                    if (rowPos) { rowPos[at] = t0 + j; rowRecKey[at] = (uint64_t) r << 32 | (uint64_t) (e[j] - 1); }
                }
                at++;
            }
    }
#pragma unroll
    for (int d = WAVE / 2; d; d >>= 1) passed += __shfl_xor(passed, d);
    if (wl == 0 && passed) atomicAdd(words + 2, (unsigned long long) passed);
}

// the rows sorted by group << keyBits | key: flag[i] = row i is the first of its (group, key)
__global__ void __launch_bounds__(256) k_fa_screen_flag(const uint64_t *__restrict__ groupKey, uint64_t n, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        flag[i] = i == 0 || groupKey[i] != groupKey[i - 1];
}

// k_fa_sketch_compact for these rows: a flagged row's key index goes to out[pos]; the first row of a group leaves its place in
// groupStart (the groups without a row keep the host's filling); the last row leaves the number of distinct rows
__global__ void __launch_bounds__(256) k_fa_screen_compact(const uint64_t *__restrict__ groupKey, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint64_t n,
                                                           uint32_t keyBits, uint32_t *__restrict__ out, unsigned long long *__restrict__ groupStart,
                                                           unsigned long long *__restrict__ total) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        if (flag[i]) {
            out[pos[i]] = (uint32_t) (groupKey[i] & (((uint64_t) 1 << keyBits) - 1));
            if (i == 0 || groupKey[i] >> keyBits != groupKey[i - 1] >> keyBits) groupStart[groupKey[i] >> keyBits] = pos[i];
        }
        if (i == n - 1) *total = (unsigned long long) pos[i] + flag[i];
    }
}

// mbgc_fasta_sketch_pairs_dev: a wave per pair. The lanes stride over the shorter of the two strictly ascending lists, each lane looks
// its hash up in the longer one by bisection; the finds are counted by ballot and popcount — no atomics, the count is the wave's own.
__global__ void __launch_bounds__(256) k_fa_sketch_pairs(const uint64_t *__restrict__ hashes, const uint64_t *__restrict__ start, uint32_t ngroups, const uint32_t *__restrict__ pairs,
                                                         uint64_t npairs, uint32_t *__restrict__ shared) {
    const uint32_t wl = threadIdx.x & (WAVE - 1), waves = blockDim.x / WAVE;
    for (uint64_t q = (uint64_t) blockIdx.x * waves + threadIdx.x / WAVE; q < npairs; q += (uint64_t) gridDim.x * waves) {      // (uniform over the wave)
        uint32_t i, j;
        if (pairs) { i = pairs[2 * q]; j = pairs[2 * q + 1]; } else sketch_pair_of(q, ngroups, i, j);
        uint64_t a0 = start[i], na = start[i + 1] - a0, b0 = start[j], nb = start[j + 1] - b0;
        if (na > nb) { const uint64_t t0 = a0, tn = na; a0 = b0; na = nb; b0 = t0; nb = tn; }
        uint32_t cnt = 0;
        for (uint64_t at = 0; at < na; at += WAVE) {                         // (na == 0: an empty side, nothing is searched)
            const bool found = at + wl < na && sketch_holds(hashes + b0, nb, hashes[a0 + at + wl]);
            cnt += (uint32_t) __popcll(__ballot(found));
        }
        if (wl == 0) shared[q] = cnt;
    }
}

// mbgc_fasta_crc_dev: a wave per 64 / G rows of one class (the lane step, the classes and the tables: fasta_crc.h). The lanes of a group
// fold their values by shuffles; a row that is a whole range stores its word, a piece of a cut range moves its value over the bytes
// behind it (the lanes' factors multiplied by shuffles) and XORs it into the range's word.
template <uint32_t LOOKUP>
__global__ void __launch_bounds__(CRC_THREADS) k_fa_crc(const uint8_t *__restrict__ seq, const CrcRow *__restrict__ rows, const uint64_t *__restrict__ behind,
                                                        const CrcPlan plan, const CrcConsts *__restrict__ K, uint32_t *__restrict__ out) {
    __shared__ CrcShared<LOOKUP> S;
    crc_fill_shared(S, K, threadIdx.x, CRC_THREADS);
    __syncthreads();
    const uint32_t lane = threadIdx.x & (CRC_LANES - 1), nwaves = plan.wave0[CRC_CLASSES];
    for (uint32_t w = blockIdx.x * CRC_WAVES + threadIdx.x / CRC_LANES; w < nwaves; w += gridDim.x * CRC_WAVES) {     // (the same w for a whole wave)
        uint32_t c = 0, wave0 = plan.wave0[0], row0 = plan.row0[0], rowEnd = plan.row0[1];
#pragma unroll
        for (uint32_t k = 1; k < CRC_CLASSES; k++)
            if (w >= plan.wave0[k]) { c = k; wave0 = plan.wave0[k]; row0 = plan.row0[k]; rowEnd = plan.row0[k + 1]; }
        const uint32_t G = 1u << (2 * c), row = row0 + (w - wave0) * (CRC_LANES >> (2 * c)) + (lane >> (2 * c));
        CrcRow R = {0, 0, 0};
        uint32_t v = 0;
        if (row < rowEnd) { R = rows[row]; v = crc_lane_step<LOOKUP>(seq, R, G, lane, S); }
        for (uint32_t d = 1; d < G; d <<= 1) v ^= (uint32_t) __shfl_xor((int) v, (int) d);
        if (c + 1 < CRC_CLASSES) {
            if ((lane & (G - 1)) == 0 && row < rowEnd) out[R.rec & ~CRC_FIRST] = v;
            continue;
        }
        const uint64_t b = behind[row - row0];                             // (one row per wave: uniform)
        if (b) {
            uint32_t f = crc_pow_lane(b, lane, S);
            for (uint32_t d = 1; d < CRC_LANES; d <<= 1) f = crc_mulmod(f, (uint32_t) __shfl_xor((int) f, (int) d));
            v = crc_mulmod(v, f);
        }
        if (lane == 0) atomicXor(out + (R.rec & ~CRC_FIRST), v);
    }
}

// pieces of a device buffer packed back to back, each followed by one separator byte (the headers of a -i batch: only they travel
// back to the host, not the elements): one workgroup per piece
__global__ void __launch_bounds__(THREADS) k_fa_gather(const uint8_t *__restrict__ src, const uint64_t *__restrict__ tab, uint32_t piece0, uint32_t npieces,
                                                       uint8_t sep, uint8_t *__restrict__ dst) {       // tab: rows of {source offset, length, destination offset}
    const uint32_t k = piece0 + blockIdx.x;
    if (k >= npieces) return;
    const uint64_t so = tab[3 * (uint64_t) k], len = tab[3 * (uint64_t) k + 1], to = tab[3 * (uint64_t) k + 2];
    for (uint64_t i = threadIdx.x; i < len; i += THREADS) dst[to + i] = src[so + i];
    if (threadIdx.x == 0) dst[to + len] = sep;
}

// ---- the protein-profile probe (MGMP_Params::probeProteinsProfile, matching/MGMP_Params.h:86-127; rule in mbgc_fasta.h)
// The host clips the records to what the probe still takes (index arithmetic on the record table, which it holds) and leaves out
// the empty ones; the bytes are counted and the rule's predicate is evaluated here, where the contigs lie.
struct ProbeRec { uint64_t off; uint32_t len, index; };          // where the record lies, its clipped length (> 0), its number in the caller's table
struct ProbeOut { int32_t fired, remaining, nonStd, pad; uint64_t record; };

constexpr uint64_t probe_bit(char c) { return 1ull << (c - 64); }      // the standard symbols all lie in 64..127
constexpr uint64_t PROBE_STD = probe_bit('a') | probe_bit('c') | probe_bit('g') | probe_bit('t') | probe_bit('u') | probe_bit('A') |
                               probe_bit('C') | probe_bit('G') | probe_bit('T') | probe_bit('U') | probe_bit('N');
__device__ __forceinline__ uint32_t probe_non_std(uint32_t c) { return (c >> 6) != 1u || !((PROBE_STD >> (c & 63u)) & 1u) ? 1u : 0u; }

// one wave per record: 16 bytes per lane and step, the record's non-standard bytes counted by ballots
__global__ void __launch_bounds__(THREADS) k_fa_probe_count(const uint8_t *__restrict__ seq, const ProbeRec *__restrict__ recs, uint32_t nrec,
                                                            uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), wavesPerBlock = THREADS / WAVE;
    for (uint32_t r = blockIdx.x * wavesPerBlock + threadIdx.x / WAVE; r < nrec; r += gridDim.x * wavesPerBlock) {   // (the same r for a whole wave)
        const uint8_t *src = seq + recs[r].off;
        const uint32_t len = recs[r].len;
        uint32_t cnt = 0;
        for (uint32_t base = 0; base < len; base += WAVE * PER) {
            const uint32_t o = base + lane * PER;
            uint32_t bad = 0;                                            // bit j: byte o + j is non-standard
            if (o + PER <= len) {
                uint4 t;
                memcpy(&t, src + o, PER);
                const uint32_t w[4] = {t.x, t.y, t.z, t.w};
                for (int j = 0; j < PER; j++) bad |= probe_non_std((w[j >> 2] >> (8 * (j & 3))) & 0xffu) << j;
            } else
                for (uint32_t q = o; q < len && q < o + PER; q++) bad |= probe_non_std(src[q]) << (q - o);
            for (int j = 0; j < PER; j++) cnt += (uint32_t) __popcll(__ballot((bad >> j) & 1u));
        }
        if (lane == 0) counts[r] = cnt;
    }
}

// one wave walks the records in order, 64 at a time: prefix sums of the clipped lengths and the counts give every record the
// state the reference has behind it; the first record whose predicate holds fires
__global__ void __launch_bounds__(WAVE) k_fa_probe_walk(const ProbeRec *__restrict__ recs, const uint32_t *__restrict__ counts, uint32_t nrec,
                                                        int32_t remaining, int32_t nonStd, int32_t k, ProbeOut *__restrict__ out) {
    const uint32_t lane = threadIdx.x;
    int32_t fired = 0, record = 0;
    for (uint32_t base = 0; base < nrec && !fired; base += WAVE) {
        const uint32_t r = base + lane;
        const int32_t len = r < nrec ? (int32_t) recs[r].len : 0, cnt = r < nrec ? (int32_t) counts[r] : 0;
        const int32_t index = r < nrec ? (int32_t) recs[r].index : 0;
        int32_t sumLen = len, sumCnt = cnt;                             // inclusive
        for (int d = 1; d < WAVE; d <<= 1) {
            const int32_t y = __shfl_up(sumLen, d), z = __shfl_up(sumCnt, d);
            if ((int) lane >= d) { sumLen += y; sumCnt += z; }
        }
        const int32_t probeLen = MBGC_FASTA_PROBE_MAX_LEN - (remaining - sumLen), running = nonStd + sumCnt;
        const bool fire = len > 0 && probeLen >= MBGC_FASTA_PROBE_MIN_LEN && k != 16 && running * 100 / (len > 0 ? len : 1) > 10;
        const unsigned long long m = __ballot(fire);
        if (m) {
            const int f = __ffsll(m) - 1;
            fired = 1; record = __shfl(index, f);
            remaining = 0; nonStd = __shfl(running, f);
        } else {
            remaining -= __shfl(sumLen, WAVE - 1); nonStd += __shfl(sumCnt, WAVE - 1);
        }
    }
    if (lane == 0) { out->fired = fired; out->remaining = remaining; out->nonStd = nonStd; out->pad = 0; out->record = (uint64_t) (uint32_t) record; }
}

std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define FCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fa::fail(-100, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define FTRY(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)      // a step that has said itself what failed

// a device array of the handle's: it grows and is never shrunk, and is freed with the handle (mbgc_fasta_destroy deletes it)
template <class T>
struct Buf {
    T *p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { if (p) (void) hipFree(p); }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        if (p) (void) hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = n + n / 4 + 64;
        if (hipMalloc((void **) &p, want * sizeof(T)) != hipSuccess) return fail(-101, "device allocation of %zu bytes failed", want * sizeof(T));
        cap = want;
        return 0;
    }
};

// the time of a stretch of a stream, by a pair of events made at the first start that wants it: start() in front of the launches,
// stop() behind them, read() behind the synchronise. A start that does not want the time makes the other two do nothing.
struct Timer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool on = false;
    int start(hipStream_t stream, bool wanted = true) {
        on = wanted;
        if (!on) return 0;
        for (hipEvent_t &e : ev) if (!e) FCHK(hipEventCreate(&e));
        FCHK(hipEventRecord(ev[0], stream));
        return 0;
    }
    int stop(hipStream_t stream) {
        if (on) FCHK(hipEventRecord(ev[1], stream));
        return 0;
    }
    int read(double *ms) {                                             // (ms == nullptr: the caller does not ask)
        float t = 0;
        if (on && ms) { FCHK(hipEventElapsedTime(&t, ev[0], ev[1])); *ms = t; }
        return 0;
    }
    void destroy() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};

}  // namespace fa

struct mbgc_fasta {
    int device = 0;
    hipStream_t stream = nullptr;
    fa::Buf<fa::FileDesc> dFiles;
    fa::Buf<uint32_t> dOwner;
    fa::Buf<fa::ChunkSum> dSums;
    fa::Buf<fa::ChunkIn> dIns;
    fa::Buf<fa::FileOut> dOut;
    fa::Buf<uint64_t> dBases;
    fa::Buf<mbgc_fasta_record_t> dRecs;
    fa::Buf<uint64_t> dShift;                   // lossy rule: every file's bytes in front of its first marker
    fa::Buf<uint8_t> dHostIn, dHostOut;         // mbgc_fasta_parse_host: the file and its sequences on the device
    fa::Buf<uint32_t> dTileFirst;               // mbgc_fasta_split_dev: first '>' (first mark, under tileFlags) of every tile, and its result
    fa::Buf<uint64_t> dSplit;
    uint32_t tileFlags = 0;                     // the flags dTileFirst was made with
    fa::Buf<fa::FmtRec> dFmtRecs;               // mbgc_fasta_format_dev: the record table and the tiles' owners
    fa::Buf<uint32_t> dFmtOwner;
    fa::Timer timer;                            // around the launches of whichever entry point runs (one call at a time uses the handle)
    fa::Buf<fa::CmpPiece> dCmpPieces;           // mbgc_fasta_compare_dev: the piece table, the tiles' owners, the slots' results
    fa::Buf<uint32_t> dCmpOwner;
    fa::Buf<unsigned long long> dCmpOut;
    fa::Buf<fa::PackPiece> dPackPieces;         // mbgc_fasta_pack_dev: the piece table and the tiles' owners
    fa::Buf<uint32_t> dPackOwner;
    fa::Buf<uint64_t> dSelRecs;                 // mbgc_fasta_match_headers_dev: the headers' offsets and lengths, the pattern table, the bits
    fa::Buf<fa::SelSlot> dSelSlots;
    fa::Buf<fa::SelPat> dSelPats;
    fa::Buf<uint8_t> dSelBytes;
    fa::Buf<uint32_t> dSelChosen;
    fa::Buf<fa::ScanRec> dScanRecs;             // scan_prepare, for find, stats, sketch and dups: the last call's records and their tiles' prefix sum
    fa::Buf<uint64_t> dScanTiles;
    std::vector<uint64_t> scanTileStart;        // the host's side of dScanTiles
    fa::Buf<fa::FindSlot> dFindSlots;           // mbgc_fasta_find_dev: the gram table, the hit rows and their cursor
    fa::Buf<fa::FindSeed> dFindSeeds;
    fa::Buf<fa::FindPat> dFindPats;
    fa::Buf<uint8_t> dFindBytes;
    fa::Buf<mbgc_fasta_hit_t> dFindHits;
    fa::Buf<unsigned long long> dFindCursor;
    fa::Buf<uint32_t> dIupacBitmap, dIupacStart;                      // mbgc_fasta_find_iupac_dev: the bitmap, the chains' starts, the rows, the patterns and
    fa::Buf<fa::IupacRow> dIupacRows;                                 // their masks, the cursor with the rows walked behind it (hits: dFindHits)
    fa::Buf<fa::IupacPat> dIupacPats;
    fa::Buf<uint8_t> dIupacMasks;
    fa::Buf<unsigned long long> dIupacStats;
    uint64_t iupacRows = 0, iupacWalked = 0;                          // the last call's: mbgc_fasta_find_iupac_last
    fa::Buf<unsigned long long> dStatsCounts;   // mbgc_fasta_stats_dev: the records' rows, the edges and their cursor
    fa::Buf<fa::StatsEdge> dStatsEdges;
    fa::Buf<unsigned long long> dStatsCursor;
    uint64_t statsEdgeCap = 0;                  // rows of dStatsEdges the kernel may write: STATS_EDGES_FIRST, then the largest count seen
    uint64_t statsEdges = 0, statsReruns = 0;   // the last call's: mbgc_fasta_stats_last
    fa::Buf<uint32_t> dSkGroups;                // mbgc_fasta_sketch_dev: the records' groups, the groups' k-mers and starts,
    fa::Buf<unsigned long long> dSkKmers, dSkStart, dSkWords;     // the cursor and the distinct total (dSkWords), the rows twice over (the sort's two sides),
    fa::Buf<uint64_t> dSkHash, dSkHash2;        // the flags, their sums and the sort's scratch
    fa::Buf<uint32_t> dSkGroup, dSkGroup2, dSkFlag, dSkPos;
    fa::Buf<uint8_t> dSkTmp;
    uint64_t sketchRowCap = 0;                  // rows the kernel may write: SKETCH_ROWS_FIRST, then the largest count seen
    uint64_t sketchRows = 0, sketchReruns = 0;  // the last call's: mbgc_fasta_sketch_last
    double sketchSortMs = 0;
    fa::Buf<uint32_t> dScrGroups, dScrFilter, dScrTable, dScrFound;    // mbgc_fasta_screen_dev: the records' groups, the filter, the table, the found lists;
    fa::Buf<uint64_t> dScrKeys, dScrGK, dScrGK2, dScrPos, dScrPos2, dScrRK, dScrRK2;     // the keys, the rows twice over (the sorts' two sides);
    fa::Buf<unsigned long long> dScrStart, dScrWords;                   // the groups' starts; the cursor, the distinct total, the filter passes
    std::vector<uint32_t> scrFilter, scrTable;                          // the host's side of filter and table (the copies may read them until the call synchronises)
    uint64_t screenRowCap = 0;                                          // rows the kernel may write: SCREEN_ROWS_FIRST, then the largest count seen
    uint64_t screenRows = 0, screenPasses = 0, screenReruns = 0;        // the last call's: mbgc_fasta_screen_last
    double screenSortMs = 0;
    fa::Timer sortTimer;                        // around the sort and the compaction (the scan: `timer`)
    fa::Buf<unsigned long long> dDupRows;       // mbgc_fasta_dups_dev: the records' eight sums, the pair list, the pairs' verdicts
    fa::Buf<fa::DupsPair> dDupPairs;
    fa::Buf<uint32_t> dDupRefuted;
    uint64_t dupBuckets = 0, dupVerified = 0, dupRefuted = 0;     // the last call's: mbgc_fasta_dups_last
    double dupVerifyMs = 0;
    fa::Buf<uint64_t> dPairHashes, dPairStart;  // mbgc_fasta_sketch_pairs_dev: the sketches, their starts, the pair list, the answers
    fa::Buf<uint32_t> dPairList, dPairShared;
    fa::Buf<fa::CrcRow> dCrcRows;               // mbgc_fasta_crc_dev: the rows, the bytes behind the cut ranges' pieces, the ranges' words, the constants
    fa::Buf<uint64_t> dCrcBehind;
    fa::Buf<uint32_t> dCrcOut;
    fa::Buf<fa::CrcConsts> dCrcConsts;
    fa::Buf<fa::InfJob> dInfJobs;               // mbgc_fasta_inflate_dev: the jobs and their results
    fa::Buf<fa::InfResult> dInfResults;
    fa::Buf<fa::DefChunk> dDefChunks;           // mbgc_fasta_deflate_dev: the chunk table, the chunks' slots and what they hold, the pack tables
    fa::Buf<uint8_t> dDefSlots;
    fa::Buf<fa::DefChunkOut> dDefOuts;
    fa::Buf<fa::DefPackIn> dDefPack;
    fa::Buf<fa::DefJobIn> dDefJobs;
    fa::Buf<uint32_t> dDefCrc;
    hipStream_t copyStream = nullptr;           // mbgc_fasta_download_begin / _wait: a download beside the kernels of `stream`
    hipEvent_t copyEv[2] = {nullptr, nullptr};
    bool copyPending = false;
    fa::Buf<uint64_t> dGatherTab;               // mbgc_fasta_gather_dev
    fa::Buf<uint8_t> dGatherOut;
    fa::Buf<fa::ProbeRec> dProbeRecs;           // mbgc_fasta_probe_dev: the clipped records, their counts, the result
    fa::Buf<uint32_t> dProbeCounts;
    fa::Buf<fa::ProbeOut> dProbeOut;
    uint64_t hostParsedBytes = 0;               // sequence bytes mbgc_fasta_parse_host2 left in dHostOut (mbgc_fasta_probe_host)
};

namespace fa {

// the first of recs[0, n) that does not lie inside a buffer of seqBytes bytes; n when all do
static uint64_t first_outside(const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint64_t seqBytes) {
    uint64_t r = 0;
    while (r < n && recs[r].off <= seqBytes && recs[r].len <= seqBytes - recs[r].off) r++;
    return r;
}

// How find, stats, dups and sketch (`what`) open: the records are counted and held to the buffer — a refusal touches nothing —, cut
// into the tiles of fasta_tiles.h, positionsOf(r) being the start positions the scan has in record r, and, when there is a tile at all,
// uploaded with the tiles' prefix sum to dScanRecs / dScanTiles on the handle's stream. -> 0 and the number of tiles, or the refusal
template <class Positions>
static int scan_prepare(mbgc_fasta *p, const char *what, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                        Positions positionsOf, uint64_t &ntiles) {
    static_assert(sizeof(ScanRec) == sizeof(mbgc_fasta_crc_rec_t), "the kernels read the ABI's ranges");
    if (n >= 0xffffffffull) return fail(-103, "%s: %llu records in one call", what, (unsigned long long) n);
    if (const uint64_t r = first_outside(recs, n, seqBytes); r < n) return fail(-103, "%s: record %llu lies outside the buffer", what, (unsigned long long) r);
    std::vector<uint64_t> &tileStart = p->scanTileStart;             // (the handle's: the copy below may read it until the entry point synchronises)
    tileStart.assign(n + 1, 0);
    for (uint64_t r = 0; r < n; r++) tileStart[r + 1] = tileStart[r] + scan_tiles_of((uintptr_t) seq_dev + recs[r].off, positionsOf(r));
    ntiles = tileStart[n];
    if (ntiles == 0) return 0;
    FCHK(hipSetDevice(p->device));
    FTRY(p->dScanRecs.reserve(n));
    FTRY(p->dScanTiles.reserve(n + 1));
    FCHK(hipMemcpyAsync(p->dScanRecs.p, recs, n * sizeof(ScanRec), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dScanTiles.p, tileStart.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    return 0;
}

}  // namespace fa

extern "C" {

const char *mbgc_fasta_last_error(void) { return fa::g_err.c_str(); }

int mbgc_fasta_create(mbgc_fasta_t **out, int device) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
        return fa::fail(-102, "no HIP device %d (the input stage has no CPU fallback)", device);
    FCHK(hipSetDevice(device));
    mbgc_fasta *p = new mbgc_fasta();
    p->device = device;
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) { delete p; return fa::fail(-100, "hipStreamCreate failed"); }
    *out = p;
    return 0;
}

void mbgc_fasta_destroy(mbgc_fasta_t *p) {
    if (!p) return;
    (void) hipSetDevice(p->device);
    if (p->stream) { (void) hipStreamSynchronize(p->stream); (void) hipStreamDestroy(p->stream); }
    if (p->copyStream) { (void) hipStreamSynchronize(p->copyStream); (void) hipStreamDestroy(p->copyStream); }
    p->timer.destroy();
    p->sortTimer.destroy();
    for (hipEvent_t e : p->copyEv) if (e) (void) hipEventDestroy(e);
    delete p;                                                         // (every fa::Buf frees itself)
}

int mbgc_fasta_parse_batch_dev2(mbgc_fasta_t *p, const uint8_t *files_dev, const uint64_t *fileOff, int nf, uint32_t flags,
                                uint8_t *seq_out_dev, uint64_t outCap, uint64_t *seqBase,
                                mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *recBase,
                                uint64_t *dnaLineLen, int *status) {
    using namespace fa;
    if (nf <= 0) return fail(-103, "empty batch");
    if (flags & ~(uint32_t) (MBGC_FASTA_UPPERCASE | MBGC_FASTA_LOSSY)) return fail(-103, "unknown parse flags %#x", flags);
    const bool lossy = flags & MBGC_FASTA_LOSSY;
    const int uppercaseDNA = (flags & MBGC_FASTA_UPPERCASE) != 0;
    FCHK(hipSetDevice(p->device));
    std::vector<FileDesc> files(nf);
    std::vector<uint32_t> owner;
    uint32_t chunks = 0;
    for (int i = 0; i < nf; i++) {
        if (fileOff[i + 1] < fileOff[i]) return fail(-103, "file offsets must ascend");
        files[i].off = fileOff[i]; files[i].n = fileOff[i + 1] - fileOff[i];
        files[i].chunk0 = chunks;
        files[i].nchunks = (uint32_t) ((files[i].n + CHUNK - 1) / CHUNK);
        owner.insert(owner.end(), files[i].nchunks, (uint32_t) i);
        chunks += files[i].nchunks;
    }
    int r;
    if ((r = p->dFiles.reserve(nf)) || (r = p->dOwner.reserve(std::max<uint32_t>(chunks, 1))) || (r = p->dSums.reserve(std::max<uint32_t>(chunks, 1))) ||
        (r = p->dIns.reserve(std::max<uint32_t>(chunks, 1))) || (r = p->dOut.reserve(nf)) || (r = p->dBases.reserve(2 * (size_t) nf + 2)) ||
        (lossy && (r = p->dShift.reserve(nf))))
        return r;
    FCHK(hipMemcpyAsync(p->dFiles.p, files.data(), nf * sizeof(FileDesc), hipMemcpyHostToDevice, p->stream));
    if (chunks) FCHK(hipMemcpyAsync(p->dOwner.p, owner.data(), chunks * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    if (lossy) {
        // (the files' chunks are counted from their whole sizes: those behind a file's cut end are empty)
        k_fa_first_marker<<<dim3(nf), dim3(THREADS), 0, p->stream>>>(files_dev, p->dFiles.p, p->dShift.p);
        if (chunks) k_fa_summary<true><<<dim3(chunks), dim3(THREADS), 0, p->stream>>>(files_dev, p->dFiles.p, p->dOwner.p, p->dSums.p);
        k_fa_scan<true><<<dim3(nf), dim3(WAVE), 0, p->stream>>>(files_dev, p->dFiles.p, p->dSums.p, p->dIns.p, p->dOut.p);
    } else {
        if (chunks) k_fa_summary<false><<<dim3(chunks), dim3(THREADS), 0, p->stream>>>(files_dev, p->dFiles.p, p->dOwner.p, p->dSums.p);
        k_fa_scan<false><<<dim3(nf), dim3(WAVE), 0, p->stream>>>(files_dev, p->dFiles.p, p->dSums.p, p->dIns.p, p->dOut.p);
    }
    FCHK(hipGetLastError());
    std::vector<FileOut> fo(nf);
    FCHK(hipMemcpyAsync(fo.data(), p->dOut.p, nf * sizeof(FileOut), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    std::vector<uint64_t> bases(2 * (size_t) nf + 2);
    uint64_t *sb = bases.data(), *rb = bases.data() + nf + 1;
    sb[0] = 0; rb[0] = 0;
    for (int i = 0; i < nf; i++) { sb[i + 1] = sb[i] + fo[i].kept; rb[i + 1] = rb[i] + fo[i].recs; }
    if (sb[nf] > outCap) return fail(-104, "sequence output needs %llu bytes, capacity %llu", (unsigned long long) sb[nf], (unsigned long long) outCap);
    if (rb[nf] > recCap) { recBase[nf] = rb[nf]; return fail(-104, "record table needs %llu entries, capacity %llu", (unsigned long long) rb[nf], (unsigned long long) recCap); }
    if ((r = p->dRecs.reserve(std::max<uint64_t>(rb[nf], 1)))) return r;
    FCHK(hipMemcpyAsync(p->dBases.p, bases.data(), bases.size() * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    if (chunks && lossy)
        k_fa_emit<true><<<dim3(chunks), dim3(THREADS), 0, p->stream>>>(files_dev, p->dFiles.p, p->dOwner.p, p->dSums.p, p->dIns.p, p->dBases.p,
                                                                       p->dBases.p + nf + 1, uppercaseDNA, seq_out_dev, p->dRecs.p, p->dOut.p, p->dShift.p);
    else if (chunks)
        k_fa_emit<false><<<dim3(chunks), dim3(THREADS), 0, p->stream>>>(files_dev, p->dFiles.p, p->dOwner.p, p->dSums.p, p->dIns.p, p->dBases.p,
                                                                        p->dBases.p + nf + 1, uppercaseDNA, seq_out_dev, p->dRecs.p, p->dOut.p, nullptr);
    FCHK(hipGetLastError());
    if (rb[nf]) FCHK(hipMemcpyAsync(records, p->dRecs.p, rb[nf] * sizeof(mbgc_fasta_record_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipMemcpyAsync(fo.data(), p->dOut.p, nf * sizeof(FileOut), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    for (int i = 0; i < nf; i++) {
        seqBase[i] = sb[i]; recBase[i] = rb[i];
        // a record's contig ends where the next one starts
        for (uint64_t k = rb[i]; k < rb[i + 1]; k++) {
            records[k].seqLen = (k + 1 < rb[i + 1] ? records[k + 1].seqOff : fo[i].kept) - records[k].seqOff;
        }
        // kseq status and KSEQ_DNA_LINE_LENGTH (kseq.h:251-265, MGMP.cpp:12-14)
        const bool haveLine = fo[i].minLine != ~0ull;
        const unsigned long long L = haveLine ? fo[i].minLine : 0;
        if (lossy) {                                                 // never -3 or -4; the longest line (kseq.h:301-312)
            status[i] = fo[i].firstNotGt ? MBGC_FASTA_EFASTQ : MBGC_FASTA_OK;
            dnaLineLen[i] = status[i] == MBGC_FASTA_OK ? fo[i].maxLine : 0;
            continue;
        }
        int st = MBGC_FASTA_OK;
        if (fo[i].firstNotGt) st = MBGC_FASTA_ENOTFASTA;
        else if (fo[i].emptyLine || (haveLine && fo[i].minLine != fo[i].maxLine) || (haveLine && fo[i].maxLast > L)) st = MBGC_FASTA_ELINES;
        status[i] = st;
        dnaLineLen[i] = st == MBGC_FASTA_OK ? L : 0;
    }
    seqBase[nf] = sb[nf]; recBase[nf] = rb[nf];
    return 0;
}

int mbgc_fasta_parse_batch_dev(mbgc_fasta_t *p, const uint8_t *files_dev, const uint64_t *fileOff, int nf, int uppercaseDNA,
                               uint8_t *seq_out_dev, uint64_t outCap, uint64_t *seqBase,
                               mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *recBase,
                               uint64_t *dnaLineLen, int *status) {
    return mbgc_fasta_parse_batch_dev2(p, files_dev, fileOff, nf, uppercaseDNA ? MBGC_FASTA_UPPERCASE : 0u, seq_out_dev, outCap, seqBase,
                                       records, recCap, recBase, dnaLineLen, status);
}

int mbgc_fasta_parse_host(mbgc_fasta_t *p, const uint8_t *file_host, uint64_t n, int uppercaseDNA, uint8_t *seq_out_host,
                          uint64_t *seqBytes, mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *nrec,
                          uint64_t *dnaLineLen, int *status) {
    return mbgc_fasta_parse_host2(p, file_host, n, uppercaseDNA ? MBGC_FASTA_UPPERCASE : 0u, seq_out_host, seqBytes, records, recCap, nrec,
                                  dnaLineLen, status);
}

int mbgc_fasta_parse_host2(mbgc_fasta_t *p, const uint8_t *file_host, uint64_t n, uint32_t flags, uint8_t *seq_out_host,
                           uint64_t *seqBytes, mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *nrec,
                           uint64_t *dnaLineLen, int *status) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    int r;
    p->hostParsedBytes = 0;
    if ((r = p->dHostIn.reserve(std::max<uint64_t>(n, 1))) || (r = p->dHostOut.reserve(std::max<uint64_t>(n, 1)))) return r;
    if (n) FCHK(hipMemcpy(p->dHostIn.p, file_host, n, hipMemcpyHostToDevice));
    const uint64_t off[2] = {0, n};
    uint64_t sb[2] = {0, 0}, rb[2] = {0, 0};
    *nrec = 0; *seqBytes = 0;
    if (n == 0) { *status = MBGC_FASTA_OK; *dnaLineLen = 0; return 0; }
    r = mbgc_fasta_parse_batch_dev2(p, p->dHostIn.p, off, 1, flags, p->dHostOut.p, n, sb, records, recCap, rb, dnaLineLen, status);
    if (r) { *nrec = rb[1]; return r; }
    *nrec = rb[1]; *seqBytes = sb[1];
    p->hostParsedBytes = sb[1];
    if (sb[1]) FCHK(hipMemcpy(seq_out_host, p->dHostOut.p, sb[1], hipMemcpyDeviceToHost));
    return 0;
}

int mbgc_fasta_probe_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const uint64_t *recOff, const uint64_t *recLen,
                         uint64_t nrec, int k, mbgc_fasta_probe_state_t *state_inout, mbgc_fasta_probe_result_t *result_out) {
    using namespace fa;
    const int32_t remaining0 = state_inout->probe_remaining, nonStd0 = state_inout->probe_non_std_count;
    if (remaining0 < 0 || remaining0 > MBGC_FASTA_PROBE_MAX_LEN || nonStd0 < 0 || nonStd0 > MBGC_FASTA_PROBE_MAX_LEN)
        return fail(-103, "probe: state (%d, %d) is none the rule can reach", remaining0, nonStd0);
    if (nrec > UINT32_MAX) return fail(-103, "probe: %llu records", (unsigned long long) nrec);
    // the records the probe still reaches, clipped (an empty one changes nothing: left out)
    std::vector<ProbeRec> tab;
    uint64_t left = (uint64_t) remaining0;
    for (uint64_t r = 0; r < nrec && left; r++) {
        if (recOff[r] > seqBytes || recLen[r] > seqBytes - recOff[r]) return fail(-103, "probe: record %llu lies outside the sequence bytes", (unsigned long long) r);
        const uint64_t len = std::min<uint64_t>(recLen[r], left);
        if (!len) continue;
        tab.push_back(ProbeRec{recOff[r], (uint32_t) len, (uint32_t) r});
        left -= len;
    }
    *result_out = mbgc_fasta_probe_result_t{0, 0, 0, *state_inout};
    if (tab.empty()) return 0;
    FCHK(hipSetDevice(p->device));
    const uint32_t n = (uint32_t) tab.size();
    int rc;
    if ((rc = p->dProbeRecs.reserve(n)) || (rc = p->dProbeCounts.reserve(n)) || (rc = p->dProbeOut.reserve(1))) return rc;
    FCHK(hipMemcpyAsync(p->dProbeRecs.p, tab.data(), n * sizeof(ProbeRec), hipMemcpyHostToDevice, p->stream));
    const uint32_t wavesPerBlock = THREADS / WAVE;
    k_fa_probe_count<<<dim3(std::min<uint32_t>((n + wavesPerBlock - 1) / wavesPerBlock, 1024)), dim3(THREADS), 0, p->stream>>>(seq_dev, p->dProbeRecs.p, n, p->dProbeCounts.p);
    k_fa_probe_walk<<<dim3(1), dim3(WAVE), 0, p->stream>>>(p->dProbeRecs.p, p->dProbeCounts.p, n, remaining0, nonStd0, k, p->dProbeOut.p);
    FCHK(hipGetLastError());
    ProbeOut out;
    FCHK(hipMemcpyAsync(&out, p->dProbeOut.p, sizeof out, hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    result_out->fired = out.fired; result_out->record = out.fired ? out.record : 0;
    result_out->state.probe_remaining = out.remaining; result_out->state.probe_non_std_count = out.nonStd;
    *state_inout = result_out->state;
    return 0;
}

int mbgc_fasta_probe_host(mbgc_fasta_t *p, const mbgc_fasta_record_t *records, uint64_t nrec, int k,
                          mbgc_fasta_probe_state_t *state_inout, mbgc_fasta_probe_result_t *result_out) {
    std::vector<uint64_t> off(nrec), len(nrec);
    for (uint64_t r = 0; r < nrec; r++) { off[r] = records[r].seqOff; len[r] = records[r].seqLen; }
    return mbgc_fasta_probe_dev(p, p->dHostOut.p, p->hostParsedBytes, off.data(), len.data(), nrec, k, state_inout, result_out);
}

int mbgc_fasta_split_buf_dev2(mbgc_fasta_t *p, const uint8_t *buf_dev, uint64_t start, uint64_t n, uint64_t scannedBefore, int isFileEnd,
                              uint64_t firstMin, uint64_t nextMin, uint32_t flags, int maxElems, uint64_t *ends, int *nElems) {
    using namespace fa;
    *nElems = 0;
    if (flags & ~(MBGC_FASTA_SPLIT_LINE_START | MBGC_FASTA_SPLIT_AT)) return fail(-103, "split: unknown flags %#x", flags);
    if (maxElems <= 0 || firstMin == 0 || nextMin == 0) return fail(-103, "split: maxElems and the minimal element sizes must be positive");
    if (start > n || scannedBefore > n) return fail(-103, "split: the window starts or was scanned behind its end");
    if (n == start) return 0;
    if (n > ((uint64_t) 1 << 40)) return fail(-103, "split: a window of %llu bytes", (unsigned long long) n);
    FCHK(hipSetDevice(p->device));
    const uint32_t ntiles = (uint32_t) ((n + CHUNK - 1) / CHUNK);
    if (ntiles > p->dTileFirst.cap) scannedBefore = 0;              // (the tile array is made anew: nothing of it is kept)
    if (flags != p->tileFlags) scannedBefore = 0;                   // (... or holds another rule's marks)
    p->tileFlags = flags;
    int r;
    if ((r = p->dTileFirst.reserve(ntiles)) || (r = p->dSplit.reserve((size_t) maxElems + 1))) return r;
    // the tiles that were whole at the last call stand; the pass starts at the first one that was not, or that lies before the
    // window's start (nothing reads those)
    const uint32_t tile0 = (uint32_t) (std::max(scannedBefore, start / CHUNK * CHUNK) / CHUNK);
    switch (flags) {
    case 0: launch_split<0>(p->stream, buf_dev, start, n, tile0, ntiles, isFileEnd, firstMin, nextMin, maxElems, p->dTileFirst.p, p->dSplit.p); break;
    case 1: launch_split<1>(p->stream, buf_dev, start, n, tile0, ntiles, isFileEnd, firstMin, nextMin, maxElems, p->dTileFirst.p, p->dSplit.p); break;
    case 2: launch_split<2>(p->stream, buf_dev, start, n, tile0, ntiles, isFileEnd, firstMin, nextMin, maxElems, p->dTileFirst.p, p->dSplit.p); break;
    default: launch_split<3>(p->stream, buf_dev, start, n, tile0, ntiles, isFileEnd, firstMin, nextMin, maxElems, p->dTileFirst.p, p->dSplit.p); break;
    }
    FCHK(hipGetLastError());
    // the count and the ends in one copy (a round's elements are a handful; a longer list takes a second one)
    const size_t FIRST = 256;
    uint64_t res[FIRST + 1];
    const size_t first = std::min<size_t>((size_t) maxElems, FIRST);
    FCHK(hipMemcpyAsync(res, p->dSplit.p, (first + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    const uint64_t ne = res[0];
    if (ne > (uint64_t) maxElems) return fail(-100, "split: %llu elements for a capacity of %d", (unsigned long long) ne, maxElems);
    memcpy(ends, res + 1, std::min<size_t>(ne, first) * sizeof(uint64_t));
    if (ne > first) {
        FCHK(hipMemcpyAsync(ends + first, p->dSplit.p + 1 + first, (ne - first) * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
    }
    *nElems = (int) ne;
    return 0;
}

int mbgc_fasta_split_buf_dev(mbgc_fasta_t *p, const uint8_t *buf_dev, uint64_t start, uint64_t n, uint64_t scannedBefore, int isFileEnd,
                             uint64_t firstMin, uint64_t nextMin, int maxElems, uint64_t *ends, int *nElems) {
    return mbgc_fasta_split_buf_dev2(p, buf_dev, start, n, scannedBefore, isFileEnd, firstMin, nextMin, 0, maxElems, ends, nElems);
}

int mbgc_fasta_split_dev(mbgc_fasta_t *p, const uint8_t *bytes_dev, uint64_t n, int isFileEnd, uint64_t firstMin, uint64_t nextMin,
                         int maxElems, uint64_t *ends, int *nElems) {
    return mbgc_fasta_split_buf_dev(p, bytes_dev, 0, n, 0, isFileEnd, firstMin, nextMin, maxElems, ends, nElems);
}

int mbgc_fasta_format_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const uint8_t *headers_dev, uint64_t headerBytes,
                          const mbgc_fasta_format_rec_t *recs, uint64_t nrec, uint8_t *text_dev, uint64_t textCap, uint64_t *textOff,
                          double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(FmtIn) == sizeof(mbgc_fasta_format_rec_t), "the table builder reads the ABI's records");
    if (kernelMs) *kernelMs = 0;
    if (nrec >= 0xffffffffull) return fail(-103, "format: %llu records in one call", (unsigned long long) nrec);
    for (uint64_t k = 0; k < nrec; k++) {
        const mbgc_fasta_format_rec_t &x = recs[k];
        if (x.seqOff > seqBytes || x.seqLen > seqBytes - x.seqOff || x.headerOff > headerBytes || x.headerLen > headerBytes - x.headerOff)
            return fail(-103, "format: record %llu lies outside the sequences or the headers", (unsigned long long) k);
    }
    std::vector<FmtRec> table;
    const uint64_t total = fmt_build_table((const FmtIn *) recs, nrec, table, textOff);
    if (total > textCap) return fail(-104, "text output needs %llu bytes, capacity %llu", (unsigned long long) total, (unsigned long long) textCap);
    if (total == 0) return 0;
    FCHK(hipSetDevice(p->device));
    const uint32_t mis = (uint32_t) ((uintptr_t) text_dev & (PER - 1));
    const uint64_t nt64 = (total + mis + CHUNK - 1) / CHUNK;
    if (nt64 >= 0xffffffffull) return fail(-103, "format: %llu bytes of text in one call", (unsigned long long) total);
    const uint32_t ntiles = (uint32_t) nt64;
    std::vector<uint32_t> owner;
    fmt_build_owner(table, nrec, mis, ntiles, owner);
    int rc;
    if ((rc = p->dFmtRecs.reserve(nrec + 1)) || (rc = p->dFmtOwner.reserve((size_t) ntiles + 1))) return rc;
    FCHK(hipMemcpyAsync(p->dFmtRecs.p, table.data(), (nrec + 1) * sizeof(FmtRec), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dFmtOwner.p, owner.data(), ((size_t) ntiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint32_t t0 = 0; t0 < ntiles; t0 += FMT_SLICE)
        k_fa_format<<<dim3(std::min(FMT_SLICE, ntiles - t0)), dim3(THREADS), 0, p->stream>>>(seq_dev, seqBytes, headers_dev, p->dFmtRecs.p, p->dFmtOwner.p,
                                                                                            t0, ntiles, mis, total, text_dev);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    return 0;
}

int mbgc_fasta_compare_dev(mbgc_fasta_t *p, const uint8_t *a_dev, uint64_t aBytes, const uint8_t *b_dev, uint64_t bBytes,
                           const mbgc_fasta_compare_piece_t *pieces, uint64_t npieces, uint64_t *firstDiff, uint32_t nslots, double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(CmpIn) == sizeof(mbgc_fasta_compare_piece_t), "the table builder reads the ABI's pieces");
    if (kernelMs) *kernelMs = 0;
    if (npieces >= 0xffffffffull) return fail(-103, "compare: %llu pieces in one call", (unsigned long long) npieces);
    for (uint64_t k = 0; k < npieces; k++) {
        const mbgc_fasta_compare_piece_t &x = pieces[k];
        if (x.aOff > aBytes || x.len > aBytes - x.aOff || x.bOff > bBytes || x.len > bBytes - x.bOff)
            return fail(-103, "compare: piece %llu lies outside the buffers", (unsigned long long) k);
        if (x.slot >= nslots) return fail(-103, "compare: piece %llu names slot %u of %u", (unsigned long long) k, x.slot, nslots);
    }
    std::vector<CmpPiece> table;
    const uint64_t total = cmp_build_table((const CmpIn *) pieces, npieces, (uint64_t) (uintptr_t) a_dev, table);
    const uint64_t nt64 = (total + CHUNK - 1) / CHUNK;
    if (nt64 >= 0xffffffffull) return fail(-103, "compare: %llu bytes in one call", (unsigned long long) total);
    if (total == 0 || nslots == 0) {
        for (uint32_t s = 0; s < nslots; s++) firstDiff[s] = UINT64_MAX;
        return 0;
    }
    FCHK(hipSetDevice(p->device));
    const uint32_t ntiles = (uint32_t) nt64;
    std::vector<uint32_t> owner;
    cmp_build_owner(table, ntiles, owner);
    int rc;
    if ((rc = p->dCmpPieces.reserve(table.size())) || (rc = p->dCmpOwner.reserve((size_t) ntiles + 1)) || (rc = p->dCmpOut.reserve(nslots))) return rc;
    FCHK(hipMemcpyAsync(p->dCmpPieces.p, table.data(), table.size() * sizeof(CmpPiece), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dCmpOwner.p, owner.data(), ((size_t) ntiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemsetAsync(p->dCmpOut.p, 0xff, (size_t) nslots * sizeof(unsigned long long), p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint32_t t0 = 0; t0 < ntiles; t0 += FMT_SLICE)
        k_fa_compare<<<dim3(std::min(FMT_SLICE, ntiles - t0)), dim3(THREADS), 0, p->stream>>>(a_dev, b_dev, p->dCmpPieces.p, p->dCmpOwner.p, t0, ntiles, total,
                                                                                             p->dCmpOut.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    std::vector<unsigned long long> out(nslots);                     // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(out.data(), p->dCmpOut.p, (size_t) nslots * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    for (uint32_t s = 0; s < nslots; s++) firstDiff[s] = out[s];
    return 0;
}

int mbgc_fasta_pack_dev(mbgc_fasta_t *p, const uint8_t *src_dev, uint64_t srcBytes, const mbgc_fasta_pack_piece_t *pieces, uint64_t n, uint32_t flags,
                        uint8_t *dst_dev, uint64_t dstCap, uint64_t *dstOff, double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(PackIn) == sizeof(mbgc_fasta_pack_piece_t), "the table builder reads the ABI's pieces");
    if (kernelMs) *kernelMs = 0;
    if (flags & ~(uint32_t) MBGC_FASTA_UPPERCASE) return fail(-103, "pack: unknown flags %#x", flags);
    if (n >= 0xffffffffull) return fail(-103, "pack: %llu pieces in one call", (unsigned long long) n);
    for (uint64_t k = 0; k < n; k++)
        if (pieces[k].srcOff > srcBytes || pieces[k].len > srcBytes - pieces[k].srcOff)
            return fail(-103, "pack: piece %llu lies outside the source", (unsigned long long) k);
    const uintptr_t s0 = (uintptr_t) src_dev, d0 = (uintptr_t) dst_dev;
    if (srcBytes && dstCap && s0 < d0 + dstCap && d0 < s0 + srcBytes) return fail(-103, "pack: the source and the destination overlap");
    std::vector<PackPiece> table;
    const uint64_t total = pack_build_table((const PackIn *) pieces, n, table, dstOff);
    if (total > dstCap) return fail(-104, "packed output needs %llu bytes, capacity %llu", (unsigned long long) total, (unsigned long long) dstCap);
    if (total == 0) return 0;
    FCHK(hipSetDevice(p->device));
    const uint32_t mis = (uint32_t) (d0 & (uintptr_t) (PER - 1));
    const uint64_t nt64 = (total + mis + CHUNK - 1) / CHUNK;
    if (nt64 >= 0xffffffffull) return fail(-103, "pack: %llu bytes in one call", (unsigned long long) total);
    const uint32_t ntiles = (uint32_t) nt64;
    std::vector<uint32_t> owner;
    pack_build_owner(table, mis, ntiles, owner);
    int rc;
    if ((rc = p->dPackPieces.reserve(table.size())) || (rc = p->dPackOwner.reserve((size_t) ntiles + 1))) return rc;
    FCHK(hipMemcpyAsync(p->dPackPieces.p, table.data(), table.size() * sizeof(PackPiece), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dPackOwner.p, owner.data(), ((size_t) ntiles + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint32_t t0 = 0; t0 < ntiles; t0 += FMT_SLICE)
        k_fa_pack<<<dim3(std::min(FMT_SLICE, ntiles - t0)), dim3(THREADS), 0, p->stream>>>(src_dev, p->dPackPieces.p, p->dPackOwner.p, t0, ntiles, mis, total,
                                                                                          (flags & MBGC_FASTA_UPPERCASE) ? 1 : 0, dst_dev);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    return 0;
}

int mbgc_fasta_match_headers_dev(mbgc_fasta_t *p, const uint8_t *headers_dev, uint64_t headerBytes, const uint64_t *hdrOff, const uint64_t *hdrLen,
                                 uint64_t nrec, const uint8_t *patterns, const uint64_t *patOff, uint64_t npat, uint32_t *chosen, double *kernelMs) {
    using namespace fa;
    if (kernelMs) *kernelMs = 0;
    if (nrec >= 0xffffffffull || npat >= 0x7fffffffull) return fail(-103, "match: %llu records, %llu patterns in one call", (unsigned long long) nrec, (unsigned long long) npat);
    for (uint64_t r = 0; r < nrec; r++)
        if (hdrOff[r] > headerBytes || hdrLen[r] > headerBytes - hdrOff[r]) return fail(-103, "match: header %llu lies outside the headers", (unsigned long long) r);
    for (uint64_t k = 0; k < npat; k++) {
        if (patOff[k + 1] <= patOff[k]) return fail(-103, "match: pattern %llu is empty", (unsigned long long) k);
        if (memchr(patterns + patOff[k], '\n', patOff[k + 1] - patOff[k])) return fail(-103, "match: pattern %llu holds a line feed", (unsigned long long) k);
    }
    const size_t words = (size_t) ((nrec + 31) / 32);
    if (nrec == 0) return 0;
    if (npat == 0) { memset(chosen, 0, words * sizeof(uint32_t)); return 0; }
    SelTable T;
    sel_build_table(patterns, patOff, npat, T);
    FCHK(hipSetDevice(p->device));
    const uint64_t patBytes = patOff[npat];                          // (the table's offsets count from the caller's `patterns`)
    int rc;
    if ((rc = p->dSelRecs.reserve(2 * nrec)) || (rc = p->dSelSlots.reserve(T.slots.size())) || (rc = p->dSelPats.reserve(T.pats.size())) ||
        (rc = p->dSelBytes.reserve(patBytes)) || (rc = p->dSelChosen.reserve(words))) return rc;
    FCHK(hipMemcpyAsync(p->dSelRecs.p, hdrOff, nrec * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dSelRecs.p + nrec, hdrLen, nrec * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dSelSlots.p, T.slots.data(), T.slots.size() * sizeof(SelSlot), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dSelPats.p, T.pats.data(), T.pats.size() * sizeof(SelPat), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dSelBytes.p, patterns, patBytes, hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemsetAsync(p->dSelChosen.p, 0, words * sizeof(uint32_t), p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    k_fa_match_headers<<<dim3((uint32_t) std::min<uint64_t>(nrec, 1u << 16)), dim3(WAVE), 0, p->stream>>>(headers_dev, p->dSelRecs.p, p->dSelRecs.p + nrec, nrec, T.m,
                                                                                                        p->dSelSlots.p, T.bits, p->dSelPats.p, p->dSelBytes.p, p->dSelChosen.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    std::vector<uint32_t> out(words);                                // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(out.data(), p->dSelChosen.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    memcpy(chosen, out.data(), words * sizeof(uint32_t));
    return 0;
}

int mbgc_fasta_find_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                        const uint8_t *patterns_host, const uint64_t *patOff, uint64_t npat, uint32_t maxMismatches,
                        mbgc_fasta_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs) {
    using namespace fa;
    if (kernelMs) *kernelMs = 0;
    const uint32_t K = maxMismatches;
    if (K > FIND_MAX_K) return fail(-103, "find: %u mismatches (at most %u)", K, FIND_MAX_K);
    if (n >= 0xffffffffull || npat >= 0xffffffffull / (FIND_MAX_K + 1)) return fail(-103, "find: %llu records, %llu patterns in one call", (unsigned long long) n, (unsigned long long) npat);
    for (uint64_t q = 0; q < npat; q++) {
        if (patOff[q + 1] < patOff[q]) return fail(-103, "find: pattern %llu ends in front of its start", (unsigned long long) q);
        const uint64_t len = patOff[q + 1] - patOff[q];
        if (len < (uint64_t) FIND_GRAM * (K + 1)) return fail(-103, "find: pattern %llu has %llu bytes, %u mismatches need at least %u", (unsigned long long) q, (unsigned long long) len, K, FIND_GRAM * (K + 1));
        if (len > FIND_MAX_LEN) return fail(-103, "find: pattern %llu has %llu bytes (at most %u)", (unsigned long long) q, (unsigned long long) len, FIND_MAX_LEN);
        for (uint64_t i = patOff[q]; i < patOff[q + 1]; i++)
            if ((uint8_t) ((patterns_host[i] | 0x20) - 'a') >= 26) return fail(-103, "find: pattern %llu holds a byte that is no letter (0x%02x at %llu)", (unsigned long long) q, patterns_host[i], (unsigned long long) (i - patOff[q]));
    }
    FindTable T;                                                     // (made only when there is something to search with and in)
    if (n && npat) find_build_table(patterns_host, patOff, npat, K, T);
    uint64_t ntiles = 0;
    FTRY(scan_prepare(p, "find", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return npat ? find_positions(recs[r].len, T.shortest) : 0; }, ntiles));
    if (ntiles == 0) { *nHits = 0; return 0; }                       // (no record, no pattern, or no record as long as the shortest pattern)
    int rc;
    if ((rc = p->dFindSlots.reserve(T.slots.size())) || (rc = p->dFindSeeds.reserve(T.seeds.size())) ||
        (rc = p->dFindPats.reserve(T.pats.size())) || (rc = p->dFindBytes.reserve(T.bytes.size())) || (rc = p->dFindHits.reserve(std::max<uint64_t>(hitCap, 1))) ||
        (rc = p->dFindCursor.reserve(1))) return rc;
    FCHK(hipMemcpyAsync(p->dFindSlots.p, T.slots.data(), T.slots.size() * sizeof(FindSlot), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dFindSeeds.p, T.seeds.data(), T.seeds.size() * sizeof(FindSeed), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dFindPats.p, T.pats.data(), T.pats.size() * sizeof(FindPat), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dFindBytes.p, T.bytes.data(), T.bytes.size(), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemsetAsync(p->dFindCursor.p, 0, sizeof(unsigned long long), p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    // one launch whatever n is: the blocks stride over the tiles, four blocks of four waves to a CU
    const dim3 grid((uint32_t) std::min<uint64_t>(ntiles, 1024));
    if (T.bits <= FIND_LDS_BITS)
        k_fa_find<true><<<grid, dim3(FIND_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScanTiles.p, (uint32_t) n, ntiles, p->dFindSlots.p, T.bits, p->dFindSeeds.p,
                                                                    p->dFindPats.p, p->dFindBytes.p, K, p->dFindHits.p, hitCap, p->dFindCursor.p);
    else
        k_fa_find<false><<<grid, dim3(FIND_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScanTiles.p, (uint32_t) n, ntiles, p->dFindSlots.p, T.bits, p->dFindSeeds.p,
                                                                     p->dFindPats.p, p->dFindBytes.p, K, p->dFindHits.p, hitCap, p->dFindCursor.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    unsigned long long count = 0;
    FCHK(hipMemcpyAsync(&count, p->dFindCursor.p, sizeof count, hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    *nHits = count;
    if (count > hitCap) return fail(-104, "find: %llu hits, the buffer holds %llu", count, (unsigned long long) hitCap);
    if (count == 0) return 0;
    std::vector<mbgc_fasta_hit_t> out(count);                        // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(out.data(), p->dFindHits.p, count * sizeof(mbgc_fasta_hit_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    std::sort(out.begin(), out.end(), [](const mbgc_fasta_hit_t &a, const mbgc_fasta_hit_t &b) {
        if (a.rec != b.rec) return a.rec < b.rec;
        if (a.pos != b.pos) return a.pos < b.pos;
        return a.pattern < b.pattern;
    });
    memcpy(hits_host, out.data(), count * sizeof(mbgc_fasta_hit_t));
    return 0;
}

int mbgc_fasta_find_iupac_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                              const uint8_t *patterns_host, const uint64_t *patOff, uint64_t npat, uint32_t maxMismatches,
                              mbgc_fasta_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs) {
    using namespace fa;
    if (kernelMs) *kernelMs = 0;
    const uint32_t K = maxMismatches;
    if (K > FIND_MAX_K) return fail(-103, "find-iupac: %u mismatches (at most %u)", K, FIND_MAX_K);
    // (every row is a 32-bit index: a pattern has at most (FIND_MAX_K + 1) IUPAC_MAX_EXPAND of them)
    if (n >= 0xffffffffull || npat >= 0xffffffffull / ((FIND_MAX_K + 1) * IUPAC_MAX_EXPAND))
        return fail(-103, "find-iupac: %llu records, %llu patterns in one call", (unsigned long long) n, (unsigned long long) npat);
    for (uint64_t q = 0; q < npat; q++) {
        if (patOff[q + 1] < patOff[q]) return fail(-103, "find-iupac: pattern %llu ends in front of its start", (unsigned long long) q);
        const uint64_t len = patOff[q + 1] - patOff[q];
        if (len < (uint64_t) IUPAC_GRAM * (K + 1)) return fail(-103, "find-iupac: pattern %llu has %llu letters, %u mismatches need at least %u", (unsigned long long) q, (unsigned long long) len, K, IUPAC_GRAM * (K + 1));
        if (len > FIND_MAX_LEN) return fail(-103, "find-iupac: pattern %llu has %llu letters (at most %u)", (unsigned long long) q, (unsigned long long) len, FIND_MAX_LEN);
        for (uint64_t i = patOff[q]; i < patOff[q + 1]; i++)
            if (!iupac_mask(patterns_host[i])) return fail(-103, "find-iupac: pattern %llu holds a byte that is no IUPAC letter (0x%02x at %llu)", (unsigned long long) q, patterns_host[i], (unsigned long long) (i - patOff[q]));
    }
    // (the table is made whatever the records are: a pattern that cannot be searched is refused, not passed over)
    IupacTable T;
    uint64_t badPat = 0;
    uint32_t badSeg = 0, badGrams = 0;
    if (npat && !iupac_build_table(patterns_host, patOff, npat, K, T, badPat, badSeg, badGrams))
        return fail(-103, "find-iupac: pattern %llu, segment %u (letters %u to %u): its best window of %u letters stands for %u sequences (at most %u): too many degenerate letters in a row",
                    (unsigned long long) badPat, badSeg, badSeg * (uint32_t) ((patOff[badPat + 1] - patOff[badPat]) / (K + 1)) + 1,
                    (badSeg + 1) * (uint32_t) ((patOff[badPat + 1] - patOff[badPat]) / (K + 1)), IUPAC_GRAM, badGrams, IUPAC_MAX_EXPAND);
    uint64_t ntiles = 0;
    FTRY(scan_prepare(p, "find-iupac", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return npat ? find_positions(recs[r].len, T.shortest) : 0; }, ntiles));
    p->iupacRows = T.rows.size(); p->iupacWalked = 0;
    if (ntiles == 0) { *nHits = 0; return 0; }                       // (no record, no pattern, or no record as long as the shortest pattern)
    int rc;
    if ((rc = p->dIupacBitmap.reserve(T.bitmap.size())) || (rc = p->dIupacStart.reserve(T.gramStart.size())) || (rc = p->dIupacRows.reserve(T.rows.size())) ||
        (rc = p->dIupacPats.reserve(T.pats.size())) || (rc = p->dIupacMasks.reserve(T.masks.size())) || (rc = p->dFindHits.reserve(std::max<uint64_t>(hitCap, 1))) ||
        (rc = p->dIupacStats.reserve(IUPAC_WALKED + 1))) return rc;
    FCHK(hipMemcpyAsync(p->dIupacBitmap.p, T.bitmap.data(), T.bitmap.size() * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dIupacStart.p, T.gramStart.data(), T.gramStart.size() * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dIupacRows.p, T.rows.data(), T.rows.size() * sizeof(IupacRow), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dIupacPats.p, T.pats.data(), T.pats.size() * sizeof(IupacPat), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dIupacMasks.p, T.masks.data(), T.masks.size(), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemsetAsync(p->dIupacStats.p, 0, (IUPAC_WALKED + 1) * sizeof(unsigned long long), p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    // one launch whatever n is, as k_fa_find's: the blocks stride over the tiles
    k_fa_find_iupac<<<dim3((uint32_t) std::min<uint64_t>(ntiles, 1024)), dim3(FIND_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScanTiles.p, (uint32_t) n, ntiles,
        p->dIupacBitmap.p, p->dIupacStart.p, p->dIupacRows.p, p->dIupacPats.p, p->dIupacMasks.p, K, p->dFindHits.p, hitCap, p->dIupacStats.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    unsigned long long stats[IUPAC_WALKED + 1] = {0};
    FCHK(hipMemcpyAsync(stats, p->dIupacStats.p, sizeof stats, hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    const unsigned long long count = stats[0];
    p->iupacWalked = stats[IUPAC_WALKED];
    *nHits = count;
    if (count > hitCap) return fail(-104, "find-iupac: %llu hits, the buffer holds %llu", count, (unsigned long long) hitCap);
    if (count == 0) return 0;
    std::vector<mbgc_fasta_hit_t> out(count);                        // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(out.data(), p->dFindHits.p, count * sizeof(mbgc_fasta_hit_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    std::sort(out.begin(), out.end(), [](const mbgc_fasta_hit_t &a, const mbgc_fasta_hit_t &b) {
        if (a.rec != b.rec) return a.rec < b.rec;
        if (a.pos != b.pos) return a.pos < b.pos;
        return a.pattern < b.pattern;
    });
    memcpy(hits_host, out.data(), count * sizeof(mbgc_fasta_hit_t));
    return 0;
}

void mbgc_fasta_find_iupac_last(const mbgc_fasta_t *p, uint64_t *tableRows, uint64_t *rowsWalked) {
    if (tableRows) *tableRows = p->iupacRows;
    if (rowsWalked) *rowsWalked = p->iupacWalked;
}

int mbgc_fasta_stats_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint32_t flags,
                         uint64_t minRunN, uint64_t minRunLower, mbgc_fasta_counts_t *counts_host, mbgc_fasta_run_t *runs_host, uint64_t runCap,
                         uint64_t *nRuns, double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(mbgc_fasta_counts_t) == 8 * sizeof(uint64_t) && sizeof(StatsEdge) == 16, "a record's row is eight words; an edge is sixteen bytes");
    const bool counting = (flags & MBGC_FASTA_STATS_COUNTS) != 0;
    const uint32_t want = (flags & MBGC_FASTA_STATS_NRUNS ? STATS_CLS_N : 0u) | (flags & MBGC_FASTA_STATS_LOWER ? STATS_CLS_LOWER : 0u);
    uint64_t ntiles = 0;                                             // (nothing asked: no position is looked at)
    FTRY(scan_prepare(p, "stats", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return counting || want ? recs[r].len : 0; }, ntiles));
    if (kernelMs) *kernelMs = 0;
    p->statsEdges = p->statsReruns = 0;
    if (ntiles == 0) {                                               // (no byte to look at, or nothing asked)
        if (counting && n) memset(counts_host, 0, n * sizeof(mbgc_fasta_counts_t));
        *nRuns = 0;
        return 0;
    }
    int rc;
    if ((rc = p->dStatsCounts.reserve(8 * n)) || (rc = p->dStatsCursor.reserve(1)) ||
        (rc = p->dStatsEdges.reserve(std::max<uint64_t>(STATS_EDGES_FIRST, p->statsEdgeCap)))) return rc;
    // the edge buffer is this call's own: when the cursor passed it, it grows to the cursor's count and the kernel runs again
    uint64_t edgeCap = std::max<uint64_t>(STATS_EDGES_FIRST, p->statsEdgeCap);
    unsigned long long count = 0;
    for (;;) {
        if (counting) FCHK(hipMemsetAsync(p->dStatsCounts.p, 0, 8 * n * sizeof(unsigned long long), p->stream));
        FCHK(hipMemsetAsync(p->dStatsCursor.p, 0, sizeof(unsigned long long), p->stream));
        FTRY(p->timer.start(p->stream, kernelMs != nullptr));
        // one launch whatever n is: the blocks stride over the tiles, eight blocks of four waves to a CU (a wave has one load in flight)
        k_fa_stats<<<dim3((uint32_t) std::min<uint64_t>(ntiles, 2048)), dim3(STATS_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScanTiles.p, (uint32_t) n, ntiles,
                                                                                                              counting, want, p->dStatsCounts.p, p->dStatsEdges.p, edgeCap, p->dStatsCursor.p);
        FCHK(hipGetLastError());
        FTRY(p->timer.stop(p->stream));
        FCHK(hipMemcpyAsync(&count, p->dStatsCursor.p, sizeof count, hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
        FTRY(p->timer.read(kernelMs));
        if (count <= edgeCap) break;
        if ((rc = p->dStatsEdges.reserve(count))) return rc;
        edgeCap = p->statsEdgeCap = count;
        p->statsReruns++;
    }
    p->statsEdges = count;
    // the edges of a (record, class) sorted by position: its starts, then its ends — the i-th start pairs with the i-th end
    std::vector<StatsEdge> e(count);
    if (count) FCHK(hipMemcpyAsync(e.data(), p->dStatsEdges.p, count * sizeof(StatsEdge), hipMemcpyDeviceToHost, p->stream));
    std::vector<mbgc_fasta_counts_t> rows(counting ? n : 0);         // (the caller's arrays stay as they are unless the call gets this far)
    if (counting) FCHK(hipMemcpyAsync(rows.data(), p->dStatsCounts.p, n * sizeof(mbgc_fasta_counts_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    std::sort(e.begin(), e.end(), [](const StatsEdge &a, const StatsEdge &b) {
        if (a.rec != b.rec) return a.rec < b.rec;
        if ((a.kind & 1) != (b.kind & 1)) return (a.kind & 1) < (b.kind & 1);
        if (a.kind != b.kind) return a.kind < b.kind;
        return a.pos < b.pos;
    });
    std::vector<mbgc_fasta_run_t> out;
    const uint64_t least[2] = {std::max<uint64_t>(minRunN, 1), std::max<uint64_t>(minRunLower, 1)};
    for (size_t at = 0; at < e.size();) {
        size_t ends = at, next;
        while (ends < e.size() && e[ends].rec == e[at].rec && e[ends].kind == e[at].kind) ends++;
        for (next = ends; next < e.size() && e[next].rec == e[at].rec && e[next].kind == (e[at].kind | 2u); next++) {}
        if ((e[at].kind & 2u) || next - ends != ends - at) return fail(-105, "stats: internal: edges do not pair (record %u, class %u)", e[at].rec, e[at].kind & 1u);
        for (size_t i = 0; i < ends - at; i++) {
            if (e[ends + i].pos < e[at + i].pos) return fail(-105, "stats: internal: edges do not pair (record %u, class %u)", e[at].rec, e[at].kind & 1u);
            const uint64_t len = e[ends + i].pos - e[at + i].pos + 1;
            if (len >= least[e[at].kind & 1u]) out.push_back(mbgc_fasta_run_t{e[at + i].pos, len, e[at].rec, e[at].kind & 1u});
        }
        at = next;
    }
    if (counting) memcpy(counts_host, rows.data(), n * sizeof(mbgc_fasta_counts_t));
    *nRuns = out.size();
    if (out.size() > runCap) return fail(-104, "stats: %zu runs, the buffer holds %llu", out.size(), (unsigned long long) runCap);
    if (!out.empty()) memcpy(runs_host, out.data(), out.size() * sizeof(mbgc_fasta_run_t));
    return 0;
}

void mbgc_fasta_stats_last(const mbgc_fasta_t *p, uint64_t *edges, uint64_t *reruns) {
    if (edges) *edges = p->statsEdges;
    if (reruns) *reruns = p->statsReruns;
}

const uint8_t *mbgc_fasta_dups_comp_table(void) {
    static uint8_t table[256];
    static std::once_flag once;
    std::call_once(once, [] { for (uint32_t b = 0; b < 256; b++) table[b] = fa::dups_comp((uint8_t) b); });
    return table;
}

int mbgc_fasta_dups_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint32_t flags,
                        mbgc_fasta_dup_t *out_host, uint64_t *nClasses, double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(mbgc_fasta_dup_t) == 8 && sizeof(DupsPair) == 16, "a record's answer is two words; a pair is four");
    static_assert(MBGC_FASTA_DUPS_FORWARD_ONLY == DUPS_FORWARD_ONLY && MBGC_FASTA_DUPS_EXACT_CASE == DUPS_EXACT_CASE && MBGC_FASTA_DUPS_WEAK_HASH == DUPS_WEAK_HASH, "the flags");
    // an unknown flag is reported in front of a record outside the buffer, and behind too many records (scan_prepare reports those two)
    const bool unknownFlags = (flags & ~(DUPS_FORWARD_ONLY | DUPS_EXACT_CASE | DUPS_WEAK_HASH)) != 0;
    if (unknownFlags && n < 0xffffffffull) return fail(-103, "dups: unknown flags %#x", flags);
    // ---- the fingerprints: one pass over the tiles of every record with a byte
    uint64_t ntiles = 0;
    FTRY(scan_prepare(p, "dups", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return recs[r].len; }, ntiles));
    if (kernelMs) *kernelMs = 0;
    p->dupBuckets = p->dupVerified = p->dupRefuted = 0;
    p->dupVerifyMs = 0;
    *nClasses = 0;
    if (n == 0) return 0;
    const bool forwardOnly = (flags & DUPS_FORWARD_ONLY) != 0;
    const uint32_t exactCase = (flags & DUPS_EXACT_CASE) != 0;
    std::vector<unsigned long long> rows(8 * n, 0);
    if (ntiles) {
        int rc;
        if ((rc = p->dDupRows.reserve(8 * n)) || (rc = p->dDupPairs.reserve(n)) || (rc = p->dDupRefuted.reserve(n))) return rc;
        FCHK(hipMemsetAsync(p->dDupRows.p, 0, 8 * n * sizeof(unsigned long long), p->stream));
        FTRY(p->timer.start(p->stream));
        // one launch whatever n is: the blocks stride over the tiles, as k_fa_stats's do
        k_fa_dups<<<dim3((uint32_t) std::min<uint64_t>(ntiles, 2048)), dim3(DUPS_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScanTiles.p, (uint32_t) n, ntiles,
                                                                                                            exactCase, p->dDupRows.p);
        FCHK(hipGetLastError());
        FTRY(p->timer.stop(p->stream));
        FCHK(hipMemcpyAsync(rows.data(), p->dDupRows.p, 8 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
        FTRY(p->timer.read(kernelMs));
    }
    typedef std::array<uint32_t, 4> Print;
    std::vector<Print> fw(n), rv(n), canon(n);
    for (uint64_t r = 0; r < n; r++) {
        DupsPrint f, b;
        dups_finish(&rows[8 * r], recs[r].len, f, b);
        for (int i = 0; i < 4; i++) { fw[r][i] = f.v[i]; rv[r][i] = b.v[i]; }
        if (flags & DUPS_WEAK_HASH) { fw[r] = Print{0, 0, 0, fw[r][3] & 15u}; rv[r] = Print{0, 0, 0, rv[r][3] & 15u}; }     // (a switch of the tests: the exactness step on ordinary inputs)
        canon[r] = forwardOnly ? fw[r] : std::min(fw[r], rv[r]);
    }
    // ---- the buckets: equal (length, canonical fingerprint), the members in index order. n counts records: a sort on the host
    std::vector<uint32_t> order(n);
    for (uint64_t r = 0; r < n; r++) order[r] = (uint32_t) r;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (recs[a].len != recs[b].len) return recs[a].len < recs[b].len;
        if (canon[a] != canon[b]) return canon[a] < canon[b];
        return a < b;
    });
    // ---- the exactness step. A bucket's first member is its first representative. Every other member is held against the bucket's
    // representatives one after the other, forward first, then as the reverse complement, a comparison the fingerprints exclude being
    // passed over; all members' next comparisons are one launch (a round). A member that no representative equals becomes one — but
    // only as the LOWEST member of its bucket that is still open, so that a representative is the lowest index of its class; a higher
    // one waits for the round after. The strand is the comparison's that held: forward is always tried first, so a record that equals
    // its representative both ways gets 0.
    struct Open { uint32_t rec, bucket, cand, phase; };
    std::vector<std::vector<uint32_t>> reps;
    std::vector<Open> open, still;
    std::vector<mbgc_fasta_dup_t> out(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t r = order[i];
        if (i == 0 || recs[r].len != recs[order[i - 1]].len || canon[r] != canon[order[i - 1]]) { reps.push_back({r}); out[r] = mbgc_fasta_dup_t{r, 0}; }
        else open.push_back(Open{r, (uint32_t) (reps.size() - 1), 0, 0});
    }
    p->dupBuckets = reps.size();
    std::vector<DupsPair> pairs;
    std::vector<size_t> asked;                                       // pair k is open[asked[k]]'s
    std::vector<uint32_t> verdict;
    std::vector<char> lowerOpen(reps.size());
    while (!open.empty()) {
        pairs.clear(); asked.clear();
        std::fill(lowerOpen.begin(), lowerOpen.end(), 0);
        for (size_t k = 0; k < open.size(); k++) {                   // (a bucket's members: in index order)
            Open &m = open[k];
            std::vector<uint32_t> &R = reps[m.bucket];
            while (m.cand < R.size()) {                              // the next comparison the fingerprints do not exclude
                if (m.phase == 0) { if (fw[m.rec] == fw[R[m.cand]]) break; m.phase = 1; }
                if (!forwardOnly && fw[m.rec] == rv[R[m.cand]]) break;
                m.phase = 0; m.cand++;
            }
            if (m.cand == R.size()) {
                if (!lowerOpen[m.bucket]) { R.push_back(m.rec); out[m.rec] = mbgc_fasta_dup_t{m.rec, 0}; m.rec = 0xffffffffu; }     // (closed: a representative)
                else lowerOpen[m.bucket] = 1;
                continue;
            }
            lowerOpen[m.bucket] = 1;
            if (recs[m.rec].len == 0) { out[m.rec] = mbgc_fasta_dup_t{R[m.cand], 0}; m.rec = 0xffffffffu; continue; }            // (no byte to compare)
            pairs.push_back(DupsPair{m.rec, R[m.cand], m.phase, 0});
            asked.push_back(k);
        }
        if (!pairs.empty()) {
            verdict.assign(pairs.size(), 0);
            FCHK(hipMemcpyAsync(p->dDupPairs.p, pairs.data(), pairs.size() * sizeof(DupsPair), hipMemcpyHostToDevice, p->stream));
            FCHK(hipMemsetAsync(p->dDupRefuted.p, 0, pairs.size() * sizeof(uint32_t), p->stream));
            FTRY(p->timer.start(p->stream));
            k_fa_dups_verify<<<dim3((uint32_t) std::min<size_t>(pairs.size(), 4096)), dim3(DUPS_THREADS), 0, p->stream>>>(seq_dev, p->dScanRecs.p, p->dDupPairs.p, (uint32_t) pairs.size(),
                                                                                                                          exactCase, p->dDupRefuted.p);
            FCHK(hipGetLastError());
            FTRY(p->timer.stop(p->stream));
            FCHK(hipMemcpyAsync(verdict.data(), p->dDupRefuted.p, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
            FCHK(hipStreamSynchronize(p->stream));
            double ms = 0;
            FTRY(p->timer.read(&ms));
            p->dupVerifyMs += ms;
            p->dupVerified += pairs.size();
            for (size_t k = 0; k < pairs.size(); k++) {
                Open &m = open[asked[k]];
                if (!verdict[k]) { out[m.rec] = mbgc_fasta_dup_t{pairs[k].rep, pairs[k].strand}; m.rec = 0xffffffffu; continue; }
                p->dupRefuted++;
                if (m.phase == 0) m.phase = 1; else { m.phase = 0; m.cand++; }
            }
        }
        still.clear();
        for (const Open &m : open) if (m.rec != 0xffffffffu) still.push_back(m);
        open.swap(still);
    }
    for (const std::vector<uint32_t> &R : reps) *nClasses += R.size();
    memcpy(out_host, out.data(), n * sizeof(mbgc_fasta_dup_t));
    return 0;
}

void mbgc_fasta_dups_last(const mbgc_fasta_t *p, uint64_t *buckets, uint64_t *verified, uint64_t *refuted, double *verifyMs) {
    if (buckets) *buckets = p->dupBuckets;
    if (verified) *verified = p->dupVerified;
    if (refuted) *refuted = p->dupRefuted;
    if (verifyMs) *verifyMs = p->dupVerifyMs;
}

int mbgc_fasta_sketch_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, const uint32_t *group_host, uint32_t ngroups,
                          uint32_t k, uint64_t maxHash, uint64_t *hashes_host, uint64_t cap, uint64_t *groupStart_host, uint64_t *kmers_host, uint64_t *total, double *kernelMs) {
    using namespace fa;
    if (k < 1 || k > 32) return fail(-103, "sketch: k = %u (1 to 32)", k);
    // the faults are reported in record order, a record outside the buffer in front of its own group: a group is looked at only in
    // front of the first such record, which scan_prepare reports (as it does too many records, in front of both)
    const uint64_t inside = n < 0xffffffffull ? first_outside(recs, n, seqBytes) : 0;
    for (uint64_t r = 0; r < inside; r++)
        if (group_host[r] >= ngroups) return fail(-103, "sketch: record %llu names group %u of %u", (unsigned long long) r, group_host[r], ngroups);
    uint64_t ntiles = 0;
    FTRY(scan_prepare(p, "sketch", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return sketch_positions(recs[r].len, k); }, ntiles));
    if (kernelMs) *kernelMs = 0;
    p->sketchRows = p->sketchReruns = 0;
    p->sketchSortMs = 0;
    *total = 0;
    for (uint32_t g = 0; g <= ngroups; g++) groupStart_host[g] = 0;
    for (uint32_t g = 0; g < ngroups; g++) kmers_host[g] = 0;
    if (ntiles == 0) return 0;                                       // (no record holds a k-mer)
    int rc;
    if ((rc = p->dSkGroups.reserve(n)) || (rc = p->dSkKmers.reserve(ngroups)) || (rc = p->dSkStart.reserve(ngroups)) || (rc = p->dSkWords.reserve(2))) return rc;
    FCHK(hipMemcpyAsync(p->dSkGroups.p, group_host, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    // the row buffer is this call's own: when the cursor passed it, it grows to the cursor's count and the kernel runs again
    uint64_t rowCap = std::max<uint64_t>(SKETCH_ROWS_FIRST, p->sketchRowCap);
    unsigned long long count = 0;
    for (;;) {
        if ((rc = p->dSkHash.reserve(rowCap)) || (rc = p->dSkGroup.reserve(rowCap))) return rc;
        FCHK(hipMemsetAsync(p->dSkKmers.p, 0, ngroups * sizeof(unsigned long long), p->stream));
        FCHK(hipMemsetAsync(p->dSkWords.p, 0, 2 * sizeof(unsigned long long), p->stream));
        FTRY(p->timer.start(p->stream));
        // one launch whatever n is: the blocks stride over the tiles, eight blocks of four waves to a CU
        k_fa_sketch<<<dim3((uint32_t) std::min<uint64_t>(ntiles, 2048)), dim3(SKETCH_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dSkGroups.p, p->dScanTiles.p, (uint32_t) n,
                                                                                                                 ntiles, k, maxHash, p->dSkKmers.p, p->dSkHash.p, p->dSkGroup.p, rowCap, p->dSkWords.p);
        FCHK(hipGetLastError());
        FTRY(p->timer.stop(p->stream));
        FCHK(hipMemcpyAsync(&count, p->dSkWords.p, sizeof count, hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
        FTRY(p->timer.read(kernelMs));
        if (count <= rowCap) break;
        if (count >= 0xffffffffull) return fail(-103, "sketch: %llu rows in one call (a larger scale, or fewer records)", count);
        rowCap = p->sketchRowCap = count;
        p->sketchReruns++;
    }
    p->sketchRows = count;
    std::vector<unsigned long long> kmers(ngroups), starts(ngroups, ~0ull);
    FCHK(hipMemcpyAsync(kmers.data(), p->dSkKmers.p, ngroups * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    unsigned long long distinct = 0;
    if (count) {
        // a stable sort by hash, then a stable sort by group: (group, hash) order; the first row of every (group, hash) is flagged, the
        // flags' exclusive sum is the row's place among the distinct ones
        uint32_t gbits = 1;
        while (gbits < 32 && ((uint64_t) 1 << gbits) < ngroups) gbits++;
        if ((rc = p->dSkHash2.reserve(count)) || (rc = p->dSkGroup2.reserve(count)) || (rc = p->dSkFlag.reserve(count)) || (rc = p->dSkPos.reserve(count))) return rc;
        size_t t1 = 0, t2 = 0, t3 = 0;
        FCHK(rocprim::radix_sort_pairs(nullptr, t1, p->dSkHash.p, p->dSkHash2.p, p->dSkGroup.p, p->dSkGroup2.p, (size_t) count, 0u, 64u, p->stream));
        FCHK(rocprim::radix_sort_pairs(nullptr, t2, p->dSkGroup2.p, p->dSkGroup.p, p->dSkHash2.p, p->dSkHash.p, (size_t) count, 0u, gbits, p->stream));
        FCHK(rocprim::exclusive_scan(nullptr, t3, p->dSkFlag.p, p->dSkPos.p, 0u, (size_t) count, rocprim::plus<uint32_t>(), p->stream));
        const size_t tb = std::max(t1, std::max(t2, t3));
        if ((rc = p->dSkTmp.reserve(tb))) return rc;
        const uint32_t blocks = (uint32_t) std::min<uint64_t>((count + 255) / 256, 4096);
        FCHK(hipMemsetAsync(p->dSkStart.p, 0xff, ngroups * sizeof(unsigned long long), p->stream));
        FTRY(p->sortTimer.start(p->stream));
        FCHK(rocprim::radix_sort_pairs(p->dSkTmp.p, t1, p->dSkHash.p, p->dSkHash2.p, p->dSkGroup.p, p->dSkGroup2.p, (size_t) count, 0u, 64u, p->stream));
        FCHK(rocprim::radix_sort_pairs(p->dSkTmp.p, t2, p->dSkGroup2.p, p->dSkGroup.p, p->dSkHash2.p, p->dSkHash.p, (size_t) count, 0u, gbits, p->stream));
        k_fa_sketch_flag<<<dim3(blocks), dim3(256), 0, p->stream>>>(p->dSkHash.p, p->dSkGroup.p, count, p->dSkFlag.p);
        FCHK(hipGetLastError());
        FCHK(rocprim::exclusive_scan(p->dSkTmp.p, t3, p->dSkFlag.p, p->dSkPos.p, 0u, (size_t) count, rocprim::plus<uint32_t>(), p->stream));
        k_fa_sketch_compact<<<dim3(blocks), dim3(256), 0, p->stream>>>(p->dSkHash.p, p->dSkGroup.p, p->dSkFlag.p, p->dSkPos.p, count, p->dSkHash2.p, p->dSkStart.p, p->dSkWords.p + 1);
        FCHK(hipGetLastError());
        FTRY(p->sortTimer.stop(p->stream));
        FCHK(hipMemcpyAsync(&distinct, p->dSkWords.p + 1, sizeof distinct, hipMemcpyDeviceToHost, p->stream));
        FCHK(hipMemcpyAsync(starts.data(), p->dSkStart.p, ngroups * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    }
    FCHK(hipStreamSynchronize(p->stream));
    if (count) FTRY(p->sortTimer.read(&p->sketchSortMs));
    // a group without a row starts where the next one does
    groupStart_host[ngroups] = distinct;
    for (uint32_t g = ngroups; g-- > 0;) groupStart_host[g] = starts[g] == ~0ull ? groupStart_host[g + 1] : starts[g];
    for (uint32_t g = 0; g < ngroups; g++) kmers_host[g] = kmers[g];
    *total = distinct;
    if (distinct > cap) return fail(-104, "sketch: %llu hashes, the buffer holds %llu", distinct, (unsigned long long) cap);
    if (distinct) {
        FCHK(hipMemcpyAsync(hashes_host, p->dSkHash2.p, distinct * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
    }
    return 0;
}

void mbgc_fasta_sketch_last(const mbgc_fasta_t *p, uint64_t *rows, uint64_t *reruns) {
    if (rows) *rows = p->sketchRows;
    if (reruns) *reruns = p->sketchReruns;
}

double mbgc_fasta_sketch_sort_ms(const mbgc_fasta_t *p) { return p->sketchSortMs; }

int mbgc_fasta_screen_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, const uint32_t *group_host, uint32_t ngroups,
                          uint32_t k, const uint64_t *keys_host, uint64_t nkeys, uint32_t *found_host, uint64_t foundCap, uint64_t *groupStart_host, uint64_t *total,
                          mbgc_fasta_screen_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs) {
    using namespace fa;
    if (k < 1 || k > 32) return fail(-103, "screen: k = %u (1 to 32)", k);
    if (nkeys == 0 || nkeys > SCREEN_MAX_KEYS) return fail(-103, "screen: %llu keys in one call (1 to 2^%u)", (unsigned long long) nkeys, SCREEN_KEYS_LOG);
    for (uint64_t i = 0; i < nkeys; i++) {
        if (k < 32 && keys_host[i] >> (2 * k)) return fail(-103, "screen: key %llu has bits above 2 k = %u", (unsigned long long) i, 2 * k);
        if (i && keys_host[i] <= keys_host[i - 1]) return fail(-103, "screen: the keys do not ascend strictly (at %llu)", (unsigned long long) i);
    }
    // (records and groups: the order of mbgc_fasta_sketch_dev's refusals)
    const uint64_t inside = n < 0xffffffffull ? first_outside(recs, n, seqBytes) : 0;
    uint64_t longest = 0;
    for (uint64_t r = 0; r < inside; r++) {
        if (group_host[r] >= ngroups) return fail(-103, "screen: record %llu names group %u of %u", (unsigned long long) r, group_host[r], ngroups);
        longest = std::max<uint64_t>(longest, recs[r].len);
    }
    uint64_t ntiles = 0;
    FTRY(scan_prepare(p, "screen", seq_dev, seqBytes, recs, n, [&](uint64_t r) { return sketch_positions(recs[r].len, k); }, ntiles));
    if (kernelMs) *kernelMs = 0;
    p->screenRows = p->screenPasses = p->screenReruns = 0;
    p->screenSortMs = 0;
    *total = *nHits = 0;
    for (uint32_t g = 0; g <= ngroups; g++) groupStart_host[g] = 0;
    if (ntiles == 0) return 0;                                       // (no record holds a k-mer)
    // ---- the filter and the table, built here and uploaded
    const uint64_t slots = screen_slots(nkeys);
    p->scrFilter.resize(SCREEN_FILTER_WORDS);
    p->scrTable.resize(slots);
    screen_build_filter(keys_host, nkeys, p->scrFilter.data());
    screen_build_table(keys_host, nkeys, p->scrTable.data(), slots);
    uint32_t keyBits = 1, gbits = 1, rbits = 1, pbits = 1;
    while (((uint64_t) 1 << keyBits) < nkeys) keyBits++;
    while (gbits < 32 && ((uint64_t) 1 << gbits) < ngroups) gbits++;
    while (rbits < 32 && ((uint64_t) 1 << rbits) < n) rbits++;
    while (pbits < 64 && ((uint64_t) 1 << pbits) < longest) pbits++;
    int rc;
    if ((rc = p->dScrGroups.reserve(n)) || (rc = p->dScrFilter.reserve(SCREEN_FILTER_WORDS)) || (rc = p->dScrTable.reserve(slots)) || (rc = p->dScrKeys.reserve(nkeys)) ||
        (rc = p->dScrStart.reserve(ngroups)) || (rc = p->dScrWords.reserve(3))) return rc;
    FCHK(hipMemcpyAsync(p->dScrGroups.p, group_host, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dScrFilter.p, p->scrFilter.data(), SCREEN_FILTER_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dScrTable.p, p->scrTable.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dScrKeys.p, keys_host, nkeys * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    // ---- the scan. The row buffer is this call's own: when the cursor passed it, it grows to the cursor's count and the kernel runs again
    const bool wantHits = hits_host != nullptr;
    uint64_t rowCap = std::max<uint64_t>(SCREEN_ROWS_FIRST, p->screenRowCap);
    unsigned long long words[3] = {0, 0, 0};
    for (;;) {
        if ((rc = p->dScrGK.reserve(rowCap)) || (wantHits && ((rc = p->dScrPos.reserve(rowCap)) || (rc = p->dScrRK.reserve(rowCap))))) return rc;
        FCHK(hipMemsetAsync(p->dScrWords.p, 0, 3 * sizeof(unsigned long long), p->stream));
        FTRY(p->timer.start(p->stream));
        // one launch whatever n is: the blocks stride over the tiles (k_fa_sketch's grid; four of these blocks fit a CU at a time)
        k_fa_screen<<<dim3((uint32_t) std::min<uint64_t>(ntiles, 2048)), dim3(SCREEN_THREADS), 0, p->stream>>>(seq_dev, seqBytes, p->dScanRecs.p, p->dScrGroups.p, p->dScanTiles.p, (uint32_t) n,
                                                                                                                 ntiles, k, p->dScrFilter.p, p->dScrTable.p, (uint32_t) (slots - 1), p->dScrKeys.p, keyBits,
                                                                                                                 p->dScrGK.p, wantHits ? p->dScrPos.p : nullptr, wantHits ? p->dScrRK.p : nullptr, rowCap,
                                                                                                                 p->dScrWords.p);
        FCHK(hipGetLastError());
        FTRY(p->timer.stop(p->stream));
        FCHK(hipMemcpyAsync(words, p->dScrWords.p, sizeof words, hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
        FTRY(p->timer.read(kernelMs));
        if (words[0] <= rowCap) break;
        if (words[0] >= 0xffffffffull) return fail(-103, "screen: %llu rows in one call (fewer keys, or fewer records)", words[0]);
        rowCap = p->screenRowCap = words[0];
        p->screenReruns++;
    }
    const unsigned long long count = words[0];
    p->screenRows = count;
    p->screenPasses = words[2];
    *nHits = count;                                                  // (a position holds one k-mer, a k-mer is one key: every row is a hit, once)
    std::vector<unsigned long long> starts(ngroups, ~0ull);
    unsigned long long distinct = 0;
    const bool sortHits = wantHits && count && count <= hitCap;
    if (count) {
        // one sort of group << keyBits | key; the first row of every (group, key) is flagged, the flags' exclusive sum is the row's place
        // among the distinct ones. The hits: a stable sort by position, then a stable sort by record
        if ((rc = p->dScrGK2.reserve(count)) || (rc = p->dSkFlag.reserve(count)) || (rc = p->dSkPos.reserve(count)) || (rc = p->dScrFound.reserve(count)) ||
            (sortHits && ((rc = p->dScrPos2.reserve(count)) || (rc = p->dScrRK2.reserve(count))))) return rc;
        size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        FCHK(rocprim::radix_sort_keys(nullptr, t1, p->dScrGK.p, p->dScrGK2.p, (size_t) count, 0u, keyBits + gbits, p->stream));
        FCHK(rocprim::exclusive_scan(nullptr, t2, p->dSkFlag.p, p->dSkPos.p, 0u, (size_t) count, rocprim::plus<uint32_t>(), p->stream));
        if (sortHits) {
            FCHK(rocprim::radix_sort_pairs(nullptr, t3, p->dScrPos.p, p->dScrPos2.p, p->dScrRK.p, p->dScrRK2.p, (size_t) count, 0u, pbits, p->stream));
            FCHK(rocprim::radix_sort_pairs(nullptr, t4, p->dScrRK2.p, p->dScrRK.p, p->dScrPos2.p, p->dScrPos.p, (size_t) count, 32u, 32u + rbits, p->stream));
        }
        if ((rc = p->dSkTmp.reserve(std::max(std::max(t1, t2), std::max(t3, t4))))) return rc;
        const uint32_t blocks = (uint32_t) std::min<uint64_t>((count + 255) / 256, 4096);
        FCHK(hipMemsetAsync(p->dScrStart.p, 0xff, ngroups * sizeof(unsigned long long), p->stream));
        FTRY(p->sortTimer.start(p->stream));
        FCHK(rocprim::radix_sort_keys(p->dSkTmp.p, t1, p->dScrGK.p, p->dScrGK2.p, (size_t) count, 0u, keyBits + gbits, p->stream));
        k_fa_screen_flag<<<dim3(blocks), dim3(256), 0, p->stream>>>(p->dScrGK2.p, count, p->dSkFlag.p);
        FCHK(hipGetLastError());
        FCHK(rocprim::exclusive_scan(p->dSkTmp.p, t2, p->dSkFlag.p, p->dSkPos.p, 0u, (size_t) count, rocprim::plus<uint32_t>(), p->stream));
        k_fa_screen_compact<<<dim3(blocks), dim3(256), 0, p->stream>>>(p->dScrGK2.p, p->dSkFlag.p, p->dSkPos.p, count, keyBits, p->dScrFound.p, p->dScrStart.p, p->dScrWords.p + 1);
        FCHK(hipGetLastError());
        if (sortHits) {
            FCHK(rocprim::radix_sort_pairs(p->dSkTmp.p, t3, p->dScrPos.p, p->dScrPos2.p, p->dScrRK.p, p->dScrRK2.p, (size_t) count, 0u, pbits, p->stream));
            FCHK(rocprim::radix_sort_pairs(p->dSkTmp.p, t4, p->dScrRK2.p, p->dScrRK.p, p->dScrPos2.p, p->dScrPos.p, (size_t) count, 32u, 32u + rbits, p->stream));
        }
        FTRY(p->sortTimer.stop(p->stream));
        FCHK(hipMemcpyAsync(&distinct, p->dScrWords.p + 1, sizeof distinct, hipMemcpyDeviceToHost, p->stream));
        FCHK(hipMemcpyAsync(starts.data(), p->dScrStart.p, ngroups * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
        FCHK(hipStreamSynchronize(p->stream));
        FTRY(p->sortTimer.read(&p->screenSortMs));
    }
    // a group without a row starts where the next one does
    groupStart_host[ngroups] = distinct;
    for (uint32_t g = ngroups; g-- > 0;) groupStart_host[g] = starts[g] == ~0ull ? groupStart_host[g + 1] : starts[g];
    *total = distinct;
    if (distinct > foundCap) return fail(-104, "screen: %llu found keys, the buffer holds %llu", distinct, (unsigned long long) foundCap);
    if (distinct) FCHK(hipMemcpyAsync(found_host, p->dScrFound.p, distinct * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    std::vector<uint64_t> pos, recKey;
    if (sortHits) {
        pos.resize(count); recKey.resize(count);
        FCHK(hipMemcpyAsync(pos.data(), p->dScrPos.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        FCHK(hipMemcpyAsync(recKey.data(), p->dScrRK.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
    }
    FCHK(hipStreamSynchronize(p->stream));
    if (wantHits && count > hitCap) return fail(-104, "screen: %llu hits, the buffer holds %llu", count, (unsigned long long) hitCap);
    for (uint64_t i = 0; sortHits && i < count; i++) hits_host[i] = mbgc_fasta_screen_hit_t{pos[i], (uint32_t) (recKey[i] >> 32), (uint32_t) recKey[i]};
    return 0;
}

void mbgc_fasta_screen_last(const mbgc_fasta_t *p, uint64_t *hitRows, uint64_t *filterPasses, uint64_t *reruns, double *sortMs) {
    if (hitRows) *hitRows = p->screenRows;
    if (filterPasses) *filterPasses = p->screenPasses;
    if (reruns) *reruns = p->screenReruns;
    if (sortMs) *sortMs = p->screenSortMs;
}

int mbgc_fasta_sketch_pairs_dev(mbgc_fasta_t *p, const uint64_t *hashes_host, const uint64_t *groupStart_host, uint32_t ngroups, const uint32_t *pairs_host, uint64_t npairs,
                                uint32_t *shared_host, double *kernelMs) {
    using namespace fa;
    if (groupStart_host[0] != 0) return fail(-103, "pairs: the first group starts at %llu", (unsigned long long) groupStart_host[0]);
    for (uint32_t g = 0; g < ngroups; g++) {
        if (groupStart_host[g + 1] < groupStart_host[g]) return fail(-103, "pairs: group %u ends in front of its start", g);
        for (uint64_t i = groupStart_host[g] + 1; i < groupStart_host[g + 1]; i++)
            if (hashes_host[i] <= hashes_host[i - 1]) return fail(-103, "pairs: the hashes of group %u do not ascend strictly (at %llu)", g, (unsigned long long) (i - groupStart_host[g]));
    }
    const uint64_t nh = groupStart_host[ngroups];
    if (nh >= 0xffffffffull) return fail(-103, "pairs: %llu hashes in one call", (unsigned long long) nh);
    if (!pairs_host && npairs != (uint64_t) ngroups * (ngroups ? ngroups - 1 : 0) / 2)
        return fail(-103, "pairs: %llu pairs asked without a list, %u groups have %llu", (unsigned long long) npairs, ngroups, (unsigned long long) ngroups * (ngroups ? ngroups - 1 : 0) / 2);
    if (pairs_host)
        for (uint64_t q = 0; q < 2 * npairs; q++)
            if (pairs_host[q] >= ngroups) return fail(-103, "pairs: pair %llu names group %u of %u", (unsigned long long) (q / 2), pairs_host[q], ngroups);
    if (kernelMs) *kernelMs = 0;
    if (npairs == 0) return 0;
    FCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = p->dPairHashes.reserve(std::max<uint64_t>(nh, 1))) || (rc = p->dPairStart.reserve(ngroups + 1)) || (rc = p->dPairShared.reserve(npairs)) ||
        (pairs_host && (rc = p->dPairList.reserve(2 * npairs)))) return rc;
    if (nh) FCHK(hipMemcpyAsync(p->dPairHashes.p, hashes_host, nh * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dPairStart.p, groupStart_host, (ngroups + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    if (pairs_host) FCHK(hipMemcpyAsync(p->dPairList.p, pairs_host, 2 * npairs * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream));
    // a wave per pair, four to a block; the waves stride over the pairs
    k_fa_sketch_pairs<<<dim3((uint32_t) std::min<uint64_t>((npairs + 3) / 4, 8192)), dim3(256), 0, p->stream>>>(p->dPairHashes.p, p->dPairStart.p, ngroups, pairs_host ? p->dPairList.p : nullptr,
                                                                                                                  npairs, p->dPairShared.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    FCHK(hipMemcpyAsync(shared_host, p->dPairShared.p, npairs * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    return 0;
}

int mbgc_fasta_crc_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint32_t *crc_out_host,
                       double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(CrcIn) == sizeof(mbgc_fasta_crc_rec_t), "the table builder reads the ABI's ranges");
    if (kernelMs) *kernelMs = 0;
    if (n >= CRC_FIRST) return fail(-103, "crc: %llu ranges in one call", (unsigned long long) n);
    if (const uint64_t k = first_outside(recs, n, seqBytes); k < n) return fail(-103, "crc: range %llu lies outside the buffer", (unsigned long long) k);
    uint64_t nrows = 0;
    for (uint64_t k = 0; k < n; k++) nrows += (recs[k].len + CRC_PIECE - 1) / CRC_PIECE;
    if (nrows >= 0xffffffffull) return fail(-103, "crc: %llu rows in one call", (unsigned long long) nrows);
    if (nrows == 0) {
        for (uint64_t k = 0; k < n; k++) crc_out_host[k] = 0;
        return 0;
    }
    std::vector<CrcRow> rows;
    std::vector<uint64_t> behind;
    CrcPlan plan;
    const uint64_t nwaves = crc_build_table((const CrcIn *) recs, n, rows, behind, plan);
    FCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = p->dCrcRows.reserve(rows.size())) || (rc = p->dCrcBehind.reserve(behind.size() + 1)) || (rc = p->dCrcOut.reserve(n))) return rc;
    if (!p->dCrcConsts.p) {
        static const CrcConsts consts = [] { CrcConsts K; crc_build_consts(K); return K; }();
        if ((rc = p->dCrcConsts.reserve(1))) return rc;
        FCHK(hipMemcpyAsync(p->dCrcConsts.p, &consts, sizeof consts, hipMemcpyHostToDevice, p->stream));
    }
    FCHK(hipMemcpyAsync(p->dCrcRows.p, rows.data(), rows.size() * sizeof(CrcRow), hipMemcpyHostToDevice, p->stream));
    if (!behind.empty()) FCHK(hipMemcpyAsync(p->dCrcBehind.p, behind.data(), behind.size() * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemsetAsync(p->dCrcOut.p, 0, n * sizeof(uint32_t), p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    // one launch whatever n is: the waves stride over the rows. MBGC_HIP_CRC_LOOKUP=nibble: the per-bank nibble tables, the alternative
    // profiles/crc_bench.py measures the byte table against
    static const bool byteTable = !(getenv("MBGC_HIP_CRC_LOOKUP") && strcmp(getenv("MBGC_HIP_CRC_LOOKUP"), "nibble") == 0);
    const dim3 grid((uint32_t) std::min<uint64_t>((nwaves + CRC_WAVES - 1) / CRC_WAVES, 2048));
    if (byteTable) k_fa_crc<CRC_LOOKUP_BYTE><<<grid, dim3(CRC_THREADS), 0, p->stream>>>(seq_dev, p->dCrcRows.p, p->dCrcBehind.p, plan, p->dCrcConsts.p, p->dCrcOut.p);
    else k_fa_crc<CRC_LOOKUP_NIBBLE><<<grid, dim3(CRC_THREADS), 0, p->stream>>>(seq_dev, p->dCrcRows.p, p->dCrcBehind.p, plan, p->dCrcConsts.p, p->dCrcOut.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    std::vector<uint32_t> out(n);                                    // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(out.data(), p->dCrcOut.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    for (uint64_t k = 0; k < n; k++) crc_out_host[k] = recs[k].len ? ~out[k] : 0u;      // the final XOR, once per range
    return 0;
}

int mbgc_fasta_crc_host(mbgc_fasta_t *p, const mbgc_fasta_record_t *records, uint64_t nrec, uint32_t *crc_out_host, double *kernelMs) {
    std::vector<mbgc_fasta_crc_rec_t> recs(nrec);
    for (uint64_t r = 0; r < nrec; r++) recs[r] = mbgc_fasta_crc_rec_t{records[r].seqOff, records[r].seqLen};
    return mbgc_fasta_crc_dev(p, p->dHostOut.p, p->hostParsedBytes, recs.data(), nrec, crc_out_host, kernelMs);
}

uint32_t mbgc_fasta_crc_combine(uint32_t crcA, uint32_t crcB, uint64_t lenB) { return fa::crc_mulmod(fa::crc_xpow8(lenB), crcA) ^ crcB; }

int mbgc_fasta_inflate_dev(mbgc_fasta_t *p, const uint8_t *gz_dev, uint64_t gzBytes, uint8_t *out_dev, uint64_t outBytes,
                           const mbgc_fasta_inflate_job_t *jobs, uint64_t njobs, mbgc_fasta_inflate_result_t *results, double *kernelMs) {
    using namespace fa;
    static_assert(sizeof(InfJob) == sizeof(mbgc_fasta_inflate_job_t) && sizeof(InfResult) == sizeof(mbgc_fasta_inflate_result_t), "the kernel reads the ABI's jobs");
    static_assert(INF_OK == MBGC_INFLATE_OK && INF_ESHORT == MBGC_INFLATE_ESHORT && INF_EDATA == MBGC_INFLATE_EDATA && INF_ECHECK == MBGC_INFLATE_ECHECK, "status codes");
    if (kernelMs) *kernelMs = 0;
    if (njobs >= 0xffffffffull) return fail(-103, "inflate: %llu jobs in one call", (unsigned long long) njobs);
    std::vector<std::pair<uint64_t, uint64_t>> ranges;               // the output ranges that hold bytes
    for (uint64_t k = 0; k < njobs; k++) {
        const mbgc_fasta_inflate_job_t &x = jobs[k];
        if (x.inOff > gzBytes || x.inLen > gzBytes - x.inOff || x.outOff > outBytes || x.outCap > outBytes - x.outOff)
            return fail(-103, "inflate: job %llu lies outside the buffers", (unsigned long long) k);
        if (x.outCap) ranges.emplace_back(x.outOff, x.outOff + x.outCap);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); k++)
        if (ranges[k].first < ranges[k - 1].second) return fail(-103, "inflate: the output ranges of two jobs overlap at byte %llu", (unsigned long long) ranges[k].first);
    // the two buffers may be one, or overlap: no job's input may lie where a job's output is written (the output ranges are
    // sorted and apart, so the last one that starts in front of the input's end is the one that can reach into it)
    const uint64_t gzA = (uint64_t) (uintptr_t) gz_dev, outA = (uint64_t) (uintptr_t) out_dev;
    if (gzA < outA + outBytes && outA < gzA + gzBytes)
        for (uint64_t k = 0; k < njobs; k++) {
            const uint64_t a = gzA + jobs[k].inOff, e = a + jobs[k].inLen;
            if (a == e || e <= outA) continue;
            auto it = std::lower_bound(ranges.begin(), ranges.end(), std::make_pair(e - outA, (uint64_t) 0));   // the first range that starts at or behind the input's end
            if (it != ranges.begin() && outA + std::prev(it)->second > a)
                return fail(-103, "inflate: the input of job %llu overlaps a job's output range", (unsigned long long) k);
        }
    if (njobs == 0) return 0;
    FCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = p->dInfJobs.reserve(njobs)) || (rc = p->dInfResults.reserve(njobs))) return rc;
    FCHK(hipMemcpyAsync(p->dInfJobs.p, jobs, njobs * sizeof(InfJob), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint64_t k0 = 0; k0 < njobs; k0 += FMT_SLICE)
        k_fa_inflate<<<dim3((uint32_t) std::min<uint64_t>(FMT_SLICE, njobs - k0)), dim3(INF_WAVE), 0, p->stream>>>(gz_dev, out_dev, p->dInfJobs.p, (uint32_t) k0, (uint32_t) njobs,
                                                                                                                  p->dInfResults.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    std::vector<InfResult> got(njobs);                               // (the caller's array stays as it is unless the whole call succeeds)
    FCHK(hipMemcpyAsync(got.data(), p->dInfResults.p, njobs * sizeof(InfResult), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    FTRY(p->timer.read(kernelMs));
    memcpy(results, got.data(), njobs * sizeof(InfResult));
    return 0;
}

uint64_t mbgc_fasta_deflate_bound(uint64_t inLen) {
    return 18 + std::max<uint64_t>(1, (inLen + MBGC_DEFLATE_CHUNK - 1) / MBGC_DEFLATE_CHUNK) * 10 + inLen;
}

int mbgc_fasta_deflate_dev(mbgc_fasta_t *p, const uint8_t *text_dev, uint64_t textBytes, const mbgc_fasta_deflate_job_t *jobs, uint64_t njobs,
                           uint8_t *gz_dev, uint64_t gzCap, mbgc_fasta_deflate_result_t *results, uint64_t *gzBytes, double *kernelMs) {
    using namespace fa;
    static_assert(DEF_CHUNK == MBGC_DEFLATE_CHUNK, "the chunk of the ABI");
    if (kernelMs) *kernelMs = 0;
    if (gzBytes) *gzBytes = 0;
    uint64_t nc64 = 0;
    for (uint64_t k = 0; k < njobs; k++) {
        const mbgc_fasta_deflate_job_t &x = jobs[k];
        if (x.inOff > textBytes || x.inLen > textBytes - x.inOff) return fail(-103, "deflate: job %llu lies outside the text", (unsigned long long) k);
        nc64 += std::max<uint64_t>(1, (x.inLen + DEF_CHUNK - 1) / DEF_CHUNK);
    }
    if (njobs >= 0xffffffffull || nc64 >= 0xffffffffull) return fail(-103, "deflate: %llu jobs, %llu chunks in one call", (unsigned long long) njobs, (unsigned long long) nc64);
    if (njobs == 0) return 0;
    const uint32_t nc = (uint32_t) nc64;
    std::vector<DefChunk> chunks(nc);
    std::vector<DefJobIn> jtab(njobs);
    std::vector<DefPackIn> pack(nc);
    for (uint64_t k = 0, c = 0; k < njobs; k++) {
        const uint32_t m = (uint32_t) std::max<uint64_t>(1, (jobs[k].inLen + DEF_CHUNK - 1) / DEF_CHUNK);
        jtab[k] = {jobs[k].inLen, (uint32_t) c, m};
        for (uint32_t i = 0; i < m; i++, c++) {
            const uint64_t at = (uint64_t) i * DEF_CHUNK;
            chunks[c] = {jobs[k].inOff + at, (uint32_t) std::min<uint64_t>(DEF_CHUNK, jobs[k].inLen - at), i + 1 == m ? 1u : 0u};
            pack[c] = {0, (uint32_t) k, (i == 0 ? 1u : 0u) | (i + 1 == m ? 2u : 0u)};
        }
    }
    FCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = p->dDefChunks.reserve(nc)) || (rc = p->dDefSlots.reserve((size_t) nc * DEF_SLOT)) || (rc = p->dDefOuts.reserve(nc)) || (rc = p->dDefPack.reserve(nc)) ||
        (rc = p->dDefJobs.reserve(njobs)) || (rc = p->dDefCrc.reserve(njobs)))
        return rc;
    FCHK(hipMemcpyAsync(p->dDefChunks.p, chunks.data(), nc * sizeof(DefChunk), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint32_t c0 = 0; c0 < nc; c0 += FMT_SLICE)
        k_fa_deflate<<<dim3(std::min(FMT_SLICE, nc - c0)), dim3(DEF_WAVE), 0, p->stream>>>(text_dev, p->dDefChunks.p, c0, nc, p->dDefSlots.p, p->dDefOuts.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    // the chunks' sizes come back (8 bytes per chunk with their CRCs); the scan that places them runs here
    std::vector<DefChunkOut> outs(nc);
    FCHK(hipMemcpyAsync(outs.data(), p->dDefOuts.p, nc * sizeof(DefChunkOut), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    double ms = 0;
    FTRY(p->timer.read(&ms));
    std::vector<mbgc_fasta_deflate_result_t> res(njobs);
    uint64_t at = 0;
    for (uint64_t k = 0; k < njobs; k++) {
        res[k] = {at, 0, 0, jtab[k].nchunks, 0, 0};
        at += 10;
        for (uint32_t c = jtab[k].chunk0; c < jtab[k].chunk0 + jtab[k].nchunks; c++) {
            const uint32_t bytes = outs[c].bytes & ~DEF_STORED;
            if (bytes > DEF_CHUNK + 10) return fail(-100, "deflate: chunk %u reports %u bytes", c, bytes);
            pack[c].dst = at;
            at += bytes;
            res[k].storedChunks += (outs[c].bytes & DEF_STORED) != 0;
        }
        at += 8;
        res[k].outLen = at - res[k].outOff;
    }
    if (gzBytes) *gzBytes = at;
    if (at > gzCap) return fail(-104, "gzip output needs %llu bytes, capacity %llu", (unsigned long long) at, (unsigned long long) gzCap);
    FCHK(hipMemcpyAsync(p->dDefPack.p, pack.data(), nc * sizeof(DefPackIn), hipMemcpyHostToDevice, p->stream));
    FCHK(hipMemcpyAsync(p->dDefJobs.p, jtab.data(), njobs * sizeof(DefJobIn), hipMemcpyHostToDevice, p->stream));
    FTRY(p->timer.start(p->stream, kernelMs != nullptr));
    for (uint32_t c0 = 0; c0 < nc; c0 += FMT_SLICE)
        k_fa_deflate_pack<<<dim3(std::min(FMT_SLICE, nc - c0)), dim3(DEF_WAVE), 0, p->stream>>>(p->dDefSlots.p, p->dDefOuts.p, p->dDefPack.p, p->dDefJobs.p, c0, nc, gz_dev,
                                                                                               p->dDefCrc.p);
    FCHK(hipGetLastError());
    FTRY(p->timer.stop(p->stream));
    std::vector<uint32_t> crcs(njobs);
    FCHK(hipMemcpyAsync(crcs.data(), p->dDefCrc.p, njobs * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    double packMs = 0;
    FTRY(p->timer.read(&packMs));
    if (kernelMs) *kernelMs = ms + packMs;
    for (uint64_t k = 0; k < njobs; k++) res[k].crc32 = crcs[k];
    memcpy(results, res.data(), njobs * sizeof(mbgc_fasta_deflate_result_t));
    return 0;
}

int mbgc_fasta_download_begin(mbgc_fasta_t *p, void *dst_host, const uint8_t *src_dev, uint64_t bytes) {
    using namespace fa;
    if (p->copyPending) return fail(-103, "download_begin: the download before this one has not been waited for");
    FCHK(hipSetDevice(p->device));
    if (!p->copyStream) {
        FCHK(hipStreamCreateWithFlags(&p->copyStream, hipStreamNonBlocking));
        FCHK(hipEventCreate(&p->copyEv[0])); FCHK(hipEventCreate(&p->copyEv[1]));
    }
    FCHK(hipEventRecord(p->copyEv[0], p->copyStream));
    if (bytes) FCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, p->copyStream));
    FCHK(hipEventRecord(p->copyEv[1], p->copyStream));
    p->copyPending = true;
    return 0;
}

int mbgc_fasta_download_wait(mbgc_fasta_t *p, double *copyMs) {
    using namespace fa;
    if (copyMs) *copyMs = 0;
    if (!p->copyPending) return 0;
    FCHK(hipSetDevice(p->device));
    p->copyPending = false;
    FCHK(hipStreamSynchronize(p->copyStream));
    if (copyMs) { float ms = 0; FCHK(hipEventElapsedTime(&ms, p->copyEv[0], p->copyEv[1])); *copyMs = ms; }
    return 0;
}

int mbgc_fasta_gather_dev(mbgc_fasta_t *p, const uint8_t *src_dev, uint64_t srcBytes, const uint64_t *off, const uint64_t *len, uint64_t n,
                          uint8_t sep, uint8_t *out_host, uint64_t outCap, uint64_t *outBytes) {
    using namespace fa;
    *outBytes = 0;
    if (n >= 0xffffffffull) return fail(-103, "gather: %llu pieces in one call", (unsigned long long) n);
    std::vector<uint64_t> tab(3 * (size_t) n);
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        if (off[k] > srcBytes || len[k] > srcBytes - off[k]) return fail(-103, "gather: piece %llu lies outside the buffer", (unsigned long long) k);
        tab[3 * k] = off[k]; tab[3 * k + 1] = len[k]; tab[3 * k + 2] = total;
        total += len[k] + 1;
    }
    *outBytes = total;
    if (total > outCap) return fail(-104, "gather needs %llu bytes, capacity %llu", (unsigned long long) total, (unsigned long long) outCap);
    if (n == 0) return 0;
    FCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = p->dGatherTab.reserve(tab.size())) || (rc = p->dGatherOut.reserve(total))) return rc;
    FCHK(hipMemcpyAsync(p->dGatherTab.p, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
    for (uint64_t k0 = 0; k0 < n; k0 += FMT_SLICE)
        k_fa_gather<<<dim3((uint32_t) std::min<uint64_t>(FMT_SLICE, n - k0)), dim3(THREADS), 0, p->stream>>>(src_dev, p->dGatherTab.p, (uint32_t) k0, (uint32_t) n, sep, p->dGatherOut.p);
    FCHK(hipGetLastError());
    FCHK(hipMemcpyAsync(out_host, p->dGatherOut.p, total, hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    return 0;
}

int mbgc_fasta_dev_alloc(mbgc_fasta_t *p, uint64_t bytes, uint8_t **out) {
    using namespace fa;
    *out = nullptr;
    FCHK(hipSetDevice(p->device));
    if (hipMalloc((void **) out, bytes ? bytes : 1) != hipSuccess) { (void) hipGetLastError(); return fail(-101, "device allocation of %llu bytes failed", (unsigned long long) bytes); }
    return 0;
}

int mbgc_fasta_dev_free(mbgc_fasta_t *p, uint8_t *ptr) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    if (ptr) FCHK(hipFree(ptr));
    return 0;
}

int mbgc_fasta_dev_copy(mbgc_fasta_t *p, uint8_t *dst_dev, const uint8_t *src_dev, uint64_t bytes) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    if (bytes) FCHK(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    return 0;
}

int mbgc_fasta_download(mbgc_fasta_t *p, void *dst_host, const uint8_t *src_dev, uint64_t bytes) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    if (bytes) FCHK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    return 0;
}

// Page-locked staging memory. hipHostMalloc takes 33-37 ms for a round's 160 MB on this host (profiles/pin_bench.hip) — twice,
// in front of the first round; memory of the process's own in 2 MB pages (madvise, where the system gives them) is registered in
// about 1 ms once it is there, and touching it takes 10 ms instead of 27. So: mmap, ask for huge pages, register.
namespace fa {
static std::mutex g_hostMu;
static std::map<void *, std::pair<void *, size_t>> g_hostMaps;      // registered pointer -> (mapping, its length)
}

int mbgc_fasta_host_alloc(mbgc_fasta_t *p, uint64_t bytes, void **out) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    *out = nullptr;
    const size_t HUGE = (size_t) 2 << 20, n = ((bytes ? bytes : 1) + HUGE - 1) & ~(HUGE - 1);
    void *m = mmap(nullptr, n + HUGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) return fail(-101, "cannot map %llu B of host memory", (unsigned long long) bytes);
    void *a = (void *) (((uintptr_t) m + HUGE - 1) & ~(uintptr_t) (HUGE - 1));
    (void) madvise(a, n, MADV_HUGEPAGE);
    if (hipHostRegister(a, n, hipHostRegisterDefault) != hipSuccess) {
        (void) hipGetLastError();
        munmap(m, n + HUGE);
        return fail(-101, "cannot pin %llu B of host memory", (unsigned long long) bytes);
    }
    { std::lock_guard<std::mutex> g(g_hostMu); g_hostMaps[a] = std::make_pair(m, n + HUGE); }
    *out = a;
    return 0;
}

int mbgc_fasta_host_free(mbgc_fasta_t *p, void *ptr) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    if (!ptr) return 0;
    std::pair<void *, size_t> m;
    {
        std::lock_guard<std::mutex> g(g_hostMu);
        auto it = g_hostMaps.find(ptr);
        if (it == g_hostMaps.end()) return fail(-100, "mbgc_fasta_host_free: not a pointer of mbgc_fasta_host_alloc");
        m = it->second;
        g_hostMaps.erase(it);
    }
    FCHK(hipHostUnregister(ptr));
    munmap(m.first, m.second);
    return 0;
}

int mbgc_fasta_upload(mbgc_fasta_t *p, uint8_t *dst_dev, const void *src_host, uint64_t bytes) {
    using namespace fa;
    FCHK(hipSetDevice(p->device));
    if (bytes) FCHK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, p->stream));
    FCHK(hipStreamSynchronize(p->stream));
    return 0;
}

}  // extern "C"
