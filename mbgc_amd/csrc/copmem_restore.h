// The inverse of the `-m3` reverse-complement pass (include/mbgc_copmem.h): SimpleSequenceMatcher::restoreRCMatchedSequence,
// matching/SimpleSequenceMatcher.cpp:178-211, which the reference's decoder calls at MBGC_Decoder.cpp:1137. There it is a
// sequential loop — find a mark, append the reverse complement of text already restored, go on. Here, two steps:
//
//   plan    the positions of RC_MATCH_MARK in the cut stream are compacted in order (per-tile counts, a rocPRIM scan, an ordered
//           write); the byte-frugal varints of rcMapLen (readUIntByteFrugal, utils/helper.h:232-241) are decoded in parallel — a
//           byte below 128 ends a value, a scan of those flags numbers the values, the first byte of each decodes it; a scan of
//           the lengths gives cum[i] and d[i] = markPos[i] - i + cum[i], where match i starts in restored coordinates. Every
//           bound is checked here, before any position taken from the maps is used as an address: src[i] + len[i] <= d[i].
//   fill    every output position is resolved on its own: binary search of d[] for the match or literal run it lies in; inside
//           a match it is mirrored into the source (one hop, strictly lower position) and searched again; a literal is read from
//           the cut stream. complementsLUT is applied as it would be after that many hops (lut . lut . lut == lut).
// Included by copmem.hip (uses cm::Buf, cm::fail, CCHK). What one item or lane does is copmem_restore_lane.h, plain C++ that
// tests/rcrestore_emu.cpp runs on the CPU; here are the kernels around it — staging, tile loops, scan, atomics — and the host's calls.
#pragma once

#include <rocprim/block/block_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace cmr {

using cm::Buf;
using cm::fail;

#include "copmem_restore_lane.h"                     // constants, Plan, and what one item or lane does: plain C++

struct State {
    Buf<uint8_t> dCut, dMapOff, dMapLen, dLut, dTmp, dOut;
    Buf<uint64_t> dCounts, dTileOff, dMarkPos, dValIdx, dVal, dLen, dCum, dD, dSrc, dRes;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool planned = false;
    uint64_t n = 0, M = 0, orgLen = 0;
    void release() {
        dCut.release(); dMapOff.release(); dMapLen.release(); dLut.release(); dTmp.release(); dOut.release(); dCounts.release(); dTileOff.release();
        dMarkPos.release(); dValIdx.release(); dVal.release(); dLen.release(); dCum.release(); dD.release(); dSrc.release(); dRes.release();
        if (ev0) (void) hipEventDestroy(ev0);
        if (ev1) (void) hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
};

__device__ __forceinline__ uint32_t marks_in(const uint4 v) {
    uint32_t c = 0;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) c += ((w[k] >> (8 * b)) & 0xFFu) == MARK;
    return c;
}

// ---- plan ----------------------------------------------------------------------------------------------------------------
// cut is padded with zero bytes up to a multiple of 16 (and beyond): a lane's 16-byte load never leaves the allocation
__global__ void __launch_bounds__(TPB) k_mark_count(const uint8_t *__restrict__ cut, uint64_t n, uint64_t *__restrict__ counts, uint64_t ntiles) {
    __shared__ uint32_t sCount;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        const uint64_t p = tile * TILE + (uint64_t) threadIdx.x * LANE;
        if (p < n) {
            const uint32_t c = marks_in(*(const uint4 *) (cut + p));
            if (c) atomicAdd(&sCount, c);
        }
        __syncthreads();
        if (threadIdx.x == 0) counts[tile] = sCount;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(TPB) k_mark_write(const uint8_t *__restrict__ cut, uint64_t n, const uint64_t *__restrict__ tileOff,
                                                    uint64_t *__restrict__ markPos, uint64_t M, uint64_t ntiles) {
    using Scan = rocprim::block_scan<uint32_t, TPB>;
    __shared__ typename Scan::storage_type tmp;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t first = tileOff[tile];
        if (tileOff[tile + 1] == first) continue;                          // (the same for the whole workgroup)
        const uint64_t p = tile * TILE + (uint64_t) threadIdx.x * LANE;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < n) v = *(const uint4 *) (cut + p);
        const uint32_t c = marks_in(v);
        uint32_t before = 0;
        Scan().exclusive_scan(c, before, 0u, tmp);
        __syncthreads();
        if (c) {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint64_t at = first + before;
            for (int b = 0; b < LANE; b++)
                if (((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) == MARK) {
                    if (at < M) markPos[at] = p + b;
                    at++;
                }
        }
    }
}
// one thread per byte of rcMapLen; the first byte of a value decodes it (little-endian base 128, the last byte below 128)
__global__ void __launch_bounds__(TPB) k_varint_decode(const uint8_t *__restrict__ bytes, uint64_t nbytes, const uint64_t *__restrict__ valIdx,
                                                       uint64_t *__restrict__ val, uint64_t nval, uint64_t *__restrict__ res) {
    const uint64_t stride = (uint64_t) gridDim.x * TPB;
    for (uint64_t j = (uint64_t) blockIdx.x * TPB + threadIdx.x; j < nbytes; j += stride) {
        if (!value_starts_at(bytes, j)) continue;
        bool tooLong;
        const uint64_t v = value_at(bytes, nbytes, j, tooLong);
        if (tooLong) atomicOr((unsigned long long *) &res[0], (unsigned long long) E_VARINT_LONG);
        const uint64_t at = valIdx[j];
        if (at < nval) val[at] = v;
    }
}
__global__ void __launch_bounds__(TPB) k_lengths(const uint64_t *__restrict__ val, uint64_t M, uint64_t *__restrict__ len) {
    const uint64_t stride = (uint64_t) gridDim.x * TPB;
    for (uint64_t i = (uint64_t) blockIdx.x * TPB + threadIdx.x; i <= M; i += stride) len[i] = length_of(val, M, i);
}
// d[i], src[i], and the check that makes the fill's walk end inside the text: src[i] + len[i] <= d[i]
__global__ void __launch_bounds__(TPB) k_check(const uint64_t *__restrict__ markPos, const uint8_t *__restrict__ mapOff, int offBytes,
                                               const uint64_t *__restrict__ len, const uint64_t *__restrict__ cum, uint64_t M,
                                               uint64_t *__restrict__ d, uint64_t *__restrict__ src, uint64_t *__restrict__ res) {
    const uint64_t stride = (uint64_t) gridDim.x * TPB;
    for (uint64_t i = (uint64_t) blockIdx.x * TPB + threadIdx.x; i < M; i += stride) {
        uint64_t di, s;
        if (!match_in_bounds(markPos, mapOff, offBytes, len, cum, i, di, s)) {
            atomicOr((unsigned long long *) &res[0], (unsigned long long) E_SOURCE);
            atomicMin((unsigned long long *) &res[1], (unsigned long long) i);
        }
        d[i] = di; src[i] = s;
    }
}

// ---- fill ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_restore_fill(Plan P, uint8_t *__restrict__ dst, const uint8_t *__restrict__ lut, uint32_t *__restrict__ deepest) {
    __shared__ uint8_t sl[256];
    __shared__ uint64_t sLo, sHi;
    sl[threadIdx.x] = lut[threadIdx.x];
    const uint64_t ntiles = (P.orgLen + TILE - 1) / TILE;
    uint32_t maxHops = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) {                                            // the matches that start inside the tile: [sLo, sHi)
            uint64_t lo, hi;
            matches_of_tile(P, tile, lo, hi);
            sLo = lo; sHi = hi;
        }
        __syncthreads();
        const uint64_t p0 = tile * TILE + (uint64_t) threadIdx.x * LANE;
        if (p0 >= P.orgLen) continue;
        restore_lane(P, sl, dst, p0, sLo, sHi, maxHops);
    }
    if (maxHops) atomicMax(deepest, maxHops);
}

static unsigned grid_for(uint64_t items, uint64_t perBlock) {
    const uint64_t blocks = (items + perBlock - 1) / perBlock;
    return (unsigned) std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 8192);
}

// uploads, plans, validates: 0, -4 (malformed, nothing of the maps was used as an address) or an error of the device
static int plan(State &S, hipStream_t st, const uint8_t *seq, uint64_t n, const uint8_t *mapOff, uint64_t mapOffLen, const uint8_t *mapLen,
                uint64_t mapLenLen, int offBytes, uint64_t *orgLen, uint64_t stats[4], double *kernelMs) {
    S.planned = false;
    *orgLen = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (kernelMs) *kernelMs = 0;
    if (offBytes != 0 && offBytes != 4 && offBytes != 8) return fail(-1, "the width of an rcMapOff entry is 4 or 8 bytes (or 0: the reference's rule), not %d", offBytes);
    if (n >= CAP) return fail(-103, "sequence too long");
    if (!S.ev0) { CCHK(hipEventCreate(&S.ev0)); CCHK(hipEventCreate(&S.ev1)); }
    int r;
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    if ((r = S.dCut.reserve(ntiles * TILE + CUT_PAD)) || (r = S.dMapOff.reserve(mapOffLen + 8)) || (r = S.dMapLen.reserve(mapLenLen + 8)) || (r = S.dLut.reserve(256)) ||
        (r = S.dCounts.reserve(ntiles + 1)) || (r = S.dTileOff.reserve(ntiles + 1)) || (r = S.dValIdx.reserve(mapLenLen + 1)) || (r = S.dRes.reserve(4)))
        return r;
    uint8_t lut[256];
    cm::complements_lut(lut);
    CCHK(hipMemcpyAsync(S.dLut.p, lut, 256, hipMemcpyHostToDevice, st));
    if (n) CCHK(hipMemcpyAsync(S.dCut.p, seq, n, hipMemcpyHostToDevice, st));
    CCHK(hipMemsetAsync(S.dCut.p + n, 0, ntiles * TILE + CUT_PAD - n, st));
    if (mapOffLen) CCHK(hipMemcpyAsync(S.dMapOff.p, mapOff, mapOffLen, hipMemcpyHostToDevice, st));
    if (mapLenLen) CCHK(hipMemcpyAsync(S.dMapLen.p, mapLen, mapLenLen, hipMemcpyHostToDevice, st));
    const uint64_t res0[4] = {0, SAT, 0, 0};                               // error bits, first match with a bad source
    CCHK(hipMemcpyAsync(S.dRes.p, res0, sizeof res0, hipMemcpyHostToDevice, st));
    CCHK(hipEventRecord(S.ev0, st));
    // ---- the marks, in order
    size_t t1 = 0, t2 = 0;
    CCHK(rocprim::exclusive_scan(nullptr, t1, S.dCounts.p, S.dTileOff.p, (uint64_t) 0, (size_t) ntiles + 1, rocprim::plus<uint64_t>(), st));
    auto ends = rocprim::make_transform_iterator(S.dMapLen.p, EndsValue());
    CCHK(rocprim::exclusive_scan(nullptr, t2, ends, S.dValIdx.p, (uint64_t) 0, (size_t) mapLenLen + 1, rocprim::plus<uint64_t>(), st));
    if ((r = S.dTmp.reserve(std::max(t1, t2) + 256))) return r;
    size_t tb;
    CCHK(hipMemsetAsync(S.dCounts.p, 0, (ntiles + 1) * sizeof(uint64_t), st));
    if (ntiles) k_mark_count<<<dim3(grid_for(ntiles, 1)), dim3(TPB), 0, st>>>(S.dCut.p, n, S.dCounts.p, ntiles);
    tb = S.dTmp.cap;
    CCHK(rocprim::exclusive_scan(S.dTmp.p, tb, S.dCounts.p, S.dTileOff.p, (uint64_t) 0, (size_t) ntiles + 1, rocprim::plus<uint64_t>(), st));
    uint64_t M = 0, nval = 0;
    CCHK(hipMemcpyAsync(&M, S.dTileOff.p + ntiles, 8, hipMemcpyDeviceToHost, st));
    // ---- the values of rcMapLen, numbered
    if (mapLenLen) {
        CCHK(hipMemsetAsync(S.dMapLen.p + mapLenLen, 0, 8, st));           // (a value's end behind the last byte: the scan's last entry counts all)
        tb = S.dTmp.cap;
        CCHK(rocprim::exclusive_scan(S.dTmp.p, tb, ends, S.dValIdx.p, (uint64_t) 0, (size_t) mapLenLen + 1, rocprim::plus<uint64_t>(), st));
        CCHK(hipMemcpyAsync(&nval, S.dValIdx.p + mapLenLen, 8, hipMemcpyDeviceToHost, st));
    }
    CCHK(hipStreamSynchronize(st));
    // ---- what the sizes alone decide
    if (M == 0 && mapOffLen) return fail(-4, "malformed rcMapOff: %llu bytes, and no mark in the sequence", (unsigned long long) mapOffLen);
    if (M && (mapOffLen % M || (mapOffLen / M != 4 && mapOffLen / M != 8)))
        return fail(-4, "malformed rcMapOff: %llu bytes for %llu marks (4 or 8 bytes each)", (unsigned long long) mapOffLen, (unsigned long long) M);
    const int width = M ? (int) (mapOffLen / M) : 0;
    if (M && offBytes && width != offBytes)
        return fail(-4, "malformed rcMapOff: %llu bytes for %llu marks of %d bytes each", (unsigned long long) mapOffLen, (unsigned long long) M, offBytes);
    if (mapLenLen == 0 && M) return fail(-4, "malformed rcMapLen: empty, and %llu marks in the sequence", (unsigned long long) M);
    if (mapLenLen && mapLen[mapLenLen - 1] >= 128) return fail(-4, "malformed rcMapLen: the last value does not end");
    if (mapLenLen && nval != M + 1)
        return fail(-4, "malformed rcMapLen: %llu values for the minimal length and %llu marks", (unsigned long long) nval, (unsigned long long) M);
    uint64_t total = 0, minLen = 0;
    if (mapLenLen) {
        if ((r = S.dMarkPos.reserve(M + 1)) || (r = S.dVal.reserve(M + 1)) || (r = S.dLen.reserve(M + 1)) || (r = S.dCum.reserve(M + 1)) ||
            (r = S.dD.reserve(M + 1)) || (r = S.dSrc.reserve(M + 1)))
            return r;
        CCHK(rocprim::exclusive_scan(nullptr, t1, S.dLen.p, S.dCum.p, (uint64_t) 0, (size_t) M + 1, SatAdd(), st));
        if ((r = S.dTmp.reserve(t1 + 256))) return r;                      // (nothing is in flight: the stream was waited for)
        if (M) k_mark_write<<<dim3(grid_for(ntiles, 1)), dim3(TPB), 0, st>>>(S.dCut.p, n, S.dTileOff.p, S.dMarkPos.p, M, ntiles);
        k_varint_decode<<<dim3(grid_for(mapLenLen, TPB)), dim3(TPB), 0, st>>>(S.dMapLen.p, mapLenLen, S.dValIdx.p, S.dVal.p, M + 1, S.dRes.p);
        k_lengths<<<dim3(grid_for(M + 1, TPB)), dim3(TPB), 0, st>>>(S.dVal.p, M, S.dLen.p);
        tb = S.dTmp.cap;
        CCHK(rocprim::exclusive_scan(S.dTmp.p, tb, S.dLen.p, S.dCum.p, (uint64_t) 0, (size_t) M + 1, SatAdd(), st));
        if (M) k_check<<<dim3(grid_for(M, TPB)), dim3(TPB), 0, st>>>(S.dMarkPos.p, S.dMapOff.p, width, S.dLen.p, S.dCum.p, M, S.dD.p, S.dSrc.p, S.dRes.p);
        CCHK(hipGetLastError());
        uint64_t res[4];
        CCHK(hipMemcpyAsync(res, S.dRes.p, sizeof res, hipMemcpyDeviceToHost, st));
        CCHK(hipMemcpyAsync(&total, S.dCum.p + M, 8, hipMemcpyDeviceToHost, st));
        CCHK(hipMemcpyAsync(&minLen, S.dVal.p, 8, hipMemcpyDeviceToHost, st));
        CCHK(hipEventRecord(S.ev1, st));
        CCHK(hipStreamSynchronize(st));
        if (res[0] & E_VARINT_LONG) return fail(-4, "malformed rcMapLen: a value of more than %d bytes", MAX_VARINT);
        if (minLen > UINT32_MAX) return fail(-4, "malformed rcMapLen: a minimal match length beyond 32 bits");
        if (total == SAT) return fail(-4, "malformed rcMapLen: the lengths add up beyond 64 bits");
        if (res[0] & E_SOURCE)
            return fail(-4, "malformed rcMapOff / rcMapLen: the source of match %llu does not end before the match starts", (unsigned long long) res[1]);
    } else {
        CCHK(hipEventRecord(S.ev1, st));
        CCHK(hipStreamSynchronize(st));
    }
    const uint64_t org = n - M + total;
    // MarkAndRemoveExactMatches wrote 4-byte offsets iff the uncut sequence had at most UINT32_MAX bytes (SimpleSequenceMatcher.cpp:103,:183)
    if (M && !offBytes && (width == 4) != (org <= UINT32_MAX))
        return fail(-4, "malformed rcMapOff: %d-byte offsets for a sequence of %llu bytes", width, (unsigned long long) org);
    if (kernelMs) { float ms = 0; CCHK(hipEventElapsedTime(&ms, S.ev0, S.ev1)); *kernelMs = ms; }
    S.n = n; S.M = M; S.orgLen = org; S.planned = true;
    *orgLen = org;
    if (stats) { stats[0] = M; stats[1] = total; stats[2] = 0; stats[3] = minLen; }
    return 0;
}

static int fill(State &S, hipStream_t st, int device, uint8_t *dstDev, uint64_t cap, uint8_t *dstHost, double *kernelMs, uint64_t *deepest) {
    if (kernelMs) *kernelMs = 0;
    if (deepest) *deepest = 0;
    if (!S.planned) return fail(-1, "no planned restore (mbgc_copmem_rc_restore_plan comes first)");
    if (cap < S.orgLen) return fail(-4, "the restored sequence has %llu bytes, the destination holds %llu", (unsigned long long) S.orgLen, (unsigned long long) cap);
    if (!dstDev && !dstHost) return fail(-1, "no destination");
    int r;
    if (dstDev) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dstDev) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
            (void) hipGetLastError();
            return fail(-1, "the destination is not memory of device %d", device);
        }
    } else {
        if ((r = S.dOut.reserve(S.orgLen + 64))) return r;
        dstDev = S.dOut.p;
    }
    if (S.orgLen) {
        Plan P = {S.dCut.p, S.dD.p, S.dSrc.p, S.dLen.p, S.dCum.p, S.M, S.n, S.orgLen};
        if (S.M == 0) {                                                    // no match: cum[0] is all the fill reads of the plan
            if ((r = S.dCum.reserve(1))) return r;
            P.cum = S.dCum.p;
            CCHK(hipMemsetAsync(S.dCum.p, 0, 8, st));
        }
        uint32_t *deep = (uint32_t *) (S.dRes.p + 2);
        CCHK(hipMemsetAsync(deep, 0, 8, st));
        CCHK(hipEventRecord(S.ev0, st));
        k_restore_fill<<<dim3(grid_for(S.orgLen, TILE)), dim3(TPB), 0, st>>>(P, dstDev, S.dLut.p, deep);
        CCHK(hipGetLastError());
        CCHK(hipEventRecord(S.ev1, st));
        uint64_t deepHost = 0;
        CCHK(hipMemcpyAsync(&deepHost, deep, 8, hipMemcpyDeviceToHost, st));
        if (dstHost) CCHK(hipMemcpyAsync(dstHost, dstDev, S.orgLen, hipMemcpyDeviceToHost, st));
        CCHK(hipStreamSynchronize(st));
        if (kernelMs) { float ms = 0; CCHK(hipEventElapsedTime(&ms, S.ev0, S.ev1)); *kernelMs = ms; }
        if (deepest) *deepest = deepHost & 0xFFFFFFFFu;
    }
    return 0;
}

}  // namespace cmr
