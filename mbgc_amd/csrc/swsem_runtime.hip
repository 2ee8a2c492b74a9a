// Host runtime + C ABI (include/mbgc_swsem.h) of the MI355X match-finding path.
// The host keeps exactly the scalar state the reference keeps in SlidingWindowSparseEMMatcher
// (pos1, reachedRefLengthCount, samplingPos, swEnd, the worker-lock deque); the reference bytes,
// the hash table and every per-round intermediate live in HBM.
// One translation unit: the kernels, then the runtime's parts in the order they build on each other, then the C ABI.
#include "../../include/mbgc_swsem.h"
#include "swsem_kernels.hip"
#include "swsem_resolve4.hip"
#include "swsem_emit.hip"
#include "swsem_decode.hip"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

using namespace swk;

#include "swsem_runtime_state.h"      // the handle: loader state, owned buffers and events, switches
#include "swsem_runtime_streams.h"    // side-stream pool and dealing
#include "swsem_runtime_loader.h"     // staged copies, loader, insertion, finalize
#include "swsem_runtime_match.h"      // match batch
#include "swsem_runtime_emit.h"       // emission and the speculative finalize
#include "swsem_runtime_decode.h"     // decoder driver

namespace {

// initParams, SlidingWindowSparseEMMatcher.cpp:74-104
void init_params(swsem *h) {
    const int L = h->L;
    if (L > 110) h->K = 56;
    else if (L > 62) h->K = 44;
    else if (L > 53) h->K = 40;
    else if (L > 46) h->K = 36;
    else if (L > 42) h->K = 32;
    else if (L > 32) h->K = 28;
    else h->K = (L / 4 - 1) * 4;
    const int KmmL = (L / 4 - 1) * 4;
    if (KmmL < h->K) h->K = KmmL;
    uint8_t i = 24;
    do {
        h->hash_size = ((uint32_t) 1) << (i++);
    } while (i <= 31 && h->hash_size < h->maxRefLength / (uint64_t) h->k1);
    h->mask = h->hash_size - 1;
    h->fpBits = 10;                        // of the K-mer's second hash (swsem_device.h, fp_step); 22 bits are left for the epoch
}

void build_lut(uint8_t *lut) {
    for (int i = 0; i < 256; i++) lut[i] = (uint8_t) i;
    lut[127] = 0;   // the reference's table constructor stops at i < CHAR_MAX, utils/helper.cpp:321-322
    const char *from = "AaCcGgTtNnUuYyRrKkMmBbDdHhVvWwSs";
    const char *to = "TTGGCCAANNAARRYYMMKKVVHHDDBBSSWW";
    for (int i = 0; from[i]; i++) lut[(uint8_t) from[i]] = (uint8_t) to[i];
}

}  // namespace

// a decoder's handle (swsem_create_decoder) has a reference buffer and nothing of the matcher
#define MATCHER_ONLY(h) do { if ((h)->decoder) return fail(SWSEM_EINVAL, "%s: the handle is a decoder's (swsem_create_decoder): it has no hash table", __func__); } while (0)

extern "C" {

const char *swsem_last_error(void) { return g_err.c_str(); }

int swsem_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int swsem_device_numa_node(int device) {
    char bus[64] = {0};
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count ||
        hipDeviceGetPCIBusId(bus, (int) sizeof bus, device) != hipSuccess) {
        (void) hipGetLastError();                                      // (a failed query must not be the next launch's "last error")
        return -1;
    }
    for (char *c = bus; *c; c++) *c = (char) tolower((unsigned char) *c);
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

int swsem_create(swsem_t **out, uint64_t maxRefLength, int L, int k1, int k2, int skipMargin, int device) {
    *out = nullptr;
    if (k1 <= 0) return fail(SWSEM_EINVAL, "s - reference sampling step - should be a positive integer.");   // MBGC_Params.h:593-597
    if (k2 != 1) return fail(SWSEM_EINVAL, "k2 = %d unsupported (MBGC always uses k2 = 1, MGMP_Params.h:202)", k2);
    if (L < 16) return fail(SWSEM_EINVAL, "Error: Minimal matching length too short!");
    if (maxRefLength < 64 || (maxRefLength >> __builtin_ctz((unsigned) k1)) >= (1ull << 32))
        return fail(SWSEM_EINVAL, "reference length limit %llu out of range", (unsigned long long) maxRefLength);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
        return fail(SWSEM_ENODEV, "no HIP device %d (the HIP path has no CPU fallback)", device);
    HIPCHK(hipSetDevice(device));
    g_eventsFailed = false;
    swsem *h = new swsem();                                 // (its events are made here, on this device)
    h->device = device;
    if (g_eventsFailed) { swsem_destroy(h); return fail(SWSEM_EHIP, "hipEventCreate failed"); }
    h->sw = read_switches();                                // every environment switch of the library: see Switches
    if (h->sw.overlapFixed >= 0) h->overlap = (uint32_t) h->sw.overlapFixed;
    h->maxRefLength = maxRefLength;
    h->L = L; h->k1 = k1; h->skipMargin = skipMargin;
    h->k1ord = __builtin_ctz((unsigned) k1);
    h->ld.swEnd = maxRefLength;
    h->swSize = maxRefLength / SW_WIDTH_FACTOR;
    init_params(h);
    // an even k1: SlidingWindowExpSparseEMMatcher — entries hold position >> ctz(k1), sampling starts at k1 (.cpp:494-503); an odd
    // one: the base class (MGMP.cpp:170-176) — htEncodePos / htDecodePos are the identity (.h:74-76: k1ord = 0 here), sampling
    // starts at REF_SHIFT (.h:78), which is also where a wrap puts it back, so the off-grid samples of the Exp variant do not occur
    h->ld.samplingPos = (k1 % 2) ? REF_SHIFT : (uint64_t) k1;
    // (with an odd k1 a lap tag per sampling slot would be two bytes per reference byte: stale entries are visited instead, same results)
    h->useTags = h->k1ord != 0 && h->sw.lapTags;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { swsem_destroy(h); return fail(SWSEM_EHIP, "hipStreamCreate failed"); }
    h->ownStream = true;
    int least = 0, greatest = 0;                            // numerically: least >= greatest
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess) { h->prioLow = least; h->prioHigh = greatest; }
    { int d = deal_streams(h); if (d) { swsem_destroy(h); return d; } }
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) h->waveSlots = (uint32_t) pr.multiProcessorCount * 4u * RESOLVE_WAVES_PER_SIMD; }
    const size_t nSlots = (size_t) ((maxRefLength + REF_SLACK) >> h->k1ord) + 2;
    // the summary of the tags (RefView::tagSum); its kernels take k1 for a slot's length, so only where k1 is a power of two
    h->tagSumShift = h->useTags && k1 == (1 << h->k1ord) ? h->sw.tagSumShift : 0;
    h->tagSumEntries = h->tagSumShift ? (uint32_t) (((nSlots - 1) >> h->tagSumShift) + 1) : 0u;
    if (hipMalloc((void **) &h->ref, maxRefLength + REF_SLACK) != hipSuccess ||
        (h->useTags && hipMalloc((void **) &h->tags, nSlots * sizeof(uint16_t)) != hipSuccess) ||
        (h->tagSumEntries && hipMalloc((void **) &h->tagSum, (size_t) h->tagSumEntries * sizeof(uint16_t)) != hipSuccess) ||
        hipMalloc((void **) &h->ht, (size_t) h->hash_size * sizeof(ht_entry)) != hipSuccess ||
        hipMalloc((void **) &h->lut, 256) != hipSuccess) {
        swsem_destroy(h);
        return fail(SWSEM_ENOMEM, "cannot allocate %llu B reference + %llu B hash table in HBM",
                    (unsigned long long) maxRefLength, (unsigned long long) h->hash_size * 8ull);
    }
    uint8_t lut[256];
    build_lut(lut);
    HIPCHK(hipMemcpy(h->lut, lut, 256, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(h->ht, 0, (size_t) h->hash_size * sizeof(ht_entry), h->stream));
    if (h->tags) HIPCHK(hipMemsetAsync(h->tags, 0, nSlots * sizeof(uint16_t), h->stream));
    if (h->tagSum) HIPCHK(hipMemsetAsync(h->tagSum, 0xFF, (size_t) h->tagSumEntries * sizeof(uint16_t), h->stream));   // TAGSUM_MIXED: nothing is claimed yet
    // start1[0] = 0 (.cpp:335); the rest of the buffer is written before it is ever read, the slack
    // past the end is zeroed because the reference's own reads run a few bytes over (:224, ENC:337)
    // the whole buffer starts out as zeros (the reference reads — harmlessly — bytes it has not loaded yet, e.g. the one at the
    // loading position in extendMatchRight; left as allocated they would be whatever an earlier process had there)
    HIPCHK(hipMemsetAsync(h->ref, 0, maxRefLength, h->stream));
    HIPCHK(hipMemsetAsync(h->ref + maxRefLength, 0, REF_SLACK, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h;
    return SWSEM_OK;
}

void swsem_destroy(swsem_t *h) {
    if (!h) return;
    (void) hipSetDevice(h->device);
    for (auto &E : h->slot) E.deferred2b = false;                    // (automata that were never queued: nobody wants their bytes any more)
    for (hipStream_t s : {h->stream, h->stream2, h->stream3, h->streamUp, h->streamAux, h->streamLoad}) if (s) (void) hipStreamSynchronize(s);
    h->drain_events();
    if (h->sw.debugStats) {                                          // diagnostics: the stitch's and the pairing chain's counters of this handle
        fprintf(stderr, "swsem stitch: blocks replayed %llu, accepted in runs %llu, tested one by one %llu, jumped over %llu\n",
                (unsigned long long) h->stitchDiag[0], (unsigned long long) h->stitchDiag[1], (unsigned long long) h->stitchDiag[2], (unsigned long long) h->stitchDiag[3]);
        fprintf(stderr, "swsem stitch: replayed ahead of the walk %llu, taken %llu, refused and replayed in place %llu, most in one batch %llu, warm-up positions at the end %u\n",
                (unsigned long long) h->stitchDiag[4], (unsigned long long) h->stitchDiag[5], (unsigned long long) h->stitchDiag[6], (unsigned long long) h->stitchDiag[7], h->overlap);
        uint64_t t[8];
        if (swsem_debug_emit_stats(h, t) == SWSEM_OK && (t[4] | t[5] | t[6] | t[7]))
            fprintf(stderr, "swsem pairing chain: foreign-boundary steps %llu, blocks not accepted %llu, groups replayed %llu, blocks given up %llu\n",
                    (unsigned long long) t[4], (unsigned long long) t[5], (unsigned long long) t[6], (unsigned long long) t[7]);
    }
    if (h->stream3) (void) hipStreamDestroy(h->stream3);             // (the side streams are the pool's: never destroyed)
    if (h->ownStream && h->stream) (void) hipStreamDestroy(h->stream);
    delete h;                                                        // every buffer and event it owns goes with it
}

int swsem_set_stream(swsem_t *h, void *s) { MATCHER_ONLY(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->ownStream) (void) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t) s;
    h->ownStream = false;
    return deal_streams(h);                                           // (another main stream, maybe another pipe)
}
int swsem_synchronize(swsem_t *h) { HIPCHK(hipStreamSynchronize(h->stream)); return SWSEM_OK; }

void swsem_disable_sliding_window(swsem_t *h) { h->swSize = 0; h->ld.swEnd = h->circular ? 0 : h->maxRefLength; }
void swsem_set_sliding_window_size(swsem_t *h, int f) { h->swSize = h->maxRefLength / (uint64_t) (uint8_t) f; }
void swsem_disable_circular_buffer(swsem_t *h) { h->circular = false; h->ld.swEnd = h->maxRefLength; }
uint64_t swsem_get_ref_length(const swsem_t *h) { return h->refLength(); }
uint64_t swsem_get_loading_position(const swsem_t *h) { return (uint64_t) h->ld.pos1; }
uint64_t swsem_get_loaded_ref_length(const swsem_t *h) { return loaded_ref_length(h); }
uint64_t swsem_get_max_ref_length(const swsem_t *h) { return h->maxRefLength; }
uint64_t swsem_get_dropped_bytes(const swsem_t *h) { return h->ld.droppedBytes; }
uint64_t swsem_get_sliding_window_size(const swsem_t *h) { return h->circular ? h->swSize : 0; }
void swsem_set_position(swsem_t *h, uint64_t p, int laps) { h->ld.pos1 = (int64_t) p; h->ld.laps = laps; h->ld.pristine = false; }
int swsem_get_K(const swsem_t *h) { return h->K; }
uint32_t swsem_get_hash_size(const swsem_t *h) { return h->hash_size; }

// acquireWorkerMatchingLockPos, .cpp:361-378
uint64_t swsem_acquire_lock(swsem_t *h) {
    if (h->swSize == 0 || !h->circular) return h->ld.swEnd;
    uint64_t w = (uint64_t) h->ld.pos1 + h->swSize;
    if (h->ld.laps || w > h->maxRefLength) {
        if (w > h->maxRefLength) w -= h->maxRefLength - REF_SHIFT;
    } else
        w = h->maxRefLength;
    if (h->ld.locks.empty()) h->ld.swEnd = w;
    h->ld.locks.push_back(w);
    return w;
}

int swsem_release_lock(swsem_t *h, uint64_t v) { MATCHER_ONLY(h); return release_lock(h, v); }

int swsem_load_ref_dev(swsem_t *h, const uint8_t *t, uint64_t len, int loadRC, int addSep, int sep) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    int r = load_pieces(h, t, len, false, addSep != 0, sep);
    if (r) return r;
    if (loadRC) r = load_pieces(h, t, len, true, addSep != 0, sep);
    return r;
}

int swsem_load_ref(swsem_t *h, const uint8_t *t, uint64_t len, int loadRC, int addSep, int sep) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    if (len == 0) return SWSEM_OK;
    int r = h->stage.reserve(len + 64);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(h->stage.p, t, len, hipMemcpyHostToDevice, h->stream));
    r = swsem_load_ref_dev(h, h->stage.p, len, loadRC, addSep, sep);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(h->stream));   // the staging buffer is reused by the next call
    return SWSEM_OK;
}
int swsem_load_separator(swsem_t *h, int sep) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    return load_separator(h, sep);
}

int swsem_finalize_targets(swsem_t *h, int n, const uint8_t *const *ext_dev, const uint64_t *ext_len, int addSep, int sep,
                           int lazySeparator, const uint64_t *lockPos, uint64_t *loadedAfter) { MATCHER_ONLY(h);
    return finalize_impl(h, n, ext_dev, ext_len, addSep, sep, lazySeparator, lockPos, loadedAfter, nullptr);
}

int swsem_match_batch_dev(swsem_t *h, const uint8_t *q, const uint64_t *offsets, int n, uint32_t minLen, const uint64_t *lockPos) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    return run_batch(h, q, offsets, n, minLen, lockPos);
}

int swsem_batch_counts(swsem_t *h, uint64_t *nm) { MATCHER_ONLY(h);
    if (!h->batchValid) return fail(SWSEM_EINVAL, "no batch results");
    if (h->matchCount.size() != h->contigs.size()) { int r = fetch_counts(h); if (r) return r; }
    for (size_t c = 0; c < h->contigs.size(); c++) nm[c] = h->matchCount[c];
    return SWSEM_OK;
}

int swsem_batch_matches(swsem_t *h, int c, swsem_match_t *out, uint64_t cap) { MATCHER_ONLY(h);
    if (!h->batchValid || c < 0 || c >= (int) h->contigs.size()) return fail(SWSEM_EINVAL, "no such contig in the batch");
    if (h->matchCount.size() != h->contigs.size()) { int r = fetch_counts(h); if (r) return r; }
    const uint64_t n = std::min<uint64_t>(cap, h->matchCount[c]);
    if (n) HIPCHK(hipMemcpy(out, h->dMatches.p + h->contigs[c].matchBase, n * sizeof(Match), hipMemcpyDeviceToHost));
    return SWSEM_OK;
}

int swsem_batch_fingerprint(swsem_t *h, uint64_t *fp, uint64_t *tot, uint64_t *len) { MATCHER_ONLY(h);
    if (!h->batchValid) return fail(SWSEM_EINVAL, "no batch results");
    k_fingerprint<<<1, 1, 0, h->stream>>>(h->dContigs.p, (int) h->contigs.size(), h->dMatches.p, h->dMatchCount.p, h->dStats.p + 4);
    unsigned long long o[3];
    HIPCHK(hipMemcpyAsync(o, h->dStats.p + 4, sizeof o, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *fp = o[0]; *tot = o[1]; *len = o[2];
    h->stats[3] = o[1]; h->stats[4] = o[2];
    return SWSEM_OK;
}

int swsem_match(swsem_t *h, const uint8_t *query, uint64_t len, uint32_t minLen, uint64_t lockPos,
                const swsem_match_t **matches, uint64_t *nmatches) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    *matches = nullptr; *nmatches = 0;
    int r = swsem_emit_batch_end(h);                   // an emission still running reads the staged query
    if (r) return r;
    if ((r = h->stage.reserve(len + 64))) return r;
    if (len) HIPCHK(hipMemcpyAsync(h->stage.p, query, len, hipMemcpyHostToDevice, h->stream));
    const uint64_t offs[2] = {0, len};
    if ((r = run_batch(h, h->stage.p, offs, 1, minLen, &lockPos))) return r;
    if ((r = fetch_counts(h))) return r;
    h->hostMatches.resize(h->matchCount[0]);
    if (h->matchCount[0])
        HIPCHK(hipMemcpy(h->hostMatches.data(), h->dMatches.p, h->matchCount[0] * sizeof(Match), hipMemcpyDeviceToHost));
    *matches = h->hostMatches.data();
    *nmatches = h->matchCount[0];
    return SWSEM_OK;
}

// plain device-memory helpers so that host code above this ABI needs no HIP headers
int swsem_dev_malloc(swsem_t *h, uint64_t bytes, void **out) {
    HIPCHK(hipSetDevice(h->device));
    *out = nullptr;
    if (hipMalloc(out, bytes ? bytes : 1) != hipSuccess) return fail(SWSEM_ENOMEM, "device allocation of %llu bytes failed", (unsigned long long) bytes);
    return SWSEM_OK;
}
int swsem_dev_free(swsem_t *h, void *p) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (p) HIPCHK(hipFree(p));
    return SWSEM_OK;
}
int swsem_dev_upload(swsem_t *h, void *dst_dev, const void *src, uint64_t bytes) {
    HIPCHK(hipSetDevice(h->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SWSEM_OK;
}
int swsem_dev_download(swsem_t *h, void *dst, const void *src_dev, uint64_t bytes) {
    HIPCHK(hipSetDevice(h->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SWSEM_OK;
}
int swsem_dev_copy(swsem_t *h, void *dst_dev, const void *src_dev, uint64_t bytes) {
    HIPCHK(hipSetDevice(h->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, h->stream));
    return SWSEM_OK;
}

// PgHelpers::upperReverseComplement on device buffers (utils/helper.cpp:405-410): lets the caller build a
// target's extension string "contig + RC(contig)" (MGMP.cpp:389-398) without leaving HBM.
int swsem_revcomp_dev(swsem_t *h, const uint8_t *src_dev, uint64_t n, uint8_t *dst_dev) {
    HIPCHK(hipSetDevice(h->device));
    if (n == 0) return SWSEM_OK;
    const uint64_t thr = (n + 3) / 4;
    const unsigned blocks = (unsigned) std::min<uint64_t>((thr + 255) / 256, 8192);
    h->mark(SWSEM_K_LOAD, true);
    k_load_rc<<<dim3(blocks), dim3(256), 0, h->stream>>>(src_dev, dst_dev, n, h->lut);
    h->mark(SWSEM_K_LOAD, false);
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}

int swsem_debug_copy_ref(swsem_t *h, uint64_t from, uint64_t n, uint8_t *out) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->ref + from, n, hipMemcpyDeviceToHost));
    return SWSEM_OK;
}

int swsem_debug_write_ref(swsem_t *h, uint64_t from, uint64_t n, const uint8_t *in) { MATCHER_ONLY(h);
    if (from + n > h->maxRefLength) return fail(SWSEM_EINVAL, "swsem_debug_write_ref: beyond the buffer");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->stream2));
    HIPCHK(hipMemcpy(h->ref + from, in, n, hipMemcpyHostToDevice));
    {   // the bytes of these slots changed without a sample: their tags say so
        const uint64_t s0 = from >= (uint64_t) h->K ? (from - h->K + 1) >> h->k1ord : 0, s1 = (from + n + ((1ull << h->k1ord) - 1)) >> h->k1ord;
        if (h->tags && s1 > s0) HIPCHK(hipMemset(h->tags + s0, 0, (s1 - s0) * sizeof(uint16_t)));
        if (h->tagSum && s1 > s0) {
            const uint64_t b0 = s0 >> h->tagSumShift, b1 = std::min<uint64_t>(((s1 - 1) >> h->tagSumShift) + 1, h->tagSumEntries);
            if (b1 > b0) HIPCHK(hipMemset(h->tagSum + b0, 0xFF, (b1 - b0) * sizeof(uint16_t)));
        }
    }
    return SWSEM_OK;
}

int swsem_debug_copy_ht(swsem_t *h, uint32_t *out) { MATCHER_ONLY(h);
    DevBuf<uint32_t> tmp;
    int r = tmp.reserve(h->hash_size);
    if (r) return r;
    k_ht_low_words<<<dim3((h->hash_size + 255) / 256), dim3(256), 0, h->stream>>>(h->ht, tmp.p, h->hash_size, h->fpBits);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, tmp.p, (size_t) h->hash_size * 4, hipMemcpyDeviceToHost));
    return SWSEM_OK;
}

// diagnostics: the lap tags (one per sampling slot) and their summary (one entry per 2^shift slots, 0xFFFF: mixed) as the device
// holds them behind everything queued on the main stream. *n: how many there are (cap of them are copied at most); a handle
// without tags, or without a summary, reports 0.
int swsem_debug_tags(swsem_t *h, uint16_t *out, uint64_t cap, uint64_t *n) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    *n = h->tags ? ((h->maxRefLength + REF_SLACK) >> h->k1ord) + 2 : 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (std::min(cap, *n)) HIPCHK(hipMemcpy(out, h->tags, std::min(cap, *n) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return SWSEM_OK;
}
int swsem_debug_tag_summary(swsem_t *h, uint16_t *out, uint64_t cap, uint64_t *n, int *shift) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    *n = h->tagSum ? h->tagSumEntries : 0;
    *shift = h->tagSum ? h->tagSumShift : 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (std::min(cap, *n)) HIPCHK(hipMemcpy(out, h->tagSum, std::min(cap, *n) * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return SWSEM_OK;
}

// diagnostics: per resolve block of the last batch {ticks, candidates visited, rows on the stack}
int swsem_debug_block_times(swsem_t *h, uint64_t *out, uint64_t cap, uint64_t *n) { MATCHER_ONLY(h);
    uint64_t nb = 0;
    for (auto &c : h->contigs) nb += c.nrb;
    *n = nb;
    if (nb > cap) nb = cap;
    std::vector<BlockRec> tmp(nb);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nb) HIPCHK(hipMemcpy(tmp.data(), h->dRecs.p, nb * sizeof(BlockRec), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nb; i++) { out[3 * i] = tmp[i].cycles; out[3 * i + 1] = tmp[i].visits; out[3 * i + 2] = tmp[i].emits; }
    return SWSEM_OK;
}

// counters of the emission's pairing chain since the handle was made, summed over the emission slots:
// out[4] steps that went by an inherited boundary other than the match's own, out[5] blocks of the speculative pass that were
// not accepted, out[6] groups of 64 matches the stitch replayed, out[7] blocks given up for too many inherited boundaries
int swsem_debug_emit_stats(swsem_t *h, uint64_t out[8]) { MATCHER_ONLY(h);
    HIPCHK(hipDeviceSynchronize());
    for (int k = 0; k < 8; k++) out[k] = 0;
    for (auto &E : h->slot) {
        if (!E.dEStat.p || !E.statZeroed) continue;
        unsigned long long t[8];
        HIPCHK(hipMemcpy(t, E.dEStat.p, sizeof t, hipMemcpyDeviceToHost));
        for (int k = 0; k < 8; k++) out[k] += t[k];
    }
    return SWSEM_OK;
}

#ifdef SWSEM_DIAG_PHASES
// diagnostics build only: phase sums of every resolve launch since the last call (g_diag), then reset
int swsem_debug_phases(swsem_t *h, uint64_t *out) {
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long z[8] = {0};
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(swk::g_diag), sizeof z));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(swk::g_diag), z, sizeof z));
    return SWSEM_OK;
}
#endif

int swsem_profile_enable(swsem_t *h, int on) {
    h->drain_events();
    h->prof = on != 0;
    memset(h->profMs, 0, sizeof h->profMs);
    memset(h->profN, 0, sizeof h->profN);
    return SWSEM_OK;
}

int swsem_profile_get(swsem_t *h, double ms[SWSEM_K_COUNT], uint64_t n[SWSEM_K_COUNT]) {
    h->drain_events();
    for (int i = 0; i < SWSEM_K_COUNT; i++) { ms[i] = h->profMs[i]; n[i] = h->profN[i]; }
    return SWSEM_OK;
}

int swsem_batch_stats(swsem_t *h, uint64_t s[9]) { MATCHER_ONLY(h);
    if (!h->batchValid) return fail(SWSEM_EINVAL, "no batch results");
    for (int i = 0; i < 9; i++) s[i] = h->stats[i];
    return SWSEM_OK;
}

void swsem_emit_params_default(swsem_emit_params_t *p, int mode) {
    memset(p, 0, sizeof(*p));
    p->enableExtensionsWithMismatches = 1;
    p->mismatchesWithExclusion = 1;
    p->lazyDecompressionSupport = 1;
    p->enable40bitReference = 0;
    p->frugal64bitLenEncoding = 1;
    p->gapDepthOffsetEncoding = 64;                     // MBGC_Params.h:51
    p->gapDepthMismatchesEncoding = 2;                  // :52
    p->gapBreakingMatchMinLength = 256;                 // :53
    p->mmsMatchBonus = 50;                              // initMismatchesMatchingScoreParams, :92-97
    p->mmsMismatchPenalty = 50;
    p->mmsMismatchesScoreThreshold = 500;
    p->mmsMismatchesInitialScore = 125;
    p->allowedTargetsOutrunForDissimilarContigs = 1;    // MGMP_Params.h:60
    p->minimalLengthForDissimilarContigs = 1024;        // :64
    p->unmatchedFractionFactorTweakForDissimilarContigs = 16;   // :61
    if (mode == 0) {                                    // MBGC_Params.h:893-902
        p->allowedTargetsOutrunForDissimilarContigs = 4;
        p->unmatchedFractionFactorTweakForDissimilarContigs = 32;
        p->frugal64bitLenEncoding = 0;
    }
    if (mode == 2) {                                    // :903-906
        p->allowedTargetsOutrunForDissimilarContigs = 0;
        p->unmatchedFractionFactorTweakForDissimilarContigs = 2;
    }
}

int swsem_emit_batch_begin(swsem_t *h, const swsem_emit_params_t *p, int n, const int *contigIdx, const uint64_t *lockPos,
                           const int *factor, const int64_t *processed, const int64_t *targetIdx,
                           const uint64_t *refExtLoadedPos, uint64_t nLoaded) { MATCHER_ONLY(h);
    return emit_begin_impl(h, p, n, contigIdx, lockPos, factor, processed, targetIdx, refExtLoadedPos, nLoaded, nullptr, nullptr);
}

int swsem_emit_batch_begin_spec(swsem_t *h, const swsem_emit_params_t *p, int n, const int *contigIdx, const uint64_t *lockPos,
                                const int *factor, const int64_t *processed, const int64_t *targetIdx,
                                const uint64_t *refExtLoadedPos, uint64_t nLoaded, const swsem_spec_finalize_t *spec, int *applied) { MATCHER_ONLY(h);
    return emit_begin_impl(h, p, n, contigIdx, lockPos, factor, processed, targetIdx, refExtLoadedPos, nLoaded, spec, applied);
}

// waits for every emission still in its second phase (oldest first); afterwards their streams can be fetched
int swsem_emit_batch_end(swsem_t *h) { MATCHER_ONLY(h);
    int r = end_slot(h, h->latest ^ 1);
    return r ? r : end_slot(h, h->latest);
}

// result calls read the latest emission (previous = 0) or the one before it (previous = 1), which may have been
// left running across the next swsem_emit_batch_begin
int swsem_emit_select(swsem_t *h, int previous) { MATCHER_ONLY(h);
    h->selected = previous ? (h->latest ^ 1) : -1;
    return SWSEM_OK;
}

int swsem_emit_batch(swsem_t *h, const swsem_emit_params_t *p, int n, const int *contigIdx, const uint64_t *lockPos,
                     const int *factor, const int64_t *processed, const int64_t *targetIdx,
                     const uint64_t *refExtLoadedPos, uint64_t nLoaded) { MATCHER_ONLY(h);
    int r = swsem_emit_batch_begin(h, p, n, contigIdx, lockPos, factor, processed, targetIdx, refExtLoadedPos, nLoaded);
    return r ? r : swsem_emit_batch_end(h);
}

void swsem_emit_set_host_copy(swsem_t *h, int on) { h->emitHostCopy = on != 0; }

// unmatchedChars (the return value of processMatches, SWSEM_SKIPPED when skipped) of every result
int swsem_emit_unmatched(swsem_t *h, uint64_t *unmatched) { MATCHER_ONLY(h);
    EmitSlot &E = h->slot[h->latest];
    for (size_t k = 0; k < E.eout.size(); k++) unmatched[k] = E.eout[k].unmatchedChars;
    return SWSEM_OK;
}

// The arena is written packed — every stream of the last emit batch back to back, (result, stream)
// major — so handing it on is one device-to-device copy.
int swsem_emit_pack_dev(swsem_t *h, uint8_t *dst_dev, uint64_t cap, uint64_t *sizes, uint64_t *total) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    EmitSlot &E = h->sel();
    { int e = end_slot(h, (int) (&E - h->slot)); if (e) return e; }
    if (sizes)
        for (size_t k = 0; k < E.eout.size(); k++)
            for (int st = 0; st < SWSEM_NSTREAMS; st++) sizes[k * SWSEM_NSTREAMS + st] = E.eout[k].size[st];
    if (dst_dev && E.packedBytes) {
        if (E.packedBytes > cap) return fail(SWSEM_EINVAL, "swsem_emit_pack_dev: buffer too small");
        // on the emission's own stream, and waited for: the consumer may be on any stream, and the main stream
        // may already hold the next round's match-finding
        HIPCHK(hipMemcpyAsync(dst_dev, E.dEArena.p, E.packedBytes, hipMemcpyDeviceToDevice, h->s3()));
        HIPCHK(hipStreamSynchronize(h->s3()));
    }
    if (total) *total = E.packedBytes;
    return SWSEM_OK;
}

int swsem_emit_pack_dev_on(swsem_t *h, uint8_t *dst_dev, uint64_t cap, void *stream) { MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    EmitSlot &E = h->sel();
    { int e = end_slot(h, (int) (&E - h->slot)); if (e) return e; }       // (the emission has finished: its event was waited for)
    if (!E.packedBytes) return SWSEM_OK;
    if (!dst_dev || E.packedBytes > cap) return fail(SWSEM_EINVAL, "swsem_emit_pack_dev_on: buffer too small");
    HIPCHK(hipMemcpyAsync(dst_dev, E.dEArena.p, E.packedBytes, hipMemcpyDeviceToDevice, stream ? (hipStream_t) stream : h->stream));
    return SWSEM_OK;
}

int swsem_emit_counters(swsem_t *h, uint64_t *out) { MATCHER_ONLY(h);
    EmitSlot &E = h->sel();
    { int e = end_slot(h, (int) (&E - h->slot)); if (e) return e; }
    for (size_t k = 0; k < E.eout.size(); k++) {
        const EmitOut &o = E.eout[k];
        const uint64_t v[6] = {o.unmatchedChars, o.extMatched, o.extMismatches, o.totalMatched, o.removed, o.nmatches};
        memcpy(out + k * 6, v, sizeof v);
    }
    return SWSEM_OK;
}

int swsem_emit_result(swsem_t *h, int k, swsem_streams_t *out) { MATCHER_ONLY(h);
    EmitSlot &E = h->sel();
    { int e = end_slot(h, (int) (&E - h->slot)); if (e) return e; }
    if (k < 0 || k >= (int) E.eout.size()) return fail(SWSEM_EINVAL, "swsem_emit_result: no result %d", k);
    if (!E.hostStreamsValid) {
        { int r = E.next_host_streams(E.packedBytes + 1); if (r) return r; }
        if (E.packedBytes) HIPCHK(hipMemcpyAsync(E.hostStreams().p, E.dEArena.p, E.packedBytes, hipMemcpyDeviceToHost, h->s3()));
        HIPCHK(hipStreamSynchronize(h->s3()));
        E.hostStreamsValid = true;
    }
    const EmitOut &o = E.eout[k];
    for (int st = 0; st < SWSEM_NSTREAMS; st++) {
        out->data[st] = E.hostStreams().p + E.hostStreamOff[(size_t) k * SWSEM_NSTREAMS + st];
        out->size[st] = o.size[st];
    }
    out->unmatchedChars = o.unmatchedChars;
    out->extensionsMatchedChars = o.extMatched;
    out->extensionsMismatches = o.extMismatches;
    out->totalMatched = o.totalMatched;
    out->removedGapBreakingMatches = o.removed;
    out->nmatches = o.nmatches;
    return SWSEM_OK;
}

int swsem_decode_contigs_dev(swsem_t *h, const swsem_emit_params_t *p, int n, const swsem_decode_job_t *jobs, uint64_t *destLen, int64_t *unmatched) {
    HIPCHK(hipSetDevice(h->device));
    if (n <= 0) return SWSEM_OK;
    std::vector<DecodeJob> jb(n);
    for (int k = 0; k < n; k++) {
        for (int st = 0; st < SWSEM_NSTREAMS; st++) { jb[k].stream[st] = jobs[k].stream_dev[st]; jb[k].size[st] = jobs[k].size[st]; }
        jb[k].refLockPos = jobs[k].refLockPos; jb[k].dest = jobs[k].dest_dev; jb[k].destCap = jobs[k].destCap; jb[k].expect = nullptr;
    }
    std::vector<DecodeOut> outs;
    int r = decode_jobs(h, p, n, jb, outs);
    if (r) return r;
    for (int k = 0; k < n; k++) { destLen[k] = outs[k].destLen; unmatched[k] = outs[k].unmatched; }
    return SWSEM_OK;
}

int swsem_create_decoder(swsem_t **out, uint64_t maxRefLength, int device) {
    *out = nullptr;
    if (maxRefLength < 64) return fail(SWSEM_EINVAL, "reference length limit %llu out of range", (unsigned long long) maxRefLength);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
        return fail(SWSEM_ENODEV, "no HIP device %d (the HIP path has no CPU fallback)", device);
    HIPCHK(hipSetDevice(device));
    g_eventsFailed = false;
    swsem *h = new swsem();
    h->device = device;
    h->decoder = true;
    if (g_eventsFailed) { swsem_destroy(h); return fail(SWSEM_EHIP, "hipEventCreate failed"); }
    h->maxRefLength = maxRefLength;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { swsem_destroy(h); return fail(SWSEM_EHIP, "hipStreamCreate failed"); }
    h->ownStream = true;
    if (hipMalloc((void **) &h->ref, maxRefLength + REF_SLACK) != hipSuccess || hipMalloc((void **) &h->lut, 256) != hipSuccess) {
        swsem_destroy(h);
        return fail(SWSEM_ENOMEM, "cannot allocate %llu B reference in HBM", (unsigned long long) maxRefLength);
    }
    uint8_t lut[256];
    build_lut(lut);
    HIPCHK(hipMemcpy(h->lut, lut, 256, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(h->ref, 0, maxRefLength + REF_SLACK, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h;
    return SWSEM_OK;
}

int swsem_decode_plan_chain_dev(swsem_t *h, const swsem_emit_params_t *p, const uint8_t *const stream_dev[SWSEM_NSTREAMS], const uint64_t size[SWSEM_NSTREAMS],
                                int nstarts, const swsem_chain_start_t *starts, int ntargets, const uint32_t *seqCount, const uint64_t *lockPos,
                                uint64_t ncontigs, swsem_chain_contig_t *out, int *firstBadChain) {
    HIPCHK(hipSetDevice(h->device));
    if (nstarts <= 0 || ntargets <= 0 || !firstBadChain) return fail(SWSEM_EINVAL, "swsem_decode_plan_chain_dev: no chain start");
    ChainStreams S;
    for (int st = 0; st < SWSEM_NSTREAMS; st++) { S.p[st] = stream_dev[st]; S.n[st] = size[st]; }
    return decode_plan_chain(h, p, S, nstarts, starts, ntargets, seqCount, lockPos, ncontigs, out, firstBadChain);
}

int swsem_decode_fill_range_dev(swsem_t *h, uint64_t c0, uint64_t c1, uint8_t *dest_dev, const uint64_t *destOff, uint64_t *nbad) {
    HIPCHK(hipSetDevice(h->device));
    int r = decode_fill_range(h, c0, c1, dest_dev, destOff);
    if (r || !nbad) return r;
    std::vector<uint32_t> bad(c1 - c0);
    if (c1 > c0) HIPCHK(hipMemcpyAsync(bad.data(), h->chain.dBad.p + c0, (c1 - c0) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *nbad = 0;
    for (uint32_t b : bad) *nbad += b != 0;
    return SWSEM_OK;
}

int swsem_decode_closure_dev(swsem_t *h, uint64_t refTotalLength, uint64_t nrows, const swsem_prov_row_t *rows, uint64_t ncontigs, const uint64_t *timeOf,
                             uint64_t nunits, const swsem_fill_unit_t *units, uint32_t *need) {
    HIPCHK(hipSetDevice(h->device));
    if (!h->decoder) return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: the handle is no decoder's (swsem_create_decoder)");
    if (!timeOf || !need || (nrows && !rows) || (nunits && !units)) return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: a table is missing");
    return decode_closure(h, refTotalLength, nrows, rows, ncontigs, timeOf, nunits, units, need);
}

int swsem_decode_closure_region_dev(swsem_t *h, uint64_t refTotalLength, uint64_t nrows, const swsem_prov_row_region_t *rows, uint64_t ncontigs, const uint64_t *timeOf,
                                    uint64_t nunits, const swsem_fill_unit_t *units, uint32_t granuleShift, const uint64_t *granBase, uint32_t *needGranules,
                                    uint32_t *needContigs, uint64_t *filledBases) {
    HIPCHK(hipSetDevice(h->device));
    if (!h->decoder) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: the handle is no decoder's (swsem_create_decoder)");
    if (!timeOf || !granBase || !needGranules || !needContigs || (nrows && !rows) || (nunits && !units)) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: a table is missing");
    return decode_closure_region(h, refTotalLength, nrows, rows, ncontigs, timeOf, nunits, units, granuleShift, granBase, needGranules, needContigs, filledBases);
}

int swsem_decode_fill_region_dev(swsem_t *h, uint64_t c0, uint64_t c1, uint8_t *dest_dev, const uint64_t *destOff, uint64_t *nbad) {
    HIPCHK(hipSetDevice(h->device));
    int r = decode_fill_range(h, c0, c1, dest_dev, destOff, true);
    if (r || !nbad) return r;
    std::vector<uint32_t> bad(c1 - c0);
    if (c1 > c0) HIPCHK(hipMemcpyAsync(bad.data(), h->chain.dBad.p + c0, (c1 - c0) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *nbad = 0;
    for (uint32_t b : bad) *nbad += b != 0;
    return SWSEM_OK;
}

int swsem_debug_copy_records(swsem_t *h, uint64_t contig, swsem_decode_record_t *out, uint64_t cap, uint64_t *n) {
    HIPCHK(hipSetDevice(h->device));
    if (!h->decoder || !n || (cap && !out)) return fail(SWSEM_EINVAL, "swsem_debug_copy_records: a decoder's handle, a count and a buffer");
    return decode_copy_records(h, contig, out, cap, n);
}

int swsem_decode_load_dev(swsem_t *h, const uint8_t *src_dev, int n, const swsem_load_seg_t *segs) {
    HIPCHK(hipSetDevice(h->device));
    return decode_load(h, src_dev, n, segs);
}

int swsem_emit_verify(swsem_t *h, int *nbad, int *firstBad, uint64_t *firstDiff) {
    MATCHER_ONLY(h);
    HIPCHK(hipSetDevice(h->device));
    EmitSlot &E = h->sel();
    { int e = end_slot(h, (int) (&E - h->slot)); if (e) return e; }
    const int n = (int) E.eout.size();
    *nbad = 0; if (firstBad) *firstBad = -1; if (firstDiff) *firstDiff = UINT64_MAX;
    if (n == 0) return SWSEM_OK;
    uint64_t total = 0;
    for (int k = 0; k < n; k++) total += E.ecg[k].n + 16;
    int r;
    if ((r = h->dDecode.reserve(total))) return r;
    std::vector<DecodeJob> jb;
    std::vector<int> which;
    uint64_t at = 0;
    for (int k = 0; k < n; k++) {
        if (E.eout[k].unmatchedChars == UINT64_MAX) { at += E.ecg[k].n + 16; continue; }   // given up as dissimilar: nothing was emitted
        DecodeJob j;
        for (int st = 0; st < SWSEM_NSTREAMS; st++) { j.stream[st] = E.dEArena.p + E.hostStreamOff[(size_t) k * SWSEM_NSTREAMS + st]; j.size[st] = E.eout[k].size[st]; }
        j.refLockPos = E.ecg[k].lock; j.dest = h->dDecode.p + at; j.destCap = E.ecg[k].n; j.expect = E.qdev + E.ecg[k].qoff;
        at += E.ecg[k].n + 16;
        jb.push_back(j); which.push_back(k);
    }
    if (jb.empty()) return SWSEM_OK;
    std::vector<DecodeOut> outs;
    if ((r = decode_jobs(h, &E.params, (int) jb.size(), jb, outs))) return r;
    for (size_t i = 0; i < jb.size(); i++) {
        const int k = which[i];
        const bool ok = outs[i].unmatched >= 0 && outs[i].destLen == E.ecg[k].n && outs[i].firstDiff == UINT64_MAX &&
                        (uint32_t) outs[i].unmatched == (uint32_t) E.eout[k].unmatchedChars;
        if (!ok) {
            if (*nbad == 0) { if (firstBad) *firstBad = k; if (firstDiff) *firstDiff = outs[i].unmatched < 0 ? outs[i].destLen : outs[i].firstDiff; }
            (*nbad)++;
        }
    }
    return SWSEM_OK;
}

int swsem_emit(swsem_t *h, const swsem_emit_params_t *p, int contig, uint64_t lockPos, int factor, int64_t processed,
               int64_t targetIdx, const uint64_t *loaded, uint64_t nLoaded, swsem_streams_t *out) { MATCHER_ONLY(h);
    int r = swsem_emit_batch(h, p, 1, &contig, &lockPos, &factor, &processed, &targetIdx, loaded, nLoaded);
    if (r) return r;
    return swsem_emit_result(h, 0, out);
}

}  // extern "C"
