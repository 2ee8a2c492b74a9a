// Part of swsem_runtime.hip (one translation unit): the handle's state and the types that own its resources.
#define SWSEM_ESPEC (-100)   /* internal: a speculative finalize cannot be queued (it would need an ungated write) */

namespace {

thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(SWSEM_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

constexpr uint64_t REF_SHIFT = 1;          // SlidingWindowSparseEMMatcher.h:14
constexpr int SW_WIDTH_FACTOR = 16;        // .h:47
constexpr uint64_t REF_SLACK = 256;
constexpr uint64_t COPY_WGS = 2048;        // workgroups of the finalize's copies (a grid that is resident at once: k_copy_multi)
constexpr uint32_t EMIT_THIN_MAX = 512;    // emissions of at most this many chunks of 256 gap tasks run their byte automata with 16 tasks per wave
constexpr uint32_t RB_MIN = 2048 / RBU;    // shortest resolve block (units of RBU positions)
constexpr uint32_t CAND_MAX = 4096;        // rejected blocks of a batch k_stitch_replay replays ahead of the walk, at most (and at most CAND_BYTES of scratch)
constexpr uint64_t CAND_BYTES = 128ull << 20;
// dStats, zeroed per batch: [2] hits, [3] blocks replayed, [5..7] the stitch's walk (runs / one by one / jumped over; k_fingerprint, a test
// hook, later puts its three words at [4..6]), [8] candidates listed, [9] taken by the walk, [10] refused by it
constexpr int NSTATS = 16;

// The three kinds of resource a handle owns. Each frees what it holds when the handle is deleted (on the handle's
// device: swsem_destroy) and none can be copied.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if (p) (void) hipFree(p); }
    int reserve(size_t n) {
        if (n <= cap) return SWSEM_OK;
        if (p) (void) hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 8 + 64;
        if (hipMalloc((void **) &p, want * sizeof(T)) != hipSuccess) {
            p = nullptr;
            return fail(SWSEM_ENOMEM, "device allocation of %zu bytes failed", want * sizeof(T));
        }
        cap = want;
        return SWSEM_OK;
    }
};

// Page-locked host memory, grow-only. (Re)allocating it synchronises the whole device, so every user names the size it
// grows to (`want` bytes, generous: it must not recur in steady state), and has waited for whatever still uses the old block.
struct PinBuf : NoCopy {
    uint8_t *p = nullptr;
    size_t cap = 0;
    ~PinBuf() { if (p) (void) hipHostFree(p); }
    int reserve(size_t bytes, size_t want, unsigned flags = hipHostMallocCoherent | hipHostMallocMapped) {
        if (bytes <= cap) return SWSEM_OK;
        if (p) (void) hipHostFree(p);
        p = nullptr; cap = 0;
        if (hipHostMalloc((void **) &p, want, flags) != hipSuccess) {
            p = nullptr;
            return fail(SWSEM_ENOMEM, "cannot pin %zu B of host memory", want);
        }
        cap = want;
        return SWSEM_OK;
    }
};

// An event without timing, made with the handle (swsem_create looks at g_eventsFailed once the handle stands).
thread_local bool g_eventsFailed = false;
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    Event() { if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; g_eventsFailed = true; } }
    ~Event() { if (e) (void) hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

struct ProfEvent { hipEvent_t a, b; int fam; };

// The loader's scalar state (names follow SlidingWindowSparseEMMatcher.h:29-49,78): everything load_pieces,
// insert_samples, load_separator and the lock calls change. A speculative finalize that is not applied takes ALL of it
// back by assigning the copy made before it (emit_begin_impl) — a field the loader changes belongs here, nowhere else.
struct LoaderState {
    int64_t pos1 = REF_SHIFT;
    int laps = 0;                          // reachedRefLengthCount
    uint64_t samplingPos = 0, swEnd = 0;
    std::deque<uint64_t> locks;            // workersSwEndPositions
    uint32_t epoch = 1;
    uint32_t eCur = 0, ePrev = 0;          // first epoch of the current / previous lap (ht_value's staleness test)
    // the separator at the window's end (the byte before the loading position, when the loader stands at the window's
    // end) has been written with this value at this position in this lap: writing it again changes nothing
    int64_t sepEndPos = -1; int sepEndLaps = -1, sepEndVal = -1;
    bool pristine = true;                  // the loader has only moved forward (wraps included: told by epochs); false after swsem_set_position
    uint64_t droppedBytes = 0;             // extension bytes loadRef gave up at the window's end (.cpp:433: the rest of a text is dropped when the loader reaches swEnd)

    bool sep_end_done(int sep) const { return pos1 == sepEndPos && laps == sepEndLaps && sep == sepEndVal; }
    void sep_end_set(int64_t at, int sep) { sepEndPos = at; sepEndLaps = laps; sepEndVal = sep; }
    uint64_t refLength(uint64_t maxRefLength) const { return laps ? maxRefLength : (uint64_t) pos1; }
    // the loader has reached the buffer's end and the window lets it go on: the next lap begins (.cpp:404-409, :441-446)
    void wrap_if_at_end(uint64_t maxRefLength) {
        if ((uint64_t) pos1 != maxRefLength || swEnd == maxRefLength) return;
        laps++;
        ePrev = eCur; eCur = epoch;        // (entries of older laps are told by their epochs, ht_value)
        pos1 = REF_SHIFT;
        samplingPos = REF_SHIFT;
    }
};

// What the environment asks of a handle, read once (swsem_create). bench.py names the first four, the tests the next
// two; the last three are diagnostics.
struct Switches {
    bool seqResolve = false;               // SWSEM_RESOLVE=seq: one wave per contig (cross-check path)
    bool simt = true;                      // four chains per wave (k_resolve_blocks4); SWSEM_CHAINS=1: one chain per wave (k_resolve_blocks)
    uint32_t rbFixed = 0;                  // SWSEM_RB=n: resolve blocks of n * 1024 positions instead of the length chosen per batch
    int overlapFixed = -1;                 // SWSEM_OVERLAP=n: n warm-up positions in front of every resolve block, not adapted (-1: adapted, take_counts)
    uint32_t profMask = ~0u;               // families that get event brackets (SWSEM_PROF_FAMS: every bracket is two markers in the queue)
    int metaWarm = swk::MWARM;             // warm-up matches of the pairing chain's speculative blocks (SWSEM_META_WARM: fewer, so that blocks fail)
    bool lapTags = true;                   // SWSEM_LAP_TAGS=0: every stale entry is visited (the table image and the results are the same)
    int tagSumShift = 12;                  // SWSEM_TAGSUM_SHIFT=n: one summary entry per 2^n sampling slots (RefView::tagSum); 0: no summary
    bool streamCalib = true;               // SWSEM_STREAM_CALIB=0: no measurement, the side streams in the order they were made
    bool streamDebug = false;              // SWSEM_STREAM_DEBUG: prints the deal of the side streams
    bool debugStats = false;               // SWSEM_DEBUG_STATS: the stitch's and the pairing chain's counters at swsem_destroy
};
Switches read_switches() {
    Switches s;
    if (const char *e = getenv("SWSEM_RESOLVE")) s.seqResolve = strcmp(e, "seq") == 0;
    if (const char *e = getenv("SWSEM_CHAINS")) s.simt = atoi(e) != 1;
    if (const char *e = getenv("SWSEM_RB")) { int x = atoi(e); if (x >= 1 && x <= 256) s.rbFixed = (uint32_t) x * (1024 / RBU); }
    if (const char *e = getenv("SWSEM_OVERLAP")) { int x = atoi(e); if (x >= 0 && x <= swk::OVERLAP_MAX) s.overlapFixed = x; }
    if (const char *e = getenv("SWSEM_PROF_FAMS")) s.profMask = (uint32_t) strtoul(e, nullptr, 0);
    if (const char *e = getenv("SWSEM_META_WARM")) s.metaWarm = std::min(swk::MWARM, std::max(0, atoi(e)));
    if (const char *e = getenv("SWSEM_LAP_TAGS")) s.lapTags = atoi(e) != 0;
    if (const char *e = getenv("SWSEM_TAGSUM_SHIFT")) { int x = atoi(e); if (x >= 0 && x <= 24) s.tagSumShift = x; }
    if (const char *e = getenv("SWSEM_STREAM_CALIB")) s.streamCalib = atoi(e) != 0;
    s.streamDebug = getenv("SWSEM_STREAM_DEBUG") != nullptr;
    s.debugStats = getenv("SWSEM_DEBUG_STATS") != nullptr;
    return s;
}

// what prepare_inserts has uploaded for the launches that follow (launch_inserts)
struct PreparedInserts {
    size_t np = 0, nc = 0, nb = 0, ne = 0, ns = 0;
    const SumRun *dSums = nullptr;
    bool beside = false;
    uint64_t nSamples = 0, nEdge = 0, copyBlocks = 0;
    const InsertPiece *dPieces = nullptr, *dEdge = nullptr;
    const uint64_t *dFirst = nullptr, *dCFirst = nullptr, *dEFirst = nullptr;
    const CopyPiece *dCopies = nullptr;
    const BytePiece *dBytes = nullptr;
};

// One of the two emissions in flight: the second phase of one batch can still be running while the next is begun.
struct EmitSlot {
    DevBuf<EmitContig> dECg;
    DevBuf<EmitOut> dEOut;
    DevBuf<int> dEWhich;
    DevBuf<uint32_t> dEOwner, dESpanOwner;
    DevBuf<EMatch> dEM;
    DevBuf<uint64_t> dENext0, dELoaded, dEPack;
    DevBuf<uint64_t> dERawLp, dERawNext0;  // per stitched row: the source regions looked up beside pass 1 (k_emit_regions_raw)
    DevBuf<uint8_t> dERm, dEArena;
    DevBuf<uint32_t> dEKeep, dEMeta, dECorr, dESz, dEOfs, dEChunk;
    DevBuf<MetaRec> dEStates;
    DevBuf<unsigned long long> dEStat, dEPm, dELit, dEBad;
    DevBuf<LongCopy> dELong;
    DevBuf<uint32_t> dELongCount;
    bool statZeroed = false;
    std::vector<EmitContig> ecg;
    std::vector<uint32_t> chunkOwner, spanOwner;
    std::vector<int> ewhich;
    std::vector<uint64_t> eloaded;
    std::vector<EmitOut> eout;
    Event evDone;
    Event evMetaDone;                    // behind the pairing kernels (the byte automata wait for it)
    bool outstanding = false, refGuarded = false;
    bool donePending = false;            // evDone has not been recorded for this emission yet (its byte automata are queued behind the speculative finalize)
    // the byte automata of the second phase wait to be queued: at the next batch's resolve launch, gated on that kernel's
    // start (run_phase2b), or by whoever needs this emission's results first
    bool deferred2b = false, waitFin2b = false;
    EmitView v2b; uint32_t grid2b = 0; int n2b = 0;
    const uint8_t *qdev = nullptr;       // query buffer the emission reads
    swsem_emit_params_t params;          // its parameters
    uint64_t emitPos1 = 0;               // loading position the emission started at
    uint64_t lockMin = UINT64_MAX;       // lowest matching-lock position of its contigs (UINT64_MAX: some contig had none)
    int emitLaps = 0;                    // laps of the buffer when it started
    int emitN = 0;
    PinBuf pinE;                         // the second phase's results (EmitOut per contig)
    // The streams on the host: page-locked (the copy runs at the link's rate and nothing is zero-filled).
    // Two host buffers per slot, used in turn: the views of an emission (swsem_emit_view) stay valid while the NEXT emission
    // of the same slot is begun, runs and is taken — a caller that copies the bytes out on a thread of its own has two
    // emissions' time for it, not the gap between taking one emission and beginning the next (mgmp_driver.cpp: the large
    // literal and flag streams of divergent collections, 0.4 bytes per base, were waited for there).
    PinBuf hostHalf[2];
    int hostAt = 0;
    PinBuf &hostStreams() { return hostHalf[hostAt]; }
    // the other half (this one may still be read through the views of the slot's last emission), grown to n bytes
    int next_host_streams(size_t n) { hostAt ^= 1; return hostStreams().reserve(n, n + n / 2 + 4096, hipHostMallocDefault); }
    std::vector<uint64_t> hostStreamOff; // [k * NSTREAMS + s] offset into hostStreams()
    bool hostStreamsValid = false;
    uint64_t packedBytes = 0;
};

}  // namespace

struct swsem {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    Switches sw;
    // --- reference state
    uint8_t *ref = nullptr;                // start1
    ht_entry *ht = nullptr;
    uint8_t *lut = nullptr;                // upper-complement LUT, utils/helper.cpp:312-338
    uint16_t *tags = nullptr;              // per sampling slot: lap_tag of its last on-grid sampling (swsem_device.h, lap_want)
    bool useTags = true;                   // (not with an odd k1, not with SWSEM_LAP_TAGS=0)
    // The summary of tags[] (RefView::tagSum): tagSumEntries entries, one per 2^tagSumShift sampling slots; null: none. Only the
    // device holds it. The host never needs an entry's old value: whatever a loader step touches gets a new one from the step's
    // own piece arithmetic (note_piece, note_bytes), and the runs collected here leave with the step's tables (prepare_inserts)
    // to be written behind the same gate as the tag writes they describe (k_set_tagsum).
    uint16_t *tagSum = nullptr;
    int tagSumShift = 0;
    uint32_t tagSumEntries = 0;
    struct SumSpan { uint64_t a, b; uint32_t val; };   // coarse blocks [a, b) -> val
    std::vector<SumSpan> sumUniform, sumMixed;
    std::vector<SumRun> sumRuns;           // plan_tag_summary's result for the flush being prepared
    LoaderState ld;
    uint64_t maxRefLength = 0;
    int L = 0, K = 0, k1 = 0, skipMargin = 0, k1ord = 0;
    uint32_t hash_size = 0, mask = 0;
    uint64_t swSize = 0;
    bool circular = true;
    int fpBits = 0;                        // fingerprint bits of a table entry
    uint64_t hostProbes = 0;               // query positions of the batch
    bool deferInserts = false;             // collect the insertion phases of a finalize call into one launch
    bool specMode = false;                 // a speculative finalize is being queued: nothing may be written outside its gated launches
    DevBuf<uint32_t> dGate;
    DevBuf<uint8_t> dPred;
    std::vector<InsertPiece> pendingPieces;
    std::vector<InsertPiece> edgePieces;   // prepare_inserts: the samples left to the launch behind the copies
    // the insertion hashes from the copies' sources, the copies run beside it on streamLoad
    int prioLow = 0, prioHigh = 0;         // the device's stream priority range
    Event evLoadFork, evLoadDone;
    std::vector<CopyPiece> pendingCopies;    // ... and its byte writes: device-to-device copies,
    std::vector<BytePiece> pendingBytes;     // then single bytes (separators), each list in program order
    DevBuf<uint64_t> dTables;                // one upload: insert pieces, their prefix, copy pieces, their prefix, bytes
    // pinned staging for that upload (two, used in turn); reused once its copy has completed
    struct HostTab { PinBuf buf; Event ev; bool pending = false; } hostTables[2];
    int hostTableSel = 0;
    PreparedInserts prep;
    // the side streams, dealt from the device's pool (deal_streams) and never destroyed: the byte automata of an emission's
    // second phase; the finalize's copies; table uploads; the pairing kernels
    hipStream_t stream2 = nullptr, streamLoad = nullptr, streamUp = nullptr, streamAux = nullptr;
    Event evTables, evRoundTop;
    bool roundTopFresh = false;            // evRoundTop was recorded by the batch this emission belongs to (run_batch), not an older one
    // --- per-round scratch
    DevBuf<uint8_t> stage;                 // host text / host query staging
    DevBuf<Contig> dContigs;
    DevBuf<uint32_t> dMatchCount, dRbContig, dRbOrder;
    std::vector<uint32_t> rbOrderHost, rbOrderKey;   // the table on the device is kept while the batches keep their shape (rbOrderKey)
    uint32_t chainsPerWave = 1;            // of the last batch
    hipStream_t stream3 = nullptr;         // device-to-host copies of emitted streams (end_slot): made when first needed (see s3)
    hipStream_t s3() {
        if (!stream3 && hipStreamCreateWithFlags(&stream3, hipStreamNonBlocking) != hipSuccess) stream3 = stream;
        return stream3;
    }
    Event evMatched;                       // chains of the last batch done
    std::vector<uint32_t> rbContigHost;
    DevBuf<Match> dMatches;
    DevBuf<Row> dRegions, dReplay;
    DevBuf<BlockRec> dRecs;
    DevBuf<FastRec> dFast;
    // the rejected blocks replayed ahead of the stitch's walk (k_stitch_pre lists them, k_stitch_replay runs them): block -> slot,
    // slot -> block, every slot's result and its rows
    DevBuf<uint32_t> dCandOf, dCandBlock;
    DevBuf<CandRec> dCand;
    DevBuf<Row> dCandArea;
    DevBuf<uint32_t> dSegStart, dKeepN, dDstOff;
    DevBuf<int32_t> dPrev;
    DevBuf<unsigned long long> dStats;
    DevBuf<uint8_t> dDecode;                 // contigs given back by the device decoder (swsem_emit_verify)
    DevBuf<DecodeJob> dJobs;
    DevBuf<DecRec> dDecRecs;                 // the plan pass's records, contig after contig (swsem_decode.hip)
    DevBuf<DecPlanOut> dDecPlan;
    DevBuf<uint64_t> dDecAux;                // per contig: record base (n + 1), first differing byte (n), malformed flag (n, as u32 pairs)
    // --- the decoder's side (swsem_create_decoder): a reference buffer, no table; the chained plan of a collection
    bool decoder = false;
    struct ChainState {
        DevBuf<ChainStart> dStarts;
        DevBuf<ChainContig> dContigs;
        DevBuf<uint32_t> dSeqCount, dChainBad, dBad;
        DevBuf<uint64_t> dLock, dRecBase;
        DevBuf<LoadSeg> dSegs;
        DevBuf<ProvRow> dProv;               // the closure of a selection: provenance table, per-contig times, need bitmap
        DevBuf<uint64_t> dTime;
        DevBuf<uint32_t> dNeed;
        DevBuf<ProvRowG> dProvG;             // the closure of --region: rows that name the owner's bytes, the granule bitmap, its prefix offsets
        DevBuf<uint32_t> dNeedG;
        DevBuf<uint64_t> dGranBase;
        uint32_t granShift = 0;              // log2 of the granule; regionFor: the plan (its contig count) the bitmap was made for, 0 = none
        uint64_t regionFor = 0;
        ChainStreams streams = {};
        swsem_emit_params_t params = {};
        uint64_t n = 0;                      // contigs planned
        std::vector<uint64_t> nrec, destLen, litEnd, lock;
        const uint8_t *jobsDest = nullptr;   // dJobs has been filled for this destination
    } chain;
    // --- emission
    EmitSlot slot[2];
    int latest = 0;                          // slot of the last swsem_emit_batch_begin
    // largest request seen so far: a slot is always sized for it, so the second slot does not regrow (= hipFree +
    // hipMalloc, a device-wide stall) the first time it meets a full-size batch
    uint64_t capN = 0, capRows = 0, capArena = 0, capLoaded = 0, capChunks = 0;
    int selected = -1;                       // slot the result calls read (-1: the latest), swsem_emit_select
    EmitSlot &sel() { return slot[selected < 0 ? latest : selected]; }
    // pinned landing zone for everything a batch hands back to the host (queue_counts)
    PinBuf pin; size_t pinExtraAt = 0;
    // small host tables travel through a pinned ring: an asynchronous copy from pageable memory is staged by the
    // runtime and can block the calling thread for milliseconds when its staging pool is busy
    PinBuf ring; size_t ringAt = 0;
    // emission in two phases: pass 1 (what the extension policy needs) on `stream`, the rest on `stream2` behind evP1,
    // so that the caller can queue the round's finalize and the next round's match-finding next to it
    Event evP1;
    Event evFin;                           // behind the speculative finalize (see emit_begin_impl)
    Event evMeta;                          // behind the last emission's k_emit_meta_spec
    Event evRegions;                       // behind k_emit_regions_raw (k_emit_p1_compact waits for it)
    bool metaPending = false;
    bool emitHostCopy = true;              // copy the streams to the host inside swsem_emit_batch
    // Warm-up positions of a speculative block chain (at most OVERLAP_MAX): a chain started from the empty state falls into step with the
    // true one after a few emissions, and how many positions that takes depends on the collection (on how far apart its matches
    // lie). Too short and many blocks are rejected (replayed by k_stitch_replay, and by the stitch's walk itself where they follow each other);
    // too long and every block scans positions twice. Adapted from the share of rejected blocks the last full batch reported
    // (take_counts) unless SWSEM_OVERLAP fixes it: the results never depend on it.
    uint32_t overlap = 1024, batchBlocks = 0, batchCands = 0;
    uint32_t rb = 8;                       // length of a resolve block in units of RBU positions: chosen per batch (batch_layout) unless SWSEM_RB fixes it
    // over the handle's life: resolve blocks replayed / accepted in runs / tested one by one / jumped over / replayed ahead of the walk
    // (candidates) / of those taken by the walk / refused by it and replayed in place; [7] the most candidates one batch had (SWSEM_DEBUG_STATS)
    uint64_t stitchDiag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t slotPercent = 95;             // share of the wave slots a launch's blocks are sized for (80 %: +5 % on the 4.35e9-byte sizing, -3 % on configs[2]'s)
    uint32_t waveSlots = 256 * 4 * RESOLVE_WAVES_PER_SIMD;   // resolve waves the device holds at once (CUs x SIMDs x waves)
    std::vector<Contig> contigs;
    std::vector<uint32_t> matchCount;
    std::vector<swsem_match_t> hostMatches;
    const uint8_t *qdev = nullptr;         // query buffer of the last batch
    uint32_t minLen = 0;
    bool batchValid = false;
    uint64_t stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // --- profiling
    bool prof = false;
    std::deque<ProfEvent> events;
    double profMs[SWSEM_K_COUNT] = {0};
    uint64_t profN[SWSEM_K_COUNT] = {0};

    CopySegs segs;                         // small copies staged for one launch (stage_copy / flush_copies)
    hipStream_t segStream = nullptr;

    uint64_t refLength() const { return ld.refLength(maxRefLength); }
    RefView view() const {
        RefView v;
        v.ref = ref; v.ht = ht; v.pos1 = (uint64_t) ld.pos1; v.refLength = refLength(); v.maxRefLength = maxRefLength;
        v.mask = mask; v.fpBits = fpBits; v.fpCheck = (fpBits && ld.pristine) ? (ld.laps ? 2 : 1) : 0; v.eCur = ld.eCur; v.ePrev = ld.ePrev;
        // (position << k1ord) + K + 1 <= pos1  <=>  value <= curMax;   (position << k1ord) >= pos1  <=>  value >= prevMin
        v.curMax = ld.pos1 >= (int64_t) K + 1 ? (uint32_t) (((uint64_t) ld.pos1 - K - 1) >> k1ord) : 0u;
        v.prevMin = (uint32_t) ((((uint64_t) ld.pos1) + (1ull << k1ord) - 1) >> k1ord); v.K = K; v.k1ord = k1ord; v.skipMargin = skipMargin; v.minLen = minLen;
        v.tagSum = useTags ? tagSum : nullptr; v.tagSumShift = tagSumShift;
        v.tags = useTags ? tags : nullptr; v.tagCur = swk::lap_tag(ld.laps); v.tagPrev = ld.laps ? swk::lap_tag(ld.laps - 1) : 0u;
        return v;
    }
    // event pairs are recycled: creating events by the hundred makes the runtime grow its signal pool now and
    // then, which can stall the calling thread in the middle of a measurement
    std::vector<ProfEvent> idle;
    void account(const ProfEvent &e) {
        float ms = 0;
        (void) hipEventElapsedTime(&ms, e.a, e.b);
        profMs[e.fam] += ms; profN[e.fam]++;
        idle.push_back(e);
    }
    void mark(int fam, bool begin, hipStream_t on = nullptr) {
        if (!prof || !((sw.profMask >> fam) & 1u)) return;
        if (!on) on = stream;
        if (begin) {
            while (events.size() > 1 && hipEventQuery(events.front().b) == hipSuccess) {   // harvest what has finished
                account(events.front());
                events.pop_front();
            }
            ProfEvent e;
            if (!idle.empty()) { e = idle.back(); idle.pop_back(); }
            else { (void) hipEventCreate(&e.a); (void) hipEventCreate(&e.b); }
            e.fam = fam;
            (void) hipEventRecord(e.a, on);
            events.push_back(e);
        } else
            (void) hipEventRecord(events.back().b, on);
    }
    void drain_events() {
        for (auto &e : events) {
            (void) hipEventSynchronize(e.b);
            account(e);
        }
        events.clear();
    }
    // (the buffers and events above free themselves; what is left are the four exact-size allocations and the timing pairs)
    ~swsem() {
        for (void *p : {(void *) ref, (void *) tags, (void *) tagSum, (void *) ht, (void *) lut}) if (p) (void) hipFree(p);
        drain_events();
        for (auto &e : idle) { (void) hipEventDestroy(e.a); (void) hipEventDestroy(e.b); }
    }
};
