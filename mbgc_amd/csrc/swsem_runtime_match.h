// Part of swsem_runtime.hip: one batch of match-finding (resolve, stitch, gather) and its counts' way back to the host.
namespace {

// Launch order of the resolve blocks (h->contigs filled in). The genomes of a collection resemble each other, so the
// blocks that scan the same offsets of a round's contigs look up the same buckets and compare against the same
// reference windows. Workgroups are dealt round-robin over the eight XCDs (slot s -> XCD s mod 8, MI355X_MICROARCH.md
// "Workgroup dispatch": observed, for speed only) and each XCD has its own L2: such a group of blocks is given
// consecutive slots of ONE XCD, so one of them fetches a sector from HBM and the others find it in that L2. Groups
// larger than 64 blocks are cut (a batch of many one-block contigs must still spread over the chip), every piece goes
// to the XCD with the shortest list so far, and the lists are padded to one length with empty slots.
bool build_resolve_order(swsem *h, uint32_t rblocks, uint32_t per) {
    std::vector<uint32_t> key;
    key.reserve(h->contigs.size() + 3);
    key.push_back(rblocks); key.push_back(per);
    for (auto &cg : h->contigs) key.push_back(cg.nrb);
    if (key == h->rbOrderKey && !h->rbOrderHost.empty()) return false;       // same shape as the last batch: the device table stands
    h->rbOrderKey.swap(key);
    std::vector<uint32_t> &order = h->rbOrderHost;
    order.clear();
    uint32_t maxNrb = 0;
    for (auto &cg : h->contigs) maxNrb = std::max(maxNrb, cg.nrb);
    // contigs by descending block count: the contigs that still have a block at offset b are a prefix
    std::vector<uint32_t> byLen(h->contigs.size());
    for (uint32_t c = 0; c < byLen.size(); c++) byLen[c] = c;
    std::stable_sort(byLen.begin(), byLen.end(), [&](uint32_t a, uint32_t b) { return h->contigs[a].nrb > h->contigs[b].nrb; });
    std::vector<uint32_t> lists[8];                                          // wave slots (per block ids each) of every XCD
    std::vector<uint32_t> grp;
    size_t alive = byLen.size();
    const size_t piece = 64;                                                 // blocks of one offset kept together on an XCD
    for (uint32_t b = 0; b < maxNrb; b++) {
        while (alive && h->contigs[byLen[alive - 1]].nrb <= b) alive--;
        grp.assign(byLen.begin(), byLen.begin() + alive);
        if (!std::is_sorted(grp.begin(), grp.end())) std::sort(grp.begin(), grp.end());   // contig order inside a group
        for (size_t i = 0; i < grp.size(); i += piece) {
            int best = 0;
            for (int x = 1; x < 8; x++) if (lists[x].size() < lists[best].size()) best = x;
            const size_t e = std::min(grp.size(), i + piece);
            for (size_t k = i; k < e; k++) lists[best].push_back(h->contigs[grp[k]].rb0 + b);
            while (lists[best].size() % per) lists[best].push_back(0xFFFFFFFFu);          // the last wave of the piece may run fewer chains
        }
    }
    size_t len = 0;
    for (auto &l : lists) len = std::max(len, l.size() / per);
    order.assign(len * 8 * per, 0xFFFFFFFFu);
    for (int x = 0; x < 8; x++)
        for (size_t j = 0; j < lists[x].size() / per; j++)
            for (uint32_t k = 0; k < per; k++) order[(j * 8 + x) * per + k] = lists[x][j * per + k];
    return true;
}

struct BatchShape {
    uint64_t matchRows = 0, bases = 0, probes = 0;
    uint32_t rblocks = 0;                  // resolve blocks of the batch
    uint32_t rslots = 0;                   // waves of the resolve launch (batch_upload: the launch order's length)
    uint32_t cap = 0;                      // rows a block chain can hold: disjoint matches, each containing the K-mer of a distinct visited hit
    bool blocks = false;                   // resolve blocks, stitch and gather (not one wave per contig)
    uint32_t cands = 0;                    // slots of the replays ahead of the walk (k_stitch_replay's grid)
};

// Step 1, host arithmetic only: the block length of this batch, h->contigs and the block -> contig table.
int batch_layout(swsem *h, const uint64_t *offsets, int n, uint32_t minLen, const uint64_t *lockPos, BatchShape &B) {
    h->contigs.assign(n, Contig());
    std::vector<uint32_t> &rbContig = h->rbContigHost;   // uploaded asynchronously
    rbContig.clear();
    // Block chains are latency-bound and a launch lasts as long as its slowest wave: the blocks are sized so
    // that all of them are resident at once and there are as many as that allows.
    // Fewer, longer blocks leave wave slots empty; more of them run in two generations and lengthen the
    // sequential stitch. At least 2048 positions: a small batch (one target of the sequential schedule) fills few wave slots
    // whatever the block length, and then short chains are what is fast (the warm-up positions per 2048 of its own).
    uint64_t allUnits = 0;                          // in units of RBU positions
    for (int c = 0; c < n; c++) {
        const uint64_t len = offsets[c + 1] - offsets[c];
        allUnits += len >= (uint64_t) h->K ? (len - h->K + 1 + RBU - 1) / RBU : 0;
    }
    h->chainsPerWave = (h->sw.simt && !h->sw.seqResolve && h->K <= K_MAX4) ? (uint32_t) GC : 1u;
    const uint64_t waves = h->chainsPerWave > 1 ? (uint64_t) h->waveSlots / RESOLVE_WAVES_PER_SIMD * RESOLVE4_WAVES_PER_SIMD : h->waveSlots;
    const uint64_t slots = std::max<uint64_t>(1, waves * h->chainsPerWave * h->slotPercent / 100);
    h->rb = h->sw.rbFixed ? h->sw.rbFixed : (uint32_t) std::min<uint64_t>(65536 / RBU, std::max<uint64_t>(RB_MIN, (allUnits + slots - 1) / slots));   // (a small batch — one target of the sequential schedule — runs short chains: it is their length that takes the time)
    for (int c = 0; c < n; c++) {
        Contig &cg = h->contigs[c];
        cg.qoff = offsets[c];
        cg.n = offsets[c + 1] - offsets[c];
        // query positions are 32-bit signed in the resolve automaton (and uint32 in processMatches, MBGC_Encoder.cpp:145)
        if (cg.n >= (1ull << 31) - (1ull << 20)) return fail(SWSEM_EINVAL, "contig %d longer than 2^31 - 2^20 bytes", c);
        cg.lock = lockPos ? lockPos[c] : UINT64_MAX;
        const uint64_t npos = cg.n >= (uint64_t) h->K ? cg.n - h->K + 1 : 0;
        B.probes += npos;
        cg.matchBase = B.matchRows;
        B.matchRows += cg.n / minLen + 2;
        cg.rb0 = B.rblocks;
        cg.nrb = (uint32_t) ((npos + (uint64_t) h->rb * RBU - 1) / ((uint64_t) h->rb * RBU));
        for (uint32_t t = 0; t < cg.nrb; t++) rbContig.push_back((uint32_t) c);
        B.rblocks += cg.nrb;
        B.bases += cg.n;
    }
    B.blocks = !h->sw.seqResolve && B.rblocks != 0;
    B.cap = (uint32_t) ((h->rb * RBU + OVERLAP_MAX + h->K) / h->K + 8);
    B.cands = (uint32_t) std::min<uint64_t>(std::min<uint64_t>(B.rblocks, CAND_MAX), std::max<uint64_t>(1, CAND_BYTES / ((2 * B.cap + SNAP) * sizeof(Row))));
    return SWSEM_OK;
}

// Step 2: device buffers for that shape, the tables' uploads, the statistics zeroed — one staged launch on the main stream.
int batch_upload(swsem *h, int n, BatchShape &B) {
    const uint32_t rblocks = B.rblocks;
    int r;
    if ((r = h->dContigs.reserve(n)) || (r = h->dMatchCount.reserve(n)) || (r = h->dStats.reserve(NSTATS)) || (r = h->dMatches.reserve(B.matchRows))) return r;
    if (B.blocks && ((r = h->dRegions.reserve((size_t) rblocks * B.cap)) || (r = h->dReplay.reserve((size_t) n * B.cap)) || (r = h->dRecs.reserve(rblocks)) ||
                     (r = h->dFast.reserve(rblocks)) || (r = h->dSegStart.reserve(rblocks)) || (r = h->dKeepN.reserve(rblocks)) ||
                     (r = h->dDstOff.reserve(rblocks)) || (r = h->dPrev.reserve(rblocks)) || (r = h->dCandOf.reserve(rblocks)) ||
                     (r = h->dCandBlock.reserve(B.cands)) || (r = h->dCand.reserve(B.cands)) || (r = h->dCandArea.reserve((size_t) B.cands * (2 * B.cap + SNAP)))))
        return r;
    if ((r = upload(h, h->dContigs.p, h->contigs.data(), n * sizeof(Contig), h->stream))) return r;
    if ((r = h->dRbContig.reserve(std::max<uint32_t>(rblocks, 1)))) return r;
    if (rblocks) {
        const uint32_t *had = h->dRbOrder.p;
        const bool fresh = build_resolve_order(h, rblocks, h->chainsPerWave);
        B.rslots = (uint32_t) (h->rbOrderHost.size() / h->chainsPerWave);
        if ((r = h->dRbOrder.reserve(h->rbOrderHost.size() + h->rbOrderHost.size() / 4 + 64))) return r;
        if ((r = upload(h, h->dRbContig.p, h->rbContigHost.data(), rblocks * sizeof(uint32_t), h->stream))) return r;
        if ((fresh || had != h->dRbOrder.p) && (r = upload(h, h->dRbOrder.p, h->rbOrderHost.data(), h->rbOrderHost.size() * sizeof(uint32_t), h->stream)))
            return r;
    }
    if ((r = zero_dev(h, h->dStats.p, NSTATS * sizeof(unsigned long long), h->stream))) return r;
    return flush_copies(h);
}

// Step 3: the launches.
int batch_launch(swsem *h, const uint8_t *qdev, int n, const BatchShape &B) {
    const uint32_t rblocks = B.rblocks, rslots = B.rslots, cap = B.cap;
    int r;
    const RefView v = h->view();
    const bool wrapped = v.fpCheck == 2;                // kernels instantiated with / without the lap epochs (ht_value)
    if (!B.blocks)
        for (auto &E : h->slot) if ((r = run_phase2b(h, E, false))) return r;
    // "this batch begins here": everything queued on the main stream before it has finished when this event has (the uploads
    // of the emission that follows wait for nothing else, emit_upload_tables)
    HIPCHK(hipEventRecord(h->evRoundTop, h->stream));
    h->roundTopFresh = true;
    if (!B.blocks) {
        h->mark(SWSEM_K_RESOLVE, true);
        if (wrapped) k_resolve_seq<true><<<dim3(n), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dMatches.p, h->dMatchCount.p);
        else k_resolve_seq<false><<<dim3(n), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dMatches.p, h->dMatchCount.p);
        h->mark(SWSEM_K_RESOLVE, false);
    } else {
        h->batchBlocks = rblocks; h->batchCands = B.cands;
        // An emission whose byte automata wait to be queued (run_phase2b): they are handed to the second stream AFTER the
        // resolve kernel has been handed to the first, behind an event recorded just before it — whatever hardware queues
        // the two streams share, the resolve is dealt its wave slots first.
        if (h->metaPending) { HIPCHK(hipStreamWaitEvent(h->stream, h->evMeta, 0)); h->metaPending = false; }
        bool anyDeferred = false;
        for (auto &E : h->slot) anyDeferred |= E.deferred2b;
        if (anyDeferred) HIPCHK(hipEventRecord(h->evFin, h->stream));
        h->mark(SWSEM_K_RESOLVE, true);
        if (h->chainsPerWave == (uint32_t) GC) {
            if (wrapped) k_resolve_blocks4<true><<<dim3(rslots), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRbOrder.p, h->dRegions.p, cap, h->rb, h->dRecs.p, h->overlap);
            else k_resolve_blocks4<false><<<dim3(rslots), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRbOrder.p, h->dRegions.p, cap, h->rb, h->dRecs.p, h->overlap);
        } else {
            if (wrapped) k_resolve_blocks<true><<<dim3(rslots), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRbOrder.p, h->dRegions.p, cap, h->rb, h->dRecs.p, h->overlap);
            else k_resolve_blocks<false><<<dim3(rslots), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRbOrder.p, h->dRegions.p, cap, h->rb, h->dRecs.p, h->overlap);
        }
        h->mark(SWSEM_K_RESOLVE, false);
        if (anyDeferred) {
            HIPCHK(hipStreamWaitEvent(h->stream2, h->evFin, 0));
            for (auto &E : h->slot) if ((r = run_phase2b(h, E, true))) return r;
        }
        h->mark(SWSEM_K_STITCH, true);
        unsigned long long *candCount = h->dStats.p + 8;
        k_stitch_pre<<<dim3((rblocks + 255) / 256), dim3(256), 0, h->stream>>>(h->dContigs.p, h->dRbContig.p, h->dRecs.p, h->rb, rblocks, h->dFast.p,
                                                                               h->dCandOf.p, h->dCandBlock.p, candCount, B.cands);
        // the rejected blocks, all at once (a wave that finds no candidate in its slot ends at once), then the walk
        if (wrapped) k_stitch_replay<true><<<dim3(B.cands), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRegions.p, h->dCandArea.p, cap, h->rb, h->dRecs.p,
                                                                                       h->dCandBlock.p, candCount, B.cands, h->dCand.p, h->dCandOf.p, h->dFast.p);
        else k_stitch_replay<false><<<dim3(B.cands), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRbContig.p, h->dRegions.p, h->dCandArea.p, cap, h->rb, h->dRecs.p,
                                                                                 h->dCandBlock.p, candCount, B.cands, h->dCand.p, h->dCandOf.p, h->dFast.p);
        if (wrapped) k_stitch<true><<<dim3(n), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRegions.p, h->dReplay.p, cap, h->rb, h->dRecs.p, h->dFast.p, h->dSegStart.p,
                                                                          h->dKeepN.p, h->dPrev.p, h->dDstOff.p, h->dMatchCount.p, h->dStats.p, h->dCandOf.p, h->dCand.p, h->dCandArea.p);
        else k_stitch<false><<<dim3(n), dim3(WAVE), 0, h->stream>>>(v, qdev, h->dContigs.p, h->dRegions.p, h->dReplay.p, cap, h->rb, h->dRecs.p, h->dFast.p, h->dSegStart.p,
                                                                    h->dKeepN.p, h->dPrev.p, h->dDstOff.p, h->dMatchCount.p, h->dStats.p, h->dCandOf.p, h->dCand.p, h->dCandArea.p);
        k_gather<<<dim3(rblocks), dim3(WAVE), 0, h->stream>>>(h->dContigs.p, h->dRbContig.p, h->dRegions.p, cap, h->dSegStart.p,
                                                            h->dKeepN.p, h->dDstOff.p, h->dMatches.p);
        h->mark(SWSEM_K_STITCH, false);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->evMatched, h->stream));
    return SWSEM_OK;
}

int run_batch(swsem *h, const uint8_t *qdev, const uint64_t *offsets, int n, uint32_t minLen, const uint64_t *lockPos) {
    if (n <= 0) return fail(SWSEM_EINVAL, "empty batch");
    if (minLen < (uint32_t) h->K)   // SlidingWindowSparseEMMatcher.cpp:480-483
        return fail(SWSEM_EINVAL, "Minimal matching length cannot be smaller than K (%u < %d)", minLen, h->K);
    h->batchValid = false;
    h->matchCount.clear();
    h->minLen = minLen;
    BatchShape B;
    int r;
    if ((r = batch_layout(h, offsets, n, minLen, lockPos, B)) || (r = batch_upload(h, n, B)) || (r = batch_launch(h, qdev, n, B))) return r;
    h->qdev = qdev;
    h->stats[0] = B.bases;
    h->hostProbes = B.probes;
    h->batchValid = true;
    return SWSEM_OK;
}

// Pinned landing zone for everything a batch hands back to the host: {stats[NSTATS] | match counts | emit results}:
// the copies queue up back to back and one wait serves them all. Queues the copies of the match counts and
// statistics (no wait; staged: the caller adds what it wants beside them and flushes).
int queue_counts(swsem *h, size_t extraBytes, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    const size_t n = h->contigs.size();
    const size_t countsAt = NSTATS * sizeof(unsigned long long), extraAt = (countsAt + n * sizeof(uint32_t) + 63) & ~(size_t) 63;
    const size_t bytes = extraAt + extraBytes;
    int r = h->pin.reserve(bytes, std::max<size_t>(2 * bytes, 1 << 20));       // see prepare_inserts: no regrowth in steady state
    if (r) return r;
    if ((r = download(h, h->pin.p, h->dStats.p, NSTATS * sizeof(unsigned long long), st)) ||
        (r = download(h, h->pin.p + countsAt, h->dMatchCount.p, n * sizeof(uint32_t), st)))
        return r;
    h->pinExtraAt = extraAt;
    return SWSEM_OK;
}

// after the wait: pinned block -> host state
void take_counts(swsem *h) {
    const size_t n = h->contigs.size();
    const unsigned long long *st = (const unsigned long long *) h->pin.p;
    const uint32_t *counts = (const uint32_t *) (h->pin.p + NSTATS * sizeof(unsigned long long));
    h->matchCount.assign(counts, counts + n);
    const uint64_t cands = std::min<uint64_t>(st[8], h->batchCands);   // replayed ahead of the walk (what the list had no room for was not)
    h->stats[1] = h->hostProbes; h->stats[2] = st[2]; h->stats[5] = st[3];
    h->stats[6] = st[9]; h->stats[7] = cands - std::min<uint64_t>(cands, st[9]); h->stats[8] = st[10];
    h->stitchDiag[0] += st[3]; h->stitchDiag[1] += st[5]; h->stitchDiag[2] += st[6]; h->stitchDiag[3] += st[7];
    h->stitchDiag[4] += cands; h->stitchDiag[5] += st[9]; h->stitchDiag[6] += st[10]; h->stitchDiag[7] = std::max<uint64_t>(h->stitchDiag[7], st[8]);
    if (h->batchBlocks >= 2048 && h->sw.overlapFixed < 0) {                                  // (a batch large enough for the share to mean something)
        // Rejected blocks are replayed side by side (k_stitch_replay) and accepted inside the walk's runs, so what a shorter warm-up
        // costs is that launch — as long as its slowest replay — while every block saves the positions it no longer scans twice. On
        // configs[2] (MEASUREMENTS §0b): 768 / 640 / 512 / 384 / 256 positions reject 0.09 / 0.33 / 1.2 / 4.1 / 13.7 % of the blocks
        // and 512 is the fastest; from 4 % on rejected blocks begin to follow each other, and those the walk replays itself.
        const uint64_t replayed = st[3];
        if (replayed * 40 > h->batchBlocks) h->overlap = std::min<uint32_t>((uint32_t) OVERLAP_MAX, h->overlap + 128);          // > 2.5 %: longer
        else if (replayed * 160 < h->batchBlocks) h->overlap = std::max<uint32_t>(384u, h->overlap - 128);         // < 0.625 %: shorter
        h->batchBlocks = 0;                                          // (these counts are taken once per batch)
    }
    uint64_t tot = 0;
    for (size_t c = 0; c < n; c++) tot += h->matchCount[c];
    h->stats[3] = tot;
}

int fetch_counts(swsem *h) {
    int r = queue_counts(h, 0);
    if (r || (r = flush_copies(h))) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    take_counts(h);
    return SWSEM_OK;
}

}  // namespace
