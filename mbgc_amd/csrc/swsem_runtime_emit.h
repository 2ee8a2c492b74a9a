// Part of swsem_runtime.hip: processMatches for a batch's contigs in two slots, with the speculative finalize queued
// behind its first pass. (The byte automata of the second phase are queued by run_phase2b, swsem_runtime_loader.h.)
namespace {

// waits for the second phase of the emission in slot si, if one is running, and takes its results
int end_slot(swsem *h, int si) {
    EmitSlot &E = h->slot[si];
    if (!E.outstanding) return SWSEM_OK;
    HIPCHK(hipSetDevice(h->device));
    { int d = run_phase2b(h, E, false); if (d) return d; }            // (nobody launched a resolve since: nothing to wait for)
    HIPCHK(hipEventSynchronize(E.evDone));
    E.outstanding = false;
    const int n = E.emitN;
    E.eout.assign((const EmitOut *) E.pinE.p, (const EmitOut *) E.pinE.p + n);
    uint64_t tot = 0;
    E.hostStreamOff.assign((size_t) n * SWSEM_NSTREAMS, 0);
    for (int k = 0; k < n; k++)
        for (int st = 0; st < SWSEM_NSTREAMS; st++) {
            if (E.eout[k].unmatchedChars == UINT64_MAX) E.eout[k].size[st] = 0;
            E.hostStreamOff[(size_t) k * SWSEM_NSTREAMS + st] = tot;       // == packBase on the device
            tot += E.eout[k].size[st];
        }
    E.packedBytes = tot;
    E.hostStreamsValid = false;
    if (h->emitHostCopy) {
        int r = E.next_host_streams(tot + 1);
        if (r) return r;
        if (tot) HIPCHK(hipMemcpyAsync(E.hostStreams().p, E.dEArena.p, tot, hipMemcpyDeviceToHost, h->s3()));
        HIPCHK(hipStreamSynchronize(h->s3()));
        E.hostStreamsValid = true;
    }
    return SWSEM_OK;
}

// ---- the steps of emit_begin_impl, in the order it takes them

// Slot layout, host arithmetic only: per contig its rows, chunk and span owners and stream bases in the arena.
int emit_layout(swsem *h, EmitSlot &E, int n, const int *contigIdx, const uint64_t *lockPos, const int *factor,
                const int64_t *processed, const int64_t *targetIdx, uint64_t &rows, uint64_t &arena) {
    E.ecg.assign(n, EmitContig());
    std::vector<int> &which = E.ewhich;       // uploaded asynchronously: must outlive this call
    which.assign(n, 0);
    rows = 0; arena = 0;
    E.chunkOwner.clear(); E.spanOwner.clear();
    for (int k = 0; k < n; k++) {
        const int c = contigIdx ? contigIdx[k] : k;
        if (c < 0 || c >= (int) h->contigs.size()) return fail(SWSEM_EINVAL, "swsem_emit: no contig %d in the batch", c);
        which[k] = c;
        EmitContig &e = E.ecg[k];
        const Contig &cg = h->contigs[c];
        // rows are reserved for the most matches a contig can have, so no round trip to the host is needed
        // between match-finding and emission
        const uint64_t nm = cg.n / (h->minLen ? h->minLen : 1) + 2;
        e.qoff = cg.qoff; e.n = cg.n; e.matchBase = cg.matchBase;
        e.lock = lockPos ? lockPos[k] : UINT64_MAX;
        e.scratchBase = rows;
        e.cap = (uint32_t) (nm + 2);
        rows += e.cap;
        e.chunk0 = (uint32_t) E.chunkOwner.size();
        E.chunkOwner.insert(E.chunkOwner.end(), (e.cap + CH - 1) / CH, (uint32_t) k);
        e.span0 = (uint32_t) E.spanOwner.size();
        E.spanOwner.insert(E.spanOwner.end(), (e.cap + MSPAN - 1) / MSPAN, (uint32_t) k);
        e.factor = factor ? factor[k] : 128;
        e.processed = processed ? processed[k] : 0;
        e.targetIdx = targetIdx ? targetIdx[k] : 0;
        const uint64_t szs[SWSEM_NSTREAMS] = {cg.n + nm + 16, 4 * nm + 16, nm + 16, 14 * nm + 16, nm + 16, cg.n + 2 * nm + 16};
        for (int st = 0; st < SWSEM_NSTREAMS; st++) { e.streamBase[st] = arena; arena += (szs[st] + 15) & ~15ull; }
    }
    return SWSEM_OK;
}

// Slot reservation, for the largest request seen so far.
int emit_reserve(swsem *h, EmitSlot &E, int n, uint64_t rows, uint64_t arena, uint64_t nLoaded) {
    h->capN = std::max<uint64_t>(h->capN, (uint64_t) n); h->capRows = std::max(h->capRows, rows); h->capArena = std::max(h->capArena, arena);
    if (nLoaded + 1 > h->capLoaded) h->capLoaded = std::max<uint64_t>(4096, 2 * (nLoaded + 1));   // (regrowing a buffer waits for the whole device: rarely)
    h->capChunks = std::max<uint64_t>(h->capChunks, E.chunkOwner.size());
    const uint64_t N = h->capN, R = h->capRows, A = h->capArena, Cn = h->capChunks;
    int r;
    if ((r = E.dECg.reserve(N)) || (r = E.dEOut.reserve(N)) || (r = E.dEWhich.reserve(N)) || (r = E.dEM.reserve(R)) ||
        (r = E.dENext0.reserve(R)) || (r = E.dERawLp.reserve(R)) || (r = E.dERawNext0.reserve(R)) || (r = E.dERm.reserve(R)) ||
        (r = E.dEKeep.reserve(R)) || (r = E.dEMeta.reserve(R)) || (r = E.dECorr.reserve(R)) ||
        (r = E.dESz.reserve(R * 6)) || (r = E.dEOfs.reserve(R * 6)) || (r = E.dEArena.reserve(A)) || (r = E.dELoaded.reserve(h->capLoaded)) ||
        (r = E.dEStat.reserve(8)) || (r = E.dELong.reserve(LONG_COPY_CAP)) || (r = E.dELongCount.reserve(4)) || (r = E.dEPm.reserve(R)) ||
        (r = E.dELit.reserve((size_t) Cn * (CH / WAVE))) || (r = E.dEBad.reserve(Cn)) || (r = E.dEOwner.reserve(Cn)) || (r = E.dESpanOwner.reserve(Cn)) ||
        (r = E.dEStates.reserve((size_t) Cn * (CH / MB) * 2)) || (r = E.dEChunk.reserve((size_t) Cn * 6)) ||
        (r = E.dEPack.reserve((size_t) N * SWSEM_NSTREAMS)))
        return r;
    if (!E.statZeroed) { HIPCHK(hipMemsetAsync(E.dEStat.p, 0, 8 * sizeof(unsigned long long), h->stream)); E.statZeroed = true; }
    return SWSEM_OK;
}

// Table uploads. The emission's tables (and, behind them, the speculative finalize's: spec_plan) travel on a stream of
// their own that waits for nothing but the point where this batch began: they land while the chains are still running,
// and neither they nor their launch gaps sit between the stitch and the first pass. (An emission that is not the first
// of its batch — a retry pass over some of its contigs — has no such point: its uploads are ordered behind everything
// queued so far.)
int emit_upload_tables(swsem *h, EmitSlot &E, int n, const uint64_t *refExtLoadedPos, uint64_t nLoaded, const swsem_spec_finalize_t *spec) {
    hipStream_t up = h->streamUp;
    int r;
    if (!h->roundTopFresh) HIPCHK(hipEventRecord(h->evRoundTop, h->stream));
    h->roundTopFresh = false;
    HIPCHK(hipStreamWaitEvent(up, h->evRoundTop, 0));
    if ((r = upload(h, E.dEOwner.p, E.chunkOwner.data(), E.chunkOwner.size() * sizeof(uint32_t), up))) return r;
    if ((r = upload(h, E.dESpanOwner.p, E.spanOwner.data(), E.spanOwner.size() * sizeof(uint32_t), up))) return r;
    if ((r = upload(h, E.dECg.p, E.ecg.data(), n * sizeof(EmitContig), up)) || (r = upload(h, E.dEWhich.p, E.ewhich.data(), n * sizeof(int), up))) return r;
    E.eloaded.assign(refExtLoadedPos, refExtLoadedPos + nLoaded);
    if ((r = upload(h, E.dELoaded.p, E.eloaded.data(), nLoaded * sizeof(uint64_t), up))) return r;
    if (spec) {                                                      // the prediction k_spec_verify checks pass 1 against
        if ((r = h->dGate.reserve(4)) || (r = h->dPred.reserve(2 * (size_t) n + 64))) return r;
        if ((r = upload(h, h->dPred.p, spec->predExt, n, up)) || (r = upload(h, h->dPred.p + n, spec->predRC, n, up))) return r;
    }
    return flush_copies(h);
}

// what the emission's kernels are given, and the emission on the books from here on (the plan of the speculative
// finalize asks ref_write_guard about it)
EmitView emit_book(swsem *h, EmitSlot &E, int si, const swsem_emit_params_t *p, int n, uint64_t nLoaded, bool regionsAhead) {
    EmitView v;
    v.ref = h->ref; v.qbuf = h->qdev; v.matches = h->dMatches.p; v.matchCount = h->dMatchCount.p;
    v.pos1 = (uint64_t) h->ld.pos1; v.refLength = h->refLength(); v.maxRefLength = h->maxRefLength;
    v.loaded = E.dELoaded.p; v.nLoaded = (uint32_t) nLoaded; v.p = *p;
    v.em = E.dEM.p; v.next0 = E.dENext0.p; v.removed = E.dERm.p; v.keepIdx = E.dEKeep.p;
    v.rawLp = regionsAhead ? E.dERawLp.p : nullptr; v.rawNext0 = regionsAhead ? E.dERawNext0.p : nullptr;
    v.meta = E.dEMeta.p; v.corr = E.dECorr.p; v.sz = E.dESz.p; v.arena = E.dEArena.p; v.out = E.dEOut.p;
    v.packBase = E.dEPack.p;
    v.pairMask = E.dEPm.p; v.litBits = E.dELit.p; v.metaBad = E.dEBad.p;
    v.longCopies = E.dELong.p; v.longCount = E.dELongCount.p;
    v.ofs = E.dEOfs.p;
    v.chunkCnt = E.dEChunk.p;
    v.chunkOwner = E.dEOwner.p; v.spanOwner = E.dESpanOwner.p;
    v.ncontigs = (uint32_t) n;
    E.v2b = v; E.grid2b = (uint32_t) E.chunkOwner.size(); E.n2b = n;
    E.donePending = true;
    h->latest = si; h->selected = -1;
    E.outstanding = true; E.refGuarded = false; E.emitN = n; E.emitPos1 = (uint64_t) h->ld.pos1; E.qdev = h->qdev; E.params = *p;
    E.emitLaps = h->ld.laps;
    uint64_t lm = UINT64_MAX; bool all = true;
    for (int k = 0; k < n; k++) { if (E.ecg[k].lock == UINT64_MAX) all = false; else lm = std::min(lm, E.ecg[k].lock); }
    E.lockMin = all ? lm : UINT64_MAX;
    E.packedBytes = 0; E.hostStreamsValid = false;
    E.deferred2b = false;
    return v;
}

// Plan of the speculative finalize. The host's half first (lock window, piece schedule, separators: load_pieces and its
// callees, nothing launched): it can find that this finalize cannot be queued behind a gate at all (SWSEM_ESPEC: a write
// that would have to wait for an older emission, a separator over an already hashed byte). With several replicas that has
// to be known BEFORE the verdicts are reduced: a replica that cannot apply the round must say so in the reduction, or the
// others apply it without it. Then the finalize's tables, on the uploads' stream too. The caller holds the copy of
// h->ld this plan is taken back to.
int spec_plan(swsem *h, const swsem_spec_finalize_t *spec, const uint32_t *gate, bool &planned) {
    h->specMode = true;
    int r = finalize_impl(h, spec->ntargets, spec->ext_dev, spec->ext_len, spec->addSep, spec->sep, spec->lazySeparator, spec->lockPos,
                          spec->loadedAfter, gate, true);
    h->specMode = false;
    planned = r == SWSEM_OK;
    if (r == SWSEM_ESPEC) return SWSEM_OK;                           // not possible this time: nothing will be queued
    if (r) return r;
    return prepare_inserts(h, h->streamUp);
}

// Pass 1 on the main stream behind the tables, and its results' way to the host (unmatchedChars, the dissimilarity
// verdict), with the match counts and statistics: one pinned block, one wait (evP1).
//
// The source-region lookups of the pairing chain's lazy rule (k_emit_regions_raw, when v.rawLp is set) run beside it on
// streamAux, behind the batch's match-finding (evMatched) and the tables: between the gather and the table insertion the
// chip runs a handful of workgroups (30 µs there), while behind pass 1 the same lookups ran beside the request-bound insertion
// and took 230 µs — with the next batch's resolve waiting for the chain they head (evMeta, batch_launch). They index the
// stitched rows, so they need nothing of pass 1; k_emit_p1_compact takes their values along to the rows it keeps and is the
// one kernel that waits for them (evRegions), two launches after they were queued. (No event bracket of their own: the
// families' per-launch figures keep their meaning.)
// Only the first emission of a batch takes this path (the caller decides: emit_begin_impl). A later one — another pass
// over some of the same batch's contigs — has no "match-finding ended here" point that lies ahead of it: it keeps
// k_emit_meta_regions behind pass 1. (A unit of stopped targets that is matched again is a batch of its own, and its
// emission the first of that batch.)
int emit_pass1(swsem *h, EmitSlot &E, const EmitView &v, int n) {
    const dim3 grid2(E.grid2b);
    int r;
    HIPCHK(hipEventRecord(h->evTables, h->streamUp));
    if (v.rawLp) {
        HIPCHK(hipStreamWaitEvent(h->streamAux, h->evMatched, 0));
        HIPCHK(hipStreamWaitEvent(h->streamAux, h->evTables, 0));
        k_emit_regions_raw<<<grid2, dim3(CH), 0, h->streamAux>>>(v, E.dECg.p, E.dEWhich.p);
        HIPCHK(hipEventRecord(h->evRegions, h->streamAux));
    }
    HIPCHK(hipStreamWaitEvent(h->stream, h->evTables, 0));
    hipStream_t sP = h->stream;
    h->mark(SWSEM_K_EMIT, true, sP);
    k_emit_p1_removed<<<grid2, dim3(CH), 0, sP>>>(v, E.dECg.p, E.dEWhich.p);
    k_emit_p1_scan<<<dim3(n), dim3(CH), 0, sP>>>(v, E.dECg.p, E.dEWhich.p);
    if (v.rawLp) HIPCHK(hipStreamWaitEvent(sP, h->evRegions, 0));
    k_emit_p1_compact<<<grid2, dim3(CH), 0, sP>>>(v, E.dECg.p, E.dEWhich.p);
    k_emit_p1_finish<<<dim3(n), dim3(CH), 0, sP>>>(v, E.dECg.p);
    h->mark(SWSEM_K_EMIT, false, sP);
    HIPCHK(hipGetLastError());
    if ((r = queue_counts(h, n * sizeof(EmitOut), sP))) return r;
    if ((r = download(h, h->pin.p + h->pinExtraAt, E.dEOut.p, n * sizeof(EmitOut), sP)) || (r = flush_copies(h))) return r;
    HIPCHK(hipEventRecord(h->evP1, sP));
    return SWSEM_OK;
}

// The pairing kernels on streamAux behind pass 1 (k_emit_meta_regions only where the lookups were not made beside pass 1:
// emit_pass1). The byte automata (sizes .. write) that follow them are queued later
// (run_phase2b): behind the speculative finalize, and not before the next batch's resolve kernel has been handed over.
int emit_pairing(swsem *h, EmitSlot &E, const EmitView &v, int n) {
    const dim3 grid2(E.grid2b), spans((uint32_t) E.spanOwner.size());
    const size_t outBytes = n * sizeof(EmitOut);
    int r = E.pinE.reserve(outBytes, std::max<size_t>(2 * outBytes, 1 << 20));
    if (r) return r;
    HIPCHK(hipStreamWaitEvent(h->streamAux, h->evP1, 0));
    h->mark(SWSEM_K_EMIT2, true, h->streamAux);
    if (!v.rawLp) k_emit_meta_regions<<<grid2, dim3(CH), 0, h->streamAux>>>(v, E.dECg.p);
    k_emit_meta_masks<<<spans, dim3(MLANES), 0, h->streamAux>>>(v, E.dECg.p);
    k_emit_meta_spec<<<spans, dim3(MLANES), 0, h->streamAux>>>(v, E.dECg.p, E.dEStates.p, h->sw.metaWarm, E.dEStat.p);
    // (the next batch's resolve is launched behind this kernel, batch_launch: a launch of thousands of waves that is still
    // running takes the slots the resolve's blocks are sized for, and the blocks that have to wait double its time)
    HIPCHK(hipEventRecord(h->evMeta, h->streamAux));
    h->metaPending = true;
    k_emit_meta_check<<<grid2, dim3(WAVE), 0, h->streamAux>>>(v, E.dECg.p, E.dEStates.p, E.dEStat.p);
    k_emit_meta_stitch<<<dim3(n), dim3(WAVE), 0, h->streamAux>>>(v, E.dECg.p, E.dEStates.p, E.dEStat.p);
    h->mark(SWSEM_K_EMIT2, false, h->streamAux);
    HIPCHK(hipEventRecord(E.evMetaDone, h->streamAux));
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}

// The gate: the device's check of the prediction behind pass 1, the word's reduction over the replicas, and — when the
// plan stood — the finalize's launches behind it (`queued`): the copies start the moment pass 1 ends, the insertion is
// queued behind pass 1 too, and every one of them does nothing unless k_spec_verify's word says the prediction held.
int spec_gate(swsem *h, EmitSlot &E, const swsem_spec_finalize_t *spec, uint32_t *gate, int n, bool planned, bool &queued, bool &exchanged) {
    k_spec_verify<<<1, 256, 0, h->stream>>>(E.dEOut.p, E.dECg.p, n, h->dPred.p, h->dPred.p + n, spec->factor, spec->rcFactor, gate);
    if (spec->veto || !planned) HIPCHK(hipMemsetAsync(gate, 0, sizeof(uint32_t), h->stream));
    // several replicas: the word becomes the minimum over all of them before anything gated by it is queued
    if (spec->exchange) {
        if (spec->exchange(spec->exchange_ctx, 0, gate, (void *) h->stream)) return fail(SWSEM_EHIP, "speculative finalize: the exchange between the replicas failed");
        exchanged = true;
    }
    if (planned) {
        int r = launch_inserts(h, gate);
        if (r) return r;
        queued = true;
    }
    return SWSEM_OK;
}

// The host's verdict on a queued finalize, from the values pass 1 handed back: the same test k_spec_verify makes, and
// every other replica's.
bool spec_verdict(swsem *h, const EmitSlot &E, const swsem_spec_finalize_t *spec, int n, bool exchanged) {
    bool ok = !spec->veto;
    for (int k = 0; k < n && ok; k++) {
        const uint64_t un = E.eout[k].unmatchedChars, len = E.ecg[k].n;
        ok = un != UINT64_MAX && (un * (uint64_t) spec->factor > len) == (spec->predExt[k] != 0) &&
             (un * (uint64_t) spec->rcFactor > len) == (spec->predRC[k] != 0);
    }
    if (exchanged) ok = spec->exchange(spec->exchange_ctx, 1, nullptr, (void *) h->stream) == 1 && ok;
    return ok;
}

// processMatches for `n` contigs of the last batch in one pass (the reference runs it per contig on the
// worker thread that matched it, MGMP.cpp:381). Results stay on the handle until the next emit call.
//
// Speculative finalize (`spec` with targets): the round's loadRef / loadSeparator / lock releases are worked out on the
// host now, under the caller's prediction of every contig's extension decision, and queued behind a device-side check of
// that prediction — so the copies and the table insertion start the moment pass 1 ends instead of after the host's round
// trip. The host comes to the same verdict from the values pass 1 hands back and keeps or undoes its bookkeeping
// accordingly; when the prediction fails nothing on the device has changed.
int emit_begin_impl(swsem *h, const swsem_emit_params_t *p, int n, const int *contigIdx, const uint64_t *lockPos,
                    const int *factor, const int64_t *processed, const int64_t *targetIdx,
                    const uint64_t *refExtLoadedPos, uint64_t nLoaded, const swsem_spec_finalize_t *spec, int *applied) {
    HIPCHK(hipSetDevice(h->device));
    if (applied) *applied = 0;
    if (spec && spec->ntargets <= 0) spec = nullptr;
    const int si = h->latest ^ 1;                                     // the slot not used by the previous emission
    { int e = end_slot(h, si); if (e) return e; }                    // its scratch is about to be reused
    EmitSlot &E = h->slot[si];
    if (!h->batchValid) return fail(SWSEM_EINVAL, "swsem_emit: no match results on the handle");
    if (n <= 0) return fail(SWSEM_EINVAL, "swsem_emit: empty request");
    if (p->lazyDecompressionSupport && nLoaded == 0) return fail(SWSEM_EINVAL, "swsem_emit: lazy mode needs refExtLoadedPosArr");
    if (p->gapDepthOffsetEncoding > 64 || p->gapDepthOffsetEncoding < 0)
        return fail(SWSEM_EINVAL, "gapDepthOffsetEncoding %d out of range (MAX_GAP_DEPTH / 2)", p->gapDepthOffsetEncoding);
    int r;
    uint64_t rows, arena;
    // the first emission since the batch's match-finding was launched (emit_upload_tables takes the flag down): its region
    // lookups run beside pass 1 (emit_pass1)
    const bool regionsAhead = h->roundTopFresh && p->lazyDecompressionSupport;
    if ((r = emit_layout(h, E, n, contigIdx, lockPos, factor, processed, targetIdx, rows, arena)) ||
        (r = emit_reserve(h, E, n, rows, arena, nLoaded)) ||
        (r = emit_upload_tables(h, E, n, refExtLoadedPos, nLoaded, spec)))
        return r;
    // no synchronisation here: the kernels below queue up behind match-finding while it is still running
    const EmitView v = emit_book(h, E, si, p, n, nLoaded, regionsAhead);
    const LoaderState snap = h->ld;                                  // what a finalize that is not applied goes back to
    bool planned = false, queued = false, exchanged = false;
    uint32_t *gate = spec ? (spec->gate_dev ? spec->gate_dev : h->dGate.p) : nullptr;
    if (spec && (r = spec_plan(h, spec, gate, planned))) return r;
    const bool needCounts = h->matchCount.size() != h->contigs.size();
    if ((r = emit_pass1(h, E, v, n))) return r;
    if ((r = emit_pairing(h, E, v, n))) return r;
    if (spec) {
        if ((r = spec_gate(h, E, spec, gate, n, planned, queued, exchanged))) return r;
        if (!queued) h->ld = snap;
    }
    E.deferred2b = true; E.waitFin2b = queued;                       // the byte automata: behind the finalize when one was queued
    // While pass 1 runs: the emission before this one — its second phase ran beside this batch's match-finding — is taken now, its
    // streams copied to the host (end_slot), instead of when the caller asks for them right after this call returns: on divergent
    // collections that copy is megabytes per emission and stood between one unit's loads and the next unit's launch.
    if (h->emitHostCopy) { int e = end_slot(h, si ^ 1); if (e) return e; }
    HIPCHK(hipEventSynchronize(h->evP1));                           // pass 1 and its copies to the host (not what was queued after them)
    if (needCounts) take_counts(h);
    E.eout.assign((const EmitOut *) (h->pin.p + h->pinExtraAt), (const EmitOut *) (h->pin.p + h->pinExtraAt) + n);
    if (queued) {
        if (spec_verdict(h, E, spec, n, exchanged)) { if (applied) *applied = 1; }
        else h->ld = snap;
    } else if (exchanged)
        (void) spec->exchange(spec->exchange_ctx, 1, nullptr, (void *) h->stream);   // (this replica said no in the reduction: the word is 0 everywhere; taken so that the exchange's state is the same on every rank)
    return SWSEM_OK;
}

}  // namespace
