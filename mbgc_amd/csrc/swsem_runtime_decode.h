// Part of swsem_runtime.hip: the driver of the decoder's automaton on the device (swsem_decode.hip).
namespace {

int decode_jobs(swsem *h, const swsem_emit_params_t *p, int n, const std::vector<DecodeJob> &jobs, std::vector<DecodeOut> &outs) {
    int r;
    // records a contig can need: one per mapLen entry (two bytes at least, four without the frugal encoding) + the tail
    std::vector<uint64_t> aux(3 * (size_t) n + 1, 0);
    uint64_t *recBase = aux.data(), *firstDiff = recBase + n + 1;
    uint32_t *badFlags = (uint32_t *) (firstDiff + n);
    for (int k = 0; k < n; k++) {
        recBase[k + 1] = recBase[k] + jobs[k].size[SWSEM_LEN] / (p->frugal64bitLenEncoding ? 2 : 4) + 2;
        firstDiff[k] = UINT64_MAX;
    }
    if ((r = h->dJobs.reserve(n)) || (r = h->dDecPlan.reserve(n)) || (r = h->dDecAux.reserve(aux.size())) || (r = h->dDecRecs.reserve(recBase[n]))) return r;
    HIPCHK(hipMemcpyAsync(h->dJobs.p, jobs.data(), (size_t) n * sizeof(DecodeJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->dDecAux.p, aux.data(), aux.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    const uint64_t *dRecBase = h->dDecAux.p;
    unsigned long long *dFirstDiff = (unsigned long long *) (h->dDecAux.p + n + 1);
    uint32_t *dBad = (uint32_t *) (h->dDecAux.p + 2 * (size_t) n + 1);
    k_decode_plan<<<dim3(n), dim3(WAVE), 0, h->stream>>>(*p, h->dJobs.p, h->dDecRecs.p, dRecBase, h->dDecPlan.p, h->maxRefLength + REF_SLACK);
    HIPCHK(hipGetLastError());
    std::vector<DecPlanOut> plans(n);
    HIPCHK(hipMemcpyAsync(plans.data(), h->dDecPlan.p, (size_t) n * sizeof(DecPlanOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    // grid.y holds at most 65 535 blocks: contigs go in slices of that many, each slice sized by its own longest contig
    // (a batch of draft assemblies — tens of targets of a thousand contigs each — has more)
    constexpr int YMAX = 65535;
    for (int c0 = 0; c0 < n; c0 += YMAX) {
        const int cn = std::min(YMAX, n - c0);
        uint64_t maxRec = 0, maxLen = 0;
        bool anyExpect = false;
        for (int k = c0; k < c0 + cn; k++) {
            if (plans[k].unmatched < 0) continue;
            maxRec = std::max(maxRec, plans[k].nrec); maxLen = std::max(maxLen, plans[k].destLen);
            anyExpect |= jobs[k].expect != nullptr;
        }
        if ((maxRec + 255) / 256 > 0x7FFFFFFFull || (maxLen + 4095) / 4096 > 0x7FFFFFFFull) return fail(SWSEM_EINVAL, "swsem decode: a contig too long for one launch");
        if (maxRec) k_decode_fill<<<dim3((unsigned) ((maxRec + 255) / 256), (unsigned) cn), dim3(256), 0, h->stream>>>(h->ref, *p, h->dJobs.p, h->dDecRecs.p, dRecBase, h->dDecPlan.p, dBad, h->maxRefLength + REF_SLACK, (uint32_t) c0);
        if (anyExpect && maxLen) k_decode_check<<<dim3((unsigned) ((maxLen + 4095) / 4096), (unsigned) cn), dim3(256), 0, h->stream>>>(h->dJobs.p, h->dDecPlan.p, dFirstDiff, (uint32_t) c0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(aux.data(), h->dDecAux.p, aux.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    outs.resize(n);
    for (int k = 0; k < n; k++) {
        const bool bad = plans[k].unmatched < 0 || badFlags[k] != 0;
        outs[k].destLen = plans[k].destLen; outs[k].unmatched = bad ? -1 : plans[k].unmatched; outs[k].firstDiff = bad ? UINT64_MAX : firstDiff[k];
    }
    return SWSEM_OK;
}

// The chained plan of a collection (k_decode_plan_chain): records, plan rows and record bases stay in HBM for the fills.
int decode_plan_chain(swsem *h, const swsem_emit_params_t *p, const ChainStreams &S, int nstarts, const swsem_chain_start_t *starts, int ntargets,
                      const uint32_t *seqCount, const uint64_t *lockPos, uint64_t ncontigs, swsem_chain_contig_t *out, int *firstBadChain) {
    static_assert(sizeof(ChainContig) == sizeof(swsem_chain_contig_t), "swsem_chain_contig_t");
    auto &C = h->chain;
    C.n = 0; C.jobsDest = nullptr; C.regionFor = 0;
    int r;
    const uint64_t w = p->frugal64bitLenEncoding ? 2 : 4;
    // records a chain can need: one per mapLen entry of its span (two bytes at least, four without the frugal encoding) and a
    // tail per contig, + 1 (decode_jobs: the same per contig)
    std::vector<ChainStart> cs(nstarts);
    std::vector<uint64_t> lockOf(ncontigs);
    uint64_t recTotal = 0, contigAt = 0;
    uint32_t targetAt = 0;
    for (int k = 0; k < nstarts; k++) {
        const swsem_chain_start_t &a = starts[k];
        if (a.firstTarget != targetAt || (uint64_t) a.firstTarget + a.nTargets > (uint64_t) ntargets)
            return fail(SWSEM_EINVAL, "swsem_decode_plan_chain_dev: chain %d does not start where chain %d ended", k, k - 1);
        ChainStart &c = cs[k];
        uint64_t nc = 0;
        for (uint32_t t = a.firstTarget; t < a.firstTarget + a.nTargets; t++) {
            for (uint32_t s = 0; s < seqCount[t]; s++) { if (contigAt + nc >= ncontigs) return fail(SWSEM_EINVAL, "swsem_decode_plan_chain_dev: more sequences than contigs"); lockOf[contigAt + nc++] = lockPos[t]; }
        }
        for (int st = 0; st < SWSEM_NSTREAMS; st++) { c.cur[st] = a.cur[st]; c.end[st] = a.end[st]; }
        // the span of mapLen bytes: up to the chain's end where it is known, else to the stream's
        const uint64_t lenEnd = a.checkEnd && a.end[SWSEM_LEN] <= S.n[SWSEM_LEN] ? a.end[SWSEM_LEN] : S.n[SWSEM_LEN];
        const uint64_t span = lenEnd > a.cur[SWSEM_LEN] ? lenEnd - a.cur[SWSEM_LEN] : 0;
        c.firstTarget = a.firstTarget; c.nTargets = a.nTargets; c.checkEnd = a.checkEnd; c.pad = 0;
        c.firstContig = contigAt; c.recBase = recTotal; c.recCap = span / w + 2 * nc + 2;
        recTotal += c.recCap; contigAt += nc; targetAt += a.nTargets;
    }
    if (contigAt != ncontigs || targetAt != (uint32_t) ntargets) return fail(SWSEM_EINVAL, "swsem_decode_plan_chain_dev: the chains cover %llu contigs of %llu", (unsigned long long) contigAt, (unsigned long long) ncontigs);
    if (ncontigs == 0) return SWSEM_OK;
    if ((r = C.dStarts.reserve(nstarts)) || (r = C.dContigs.reserve(ncontigs)) || (r = C.dSeqCount.reserve(ntargets)) || (r = C.dLock.reserve(ntargets)) ||
        (r = C.dRecBase.reserve(ncontigs)) || (r = C.dChainBad.reserve(nstarts)) || (r = C.dBad.reserve(ncontigs)) ||
        (r = h->dDecPlan.reserve(ncontigs)) || (r = h->dDecRecs.reserve(recTotal))) return r;
    HIPCHK(hipMemcpyAsync(C.dStarts.p, cs.data(), cs.size() * sizeof(ChainStart), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dSeqCount.p, seqCount, (size_t) ntargets * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dLock.p, lockPos, (size_t) ntargets * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->dDecPlan.p, 0xFF, ncontigs * sizeof(DecPlanOut), h->stream));          // (unmatched = -1 until planned)
    HIPCHK(hipMemsetAsync(C.dContigs.p, 0xFF, ncontigs * sizeof(ChainContig), h->stream));
    HIPCHK(hipMemsetAsync(C.dRecBase.p, 0, ncontigs * sizeof(uint64_t), h->stream));
    HIPCHK(hipMemsetAsync(C.dBad.p, 0, ncontigs * sizeof(uint32_t), h->stream));
    k_decode_plan_chain<<<dim3((unsigned) nstarts), dim3(WAVE), 0, h->stream>>>(*p, S, C.dStarts.p, C.dSeqCount.p, C.dLock.p, h->dDecRecs.p, h->dDecPlan.p,
                                                                                  C.dContigs.p, C.dRecBase.p, C.dChainBad.p, h->maxRefLength + REF_SLACK);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> bad(nstarts);
    HIPCHK(hipMemcpyAsync(out, C.dContigs.p, ncontigs * sizeof(ChainContig), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(bad.data(), C.dChainBad.p, (size_t) nstarts * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    C.streams = S; C.params = *p; C.n = ncontigs;
    C.nrec.resize(ncontigs); C.destLen.resize(ncontigs); C.litEnd.resize(ncontigs); C.lock = lockOf;
    for (uint64_t c = 0; c < ncontigs; c++) { C.nrec[c] = out[c].unmatched < 0 ? 0 : out[c].nrec; C.destLen[c] = out[c].destLen; C.litEnd[c] = out[c].litEnd; }
    *firstBadChain = -1;
    for (int k = nstarts - 1; k >= 0; k--) if (bad[k]) *firstBadChain = k;
    return SWSEM_OK;
}

// contigs [c0, c1) of the planned collection into dest + destOff[c]: one k_decode_fill launch (slices of 65 535 contigs);
// masked: k_decode_fill_region against the granule bitmap decode_closure_region left in the handle
int decode_fill_range(swsem *h, uint64_t c0, uint64_t c1, uint8_t *dest, const uint64_t *destOff, bool masked = false) {
    auto &C = h->chain;
    if (masked && (C.regionFor != C.n || C.n == 0)) return fail(SWSEM_EINVAL, "swsem_decode_fill_region_dev: no granule closure has been made for this plan (swsem_decode_closure_region_dev)");
    if (c1 > C.n || c0 > c1) return fail(SWSEM_EINVAL, "swsem_decode_fill_range_dev: contigs [%llu, %llu) of %llu planned", (unsigned long long) c0, (unsigned long long) c1, (unsigned long long) C.n);
    int r;
    if (C.jobsDest != dest || !dest) {
        std::vector<DecodeJob> jobs(C.n);
        for (uint64_t c = 0; c < C.n; c++) {
            DecodeJob &j = jobs[c];
            for (int st = 0; st < SWSEM_NSTREAMS; st++) { j.stream[st] = C.streams.p[st]; j.size[st] = C.streams.n[st]; }
            j.size[SWSEM_LIT] = C.litEnd[c];                                  // (the fill reads literals up to the contig's separator, flags as far as the plan said)
            j.refLockPos = C.lock[c]; j.dest = dest + destOff[c]; j.destCap = destOff[c + 1] - destOff[c]; j.expect = nullptr;
        }
        if ((r = h->dJobs.reserve(C.n))) return r;
        HIPCHK(hipMemcpyAsync(h->dJobs.p, jobs.data(), C.n * sizeof(DecodeJob), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));                               // (the table is pageable host memory)
        C.jobsDest = dest;
    }
    // (a contig that is never filled needs no place: a selection's buffer holds the contigs of its closure only)
    for (uint64_t c = c0; c < c1; c++)
        if (destOff[c + 1] - destOff[c] < C.destLen[c]) return fail(SWSEM_EINVAL, "swsem_decode_fill_range_dev: contig %llu does not fit its place", (unsigned long long) c);
    constexpr uint64_t YMAX = 65535;
    for (uint64_t a = c0; a < c1; a += YMAX) {
        const uint64_t cn = std::min<uint64_t>(YMAX, c1 - a);
        uint64_t maxRec = 0;
        for (uint64_t c = a; c < a + cn; c++) maxRec = std::max(maxRec, C.nrec[c]);
        if ((maxRec + 255) / 256 > 0x7FFFFFFFull) return fail(SWSEM_EINVAL, "swsem decode: a contig too long for one launch");
        if (!maxRec) continue;
        const dim3 grid((unsigned) ((maxRec + 255) / 256), (unsigned) cn);
        if (masked) {
            const GranuleNeed g = {C.dNeedG.p, C.dNeed.p, C.dGranBase.p, C.granShift};
            k_decode_fill_region<<<grid, dim3(256), 0, h->stream>>>(h->ref, C.params, h->dJobs.p, h->dDecRecs.p, C.dRecBase.p, h->dDecPlan.p, C.dBad.p, h->maxRefLength + REF_SLACK, (uint32_t) a, g);
        } else k_decode_fill<<<grid, dim3(256), 0, h->stream>>>(h->ref, C.params, h->dJobs.p, h->dDecRecs.p, C.dRecBase.p, h->dDecPlan.p, C.dBad.p, h->maxRefLength + REF_SLACK, (uint32_t) a);
    }
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}

// The dependency closure of the contigs whose need bits are set (k_decode_closure): table, times and bitmap go up once, the
// fill units are swept in reverse order, one launch each (slices of 65 535 contigs), back to back on the handle's stream with
// nothing waited for between them; then the bitmap comes down.
int decode_closure(swsem *h, uint64_t refTotalLength, uint64_t nrows, const swsem_prov_row_t *rows, uint64_t ncontigs, const uint64_t *timeOf,
                   uint64_t nunits, const swsem_fill_unit_t *units, uint32_t *need) {
    static_assert(sizeof(ProvRow) == sizeof(swsem_prov_row_t) && sizeof(ProvRow) == 24, "swsem_prov_row_t");
    auto &C = h->chain;
    if (ncontigs != C.n || ncontigs == 0 || ncontigs > 0xFFFFFFFFull) return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: %llu contigs, %llu planned", (unsigned long long) ncontigs, (unsigned long long) C.n);
    if (refTotalLength == 0) return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: reference length");
    for (uint64_t k = 0; k < nrows; k++) {
        if (rows[k].owner >= (int64_t) ncontigs || (k && rows[k].vstart < rows[k - 1].vstart + rows[k - 1].len))
            return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: row %llu of the provenance table is out of order or names no planned contig", (unsigned long long) k);
    }
    for (uint64_t u = 0; u < nunits; u++)
        if (units[u].c0 > units[u].c1 || units[u].c1 > ncontigs) return fail(SWSEM_EINVAL, "swsem_decode_closure_dev: unit %llu leaves the plan", (unsigned long long) u);
    const size_t words = (size_t) ((ncontigs + 31) / 32);
    int r;
    if ((r = C.dProv.reserve(nrows + 1)) || (r = C.dTime.reserve(ncontigs)) || (r = C.dNeed.reserve(words))) return r;
    if (nrows) HIPCHK(hipMemcpyAsync(C.dProv.p, rows, nrows * sizeof(ProvRow), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dTime.p, timeOf, ncontigs * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dNeed.p, need, words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    constexpr uint64_t YMAX = 65535;
    for (uint64_t u = nunits; u-- > 0;) {
        for (uint64_t a = units[u].c0; a < units[u].c1; a += YMAX) {
            const uint64_t cn = std::min<uint64_t>(YMAX, units[u].c1 - a);
            uint64_t maxRec = 0;
            for (uint64_t c = a; c < a + cn; c++) maxRec = std::max(maxRec, C.nrec[c]);
            if ((maxRec + 255) / 256 > 0x7FFFFFFFull) return fail(SWSEM_EINVAL, "swsem decode: a contig too long for one launch");
            if (maxRec) k_decode_closure<<<dim3((unsigned) ((maxRec + 255) / 256), (unsigned) cn), dim3(256), 0, h->stream>>>(h->dDecRecs.p, C.dRecBase.p, h->dDecPlan.p, C.dProv.p, nrows, C.dTime.p, C.dNeed.p, refTotalLength, (uint32_t) a, (uint32_t) units[u].c0);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(need, C.dNeed.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SWSEM_OK;
}

// The closure of `d --region` (k_decode_closure_region): as decode_closure, the need state a bitmap over granules of 2^shift
// bytes (contig c's from bit granBase[c] on) beside the contig bits. Every row and offset is held to the plan before a launch:
// a row that names bytes its owner does not have would set bits of another contig's granules, or beyond the bitmap. Both
// bitmaps stay in the handle for swsem_decode_fill_region_dev.
int decode_closure_region(swsem *h, uint64_t refTotalLength, uint64_t nrows, const swsem_prov_row_region_t *rows, uint64_t ncontigs, const uint64_t *timeOf,
                          uint64_t nunits, const swsem_fill_unit_t *units, uint32_t granuleShift, const uint64_t *granBase, uint32_t *needGranules, uint32_t *needContigs,
                          uint64_t *filledBases) {
    static_assert(sizeof(ProvRowG) == sizeof(swsem_prov_row_region_t) && sizeof(ProvRowG) == 40, "swsem_prov_row_region_t");
    auto &C = h->chain;
    C.regionFor = 0;
    if (ncontigs != C.n || ncontigs == 0 || ncontigs > 0xFFFFFFFFull) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: %llu contigs, %llu planned", (unsigned long long) ncontigs, (unsigned long long) C.n);
    if (refTotalLength == 0) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: reference length");
    if (granuleShift < 4 || granuleShift > 30) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: a granule of 2^%u bytes (16 B to 1 GiB)", granuleShift);
    const uint64_t G = 1ull << granuleShift;
    if (granBase[0] != 0) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: the granule offsets do not start at 0");
    for (uint64_t c = 0; c < ncontigs; c++)
        if (granBase[c + 1] - granBase[c] != (C.destLen[c] + G - 1) / G) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: contig %llu does not have the granules of its length", (unsigned long long) c);
    for (uint64_t k = 0; k < nrows; k++) {
        const swsem_prov_row_region_t &w = rows[k];
        if (w.owner >= (int64_t) ncontigs || (k && w.vstart < rows[k - 1].vstart + rows[k - 1].len))
            return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: row %llu of the provenance table is out of order or names no planned contig", (unsigned long long) k);
        if (w.owner < 0 || w.len == 0) continue;
        const uint64_t n = C.destLen[w.owner];
        const bool inside = w.reversed ? (w.ownerFirst < n && w.len <= w.ownerFirst + 1) : (w.ownerFirst <= n && w.len <= n - w.ownerFirst);
        if (!inside) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: row %llu of the provenance table names bytes its owner does not have", (unsigned long long) k);
    }
    for (uint64_t u = 0; u < nunits; u++)
        if (units[u].c0 > units[u].c1 || units[u].c1 > ncontigs) return fail(SWSEM_EINVAL, "swsem_decode_closure_region_dev: unit %llu leaves the plan", (unsigned long long) u);
    const size_t words = (size_t) ((ncontigs + 31) / 32), gwords = (size_t) ((granBase[ncontigs] + 31) / 32);
    int r;
    if ((r = C.dProvG.reserve(nrows + 1)) || (r = C.dTime.reserve(ncontigs)) || (r = C.dNeed.reserve(words)) || (r = C.dNeedG.reserve(gwords + 3)) || (r = C.dGranBase.reserve(ncontigs + 1))) return r;
    if (nrows) HIPCHK(hipMemcpyAsync(C.dProvG.p, rows, nrows * sizeof(ProvRowG), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dTime.p, timeOf, ncontigs * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dGranBase.p, granBase, (ncontigs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(C.dNeed.p, needContigs, words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (gwords) HIPCHK(hipMemcpyAsync(C.dNeedG.p, needGranules, gwords * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    // (the counter of filled bases: eight bytes behind the bitmap, on an eight-byte boundary)
    unsigned long long *dFilled = (unsigned long long *) (C.dNeedG.p + ((gwords + 1) & ~(size_t) 1));
    HIPCHK(hipMemsetAsync(dFilled, 0, sizeof *dFilled, h->stream));
    constexpr uint64_t YMAX = 65535;
    for (uint64_t u = nunits; u-- > 0;) {
        for (uint64_t a = units[u].c0; a < units[u].c1; a += YMAX) {
            const uint64_t cn = std::min<uint64_t>(YMAX, units[u].c1 - a);
            uint64_t maxRec = 0;
            for (uint64_t c = a; c < a + cn; c++) maxRec = std::max(maxRec, C.nrec[c]);
            if ((maxRec + 255) / 256 > 0x7FFFFFFFull) return fail(SWSEM_EINVAL, "swsem decode: a contig too long for one launch");
            if (maxRec) k_decode_closure_region<<<dim3((unsigned) ((maxRec + 255) / 256), (unsigned) cn), dim3(256), 0, h->stream>>>(h->dDecRecs.p, C.dRecBase.p, h->dDecPlan.p, C.dProvG.p, nrows, C.dTime.p, C.dNeedG.p, C.dNeed.p, C.dGranBase.p, granuleShift, refTotalLength, (uint32_t) a, (uint32_t) units[u].c0, dFilled);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(needContigs, C.dNeed.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (gwords) HIPCHK(hipMemcpyAsync(needGranules, C.dNeedG.p, gwords * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    unsigned long long filled = 0;
    HIPCHK(hipMemcpyAsync(&filled, dFilled, sizeof filled, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (filledBases) *filledBases = filled;
    C.granShift = granuleShift; C.regionFor = C.n;
    return SWSEM_OK;
}

// the planned records of contig c as the plan left them (tests and the host referee of the granule closure)
int decode_copy_records(swsem *h, uint64_t c, swsem_decode_record_t *out, uint64_t cap, uint64_t *n) {
    static_assert(sizeof(DecRec) == sizeof(swsem_decode_record_t) && sizeof(DecRec) == 104, "swsem_decode_record_t");
    auto &C = h->chain;
    if (c >= C.n) return fail(SWSEM_EINVAL, "swsem_debug_copy_records: contig %llu of %llu planned", (unsigned long long) c, (unsigned long long) C.n);
    *n = C.nrec[c];
    const uint64_t m = std::min(cap, C.nrec[c]);
    if (!m) return SWSEM_OK;
    uint64_t base = 0;
    HIPCHK(hipMemcpyAsync(&base, C.dRecBase.p + c, sizeof base, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(out, h->dDecRecs.p + base, m * sizeof(DecRec), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SWSEM_OK;
}

// segments of the decoder's load schedule, in order: what overlaps something queued before it in the call waits for a launch of
// its own (a separator over a loaded byte, a reverse complement that reads what the target has just loaded)
int decode_load(swsem *h, const uint8_t *src, int n, const swsem_load_seg_t *segs) {
    constexpr uint64_t CHUNK = 1 << 15;
    auto &C = h->chain;
    std::vector<LoadSeg> batch;
    std::vector<std::pair<uint64_t, uint64_t>> written;                         // [from, to) of the reference buffer, this launch
    auto flush = [&]() -> int {
        if (batch.empty()) return SWSEM_OK;
        int r = C.dSegs.reserve(batch.size());
        if (r) return r;
        HIPCHK(hipMemcpyAsync(C.dSegs.p, batch.data(), batch.size() * sizeof(LoadSeg), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));                               // (pageable memory; the table is reused by the next launch)
        k_decode_load<<<dim3((unsigned) batch.size()), dim3(256), 0, h->stream>>>(C.dSegs.p, h->lut);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        batch.clear(); written.clear();
        return SWSEM_OK;
    };
    const uint64_t refBytes = h->maxRefLength;
    for (int k = 0; k < n; k++) {
        const swsem_load_seg_t &s = segs[k];
        const bool byte = (s.flags & SWSEM_SEG_BYTE) != 0, fromRef = (s.flags & SWSEM_SEG_FROM_REF) != 0;
        const uint64_t len = byte ? 1 : s.len;
        if (len == 0) continue;
        if (s.dst > refBytes || len > refBytes - s.dst || (fromRef && !byte && (s.src > refBytes || len > refBytes - s.src)))
            return fail(SWSEM_EINVAL, "swsem_decode_load_dev: segment %d leaves the reference buffer", k);
        bool clash = false;
        for (auto &w : written)
            if ((s.dst < w.second && w.first < s.dst + len) || (fromRef && !byte && s.src < w.second && w.first < s.src + len)) { clash = true; break; }
        if (clash || batch.size() + len / CHUNK + 1 > 60000 || written.size() > 4096) { int r = flush(); if (r) return r; }
        written.emplace_back(s.dst, s.dst + len);
        if (byte) { LoadSeg g = {nullptr, h->ref + s.dst, 1, LSEG_BYTE, (uint32_t) (s.src & 0xFF)}; batch.push_back(g); continue; }
        const uint8_t *from = (fromRef ? h->ref : src) + s.src;
        const bool rc = (s.flags & SWSEM_SEG_RC) != 0;
        for (uint64_t o = 0; o < len; o += CHUNK) {
            const uint64_t m = std::min(CHUNK, len - o);
            // (reverse complement: destination bytes [o, o + m) are the complement of source bytes [len - o - m, len - o), backwards)
            LoadSeg g = {rc ? from + (len - o - m) : from + o, h->ref + s.dst + o, m, rc ? (uint32_t) LSEG_RC : 0u, 0u};
            batch.push_back(g);
        }
    }
    return flush();
}

}  // namespace
