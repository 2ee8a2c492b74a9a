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

}  // namespace
