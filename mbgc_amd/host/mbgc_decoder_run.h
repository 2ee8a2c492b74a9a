// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_streams.h): one pass on the device. The provenance table and
// the fill units (host only), and the DecodedCollection: the decoder's handle with the streams, the plan, the load schedule and
// the sequence buffer in HBM, built by plan + schedule, the closure of --select, and the forward run.
#pragma once

namespace {
struct PassTimes { double plan = 0, closure = 0, fill = 0, load = 0; uint64_t waves = 0, widest = 0; };

// ---- the provenance table: whose bytes lie where in the reference buffer, at every moment
// The loader only moves forward, so a load has a virtual position lap x refTotalLength + refPos and the schedule is a table
// sorted by it. Only loads of planned contigs have rows: the initial reference and the separators are nobody's (they cost
// nothing: G0 is literals). A FROM_REF segment (the per-target reverse complement of :608-616) is resolved at once into the
// contigs whose loads wrote its source range, mirrored. THE SUPERSET RULE: a separator that later overwrote one byte of a
// segment (the lazy mode's mark at the lock position) is ignored — the byte keeps its owner; with the read ranges of the
// records, which are the read hull's, the closure that follows from this table may hold more than what is read, never less.
struct Provenance {
    uint64_t L = 0, cur = REF_SHIFT;                               // the loader's virtual position (refPos == L: (lap + 1) x L)
    std::vector<swsem_prov_row_t> rows;
    // --region: which bytes of its owner a row's load wrote — ownerFirst: the owner's byte the load's first byte is made of;
    // reversed: the load ran backwards over the owner (a reverse complement). One entry per row.
    struct Ext { uint64_t ownerFirst; uint32_t reversed; };
    std::vector<Ext> ext;

    // the rows that own a piece of physical range [p0, p1) as the loader left the buffer at virtual position tv: f(physFrom, physTo,
    // row, base) with base + phys = the virtual position. Below the loader's position the bytes are this lap's, from it on the lap
    // before's (before the first lap: never written); a range that straddles the position is split there. (k_decode_closure: the
    // same on the device.)
    template <class F> void queryRows(uint64_t tv, uint64_t p0, uint64_t p1, F f) const {
        if (p1 > L) p1 = L;
        if (p0 >= p1) return;
        const uint64_t lap = tv / L, rp = tv % L;
        auto part = [&](uint64_t a, uint64_t b, uint64_t base) {
            const uint64_t va = base + a, vb = base + b;
            size_t i = (size_t) (std::partition_point(rows.begin(), rows.end(), [&](const swsem_prov_row_t &r) { return r.vstart + r.len <= va; }) - rows.begin());
            for (; i < rows.size() && rows[i].vstart < vb; i++)
                f(std::max(va, rows[i].vstart) - base, std::min(vb, rows[i].vstart + rows[i].len) - base, i, base);
        };
        if (p0 < rp) part(p0, std::min(p1, rp), lap * L);
        if (p1 > rp && lap) part(std::max(p0, rp), p1, (lap - 1) * L);
    }
    // the owned pieces: f(physFrom, physTo, owner)
    template <class F> void query(uint64_t tv, uint64_t p0, uint64_t p1, F f) const {
        queryRows(tv, p0, p1, [&](uint64_t a, uint64_t b, size_t i, uint64_t) { f(a, b, rows[i].owner); });
    }
    // bytes [k0, k0 + n) of row i's load are bytes [*, * + n) of its owner
    uint64_t ownerFrom(size_t i, uint64_t k0, uint64_t n) const { return ext[i].reversed ? ext[i].ownerFirst + 1 - (k0 + n) : ext[i].ownerFirst + k0; }
    // the next segment of the schedule, in serial order; contigs from firstPlanned on are the planned ones (owner = contig - firstPlanned)
    void add(const LoadSegment &s, uint64_t firstPlanned) {
        if (s.length == 0) return;
        if (s.contig == LoadSegment::SEPARATOR && s.length == 1 && (s.refPos + 1) % L == cur % L) return;   // written over the last loaded byte: the superset rule
        const uint64_t v = cur + (s.refPos + L - cur % L) % L;      // the next virtual position that lies at refPos
        if (s.contig == LoadSegment::FROM_REF) {
            std::vector<std::pair<swsem_prov_row_t, Ext>> got;
            queryRows(cur, s.offset, s.offset + s.length, [&](uint64_t a, uint64_t b, size_t i, uint64_t base) {
                const uint64_t at = s.reverseComplement ? s.length - (b - s.offset) : a - s.offset;
                // the same bytes of the same owner, read in the other direction when this load reverses them
                const uint64_t oa = ownerFrom(i, base + a - rows[i].vstart, b - a);
                const uint32_t rev = ext[i].reversed ^ (s.reverseComplement ? 1u : 0u);
                got.push_back({{v + at, b - a, rows[i].owner}, {rev ? oa + (b - a) - 1 : oa, rev}});
            });
            std::sort(got.begin(), got.end(), [](const std::pair<swsem_prov_row_t, Ext> &x, const std::pair<swsem_prov_row_t, Ext> &y) { return x.first.vstart < y.first.vstart; });
            for (const auto &g : got) { rows.push_back(g.first); ext.push_back(g.second); }
        } else if (s.contig >= 0 && (uint64_t) s.contig >= firstPlanned) {
            rows.push_back({v, s.length, (int64_t) ((uint64_t) s.contig - firstPlanned)});
            ext.push_back({s.reverseComplement ? s.offset + s.length - 1 : s.offset, s.reverseComplement ? 1u : 0u});
        }
        cur = v + s.length;
    }
    std::vector<swsem_prov_row_region_t> regionRows() const {
        std::vector<swsem_prov_row_region_t> out(rows.size());
        for (size_t i = 0; i < rows.size(); i++) out[i] = {rows[i].vstart, rows[i].len, rows[i].owner, ext[i].ownerFirst, ext[i].reversed, 0};
        return out;
    }

    // ---- the closure of --region on the host: the referee of k_decode_closure_region, the same rule restated. N: the need state
    // (granBase: bit of every contig's first granule, + 1 entry; gran / contig: the two bitmaps, in: the chosen regions', out: the
    // closure; filled: the bases the needed records write). recs[c]: the plan's records of contig c. The units are swept last
    // first; inside a unit the order is free, since an owner at or behind the unit's first contig is never marked.
    struct RegionNeed { uint32_t shift = 8; std::vector<uint64_t> granBase; std::vector<uint32_t> gran, contig; uint64_t filled = 0; };
    static bool anyGranule(const RegionNeed &N, uint64_t c, uint64_t a, uint64_t b) {             // a byte of [a, b) of contig c in a needed granule
        for (uint64_t g = N.granBase[c] + (a >> N.shift); g <= N.granBase[c] + ((b - 1) >> N.shift); g++) if ((N.gran[g >> 5] >> (g & 31)) & 1u) return true;
        return false;
    }
    void closureRegion(const std::vector<std::vector<swsem_decode_record_t>> &recs, const std::vector<uint64_t> &destLen, const std::vector<uint64_t> &timeOf,
                       const std::vector<swsem_fill_unit_t> &units, RegionNeed &N) const {
        for (size_t u = units.size(); u-- > 0;)
            for (uint64_t c = units[u].c0; c < units[u].c1; c++) {
                if (!((N.contig[c >> 5] >> (c & 31)) & 1u)) continue;
                for (size_t i = 0; i < recs[c].size(); i++) {
                    const swsem_decode_record_t &r = recs[c][i];
                    const uint64_t end = i + 1 < recs[c].size() ? recs[c][i + 1].destAt : destLen[c];
                    if (r.destAt >= end || !anyGranule(N, c, r.destAt, end)) continue;
                    N.filled += end - r.destAt;
                    if (r.flags & 16u) continue;                                                   // (REC_TAIL: literals only)
                    // rec_read_ranges (swsem_decode.hip): the match, the left extension, the right extension a byte wider at either end
                    uint64_t lo[3], hi[3];
                    int n = 0;
                    lo[n] = r.src; hi[n] = r.src + r.len; n++;
                    if (r.leftLen) { lo[n] = (uint64_t) (r.leftSrcMatch - (int64_t) r.leftLen); hi[n] = (uint64_t) r.leftSrcMatch; n++; }
                    if (r.rightLen) {
                        const uint64_t plain = (r.mark - r.litFrom) - r.leftCodes;
                        const int64_t a = (int64_t) (r.destAt + plain + r.leftLen + r.len) + r.offsetDelta - 1;
                        lo[n] = a < 0 ? 0 : (uint64_t) a; hi[n] = lo[n] + r.rightLen + 2; n++;
                    }
                    for (int q = 0; q < n; q++)
                        queryRows(timeOf[c], lo[q], hi[q], [&](uint64_t a, uint64_t b, size_t row, uint64_t base) {
                            const int64_t o = rows[row].owner;
                            if (o < 0 || (uint64_t) o >= units[u].c0) return;
                            const uint64_t oa = ownerFrom(row, base + a - rows[row].vstart, b - a), ob = oa + (b - a);
                            N.contig[o >> 5] |= 1u << (o & 31);
                            for (uint64_t g = N.granBase[o] + (oa >> N.shift); g <= N.granBase[o] + ((ob - 1) >> N.shift); g++) N.gran[g >> 5] |= 1u << (g & 31);
                        });
                }
            }
    }
};

// ---- the fill units: what is filled by one launch, and the loads that follow it. A wave — targets [t0, t1) whose contigs
// stand against the same frozen buffer, all their segments behind the fill — or one contig of a target that goes alone with
// segments [sA, sB) of that target (c0 == c1: a target without a contig, only its segments). counted: the targets the unit
// adds to the `waves:` line (a target that goes alone counts once, on its first unit).
struct FillUnit { uint64_t c0, c1; size_t t0, t1, sA, sB; uint64_t counted; bool wave; };

// The partition of the targets into fill units, from the plan's read hulls and the load schedule alone.
// segAt[t][i]: segments [segAt[t][i], segAt[t][i + 1]) of target t belong to its contig i; what follows its last contig goes
// with that one — a separator written at the lock position goes with the contig whose load reached it.
std::vector<FillUnit> partitionUnits(const std::vector<uint32_t> &seqCount, const std::vector<uint64_t> &lock, const std::vector<std::vector<LoadSegment>> &tSegs,
                                     const std::vector<swsem_chain_contig_t> &cc, uint64_t g0n, bool everyContigAlone, std::vector<std::vector<size_t>> &segAt) {
    const size_t T = seqCount.size();
    std::vector<FillUnit> units;
    segAt.assign(T, std::vector<size_t>());
    std::vector<Interval> written;                                                              // what the current wave's loads will write
    auto addWrites = [&](std::vector<Interval> &w, const std::vector<LoadSegment> &segs, size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            if (!w.empty() && w.back().to == segs[i].refPos) w.back().to += segs[i].length;
            else w.push_back({segs[i].refPos, segs[i].refPos + segs[i].length});
        }
    };
    auto reads = [&](const std::vector<Interval> &w, uint64_t c) {
        if (cc[c].minSrc >= cc[c].maxSrcEnd) return false;
        for (const Interval &i : w) if (cc[c].minSrc < i.to && i.from < cc[c].maxSrcEnd) return true;
        return false;
    };
    FillUnit wave = {};
    uint64_t waveLock = 0;
    auto closeWave = [&]() { if (wave.counted) units.push_back(wave); wave = FillUnit(); written.clear(); };
    uint64_t c = 0;
    for (size_t t = 0; t < T; t++) {
        const uint64_t c1 = c + seqCount[t];
        const std::vector<LoadSegment> &segs = tSegs[t];
        std::vector<size_t> &at = segAt[t];
        at.assign(seqCount[t] + 1, segs.size());
        {
            size_t lastOwn = 0;                                                                 // behind the last segment that is a contig's
            for (size_t i = 0; i < segs.size(); i++) if (segs[i].contig >= 0) lastOwn = i + 1;
            size_t i = 0;
            for (uint32_t s = 0; s < seqCount[t]; s++) {
                at[s] = i;
                if (s + 1 == seqCount[t]) break;
                while (i < lastOwn && (segs[i].contig < 0 || segs[i].contig <= (int64_t) (g0n + c + s))) i++;
            }
        }
        // Every target of an encoder round holds one lock position and was matched against the buffer the round found: it may be
        // filled beside the targets in front of it as long as nothing it reads is written by their loads. -t1 streams carry the
        // window's end 0 (no window): contig c + 1 may match contig c, the target goes alone, contig by contig.
        bool side = !everyContigAlone && lock[t] != 0;
        std::vector<Interval> own;
        for (uint32_t s = 0; side && s < seqCount[t]; s++) {
            if (reads(own, c + s)) side = false;
            addWrites(own, segs, at[s], at[s + 1]);
        }
        bool join = side && wave.counted && lock[t] == waveLock;
        for (uint64_t k = c; join && k < c1; k++) if (reads(written, k)) join = false;
        if (!join) closeWave();
        if (side) {
            if (!wave.counted) { wave.c0 = c; wave.t0 = t; wave.wave = true; waveLock = lock[t]; }
            wave.c1 = c1; wave.t1 = t + 1; wave.counted++;
            addWrites(written, segs, 0, segs.size());
        } else {
            for (uint32_t s = 0; s < seqCount[t]; s++) units.push_back({c + s, c + s + 1, t, t + 1, at[s], at[s + 1], s == 0 ? 1u : 0u, false});
            if (seqCount[t] == 0) units.push_back({c, c, t, t + 1, 0, segs.size(), 1, false});
        }
        c = c1;
    }
    closeWave();
    return units;
}

bool hipFail(std::string &msg, const char *what) { msg = std::string(what) + ": " + swsem_last_error(); return false; }

// ---- a collection decoded into HBM: the owner of the decoder's handle and of every device pointer of a pass (--bench: each of
// the two passes has a fresh one). Freed on every way out, the pointers before the handle.
struct DecodedCollection {
    swsem_t *h = nullptr;
    std::vector<void *> ptrs;
    const uint8_t *sdev[SWSEM_NSTREAMS] = {};                      // the streams
    std::vector<swsem_chain_contig_t> cc;                          // the plan, per planned contig
    std::vector<uint64_t> contigLen;                               // per contig of the collection, G0's first
    std::vector<LoadSegment> g0Segs;
    std::vector<std::vector<LoadSegment>> tSegs;                   // the load schedule, per target
    std::vector<std::vector<size_t>> segAt;
    std::vector<FillUnit> units;
    std::vector<uint8_t> mark;                                     // per planned contig: 0 = not filled, 1 = filled as a dependency, 2 = filled because selected
    std::vector<char> targetRuns;                                  // per target: any of its contigs is filled
    std::vector<uint64_t> seqOff;                                  // the sequence buffer: G0, then the contigs that are filled
    uint8_t *seqDev = nullptr;
    uint64_t totalBases = 0;
    PassTimes times;
    uint64_t closureContigs = 0, closureBases = 0, dependencyTargets = 0;
    int sentinel = -1;                                             // tests: the sequence buffer starts as this byte everywhere
    bool region = false;                                           // --region: the fills are masked by the granule bitmap the closure left in the handle
    Provenance::RegionNeed regionNeed;                             // ... as it came back from the device
    std::vector<uint64_t> timeOf;                                  // (kept for the referee: mbgc_decoder_region_probe)
    Provenance prov;

    DecodedCollection() = default;
    DecodedCollection(const DecodedCollection &) = delete;
    DecodedCollection &operator=(const DecodedCollection &) = delete;
    ~DecodedCollection() { for (void *p : ptrs) if (p) swsem_dev_free(h, p); if (h) swsem_destroy(h); }

    bool upload(const StreamSet &S, int device, std::string &msg);
    bool planAndSchedule(const StreamSet &S, bool serial, std::string &msg);
    bool closure(const StreamSet &S, const Selection &sel, std::string &msg);
    std::vector<swsem_fill_unit_t> sweepUnits() const { std::vector<swsem_fill_unit_t> out; for (const FillUnit &u : units) if (u.c1 > u.c0) out.push_back({u.c0, u.c1}); return out; }
    bool forwardRun(const StreamSet &S, bool selecting, std::string &msg);

private:
    void toAbi(const std::vector<LoadSegment> &in, size_t a, size_t b, bool targetRuns, uint64_t g0n, std::vector<swsem_load_seg_t> &out) const;
    bool load(std::vector<swsem_load_seg_t> &segs);
    bool fill(uint64_t c0, uint64_t c1, uint64_t g0n, std::string &msg);
};

// the handle, and the streams in HBM
bool DecodedCollection::upload(const StreamSet &S, int device, std::string &msg) {
    if (swsem_create_decoder(&h, S.meta.maxRefLength, device)) return hipFail(msg, "decoder");
    for (int s = 0; s < SWSEM_NSTREAMS; s++) {
        void *p = nullptr;
        if (swsem_dev_malloc(h, S.sizes[s] + 64, &p)) return hipFail(msg, "streams");
        ptrs.push_back(p);
        if (swsem_dev_upload(h, p, S.stream[s].data(), S.sizes[s])) return hipFail(msg, "streams");
        sdev[s] = (const uint8_t *) p;
    }
    return true;
}

// the plan: once, ahead, for the whole collection; the load schedule: complete before a base exists; the fill units
bool DecodedCollection::planAndSchedule(const StreamSet &S, bool serial, std::string &msg) {
    const MbgcMeta &meta = S.meta;
    const size_t T = S.T();
    const uint64_t planned = S.planned, g0n = S.g0n;
    cc.resize(planned);
    int firstBad = -1;
    const double t0 = nowMs();
    if (planned && swsem_decode_plan_chain_dev(h, &meta.emit, sdev, S.sizes, (int) S.starts.size(), S.starts.data(), (int) T, S.seqCount.data(), S.lock.data(), planned, cc.data(), &firstBad))
        return hipFail(msg, "plan");
    times.plan = nowMs() - t0;
    if (firstBad >= 0) {
        msg = "malformed stream set: " + (S.useIndex ? "target " + std::to_string(firstBad) + " does not decode from its offsets to the next target's"
                                                      : std::string("the collection's chain does not end with its streams")) + " (a stream ran out, or bytes were left over)";
        return false;
    }
    for (uint64_t c = 0; c < planned; c++) if (cc[c].unmatched < 0) { msg = "malformed stream set: contig " + std::to_string(c) + " was not reached"; return false; }
    contigLen = S.g0ContigLen;
    for (uint64_t c = 0; c < planned; c++) contigLen.push_back(cc[c].destLen);
    MBGC_Decoder::RefState st;
    st.refTotalLength = meta.maxRefLength; st.lazyDecompressionSupport = S.lazy;
    if (!MBGC_Decoder::scheduleG0(st, S.g0Bytes, meta.rcInReference, meta.sequentialMatching, g0Segs)) { msg = "malformed stream set: the initial reference does not fit the buffer"; return false; }
    tSegs.assign(T, std::vector<LoadSegment>());
    uint64_t c = 0;
    for (size_t t = 0; t < T; t++) {
        std::vector<MBGC_Decoder::ContigInfo> info(S.seqCount[t]);
        for (uint32_t s = 0; s < S.seqCount[t]; s++) info[s] = {cc[c + s].destLen, (uint64_t) cc[c + s].unmatched};
        const uint64_t before = st.loaded();
        if (!MBGC_Decoder::scheduleTarget(st, g0n + c, info, meta.targets[t].unmatchedFractionFactor, meta.targets[t].unmatchedFractionRCFactor, meta.rcInReference,
                                          meta.contigsIndividuallyReversed, S.lock[t], tSegs[t])) {
            msg = "malformed stream set: the loads of target " + std::to_string(t) + " do not fit its lock position";
            return false;
        }
        if (S.lazy && st.loaded() - before != S.extSize[t]) {
            msg = "malformed stream set: target " + std::to_string(t) + " extends the reference by " + std::to_string(st.loaded() - before) +
                  " bytes, refExtSize says " + std::to_string(S.extSize[t]);
            return false;
        }
        c += S.seqCount[t];
    }
    if (st.reachedRefLengthCount != meta.reachedRefLengthCount || (meta.finalRefLength && (st.reachedRefLengthCount ? st.refTotalLength : st.refPos) != meta.finalRefLength)) {
        msg = "malformed stream set: the rebuilt reference ends at " + std::to_string(st.refPos) + " after " + std::to_string(st.reachedRefLengthCount) +
              " laps, the encoder's at " + std::to_string(meta.finalRefLength) + " after " + std::to_string(meta.reachedRefLengthCount);
        return false;
    }
    // waves: targets whose contigs stand against the same frozen buffer are filled by one launch
    units = partitionUnits(S.seqCount, S.lock, tSegs, cc, g0n, serial || meta.sequentialMatching, segAt);
    return true;
}

// what is filled: everything, or the closure of the chosen units (--select) or records (--select-seq), before a base exists
bool DecodedCollection::closure(const StreamSet &S, const Selection &sel, std::string &msg) {
    const size_t T = S.T();
    const uint64_t planned = S.planned, g0n = S.g0n;
    mark.assign(planned, sel.selecting ? 0 : 2);
    targetRuns.assign(T, 1);
    if (!sel.selecting) return true;
    std::vector<uint32_t> need((planned + 31) / 32, 0);
    timeOf.assign(planned, 0);
    const double t0 = nowMs();
    prov = Provenance();
    prov.L = S.meta.maxRefLength;
    for (const LoadSegment &s : g0Segs) prov.add(s, g0n);
    uint64_t c = 0;
    for (size_t t = 0; t < T; t++) {
        // a contig's time: the loader's position just before its own first load in serial order — the state --serial fills it against
        uint32_t s = 0;
        for (size_t i = 0; i <= tSegs[t].size(); i++) {
            for (; s < S.seqCount[t] && segAt[t][s] == i; s++) timeOf[c + s] = prov.cur;
            if (i < tSegs[t].size()) prov.add(tSegs[t][i], g0n);
        }
        for (uint32_t k = 0; k < S.seqCount[t]; k++) if (sel.chosen(t, c + k, g0n)) { mark[c + k] = 2; need[(c + k) >> 5] |= 1u << ((c + k) & 31); }
        c += S.seqCount[t];
    }
    const std::vector<swsem_fill_unit_t> sweep = sweepUnits();
    if (sel.selectingRegion) {
        // --region: the need state is a bitmap over granules; the chosen pieces' granules go in, the closure's come back, and the
        // contig bits with them. A chosen record without a piece in range (every region behind its end) needs nothing.
        region = true;
        Provenance::RegionNeed &N = regionNeed;
        N = Provenance::RegionNeed();
        N.shift = sel.granuleShift;
        N.granBase.assign(planned + 1, 0);
        for (uint64_t k = 0; k < planned; k++) N.granBase[k + 1] = N.granBase[k] + ((contigLen[g0n + k] + (1ull << N.shift) - 1) >> N.shift);
        N.gran.assign((N.granBase[planned] + 31) / 32 + 1, 0);
        std::fill(need.begin(), need.end(), 0u);
        for (const RegionPiece &p : sel.pieces) {
            if (p.contig < g0n || !p.len) continue;
            const uint64_t k = p.contig - g0n;
            need[k >> 5] |= 1u << (k & 31);
            for (uint64_t g = N.granBase[k] + (p.from >> N.shift); g <= N.granBase[k] + ((p.from + p.len - 1) >> N.shift); g++) N.gran[g >> 5] |= 1u << (g & 31);
        }
        N.contig = need;
        const std::vector<swsem_prov_row_region_t> rows = prov.regionRows();
        if (planned && swsem_decode_closure_region_dev(h, prov.L, rows.size(), rows.data(), planned, timeOf.data(), sweep.size(), sweep.data(), N.shift, N.granBase.data(),
                                                       N.gran.data(), N.contig.data(), &N.filled))
            return hipFail(msg, "closure");
        need = N.contig;
        // (a chosen contig that needs nothing is not filled: its mark is for --closure-out, which counts filled bytes)
        for (uint64_t k = 0; k < planned; k++) if (mark[k] == 2 && !((need[k >> 5] >> (k & 31)) & 1u)) mark[k] = 0;
    } else if (planned && swsem_decode_closure_dev(h, prov.L, prov.rows.size(), prov.rows.data(), planned, timeOf.data(), sweep.size(), sweep.data(), need.data()))
        return hipFail(msg, "closure");
    times.closure = nowMs() - t0;
    c = 0;
    for (size_t t = 0; t < T; t++) {
        bool any = false;
        for (uint32_t k = 0; k < S.seqCount[t]; k++, c++) {
            if (!mark[c] && ((need[c >> 5] >> (c & 31)) & 1u)) mark[c] = 1;
            if (mark[c]) { any = true; closureContigs++; closureBases += region ? 0 : contigLen[g0n + c]; }
        }
        targetRuns[t] = any;
        if (any && !sel.unitSel[t + 1]) dependencyTargets++;
    }
    if (region) closureBases = regionNeed.filled;                  // the bases actually filled
    return true;
}

// segments [a, b) of a schedule as the device takes them. (A selection: only the segments whose contig is filled are loaded —
// separators and G0 always, a target's own reverse complement when any of its contigs is filled; what is left out is read by
// nothing that is filled)
void DecodedCollection::toAbi(const std::vector<LoadSegment> &in, size_t a, size_t b, bool targetRuns, uint64_t g0n, std::vector<swsem_load_seg_t> &out) const {
    for (size_t i = a; i < b; i++) {
        const LoadSegment &s = in[i];
        swsem_load_seg_t g = {};
        g.dst = s.refPos; g.len = s.length;
        if (s.contig == LoadSegment::SEPARATOR) { g.flags = SWSEM_SEG_BYTE; g.src = REF_REGION_SEPARATOR; }
        else if (s.contig == LoadSegment::FROM_REF) { if (!targetRuns) continue; g.flags = SWSEM_SEG_FROM_REF | (s.reverseComplement ? SWSEM_SEG_RC : 0); g.src = s.offset; }
        else {
            if ((uint64_t) s.contig >= g0n && !mark[s.contig - g0n]) continue;
            g.flags = s.reverseComplement ? SWSEM_SEG_RC : 0; g.src = seqOff[s.contig] + s.offset;
        }
        out.push_back(g);
    }
}
bool DecodedCollection::load(std::vector<swsem_load_seg_t> &segs) {
    if (segs.empty()) return true;
    const double a = nowMs();
    const int r = swsem_decode_load_dev(h, seqDev, (int) segs.size(), segs.data());
    times.load += nowMs() - a;
    segs.clear();
    return r == 0;
}
// planned contigs [c0, c1)
bool DecodedCollection::fill(uint64_t c0, uint64_t c1, uint64_t g0n, std::string &msg) {
    if (c1 == c0) return true;
    const double a = nowMs();
    uint64_t nbad = 0;
    const int r = region ? swsem_decode_fill_region_dev(h, c0, c1, seqDev, seqOff.data() + g0n, &nbad) : swsem_decode_fill_range_dev(h, c0, c1, seqDev, seqOff.data() + g0n, &nbad);
    times.fill += nowMs() - a;
    if (r) return hipFail(msg, "fill");
    if (nbad) { msg = "malformed stream set: the bytes of a contig do not come out as planned"; return false; }
    return true;
}

// the sequence buffer — HBM and the download scale with the closure —, G0's copy, and the forward run: every unit's fill, then its
// loads (a selection: the runs of filled contigs inside the unit, one launch each)
bool DecodedCollection::forwardRun(const StreamSet &S, bool selecting, std::string &msg) {
    const uint64_t g0n = S.g0n, N = g0n + S.planned;
    seqOff.assign(N + 1, 0);
    for (uint64_t c = 0; c < N; c++) seqOff[c + 1] = seqOff[c] + (c < g0n || mark[c - g0n] ? contigLen[c] : 0);
    totalBases = seqOff[N];
    void *seqp = nullptr;
    if (swsem_dev_malloc(h, totalBases + 64, &seqp)) return hipFail(msg, "sequences");
    ptrs.push_back(seqp);
    seqDev = (uint8_t *) seqp;
    if (sentinel >= 0 && totalBases) {
        const std::string fillBytes(totalBases, (char) sentinel);
        if (swsem_dev_upload(h, seqDev, fillBytes.data(), totalBases)) return hipFail(msg, "sequences");
    }
    uint64_t at = 0;                                               // G0's bytes are literals
    for (uint64_t g = 0; g < g0n; g++) {
        if (swsem_dev_copy(h, seqDev + seqOff[g], sdev[SWSEM_LIT] + at, contigLen[g])) return hipFail(msg, "initial reference");
        at += contigLen[g] + 1;
    }
    std::vector<swsem_load_seg_t> abi;
    toAbi(g0Segs, 0, g0Segs.size(), true, g0n, abi);
    if (!load(abi)) return hipFail(msg, "initial reference");
    for (const FillUnit &u : units) {
        for (uint64_t c = u.c0; c < u.c1;) {
            if (!mark[c]) { c++; continue; }
            uint64_t e = c;
            while (e < u.c1 && mark[e]) e++;
            if (!fill(c, e, g0n, msg)) return false;
            c = e;
        }
        uint64_t width = 0;
        for (size_t t = u.t0; t < u.t1; t++) {
            toAbi(tSegs[t], u.wave ? 0 : u.sA, u.wave ? tSegs[t].size() : u.sB, targetRuns[t], g0n, abi);
            width += targetRuns[t] ? 1 : 0;
        }
        if (!load(abi)) return hipFail(msg, "load");
        if (!selecting) width = u.counted;
        if (u.counted && width) { times.waves++; times.widest = std::max(times.widest, width); }
    }
    if (swsem_synchronize(h)) return hipFail(msg, "decode");
    return true;
}
}  // namespace
