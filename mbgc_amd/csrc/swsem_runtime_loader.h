// Part of swsem_runtime.hip: staged small copies, the loader (loadRef, loadSeparator, the worker locks), the insertion
// it collects per finalize, and — because the loader's write guard is one of those who hand them over — the deferred
// byte automata of an emission.
namespace {

// Small copies between host and device go through pinned host memory that is mapped into the device's address
// space and are made by a kernel (the runtime's own small copies can block the calling thread for milliseconds on a
// side stream, and switch engines in the middle of the main one). They are staged and leave in one launch per
// flush_copies(): up to CopySegs::MAX segments, zero-fills among them.
int flush_copies(swsem *h) {
    CopySegs &sg = h->segs;
    if (sg.n == 0) return SWSEM_OK;
    const uint32_t blocks = sg.first[sg.n];
    k_copy_segs<<<dim3(blocks), dim3(256), 0, h->segStream>>>(sg);
    sg.n = 0;
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}
int stage_copy(swsem *h, void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (!bytes) return SWSEM_OK;
    CopySegs &sg = h->segs;
    if (sg.n && (h->segStream != st || sg.n == CopySegs::MAX)) { int r = flush_copies(h); if (r) return r; }
    if (sg.n == 0) { h->segStream = st; sg.first[0] = 0; }
    sg.dst[sg.n] = (uint8_t *) dst; sg.src[sg.n] = (const uint8_t *) src; sg.bytes[sg.n] = bytes;
    sg.first[sg.n + 1] = sg.first[sg.n] + (uint32_t) ((bytes + 4095) / 4096);
    sg.n++;
    return SWSEM_OK;
}
// device results -> pinned host memory; visible to the host once an event recorded behind the flush has completed
int download(swsem *h, void *dstPinned, const void *srcDev, size_t bytes, hipStream_t st) { return stage_copy(h, dstPinned, srcDev, bytes, st); }
int zero_dev(swsem *h, void *dst, size_t bytes, hipStream_t st) { return stage_copy(h, dst, nullptr, bytes, st); }

// host data -> device through the pinned ring (staged: flush_copies() launches)
int upload(swsem *h, void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (!bytes) return SWSEM_OK;
    const size_t need = (bytes + 255) & ~(size_t) 255;
    if (need * 4 > h->ring.cap) {                      // (re)allocation: rare, and the only place that waits
        int r = flush_copies(h);
        if (r) return r;
        HIPCHK(hipDeviceSynchronize());
        if ((r = h->ring.reserve(need * 4, std::max<size_t>(need * 8, 8u << 20)))) return r;
        h->ringAt = 0;
    }
    if (h->ringAt + need > h->ring.cap) {              // wrap: everything staged a lap ago has long been copied, but make sure
        { int r = flush_copies(h); if (r) return r; }
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipStreamSynchronize(h->stream2));
        if (h->stream3) HIPCHK(hipStreamSynchronize(h->s3()));
        HIPCHK(hipStreamSynchronize(h->streamUp));
        HIPCHK(hipStreamSynchronize(h->streamAux));
        h->ringAt = 0;
    }
    uint8_t *slot = h->ring.p + h->ringAt;
    h->ringAt += need;
    memcpy(slot, src, bytes);
    return stage_copy(h, dst, slot, bytes, st);
}

// The byte automata of an emission's second phase (sizes .. write), the copy of its results and its completion event, on
// the second stream. Queued with the emission they become ready when the finalize ends — the moment the next batch's resolve
// does — and whichever was dealt the wave slots first ran at the other's expense: the resolve took 2.8 ms instead of 2.1
// when it lost (steps of 3.1 and 3.9 ms, the slow kind in 40 % of the steps on the 4.35e9-byte sizing). So they are kept
// back until the next resolve kernel has been launched (batch_launch; `gated`: the caller has made the second stream wait for
// the event recorded just before that launch), or until somebody needs the emission's results.
int run_phase2b(swsem *h, EmitSlot &E, bool gated) {
    if (!E.deferred2b) return SWSEM_OK;
    E.deferred2b = false;
    if (E.waitFin2b && !gated) {                                     // behind the finalize's last kernel (everything queued so far)
        HIPCHK(hipEventRecord(h->evFin, h->stream));
        HIPCHK(hipStreamWaitEvent(h->stream2, h->evFin, 0));
    }
    HIPCHK(hipStreamWaitEvent(h->stream2, E.evMetaDone, 0));          // the pairing kernels' results (their own stream)
    const EmitView &v = E.v2b;
    const dim3 grid2(E.grid2b);
    const int n = E.n2b;
    h->mark(SWSEM_K_EMIT2, true, h->stream2);
    // (few chunks: a quarter of the tasks per wave, four times the waves — swsem_emit.hip, chunk_task)
    const bool thin = E.grid2b <= EMIT_THIN_MAX;
    if (thin) k_emit_sizes<4><<<grid2, dim3(1024), 0, h->stream2>>>(v, E.dECg.p);
    else k_emit_sizes<1><<<grid2, dim3(256), 0, h->stream2>>>(v, E.dECg.p);
    k_emit_place_sums<<<grid2, dim3(CH), 0, h->stream2>>>(v, E.dECg.p);
    k_emit_place_scan<<<dim3(n), dim3(CH), 0, h->stream2>>>(v, E.dECg.p);
    k_emit_packoffs<<<1, dim3(CH), 0, h->stream2>>>(v);
    k_emit_place_final<<<grid2, dim3(CH), 0, h->stream2>>>(v, E.dECg.p);
    if (thin) k_emit_write<4><<<grid2, dim3(1024), 0, h->stream2>>>(v, E.dECg.p);
    else k_emit_write<1><<<grid2, dim3(256), 0, h->stream2>>>(v, E.dECg.p);
    k_emit_copy_long<<<dim3(512), dim3(256), 0, h->stream2>>>(v);
    h->mark(SWSEM_K_EMIT2, false, h->stream2);
    HIPCHK(hipGetLastError());
    int r2;
    if ((r2 = flush_copies(h)) || (r2 = download(h, E.pinE.p, E.dEOut.p, (size_t) n * sizeof(EmitOut), h->stream2)) || (r2 = flush_copies(h))) return r2;
    HIPCHK(hipEventRecord(E.evDone, h->stream2));
    E.donePending = false;
    return SWSEM_OK;
}

// An emission whose second phase is still running reads reference bytes next to its matches. It never reads inside
// its own lock window [loading position it started at, its matching-lock position): candidates there were refused
// at match time (.cpp:212-220), pairs do not span the lock (TextMatchers.h:46-50), the right extension stops at the
// loading position and the left one at the lock (ENC.cpp:318-335, :379-384) — that window exists so that the
// reference's loader can write while its workers read, and loadRef never writes beyond it (.cpp:408-414). So a write
// that stays inside an emission's window runs beside it, wrap or not (tests/test_gpu_lock_window.py fills the window
// with garbage and emits again: same bytes); any other write — the separator that replaces the last loaded byte at
// the window's end, a write outside the window of an older emission, contigs without a lock — waits for the emission.
int ref_write_guard(swsem *h, uint64_t firstByte, uint64_t lastByte) {
    const int laps = h->ld.laps;
    for (auto &E : h->slot) {
        if (!E.outstanding || E.refGuarded) continue;
        bool inside = false;
        if (E.lockMin != UINT64_MAX && firstByte >= REF_SHIFT && lastByte >= firstByte) {
            if (E.lockMin > E.emitPos1)                              // window [emitPos1, lockMin)
                inside = laps == E.emitLaps && firstByte >= E.emitPos1 && lastByte < E.lockMin;
            else                                                     // it wraps: [emitPos1, end) and, a lap later, [1, lockMin)
                inside = (laps == E.emitLaps && firstByte >= E.emitPos1) || (laps == E.emitLaps + 1 && lastByte < E.lockMin);
        }
        const bool appendOnly = laps == 0 && firstByte >= E.emitPos1;      // nothing was ever written there: nothing to read
        if (!inside && !appendOnly) {
            if (E.deferred2b) { int d = run_phase2b(h, E, false); if (d) return d; }   // (its automata had not been queued yet)
            if (E.donePending) return SWSEM_ESPEC;                   // (only while a speculative finalize is being queued: it is given up)
            HIPCHK(hipStreamWaitEvent(h->stream, E.evDone, 0));
            E.refGuarded = true;
        }
    }
    return SWSEM_OK;
}

// The lap-tag summary (RefView::tagSum) is kept from the loader's own arithmetic. A step that writes text [lo, hi) and samples
// S + t k1 (t < nMain), T + u k1 (u < nTail) touches the slots whose K-mer reaches into the text and the slots whose tag it
// writes (on-grid samples only: k_insert, k_insert_multi). Of the coarse blocks that hold a touched slot, those whose every slot
// lies in the on-grid main run end up with the lap's tag in all of tags[]: they become uniform. Every other one — the piece's
// edges, its tail samples, a main run off the grid (the stretch after a wrap, which writes no tag at all) — becomes mixed. The
// spans only collect here; plan_tag_summary turns the spans of one flush into the runs k_set_tagsum writes.
void note_piece(swsem *h, uint64_t lo, uint64_t hi, uint64_t S, uint64_t nMain, uint64_t T, uint64_t nTail, uint32_t tag) {
    if (!h->tagSum) return;
    const int ord = h->k1ord, sh = h->tagSumShift;
    const uint64_t grid = (1ull << ord) - 1;
    uint64_t s0 = UINT64_MAX, s1 = 0;                                 // touched slots [s0, s1]
    auto touch = [&](uint64_t a, uint64_t b) { s0 = std::min(s0, a); s1 = std::max(s1, b); };
    if (hi > lo) touch((lo >= (uint64_t) h->K ? lo - h->K + 1 : 0) >> ord, (hi - 1) >> ord);
    const bool mainOnGrid = nMain && (S & grid) == 0;
    if (mainOnGrid) touch(S >> ord, (S >> ord) + nMain - 1);
    if (nTail && (T & grid) == 0) touch(T >> ord, (T >> ord) + nTail - 1);
    if (s0 > s1) return;
    const uint64_t b0 = s0 >> sh, b1 = (s1 >> sh) + 1;                // touched blocks [b0, b1)
    uint64_t u0 = b1, u1 = b1;                                        // of them uniform: [u0, u1)
    if (mainOnGrid && tag != swk::TAGSUM_MIXED) {
        const uint64_t a = S >> ord, b = a + nMain;
        u0 = (a + (1ull << sh) - 1) >> sh; u1 = b >> sh;
        if (u1 <= u0) u0 = u1 = b1;
    }
    if (u0 > b0) h->sumMixed.push_back({b0, u0, swk::TAGSUM_MIXED});
    if (u1 > u0) h->sumUniform.push_back({u0, u1, tag});
    if (b1 > u1) h->sumMixed.push_back({u1, b1, swk::TAGSUM_MIXED});
}
// one byte at `at` changes without a sample (a separator; k_mark_stale clears the tag of the slot whose K-mer ends there)
void note_byte(swsem *h, uint64_t at) {
    if (!h->tagSum) return;
    const uint64_t s0 = (at >= (uint64_t) h->K ? at - h->K + 1 : 0) >> h->k1ord, s1 = at >> h->k1ord;
    h->sumMixed.push_back({s0 >> h->tagSumShift, (s1 >> h->tagSumShift) + 1, swk::TAGSUM_MIXED});
}
// The spans of one flush as runs that do not overlap: a block that two steps of the flush touch is mixed, whatever either
// says (the one case that could be uniform — a later step's main run covering all of it — is given up: mixed is always safe).
void plan_tag_summary(swsem *h, std::vector<SumRun> &runs) {
    runs.clear();
    auto &U = h->sumUniform, &M = h->sumMixed;
    for (size_t i = 0; i < U.size(); i++)
        for (size_t j = i + 1; j < U.size(); j++)
            if (U[i].a < U[j].b && U[j].a < U[i].b) M.push_back({std::max(U[i].a, U[j].a), std::min(U[i].b, U[j].b), swk::TAGSUM_MIXED});
    std::sort(M.begin(), M.end(), [](const swsem::SumSpan &x, const swsem::SumSpan &y) { return x.a < y.a; });
    size_t nm = 0;                                                    // merged in place
    for (size_t i = 0; i < M.size(); i++) {
        if (nm && M[i].a <= M[nm - 1].b) M[nm - 1].b = std::max(M[nm - 1].b, M[i].b);
        else M[nm++] = M[i];
    }
    M.resize(nm);
    const uint64_t end = h->tagSumEntries;
    auto push = [&](uint64_t a, uint64_t b, uint32_t val) {
        b = std::min(b, end);
        if (a < b) runs.push_back({(uint32_t) a, (uint32_t) (b - a), val, 0u});
    };
    for (auto &u : U) {
        uint64_t cur = u.a;
        for (auto &m : M) {
            if (m.b <= cur) continue;
            if (m.a >= u.b) break;
            push(cur, std::min(m.a, u.b), u.val);                     // (nothing when m.a <= cur)
            cur = std::max(cur, m.b);
        }
        push(cur, u.b, u.val);
    }
    for (auto &m : M) push(m.a, m.b, swk::TAGSUM_MIXED);
    U.clear(); M.clear();
}

// processIgnoreCollisionsRef (.cpp:146-171): derive the two sample sets and launch one insertion. [lo, hi): the text the
// step has just written (src: where its bytes come from, when the insertion may hash them from there).
int insert_samples(swsem *h, const uint8_t *src = nullptr, uint64_t lo = 0, uint64_t hi = 0) {
    LoaderState &ld = h->ld;
    const int64_t STEP = (int64_t) h->k1 * 128;
    const int64_t E = ld.pos1 - h->K;
    const int64_t S = (int64_t) ld.samplingPos;
    uint64_t nMain = 0;
    if (S < E - STEP) {
        const int64_t blocks = ((E - STEP) - S + STEP - 1) / STEP;
        nMain = (uint64_t) blocks * 128;
    }
    const int64_t T = h->k1 + ((E - 1) / STEP) * STEP;
    uint64_t nTail = 0;
    if (T < E + 1) nTail = (uint64_t) ((E - T) / h->k1 + 1);
    const uint64_t total = nMain + nTail;
    note_piece(h, lo, hi, (uint64_t) S, nMain, (uint64_t) T, nTail, swk::lap_tag(ld.laps));
    if (total && h->deferInserts) {
        InsertPiece pc;
        pc.S = (uint64_t) S; pc.nMain = nMain; pc.T = (uint64_t) T; pc.nTail = nTail; pc.epoch = ld.epoch; pc.tag = swk::lap_tag(ld.laps);
        pc.src = src; pc.lo = lo; pc.hi = hi;                       // reference positions [lo, hi) will hold src[0 .. hi - lo)
        h->pendingPieces.push_back(pc);
    } else if (total) {
        h->mark(SWSEM_K_INSERT, true);
        k_insert<<<dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, h->stream>>>(
            h->ref, h->ht, (uint64_t) S, nMain, (uint64_t) T, nTail, h->k1, h->k1ord, h->K, h->mask, ld.epoch, h->fpBits, h->tags, swk::lap_tag(ld.laps));
        h->mark(SWSEM_K_INSERT, false);
        HIPCHK(hipGetLastError());
    }
    ld.epoch += 2;
    if (ld.epoch >= (1u << (32 - h->fpBits)) - 2) return fail(SWSEM_EINVAL, "too many load phases for the table's epoch field");
    ld.samplingPos = (uint64_t) (T + (int64_t) nTail * h->k1);
    return SWSEM_OK;
}

// private loadRef, .cpp:402-437, on a device-resident text
int flush_tag_summary(swsem *h);
int flush_inserts(swsem *h, const uint32_t *gate = nullptr);
// A flush runs its copies in one launch, its separators behind them and its insertion over the result: fine as long as no step
// writes where an earlier step of the same flush has written or sampled. A write to [a, b) that does — no sliding window and an
// extension longer than what is left of the lap, so the loader comes round to its own pieces — would race the earlier copy
// and have the earlier samples hashed from the later bytes (the reference hashes them before it goes on). Such a step has what
// is pending launched first, in order. (The samples of a step start at most K + k1 bytes in front of the text it wrote.)
bool hits_pending(const swsem *h, uint64_t a, uint64_t b) {
    const uint64_t reach = (uint64_t) h->K + (uint64_t) h->k1;
    for (auto &c : h->pendingCopies) if (a < c.dst + c.len && b + reach > c.dst) return true;
    for (auto &p : h->pendingBytes) if (p.off >= a && p.off < b) return true;
    return false;
}
int flush_if_hit(swsem *h, uint64_t a, uint64_t b) {
    if (!h->deferInserts || !hits_pending(h, a, b)) return SWSEM_OK;
    if (h->specMode) return SWSEM_ESPEC;                           // an ungated launch in the middle: give the speculation up
    return flush_inserts(h);
}
int load_pieces(swsem *h, const uint8_t *text, uint64_t len, bool rc, bool addSep, int sep) {
    LoaderState &ld = h->ld;
    while (len != 0) {
        ld.wrap_if_at_end(h->maxRefLength);
        const uint64_t tmpEnd = ld.swEnd;
        uint64_t tmpLength = len;
        const uint64_t tmpMax = tmpEnd < (uint64_t) ld.pos1 ? h->maxRefLength : tmpEnd;
        if ((uint64_t) ld.pos1 + tmpLength > tmpMax) tmpLength = tmpMax - (uint64_t) ld.pos1;
        // (a loader that stands at the window's end with that byte already the separator writes nothing — every further target of a
        // round whose loads have filled the window: no emission has to be waited for then; on collections that load every contig
        // with its reverse complement that is the second half of most rounds)
        const bool sepWrite = addSep && (uint64_t) ld.pos1 + tmpLength == ld.swEnd && !(tmpLength == 0 && ld.sep_end_done(sep));
        if (tmpLength || sepWrite) {
            // bytes this step writes: the copy, and the separator at the window's end when the copy reaches it
            // (a window that wraps has its end BELOW the loading position: only a loader that stands AT the end writes the byte before it)
            const uint64_t first = (uint64_t) ld.pos1 == ld.swEnd ? ld.swEnd - 1 : (uint64_t) ld.pos1;
            const uint64_t last = tmpLength ? (uint64_t) ld.pos1 + tmpLength - 1 : first;
            int g = ref_write_guard(h, first, last);
            if (g) return g;
        }
        if (tmpLength) { int f = flush_if_hit(h, (uint64_t) ld.pos1, (uint64_t) ld.pos1 + tmpLength); if (f) return f; }
        if (tmpLength && !rc && h->deferInserts) {                  // (nothing is launched here: no profiling bracket)
            CopyPiece cp; cp.dst = (uint64_t) ld.pos1; cp.src = text; cp.len = tmpLength;
            h->pendingCopies.push_back(cp);
        } else if (tmpLength) {
            h->mark(SWSEM_K_LOAD, true);
            if (rc) {
                const uint64_t thr = (tmpLength + 3) / 4;
                const unsigned blocks = (unsigned) std::min<uint64_t>((thr + 255) / 256, 8192);
                k_load_rc<<<dim3(blocks), dim3(256), 0, h->stream>>>(text + len - tmpLength, h->ref + ld.pos1, tmpLength, h->lut);
            } else
                HIPCHK(hipMemcpyAsync(h->ref + ld.pos1, text, tmpLength, hipMemcpyDeviceToDevice, h->stream));
            h->mark(SWSEM_K_LOAD, false);
        }
        if (sepWrite) {
            // (with the window full every target of a round comes by here and through loadSeparator's same case: once is enough)
            if (h->deferInserts) { BytePiece bp; bp.off = ld.swEnd - 1; bp.val = (uint64_t) (uint8_t) sep; h->pendingBytes.push_back(bp); }
            else k_set_byte<<<1, 1, 0, h->stream>>>(h->ref + ld.swEnd - 1, (uint8_t) sep);
            note_byte(h, ld.swEnd - 1);
            ld.sep_end_set((int64_t) ld.swEnd, sep);
        }
        const bool viaTable = tmpLength && !rc && h->deferInserts;
        const uint64_t copiedTo = (uint64_t) ld.pos1;
        ld.pos1 += (int64_t) tmpLength;
        int r = insert_samples(h, viaTable ? text : nullptr, copiedTo, copiedTo + tmpLength);
        if (r) return r;
        text += rc ? 0 : tmpLength;
        if ((uint64_t) ld.pos1 == tmpEnd) ld.droppedBytes += len - tmpLength;
        len = (uint64_t) ld.pos1 == tmpEnd ? 0 : len - tmpLength;
    }
    HIPCHK(hipGetLastError());
    return h->deferInserts ? SWSEM_OK : flush_tag_summary(h);
}

// Everything collected while deferInserts was set: all copies in one launch, the separator bytes in one (in program
// order; no copy of a round lands on a byte written by an earlier separator of the same round), then every insertion
// phase in one launch. The tables travel in a single upload. Two steps:
//   prepare_inserts      the host tables (pinned) and their upload on `upStream` (the speculative finalize's travel with the
//                        emission's own tables while the chains still run, not between pass 1 and the copies)
//   launch_inserts       the launches on the main stream: copies (on their stream), separators, the insertion, the samples at
//                        the pieces' edges
int prepare_inserts(swsem *h, hipStream_t upStream) {
    PreparedInserts &P = h->prep;
    P = PreparedInserts();
    const size_t np = h->pendingPieces.size(), nc = h->pendingCopies.size(), nb = h->pendingBytes.size();
    plan_tag_summary(h, h->sumRuns);
    const size_t ns = h->sumRuns.size();
    P.np = np; P.nc = nc; P.nb = nb; P.ns = ns;
    if (!np && !nc && !nb && !ns) return SWSEM_OK;
    // (every copy and byte collected here went through ref_write_guard when it was collected — load_pieces,
    // load_separator — with the lap count of that moment; one test of the whole span would take the two halves of a
    // round that wraps for a write across the whole buffer and give the speculative finalize up once per lap)
    constexpr uint64_t CHUNK = 256 * 16;                 // bytes per copy block
    // Insertion beside the copies: a sample whose K bytes all come out of its own piece's copy is hashed from the copy's
    // source (k_insert_multi<true>), while the copies run on a stream of their own; what is left — windows that reach into
    // the previous text or a separator, pieces without a copy — is listed as runs of its own and inserted from the buffer
    // once the copies have landed. A byte a separator of this flush overwrites is not "the copy's" any more.
    std::vector<InsertPiece> &edge = h->edgePieces;
    edge.clear();
    bool beside = np && nc;
    for (size_t i = 0; i < nc && beside; i++)            // (two copies of one flush over the same bytes: only in order)
        for (size_t j = i + 1; j < nc && beside; j++)
            beside = h->pendingCopies[i].dst + h->pendingCopies[i].len <= h->pendingCopies[j].dst || h->pendingCopies[j].dst + h->pendingCopies[j].len <= h->pendingCopies[i].dst;
    if (beside) {
        const int64_t k1 = h->k1, K = h->K;
        for (auto &pc : h->pendingPieces) {
            if (pc.src)
                for (auto &b : h->pendingBytes)
                    if (b.off >= pc.lo && b.off < pc.hi) { if (b.off - pc.lo < pc.hi - b.off) { pc.src += b.off + 1 - pc.lo; pc.lo = b.off + 1; } else pc.hi = b.off; }
            // samples p = base + t*k1, t < n, that k_insert_multi<true> does not take: p < lo or p + K > hi
            auto runs = [&](uint64_t base, uint64_t n, uint32_t epoch) {
                if (!n) return;
                int64_t a = 0, b = -1;                              // taken from the source: t in [a, b]
                if (pc.src && (int64_t) pc.hi - K >= (int64_t) base) {
                    a = (int64_t) pc.lo > (int64_t) base ? ((int64_t) pc.lo - (int64_t) base + k1 - 1) / k1 : 0;
                    b = std::min<int64_t>((int64_t) n - 1, ((int64_t) pc.hi - K - (int64_t) base) / k1);
                }
                auto push = [&](int64_t t0, int64_t t1) {           // [t0, t1)
                    if (t1 <= t0) return;
                    InsertPiece e = {};
                    e.S = base + (uint64_t) t0 * (uint64_t) k1; e.nMain = (uint64_t) (t1 - t0); e.epoch = epoch; e.tag = pc.tag;
                    edge.push_back(e);
                };
                if (b < a) push(0, (int64_t) n);
                else { push(0, a); push(b + 1, (int64_t) n); }
            };
            runs(pc.S, pc.nMain, pc.epoch);
            runs(pc.T, pc.nTail, pc.epoch + 1);
        }
    } else
        for (auto &pc : h->pendingPieces) pc.src = nullptr;
    const size_t ne = edge.size();
    const size_t wPieces = np * (sizeof(InsertPiece) / 8), wCopies = nc * (sizeof(CopyPiece) / 8), wBytes = nb * (sizeof(BytePiece) / 8), wEdge = ne * (sizeof(InsertPiece) / 8),
                 wSums = ns * (sizeof(SumRun) / 8);
    // host table: a member (two alternating ones), so the upload needs no wait before returning
    swsem::HostTab &ht = h->hostTables[h->hostTableSel ^= 1];
    const size_t words = wPieces + (np + 1) + wCopies + (nc + 1) + wBytes + wEdge + (ne + 1) + wSums;
    if (ht.pending) { HIPCHK(hipEventSynchronize(ht.ev)); ht.pending = false; }
    int r;
    if ((r = ht.buf.reserve(words * 8, std::max<size_t>(2 * words, 1 << 16) * 8))) return r;
    uint64_t *const tab = (uint64_t *) ht.buf.p;
    uint64_t *tPieces = tab, *tFirst = tPieces + wPieces, *tCopies = tFirst + np + 1, *tCFirst = tCopies + wCopies, *tBytes = tCFirst + nc + 1,
             *tEdge = tBytes + wBytes, *tEFirst = tEdge + wEdge, *tSums = tEFirst + ne + 1;
    if (np) memcpy(tPieces, h->pendingPieces.data(), np * sizeof(InsertPiece));
    tFirst[0] = 0;
    for (size_t i = 0; i < np; i++) tFirst[i + 1] = tFirst[i] + h->pendingPieces[i].nMain + h->pendingPieces[i].nTail;
    if (nc) memcpy(tCopies, h->pendingCopies.data(), nc * sizeof(CopyPiece));
    tCFirst[0] = 0;
    for (size_t i = 0; i < nc; i++) tCFirst[i + 1] = tCFirst[i] + (h->pendingCopies[i].len + CHUNK - 1) / CHUNK;
    if (nb) memcpy(tBytes, h->pendingBytes.data(), nb * sizeof(BytePiece));
    if (ne) memcpy(tEdge, edge.data(), ne * sizeof(InsertPiece));
    tEFirst[0] = 0;
    for (size_t i = 0; i < ne; i++) tEFirst[i + 1] = tEFirst[i] + edge[i].nMain;
    if (ns) memcpy(tSums, h->sumRuns.data(), ns * sizeof(SumRun));
    if ((r = h->dTables.reserve(std::max<size_t>(2 * words, 1 << 16)))) return r;   // regrowing = hipFree = a device-wide wait
    // (a kernel reading the pinned table: a runtime copy here costs an engine switch in the middle of the main stream)
    k_upload<<<dim3((unsigned) ((words * 8 + 4095) / 4096)), dim3(256), 0, upStream>>>((uint8_t *) h->dTables.p, (const uint8_t *) tab, words * 8);
    HIPCHK(hipEventRecord(ht.ev, upStream));
    ht.pending = true;
    const uint64_t *d = h->dTables.p;
    P.beside = beside; P.ne = ne;
    P.nSamples = tFirst[np]; P.nEdge = tEFirst[ne]; P.copyBlocks = tCFirst[nc];
    P.dPieces = (const InsertPiece *) (d + (tPieces - tab)); P.dFirst = d + (tFirst - tab);
    P.dCopies = (const CopyPiece *) (d + (tCopies - tab)); P.dCFirst = d + (tCFirst - tab);
    P.dBytes = (const BytePiece *) (d + (tBytes - tab));
    P.dEdge = (const InsertPiece *) (d + (tEdge - tab)); P.dEFirst = d + (tEFirst - tab);
    P.dSums = (const SumRun *) (d + (tSums - tab));
    h->pendingPieces.clear(); h->pendingCopies.clear(); h->pendingBytes.clear();
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}

int launch_inserts(swsem *h, const uint32_t *gate) {
    hipStream_t sV = h->stream;
    PreparedInserts &P = h->prep;
    const size_t np = P.np, nc = P.nc, nb = P.nb, ne = P.ne, ns = P.ns;
    if (!np && !nc && !nb && !ns) return SWSEM_OK;
    hipStream_t cs = sV;                                           // the copies' stream
    if (P.beside) {
        // (its own priority class: the runtime deals the streams of one class over a handful of hardware queues, and a copy
        // that lands on the queue of the emission's second phase runs behind 2 ms of its kernels — seen in a kernel trace)
        cs = h->streamLoad;
        HIPCHK(hipEventRecord(h->evLoadFork, sV));                   // (behind the tables, the gate and every wait the writes were given)
        HIPCHK(hipStreamWaitEvent(cs, h->evLoadFork, 0));
    }
    if (nc) {
        h->mark(SWSEM_K_LOAD, true, cs);
        k_copy_multi<<<dim3((unsigned) std::min<uint64_t>(P.copyBlocks, COPY_WGS)), dim3(256), 0, cs>>>(h->ref, P.dCopies, P.dCFirst, (int) nc, gate);
        h->mark(SWSEM_K_LOAD, false, cs);
    }
    if (nb) k_set_bytes<<<1, 1, 0, cs>>>(h->ref, P.dBytes, (int) nb, gate);
    // (the summary's entries beside the bytes: behind the same gate, and in front of the next resolve like the insertion itself)
    if (ns) k_set_tagsum<<<dim3(16), dim3(256), 0, cs>>>(h->tagSum, h->tagSumEntries, P.dSums, (int) ns, gate);
    if (P.beside) HIPCHK(hipEventRecord(h->evLoadDone, cs));
    if (np && P.nSamples) {
        h->mark(SWSEM_K_INSERT, true);
        const dim3 grid((unsigned) ((P.nSamples + 255) / 256));
        if (P.beside) k_insert_multi<true><<<grid, dim3(256), 0, h->stream>>>(h->ref, h->ht, P.dPieces, P.dFirst, (int) np, h->k1, h->k1ord, h->K, h->mask, h->fpBits, gate, h->tags);
        else k_insert_multi<false><<<grid, dim3(256), 0, h->stream>>>(h->ref, h->ht, P.dPieces, P.dFirst, (int) np, h->k1, h->k1ord, h->K, h->mask, h->fpBits, gate, h->tags);
        h->mark(SWSEM_K_INSERT, false);
    }
    if (P.beside) {
        HIPCHK(hipStreamWaitEvent(h->stream, h->evLoadDone, 0));
        if (ne && P.nEdge)
            k_insert_multi<false><<<dim3((unsigned) ((P.nEdge + 255) / 256)), dim3(256), 0, h->stream>>>(
                h->ref, h->ht, P.dEdge, P.dEFirst, (int) ne, h->k1, h->k1ord, h->K, h->mask, h->fpBits, gate, h->tags);
    }
    HIPCHK(hipGetLastError());
    return SWSEM_OK;
}

int flush_inserts(swsem *h, const uint32_t *gate) {
    int r = prepare_inserts(h, h->stream);
    return r ? r : launch_inserts(h, gate);
}
// a loader step outside a finalize (loadRef, loadSeparator called on their own) has launched its kernels itself: its summary runs follow
int flush_tag_summary(swsem *h) {
    if (h->sumUniform.empty() && h->sumMixed.empty()) return SWSEM_OK;
    return flush_inserts(h);
}

// loadSeparator, .cpp:439-451
int load_separator(swsem *h, int sep) {
    LoaderState &ld = h->ld;
    ld.wrap_if_at_end(h->maxRefLength);
    if ((uint64_t) ld.pos1 == h->maxRefLength) return SWSEM_OK;
    if ((uint64_t) ld.pos1 == ld.swEnd && ld.sep_end_done(sep)) return SWSEM_OK;    // that byte already is this separator
    { const uint64_t at = (uint64_t) ld.pos1 == ld.swEnd ? (uint64_t) ld.pos1 - 1 : (uint64_t) ld.pos1; int g = ref_write_guard(h, at, at); if (g) return g; }
    if ((uint64_t) ld.pos1 == ld.swEnd) {
        // this overwrites the last byte already loaded: insertion phases still pending hashed it as it was, and so was
        // the one sample whose K-mer ends there, if it has been inserted: its entry stops being trusted (k_mark_stale)
        if (h->specMode) return SWSEM_ESPEC;                      // an ungated write in the middle: give the speculation up
        if (h->deferInserts) { int r = flush_inserts(h); if (r) return r; }
        if (ld.pos1 >= (int64_t) h->K + REF_SHIFT)
            k_mark_stale<<<1, 1, 0, h->stream>>>(h->ref, h->ht, (uint64_t) (ld.pos1 - h->K), h->K, h->k1ord, h->mask, h->fpBits, h->tags);
        k_set_byte<<<1, 1, 0, h->stream>>>(h->ref + ld.pos1 - 1, (uint8_t) sep);
        note_byte(h, (uint64_t) ld.pos1 - 1);
        ld.sep_end_set(ld.pos1, sep);
    } else if (h->deferInserts) {
        { int f = flush_if_hit(h, (uint64_t) ld.pos1, (uint64_t) ld.pos1 + 1); if (f) return f; }
        note_byte(h, (uint64_t) ld.pos1);
        BytePiece bp; bp.off = (uint64_t) ld.pos1++; bp.val = (uint64_t) (uint8_t) sep;
        h->pendingBytes.push_back(bp);
    } else {
        note_byte(h, (uint64_t) ld.pos1);
        k_set_byte<<<1, 1, 0, h->stream>>>(h->ref + ld.pos1++, (uint8_t) sep);
    }
    HIPCHK(hipGetLastError());
    return h->deferInserts ? SWSEM_OK : flush_tag_summary(h);
}

// getLoadedRefLength, .h:108
uint64_t loaded_ref_length(const swsem *h) {
    return (uint64_t) h->ld.laps * (h->maxRefLength - REF_SHIFT) + ((uint64_t) h->ld.pos1 - REF_SHIFT);
}

// releaseWorkerMatchingLockPos, .cpp:380-400
int release_lock(swsem *h, uint64_t v) {
    if (h->swSize == 0 || !h->circular) return SWSEM_OK;
    std::deque<uint64_t> &locks = h->ld.locks;
    size_t i = 0;
    while (i < locks.size() && locks[i] != v) i++;
    if (i == locks.size()) return fail(SWSEM_ELOCK, "ERROR: Invalid worker lock value (%llu)", (unsigned long long) v);
    if (i == 0) {
        do {
            locks.pop_front();
        } while (!locks.empty() && locks.front() == UINT64_MAX);
        if (!locks.empty()) h->ld.swEnd = locks.front();
    } else
        locks[i] = UINT64_MAX;
    return SWSEM_OK;
}

// finalizeParallelProcessingOfTarget for n targets in order (MGMP.cpp:440-457, MBGC_Encoder.cpp:557-562):
// loadRef of the target's extension, the lazy-mode region separator, release of its lock position.
// loadedAfter[i] = getLoadedRefLength() after target i (what the encoder appends to refExtLoadedPosArr).
int finalize_impl(swsem *h, int n, const uint8_t *const *ext_dev, const uint64_t *ext_len, int addSep, int sep,
                  int lazySeparator, const uint64_t *lockPos, uint64_t *loadedAfter, const uint32_t *gate, bool planOnly = false) {
    HIPCHK(hipSetDevice(h->device));
    // all byte writes of the round first (copies, region separators), then every insertion phase in one
    // launch: hashing a window needs its bytes — including a separator written by a later step — in place
    h->deferInserts = true;
    int r = SWSEM_OK;
    for (int i = 0; i < n && !r; i++) {
        if (ext_len[i]) r = load_pieces(h, ext_dev[i], ext_len[i], false, addSep != 0, sep);
        if (!r && lazySeparator) r = load_separator(h, sep);
        if (!r && loadedAfter) loadedAfter[i] = loaded_ref_length(h);
        if (!r && lockPos) r = release_lock(h, lockPos[i]);
    }
    h->deferInserts = false;
    if (r == SWSEM_ESPEC) { h->pendingPieces.clear(); h->pendingCopies.clear(); h->pendingBytes.clear(); h->sumUniform.clear(); h->sumMixed.clear(); return r; }
    // planOnly (the speculative finalize): the host's bookkeeping is done and the launches are listed; the caller queues them
    // (prepare_inserts, launch_inserts) once every replica's verdict has been reduced into the gate — and knows by now whether
    // THIS replica can
    if (planOnly) return r;
    const int r2 = flush_inserts(h, gate);
    return r ? r : r2;
}

}  // namespace
