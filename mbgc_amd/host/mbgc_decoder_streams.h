// Part of mbgc_decoder.cpp (included there once, behind its file helpers): what is on disk. The stream set as `mbgc-hip c` wrote
// it, held to its meta; the units --select chooses; and THE walk over what was chosen, which every sink uses. Host only,
// but for the -m 3 restore, which runs on the device before anything reads the literals.
#pragma once

namespace {
struct Interval { uint64_t from, to; };

static const char *const STREAM_NAMES[SWSEM_NSTREAMS] = {"literals", "mapOff", "mapOff5th", "mapLen", "gapDelta", "flags"};

struct StreamSet {
    MbgcMeta meta;
    std::string stream[SWSEM_NSTREAMS];
    uint64_t sizes[SWSEM_NSTREAMS] = {};
    std::string locksPos, refExtSize;                              // the bytes of the two files, until check() has read them
    std::vector<uint64_t> lock, extSize;                           // per target (extSize: lazy mode only, else 0)
    bool lazy = false;
    std::vector<uint64_t> g0ContigLen;                             // G0: the contigs at the head of the literal stream
    uint64_t lit0 = 0, g0n = 0, g0Bytes = 0;                       // lit0: the literals behind G0 and its separators
    std::vector<uint32_t> seqCount;                                // per target
    uint64_t planned = 0;                                          // the targets' contigs
    std::vector<swsem_chain_start_t> starts;
    bool useIndex = false;
    PgTools::SimpleSequenceMatcher::RestoreStats rcStats;          // -m 3
    double rcRestoreMs = 0;
    size_t T() const { return meta.targets.size(); }
};

// <prefix>.meta and the files of the streams, as bytes; what the options refuse about the meta is refused before a stream is read
bool readStreamFiles(const std::string &prefix, const MBGC_Decoder::Options &opt, StreamSet &S, std::string &msg) {
    std::string metaBytes;
    if (!readFile(prefix + ".meta", metaBytes)) { msg = "cannot open " + prefix + ".meta (written by mbgc-hip c beside the streams)"; return false; }
    if (!S.meta.parse(metaBytes, &msg)) return false;
    if (opt.resident && S.meta.singleFastaFile) {
        msg = "the streams hold one FASTA file (mbgc-hip c -i): a single-FASTA stream set is not repacked (it has one unit, and its elements are no files)";
        return false;
    }
    if (S.meta.rcRedundancyRemoval && !opt.restoreRc) {
        msg = "the streams were written with -m 3: its reverse-complement pass over the literal stream (rcMapOff / rcMapLen) is not inverted by mbgc-hip d"
              " unless --restore-rc is given";
        return false;
    }
    for (int s = 0; s < SWSEM_NSTREAMS; s++)
        if (!readFile(prefix + "." + STREAM_NAMES[s], S.stream[s])) { msg = "cannot open " + prefix + "." + STREAM_NAMES[s]; return false; }
    if (!readFile(prefix + ".locksPos", S.locksPos) || !readFile(prefix + ".refExtSize", S.refExtSize)) { msg = "cannot open " + prefix + ".locksPos / .refExtSize"; return false; }
    return true;
}

// -m 3: the literals as they were before the reverse-complement pass cut them (MBGC_Decoder.cpp:1137), restored on the device
// before anything reads them; the meta's stream index holds offsets into the uncut literals. Its place in the order of checks:
// behind the stream files, before "no target". --bench: run twice, the second run is the timed one.
bool restoreRcLiterals(const std::string &prefix, const MBGC_Decoder::Options &opt, StreamSet &S, std::string &msg) {
    if (!S.meta.rcRedundancyRemoval) return true;
    const MbgcMeta &meta = S.meta;
    std::string rcMapOff, rcMapLen;
    if (!readFile(prefix + ".rcMapOff", rcMapOff) || !readFile(prefix + ".rcMapLen", rcMapLen)) { msg = "cannot open " + prefix + ".rcMapOff / .rcMapLen"; return false; }
    const size_t uncut = meta.index.empty() ? PgTools::SimpleSequenceMatcher::UNKNOWN_LENGTH : (size_t) meta.index[meta.index.size() - SWSEM_NSTREAMS + SWSEM_LIT];
    const std::string cutLiterals = opt.bench ? S.stream[SWSEM_LIT] : std::string();
    for (int run = 0; run < (opt.bench ? 2 : 1); run++) {
        if (run) S.stream[SWSEM_LIT] = cutLiterals;
        std::string e;
        const double t0 = nowMs();
        if (!PgTools::SimpleSequenceMatcher::restoreRCMatchedSequence(S.stream[SWSEM_LIT], rcMapOff, rcMapLen, uncut, opt.device, &e, &S.rcStats)) {
            msg = "malformed stream set: " + e;
            return false;
        }
        S.rcRestoreMs = nowMs() - t0;
    }
    return true;
}

// the side files against the meta, G0's contigs (MBGC_Decoder::decodeReference :265-317 / initReference :243-263), the counts
bool checkStreams(StreamSet &S, std::string &msg) {
    const MbgcMeta &meta = S.meta;
    const size_t T = S.T();
    const std::string &lit = S.stream[SWSEM_LIT];
    if (T == 0) { msg = "malformed stream set: no target"; return false; }
    if (S.locksPos.size() != T * sizeof(uint64_t)) { msg = "malformed stream set: locksPos does not hold one position per target"; return false; }
    if (meta.maxRefLength < 64) { msg = "malformed .meta: reference length"; return false; }
    S.lock.resize(T);
    memcpy(S.lock.data(), S.locksPos.data(), S.locksPos.size());
    S.lazy = meta.emit.lazyDecompressionSupport != 0;
    S.extSize.assign(T, 0);
    if (S.lazy) {
        size_t at = 0;
        for (size_t t = 0; t < T; t++) if (!readUInt64Frugal(S.refExtSize, at, S.extSize[t])) { msg = "malformed stream set: refExtSize ends early"; return false; }
        if (at != S.refExtSize.size()) { msg = "malformed stream set: bytes left over in refExtSize"; return false; }
    }
    for (uint32_t g = 0; g < meta.g0Contigs; g++) {
        const void *sep = S.lit0 < lit.size() ? memchr(lit.data() + S.lit0, SEQ_SEPARATOR_MARK, lit.size() - S.lit0) : nullptr;
        if (!sep) { msg = "malformed stream set: the literals end inside the initial reference"; return false; }
        const uint64_t end = (uint64_t) ((const char *) sep - lit.data());
        S.g0ContigLen.push_back(end - S.lit0);
        S.lit0 = end + 1;
    }
    S.g0n = meta.g0Contigs; S.g0Bytes = S.lit0 - S.g0n;
    S.seqCount.resize(T);
    for (size_t t = 0; t < T; t++) { S.seqCount[t] = meta.targets[t].seqsCount; S.planned += S.seqCount[t]; }
    if (S.planned > lit.size()) { msg = "malformed .meta: more sequences than literal bytes"; return false; }
    for (int s = 0; s < SWSEM_NSTREAMS; s++) S.sizes[s] = S.stream[s].size();
    return true;
}

// where the plan's chains start: at every target, from the meta's index held to the streams' sizes, or one chain over them all
bool chainStarts(bool noIndex, StreamSet &S, std::string &msg) {
    const size_t T = S.T();
    S.useIndex = !noIndex && !S.meta.index.empty();
    if (!S.useIndex) {
        swsem_chain_start_t c = {};
        c.cur[SWSEM_LIT] = S.lit0;
        for (int s = 0; s < SWSEM_NSTREAMS; s++) c.end[s] = S.sizes[s];
        c.firstTarget = 0; c.nTargets = (uint32_t) T; c.checkEnd = 1;
        S.starts.push_back(c);
        return true;
    }
    const uint64_t *ix = S.meta.index.data();
    if (ix[SWSEM_LIT] != S.lit0) { msg = "malformed .meta: the stream index does not start behind the initial reference"; return false; }
    for (size_t t = 0; t <= T; t++)
        for (int s = 0; s < SWSEM_NSTREAMS; s++)
            if (ix[t * SWSEM_NSTREAMS + s] > S.sizes[s] || (t && ix[t * SWSEM_NSTREAMS + s] < ix[(t - 1) * SWSEM_NSTREAMS + s]) || (t == T && ix[t * SWSEM_NSTREAMS + s] != S.sizes[s])) {
                msg = std::string("malformed stream set: the index of ") + STREAM_NAMES[s] + " does not fit the stream (target " + std::to_string(t) + ")";
                return false;
            }
    for (size_t t = 0; t < T; t++) {
        swsem_chain_start_t c = {};
        for (int s = 0; s < SWSEM_NSTREAMS; s++) { c.cur[s] = ix[t * SWSEM_NSTREAMS + s]; c.end[s] = ix[(t + 1) * SWSEM_NSTREAMS + s]; }
        c.firstTarget = (uint32_t) t; c.nTargets = 1; c.checkEnd = 1;
        S.starts.push_back(c);
    }
    return true;
}

// the lines of <prefix>.names, held to the meta: one per unit (G0, then every target), one for a single-FASTA collection
bool parseNames(const std::string &names, const MbgcMeta &meta, std::vector<std::string> &out, std::string &msg) {
    const size_t T = meta.targets.size();
    if (!names.empty() && names.back() != '\n') { msg = "malformed .names: the last line does not end"; return false; }
    for (size_t at = 0; at < names.size();) { const size_t e = names.find('\n', at); out.push_back(names.substr(at, e - at)); at = e + 1; }
    if (out.size() != (meta.singleFastaFile ? 1 : T + 1)) {
        msg = "malformed .names: " + std::to_string(out.size()) + " names for " + std::to_string(meta.singleFastaFile ? 1 : T + 1) + " units";
        return false;
    }
    return true;
}

// ---- --select: the units to bring back (G0, then every target), by the names mbgc-hip c wrote beside the streams; --select-seq:
// the records to bring back, by the headers written there (chooseRecords, mbgc_decoder_fasta.h: the match runs on the device)
// --region: a piece is bases [from, from + len) of contig `contig` of the collection (0-based, clamped to the record), written to unit
// `unit`'s file
struct RegionPiece { uint64_t contig, from, len; size_t unit; };
struct RegionAsk { uint64_t contig, from, to; size_t unit; };      // a spec on a chosen record, before the record's length is known

struct Selection {
    // --region (mbgc_decoder_region.h): asks: what the specs choose, by the headers; pieces: the asks held to the records' lengths, in
    // output order; granuleShift: log2 of the closure's granule
    bool selectingRegion = false;
    std::vector<RegionAsk> asks;
    std::vector<RegionPiece> pieces;
    uint64_t regionRecords = 0, regionBases = 0, regionSkipped = 0;
    uint32_t granuleShift = 8;
    std::vector<char> unitSel;                                     // per unit; all of them without a selection. --select-seq: the units that hold a chosen record
    std::vector<char> contigSel;                                   // --select-seq: per contig of the collection, G0's first; empty without it
    uint64_t selectedFiles = 0;                                    // the files that are written
    bool selecting = false, selectingSeq = false;
    uint64_t recordsChosen = 0, recordsAll = 0;                    // --select-seq
    double matchMs = 0, matchHostMs = 0;                           // the match kernel; --select-seq-host: the host's loop over the same input
    // planned contig c of target t is among what is brought back
    bool chosen(size_t t, uint64_t c, uint64_t g0n) const { return contigSel.empty() ? unitSel[t + 1] != 0 : contigSel[g0n + c] != 0; }
};

// layoutNames: the names a sink has read already (--fasta, v, r: the layout's); without them --select reads <prefix>.names itself
bool chooseUnits(const std::string &prefix, const StreamSet &S, const std::vector<std::string> &select, const std::vector<std::string> *layoutNames,
                 Selection &sel, std::string &msg) {
    const size_t T = S.T();
    sel.selecting = !select.empty();
    sel.unitSel.assign(T + 1, 1);
    if (!sel.selecting) return true;
    if (S.meta.singleFastaFile) { msg = "--select: the streams hold one FASTA file (mbgc-hip c -i): it has one name, there is nothing to select"; return false; }
    std::vector<std::string> own;
    if (!layoutNames) {
        std::string bytes;
        if (!readFile(prefix + ".names", bytes)) {
            msg = "malformed stream set: cannot open " + prefix + ".names (--select needs the names mbgc-hip c writes beside the streams)";
            return false;
        }
        if (!parseNames(bytes, S.meta, own, msg)) return false;
    }
    const std::vector<std::string> &names = layoutNames ? *layoutNames : own;
    // (-t1: the first file is G0's unit and target 0; the selection is over output files, and G0's unit is none of them)
    for (size_t u = 0; u <= T; u++) {
        sel.unitSel[u] = 0;
        if (u == 0 && S.meta.sequentialMatching) continue;
        for (const std::string &pat : select) if (names[u].find(pat) != std::string::npos) sel.unitSel[u] = 1;   // MBGC_Decoder.cpp:1022-1025
        sel.selectedFiles += sel.unitSel[u];
    }
    if (!sel.selectedFiles) {
        msg = "--select: no file of the collection matches (" + std::to_string(select.size()) + " patterns against " + prefix + ".names)";
        return false;
    }
    return true;
}

// ---- what is brought back, in collection order: unit u (0: G0, u: target u - 1) holds contigs [c0, c1) of the collection. Under -t1
// the initial reference is the first contig of target 0 again and no unit of its own; a unit that was not chosen is none. A row is a
// whole chosen unit (contigSel == nullptr: --select, or no selection; a unit without a contig has its row too) or, under
// --select-seq, one of a chosen unit's maximal runs of chosen contigs — a run never reaches over a unit's end, so a row is always
// one file's. Everything that leaves the decoder — the sequence files, the FASTA files, what `v` compares, what `r` packs — walks
// this list.
struct ChosenUnit { size_t unit; uint64_t c0, c1; };
std::vector<ChosenUnit> chosenUnits(uint64_t g0n, const uint32_t *seqCount, size_t T, const char *unitSel, const char *contigSel, bool sequentialMatching) {
    std::vector<ChosenUnit> out;
    uint64_t c = 0;
    for (size_t u = 0; u <= T; u++) {
        const uint64_t n = u == 0 ? g0n : seqCount[u - 1];
        if (unitSel[u] && !(u == 0 && sequentialMatching)) {
            if (!contigSel) out.push_back({u, c, c + n});
            else
                for (uint64_t k = c; k < c + n;) {
                    if (!contigSel[k]) { k++; continue; }
                    uint64_t e = k;
                    while (e < c + n && contigSel[e]) e++;
                    out.push_back({u, k, e});
                    k = e;
                }
        }
        c += n;
    }
    return out;
}
// what is written: the rows' contigs as ranges [from, to) of the collection's contigs, adjacent ones merged (over a unit's end too)
std::vector<Interval> mergedRanges(const std::vector<ChosenUnit> &chosen) {
    std::vector<Interval> out;
    for (const ChosenUnit &x : chosen) {
        if (x.c1 == x.c0) continue;
        if (!out.empty() && out.back().to == x.c0) out.back().to = x.c1; else out.push_back({x.c0, x.c1});
    }
    return out;
}
}  // namespace
