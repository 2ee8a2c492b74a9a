#include "mbgc_decoder.h"
#include "simple_sequence_matcher.h"
#include "gzip_inflate.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <set>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <time.h>

static const uint64_t REF_SHIFT = 1;                           // SlidingWindowSparseEMMatcher.h:14
static const uint8_t SEQ_SEPARATOR_MARK = (uint8_t) ('"' + 128);   // MBGC_Params.h:46
static const uint8_t REF_REGION_SEPARATOR = 0;                 // MGMP_Params.h:14

// ---------------------------------------------------------------- <prefix>.meta
// little endian: "MBGCHIPM", u32 version, u32 flags, u32 coderMode, k, k1, g0Contigs, u64 maxRefLength, swSize, finalRefLength,
// reachedRefLengthCount, the 15 fields of swsem_emit_params_t as i64, u32 targets, u32 indexed, per target {u32 seqsCount,
// u8 unmatchedFractionFactor, u8 unmatchedFractionRCFactor, u16 0}, then (indexed) (targets + 1) x 6 u64 stream offsets
static const char META_MAGIC[9] = "MBGCHIPM";
enum { MF_SEQUENTIAL = 1, MF_RC_IN_REF = 2, MF_CONTIGS_REVERSED = 4, MF_UPPERCASE = 8, MF_SINGLE_FASTA = 16, MF_RC_REDUNDANCY = 32 };

template <typename T> static void put(std::string &s, T v) { s.append((const char *) &v, sizeof v); }
template <typename T> static bool get(const std::string &s, size_t &at, T &v) {
    if (at + sizeof v > s.size()) return false;
    memcpy(&v, s.data() + at, sizeof v); at += sizeof v;
    return true;
}
static void emitFields(const swsem_emit_params_t &e, int64_t f[15]) {
    const int64_t v[15] = {e.enableExtensionsWithMismatches, e.mismatchesWithExclusion, e.lazyDecompressionSupport, e.enable40bitReference,
                           e.frugal64bitLenEncoding, e.gapDepthOffsetEncoding, e.gapDepthMismatchesEncoding, (int64_t) e.gapBreakingMatchMinLength,
                           e.mmsMatchBonus, e.mmsMismatchPenalty, e.mmsMismatchesScoreThreshold, e.mmsMismatchesInitialScore,
                           e.allowedTargetsOutrunForDissimilarContigs, (int64_t) e.minimalLengthForDissimilarContigs,
                           e.unmatchedFractionFactorTweakForDissimilarContigs};
    memcpy(f, v, sizeof v);
}

std::string MbgcMeta::serialize() const {
    std::string s(META_MAGIC, 8);
    put<uint32_t>(s, VERSION);
    put<uint32_t>(s, (sequentialMatching ? MF_SEQUENTIAL : 0) | (rcInReference ? MF_RC_IN_REF : 0) | (contigsIndividuallyReversed ? MF_CONTIGS_REVERSED : 0) |
                         (uppercaseDNA ? MF_UPPERCASE : 0) | (singleFastaFile ? MF_SINGLE_FASTA : 0) | (rcRedundancyRemoval ? MF_RC_REDUNDANCY : 0));
    put<uint32_t>(s, coderMode); put<uint32_t>(s, k); put<uint32_t>(s, k1); put<uint32_t>(s, g0Contigs);
    put<uint64_t>(s, maxRefLength); put<uint64_t>(s, swSize); put<uint64_t>(s, finalRefLength); put<uint64_t>(s, reachedRefLengthCount);
    int64_t f[15];
    emitFields(emit, f);
    for (int64_t v : f) put<int64_t>(s, v);
    put<uint32_t>(s, (uint32_t) targets.size());
    put<uint32_t>(s, index.empty() ? 0u : 1u);
    for (const Target &t : targets) { put<uint32_t>(s, t.seqsCount); put<uint8_t>(s, t.unmatchedFractionFactor); put<uint8_t>(s, t.unmatchedFractionRCFactor); put<uint16_t>(s, 0); }
    for (uint64_t v : index) put<uint64_t>(s, v);
    return s;
}

bool MbgcMeta::parse(const std::string &b, std::string *error) {
    auto bad = [&](const char *what) { if (error) *error = std::string("malformed .meta: ") + what; return false; };
    if (b.size() < 8 || memcmp(b.data(), META_MAGIC, 8) != 0) return bad("not a meta file of mbgc-hip c");
    size_t at = 8;
    uint32_t version = 0, flags = 0, n = 0, indexed = 0;
    if (!get(b, at, version) || version != VERSION) return bad("unknown version");
    if (!get(b, at, flags) || !get(b, at, coderMode) || !get(b, at, k) || !get(b, at, k1) || !get(b, at, g0Contigs) || !get(b, at, maxRefLength) ||
        !get(b, at, swSize) || !get(b, at, finalRefLength) || !get(b, at, reachedRefLengthCount)) return bad("truncated header");
    sequentialMatching = flags & MF_SEQUENTIAL; rcInReference = flags & MF_RC_IN_REF; contigsIndividuallyReversed = flags & MF_CONTIGS_REVERSED;
    uppercaseDNA = flags & MF_UPPERCASE; singleFastaFile = flags & MF_SINGLE_FASTA; rcRedundancyRemoval = flags & MF_RC_REDUNDANCY;
    int64_t f[15];
    for (int64_t &v : f) if (!get(b, at, v)) return bad("truncated emit parameters");
    emit.enableExtensionsWithMismatches = (int) f[0]; emit.mismatchesWithExclusion = (int) f[1]; emit.lazyDecompressionSupport = (int) f[2];
    emit.enable40bitReference = (int) f[3]; emit.frugal64bitLenEncoding = (int) f[4]; emit.gapDepthOffsetEncoding = (int) f[5];
    emit.gapDepthMismatchesEncoding = (int) f[6]; emit.gapBreakingMatchMinLength = (uint64_t) f[7]; emit.mmsMatchBonus = (int) f[8];
    emit.mmsMismatchPenalty = (int) f[9]; emit.mmsMismatchesScoreThreshold = (int) f[10]; emit.mmsMismatchesInitialScore = (int) f[11];
    emit.allowedTargetsOutrunForDissimilarContigs = (int) f[12]; emit.minimalLengthForDissimilarContigs = (uint64_t) f[13];
    emit.unmatchedFractionFactorTweakForDissimilarContigs = (int) f[14];
    if (!get(b, at, n) || !get(b, at, indexed) || indexed > 1) return bad("truncated target table");
    if ((b.size() - at) / 8 < n) return bad("truncated target table");
    targets.assign(n, Target());
    for (Target &t : targets) {
        uint16_t pad = 0;
        if (!get(b, at, t.seqsCount) || !get(b, at, t.unmatchedFractionFactor) || !get(b, at, t.unmatchedFractionRCFactor) || !get(b, at, pad)) return bad("truncated target table");
    }
    index.clear();
    if (indexed) {
        index.assign(((size_t) n + 1) * SWSEM_NSTREAMS, 0);
        for (uint64_t &v : index) if (!get(b, at, v)) return bad("truncated stream index");
    }
    if (at != b.size()) return bad("bytes left over");
    return true;
}

// ---------------------------------------------------------------- the load schedule
bool MBGC_Decoder::loadRef(RefState &st, int64_t contig, uint64_t textOffset, uint64_t seqLength, uint64_t refLockPos, bool loadRCRef,
                           std::vector<LoadSegment> &out) {
    while (seqLength != 0) {                                                                    // :653-654
        if (st.refPos == st.refTotalLength && refLockPos != st.refTotalLength) {                 // :655-658
            st.reachedRefLengthCount++;
            st.refPos = REF_SHIFT;
        }
        uint64_t tmpLength = seqLength;                                                        // :659
        const uint64_t tmpMax = refLockPos < st.refPos ? st.refTotalLength : refLockPos;         // :660
        if (st.refPos > tmpMax) return false;
        if (st.refPos + tmpLength > tmpMax) tmpLength = tmpMax - st.refPos;                      // :661-663
        if (tmpLength == 0 && st.refPos != refLockPos) return false;                            // (the recursion would not end)
        if (tmpLength) {
            // :664-668: upperReverseComplement(seqText + seqLength - tmpLength, tmpLength, ...) or the copy of the text's head
            LoadSegment s = {contig, loadRCRef ? textOffset + seqLength - tmpLength : textOffset, tmpLength, st.refPos, loadRCRef};
            if (contig == LoadSegment::SEPARATOR) s.offset = 0;
            out.push_back(s);
        }
        st.refPos += tmpLength;                                                                 // :669
        if (!loadRCRef) textOffset += tmpLength;                                                // :670
        seqLength = st.refPos == refLockPos ? 0 : seqLength - tmpLength;                         // :671
        if (st.lazyDecompressionSupport && st.refPos == refLockPos) {                           // :672-673
            const LoadSegment sep = {LoadSegment::SEPARATOR, 0, 1, refLockPos - 1, false};
            out.push_back(sep);
        }
    }
    return true;
}

bool MBGC_Decoder::scheduleTarget(RefState &st, uint64_t firstContig, const std::vector<ContigInfo> &contigs, uint8_t unmatchedFractionFactor,
                                  uint8_t unmatchedFractionRCFactor, bool rcInReference, bool contigsIndividuallyReversed, uint64_t refLockPos,
                                  std::vector<LoadSegment> &out) {
    const uint64_t startPos = st.refPos;                                                        // :564
    for (size_t i = 0; i < contigs.size(); i++) {
        const ContigInfo &c = contigs[i];
        // MGMP_Params::isContigProperForRefExtension / ...RCExtension (MGMP_Params.h:179-190)
        const bool loadContigToRef = c.unmatched * (uint64_t) unmatchedFractionFactor > c.length;   // :591
        const uint64_t extSize = loadContigToRef ? c.length : 0;                                // :596-597 (the literal extension is empty outside developer builds)
        if (!loadRef(st, (int64_t) (firstContig + i), 0, extSize, refLockPos, false, out)) return false;   // :598
        if (rcInReference && contigsIndividuallyReversed && c.unmatched * (uint64_t) unmatchedFractionRCFactor > c.length)   // :599-601
            if (!loadRef(st, (int64_t) (firstContig + i), 0, extSize, refLockPos, true, out)) return false;
    }
    if (rcInReference && !contigsIndividuallyReversed) {                                       // :608-616
        if (st.refPos >= startPos) {
            if (!loadRef(st, LoadSegment::FROM_REF, startPos, st.refPos - startPos, refLockPos, true, out)) return false;
        } else {
            const uint64_t tmpStartPos = startPos;
            if (!loadRef(st, LoadSegment::FROM_REF, 1, st.refPos - 1, refLockPos, true, out)) return false;
            if (!loadRef(st, LoadSegment::FROM_REF, tmpStartPos, st.refTotalLength - tmpStartPos, refLockPos, true, out)) return false;
        }
    }
    if (st.lazyDecompressionSupport)                                                            // :617-620
        if (!loadRef(st, LoadSegment::SEPARATOR, 0, 1, refLockPos, false, out)) return false;
    return true;
}

bool MBGC_Decoder::scheduleG0(RefState &st, uint64_t g0Bytes, bool rcInReference, bool sequentialMatching, std::vector<LoadSegment> &out) {
    // SlidingWindowSparseEMMatcher::loadRef with swEnd as initMatcher leaves it: disableSlidingWindow() puts it at 0 before the load
    // (-t1), otherwise it is the buffer's end; no separator of lazy mode belongs to this load
    RefState g = st;
    g.lazyDecompressionSupport = false;
    const uint64_t swEnd = sequentialMatching ? 0 : st.refTotalLength;
    if (!loadRef(g, 0, 0, g0Bytes, swEnd, false, out)) return false;
    if (rcInReference && !loadRef(g, 0, 0, g0Bytes, swEnd, true, out)) return false;
    st.refPos = g.refPos; st.reachedRefLengthCount = g.reachedRefLengthCount;
    return true;
}

// ---------------------------------------------------------------- the driver
static bool readFile(const std::string &path, std::string &dest) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamoff n = f.tellg();
    f.seekg(0);
    dest.resize((size_t) n);
    if (n) f.read(&dest[0], n);
    return (bool) f;
}
static bool writeFile(const std::string &path, const void *p, size_t n) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write((const char *) p, (std::streamsize) n);
    return (bool) f;
}
static double nowMs() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// PgHelpers::readUInt64Frugal, utils/helper.h:256-272
static bool readUInt64Frugal(const std::string &s, size_t &at, uint64_t &v) {
    uint16_t y16; uint32_t y32;
    if (!get(s, at, y16)) return false;
    if (y16 < UINT16_MAX) { v = y16; return true; }
    if (!get(s, at, y32)) return false;
    if (y32 < UINT32_MAX) { v = y32; return true; }
    return get(s, at, v);
}

namespace {
struct DevFree {
    swsem_t *h; std::vector<void *> ptrs;
    ~DevFree() { for (void *p : ptrs) if (p) swsem_dev_free(h, p); if (h) swsem_destroy(h); }
};
struct Interval { uint64_t from, to; };
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

    // the owned pieces of physical range [p0, p1) as the loader left the buffer at virtual position tv: f(physFrom, physTo, owner).
    // Below the loader's position the bytes are this lap's, from it on the lap before's (before the first lap: never written);
    // a range that straddles the position is split there. (k_decode_closure: the same on the device.)
    template <class F> void query(uint64_t tv, uint64_t p0, uint64_t p1, F f) const {
        if (p1 > L) p1 = L;
        if (p0 >= p1) return;
        const uint64_t lap = tv / L, rp = tv % L;
        auto part = [&](uint64_t a, uint64_t b, uint64_t base) {
            const uint64_t va = base + a, vb = base + b;
            size_t i = (size_t) (std::partition_point(rows.begin(), rows.end(), [&](const swsem_prov_row_t &r) { return r.vstart + r.len <= va; }) - rows.begin());
            for (; i < rows.size() && rows[i].vstart < vb; i++)
                f(std::max(va, rows[i].vstart) - base, std::min(vb, rows[i].vstart + rows[i].len) - base, rows[i].owner);
        };
        if (p0 < rp) part(p0, std::min(p1, rp), lap * L);
        if (p1 > rp && lap) part(std::max(p0, rp), p1, (lap - 1) * L);
    }
    // the next segment of the schedule, in serial order; contigs from firstPlanned on are the planned ones (owner = contig - firstPlanned)
    void add(const LoadSegment &s, uint64_t firstPlanned) {
        if (s.length == 0) return;
        if (s.contig == LoadSegment::SEPARATOR && s.length == 1 && (s.refPos + 1) % L == cur % L) return;   // written over the last loaded byte: the superset rule
        const uint64_t v = cur + (s.refPos + L - cur % L) % L;      // the next virtual position that lies at refPos
        if (s.contig == LoadSegment::FROM_REF) {
            std::vector<swsem_prov_row_t> got;
            query(cur, s.offset, s.offset + s.length, [&](uint64_t a, uint64_t b, int64_t owner) {
                const uint64_t at = s.reverseComplement ? s.length - (b - s.offset) : a - s.offset;
                got.push_back({v + at, b - a, owner});
            });
            std::sort(got.begin(), got.end(), [](const swsem_prov_row_t &x, const swsem_prov_row_t &y) { return x.vstart < y.vstart; });
            rows.insert(rows.end(), got.begin(), got.end());
        } else if (s.contig >= 0 && (uint64_t) s.contig >= firstPlanned)
            rows.push_back({v, s.length, (int64_t) ((uint64_t) s.contig - firstPlanned)});
        cur = v + s.length;
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
static std::vector<FillUnit> partitionUnits(const std::vector<uint32_t> &seqCount, const std::vector<uint64_t> &lock, const std::vector<std::vector<LoadSegment>> &tSegs,
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

// ---- --fasta: the layout beside the streams (<prefix>.names / .headers / .dnaLineLengths, written by mbgc-hip c)
static const uint64_t FASTA_BATCH_TEXT = 256ull << 20;            // text bytes of a batch of whole units (a larger unit is a batch of its own)
struct FastaUnit { uint64_t c0, c1; uint64_t lineLen; size_t file; uint64_t text; };   // contigs [c0, c1) of the collection, its output file
struct FastaLayout {
    std::string headers;                                           // the bytes of <prefix>.headers
    std::vector<uint64_t> hdrOff, hdrLen;                          // per contig, G0's first
    std::vector<uint64_t> lineLen;                                 // per unit, G0 first
    std::vector<std::string> names;                                // per unit (one for a single-FASTA collection)
    std::vector<std::string> outNames;                             // the files to write, in order
};
struct FastaTimes { double format = 0, download = 0, write = 0, deflate = 0; uint64_t text = 0, batches = 0, gz = 0, chunks = 0, storedChunks = 0; };
struct FastaBuffers {                                              // freed on every way out
    mbgc_fasta_t *fa = nullptr; uint8_t *hdrDev = nullptr, *textDev[2] = {nullptr, nullptr}; void *pin[2] = {nullptr, nullptr};
    uint8_t *gzDev[2] = {nullptr, nullptr};                        // --gzip: the gzip files of a batch (not allocated without it)
    std::future<bool> writing;
    ~FastaBuffers() {
        if (writing.valid()) writing.wait();
        if (!fa) return;
        mbgc_fasta_download_wait(fa, nullptr);                     // (a way out between begin and wait)
        if (hdrDev) mbgc_fasta_dev_free(fa, hdrDev);
        for (uint8_t *t : textDev) if (t) mbgc_fasta_dev_free(fa, t);
        for (uint8_t *t : gzDev) if (t) mbgc_fasta_dev_free(fa, t);
        for (void *p : pin) if (p) mbgc_fasta_host_free(fa, p);
        mbgc_fasta_destroy(fa);
    }
};

static uint64_t recordText(uint64_t headerLen, uint64_t seqLen, uint64_t lineLen) {
    const uint64_t line = (lineLen == 0 || lineLen > seqLen) ? seqLen : lineLen;
    return 2 + headerLen + (seqLen ? seqLen + (seqLen - 1) / line + 1 : 0);
}

// the file a unit goes to: the basename of its name (the reference's ignoreFastaFilesPath: nothing is written outside the
// directory), without a .gz suffix — the text is written inflated
static std::string outputName(const std::string &name) {
    std::string b = name.substr(name.find_last_of('/') == std::string::npos ? 0 : name.find_last_of('/') + 1);
    if (b.size() >= 3 && b.compare(b.size() - 3, 3, ".gz") == 0) b.resize(b.size() - 3);
    return b;
}

// the directory, with the ones above it; false: *failed = the one that could not be made
static bool makeDirs(const std::string &dir, std::string *failed) {
    for (size_t at = 1; at <= dir.size(); at++)
        if (at == dir.size() || dir[at] == '/')
            if (mkdir(dir.substr(0, at).c_str(), 0777) != 0 && errno != EEXIST) { *failed = dir.substr(0, at); return false; }
    return true;
}

// ---- `mbgc-hip v`: the originals of a batch as the read-ahead thread leaves them in a page-locked buffer
static const uint64_t VALIDATION_LOG_LIMIT = 100, VALIDATION_DUMP_LIMIT = 3;   // MBGC_Params.h:121-122
struct Original {
    std::string path;                                              // as it is named in the report (without the .gz that was tried)
    bool found = false;
    std::string unreadable;                                        // found, but its gzip stream does not inflate: why
    uint64_t size = 0;                                             // of the file, inflated
    uint64_t off = 0, n = 0;                                       // its bytes that are compared: buffer[off, off + n)
    uint64_t gzOff = 0, gzLen = 0;                                 // --inflate device: its place [off, off + n) is empty, its gzip bytes are gz[gzOff, gzOff + gzLen) of the batch
};
struct OriginalsBatch { std::vector<Original> files; double ms = 0; uint64_t bytes = 0; std::string error; std::string gz; };
struct ValidateTimes { double read = 0, upload = 0, compare = 0, inflate = 0; uint64_t compared = 0, inflatedOnDevice = 0, inflatedAgainOnHost = 0; };

// where a unit's original lies: its line of <prefix>.names; --flat: the basename `d --fasta` writes it under; --root before relative names
static std::string originalPath(const std::string &name, const std::string &root, bool flat) {
    std::string n = flat ? outputName(name) : name;
    if (!root.empty() && (n.empty() || n[0] != '/')) n = root + "/" + n;
    return n;
}

// an original opened for reading: the path, or <path>.gz when the path does not exist (MBGC_Decoder.cpp:120-129); a file that starts
// with the gzip magic is inflated whole (mgmpInOpen)
struct OpenOriginal {
    int fd = -1; bool gz = false; uint64_t size = 0; std::string inflated;
    std::string compressed; bool deferred = false;                 // deferGz: a gzip file is left compressed, size = its ISIZE trailer, until inflateNow()
    std::string broken;                                            // a gzip file that does not inflate (corrupt, truncated): the inflate's message; size = 0
    ~OpenOriginal() { if (fd >= 0) close(fd); }
    void inflateNow() {
        deferred = false;
        if (!tryInflateGzip(compressed, inflated, broken)) inflated.clear();                       // (reported as an invalid file, not the end of the run)
        size = inflated.size();
    }
    bool open(const std::string &path, std::string &error, bool deferGz = false) {
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) fd = ::open((path + ".gz").c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) { error = "cannot read " + path; return true; }
        size = (uint64_t) st.st_size;
        uint8_t head[18];
        if (size >= 18 && pread(fd, head, 18, 0) == 18 && isGzip(head, 18)) {
            compressed.assign(size, '\0');
            if (!readAt(&compressed[0], 0, size)) { error = "cannot read " + path; return true; }
            gz = true;
            if (deferGz) {
                uint32_t isize;
                memcpy(&isize, compressed.data() + compressed.size() - 4, 4);
                size = isize; deferred = true;
            } else {
                inflateNow();
                std::string().swap(compressed);
            }
        }
        return true;
    }
    bool readAt(void *dst, uint64_t at, uint64_t n) const {
        if (gz) { memcpy(dst, inflated.data() + at, n); return true; }
        for (uint64_t got = 0; got < n;) {
            const ssize_t r = pread(fd, (char *) dst + got, n - got, (off_t) (at + got));
            if (r <= 0) return false;
            got += (uint64_t) r;
        }
        return true;
    }
};

// where the first difference lies (MBGC_Decoder.cpp:157-170 on the text's records instead of its '>' bytes): `at` bytes into the text
// of record `rec` of the file's records [first, ...). A difference at a record's first byte belongs to the record in front (the equal
// part ends behind it); at the file's first byte there is no record in the equal part.
struct ErrorLocation { enum Kind { NONE, NO_SEQUENCE, HEADER, SEQUENCE } kind = NONE; uint64_t seqIdx = 0, seqPos = 0; };
static ErrorLocation locateError(uint64_t first, uint64_t rec, uint64_t at, const std::vector<uint64_t> &hdrLen, const std::vector<uint64_t> &seqLen, uint64_t lineLen) {
    ErrorLocation loc;
    if (at == 0) {
        if (rec == first) { loc.kind = ErrorLocation::NO_SEQUENCE; return loc; }
        loc.kind = ErrorLocation::SEQUENCE; loc.seqIdx = rec - 1 - first; loc.seqPos = seqLen[rec - 1];
        return loc;
    }
    loc.seqIdx = rec - first;
    const uint64_t zs = hdrLen[rec] + 2;
    if (at < zs) { loc.kind = ErrorLocation::HEADER; return loc; }
    uint64_t line = (lineLen == 0 || lineLen > seqLen[rec]) ? seqLen[rec] : lineLen;
    if (line == 0) line = 1;
    const uint64_t p = at - zs;                                    // the newlines in front of zone offset p: one per full line
    loc.kind = ErrorLocation::SEQUENCE;
    loc.seqPos = std::min(seqLen[rec], p - p / (line + 1));
    return loc;
}
}

// the lines of <prefix>.names, held to the meta: one per unit (G0, then every target), one for a single-FASTA collection
static bool parseNames(const std::string &names, const MbgcMeta &meta, std::vector<std::string> &out, std::string &msg) {
    const size_t T = meta.targets.size();
    if (!names.empty() && names.back() != '\n') { msg = "malformed .names: the last line does not end"; return false; }
    for (size_t at = 0; at < names.size();) { const size_t e = names.find('\n', at); out.push_back(names.substr(at, e - at)); at = e + 1; }
    if (out.size() != (meta.singleFastaFile ? 1 : T + 1)) {
        msg = "malformed .names: " + std::to_string(out.size()) + " names for " + std::to_string(meta.singleFastaFile ? 1 : T + 1) + " units";
        return false;
    }
    return true;
}

// reads and checks the three side files against the meta: false and a message, or the layout
static bool readFastaLayout(const std::string &prefix, const MbgcMeta &meta, uint64_t contigs, FastaLayout &L, std::string &msg) {
    std::string names, lens;
    for (const char *ext : {"names", "headers", "dnaLineLengths"})
        if (!readFile(prefix + "." + ext, ext[0] == 'n' ? names : (ext[0] == 'h' ? L.headers : lens))) {
            msg = "malformed stream set: cannot open " + prefix + "." + ext + " (--fasta needs the names, headers and line lengths mbgc-hip c writes beside the streams)";
            return false;
        }
    const size_t T = meta.targets.size();
    if (!parseNames(names, meta, L.names, msg)) return false;
    if (!L.headers.empty() && L.headers.back() != '\n') { msg = "malformed .headers: the last header does not end"; return false; }
    for (size_t at = 0; at < L.headers.size();) {
        const char *e = (const char *) memchr(L.headers.data() + at, '\n', L.headers.size() - at);
        const size_t end = (size_t) (e - L.headers.data());
        L.hdrOff.push_back(at); L.hdrLen.push_back(end - at);
        at = end + 1;
    }
    if (L.hdrOff.size() != contigs) {
        msg = "malformed .headers: " + std::to_string(L.hdrOff.size()) + " headers for " + std::to_string(contigs) + " contigs";
        return false;
    }
    if (lens.size() != (T + 1) * sizeof(uint64_t)) {
        msg = "malformed .dnaLineLengths: " + std::to_string(lens.size()) + " bytes for " + std::to_string(T + 1) + " units";
        return false;
    }
    L.lineLen.resize(T + 1);
    memcpy(L.lineLen.data(), lens.data(), lens.size());
    // the files: one for a single-FASTA collection; else one per unit that is written (under -t1 the initial reference is the first
    // contig of target 0 again and is no file of its own)
    std::set<std::string> seen;
    for (size_t u = meta.singleFastaFile ? 0 : (meta.sequentialMatching ? 1 : 0); u < L.names.size(); u++) {
        const std::string o = outputName(L.names[u]);
        if (o.empty() || o == "." || o == "..") { msg = "naming: the unit '" + L.names[u] + "' has no file name to be written under"; return false; }
        if (!seen.insert(o).second) { msg = "naming: two units would be written to the same file " + o + " (the paths of the list are dropped)"; return false; }
        L.outNames.push_back(o);
    }
    return true;
}


int MBGC_Decoder::decode(const std::string &prefix, const std::string &outPrefix, const Options &opt, std::string *error) {
    auto fail = [&](const std::string &m) { if (error) *error = m; return 1; };
    std::string metaBytes;
    if (!readFile(prefix + ".meta", metaBytes)) return fail("cannot open " + prefix + ".meta (written by mbgc-hip c beside the streams)");
    MbgcMeta meta;
    { std::string e; if (!meta.parse(metaBytes, &e)) return fail(e); }
    if (opt.resident && meta.singleFastaFile)
        return fail("the streams hold one FASTA file (mbgc-hip c -i): a single-FASTA stream set is not repacked (it has one unit, and its elements are no files)");
    if (meta.rcRedundancyRemoval && !opt.restoreRc)
        return fail("the streams were written with -m 3: its reverse-complement pass over the literal stream (rcMapOff / rcMapLen) is not inverted by mbgc-hip d"
                    " unless --restore-rc is given");
    static const char *NAMES[SWSEM_NSTREAMS] = {"literals", "mapOff", "mapOff5th", "mapLen", "gapDelta", "flags"};
    std::string stream[SWSEM_NSTREAMS], locksPos, refExtSize;
    for (int s = 0; s < SWSEM_NSTREAMS; s++)
        if (!readFile(prefix + "." + NAMES[s], stream[s])) return fail("cannot open " + prefix + "." + NAMES[s]);
    if (!readFile(prefix + ".locksPos", locksPos) || !readFile(prefix + ".refExtSize", refExtSize)) return fail("cannot open " + prefix + ".locksPos / .refExtSize");
    // -m 3: the literals as they were before the reverse-complement pass cut them (MBGC_Decoder.cpp:1137), restored on the device
    // before anything reads them; the meta's stream index holds offsets into the uncut literals
    PgTools::SimpleSequenceMatcher::RestoreStats rcStats;
    double rcRestoreMs = 0;
    if (meta.rcRedundancyRemoval) {
        std::string rcMapOff, rcMapLen;
        if (!readFile(prefix + ".rcMapOff", rcMapOff) || !readFile(prefix + ".rcMapLen", rcMapLen)) return fail("cannot open " + prefix + ".rcMapOff / .rcMapLen");
        const size_t uncut = meta.index.empty() ? PgTools::SimpleSequenceMatcher::UNKNOWN_LENGTH : (size_t) meta.index[meta.index.size() - SWSEM_NSTREAMS + SWSEM_LIT];
        const std::string cutLiterals = opt.bench ? stream[SWSEM_LIT] : std::string();
        for (int run = 0; run < (opt.bench ? 2 : 1); run++) {                                   // (bench: the second run is the timed one)
            if (run) stream[SWSEM_LIT] = cutLiterals;
            std::string e;
            const double t0 = nowMs();
            if (!PgTools::SimpleSequenceMatcher::restoreRCMatchedSequence(stream[SWSEM_LIT], rcMapOff, rcMapLen, uncut, opt.device, &e, &rcStats))
                return fail("malformed stream set: " + e);
            rcRestoreMs = nowMs() - t0;
        }
    }
    const size_t T = meta.targets.size();
    if (T == 0) return fail("malformed stream set: no target");
    if (locksPos.size() != T * sizeof(uint64_t)) return fail("malformed stream set: locksPos does not hold one position per target");
    if (meta.maxRefLength < 64) return fail("malformed .meta: reference length");
    std::vector<uint64_t> lock(T);
    memcpy(lock.data(), locksPos.data(), locksPos.size());
    const bool lazy = meta.emit.lazyDecompressionSupport != 0;
    std::vector<uint64_t> extSize(T, 0);
    if (lazy) {
        size_t at = 0;
        for (size_t t = 0; t < T; t++) if (!readUInt64Frugal(refExtSize, at, extSize[t])) return fail("malformed stream set: refExtSize ends early");
        if (at != refExtSize.size()) return fail("malformed stream set: bytes left over in refExtSize");
    }
    // G0: the contigs at the head of the literal stream (MBGC_Decoder::decodeReference :265-317 / initReference :243-263)
    std::vector<uint64_t> contigLen;
    uint64_t lit0 = 0;
    for (uint32_t g = 0; g < meta.g0Contigs; g++) {
        const void *sep = lit0 < stream[SWSEM_LIT].size() ? memchr(stream[SWSEM_LIT].data() + lit0, SEQ_SEPARATOR_MARK, stream[SWSEM_LIT].size() - lit0) : nullptr;
        if (!sep) return fail("malformed stream set: the literals end inside the initial reference");
        const uint64_t end = (uint64_t) ((const char *) sep - stream[SWSEM_LIT].data());
        contigLen.push_back(end - lit0);
        lit0 = end + 1;
    }
    const uint64_t g0n = meta.g0Contigs, g0Bytes = lit0 - g0n;
    uint64_t planned = 0;
    std::vector<uint32_t> seqCount(T);
    for (size_t t = 0; t < T; t++) { seqCount[t] = meta.targets[t].seqsCount; planned += seqCount[t]; }
    if (planned > stream[SWSEM_LIT].size()) return fail("malformed .meta: more sequences than literal bytes");
    uint64_t sizes[SWSEM_NSTREAMS];
    for (int s = 0; s < SWSEM_NSTREAMS; s++) sizes[s] = stream[s].size();
    const bool wantFasta = !opt.fastaDir.empty() || opt.validate || opt.resident;   // (`v` builds the units and batches of --fasta, and formats them; `r` takes the units)
    FastaLayout layout;
    if (wantFasta) { std::string m; if (!readFastaLayout(prefix, meta, g0n + planned, layout, m)) return fail(m); }
    FastaTimes ftimes;
    ValidateTimes vtimes;
    uint64_t validFiles = 0, invalidFiles = 0, validatedFiles = 0;
    // chain starts
    const bool useIndex = !opt.noIndex && !meta.index.empty();
    std::vector<swsem_chain_start_t> starts;
    if (useIndex) {
        const uint64_t *ix = meta.index.data();
        if (ix[SWSEM_LIT] != lit0) return fail("malformed .meta: the stream index does not start behind the initial reference");
        for (size_t t = 0; t <= T; t++)
            for (int s = 0; s < SWSEM_NSTREAMS; s++)
                if (ix[t * SWSEM_NSTREAMS + s] > sizes[s] || (t && ix[t * SWSEM_NSTREAMS + s] < ix[(t - 1) * SWSEM_NSTREAMS + s]) || (t == T && ix[t * SWSEM_NSTREAMS + s] != sizes[s]))
                    return fail(std::string("malformed stream set: the index of ") + NAMES[s] + " does not fit the stream (target " + std::to_string(t) + ")");
        for (size_t t = 0; t < T; t++) {
            swsem_chain_start_t c = {};
            for (int s = 0; s < SWSEM_NSTREAMS; s++) { c.cur[s] = ix[t * SWSEM_NSTREAMS + s]; c.end[s] = ix[(t + 1) * SWSEM_NSTREAMS + s]; }
            c.firstTarget = (uint32_t) t; c.nTargets = 1; c.checkEnd = 1;
            starts.push_back(c);
        }
    } else {
        swsem_chain_start_t c = {};
        c.cur[SWSEM_LIT] = lit0;
        for (int s = 0; s < SWSEM_NSTREAMS; s++) c.end[s] = sizes[s];
        c.firstTarget = 0; c.nTargets = (uint32_t) T; c.checkEnd = 1;
        starts.push_back(c);
    }

    // ---- --select: the units to bring back (G0, then every target), by the names mbgc-hip c wrote beside the streams
    const bool selecting = !opt.select.empty();
    std::vector<char> unitSel(T + 1, 1);
    uint64_t selectedFiles = 0;
    if (selecting) {
        if (meta.singleFastaFile) return fail("--select: the streams hold one FASTA file (mbgc-hip c -i): it has one name, there is nothing to select");
        std::vector<std::string> own;
        if (!wantFasta) {
            std::string bytes, m;
            if (!readFile(prefix + ".names", bytes)) return fail("malformed stream set: cannot open " + prefix + ".names (--select needs the names mbgc-hip c writes beside the streams)");
            if (!parseNames(bytes, meta, own, m)) return fail(m);
        }
        const std::vector<std::string> &names = wantFasta ? layout.names : own;
        // (-t1: the first file is G0's unit and target 0; the selection is over output files, and G0's unit is none of them)
        for (size_t u = 0; u <= T; u++) {
            unitSel[u] = 0;
            if (u == 0 && meta.sequentialMatching) continue;
            for (const std::string &pat : opt.select) if (names[u].find(pat) != std::string::npos) unitSel[u] = 1;   // MBGC_Decoder.cpp:1022-1025
            selectedFiles += unitSel[u];
        }
        if (!selectedFiles) return fail("--select: no file of the collection matches (" + std::to_string(opt.select.size()) + " patterns against " + prefix + ".names)");
    }

    PassTimes times;
    uint64_t outBases = 0, outContigs = 0, plannedBases = 0, closureContigs = 0, closureBases = 0, dependencyTargets = 0;
    const int passes = opt.bench ? 2 : 1;                                                        // (bench: the second pass is the timed one)
    for (int pass = 0; pass < passes; pass++) {
        times = PassTimes();
        DevFree dev = {nullptr, {}};
        auto hipFail = [&](const char *what) { return fail(std::string(what) + ": " + swsem_last_error()); };
        if (swsem_create_decoder(&dev.h, meta.maxRefLength, opt.device)) return hipFail("decoder");
        swsem_t *h = dev.h;
        const uint8_t *sdev[SWSEM_NSTREAMS];
        for (int s = 0; s < SWSEM_NSTREAMS; s++) {
            void *p = nullptr;
            if (swsem_dev_malloc(h, sizes[s] + 64, &p)) return hipFail("streams");
            dev.ptrs.push_back(p);
            if (swsem_dev_upload(h, p, stream[s].data(), sizes[s])) return hipFail("streams");
            sdev[s] = (const uint8_t *) p;
        }
        // ---- the plan: once, ahead, for the whole collection
        std::vector<swsem_chain_contig_t> cc(planned);
        int firstBad = -1;
        double t0 = nowMs();
        if (planned && swsem_decode_plan_chain_dev(h, &meta.emit, sdev, sizes, (int) starts.size(), starts.data(), (int) T, seqCount.data(), lock.data(), planned, cc.data(), &firstBad))
            return hipFail("plan");
        times.plan = nowMs() - t0;
        if (firstBad >= 0)
            return fail("malformed stream set: " + (useIndex ? "target " + std::to_string(firstBad) + " does not decode from its offsets to the next target's"
                                                             : std::string("the collection's chain does not end with its streams")) + " (a stream ran out, or bytes were left over)");
        for (uint64_t c = 0; c < planned; c++) if (cc[c].unmatched < 0) return fail("malformed stream set: contig " + std::to_string(c) + " was not reached");
        contigLen.resize(g0n);
        for (uint64_t c = 0; c < planned; c++) contigLen.push_back(cc[c].destLen);
        const uint64_t N = g0n + planned;
        // ---- the load schedule: complete before a base exists
        RefState st;
        st.refTotalLength = meta.maxRefLength; st.lazyDecompressionSupport = lazy;
        std::vector<LoadSegment> g0Segs;
        if (!scheduleG0(st, g0Bytes, meta.rcInReference, meta.sequentialMatching, g0Segs)) return fail("malformed stream set: the initial reference does not fit the buffer");
        std::vector<std::vector<LoadSegment>> tSegs(T);
        {
            uint64_t c = 0;
            for (size_t t = 0; t < T; t++) {
                std::vector<ContigInfo> info(seqCount[t]);
                for (uint32_t s = 0; s < seqCount[t]; s++) info[s] = {cc[c + s].destLen, (uint64_t) cc[c + s].unmatched};
                const uint64_t before = st.loaded();
                if (!scheduleTarget(st, g0n + c, info, meta.targets[t].unmatchedFractionFactor, meta.targets[t].unmatchedFractionRCFactor, meta.rcInReference,
                                    meta.contigsIndividuallyReversed, lock[t], tSegs[t]))
                    return fail("malformed stream set: the loads of target " + std::to_string(t) + " do not fit its lock position");
                if (lazy && st.loaded() - before != extSize[t])
                    return fail("malformed stream set: target " + std::to_string(t) + " extends the reference by " + std::to_string(st.loaded() - before) +
                                " bytes, refExtSize says " + std::to_string(extSize[t]));
                c += seqCount[t];
            }
        }
        if (st.reachedRefLengthCount != meta.reachedRefLengthCount || (meta.finalRefLength && (st.reachedRefLengthCount ? st.refTotalLength : st.refPos) != meta.finalRefLength))
            return fail("malformed stream set: the rebuilt reference ends at " + std::to_string(st.refPos) + " after " + std::to_string(st.reachedRefLengthCount) +
                        " laps, the encoder's at " + std::to_string(meta.finalRefLength) + " after " + std::to_string(meta.reachedRefLengthCount));
        // ---- waves: targets whose contigs stand against the same frozen buffer are filled by one launch
        std::vector<std::vector<size_t>> segAt;
        const std::vector<FillUnit> units = partitionUnits(seqCount, lock, tSegs, cc, g0n, opt.serial || meta.sequentialMatching, segAt);
        // ---- --select: the closure, before a base exists. mark[c]: 0 = not filled, 1 = filled as a dependency, 2 = filled because selected
        std::vector<uint8_t> mark(planned, selecting ? 0 : 2);
        std::vector<char> targetRuns(T, 1);
        if (selecting) {
            std::vector<uint32_t> need((planned + 31) / 32, 0);
            std::vector<uint64_t> timeOf(planned, 0);
            t0 = nowMs();
            Provenance prov;
            prov.L = meta.maxRefLength;
            for (const LoadSegment &s : g0Segs) prov.add(s, g0n);
            uint64_t c = 0;
            for (size_t t = 0; t < T; t++) {
                // a contig's time: the loader's position just before its own first load in serial order — the state --serial fills it against
                uint32_t s = 0;
                for (size_t i = 0; i <= tSegs[t].size(); i++) {
                    for (; s < seqCount[t] && segAt[t][s] == i; s++) timeOf[c + s] = prov.cur;
                    if (i < tSegs[t].size()) prov.add(tSegs[t][i], g0n);
                }
                if (unitSel[t + 1]) for (uint32_t k = 0; k < seqCount[t]; k++) { mark[c + k] = 2; need[(c + k) >> 5] |= 1u << ((c + k) & 31); }
                c += seqCount[t];
            }
            std::vector<swsem_fill_unit_t> sweep;
            for (const FillUnit &u : units) if (u.c1 > u.c0) sweep.push_back({u.c0, u.c1});
            if (planned && swsem_decode_closure_dev(h, prov.L, prov.rows.size(), prov.rows.data(), planned, timeOf.data(), sweep.size(), sweep.data(), need.data()))
                return hipFail("closure");
            times.closure = nowMs() - t0;
            closureContigs = closureBases = dependencyTargets = 0;
            c = 0;
            for (size_t t = 0; t < T; t++) {
                bool any = false;
                for (uint32_t k = 0; k < seqCount[t]; k++, c++) {
                    if (!mark[c] && ((need[c >> 5] >> (c & 31)) & 1u)) mark[c] = 1;
                    if (mark[c]) { any = true; closureContigs++; closureBases += contigLen[g0n + c]; }
                }
                targetRuns[t] = any;
                if (any && !unitSel[t + 1]) dependencyTargets++;
            }
        }
        // the sequence buffer: G0, then the contigs that are filled — HBM and the download scale with the closure
        std::vector<uint64_t> seqOff(N + 1, 0);
        for (uint64_t c = 0; c < N; c++) seqOff[c + 1] = seqOff[c] + (c < g0n || mark[c - g0n] ? contigLen[c] : 0);
        const uint64_t totalBases = seqOff[N];
        void *seqp = nullptr;
        if (swsem_dev_malloc(h, totalBases + 64, &seqp)) return hipFail("sequences");
        dev.ptrs.push_back(seqp);
        uint8_t *seqDev = (uint8_t *) seqp;
        {   // G0's bytes are literals
            uint64_t at = 0;
            for (uint64_t g = 0; g < g0n; g++) {
                if (swsem_dev_copy(h, seqDev + seqOff[g], sdev[SWSEM_LIT] + at, contigLen[g])) return hipFail("initial reference");
                at += contigLen[g] + 1;
            }
        }
        // (a selection: only the segments whose contig is filled are loaded — separators and G0 always, a target's own reverse
        // complement when any of its contigs is filled; what is left out is read by nothing that is filled)
        auto toAbi = [&](const std::vector<LoadSegment> &in, size_t a, size_t b, bool targetRuns, std::vector<swsem_load_seg_t> &out) {
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
        };
        auto load = [&](std::vector<swsem_load_seg_t> &segs) -> bool {
            if (segs.empty()) return true;
            const double a = nowMs();
            const int r = swsem_decode_load_dev(h, seqDev, (int) segs.size(), segs.data());
            times.load += nowMs() - a;
            segs.clear();
            return r == 0;
        };
        auto fill = [&](uint64_t c0, uint64_t c1) -> int {                                      // planned contigs [c0, c1); 0 ok, 1 HIP, 2 bytes not as planned
            if (c1 == c0) return 0;
            const double a = nowMs();
            uint64_t nbad = 0;
            const int r = swsem_decode_fill_range_dev(h, c0, c1, seqDev, seqOff.data() + g0n, &nbad);
            times.fill += nowMs() - a;
            return r ? 1 : (nbad ? 2 : 0);
        };
        std::vector<swsem_load_seg_t> abi;
        toAbi(g0Segs, 0, g0Segs.size(), true, abi);
        if (!load(abi)) return hipFail("initial reference");
        // ---- the forward run: every unit's fill, then its loads (a selection: the runs of filled contigs inside the unit, one launch each)
        for (const FillUnit &u : units) {
            for (uint64_t c = u.c0; c < u.c1;) {
                if (!mark[c]) { c++; continue; }
                uint64_t e = c;
                while (e < u.c1 && mark[e]) e++;
                const int r = fill(c, e);
                if (r) return r == 2 ? fail("malformed stream set: the bytes of a contig do not come out as planned") : hipFail("fill");
                c = e;
            }
            uint64_t width = 0;
            for (size_t t = u.t0; t < u.t1; t++) {
                toAbi(tSegs[t], u.wave ? 0 : u.sA, u.wave ? tSegs[t].size() : u.sB, targetRuns[t], abi);
                width += targetRuns[t] ? 1 : 0;
            }
            if (!load(abi)) return hipFail("load");
            if (!selecting) width = u.counted;
            if (u.counted && width) { times.waves++; times.widest = std::max(times.widest, width); }
        }
        if (swsem_synchronize(h)) return hipFail("decode");
        const uint64_t outFrom = meta.sequentialMatching ? g0n : 0;                               // (-t1: the initial reference is the first contig of target 0 again)
        // what is written: the chosen units' contigs, in collection order, as ranges [from, to) of the collection's contigs
        std::vector<Interval> outRanges;
        outBases = outContigs = plannedBases = 0;
        {
            uint64_t c = 0;
            for (size_t u = 0; u <= T; u++) {
                const uint64_t n = u == 0 ? g0n : seqCount[u - 1];
                if (unitSel[u] && c + n > outFrom && n) {
                    const uint64_t from = std::max(c, outFrom);
                    if (!outRanges.empty() && outRanges.back().to == from) outRanges.back().to = c + n; else outRanges.push_back({from, c + n});
                }
                c += n;
            }
            for (const Interval &r : outRanges) for (uint64_t k = r.from; k < r.to; k++) { outBases += contigLen[k]; outContigs++; }
            for (uint64_t k = g0n; k < N; k++) plannedBases += contigLen[k];
        }
        if (opt.resident) {
            // ---- `mbgc-hip r`: the units --fasta would write, packed out of the sequence buffer — where the contigs of
            // the closure lie among them — into a buffer of the caller's input stage; this handle and all it holds end with the return
            ResidentCollection &R = *opt.resident;
            R.units.clear();
            std::vector<mbgc_fasta_pack_piece_t> pieces;
            uint64_t c = 0;
            for (size_t u = 0; u <= T; u++) {
                const uint64_t n = u == 0 ? g0n : seqCount[u - 1], c0 = c;
                c += n;
                if ((u == 0 && meta.sequentialMatching) || !unitSel[u]) continue;
                ResidentUnit x;
                x.name = layout.names[u];
                x.lineLen = R.lineLenGiven ? R.lineLen : layout.lineLen[u];
                for (uint64_t k = c0; k < c0 + n; k++) {
                    x.headers.append(layout.headers, layout.hdrOff[k], layout.hdrLen[k]); x.headers.push_back('\n');
                    x.contigLen.push_back(contigLen[k]);
                    x.text += recordText(layout.hdrLen[k], contigLen[k], x.lineLen);
                    pieces.push_back({seqOff[k], contigLen[k]});
                }
                R.units.push_back(std::move(x));
            }
            auto faFail = [&](const char *what) { return fail(std::string(what) + ": " + mbgc_fasta_last_error()); };
            if (mbgc_fasta_dev_alloc(R.fasta, outBases + 64, &R.packedDev)) return faFail("the chosen units' bases");
            std::vector<uint64_t> dstOff(pieces.size() + 1);
            if (mbgc_fasta_pack_dev(R.fasta, seqDev, totalBases, pieces.data(), pieces.size(), R.packFlags, R.packedDev, outBases + 64, dstOff.data(), &R.packKernelMs))
                return faFail("pack");
            R.packedBytes = dstOff[pieces.size()];
            if (R.packedBytes != outBases) return fail("internal error: the packed units are not the chosen contigs");
            R.contigsDecoded = g0n + (selecting ? closureContigs : planned); R.contigsChosen = outContigs;
            R.decodeMs = times.plan + times.closure + times.fill + times.load + rcRestoreMs;
            return 0;
        }
        if (wantFasta) {
            // ---- the FASTA files again: units in order, batches of whole units of at most FASTA_BATCH_TEXT bytes of
            // text; a batch is formatted on the device, downloaded into one of two page-locked buffers, and written by a thread of
            // its own while the next batch is formatted and downloaded into the other
            ftimes = FastaTimes();
            auto faFail = [&](const char *what) { return fail(std::string(what) + ": " + mbgc_fasta_last_error()); };
            std::vector<FastaUnit> units;
            std::vector<char> fileWanted(layout.outNames.size(), 0);
            {
                uint64_t c = 0;
                for (size_t u = 0; u <= T; u++) {
                    const uint64_t n = u == 0 ? g0n : seqCount[u - 1];
                    FastaUnit x = {c, c + n, layout.lineLen[u], 0, 0};
                    c += n;
                    if (u == 0 && meta.sequentialMatching) continue;
                    if (!unitSel[u]) continue;                                                  // (--select: no other file is made, empty ones included)
                    x.file = meta.singleFastaFile ? 0 : u - (meta.sequentialMatching ? 1 : 0);
                    fileWanted[x.file] = 1;
                    for (uint64_t k = x.c0; k < x.c1; k++) x.text += recordText(layout.hdrLen[k], contigLen[k], x.lineLen);
                    units.push_back(x);
                }
            }
            uint64_t maxBatch = 0, maxGz = 0;                                                    // (maxGz: --gzip, the most a batch's gzip files take)
            std::vector<size_t> batchEnd;                                                       // units [batchEnd[b - 1], batchEnd[b])
            {
                uint64_t cur = 0, curGz = 0;
                for (size_t u = 0; u < units.size(); u++) {
                    if (cur && cur + units[u].text > (opt.batchText ? opt.batchText : FASTA_BATCH_TEXT)) {
                        batchEnd.push_back(u); maxBatch = std::max(maxBatch, cur); maxGz = std::max(maxGz, curGz); cur = curGz = 0;
                    }
                    cur += units[u].text;
                    if (opt.gzip) curGz += mbgc_fasta_deflate_bound(units[u].text);
                }
                batchEnd.push_back(units.size()); maxBatch = std::max(maxBatch, cur); maxGz = std::max(maxGz, curGz);
            }
            const bool writeFiles = !opt.validate && (!opt.bench || pass == 0);                  // (bench: the timed pass formats and downloads only)
            if (std::string failed; writeFiles && !makeDirs(opt.fastaDir, &failed)) return fail("cannot create the directory " + failed);
            FastaBuffers fb;
            if (mbgc_fasta_create(&fb.fa, opt.device)) return faFail("--fasta");
            if (mbgc_fasta_dev_alloc(fb.fa, layout.headers.size() + 64, &fb.hdrDev)) return faFail("--fasta");
            for (uint8_t *&t : fb.textDev) if (mbgc_fasta_dev_alloc(fb.fa, maxBatch + 64, &t)) return faFail("--fasta");
            if (opt.gzip) for (uint8_t *&t : fb.gzDev) if (mbgc_fasta_dev_alloc(fb.fa, maxGz + 64, &t)) return faFail("--gzip");
            for (void *&p : fb.pin) if (mbgc_fasta_host_alloc(fb.fa, std::max<uint64_t>(opt.gzip ? maxGz : maxBatch, layout.headers.size()) + 64, &p)) return faFail("--fasta");
            {   // the headers go up through page-locked memory like everything else
                memcpy(fb.pin[0], layout.headers.data(), layout.headers.size());
                if (mbgc_fasta_upload(fb.fa, fb.hdrDev, fb.pin[0], layout.headers.size())) return faFail("--fasta");
            }
            // Batch b: formatted into device buffer b & 1; its download into page-locked buffer b & 1 begins at once, on a stream of
            // its own, and is waited for after batch b + 1 has been formatted into the other device buffer; then its writer starts,
            // once the writer of batch b - 1 has ended. So the download of b and the writes of b - 1 run beside the format of b + 1,
            // and page-locked buffer b & 1 is free again (writer b - 2 was waited for) before download b begins.
            struct Piece { size_t file; uint64_t off, len; bool first; };
            std::vector<char> opened(layout.outNames.size(), 0);
            std::vector<mbgc_fasta_format_rec_t> recs;
            std::vector<uint64_t> textOff;
            std::vector<Piece> inFlight;                                                         // the pieces of the batch whose download runs
            uint8_t *inFlightHost = nullptr;
            bool downloading = false;
            auto settle = [&]() -> int {                                                        // the running download -> its writer; 0 ok, 1 device, 2 write
                if (!downloading) return 0;
                double cms = 0;
                if (mbgc_fasta_download_wait(fb.fa, &cms)) return 1;
                ftimes.download += cms;
                downloading = false;
                const double w0 = nowMs();
                const bool ok = !fb.writing.valid() || fb.writing.get();
                ftimes.write += nowMs() - w0;                                                   // (what the writes hold the pipeline up by)
                if (!ok) return 2;
                if (writeFiles) {
                    const std::string dir = opt.fastaDir, suffix = opt.gzip ? ".gz" : "";
                    const std::vector<std::string> *outNames = &layout.outNames;
                    const std::vector<Piece> pieces = inFlight;
                    const uint8_t *host = inFlightHost;
                    fb.writing = std::async(std::launch::async, [pieces, host, dir, suffix, outNames] {
                        for (const Piece &p : pieces) {
                            std::ofstream f(dir + "/" + (*outNames)[p.file] + suffix, std::ios::binary | (p.first ? std::ios::trunc : std::ios::app));
                            f.write((const char *) host + p.off, (std::streamsize) p.len);
                            f.close();                                                          // (an error may only show when the last bytes leave the buffer)
                            if (!f) return false;
                        }
                        return true;
                    });
                }
                return 0;
            };
            auto settleFail = [&](int r) { return r == 1 ? faFail("download") : fail("cannot write under " + opt.fastaDir); };
            // units [u0, u1) formatted into dst: recs and textOff hold the batch's record table afterwards; false: the device call failed
            auto formatBatch = [&](size_t u0, size_t u1, uint8_t *dst, uint64_t &bytes) -> bool {
                recs.clear();
                for (size_t u = u0; u < u1; u++)
                    for (uint64_t k = units[u].c0; k < units[u].c1; k++)
                        recs.push_back({seqOff[k], contigLen[k], layout.hdrOff[k], layout.hdrLen[k], units[u].lineLen});
                textOff.assign(recs.size() + 1, 0);
                double kms = 0;
                if (mbgc_fasta_format_dev(fb.fa, seqDev, totalBases, fb.hdrDev, layout.headers.size(), recs.data(), recs.size(), dst, maxBatch, textOff.data(), &kms))
                    return false;
                ftimes.format += kms;
                bytes = textOff[recs.size()];
                ftimes.text += bytes; ftimes.batches++;
                return true;
            };
            size_t u0 = 0;
            if (opt.validate) {
                // ---- `mbgc-hip v`: the text stays on the device. Batch b is formatted into the first text buffer while a
                // thread reads (and inflates) the originals of batch b + 1 into the page-locked buffer that batch b - 1 left; the
                // originals of b go up into the second text buffer, one compare call runs over the batch with a slot per file, and a
                // word per file comes back. A single-FASTA collection is one file over all batches: one piece per batch at the
                // file's running offset, only that slice of the original is read and uploaded.
                const bool report = pass + 1 == passes;                                         // (bench: the first pass warms up and stays quiet)
                const bool single = meta.singleFastaFile;
                const size_t nb = batchEnd.size();
                vtimes = ValidateTimes();
                validFiles = invalidFiles = 0;
                validatedFiles = single ? 1 : units.size();
                uint64_t dumped = 0;
                auto nameOf = [&](const FastaUnit &x) { return originalPath(layout.names[single ? 0 : x.file + (meta.sequentialMatching ? 1 : 0)], opt.root, opt.flat); };
                if (report && !opt.skipCompare && meta.uppercaseDNA)
                    printf("the streams were written with -U: the text is upper case, originals that hold lower-case bases differ from it\n");
                std::vector<uint64_t> batchAt(nb + 1, 0);                                        // text in front of every batch
                for (size_t b = 0, u = 0; b < nb; b++) { batchAt[b + 1] = batchAt[b]; for (; u < batchEnd[b]; u++) batchAt[b + 1] += units[u].text; }
                const uint64_t totalText = batchAt[nb];
                OpenOriginal one;                                                               // the single file, open over all batches
                bool oneFound = false, oneDiffers = false;
                ErrorLocation oneLoc;
                const std::string onePath = single && !units.empty() ? nameOf(units[0]) : std::string();
                if (single && !opt.skipCompare) {
                    const double r0 = nowMs();
                    std::string e;
                    oneFound = one.open(onePath, e);
                    if (!e.empty()) return fail(e);
                    vtimes.read += nowMs() - r0;
                }
                auto readBatch = [&](size_t b) {
                    OriginalsBatch R;
                    const double r0 = nowMs();
                    uint8_t *dst = (uint8_t *) fb.pin[b & 1];
                    const size_t ua = b ? batchEnd[b - 1] : 0, ub = batchEnd[b];
                    if (single) {
                        Original o;
                        o.path = onePath; o.found = oneFound; o.size = one.size; o.unreadable = one.broken;
                        if (oneFound && batchAt[b] < one.size) {
                            o.n = std::min(batchAt[b + 1] - batchAt[b], one.size - batchAt[b]);
                            if (!one.readAt(dst, batchAt[b], o.n)) R.error = "cannot read " + onePath;
                        }
                        R.bytes = o.n;
                        R.files.push_back(o);
                    } else {
                        for (size_t u = ua; u < ub && R.error.empty(); u++) {
                            Original o;
                            OpenOriginal f;
                            o.path = nameOf(units[u]);
                            o.found = f.open(o.path, R.error, opt.inflateOnDevice);
                            if (o.found && R.error.empty() && f.deferred) {
                                // a gzip original whose trailer states the length of our text goes up compressed and is inflated into its
                                // place beside the batch; any other one differs in size already and is inflated here, for its size
                                if (f.size == units[u].text) {
                                    o.size = o.n = f.size; o.off = R.bytes; R.bytes += o.n;
                                    o.gzOff = R.gz.size(); o.gzLen = f.compressed.size();
                                    R.gz += f.compressed;
                                    R.gz.resize((R.gz.size() + 15) & ~(size_t) 15);
                                    R.files.push_back(o);
                                    continue;
                                }
                                f.inflateNow();
                            }
                            if (o.found && R.error.empty()) {
                                o.unreadable = f.broken;
                                o.size = f.size; o.off = R.bytes; o.n = std::min(f.size, units[u].text);
                                if (!f.readAt(dst + o.off, 0, o.n)) R.error = "cannot read " + o.path;
                                R.bytes += o.n;
                            }
                            R.files.push_back(o);
                        }
                    }
                    R.ms = nowMs() - r0;
                    return R;
                };
                auto reportInvalid = [&](const std::string &path, bool sizeDiffer, uint64_t ours, uint64_t theirs, const ErrorLocation &loc) {
                    if (!report || invalidFiles >= VALIDATION_LOG_LIMIT) return;
                    const unsigned long long n = validFiles + invalidFiles;
                    if (sizeDiffer) printf("Validation ERROR: ~%llu. %s size differ (%llu instead of %llu)\n", n, path.c_str(), (unsigned long long) ours, (unsigned long long) theirs);
                    else printf("Validation ERROR: ~%llu. %s contents differ.\n", n, path.c_str());
                    if (loc.kind == ErrorLocation::SEQUENCE) printf("Error location:\t\tseqIdx = %llu\tseqPos = %llu\n", (unsigned long long) loc.seqIdx, (unsigned long long) loc.seqPos);
                    else if (loc.kind == ErrorLocation::HEADER) printf("Error in header:\t\tseqIdx = %llu\n", (unsigned long long) loc.seqIdx);
                    else if (loc.kind == ErrorLocation::NO_SEQUENCE) printf("Error in FASTA format - no sequences found in equal part.\n");
                };
                // the record of unit x (its text starts at `at` in the batch, its records at row `rec` of the batch's table) that holds text offset pos of the unit
                auto locate = [&](const FastaUnit &x, uint64_t at, size_t rec, uint64_t pos, uint64_t firstContig) {
                    const size_t nrec = (size_t) (x.c1 - x.c0);
                    if (nrec == 0) return locateError(firstContig, firstContig, 0, layout.hdrLen, contigLen, x.lineLen);
                    const size_t j = (size_t) (std::upper_bound(textOff.begin() + rec, textOff.begin() + rec + nrec, at + pos) - (textOff.begin() + rec)) - 1;
                    return locateError(firstContig, x.c0 + j, at + pos - textOff[rec + j], layout.hdrLen, contigLen, x.lineLen);
                };
                auto dumpText = [&](const std::string &name, const uint8_t *src, uint64_t n, bool append) -> int {     // 0 ok, 1 device, 2 write
                    std::string text(n, '\0');
                    if (n && mbgc_fasta_download(fb.fa, &text[0], src, n)) return 1;
                    if (std::string failed; !makeDirs(opt.dumpDir, &failed)) return 2;
                    std::ofstream f(opt.dumpDir + "/" + name, std::ios::binary | (append ? std::ios::app : std::ios::trunc));
                    f.write(text.data(), (std::streamsize) n);
                    f.close();
                    return f ? 0 : 2;
                };
                auto dumpFail = [&](int r) { return r == 1 ? faFail("--dump") : fail("cannot write under " + opt.dumpDir); };
                std::vector<mbgc_fasta_compare_piece_t> pieces;
                std::vector<uint64_t> firstDiff;
                uint8_t *gzDev = nullptr; uint64_t gzDevCap = 0;                                    // --inflate device: a batch's gzip bytes in HBM
                struct FreeGz { mbgc_fasta_t *fa; uint8_t *&p; ~FreeGz() { if (p) mbgc_fasta_dev_free(fa, p); } } freeGz{fb.fa, gzDev};
                std::future<OriginalsBatch> reading;
                if (!opt.skipCompare && nb) reading = std::async(std::launch::async, readBatch, (size_t) 0);
                for (size_t b = 0; b < nb; b++) {
                    const size_t u1 = batchEnd[b];
                    OriginalsBatch R;
                    if (!opt.skipCompare) {
                        R = reading.get();
                        if (b + 1 < nb) reading = std::async(std::launch::async, readBatch, b + 1);
                        if (!R.error.empty()) return fail(R.error);
                        vtimes.read += R.ms;
                    }
                    uint64_t bytes = 0;
                    if (!formatBatch(u0, u1, fb.textDev[0], bytes)) return faFail("format");
                    if (bytes != batchAt[b + 1] - batchAt[b]) return fail("internal error: the text of a batch is not the sum of its units");
                    if (opt.skipCompare) { u0 = u1; continue; }
                    const double up0 = nowMs();
                    if (R.gz.empty()) { if (mbgc_fasta_upload(fb.fa, fb.textDev[1], fb.pin[b & 1], R.bytes)) return faFail("upload"); }
                    else {
                        // --inflate device: the plain originals go up run by run, the gzip ones compressed, and those are inflated into their
                        // places. A job that does not end with exactly the text's length is done again by tryInflateGzip, as --inflate
                        // host does it: its verdict, its size and its message are the ones reported.
                        for (size_t i = 0; i < R.files.size();) {
                            size_t j = i;
                            while (j < R.files.size() && !R.files[j].gzLen) j++;
                            if (j > i) {
                                const uint64_t a = R.files[i].off, e = R.files[j - 1].off + R.files[j - 1].n;
                                if (e > a && mbgc_fasta_upload(fb.fa, fb.textDev[1] + a, (const uint8_t *) fb.pin[b & 1] + a, e - a)) return faFail("upload");
                            }
                            while (j < R.files.size() && R.files[j].gzLen) j++;
                            i = j;
                        }
                        if (R.gz.size() + 64 > gzDevCap) {
                            if (gzDev && mbgc_fasta_dev_free(fb.fa, gzDev)) return faFail("upload");
                            gzDev = nullptr; gzDevCap = R.gz.size() + R.gz.size() / 4 + 64;
                            if (mbgc_fasta_dev_alloc(fb.fa, gzDevCap, &gzDev)) return faFail("upload");
                        }
                        if (mbgc_fasta_upload(fb.fa, gzDev, R.gz.data(), R.gz.size())) return faFail("upload");
                        std::vector<mbgc_fasta_inflate_job_t> jobs;
                        std::vector<size_t> jobFile;
                        for (size_t i = 0; i < R.files.size(); i++)
                            if (R.files[i].gzLen) { jobs.push_back({R.files[i].gzOff, R.files[i].gzLen, R.files[i].off, R.files[i].n}); jobFile.push_back(i); }
                        std::vector<mbgc_fasta_inflate_result_t> res(jobs.size());
                        double ims = 0;
                        if (mbgc_fasta_inflate_dev(fb.fa, gzDev, R.gz.size(), fb.textDev[1], R.bytes, jobs.data(), jobs.size(), res.data(), &ims)) return faFail("inflate");
                        vtimes.inflate += ims;
                        for (size_t k = 0; k < jobs.size(); k++) {
                            Original &o = R.files[jobFile[k]];
                            if (res[k].status == MBGC_INFLATE_OK && res[k].outLen == o.n) { vtimes.inflatedOnDevice++; continue; }
                            vtimes.inflatedAgainOnHost++;
                            std::string text;
                            if (!tryInflateGzip(R.gz.substr(o.gzOff, o.gzLen), text, o.unreadable)) text.clear();
                            o.size = text.size();
                            o.n = std::min<uint64_t>(o.size, o.n);                                  // (its place is as long as our text)
                            if (o.n && mbgc_fasta_upload(fb.fa, fb.textDev[1] + o.off, text.data(), o.n)) return faFail("upload");
                        }
                    }
                    vtimes.upload += nowMs() - up0;
                    pieces.clear();
                    if (single) pieces.push_back({0, 0, R.files[0].n, 0});
                    else {
                        uint64_t at = 0;
                        for (size_t u = u0; u < u1; u++) { pieces.push_back({at, R.files[u - u0].off, R.files[u - u0].n, (uint32_t) (u - u0)}); at += units[u].text; }
                    }
                    firstDiff.assign(R.files.size(), UINT64_MAX);
                    double kms = 0;
                    if (mbgc_fasta_compare_dev(fb.fa, fb.textDev[0], bytes, fb.textDev[1], R.bytes, pieces.data(), pieces.size(), firstDiff.data(), (uint32_t) firstDiff.size(), &kms))
                        return faFail("compare");
                    vtimes.compare += kms;
                    for (const mbgc_fasta_compare_piece_t &pc : pieces) vtimes.compared += pc.len;
                    if (single) {
                        // the first difference, or — sizes differ, bytes do not — the end of the shorter of the two, in the batch that holds it
                        uint64_t pos = UINT64_MAX;
                        const uint64_t commonEnd = std::min(totalText, one.size);
                        if (oneFound && oneLoc.kind == ErrorLocation::NONE) {
                            if (firstDiff[0] != UINT64_MAX) { pos = firstDiff[0]; oneDiffers = true; }
                            else if (one.size != totalText && commonEnd >= batchAt[b] && (commonEnd < batchAt[b + 1] || b + 1 == nb)) pos = commonEnd - batchAt[b];
                        }
                        uint64_t at = 0;
                        size_t rec = 0;
                        for (size_t u = u0; u < u1 && pos != UINT64_MAX; u++) {
                            if (pos < at + units[u].text || u + 1 == u1) { oneLoc = locate(units[u], at, rec, pos - at, units[0].c0); break; }
                            at += units[u].text; rec += (size_t) (units[u].c1 - units[u].c0);
                        }
                    } else {
                        uint64_t at = 0;
                        size_t rec = 0;
                        for (size_t u = u0; u < u1; u++) {
                            const FastaUnit &x = units[u];
                            const Original &o = R.files[u - u0];
                            if (!o.found) {
                                if (report && invalidFiles < VALIDATION_LOG_LIMIT) fprintf(stderr, "Cannot find %s for validation.\n", o.path.c_str());
                                invalidFiles++;
                            } else if (!o.unreadable.empty()) {
                                if (report && invalidFiles < VALIDATION_LOG_LIMIT) fprintf(stderr, "Cannot read %s for validation: %s\n", o.path.c_str(), o.unreadable.c_str());
                                invalidFiles++;
                            } else if (o.size == x.text && firstDiff[u - u0] == UINT64_MAX) validFiles++;
                            else {
                                const uint64_t pos = firstDiff[u - u0] != UINT64_MAX ? firstDiff[u - u0] : std::min(x.text, o.size);
                                reportInvalid(o.path, o.size != x.text, x.text, o.size, locate(x, at, rec, pos, x.c0));
                                invalidFiles++;
                                if (report && !opt.dumpDir.empty() && dumped++ < VALIDATION_DUMP_LIMIT)
                                    if (const int r = dumpText(layout.outNames[x.file], fb.textDev[0] + at, x.text, false)) return dumpFail(r);
                            }
                            at += x.text; rec += (size_t) (x.c1 - x.c0);
                        }
                    }
                    u0 = u1;
                }
                if (single && !opt.skipCompare) {                                               // one file: its verdict, and its size, after the last batch
                    if (!oneFound) {
                        if (report) fprintf(stderr, "Cannot find %s for validation.\n", onePath.c_str());
                        invalidFiles++;
                    } else if (!one.broken.empty()) {
                        if (report) fprintf(stderr, "Cannot read %s for validation: %s\n", onePath.c_str(), one.broken.c_str());
                        invalidFiles++;
                    } else if (one.size == totalText && !oneDiffers) validFiles++;
                    else {
                        reportInvalid(onePath, one.size != totalText, totalText, one.size, oneLoc);
                        invalidFiles++;
                        if (report && !opt.dumpDir.empty()) {                                   // (the text of the earlier batches is gone: formatted once more)
                            const FastaTimes keep = ftimes;
                            size_t a = 0;
                            for (size_t b = 0; b < nb; a = batchEnd[b], b++) {
                                uint64_t bytes = 0;
                                if (!formatBatch(a, batchEnd[b], fb.textDev[0], bytes)) return faFail("format");
                                if (const int r = dumpText(layout.outNames[0], fb.textDev[0], bytes, b != 0)) return dumpFail(r);
                            }
                            ftimes = keep;
                        }
                    }
                }
                if (report && !opt.skipCompare) {
                    printf("Validation%s: correctly decoded %llu out of %llu files.\n", invalidFiles ? " ERROR" : "", (unsigned long long) validFiles, (unsigned long long) validatedFiles);
                    if (invalidFiles) fprintf(stderr, "Validation ERROR: errors in contents of %llu decoded files.\n", (unsigned long long) invalidFiles);
                }
            } else
            for (size_t b = 0; b < batchEnd.size(); b++) {
                const size_t u1 = batchEnd[b];
                uint64_t bytes = 0;
                if (!formatBatch(u0, u1, fb.textDev[b & 1], bytes)) return faFail("format");
                if (const int r = settle()) return settleFail(r);                               // batch b - 1: it travelled beside this batch's format
                // (the writer of b - 2, which read page-locked buffer b & 1, was waited for by that settle or the one before)
                inFlight.clear();
                uint64_t at = 0;
                for (size_t u = u0; u < u1; u++) {
                    inFlight.push_back({units[u].file, at, units[u].text, !opened[units[u].file]});
                    opened[units[u].file] = 1;
                    at += units[u].text;
                }
                if (at != bytes) return fail("internal error: the text of a batch is not the sum of its units");
                const uint8_t *src = fb.textDev[b & 1];
                if (opt.gzip) {
                    // --gzip: one deflate call over the batch, a job per piece; a piece becomes one gzip member, appended to its file
                    // like the text would be, and only the gzip bytes travel (gzDev[b & 1]: the download of batch b - 2 has been settled)
                    std::vector<mbgc_fasta_deflate_job_t> jobs;
                    for (const Piece &pc : inFlight) jobs.push_back({pc.off, pc.len});
                    std::vector<mbgc_fasta_deflate_result_t> res(jobs.size());
                    uint64_t gzBytes = 0;
                    double dms = 0;
                    if (mbgc_fasta_deflate_dev(fb.fa, fb.textDev[b & 1], bytes, jobs.data(), jobs.size(), fb.gzDev[b & 1], maxGz, res.data(), &gzBytes, &dms)) return faFail("deflate");
                    for (size_t k = 0; k < res.size(); k++) {
                        inFlight[k].off = res[k].outOff; inFlight[k].len = res[k].outLen;
                        ftimes.chunks += res[k].chunks; ftimes.storedChunks += res[k].storedChunks;
                    }
                    ftimes.deflate += dms; ftimes.gz += gzBytes;
                    bytes = gzBytes;
                    src = fb.gzDev[b & 1];
                }
                inFlightHost = (uint8_t *) fb.pin[b & 1];
                if (mbgc_fasta_download_begin(fb.fa, inFlightHost, src, bytes)) return faFail("download");
                downloading = true;
                u0 = u1;
            }
            if (const int r = settle()) return settleFail(r);
            const double w0 = nowMs();
            if (fb.writing.valid() && !fb.writing.get()) return fail("cannot write under " + opt.fastaDir);
            ftimes.write += nowMs() - w0;
            // (files of units without a record exist too, empty)
            static const unsigned char emptyGz[20] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (--gzip: the gzip file of no text)
            if (writeFiles)
                for (size_t f = 0; f < opened.size(); f++)
                    if (!opened[f] && fileWanted[f] && !writeFile(opt.fastaDir + "/" + layout.outNames[f] + (opt.gzip ? ".gz" : ""), opt.gzip ? (const char *) emptyGz : "", opt.gzip ? sizeof emptyGz : 0))
                        return fail("cannot write under " + opt.fastaDir);
        }

        if (pass + 1 == passes && !opt.bench && !opt.validate) {
            std::string seq(outBases, '\0');
            std::vector<uint64_t> outLens;
            {
                uint64_t at = 0;
                for (const Interval &r : outRanges) {                                           // (a unit's contigs lie back to back in the buffer)
                    const uint64_t n = seqOff[r.to] - seqOff[r.from];
                    if (n && swsem_dev_download(h, &seq[at], seqDev + seqOff[r.from], n)) return hipFail("download");
                    at += n;
                    outLens.insert(outLens.end(), contigLen.begin() + r.from, contigLen.begin() + r.to);
                }
            }
            std::vector<uint32_t> counts;
            if (!meta.sequentialMatching && unitSel[0]) counts.push_back(meta.g0Contigs);
            for (size_t t = 0; t < T; t++) if (unitSel[t + 1]) counts.push_back(seqCount[t]);
            if (!opt.closureOut.empty() && !writeFile(opt.closureOut, mark.data(), mark.size())) return fail("cannot write " + opt.closureOut);
            if (!writeFile(outPrefix + ".seq", seq.data(), seq.size()) ||
                !writeFile(outPrefix + ".contigLens", outLens.data(), outLens.size() * sizeof(uint64_t)) ||
                !writeFile(outPrefix + ".seqCounts", counts.data(), counts.size() * sizeof(uint32_t)))
                return fail("cannot write " + outPrefix + ".seq / .contigLens / .seqCounts");
        }
    }
    if (opt.bench && opt.validate && opt.inflateOnDevice)
        printf("{\"inflate_kernel_ms\": %.3f, \"inflated_on_device\": %llu, \"inflated_again_on_host\": %llu}\n", vtimes.inflate, (unsigned long long) vtimes.inflatedOnDevice,
               (unsigned long long) vtimes.inflatedAgainOnHost);
    if (opt.bench && opt.validate) {
        // one line: the comparison, and the headline fields of `d --bench` (the restore of -m 3 counts into the decode's time as it does there)
        const double ms = times.plan + times.closure + times.fill + times.load + rcRestoreMs;
        printf("{\"metric\": \"compared GB/s (validate: compare kernel, text and originals in HBM)\", \"value\": %.4f, \"unit\": \"GB/s\", \"compared_bytes\": %llu, "
               "\"compare_kernel_ms\": %.3f, \"upload_ms\": %.3f, \"read_inflate_ms\": %.3f, \"files\": %llu, \"valid\": %llu, \"text_bytes\": %llu, \"batches\": %llu, "
               "\"format_kernel_ms\": %.3f, \"decode_gbases_per_s\": %.4f, \"bases\": %llu, \"plan_ms\": %.3f, \"fill_ms\": %.3f, \"load_ms\": %.3f, \"targets\": %zu, "
               "\"waves\": %llu, \"serial\": %s, \"index\": %s}\n",
               vtimes.compare > 0 ? vtimes.compared / (vtimes.compare * 1e-3) / 1e9 : 0.0, (unsigned long long) vtimes.compared, vtimes.compare, vtimes.upload, vtimes.read,
               (unsigned long long) validatedFiles, (unsigned long long) validFiles, (unsigned long long) ftimes.text, (unsigned long long) ftimes.batches, ftimes.format,
               outBases / (ms * 1e-3) / 1e9, (unsigned long long) outBases, times.plan, times.fill, times.load, T, (unsigned long long) times.waves,
               opt.serial ? "true" : "false", useIndex ? "true" : "false");
    }
    if (opt.bench && !opt.validate) {
        // --restore-rc on -m 3 streams: the whole restore (upload of the cut literals, plan, fill, download) counts into the headline
        char rcJson[160] = "";
        if (meta.rcRedundancyRemoval)
            snprintf(rcJson, sizeof rcJson, ", \"rc_restore_ms\": %.3f, \"rc_marks\": %llu, \"rc_max_chain\": %llu", rcRestoreMs,
                     (unsigned long long) rcStats.marks, (unsigned long long) rcStats.maxChain);
        char selJson[256] = "";
        if (selecting)
            snprintf(selJson, sizeof selJson, ", \"closure_ms\": %.3f, \"closure_contigs\": %llu, \"closure_bases\": %llu, \"selected_targets\": %llu, \"dependency_targets\": %llu",
                     times.closure, (unsigned long long) closureContigs, (unsigned long long) closureBases, (unsigned long long) selectedFiles, (unsigned long long) dependencyTargets);
        const double ms = times.plan + times.closure + times.fill + times.load + rcRestoreMs;
        printf("{\"metric\": \"output Gbases/s (decompress: streams in HBM to sequences in HBM)\", \"value\": %.4f, \"unit\": \"Gbases/s\", \"bases\": %llu, "
               "\"plan_ms\": %.3f, \"fill_ms\": %.3f, \"load_ms\": %.3f, \"targets\": %zu, \"chain_starts\": %zu, \"plan_ms_per_target\": %.4f, \"waves\": %llu, "
               "\"serial\": %s, \"index\": %s%s%s}\n",
               outBases / (ms * 1e-3) / 1e9, (unsigned long long) outBases, times.plan, times.fill, times.load, T, starts.size(), times.plan / (double) T,
               (unsigned long long) times.waves, opt.serial ? "true" : "false", useIndex ? "true" : "false", rcJson, selJson);
    }
    if (opt.bench && wantFasta && !opt.validate)
        printf("{\"metric\": \"FASTA text GB/s (format kernel)\", \"value\": %.4f, \"unit\": \"GB/s\", \"text_bytes\": %llu, \"batches\": %llu, "
               "\"format_kernel_ms\": %.3f, \"download_ms\": %.3f, \"write_ms\": %.3f}\n",
               ftimes.format > 0 ? ftimes.text / (ftimes.format * 1e-3) / 1e9 : 0.0, (unsigned long long) ftimes.text, (unsigned long long) ftimes.batches,
               ftimes.format, ftimes.download, ftimes.write);
    if (opt.bench && wantFasta && !opt.validate && opt.gzip)
        printf("{\"metric\": \"gzip GB/s of text (deflate kernels)\", \"value\": %.4f, \"unit\": \"GB/s\", \"text_bytes\": %llu, \"gz_bytes\": %llu, "
               "\"deflate_kernel_ms\": %.3f, \"download_ms\": %.3f, \"write_ms\": %.3f, \"chunks\": %llu, \"stored_chunks\": %llu}\n",
               ftimes.deflate > 0 ? ftimes.text / (ftimes.deflate * 1e-3) / 1e9 : 0.0, (unsigned long long) ftimes.text, (unsigned long long) ftimes.gz, ftimes.deflate,
               ftimes.download, ftimes.write, (unsigned long long) ftimes.chunks, (unsigned long long) ftimes.storedChunks);
    if (selecting)
        printf("closure: %llu of %llu contigs, %llu of %llu bases, %llu selected, %llu dependency targets\n", (unsigned long long) closureContigs, (unsigned long long) planned,
               (unsigned long long) closureBases, (unsigned long long) plannedBases, (unsigned long long) selectedFiles, (unsigned long long) dependencyTargets);
    printf("waves: %llu for %zu targets\n", (unsigned long long) times.waves, T);
    printf("widest wave: %llu targets\n", (unsigned long long) times.widest);
    printf("decoded: %llu contigs, %llu bases\n", (unsigned long long) outContigs, (unsigned long long) outBases);
    return opt.validate && invalidFiles ? 2 : 0;
}

bool mbgc_hip_read_pattern_list(const char *path, std::vector<std::string> &out) {
    std::ifstream f(path);
    if (!f) return false;
    for (std::string line; std::getline(f, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty()) out.push_back(line);
    }
    return true;
}

int mbgc_hip_decompress_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--serial") opt.serial = true;
        else if (a == "--no-index") opt.noIndex = true;
        else if (a == "--bench") opt.bench = true;
        else if (a == "--restore-rc") opt.restoreRc = true;
        else if (a == "--fasta" && i + 1 < argc) opt.fastaDir = argv[++i];
        else if (a == "--gzip") opt.gzip = true;
        else if (a == "--batch-kib" && i + 1 < argc) opt.batchText = (uint64_t) atoll(argv[++i]) << 10;
        else if (a == "--select" && i + 1 < argc) { opt.select.push_back(argv[++i]); selectAsked = true; }
        else if (a == "--select-list" && i + 1 < argc) {
            if (!mbgc_hip_read_pattern_list(argv[++i], opt.select)) { fprintf(stderr, "mbgc-hip d: cannot open the pattern list %s\n", argv[i]); return EXIT_FAILURE; }
            selectAsked = true;
        }
        else if (a == "--closure-out" && i + 1 < argc) opt.closureOut = argv[++i];
        else if (a == "-d" && i + 1 < argc) opt.device = atoi(argv[++i]);
        else pos.push_back(a);
    }
    if (pos.size() != 2) {
        fprintf(stderr, "usage: mbgc-hip d [--serial] [--no-index] [--bench] [--restore-rc] [--fasta dir [--gzip] [--batch-kib K]] [--select pattern]...\n"
                        "                  [--select-list file] [--closure-out file] [-d device] <streamsPrefix> <outputPrefix>\n"
                        "  rebuilds every sequence of the collection from the raw streams and <streamsPrefix>.meta of mbgc-hip c, on the device; writes\n"
                        "  <outputPrefix>.seq (the bases of all contigs back to back), .contigLens (u64 each) and .seqCounts (u32 per file or target)\n"
                        "  --fasta dir: also the input FASTA files again, formatted on the device, as <dir>/<basename of each name of the list> (a .gz suffix\n"
                        "  is dropped: the text is written inflated; -i: the one file) from <streamsPrefix>.names / .headers / .dnaLineLengths\n"
                        "  --gzip (with --fasta): every file is written as <name>.gz, compressed on the device (one encoder: no level; the bytes are a\n"
                        "  function of the text alone); a file whose text spans batches is several gzip members back to back, which zlib, gzip -d and\n"
                        "  mbgc-hip v read as one text. --batch-kib K: text per batch (default 262144)\n"
                        "  --serial: contig by contig, each contig's loads before the next; --no-index: one chain plans the whole collection\n"
                        "  --restore-rc: streams of c -m 3 — the reverse-complement pass over the literals is inverted first, on the device, from\n"
                        "  <streamsPrefix>.rcMapOff / .rcMapLen (without it such streams are refused; no effect on other streams)\n"
                        "  --select pattern (repeatable) / --select-list file (a pattern per line): only the files whose line in <streamsPrefix>.names\n"
                        "  contains a pattern, and the contigs they depend on, are decoded; the outputs and --fasta hold the chosen files only\n"
                        "  --closure-out file: a byte per contig of the targets: 0 not filled, 1 filled as a dependency, 2 filled because chosen\n");
        return EXIT_FAILURE;
    }
    if (opt.gzip && opt.fastaDir.empty()) { fprintf(stderr, "mbgc-hip d: --gzip needs --fasta dir (it compresses the FASTA files that --fasta writes)\n"); return EXIT_FAILURE; }
    if (selectAsked) for (const std::string &pat : opt.select) if (pat.empty()) { fprintf(stderr, "mbgc-hip d: --select: an empty pattern\n"); return EXIT_FAILURE; }
    if (selectAsked && opt.select.empty()) { fprintf(stderr, "mbgc-hip d: --select-list: the list of patterns is empty\n"); return EXIT_FAILURE; }
    if (!selectAsked && !opt.closureOut.empty()) { fprintf(stderr, "mbgc-hip d: --closure-out needs a selection (--select / --select-list)\n"); return EXIT_FAILURE; }
    std::string error;
    if (MBGC_Decoder::decode(pos[0], pos[1], opt, &error) != 0) {
        fprintf(stderr, "mbgc-hip d: %s\n", error.c_str());
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

// `mbgc-hip v` (the reference's `mbgc v`, main.cpp:420-445): decode as `d` does, format as `d --fasta` does, compare on the device
int mbgc_hip_validate_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.validate = true;
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--serial") opt.serial = true;
        else if (a == "--no-index") opt.noIndex = true;
        else if (a == "--bench") opt.bench = true;
        else if (a == "--restore-rc") opt.restoreRc = true;
        else if (a == "--flat") opt.flat = true;
        else if (a == "--skip-compare") opt.skipCompare = true;
        else if (a == "--inflate" && i + 1 < argc) {                                            // where gzip originals are inflated
            const std::string w = argv[++i];
            if (w != "host" && w != "device") { fprintf(stderr, "mbgc-hip v: --inflate takes host or device\n"); return EXIT_FAILURE; }
            opt.inflateOnDevice = w == "device";
        }
        else if (a == "--root" && i + 1 < argc) opt.root = argv[++i];
        else if (a == "--dump" && i + 1 < argc) opt.dumpDir = argv[++i];
        else if (a == "--batch-kib" && i + 1 < argc) opt.batchText = (uint64_t) atoll(argv[++i]) << 10;
        else if (a == "--select" && i + 1 < argc) { opt.select.push_back(argv[++i]); selectAsked = true; }
        else if (a == "--select-list" && i + 1 < argc) {
            if (!mbgc_hip_read_pattern_list(argv[++i], opt.select)) { fprintf(stderr, "mbgc-hip v: cannot open the pattern list %s\n", argv[i]); return EXIT_FAILURE; }
            selectAsked = true;
        }
        else if (a == "--gpus") { fprintf(stderr, "mbgc-hip v: validation runs on one GPU (--gpus is an option of mbgc-hip c)\n"); return EXIT_FAILURE; }
        else if (a == "-d" && i + 1 < argc) opt.device = atoi(argv[++i]);
        else pos.push_back(a);
    }
    if (pos.size() != 1) {
        fprintf(stderr, "usage: mbgc-hip v [--serial] [--no-index] [--restore-rc] [--select pattern]... [--select-list file] [--root dir] [--flat]\n"
                        "                  [--skip-compare] [--dump dir] [--bench] [--batch-kib K] [--inflate host|device] [-d device] <streamsPrefix>\n"
                        "  validates the stream set against its FASTA files: every file is decoded and formatted on the device as d --fasta does, its original\n"
                        "  (its line of <streamsPrefix>.names, or that path with .gz; gzip files are inflated where --inflate says) is uploaded beside it and the two are\n"
                        "  compared there. Nothing is downloaded, nothing is written. Exit status 0: every file is valid; 2: a file differs or is missing\n"
                        "  --root dir: put before relative names; --flat: the basename d --fasta writes a file under (d --fasta back; v --flat --root back)\n"
                        "  --serial, --no-index, --restore-rc, --select, --select-list: as in mbgc-hip d (streams of c -m 3 need --restore-rc)\n"
                        "  --skip-compare: decode and format only, no verdict; --dump dir: the decoded text of the first 3 invalid files is written under dir\n"
                        "  --bench: two passes, the second one timed; one JSON line behind the verdict\n"
                        "  --batch-kib K: KiB of text per batch (default 262144; a knob of the tests: several batches on a small collection)\n"
                        "  --inflate device: a gzip original whose trailer states our text's length is uploaded compressed and inflated on the device beside\n"
                        "  its batch, CRC-32 and length checked there; one that does not inflate to that length there is inflated by the host, so the report is\n"
                        "  that of --inflate host (the default: zlib on the read-ahead thread). The one file of a single-FASTA collection inflates on the host\n"
                        "  streams of c -U or c --lossy are compared as they are: originals that were not upper case, or not strict FASTA, differ\n");
        return EXIT_FAILURE;
    }
    if (selectAsked) for (const std::string &pat : opt.select) if (pat.empty()) { fprintf(stderr, "mbgc-hip v: --select: an empty pattern\n"); return EXIT_FAILURE; }
    if (selectAsked && opt.select.empty()) { fprintf(stderr, "mbgc-hip v: --select-list: the list of patterns is empty\n"); return EXIT_FAILURE; }
    std::string error;
    const int r = MBGC_Decoder::decode(pos[0], std::string(), opt, &error);
    if (r == 1) { fprintf(stderr, "mbgc-hip v: %s\n", error.c_str()); return EXIT_FAILURE; }
    return r;
}

// ---------------------------------------------------------------- C exports for tests (host only, no device)
extern "C" {

// scheduleG0 (g0Bytes > 0 or ncontigs == 0) then scheduleTarget for one target; segs: rows of {contig, offset, length, refPos, rc}
int mbgc_decoder_schedule(uint64_t *refPos, uint64_t *reachedRefLengthCount, uint64_t refTotalLength, int lazy, int rcInReference,
                          int contigsIndividuallyReversed, uint64_t refLockPos, uint64_t firstContig, int ncontigs, const uint64_t *length,
                          const uint64_t *unmatched, int factor, int rcFactor, int64_t *segs, uint64_t cap, uint64_t *nsegs) {
    MBGC_Decoder::RefState st;
    st.refPos = *refPos; st.reachedRefLengthCount = *reachedRefLengthCount; st.refTotalLength = refTotalLength; st.lazyDecompressionSupport = lazy != 0;
    std::vector<MBGC_Decoder::ContigInfo> info;
    for (int i = 0; i < ncontigs; i++) info.push_back({length[i], unmatched[i]});
    std::vector<LoadSegment> out;
    if (!MBGC_Decoder::scheduleTarget(st, firstContig, info, (uint8_t) factor, (uint8_t) rcFactor, rcInReference != 0, contigsIndividuallyReversed != 0, refLockPos, out)) return -1;
    *nsegs = out.size();
    if (out.size() > cap) return -2;
    for (size_t i = 0; i < out.size(); i++) {
        const int64_t row[5] = {out[i].contig, (int64_t) out[i].offset, (int64_t) out[i].length, (int64_t) out[i].refPos, out[i].reverseComplement ? 1 : 0};
        memcpy(segs + 5 * i, row, sizeof row);
    }
    *refPos = st.refPos; *reachedRefLengthCount = st.reachedRefLengthCount;
    return 0;
}

// The provenance table over a schedule (segs: rows of {contig, offset, length, refPos, rc} in serial order, as mbgc_decoder_schedule
// writes them; contigs from firstPlanned on are owners, the loader starts at refPos 1 before the first lap), asked as the loader
// stood just before segment nBefore (nsegs: behind them all): the owned pieces of physical range [p0, p1) as rows of
// {physFrom, physTo, owner = contig - firstPlanned}. 0, or -2 (cap too small; *nout = the rows needed).
int mbgc_decoder_provenance(const int64_t *segs, uint64_t nsegs, uint64_t refTotalLength, uint64_t firstPlanned, uint64_t nBefore, uint64_t p0, uint64_t p1,
                            int64_t *out, uint64_t cap, uint64_t *nout) {
    if (refTotalLength < 2 || nBefore > nsegs) return -1;
    Provenance prov;
    prov.L = refTotalLength;
    uint64_t tv = prov.cur;
    for (uint64_t i = 0; i < nsegs; i++) {
        const LoadSegment s = {segs[5 * i], (uint64_t) segs[5 * i + 1], (uint64_t) segs[5 * i + 2], (uint64_t) segs[5 * i + 3], segs[5 * i + 4] != 0};
        if (i == nBefore) tv = prov.cur;
        prov.add(s, firstPlanned);
    }
    if (nBefore == nsegs) tv = prov.cur;
    uint64_t n = 0;
    prov.query(tv, p0, p1, [&](uint64_t a, uint64_t b, int64_t owner) {
        if (n < cap) { out[3 * n] = (int64_t) a; out[3 * n + 1] = (int64_t) b; out[3 * n + 2] = owner; }
        n++;
    });
    *nout = n;
    return n > cap ? -2 : 0;
}

// parse + serialize: 0 and the bytes again, or -1 (malformed; the message in err)
int mbgc_meta_roundtrip(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *nout, char *err, uint64_t errCap) {
    MbgcMeta m;
    std::string e;
    if (!m.parse(std::string((const char *) in, n), &e)) { if (err && errCap) snprintf(err, errCap, "%s", e.c_str()); return -1; }
    const std::string s = m.serialize();
    *nout = s.size();
    if (s.size() > cap) return -2;
    memcpy(out, s.data(), s.size());
    return 0;
}

}  // extern "C"
