#include "mbgc_decoder.h"
#include "simple_sequence_matcher.h"
#include "gzip_inflate.h"
#include "mbgc_checksums.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <fstream>
#include <future>
#include <set>
#include <thread>
#include <tuple>
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

// the stages of decode(), each included once, here, in this order (a later one uses the ones before it):
#include "mbgc_decoder_streams.h"    // what is on disk: StreamSet, Selection, the walk over the chosen units
#include "mbgc_decoder_run.h"        // one pass on the device: DecodedCollection
#include "mbgc_decoder_fasta.h"      // text out of it: FastaLayout, FastaPlan, FastaStage, the writer of d --fasta
#include "mbgc_decoder_region.h"     // d --region: the specs, the pieces, their outputs
#include "mbgc_decoder_validate.h"   // v: Validation
#include "mbgc_decoder_scan.h"       // what the scans of the chosen contigs share: ChosenRecords, FastaHandle, timedCalls, downloadRecord
#include "mbgc_decoder_check.h"      // d --check, t: the chosen contigs against <prefix>.checksums
#include "mbgc_decoder_find.h"       // f: query sequences searched in the chosen contigs
#include "mbgc_decoder_stats.h"      // s: composition, N50 and the runs of N / lower case of the chosen contigs
#include "mbgc_decoder_sketch.h"     // k: k-mer sketches of the chosen files or records and what every two of them share
#include "mbgc_decoder_dups.h"       // u: which chosen contigs are the same sequence, forward or as the reverse complement
#include "mbgc_decoder_screen.h"     // m: which chosen files or records hold the queries' k-mers, and where

namespace {
// what leaves the decoder: the chosen units' contigs; plannedBases: the bases of every target's contigs
struct OutputCount { uint64_t bases = 0, contigs = 0, plannedBases = 0; };
OutputCount countOutput(const DecodedCollection &D, uint64_t g0n, const std::vector<ChosenUnit> &chosen) {
    OutputCount out;
    for (const ChosenUnit &x : chosen) for (uint64_t k = x.c0; k < x.c1; k++) { out.bases += D.contigLen[k]; out.contigs++; }
    for (uint64_t k = g0n; k < D.contigLen.size(); k++) out.plannedBases += D.contigLen[k];
    return out;
}

// ---- `mbgc-hip r`: the units --fasta would write, packed out of the sequence buffer — where the contigs of
// the closure lie among them — into a buffer of the caller's input stage; the collection and all it holds end with decode()'s return
bool handOverResident(const DecodedCollection &D, const StreamSet &S, const Selection &sel, const FastaLayout &layout, const std::vector<ChosenUnit> &chosen,
                      const OutputCount &out, ResidentCollection &R, std::string &msg) {
    R.units.clear();
    std::vector<mbgc_fasta_pack_piece_t> pieces;
    for (const ChosenUnit &c : chosen) {
        ResidentUnit x;
        x.name = layout.names[c.unit];
        x.lineLen = R.lineLenGiven ? R.lineLen : layout.lineLen[c.unit];
        for (uint64_t k = c.c0; k < c.c1; k++) {
            x.headers.append(layout.headers, layout.hdrOff[k], layout.hdrLen[k]); x.headers.push_back('\n');
            x.contigLen.push_back(D.contigLen[k]);
            x.text += recordText(layout.hdrLen[k], D.contigLen[k], x.lineLen);
            pieces.push_back({D.seqOff[k], D.contigLen[k]});
        }
        R.units.push_back(std::move(x));
    }
    if (mbgc_fasta_dev_alloc(R.fasta, out.bases + 64, &R.packedDev)) return faFail(msg, "the chosen units' bases");
    std::vector<uint64_t> dstOff(pieces.size() + 1);
    if (mbgc_fasta_pack_dev(R.fasta, D.seqDev, D.totalBases, pieces.data(), pieces.size(), R.packFlags, R.packedDev, out.bases + 64, dstOff.data(), &R.packKernelMs))
        return faFail(msg, "pack");
    R.packedBytes = dstOff[pieces.size()];
    if (R.packedBytes != out.bases) { msg = "internal error: the packed units are not the chosen contigs"; return false; }
    R.contigsDecoded = S.g0n + (sel.selecting ? D.closureContigs : S.planned); R.contigsChosen = out.contigs;
    R.decodeMs = decodeMs(D, S);
    return true;
}

// <outPrefix>.seq / .contigLens / .seqCounts of the chosen units, and --closure-out
// (--select-seq: a file's runs of chosen records count into its one entry; oneFile: a single-FASTA set, all of them into the one)
bool writeSequenceFiles(const DecodedCollection &D, const std::vector<ChosenUnit> &chosen, const OutputCount &out, const std::string &closureOut,
                        const std::string &outPrefix, bool oneFile, std::string &msg) {
    std::string seq(out.bases, '\0');
    std::vector<uint64_t> outLens;
    uint64_t at = 0;
    for (const Interval &r : mergedRanges(chosen)) {                                            // (a unit's contigs lie back to back in the buffer)
        const uint64_t n = D.seqOff[r.to] - D.seqOff[r.from];
        if (n && swsem_dev_download(D.h, &seq[at], D.seqDev + D.seqOff[r.from], n)) return hipFail(msg, "download");
        at += n;
        outLens.insert(outLens.end(), D.contigLen.begin() + r.from, D.contigLen.begin() + r.to);
    }
    std::vector<uint32_t> counts;
    for (size_t i = 0; i < chosen.size(); i++) {
        if (i && (oneFile || chosen[i].unit == chosen[i - 1].unit)) counts.back() += (uint32_t) (chosen[i].c1 - chosen[i].c0);
        else counts.push_back((uint32_t) (chosen[i].c1 - chosen[i].c0));
    }
    if (!closureOut.empty() && !writeFile(closureOut, D.mark.data(), D.mark.size())) { msg = "cannot write " + closureOut; return false; }
    if (!writeFile(outPrefix + ".seq", seq.data(), seq.size()) ||
        !writeFile(outPrefix + ".contigLens", outLens.data(), outLens.size() * sizeof(uint64_t)) ||
        !writeFile(outPrefix + ".seqCounts", counts.data(), counts.size() * sizeof(uint32_t))) {
        msg = "cannot write " + outPrefix + ".seq / .contigLens / .seqCounts";
        return false;
    }
    return true;
}

// the JSON lines of --bench, from the numbers of the pass it is called behind (the last one)
void reportBench(const MBGC_Decoder::Options &opt, bool wantFasta, const StreamSet &S, const Selection &sel, const DecodedCollection &D, const OutputCount &out,
                 const FastaTimes &ftimes, const ValidateResult &v, const CheckResult &chk) {
    const PassTimes &times = D.times;
    const ValidateTimes &vtimes = v.times;
    const size_t T = S.T();
    // (the restore of -m 3 — upload of the cut literals, plan, fill, download — counts into the decode's time)
    const double ms = times.plan + times.closure + times.fill + times.load + S.rcRestoreMs;
    if (opt.validate && opt.inflateOnDevice)
        printf("{\"inflate_kernel_ms\": %.3f, \"inflated_on_device\": %llu, \"inflated_again_on_host\": %llu}\n", vtimes.inflate, (unsigned long long) vtimes.inflatedOnDevice,
               (unsigned long long) vtimes.inflatedAgainOnHost);
    if (opt.validate) {
        // one line: the comparison, and the headline fields of `d --bench`
        printf("{\"metric\": \"compared GB/s (validate: compare kernel, text and originals in HBM)\", \"value\": %.4f, \"unit\": \"GB/s\", \"compared_bytes\": %llu, "
               "\"compare_kernel_ms\": %.3f, \"upload_ms\": %.3f, \"read_inflate_ms\": %.3f, \"files\": %llu, \"valid\": %llu, \"text_bytes\": %llu, \"batches\": %llu, "
               "\"format_kernel_ms\": %.3f, \"decode_gbases_per_s\": %.4f, \"bases\": %llu, \"plan_ms\": %.3f, \"fill_ms\": %.3f, \"load_ms\": %.3f, \"targets\": %zu, "
               "\"waves\": %llu, \"serial\": %s, \"index\": %s}\n",
               vtimes.compare > 0 ? vtimes.compared / (vtimes.compare * 1e-3) / 1e9 : 0.0, (unsigned long long) vtimes.compared, vtimes.compare, vtimes.upload, vtimes.read,
               (unsigned long long) v.validatedFiles, (unsigned long long) v.validFiles, (unsigned long long) ftimes.text, (unsigned long long) ftimes.batches, ftimes.format,
               out.bases / (ms * 1e-3) / 1e9, (unsigned long long) out.bases, times.plan, times.fill, times.load, T, (unsigned long long) times.waves,
               opt.serial ? "true" : "false", S.useIndex ? "true" : "false");
        return;
    }
    char rcJson[160] = "";
    if (S.meta.rcRedundancyRemoval)
        snprintf(rcJson, sizeof rcJson, ", \"rc_restore_ms\": %.3f, \"rc_marks\": %llu, \"rc_max_chain\": %llu", S.rcRestoreMs,
                 (unsigned long long) S.rcStats.marks, (unsigned long long) S.rcStats.maxChain);
    char selJson[512] = "";
    int selAt = 0;
    if (sel.selecting)
        selAt = snprintf(selJson, sizeof selJson, ", \"closure_ms\": %.3f, \"closure_contigs\": %llu, \"closure_bases\": %llu, \"selected_targets\": %llu, \"dependency_targets\": %llu",
                         times.closure, (unsigned long long) D.closureContigs, (unsigned long long) D.closureBases, (unsigned long long) sel.selectedFiles, (unsigned long long) D.dependencyTargets);
    if (sel.selectingSeq)
        selAt += snprintf(selJson + selAt, sizeof selJson - selAt, ", \"header_match_ms\": %.3f, \"records_chosen\": %llu, \"records\": %llu, \"patterns\": %zu", sel.matchMs,
                          (unsigned long long) sel.recordsChosen, (unsigned long long) sel.recordsAll, opt.selectSeq.size());
    if (sel.selectingRegion)
        selAt += snprintf(selJson + selAt, sizeof selJson - selAt, ", \"header_match_ms\": %.3f, \"regions\": %zu, \"region_bases\": %llu, \"granule_bytes\": %u", sel.matchMs,
                          sel.pieces.size(), (unsigned long long) sel.regionBases, 1u << sel.granuleShift);
    if (sel.selectingSeq && opt.selectSeqHost) selAt += snprintf(selJson + selAt, sizeof selJson - selAt, ", \"header_match_host_ms\": %.3f", sel.matchHostMs);
    if (opt.check)
        snprintf(selJson + selAt, sizeof selJson - selAt, ", \"crc_kernel_ms\": %.3f, \"crc_bytes\": %llu, \"crc_gb_per_s\": %.3f", chk.kernelMs, (unsigned long long) chk.bytes,
                 chk.kernelMs > 0 ? chk.bytes / (chk.kernelMs * 1e-3) / 1e9 : 0.0);
    printf("{\"metric\": \"output Gbases/s (decompress: streams in HBM to sequences in HBM)\", \"value\": %.4f, \"unit\": \"Gbases/s\", \"bases\": %llu, "
           "\"plan_ms\": %.3f, \"fill_ms\": %.3f, \"load_ms\": %.3f, \"targets\": %zu, \"chain_starts\": %zu, \"plan_ms_per_target\": %.4f, \"waves\": %llu, "
           "\"serial\": %s, \"index\": %s%s%s}\n",
           out.bases / (ms * 1e-3) / 1e9, (unsigned long long) out.bases, times.plan, times.fill, times.load, T, S.starts.size(), times.plan / (double) T,
           (unsigned long long) times.waves, opt.serial ? "true" : "false", S.useIndex ? "true" : "false", rcJson, selJson);
    if (wantFasta)
        printf("{\"metric\": \"FASTA text GB/s (format kernel)\", \"value\": %.4f, \"unit\": \"GB/s\", \"text_bytes\": %llu, \"batches\": %llu, "
               "\"format_kernel_ms\": %.3f, \"download_ms\": %.3f, \"write_ms\": %.3f}\n",
               ftimes.format > 0 ? ftimes.text / (ftimes.format * 1e-3) / 1e9 : 0.0, (unsigned long long) ftimes.text, (unsigned long long) ftimes.batches,
               ftimes.format, ftimes.download, ftimes.write);
    if (wantFasta && opt.gzip)
        printf("{\"metric\": \"gzip GB/s of text (deflate kernels)\", \"value\": %.4f, \"unit\": \"GB/s\", \"text_bytes\": %llu, \"gz_bytes\": %llu, "
               "\"deflate_kernel_ms\": %.3f, \"download_ms\": %.3f, \"write_ms\": %.3f, \"chunks\": %llu, \"stored_chunks\": %llu}\n",
               ftimes.deflate > 0 ? ftimes.text / (ftimes.deflate * 1e-3) / 1e9 : 0.0, (unsigned long long) ftimes.text, (unsigned long long) ftimes.gz, ftimes.deflate,
               ftimes.download, ftimes.write, (unsigned long long) ftimes.chunks, (unsigned long long) ftimes.storedChunks);
}

// what `d` and `v` say behind their last pass (`r` says none of it: it returns right after the pack)
void report(const MBGC_Decoder::Options &opt, bool wantFasta, const StreamSet &S, const Selection &sel, const DecodedCollection &D, const OutputCount &out,
            const FastaTimes &ftimes, const ValidateResult &v, const CheckResult &chk) {
    if (opt.bench) reportBench(opt, wantFasta, S, sel, D, out, ftimes, v, chk);
    if (sel.selecting)
        printf("closure: %llu of %llu contigs, %llu of %llu bases, %llu selected, %llu dependency targets\n", (unsigned long long) D.closureContigs, (unsigned long long) S.planned,
               (unsigned long long) D.closureBases, (unsigned long long) out.plannedBases, (unsigned long long) sel.selectedFiles, (unsigned long long) D.dependencyTargets);
    if (sel.selectingSeq)
        printf("records: %llu of %llu chosen in %llu files\n", (unsigned long long) sel.recordsChosen, (unsigned long long) sel.recordsAll, (unsigned long long) sel.selectedFiles);
    if (sel.selectingRegion)
        printf("regions: %zu pieces of %llu records, %llu bases, %llu out of range\n", sel.pieces.size(), (unsigned long long) sel.regionRecords, (unsigned long long) sel.regionBases,
               (unsigned long long) sel.regionSkipped);
    printf("waves: %llu for %zu targets\n", (unsigned long long) D.times.waves, S.T());
    printf("widest wave: %llu targets\n", (unsigned long long) D.times.widest);
    printf("decoded: %llu contigs, %llu bases\n", (unsigned long long) out.contigs, (unsigned long long) out.bases);
    if (opt.check) reportCheck(chk);
}
}  // namespace

// The stages, in the order their failures are reported in. Per pass: decode to the device, then exactly one sink — resident (`r`),
// validate (`v`) or the FASTA files (--fasta) — and/or the sequence files, then the report. `d --check` puts the check between the
// decode and the sinks; `t` is the decode and the check with no sink at all.
int MBGC_Decoder::decode(const std::string &prefix, const std::string &outPrefix, const Options &opt, std::string *error) {
    std::string msg;
    const auto failed = [&msg, error]() { if (error) *error = msg; return 1; };
    // (`v` builds the units and batches of --fasta, and formats them; `r` takes the units)
    const bool wantFasta = !opt.fastaDir.empty() || opt.validate || opt.resident;
    StreamSet S;
    FastaLayout layout;
    Selection sel;
    if (!readStreamFiles(prefix, opt, S, msg) || !restoreRcLiterals(prefix, opt, S, msg) || !checkStreams(S, msg)) return failed();
    mbgc_checksums::Manifest manifest;
    if (opt.check && !readManifest(prefix, S, manifest, msg)) return failed();
    // (--check names a differing contig by its file and header: the whole layout)
    const bool wantLayout = wantFasta || opt.check || opt.find || opt.stats || opt.sketch || opt.dups || opt.screen;      // (`f`, `s`, `k`, `u` and `m` name a record by its file and header)
    if (wantLayout && !readFastaLayout(prefix, S.meta, S.g0n + S.planned, layout, msg)) return failed();
    if (!wantLayout && (!opt.selectSeq.empty() || !opt.regions.empty()) && !readHeaders(prefix, S.g0n + S.planned, layout, msg)) return failed();
    if (!chainStarts(opt.noIndex, S, msg)) return failed();
    // --select: with a layout its names are used, without one (plain `d`) .names is read for it; --select-seq: the records of the
    // files that passed, by their headers, on the device
    if (!chooseUnits(prefix, S, opt.select, wantFasta ? &layout.names : nullptr, sel, msg) || !chooseRecords(prefix, S, opt, layout, sel, msg) ||
        !chooseRegions(prefix, S, opt, layout, sel, msg)) return failed();
    const std::vector<ChosenUnit> chosen = chosenUnits(S.g0n, S.seqCount.data(), S.T(), sel.unitSel.data(), sel.selectingSeq ? sel.contigSel.data() : nullptr,
                                                      S.meta.sequentialMatching);
    // --bench: two passes, a fresh handle for each; the second one is the timed one, and the only one `v` and the report speak of
    const int passes = opt.bench ? 2 : 1;
    int status = 0;
    for (int pass = 0; pass < passes; pass++) {
        const bool last = pass + 1 == passes;
        DecodedCollection D;
        if (!D.upload(S, opt.device, msg) || !D.planAndSchedule(S, opt.serial, msg)) return failed();
        if (sel.selectingRegion) resolveRegions(D.contigLen, S.meta.singleFastaFile, sel);       // (the plan has said how long every record is)
        if (!D.closure(S, sel, msg) || !D.forwardRun(S, sel.selecting, msg)) return failed();
        OutputCount out = countOutput(D, S.g0n, chosen);
        // --region: what leaves the decoder is the pieces, not the chosen records they are cut from
        const RegionOutput pieces = sel.selectingRegion ? regionOutput(D, sel, layout, wantFasta) : RegionOutput();
        if (sel.selectingRegion) { out.bases = sel.regionBases; out.contigs = sel.pieces.size(); }
        // `r` ends here: no report, no sequence files
        if (opt.resident) return handOverResident(D, S, sel, layout, chosen, out, *opt.resident, msg) ? 0 : failed();
        FastaTimes ftimes;
        ValidateResult vres;
        CheckResult chk;
        if (opt.check && last && !checkChecksums(prefix, D, S, layout, chosen, manifest, opt.device, chk, msg)) return failed();
        // `f`, `s`, `k`, `u`: the scan of the chosen contigs is the sink — its lines and its summary; `f` returns 3 when nothing was found
        // `m`: the same, its own result and exit status — 3 when no (query, group) pair was reported
        if (opt.screen) {
            if (!last) continue;
            ScreenResult screen;
            uint64_t pairs = 0;
            if (!collectScreen(D, S, chosen, layout, opt, opt.bench, screen, msg) || !reportScreen(opt, layout, screen, decodeMs(D, S), pairs, msg)) return failed();
            return pairs ? 0 : 3;
        }
        if (opt.find || opt.stats || opt.sketch || opt.dups) {
            if (!last) continue;
            FindResult found;
            StatsResult stats;
            SketchResult sketch;
            DupsResult dups;
            const bool ok = opt.find    ? findQueries(D, S, layout, chosen, opt, opt.bench, found, msg) && reportFind(opt, layout, found, decodeMs(D, S), msg)
                          : opt.stats   ? collectStats(D, S, chosen, opt, opt.bench, stats, msg) && reportStats(opt, layout, stats, decodeMs(D, S), msg)
                          : opt.sketch  ? collectSketch(D, S, chosen, layout, opt, opt.bench, sketch, msg) && reportSketch(opt, sketch, decodeMs(D, S), msg)
                                        : collectDups(D, S, chosen, opt, opt.bench, dups, msg) && reportDups(opt, layout, dups, decodeMs(D, S), msg);
            if (!ok) return failed();
            return opt.find && (opt.findPrimers.empty() ? found.lines.empty() : found.amplicons.empty()) ? 3 : 0;
        }
        if (wantFasta) {
            const FastaPlan plan = sel.selectingRegion ? planFasta(pieces.rows, S.meta, pieces.layout, pieces.len, opt.batchText, opt.gzip, true)
                                                       : planFasta(chosen, S.meta, layout, D.contigLen, opt.batchText, opt.gzip, sel.selectingSeq);
            const FastaLayout &text = sel.selectingRegion ? pieces.layout : layout;              // (the pieces carry headers of their own)
            const bool writeFiles = !opt.validate && (!opt.bench || pass == 0);                  // (bench: pass 0 writes, the timed pass formats and downloads only)
            if (std::string dir; writeFiles && !makeDirs(opt.fastaDir, &dir)) { msg = "cannot create the directory " + dir; return failed(); }
            FastaStage stage;                                                                    // (behind D: it ends before the collection it reads)
            if (sel.selectingRegion) { stage.recOff = &pieces.off; stage.recLen = &pieces.len; }
            if (!stage.open(D, plan, text, opt.device, opt.gzip, msg)) return failed();
            if (opt.validate) {
                Validation v(D, plan, stage, layout, S.meta, opt, last);
                if (!v.run(msg)) return failed();
                vres = v.res;
            } else if (!writeFastaFiles(plan, stage, text, opt, writeFiles, msg)) return failed();
            ftimes = stage.times;
        }
        // the sequence files and --closure-out: on the last pass, and only without --bench and without `v`
        const bool writeSeq = last && !opt.bench && !opt.validate && !opt.writeNothing;
        if (writeSeq && sel.selectingRegion && !writeRegionFiles(D, pieces, out.bases, opt.device, opt.closureOut, outPrefix, S.meta.singleFastaFile, msg)) return failed();
        if (writeSeq && !sel.selectingRegion && !writeSequenceFiles(D, chosen, out, opt.closureOut, outPrefix, sel.selectingSeq && S.meta.singleFastaFile, msg)) return failed();
        if (last) {
            report(opt, wantFasta, S, sel, D, out, ftimes, vres, chk);
            status = (opt.validate && vres.invalidFiles) || (opt.check && chk.differs()) ? 2 : 0;
        }
    }
    return status;
}

// ---------------------------------------------------------------- the command lines
bool mbgc_hip_read_pattern_list(const char *path, std::vector<std::string> &out) {
    std::ifstream f(path);
    if (!f) return false;
    for (std::string line; std::getline(f, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty()) out.push_back(line);
    }
    return true;
}

int mbgc_hip_decode_option(char tool, int argc, char **argv, int &i, MBGC_Decoder::Options &opt, bool &selectAsked) {
    const std::string a = argv[i];
    if (a == "--serial") opt.serial = true;
    else if (a == "--no-index") opt.noIndex = true;
    else if (a == "--restore-rc") opt.restoreRc = true;
    else if (a == "--select" && i + 1 < argc) { opt.select.push_back(argv[++i]); selectAsked = true; }
    else if (a == "--select-list" && i + 1 < argc) {
        if (!mbgc_hip_read_pattern_list(argv[++i], opt.select)) { fprintf(stderr, "mbgc-hip %c: cannot open the pattern list %s\n", tool, argv[i]); return -1; }
        selectAsked = true;
    }
    else if (a == "--select-seq" && i + 1 < argc) { opt.selectSeq.push_back(argv[++i]); opt.selectSeqAsked = true; }
    else if (a == "--select-seq-list" && i + 1 < argc) {
        if (!mbgc_hip_read_pattern_list(argv[++i], opt.selectSeq)) { fprintf(stderr, "mbgc-hip %c: cannot open the pattern list %s\n", tool, argv[i]); return -1; }
        opt.selectSeqAsked = true;
    }
    else if (a == "--region" && i + 1 < argc) {
        MBGC_Decoder::RegionSpec spec;
        std::string why;
        if (!MBGC_Decoder::parseRegionSpec(argv[++i], spec, &why)) { fprintf(stderr, "mbgc-hip %c: --region '%s': %s\n", tool, argv[i], why.c_str()); return -1; }
        opt.regions.push_back(spec); opt.regionAsked = true;
    }
    else if (a == "--region-list" && i + 1 < argc) {
        std::vector<std::string> lines;
        if (!mbgc_hip_read_pattern_list(argv[++i], lines)) { fprintf(stderr, "mbgc-hip %c: cannot open the region list %s\n", tool, argv[i]); return -1; }
        for (const std::string &line : lines) {
            MBGC_Decoder::RegionSpec spec;
            std::string why;
            if (!MBGC_Decoder::parseRegionSpec(line, spec, &why)) { fprintf(stderr, "mbgc-hip %c: --region-list: '%s': %s\n", tool, line.c_str(), why.c_str()); return -1; }
            opt.regions.push_back(spec);
        }
        opt.regionAsked = true;
    }
    else if (a == "-d" && i + 1 < argc) opt.device = atoi(argv[++i]);
    else return 0;
    return 1;
}

// a decimal number of 1 to 18 digits and nothing else (it fits 64 bits) — the one parser of the command lines' counts
static bool parseDecimal(const std::string &text, uint64_t &v) {
    if (text.empty() || text.size() > 18 || text.find_first_not_of("0123456789") != std::string::npos) return false;
    v = strtoull(text.c_str(), nullptr, 10);
    return true;
}

// ... as the value of option `name` of `mbgc-hip <tool>`, which "takes <takes>" when it is none
static bool numberOption(char tool, const char *name, const char *takes, const char *text, uint64_t &v) {
    if (parseDecimal(text, v)) return true;
    fprintf(stderr, "mbgc-hip %c: %s takes %s\n", tool, name, takes);
    return false;
}

bool MBGC_Decoder::parseRegionSpec(const std::string &text, RegionSpec &out, std::string *why) {
    const auto bad = [why](const char *what) { if (why) *why = what; return false; };
    const size_t colon = text.rfind(':');
    if (colon == std::string::npos) return bad("a region is PATTERN:FROM-TO (no ':')");
    if (colon == 0) return bad("an empty pattern");
    out.pattern = text.substr(0, colon);
    if (out.pattern.find('\n') != std::string::npos) return bad("the pattern holds a line feed, a header holds none");
    const std::string range = text.substr(colon + 1);
    const size_t dash = range.find('-');
    if (dash == std::string::npos) return bad("a region is PATTERN:FROM-TO (no '-' behind the last ':')");
    uint64_t v[2];
    const std::string part[2] = {range.substr(0, dash), range.substr(dash + 1)};
    for (int k = 0; k < 2; k++)
        if (!parseDecimal(part[k], v[k])) return bad("FROM and TO are positive decimal numbers");
    if (v[0] < 1) return bad("FROM is 1-based: the first base is 1");
    if (v[0] > v[1]) return bad("FROM lies behind TO");
    out.from = v[0]; out.to = v[1];
    return true;
}

bool mbgc_hip_check_selection(char tool, const MBGC_Decoder::Options &opt, bool selectAsked) {
    if (selectAsked) for (const std::string &pat : opt.select) if (pat.empty()) { fprintf(stderr, "mbgc-hip %c: --select: an empty pattern\n", tool); return false; }
    if (selectAsked && opt.select.empty()) { fprintf(stderr, "mbgc-hip %c: --select-list: the list of patterns is empty\n", tool); return false; }
    for (const std::string &pat : opt.selectSeq) {
        if (pat.empty()) { fprintf(stderr, "mbgc-hip %c: --select-seq: an empty pattern\n", tool); return false; }
        if (pat.find('\n') != std::string::npos) { fprintf(stderr, "mbgc-hip %c: --select-seq: a pattern holds a line feed, a header holds none\n", tool); return false; }
    }
    if (opt.selectSeqAsked && opt.selectSeq.empty()) { fprintf(stderr, "mbgc-hip %c: --select-seq-list: the list of patterns is empty\n", tool); return false; }
    if (opt.regionAsked && opt.regions.empty()) { fprintf(stderr, "mbgc-hip %c: --region-list: the list of regions is empty\n", tool); return false; }
    if (opt.regionAsked && opt.selectSeqAsked) {
        fprintf(stderr, "mbgc-hip %c: --region and --select-seq / --select-seq-list in one run: a region names its records itself (PATTERN:FROM-TO)\n", tool);
        return false;
    }
    if (opt.regionAsked && opt.check) {
        fprintf(stderr, "mbgc-hip %c: --region with --check: <streamsPrefix>.checksums holds the CRC-32 of whole contigs, a part of one has none to be held against\n", tool);
        return false;
    }
    return true;
}

const char *const MBGC_HIP_D_USAGE =
    "mbgc-hip d [--serial] [--no-index] [--bench] [--restore-rc] [--fasta dir [--gzip] [--batch-kib K]] [--select pattern]...\n"
    "                  [--select-list file] [--select-seq pattern]... [--select-seq-list file] [--region 'pattern:from-to']...\n"
    "                  [--region-list file] [--closure-out file] [--check] [-d device]\n"
    "                  <streamsPrefix> <outputPrefix>\n"
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
    "  --select-seq pattern (repeatable) / --select-seq-list file (a pattern per line): only the records whose header line (without the\n"
    "  '>') contains a pattern — a plain substring, case-sensitive, matched on the device against <streamsPrefix>.headers — and the contigs\n"
    "  they depend on are decoded; with --select a record's file must pass that too. A file holds its chosen records in order, a file\n"
    "  without one is not written, .seqCounts counts the chosen records per written file; -i streams: the one file, one count\n"
    "  --region 'pattern:from-to' (repeatable) / --region-list file (a spec per line): only bases from..to (1-based, inclusive) of the records\n"
    "  whose header line contains the pattern (as --select-seq; the spec is split at its last ':') are written, and only what they depend on\n"
    "  is decoded — at the grain of granules of 256 bytes, not of contigs. to is clamped to the record's length; a region that starts behind the\n"
    "  record's end yields nothing and is counted. The pieces are written in collection order, by record, from, to (identical ones once):\n"
    "  .seq holds them back to back, .contigLens their lengths, .seqCounts the pieces per written file; --fasta writes a record per piece,\n"
    "  its header the record's with :from-to behind the first word. Prints `regions: <pieces> pieces of <records> records, <bases> bases,\n"
    "  <skipped> out of range`; the closure: line counts the bases actually filled. With --select a record's file must pass that too.\n"
    "  Not with --select-seq or --check. --bench gains regions, region_bases, granule_bytes\n"
    "  --closure-out file: a byte per contig of the targets: 0 not filled, 1 filled as a dependency, 2 filled because chosen\n"
    "  --check: before anything is written, the CRC-32 of every chosen contig's bases is taken on the device and held against\n"
    "  <streamsPrefix>.checksums (mbgc-hip c --checksums), the side files' on the host; prints `checksums: <checked> of <N> contigs checked,\n"
    "  <bad> differ` and a `checksum ERROR` line per differing contig (the first 100) or side file. Exit status 2 when anything differs —\n"
    "  the outputs are written all the same —, 1 when the manifest is missing or does not fit the set. --bench gains crc_kernel_ms,\n"
    "  crc_bytes, crc_gb_per_s\n";

const char *const MBGC_HIP_T_USAGE =
    "mbgc-hip t [--serial] [--no-index] [--restore-rc] [--select pattern]... [--select-list file] [--select-seq pattern]...\n"
    "                  [--select-seq-list file] [--bench] [-d device] <streamsPrefix>\n"
    "  tests the stream set against <streamsPrefix>.checksums without the FASTA files: d --check that writes nothing. Exit status 0: every\n"
    "  chosen contig and the side files are as mbgc-hip c --checksums (or r --checksums) saw them; 2: something differs; 1: malformed streams,\n"
    "  no manifest, or one that does not fit the set\n";

const char *const MBGC_HIP_V_USAGE =
    "mbgc-hip v [--serial] [--no-index] [--restore-rc] [--select pattern]... [--select-list file] [--root dir] [--flat]\n"
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
    "  streams of c -U or c --lossy are compared as they are: originals that were not upper case, or not strict FASTA, differ\n";

// the tail of every command that decodes: the decode, its error line, its status (1: the error; what else the command returns)
static int decodeAndReport(char tool, const std::string &prefix, const std::string &outPrefix, const MBGC_Decoder::Options &opt) {
    std::string error;
    const int r = MBGC_Decoder::decode(prefix, outPrefix, opt, &error);
    if (r == 1) { fprintf(stderr, "mbgc-hip %c: %s\n", tool, error.c_str()); return EXIT_FAILURE; }
    return r;
}

int mbgc_hip_decompress_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (const int r = mbgc_hip_decode_option('d', argc, argv, i, opt, selectAsked)) { if (r < 0) return EXIT_FAILURE; }
        else if (a == "--bench") opt.bench = true;
        else if (a == "--fasta" && i + 1 < argc) opt.fastaDir = argv[++i];
        else if (a == "--gzip") opt.gzip = true;
        else if (a == "--batch-kib" && i + 1 < argc) opt.batchText = (uint64_t) atoll(argv[++i]) << 10;
        else if (a == "--closure-out" && i + 1 < argc) opt.closureOut = argv[++i];
        else if (a == "--check") opt.check = true;
        else if (a == "--region-granule" && i + 1 < argc) {                                     // (a knob of the measurements: bytes per granule of the closure)
            const long long g = atoll(argv[++i]);
            if (g < 16 || g > (1ll << 30) || (g & (g - 1))) { fprintf(stderr, "mbgc-hip d: --region-granule takes a power of two from 16 to 1073741824\n"); return EXIT_FAILURE; }
            opt.regionGranule = (uint32_t) g;
        }
        else if (a == "--select-seq-host") opt.selectSeqHost = true;                           // (a developer switch: the host's loop beside the kernel, timed and compared)
        else pos.push_back(a);
    }
    if (pos.size() != 2) { fprintf(stderr, "usage: %s", MBGC_HIP_D_USAGE); return EXIT_FAILURE; }
    if (opt.gzip && opt.fastaDir.empty()) { fprintf(stderr, "mbgc-hip d: --gzip needs --fasta dir (it compresses the FASTA files that --fasta writes)\n"); return EXIT_FAILURE; }
    if (!mbgc_hip_check_selection('d', opt, selectAsked)) return EXIT_FAILURE;
    if (!selectAsked && !opt.selectSeqAsked && !opt.regionAsked && !opt.closureOut.empty()) { fprintf(stderr, "mbgc-hip d: --closure-out needs a selection (--select / --select-list)\n"); return EXIT_FAILURE; }
    return decodeAndReport('d', pos[0], pos[1], opt);                                           // (2: --check found a difference)
}

// `mbgc-hip t`: the stages of `d --check` without a sink
int mbgc_hip_test_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.check = opt.writeNothing = true;
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (const int r = mbgc_hip_decode_option('t', argc, argv, i, opt, selectAsked)) { if (r < 0) return EXIT_FAILURE; }
        else if (a == "--bench") opt.bench = true;
        else pos.push_back(a);
    }
    if (pos.size() != 1 || pos[0].compare(0, 1, "-") == 0) { fprintf(stderr, "usage: %s", MBGC_HIP_T_USAGE); return EXIT_FAILURE; }
    if (opt.regionAsked) {
        fprintf(stderr, "mbgc-hip t: --region / --region-list select parts of records, and the manifest holds the CRC-32 of whole contigs (an option of mbgc-hip d)\n");
        return EXIT_FAILURE;
    }
    if (!mbgc_hip_check_selection('t', opt, selectAsked)) return EXIT_FAILURE;
    return decodeAndReport('t', pos[0], std::string(), opt);
}

// The command line of `f`, `s`, `k` and `u`: the decoder's options and --bench, the command's own (own(a, i): 1 taken, 0 not its, -1
// refused with its line printed), what these commands refuse before anything is decoded, the one positional. settled(): 0, 1 for a
// refusal whose line it printed, 2 for the usage text — asked behind the --region refusal and in front of the positional. -> the exit
// status, or -1 with the stream set's prefix when the command can go on
struct ScanTool { char letter; const char *usage, *regionWhy, *fastaWhy; };      // fastaWhy == nullptr: --fasta is no option of the tool's at all
template <class Own, class Settled>
static int scanCommandLine(const ScanTool &tool, int argc, char **argv, MBGC_Decoder::Options &opt, Own own, Settled settled, std::string &prefix) {
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (const int r = mbgc_hip_decode_option(tool.letter, argc, argv, i, opt, selectAsked)) { if (r < 0) return EXIT_FAILURE; }
        else if (a == "--bench") opt.bench = true;
        else if (const int r = own(a, i)) { if (r < 0) return EXIT_FAILURE; }
        else if (a == "--check") { fprintf(stderr, "mbgc-hip %c: --check is an option of mbgc-hip d (mbgc-hip t tests a set against its manifest)\n", tool.letter); return EXIT_FAILURE; }
        else if (a == "--fasta" && tool.fastaWhy) { fprintf(stderr, "mbgc-hip %c: --fasta is an option of mbgc-hip d: %s\n", tool.letter, tool.fastaWhy); return EXIT_FAILURE; }
        else pos.push_back(a);
    }
    if (opt.regionAsked) {
        fprintf(stderr, "mbgc-hip %c: --region / --region-list select parts of records, and %s\n", tool.letter, tool.regionWhy);
        return EXIT_FAILURE;
    }
    const int s = settled();
    if (s == 1) return EXIT_FAILURE;
    if (s == 2 || pos.size() != 1 || pos[0].compare(0, 1, "-") == 0) { fprintf(stderr, "usage: %s", tool.usage); return EXIT_FAILURE; }
    if (!mbgc_hip_check_selection(tool.letter, opt, selectAsked)) return EXIT_FAILURE;
    prefix = pos[0];
    return -1;
}

const char *const MBGC_HIP_F_USAGE =
    "mbgc-hip f [--seq ACGT...]... [--seq-file queries.fa] [--mismatches K] [--forward-only] [--hits file] [--regions-out file [--flank N]]\n"
    "                  [--hit-capacity N] [--find-host] [--serial] [--no-index] [--restore-rc] [--select pattern]... [--select-list file]\n"
    "                  [--select-seq pattern]... [--select-seq-list file] [-d device] [--bench] <streamsPrefix>\n"
    "  finds query sequences in the collection without unpacking it: the chosen contigs are decoded as mbgc-hip d decodes them (--serial,\n"
    "  --no-index, --restore-rc, --select, --select-list, --select-seq, --select-seq-list: as there; contigs decoded only as dependencies are\n"
    "  not searched) and scanned where they lie, on the device; no sequence file is written. --seq: a query, named q1, q2, ... in command-line\n"
    "  order; --seq-file: a FASTA file of queries, each named by the first word of its header. Letters only, compared without case; with\n"
    "  --mismatches K (0..3, substitutions only) a query holds 8 (K + 1) to 65535 bases. The reverse complement of every query is searched\n"
    "  too (--forward-only: not); a query that is its own reverse complement is reported once, as +\n"
    "  One line per hit on stdout (--hits file: there): query, file (its line of <streamsPrefix>.names), record (the first word of its header),\n"
    "  start, end (1-based, inclusive, forward-strand coordinates also for a - hit), strand, mismatches, tab-separated; sorted by file, record,\n"
    "  start, query, + before -. Then `hits: <n> in <records> records of <files> files; <bases> bases searched, <patterns> patterns` (the\n"
    "  records and files that hold a hit). Exit status 0: at least one hit; 3: none; 1: malformed streams or a refused option\n"
    "  --regions-out file [--flank N]: a line RECORD:FROM-TO per hit, FROM = max(1, start - N), TO = end + N, identical lines once; mbgc-hip d\n"
    "  --region-list file then fetches those pieces (d clamps TO). d matches RECORD as a SUBSTRING of the header line: a record whose first\n"
    "  word is part of another record's header brings that one's piece along\n"
    "  --hit-capacity N: the first size of the hit buffer (a knob of the tests; the search is made again with the size it needs). --find-host:\n"
    "  a developer switch, the chosen contigs are downloaded and searched by a plain loop on the host, timed, and the two results must agree\n"
    "  --bench: two decodes, the second one timed, the search run six times (the median of the last five); one JSON line (find_kernel_ms,\n"
    "  bases_searched, patterns, hits, retries, decode_ms, find_gb_per_s; --find-host: find_host_ms). Not with --region or --check\n";

// what --iupac and --primers add to `f`; printed behind MBGC_HIP_F_USAGE by the general help and when one of their options stands on a
// command line that is answered with the usage text (MBGC_HIP_F_USAGE itself is what `f` printed before these options came)
const char *const MBGC_HIP_F_IUPAC_USAGE =
    "mbgc-hip f --iupac ... | f --primers NAME:FWD:REV... [--primer-file file] [--min-amplicon N] [--max-amplicon N] [--amplicons-out file] ...\n"
    "  --iupac: the queries are IUPAC patterns, a letter stands for a set of bases: A, C, G, T (or U); R = AG, Y = CT, S = CG, W = AT, K = GT,\n"
    "  M = AC; B = CGT, D = AGT, H = ACT, V = ACG; N = ACGT. A query with any other letter is refused. A text byte has a base only if it is one of\n"
    "  acgtuACGTU (u is T); a position matches if the text's base is in the query letter's set. So an N or an ambiguity letter IN THE TEXT is a\n"
    "  mismatch against everything, a query N included — unlike f without --iupac, which compares letters literally (there an N matches an N and\n"
    "  an R only an R). The reverse complement is the IUPAC one (A-T, C-G, R-Y, K-M, B-V, D-H; S, W, N are their own). --mismatches and its length\n"
    "  rule, the lines, the summary, the exit statuses and every other option of f stay as they are; --bench adds rows (of the seed table) and\n"
    "  rows_walked. Every one of the K + 1 equal parts of a query needs 8 letters in a row that stand for at most 256 sequences together (ACNNNNGT\n"
    "  does, ACNNNNNT does not): a query with a part that has no such 8 letters is refused, by name and part\n"
    "  --primers NAME:FWD:REV (repeatable; --primer-file file: a line name<TAB>fwd<TAB>rev per pair): in-silico PCR. Implies --iupac; both primers\n"
    "  are written 5'->3' and are subject to --mismatches K and its length rule, 8 (K + 1) letters: a 20-mer allows K <= 1, a 24-mer K <= 3. A +\n"
    "  product is a + hit of FWD at [s1, e1] and a - hit of REV at [s2, e2] of one record with s1 <= s2, e1 <= e2 and --min-amplicon (default 0)\n"
    "  <= e2 - s1 + 1 <= --max-amplicon (default 5000); a - product the same with REV + on the left and FWD - on the right. Every such pair of\n"
    "  hits is a product, not only the nearest; FWD-FWD and REV-REV are none. Records are linear: a product across the origin of a circular\n"
    "  genome is not found. One line per product on stdout: pair, file, record, start, end (1-based, inclusive, primers included), strand, length,\n"
    "  mismatches of the left primer, mismatches of the right primer, tab-separated; sorted by file, record, start, end, pair, + before -. Then\n"
    "  `amplicons: <n> of <pairs> primer pairs in <records> records of <files> files; <bases> bases searched` (n products; the pairs given; the\n"
    "  records and files that hold a product). The primers' own hits (queries NAME.fwd, NAME.rev) are printed only with --hits file.\n"
    "  --amplicons-out file: a line RECORD:START-END per product, identical lines once, for mbgc-hip d --region-list. Exit status 0: at least\n"
    "  one product; 3: none; 1: a refusal. Not with --seq, --seq-file or --forward-only\n";

// --seq-file: the records of a FASTA file as queries — the header's first word, the sequence lines joined
static bool readQueryFile(const char *path, std::vector<MBGC_Decoder::FindQuery> &out) {
    std::ifstream f(path);
    if (!f) return false;
    for (std::string line; std::getline(f, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') { const std::string h = line.substr(1); out.push_back({h.substr(0, h.find_first_of(" \t")), std::string()}); }
        else if (!line.empty() && !out.empty()) out.back().seq += line;
        else if (!line.empty()) out.push_back({"?", line});             // (bases in front of the first header: refused below, by this name)
    }
    return true;
}

// `mbgc-hip f`: the decode of `t` — nothing is written —, then the search in place of the check
int mbgc_hip_find_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.find = opt.writeNothing = true;
    int inlineQueries = 0;
    std::string prefix;
    // The usage text grows by the new options' part only when one of them stands on the command line as a word of its own: without
    // them `f` answers a malformed command line with the text it always printed, byte for byte (tests/golden/scan_cli_refusals.json
    // holds it). This look at argv chooses that text and nothing else — the options themselves are read by the one parser below, which
    // knows no --option=value form either, so the two cannot disagree on what was given; a later change may extend the one text and
    // its recorded copy and drop this.
    static const char *const newOptions[] = {"--iupac", "--primers", "--primer-file", "--min-amplicon", "--max-amplicon", "--amplicons-out"};
    bool newAsked = false, plainQueries = false, ampliconOptions = false;
    for (int i = 2; i < argc; i++) for (const char *o : newOptions) newAsked |= !strcmp(argv[i], o);
    const std::string usage = std::string(MBGC_HIP_F_USAGE) + (newAsked ? MBGC_HIP_F_IUPAC_USAGE : "");
    const auto addPair = [&](const std::string &name, const std::string &fwd, const std::string &rev) {
        opt.findPrimers.push_back({name, fwd, rev});
        opt.findQueries.push_back({name + ".fwd", fwd}); opt.findQueries.push_back({name + ".rev", rev});
    };
    const ScanTool tool = {'f', usage.c_str(), "a search looks at whole records (an option of mbgc-hip d; f --regions-out writes such a list)", nullptr};
    const int r = scanCommandLine(tool, argc, argv, opt, [&](const std::string &a, int &i) {
        if (a == "--seq" && i + 1 < argc) { opt.findQueries.push_back({"q" + std::to_string(++inlineQueries), argv[++i]}); plainQueries = true; }
        else if (a == "--seq-file" && i + 1 < argc) {
            if (!readQueryFile(argv[++i], opt.findQueries)) { fprintf(stderr, "mbgc-hip f: cannot open the query file %s\n", argv[i]); return -1; }
            plainQueries = true;
        }
        else if (a == "--iupac") opt.findIupac = true;
        else if (a == "--primers" && i + 1 < argc) {
            const std::string spec = argv[++i];
            const size_t c1 = spec.find(':'), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
            if (c2 == std::string::npos || spec.find(':', c2 + 1) != std::string::npos || c1 == 0 || c2 == c1 + 1 || c2 + 1 == spec.size()) {
                fprintf(stderr, "mbgc-hip f: --primers takes NAME:FWD:REV, three parts that are not empty (got %s)\n", spec.c_str());
                return -1;
            }
            addPair(spec.substr(0, c1), spec.substr(c1 + 1, c2 - c1 - 1), spec.substr(c2 + 1));
        }
        else if (a == "--primer-file" && i + 1 < argc) {
            std::ifstream f(argv[++i]);
            if (!f) { fprintf(stderr, "mbgc-hip f: cannot open the primer file %s\n", argv[i]); return -1; }
            size_t n = 0;
            for (std::string line; std::getline(f, line);) {
                n++;
                if (!line.empty() && line.back() == '\r') line.pop_back();
                if (line.empty()) continue;
                const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
                if (t2 == std::string::npos || line.find('\t', t2 + 1) != std::string::npos || t1 == 0 || t2 == t1 + 1 || t2 + 1 == line.size()) {
                    fprintf(stderr, "mbgc-hip f: --primer-file %s, line %zu: a line is name<TAB>fwd<TAB>rev, three parts that are not empty\n", argv[i], n);
                    return -1;
                }
                addPair(line.substr(0, t1), line.substr(t1 + 1, t2 - t1 - 1), line.substr(t2 + 1));
            }
        }
        else if (a == "--min-amplicon" && i + 1 < argc) { ampliconOptions = true; if (!numberOption('f', "--min-amplicon", "a number of bases", argv[++i], opt.findMinAmplicon)) return -1; }
        else if (a == "--max-amplicon" && i + 1 < argc) { ampliconOptions = true; if (!numberOption('f', "--max-amplicon", "a number of bases", argv[++i], opt.findMaxAmplicon)) return -1; }
        else if (a == "--amplicons-out" && i + 1 < argc) { ampliconOptions = true; opt.findAmpliconsOut = argv[++i]; }
        else if (a == "--mismatches" && i + 1 < argc) {
            const std::string v = argv[++i];
            if (v.size() != 1 || v[0] < '0' || v[0] > '3') { fprintf(stderr, "mbgc-hip f: --mismatches takes 0, 1, 2 or 3\n"); return -1; }
            opt.findMismatches = (uint32_t) (v[0] - '0');
        }
        else if (a == "--forward-only") opt.findForwardOnly = true;
        else if (a == "--hits" && i + 1 < argc) opt.findHitsFile = argv[++i];
        else if (a == "--regions-out" && i + 1 < argc) opt.findRegionsOut = argv[++i];
        else if (a == "--flank" && i + 1 < argc) opt.findFlank = strtoull(argv[++i], nullptr, 10);
        else if (a == "--hit-capacity" && i + 1 < argc) {
            opt.findHitCapacity = strtoull(argv[++i], nullptr, 10);
            if (!opt.findHitCapacity) { fprintf(stderr, "mbgc-hip f: --hit-capacity takes a positive number of hits\n"); return -1; }
        }
        else if (a == "--find-host") opt.findHost = true;
        else return 0;
        return 1;
    }, [&] {
        if (opt.findQueries.empty()) return 2;
        if (!opt.findPrimers.empty() && plainQueries) { fprintf(stderr, "mbgc-hip f: --primers / --primer-file and --seq / --seq-file: the primers are the queries of that search\n"); return 1; }
        if (!opt.findPrimers.empty() && opt.findForwardOnly) { fprintf(stderr, "mbgc-hip f: --primers and --forward-only: a product has a primer on either strand\n"); return 1; }
        if (opt.findPrimers.empty() && ampliconOptions) { fprintf(stderr, "mbgc-hip f: --min-amplicon, --max-amplicon and --amplicons-out go with --primers / --primer-file\n"); return 1; }
        if (opt.findMaxAmplicon < opt.findMinAmplicon) {
            fprintf(stderr, "mbgc-hip f: --max-amplicon %llu is below --min-amplicon %llu\n", (unsigned long long) opt.findMaxAmplicon, (unsigned long long) opt.findMinAmplicon);
            return 1;
        }
        return 0;
    }, prefix);
    if (r >= 0) return r;
    if (!opt.findPrimers.empty()) opt.findIupac = true;
    // the queries, held to the search's limits before anything is decoded
    const uint64_t shortest = 8ull * (opt.findMismatches + 1);
    const char *const what = opt.findPrimers.empty() ? "query" : "primer";
    for (MBGC_Decoder::FindQuery &q : opt.findQueries) {
        if (opt.findIupac) {
            // the letter table of --iupac; U is written as T from here on (the same set), so that a query equals its own reverse complement as text
            for (char &c : q.seq) {
                const char u = (char) (c & 0xDF);
                if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) || !strchr("ACGTURYSWKMBDHVN", u)) {
                    if (c > 32 && c < 127) fprintf(stderr, "mbgc-hip f: %s %s holds '%c', which is no IUPAC letter (ACGTU, RYSWKM, BDHV, N)\n", what, q.name.c_str(), c);
                    else fprintf(stderr, "mbgc-hip f: %s %s holds the byte 0x%02x, which is no IUPAC letter (ACGTU, RYSWKM, BDHV, N)\n", what, q.name.c_str(), (unsigned) (uint8_t) c);
                    return EXIT_FAILURE;
                }
                c = u == 'U' ? 'T' : u;
            }
            if (q.seq.size() < shortest) {
                fprintf(stderr, "mbgc-hip f: %s %s has %zu letters: --mismatches %u needs at least 8 (%u + 1) = %llu\n", what, q.name.c_str(), q.seq.size(), opt.findMismatches,
                        opt.findMismatches, (unsigned long long) shortest);
                return EXIT_FAILURE;
            }
            if (q.seq.size() > 65535) { fprintf(stderr, "mbgc-hip f: %s %s has %zu letters (at most 65535)\n", what, q.name.c_str(), q.seq.size()); return EXIT_FAILURE; }
            continue;
        }
        for (char &c : q.seq) {
            if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) { fprintf(stderr, "mbgc-hip f: query %s holds a byte that is no letter\n", q.name.c_str()); return EXIT_FAILURE; }
            c &= (char) 0xDF;
        }
        if (q.seq.size() < shortest) {
            fprintf(stderr, "mbgc-hip f: query %s has %zu bases: --mismatches %u needs at least %llu\n", q.name.c_str(), q.seq.size(), opt.findMismatches, (unsigned long long) shortest);
            return EXIT_FAILURE;
        }
        if (q.seq.size() > 65535) { fprintf(stderr, "mbgc-hip f: query %s has %zu bases (at most 65535)\n", q.name.c_str(), q.seq.size()); return EXIT_FAILURE; }
    }
    return decodeAndReport('f', prefix, std::string(), opt);                                    // (0: a hit, 3: none)
}

const char *const MBGC_HIP_S_USAGE =
    "mbgc-hip s [--records file] [--gaps-out file [--min-gap N]] [--masked-out file [--min-masked N]] [--stats-host] [--serial] [--no-index]\n"
    "                  [--restore-rc] [--select pattern]... [--select-list file] [--select-seq pattern]... [--select-seq-list file] [-d device] [--bench]\n"
    "                  <streamsPrefix>\n"
    "  describes the collection without unpacking it: the chosen contigs are decoded as mbgc-hip d decodes them (--serial, --no-index,\n"
    "  --restore-rc, --select, --select-list, --select-seq, --select-seq-list: as there; contigs decoded only as dependencies are not counted)\n"
    "  and scanned where they lie, on the device; no sequence file is written. One tab-separated line per file on stdout, in collection order:\n"
    "  file, records, bases, min, max, N50, L50, A, C, G, T, N, other, lower, GC. A, C, G, T (with U) and N are counted without case, other is\n"
    "  every other byte, lower the bytes in a..z whatever the letter; GC = (G + C) / (A + C + G + T), 0.000000 without one of them; N50 / L50\n"
    "  over the file's chosen records, longest first: L50 = the fewest records that hold half the file's bases, N50 = the length of the last of\n"
    "  them. Then `stats: <files> files, <records> records, <bases> bases; GC <gc>, N <n> in <runs> runs, lower-case <n>, other <n>`. A protein\n"
    "  collection is counted by the same rule: most of its letters are `other`. Exit status 0; 1: malformed streams, a refused option or a\n"
    "  file that cannot be written\n"
    "  --records file (-: stdout, in front of the files' lines): the same columns per record, `file, record` (the first word of its header) in\n"
    "  place of `file, records`, without min, max, N50 and L50\n"
    "  --gaps-out file [--min-gap N]: the runs of N / n of at least N bytes (default 1) as BED lines — record, start (0-based), end (half-open) —\n"
    "  in collection order, then by start; --masked-out file [--min-masked N]: the runs of lower case in the same way. A run never reaches\n"
    "  over a record's end\n"
    "  --stats-host: a developer switch, the chosen contigs are downloaded and counted by a plain loop on the host, and the two results must\n"
    "  agree. --bench: two decodes, the second one timed, the scan run six times (the median of the last five); one JSON line\n"
    "  (stats_kernel_ms, bases, records, edges, edge_reruns, decode_ms, stats_gb_per_s). Not with --region, --check or --fasta\n";

// `mbgc-hip s`: the decode of `t` — nothing is written —, then the statistics in place of the check
int mbgc_hip_stats_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.stats = opt.writeNothing = true;
    std::string prefix;
    const ScanTool tool = {'s', MBGC_HIP_S_USAGE, "the statistics are taken over whole records (an option of mbgc-hip d)", "s writes no sequence, it describes the set where it lies"};
    const int r = scanCommandLine(tool, argc, argv, opt, [&](const std::string &a, int &i) {
        if (a == "--records" && i + 1 < argc) opt.statsRecordsFile = argv[++i];
        else if (a == "--gaps-out" && i + 1 < argc) opt.statsGapsOut = argv[++i];
        else if (a == "--masked-out" && i + 1 < argc) opt.statsMaskedOut = argv[++i];
        else if (a == "--min-gap" && i + 1 < argc) { if (!numberOption('s', "--min-gap", "a number of bytes", argv[++i], opt.statsMinGap)) return -1; }
        else if (a == "--min-masked" && i + 1 < argc) { if (!numberOption('s', "--min-masked", "a number of bytes", argv[++i], opt.statsMinMasked)) return -1; }
        else if (a == "--stats-host") opt.statsHost = true;
        else return 0;
        return 1;
    }, [] { return 0; }, prefix);
    return r >= 0 ? r : decodeAndReport('s', prefix, std::string(), opt);
}

const char *const MBGC_HIP_K_USAGE =
    "mbgc-hip k [-k K] [--scale S] [--by-record] [--pairs-out file] [--min-shared N] [--no-pairs] [--sketches-out file] [--order-out file] [--sketch-host]\n"
    "                  [--serial] [--no-index] [--restore-rc] [--select pattern]... [--select-list file] [--select-seq pattern]... [--select-seq-list file]\n"
    "                  [-d device] [--bench] <streamsPrefix>\n"
    "  which genomes of the collection are close to which, without unpacking it: the chosen contigs are decoded as mbgc-hip d decodes them\n"
    "  (--serial, --no-index, --restore-rc, --select, --select-list, --select-seq, --select-seq-list: as there; contigs decoded only as\n"
    "  dependencies are not sketched) and hashed where they lie, on the device. A group is a file, or a record (named by the first word of its\n"
    "  header) under --by-record. Every k-mer (-k 1..32, default 21) of A/C/G/T/U letters, either case, inside one record is hashed in its\n"
    "  canonical form, and a hash is kept when it is at most (2^64 - 1) / S (--scale, default 1000; 1 keeps all): a FracMinHash sketch. The\n"
    "  hash is this project's own (fmix64 of the 2-bit packed k-mer): the sketches cannot be exchanged with Mash's or sourmash's.\n"
    "  One tab-separated line per group on stdout, in collection order: name, records, bases, kmers (valid k-mer positions), hashes (distinct\n"
    "  kept), hashes x S (the estimate of the distinct k-mers). Then one line per pair A < B of groups: nameA, nameB, hashesA, hashesB, shared,\n"
    "  jaccard = shared / (hashesA + hashesB - shared), containmentA = shared / hashesA, containmentB, distance = -ln(2 J / (1 + J)) / K (1\n"
    "  when J is 0). Then `sketch: <groups> groups, <records> records, <bases> bases; k <K>, scale <S>; <hashes> hashes of <kmers> k-mers,\n"
    "  <pairs> pairs, <n> share a hash`. Exit status 0; 1: malformed streams, a refused option or a file that cannot be written\n"
    "  --pairs-out file: the pair lines go there; --min-shared N: only the pairs that share at least N hashes; --no-pairs: no pair is\n"
    "  computed (more than 2^28 pairs are refused without it)\n"
    "  --sketches-out file: per group name, K, S, the number of hashes and the hashes as 16 hex digits, comma-separated\n"
    "  --order-out file: a file list for mbgc-hip c — first the file that shares the most hashes with all others, then the others by what they\n"
    "  share with it, descending; not with --by-record or --no-pairs\n"
    "  --sketch-host: a developer switch, the chosen contigs are downloaded, hashed and intersected by plain loops on the host, and the two\n"
    "  results must agree. --bench: two decodes, the second one timed, the scans run six times (the medians of the last five); one JSON line\n"
    "  (sketch_kernel_ms, pairs_kernel_ms, sort_ms, bases, rows, row_reruns, hashes, pairs, decode_ms, sketch_gb_per_s). Not with --region,\n"
    "  --check or --fasta\n";

// `mbgc-hip k`: the decode of `t` — nothing is written —, then the sketches in place of the check
int mbgc_hip_sketch_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.sketch = opt.writeNothing = true;
    std::string prefix;
    const ScanTool tool = {'k', MBGC_HIP_K_USAGE, "the sketches are taken over whole records (an option of mbgc-hip d)", "k writes no sequence, it compares the set where it lies"};
    const int r = scanCommandLine(tool, argc, argv, opt, [&](const std::string &a, int &i) {
        uint64_t v = 0;
        if (a == "-k" && i + 1 < argc) {
            if (!numberOption('k', "-k", "a number", argv[++i], v)) return -1;
            if (v < 1 || v > 32) { fprintf(stderr, "mbgc-hip k: -k %llu: a k-mer has 1 to 32 bases (2 bits each in one 64-bit word)\n", (unsigned long long) v); return -1; }
            opt.sketchK = (uint32_t) v;
        }
        else if (a == "--scale" && i + 1 < argc) {
            if (!numberOption('k', "--scale", "a number", argv[++i], v)) return -1;
            if (v < 1) { fprintf(stderr, "mbgc-hip k: --scale 0: a hash is kept when it is at most (2^64 - 1) / scale, 1 keeps every hash\n"); return -1; }
            opt.sketchScale = v;
        }
        else if (a == "--min-shared" && i + 1 < argc) { if (!numberOption('k', "--min-shared", "a number", argv[++i], opt.sketchMinShared)) return -1; }
        else if (a == "--by-record") opt.sketchByRecord = true;
        else if (a == "--no-pairs") opt.sketchNoPairs = true;
        else if (a == "--sketch-host") opt.sketchHost = true;
        else if (a == "--pairs-out" && i + 1 < argc) opt.sketchPairsOut = argv[++i];
        else if (a == "--sketches-out" && i + 1 < argc) opt.sketchOut = argv[++i];
        else if (a == "--order-out" && i + 1 < argc) opt.sketchOrderOut = argv[++i];
        else return 0;
        return 1;
    }, [&] {
        if (opt.sketchOrderOut.empty() || (!opt.sketchByRecord && !opt.sketchNoPairs)) return 0;
        fprintf(stderr, "mbgc-hip k: --order-out orders files by the hashes they share: not with --by-record or --no-pairs\n");
        return 1;
    }, prefix);
    return r >= 0 ? r : decodeAndReport('k', prefix, std::string(), opt);
}

const char *const MBGC_HIP_U_USAGE =
    "mbgc-hip u [--forward-only] [--exact-case] [--min-len N] [--clusters-out file] [--unique-files-out file] [--dups-host] [--serial] [--no-index]\n"
    "                  [--restore-rc] [--select pattern]... [--select-list file] [--select-seq pattern]... [--select-seq-list file] [-d device] [--bench]\n"
    "                  <streamsPrefix>\n"
    "  which records of the collection are the same sequence, without unpacking it: the chosen contigs are decoded as mbgc-hip d decodes them\n"
    "  (--serial, --no-index, --restore-rc, --select, --select-list, --select-seq, --select-seq-list: as there; contigs decoded only as\n"
    "  dependencies are not classed) and compared where they lie, on the device. Two records are the same when they have the same length and\n"
    "  the same bytes, letters compared without case (--exact-case: as they are), read forward or — unless --forward-only — one as the reverse\n"
    "  complement of the other (A-T, C-G, R-Y, K-M, B-V, D-H, either case; every other byte is its own complement). The answer is exact: a\n"
    "  fingerprint only proposes, every duplicate is compared byte by byte. A class is represented by its first record in collection order.\n"
    "  One tab-separated line per duplicate record — every record that is not its class's representative — on stdout, in collection order:\n"
    "  record (the first word of its header), file, length, strand (+, or - when it equals only the representative's reverse complement),\n"
    "  representative record, representative file. Then `dups: <records> records, <bases> bases; <classes> distinct sequences; <d> duplicate\n"
    "  records, <db> bases (<rc> as reverse complements); <df> of <files> files duplicate`. Exit status 0; 1: malformed streams, a refused\n"
    "  option or a file that cannot be written\n"
    "  --min-len N: records shorter than N (default 1, so empty records) are left out of the lines and of the duplicate counts\n"
    "  --clusters-out file: every class with more than one member, one line per member, the representative first: the same columns and the\n"
    "  class's number (1, 2, ... in collection order of the representatives)\n"
    "  --unique-files-out file: a file is a duplicate of an earlier one when the sorted lists of their records' classes are equal, whatever\n"
    "  the strands; the names of the files that are no duplicates, in collection order, one per line — a list for mbgc-hip d / r\n"
    "  --select-list. --select matches SUBSTRINGS of the names: a name that is contained in another one chooses both\n"
    "  --dups-host: a developer switch, the chosen contigs are downloaded and classed by a map over canonical strings on the host, and the\n"
    "  two results must agree. --bench: two decodes, the second one timed, the scan run six times (the medians of the last five); one JSON\n"
    "  line (dups_kernel_ms, verify_ms, bases, records, buckets, verified, refuted, decode_ms, dups_gb_per_s). Not with --region, --check\n"
    "  or --fasta\n";

// `mbgc-hip u`: the decode of `t` — nothing is written —, then the classes in place of the check
int mbgc_hip_dups_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.dups = opt.writeNothing = true;
    std::string prefix;
    const ScanTool tool = {'u', MBGC_HIP_U_USAGE, "whole records are compared (an option of mbgc-hip d)", "u writes no sequence, it compares the records where they lie"};
    const int r = scanCommandLine(tool, argc, argv, opt, [&](const std::string &a, int &i) {
        if (a == "--forward-only") opt.dupsForwardOnly = true;
        else if (a == "--exact-case") opt.dupsExactCase = true;
        else if (a == "--dups-host") opt.dupsHost = true;
        else if (a == "--min-len" && i + 1 < argc) { if (!numberOption('u', "--min-len", "a number of bytes", argv[++i], opt.dupsMinLen)) return -1; }
        else if (a == "--clusters-out" && i + 1 < argc) opt.dupsClustersOut = argv[++i];
        else if (a == "--unique-files-out" && i + 1 < argc) opt.dupsUniqueFilesOut = argv[++i];
        else return 0;
        return 1;
    }, [] { return 0; }, prefix);
    return r >= 0 ? r : decodeAndReport('u', prefix, std::string(), opt);
}

const char *const MBGC_HIP_M_USAGE =
    "mbgc-hip m [--seq ACGT...]... [--seq-file genes.fa] [-k K] [--by-record] [--min-shared N] [--min-containment F] [--loci-out file]\n"
    "                  [--regions-out file [--flank N]] [--max-gap N] [--min-locus-hits N] [--hit-capacity N] [--screen-host] [--serial] [--no-index]\n"
    "                  [--restore-rc] [--select pattern]... [--select-list file] [--select-seq pattern]... [--select-seq-list file] [-d device] [--bench]\n"
    "                  <streamsPrefix>\n"
    "  which genomes of the collection carry a query (a gene, a plasmid, a phage) in whatever allele, and where, without unpacking it: the chosen\n"
    "  contigs are decoded as mbgc-hip d decodes them (--serial, --no-index, --restore-rc, --select, --select-list, --select-seq,\n"
    "  --select-seq-list: as there; contigs decoded only as dependencies are not screened) and scanned where they lie, on the device. --seq: a\n"
    "  query, named q1, q2, ... in command-line order; --seq-file: a FASTA file of queries, each named by the first word of its header. A k-mer\n"
    "  (-k 1..32, default 21) is k letters of A/C/G/T/U, either case, inside one record or one query; its key is its canonical form — the\n"
    "  smaller of the 2-bit packed k-mer and its reverse complement, no hash. A query's keys are its distinct ones; a query shorter than K or\n"
    "  without a valid k-mer is refused, as are no query at all and more than 2^24 distinct keys. A group is a file, or a record (named by the\n"
    "  first word of its header) under --by-record. shared = the query's keys that occur in the group, containment = shared / the query's keys\n"
    "  (k-mer containment, as mash screen and the k-mer indexes answer; f finds a query with at most 3 substitutions, m an allele at 90 %)\n"
    "  One tab-separated line per query and group with shared >= --min-shared (default 1) and containment >= --min-containment (default 0) on\n"
    "  stdout, in query order, then collection order: query, group, query_kmers, shared, containment. Then `screen: <queries> queries, <keys>\n"
    "  distinct k-mers, k <K>; <groups> groups, <records> records, <bases> bases; <hits> hits, <pairs> pairs reported` (hits: the positions\n"
    "  whose k-mer is a key). Exit status 0: a pair was reported; 3: none; 1: malformed streams or a refusal\n"
    "  --loci-out file: a query's hit positions in a record, ascending, are cut wherever two neighbours are more than --max-gap (default 500)\n"
    "  apart; a piece of at least --min-locus-hits (default 3) positions is a locus: query, file, record, start (first position + 1), end\n"
    "  (last position + K), hits (its positions), distinct (the different keys among them), tab-separated, sorted by query, file, record,\n"
    "  start. Coordinates are 1-based, inclusive, forward strand. NO STRAND is reported: a canonical k-mer has none\n"
    "  --regions-out file [--flank N]: a line RECORD:FROM-TO per locus, FROM = max(1, start - N), TO = end + N, identical lines once; mbgc-hip d\n"
    "  --region-list file then fetches those pieces (d clamps TO; d matches RECORD as a SUBSTRING of the header line, as for f --regions-out)\n"
    "  The hits leave the device only for these two options. --hit-capacity N: the most hits they may take; a run with more is refused and\n"
    "  says how many there are (a query that is a whole genome of the collection hits at nearly every position)\n"
    "  --screen-host: a developer switch, the chosen contigs are downloaded and screened by plain loops over a std::set on the host, and the\n"
    "  two results must agree. --bench: two decodes, the second one timed, the scan run six times (the medians of the last five); one JSON line\n"
    "  (screen_kernel_ms, sort_ms, bases, keys, table_slots, filter_passes, hits, hit_reruns, decode_ms, screen_gb_per_s). Not with --region,\n"
    "  --check or --fasta\n";

// `mbgc-hip m`: the decode of `t` — nothing is written —, then the screen in place of the check
int mbgc_hip_screen_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.screen = opt.writeNothing = true;
    int inlineQueries = 0;
    bool lociOptions = false;
    std::string prefix;
    const ScanTool tool = {'m', MBGC_HIP_M_USAGE, "a screen looks at whole records (an option of mbgc-hip d; m --regions-out writes such a list)", "m writes no sequence, it screens the set where it lies"};
    const int r = scanCommandLine(tool, argc, argv, opt, [&](const std::string &a, int &i) {
        uint64_t v = 0;
        if (a == "--seq" && i + 1 < argc) opt.screenQueries.push_back({"q" + std::to_string(++inlineQueries), argv[++i]});
        else if (a == "--seq-file" && i + 1 < argc) {
            if (!readQueryFile(argv[++i], opt.screenQueries)) { fprintf(stderr, "mbgc-hip m: cannot open the query file %s\n", argv[i]); return -1; }
        }
        else if (a == "-k" && i + 1 < argc) {
            if (!numberOption('m', "-k", "a number", argv[++i], v)) return -1;
            if (v < 1 || v > 32) { fprintf(stderr, "mbgc-hip m: -k %llu: a k-mer has 1 to 32 bases (2 bits each in one 64-bit word)\n", (unsigned long long) v); return -1; }
            opt.screenK = (uint32_t) v;
        }
        else if (a == "--by-record") opt.screenByRecord = true;
        else if (a == "--min-shared" && i + 1 < argc) { if (!numberOption('m', "--min-shared", "a number", argv[++i], opt.screenMinShared)) return -1; }
        else if (a == "--min-containment" && i + 1 < argc) {
            char *end = nullptr;
            const char *text = argv[++i];
            opt.screenMinContainment = strtod(text, &end);
            if (!*text || *end || !(opt.screenMinContainment >= 0 && opt.screenMinContainment <= 1)) { fprintf(stderr, "mbgc-hip m: --min-containment takes a fraction from 0 to 1\n"); return -1; }
        }
        else if (a == "--loci-out" && i + 1 < argc) opt.screenLociOut = argv[++i];
        else if (a == "--regions-out" && i + 1 < argc) opt.screenRegionsOut = argv[++i];
        else if (a == "--flank" && i + 1 < argc) { lociOptions = true; if (!numberOption('m', "--flank", "a number of bases", argv[++i], opt.screenFlank)) return -1; }
        else if (a == "--max-gap" && i + 1 < argc) { lociOptions = true; if (!numberOption('m', "--max-gap", "a number of bases", argv[++i], opt.screenMaxGap)) return -1; }
        else if (a == "--min-locus-hits" && i + 1 < argc) {
            lociOptions = true;
            if (!numberOption('m', "--min-locus-hits", "a number of positions", argv[++i], opt.screenMinLocusHits)) return -1;
            if (!opt.screenMinLocusHits) { fprintf(stderr, "mbgc-hip m: --min-locus-hits 0: a locus has at least one position\n"); return -1; }
        }
        else if (a == "--hit-capacity" && i + 1 < argc) {
            lociOptions = true;
            if (!numberOption('m', "--hit-capacity", "a number of hits", argv[++i], opt.screenHitCapacity)) return -1;
            if (!opt.screenHitCapacity) { fprintf(stderr, "mbgc-hip m: --hit-capacity takes a positive number of hits\n"); return -1; }
        }
        else if (a == "--screen-host") opt.screenHost = true;
        else return 0;
        return 1;
    }, [&] {
        if (opt.screenQueries.empty()) return 2;
        if (lociOptions && opt.screenLociOut.empty() && opt.screenRegionsOut.empty()) {
            fprintf(stderr, "mbgc-hip m: --flank, --max-gap, --min-locus-hits and --hit-capacity go with --loci-out or --regions-out\n");
            return 1;
        }
        return 0;
    }, prefix);
    if (r >= 0) return r;
    // the queries, held to the screen's limits before anything is decoded
    for (const MBGC_Decoder::FindQuery &q : opt.screenQueries) {
        if (q.seq.size() < opt.screenK) { fprintf(stderr, "mbgc-hip m: query %s has %zu bases, fewer than k = %u\n", q.name.c_str(), q.seq.size(), opt.screenK); return EXIT_FAILURE; }
        if (mbgc_screen::canonsOf(q.seq, opt.screenK).empty()) {
            fprintf(stderr, "mbgc-hip m: query %s has no k-mer of %u letters of A, C, G, T or U in a row\n", q.name.c_str(), opt.screenK);
            return EXIT_FAILURE;
        }
    }
    const size_t keys = mbgc_screen::buildKeys(screenSequences(opt), opt.screenK).keys.size();
    if (keys > ((size_t) 1 << 24)) { fprintf(stderr, "mbgc-hip m: the queries have %zu distinct k-mers, more than 2^24: screen them in parts\n", keys); return EXIT_FAILURE; }
    return decodeAndReport('m', prefix, std::string(), opt);                                    // (0: a pair was reported, 3: none)
}

// `mbgc-hip v` (the reference's `mbgc v`, main.cpp:420-445): decode as `d` does, format as `d --fasta` does, compare on the device
int mbgc_hip_validate_main(int argc, char **argv) {
    MBGC_Decoder::Options opt;
    opt.validate = true;
    std::vector<std::string> pos;
    bool selectAsked = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (const int r = mbgc_hip_decode_option('v', argc, argv, i, opt, selectAsked)) { if (r < 0) return EXIT_FAILURE; }
        else if (a == "--bench") opt.bench = true;
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
        else if (a == "--gpus") { fprintf(stderr, "mbgc-hip v: validation runs on one GPU (--gpus is an option of mbgc-hip c)\n"); return EXIT_FAILURE; }
        else pos.push_back(a);
    }
    if (pos.size() != 1) { fprintf(stderr, "usage: %s", MBGC_HIP_V_USAGE); return EXIT_FAILURE; }
    if (opt.selectSeqAsked) {
        fprintf(stderr, "mbgc-hip v: --select-seq / --select-seq-list select records, and a file that holds only some of its records has no original to be validated against (an option of mbgc-hip d)\n");
        return EXIT_FAILURE;
    }
    if (opt.regionAsked) {
        fprintf(stderr, "mbgc-hip v: --region / --region-list select parts of records, and a file that holds only parts of its records has no original to be validated against (an option of mbgc-hip d)\n");
        return EXIT_FAILURE;
    }
    if (!mbgc_hip_check_selection('v', opt, selectAsked)) return EXIT_FAILURE;
    return decodeAndReport('v', pos[0], std::string(), opt);
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

// The walk over what was chosen (chosenUnits / mergedRanges, mbgc_decoder_streams.h) under --select-seq: g0n contigs in the initial
// reference, seqCount[T] per target, unitSel[T + 1] (G0's unit first), contigSel[g0n + sum(seqCount)] per contig of the collection
// (G0's first; NULL: whole units), sequentialMatching = -t1. rows: {unit, c0, c1} per maximal run of chosen contigs of a chosen unit;
// ranges: {from, to} of the merged output ranges. 0, or -2 (a cap too small; *nrows / *nranges = what is needed).
int mbgc_decoder_runs(uint64_t g0n, const uint32_t *seqCount, uint64_t T, const uint8_t *unitSel, const uint8_t *contigSel, int sequentialMatching, uint64_t *rows,
                      uint64_t rowCap, uint64_t *nrows, uint64_t *ranges, uint64_t rangeCap, uint64_t *nranges) {
    const std::vector<ChosenUnit> chosen = chosenUnits(g0n, seqCount, (size_t) T, (const char *) unitSel, (const char *) contigSel, sequentialMatching != 0);
    const std::vector<Interval> merged = mergedRanges(chosen);
    *nrows = chosen.size(); *nranges = merged.size();
    if (chosen.size() > rowCap || merged.size() > rangeCap) return -2;
    for (size_t i = 0; i < chosen.size(); i++) { rows[3 * i] = chosen[i].unit; rows[3 * i + 1] = chosen[i].c0; rows[3 * i + 2] = chosen[i].c1; }
    for (size_t i = 0; i < merged.size(); i++) { ranges[2 * i] = merged[i].from; ranges[2 * i + 1] = merged[i].to; }
    return 0;
}

// The walk over whole chosen units (no contigSel: a row per chosen unit, one without a contig too), otherwise as above.
int mbgc_decoder_units(uint64_t g0n, const uint32_t *seqCount, uint64_t T, const uint8_t *unitSel, int sequentialMatching, uint64_t *rows, uint64_t rowCap,
                       uint64_t *nrows, uint64_t *ranges, uint64_t rangeCap, uint64_t *nranges) {
    return mbgc_decoder_runs(g0n, seqCount, T, unitSel, nullptr, sequentialMatching, rows, rowCap, nrows, ranges, rangeCap, nranges);
}

// ---- --region for the tests. mbgc_region_parse: 0 and the spec's parts, or -1 and the reason in err.
int mbgc_region_parse(const char *text, char *pattern, uint64_t cap, uint64_t *from, uint64_t *to, char *err, uint64_t errCap) {
    MBGC_Decoder::RegionSpec spec;
    std::string why;
    if (!MBGC_Decoder::parseRegionSpec(text, spec, &why)) { if (err && errCap) snprintf(err, errCap, "%s", why.c_str()); return -1; }
    snprintf(pattern, cap, "%s", spec.pattern.c_str());
    *from = spec.from; *to = spec.to;
    return 0;
}
// the header of a piece (regionHeader)
int mbgc_region_header(const char *header, uint64_t from1, uint64_t to1, char *out, uint64_t cap) {
    const std::string h = regionHeader(header, from1, to1);
    if (h.size() + 1 > cap) return -2;
    memcpy(out, h.c_str(), h.size() + 1);
    return 0;
}
// resolveRegions: asks as rows of {contig, from, to} (1-based, inclusive) against contigLen; pieces as rows of {contig, from0, len} in
// output order; *skipped: the asks that start behind their record's end. 0, or -2 (cap too small; *npieces = the rows needed).
int mbgc_region_resolve(const uint64_t *asks, uint64_t nasks, const uint64_t *contigLen, uint64_t ncontigs, uint64_t *pieces, uint64_t cap, uint64_t *npieces, uint64_t *skipped) {
    Selection sel;
    for (uint64_t i = 0; i < nasks; i++) { if (asks[3 * i] >= ncontigs) return -1; sel.asks.push_back({asks[3 * i], asks[3 * i + 1], asks[3 * i + 2], 0}); }
    resolveRegions(std::vector<uint64_t>(contigLen, contigLen + ncontigs), false, sel);
    *npieces = sel.pieces.size(); *skipped = sel.regionSkipped;
    if (sel.pieces.size() > cap) return -2;
    for (size_t i = 0; i < sel.pieces.size(); i++) { pieces[3 * i] = sel.pieces[i].contig; pieces[3 * i + 1] = sel.pieces[i].from; pieces[3 * i + 2] = sel.pieces[i].len; }
    return 0;
}

// The granule closure on the host (Provenance::closureRegion) over a schedule as mbgc_decoder_provenance takes it. timeSeg[c]: contig
// c is filled against the buffer as the loader left it just before segment timeSeg[c]; recs / recBase: the planned records, contig
// after contig; units: rows of {c0, c1} in the order they run; granBase (out, ncontigs + 1), needGranules / needContigs: in, the
// chosen granules and their contigs; out, the closure. rows (may be NULL): the table as rows of {vstart, len, owner, ownerFirst,
// reversed}. 0, -1 (arguments), -2 (rowCap too small; *nrows = the rows needed).
int mbgc_decoder_region_closure(const int64_t *segs, uint64_t nsegs, uint64_t refTotalLength, uint64_t firstPlanned, uint64_t ncontigs, const uint64_t *destLen,
                                const uint64_t *timeSeg, const swsem_decode_record_t *recs, const uint64_t *recBase, const uint64_t *units, uint64_t nunits, uint32_t shift,
                                uint64_t *granBase, uint32_t *needGranules, uint32_t *needContigs, uint64_t *filled, int64_t *rows, uint64_t rowCap, uint64_t *nrows) {
    if (refTotalLength < 2 || shift > 40) return -1;
    Provenance prov;
    prov.L = refTotalLength;
    std::vector<uint64_t> curAt(nsegs + 1);
    for (uint64_t i = 0; i < nsegs; i++) {
        curAt[i] = prov.cur;
        prov.add({segs[5 * i], (uint64_t) segs[5 * i + 1], (uint64_t) segs[5 * i + 2], (uint64_t) segs[5 * i + 3], segs[5 * i + 4] != 0}, firstPlanned);
    }
    curAt[nsegs] = prov.cur;
    if (nrows) *nrows = prov.rows.size();
    if (rows) {
        if (prov.rows.size() > rowCap) return -2;
        for (size_t i = 0; i < prov.rows.size(); i++) {
            const int64_t row[5] = {(int64_t) prov.rows[i].vstart, (int64_t) prov.rows[i].len, prov.rows[i].owner, (int64_t) prov.ext[i].ownerFirst, (int64_t) prov.ext[i].reversed};
            memcpy(rows + 5 * i, row, sizeof row);
        }
    }
    Provenance::RegionNeed N;
    N.shift = shift;
    N.granBase.assign(ncontigs + 1, 0);
    std::vector<uint64_t> len(destLen, destLen + ncontigs), timeOf(ncontigs);
    std::vector<std::vector<swsem_decode_record_t>> perContig(ncontigs);
    for (uint64_t c = 0; c < ncontigs; c++) {
        if (timeSeg[c] > nsegs) return -1;
        N.granBase[c + 1] = N.granBase[c] + ((len[c] + (1ull << shift) - 1) >> shift);
        timeOf[c] = curAt[timeSeg[c]];
        perContig[c].assign(recs + recBase[c], recs + recBase[c + 1]);
    }
    memcpy(granBase, N.granBase.data(), (ncontigs + 1) * sizeof(uint64_t));
    const size_t gw = (size_t) ((N.granBase[ncontigs] + 31) / 32), cw = (size_t) ((ncontigs + 31) / 32);
    N.gran.assign(needGranules, needGranules + gw); N.gran.push_back(0);
    N.contig.assign(needContigs, needContigs + cw);
    std::vector<swsem_fill_unit_t> sweep;
    for (uint64_t u = 0; u < nunits; u++) sweep.push_back({units[2 * u], units[2 * u + 1]});
    prov.closureRegion(perContig, len, timeOf, sweep, N);
    memcpy(needGranules, N.gran.data(), gw * sizeof(uint32_t));
    memcpy(needContigs, N.contig.data(), cw * sizeof(uint32_t));
    *filled = N.filled;
    return 0;
}

// The device's granule closure and masked fill held to the host's on a stream set on disk (needs a GPU): the streams under prefix
// are planned and scheduled as `d` does it, the pieces — rows of {contig of the collection, from0, len} — go in as the need state,
// and under outPrefix come back, as raw little-endian arrays: .granBase (u64), .needDev / .needHost (u32: the granule bitmap of
// k_decode_closure_region and of Provenance::closureRegion over the records downloaded from the plan), .contigDev / .contigHost,
// .filled (u64: device, host), .seqOff (u64, per contig of the collection + 1), .contigLen, .recBase (u64, per planned contig + 1),
// .recDest (u64: every record's destAt), .masked (the sequence buffer after the masked forward run over a buffer of 0xEE bytes).
int mbgc_decoder_region_probe(const char *prefix, int restoreRc, int serial, const uint64_t *pieces, uint64_t npieces, uint32_t granule, const char *outPrefix,
                              char *err, uint64_t errCap) {
    std::string msg;
    const auto failed = [&]() { if (err && errCap) snprintf(err, errCap, "%s", msg.c_str()); return -1; };
    MBGC_Decoder::Options opt;
    opt.restoreRc = restoreRc != 0; opt.serial = serial != 0;
    StreamSet S;
    Selection sel;
    if (!readStreamFiles(prefix, opt, S, msg) || !restoreRcLiterals(prefix, opt, S, msg) || !checkStreams(S, msg) || !chainStarts(false, S, msg)) return failed();
    const uint64_t N = S.g0n + S.planned;
    sel.unitSel.assign(S.T() + 1, 1);
    sel.selecting = sel.selectingRegion = true;
    sel.contigSel.assign(N, 0);
    while ((1u << sel.granuleShift) < granule) sel.granuleShift++;
    while ((1u << sel.granuleShift) > granule) sel.granuleShift--;
    for (uint64_t i = 0; i < npieces; i++) {
        if (pieces[3 * i] >= N) { msg = "a piece names no contig"; return failed(); }
        sel.pieces.push_back({pieces[3 * i], pieces[3 * i + 1], pieces[3 * i + 2], 0});
        sel.contigSel[pieces[3 * i]] = 1;
    }
    DecodedCollection D;
    D.sentinel = 0xEE;
    if (!D.upload(S, 0, msg) || !D.planAndSchedule(S, opt.serial, msg)) return failed();
    for (const RegionPiece &p : sel.pieces) if (p.from + p.len > D.contigLen[p.contig] || !p.len) { msg = "a piece leaves its contig"; return failed(); }
    if (!D.closure(S, sel, msg)) return failed();
    // the referee: the records as the plan left them, the same table, times and units
    std::vector<std::vector<swsem_decode_record_t>> recs(S.planned);
    std::vector<uint64_t> destLen(S.planned), recBase(1, 0), recDest;
    for (uint64_t c = 0; c < S.planned; c++) {
        uint64_t n = 0;
        if (swsem_debug_copy_records(D.h, c, nullptr, 0, &n)) { hipFail(msg, "records"); return failed(); }
        recs[c].resize(n);
        if (n && swsem_debug_copy_records(D.h, c, recs[c].data(), n, &n)) { hipFail(msg, "records"); return failed(); }
        destLen[c] = D.contigLen[S.g0n + c];
        for (const swsem_decode_record_t &r : recs[c]) recDest.push_back(r.destAt);
        recBase.push_back(recDest.size());
    }
    Provenance::RegionNeed H;
    H.shift = sel.granuleShift; H.granBase = D.regionNeed.granBase;
    H.gran.assign(D.regionNeed.gran.size(), 0); H.contig.assign(D.regionNeed.contig.size(), 0);
    for (const RegionPiece &p : sel.pieces) {
        if (p.contig < S.g0n) continue;
        const uint64_t k = p.contig - S.g0n;
        H.contig[k >> 5] |= 1u << (k & 31);
        for (uint64_t g = H.granBase[k] + (p.from >> H.shift); g <= H.granBase[k] + ((p.from + p.len - 1) >> H.shift); g++) H.gran[g >> 5] |= 1u << (g & 31);
    }
    D.prov.closureRegion(recs, destLen, D.timeOf, D.sweepUnits(), H);
    if (!D.forwardRun(S, true, msg)) return failed();
    std::string masked(D.totalBases, '\0');
    if (D.totalBases && swsem_dev_download(D.h, &masked[0], D.seqDev, D.totalBases)) { hipFail(msg, "download"); return failed(); }
    const uint64_t filled[2] = {D.regionNeed.filled, H.filled};
    const std::string o = outPrefix;
    const auto put = [&](const char *ext, const void *p, size_t n) { return writeFile(o + ext, p, n); };
    if (!put(".granBase", H.granBase.data(), H.granBase.size() * 8) || !put(".needDev", D.regionNeed.gran.data(), D.regionNeed.gran.size() * 4) ||
        !put(".needHost", H.gran.data(), H.gran.size() * 4) || !put(".contigDev", D.regionNeed.contig.data(), D.regionNeed.contig.size() * 4) ||
        !put(".contigHost", H.contig.data(), H.contig.size() * 4) || !put(".filled", filled, sizeof filled) || !put(".seqOff", D.seqOff.data(), D.seqOff.size() * 8) ||
        !put(".contigLen", D.contigLen.data(), D.contigLen.size() * 8) || !put(".recBase", recBase.data(), recBase.size() * 8) ||
        !put(".recDest", recDest.data(), recDest.size() * 8) || !put(".masked", masked.data(), masked.size())) { msg = "cannot write under " + o; return failed(); }
    return 0;
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
