// Host-side drivers of the compress hot path with the reference's class names and hook surface:
//   MultipleGenomeMatchingProcessor  matching/MultipleGenomeMatchingProcessor.{h,cpp}  (file list, G0
//       reference, matcher sizing, the two target loops, in-order reference extension)
//   MBGC_Encoder                     mbgccoder/MBGC_Encoder.{h,cpp}:128-564,759-807      (the hooks
//       that collect the match/literal byte streams, and prepareAndCompressStreams' job table + container framing
//       (:641-710, include/mbgc_backend.h) around the PPMd/LZMA coders, which are NOT part of this repo: they are the
//       reference's unchanged backend, handed in as a callback)
// Policy (which contigs extend the reference, dissimilar-contig retry, lock bookkeeping) stays on the
// host exactly as in the reference; everything that touches sequence bytes runs through the C ABI.
#pragma once
#include <cstdint>
#include <deque>
#include <functional>
#include <future>
#include <mutex>
#include <string>
#include <vector>

#include "sw_matcher.h"
#include "../../include/mbgc_fasta.h"
#include "../../include/mbgc_exchange.h"
#include "../../include/mbgc_backend.h"

struct MGMP_Params {                                   // matching/MGMP_Params.h (only what this path reads)
    int k = 32, k1 = 16, k2 = 1;                       // :199-202
    static constexpr int PROTEINS_PROFILE_KMER_LENGTH = 16;               // :27
    // probeProteinsProfile's state (:90-91), carried from one load of the initial reference to the next (the -i path that falls
    // back to the sequential schedule loads it twice); the probe itself runs on the device (mbgc_fasta_probe_dev)
    mbgc_fasta_probe_state_t probe = {MBGC_FASTA_PROBE_MAX_LEN, 0};
    uint8_t skipMargin = 16;                           // :203 (24 in -m2/-m3, MBGC_Params.h:908-909)
    int referenceFactor = -1;                          // ADJUSTED_REFERENCE_FACTOR_FLAG, :24,:205
    int referenceSlidingWindowFactor = 16;             // :206
    bool enable40bitReference = true;                  // :208
    bool circularReference = true;                     // :209
    uint8_t bigReferenceCompressorRatio = 16;          // :210 (4 in -m2/-m3)
    bool refRegionSeparators = true;                   // :12
    int currentUnmatchedFractionFactor = 128;          // :71
    int unmatchedFractionRCFactor = 8;                 // :73 (128 in -m2/-m3)
    bool rcInReference = true;                         // !isRCinReferenceDisabled(), :82-84
    bool sequentialMatching = false;                   // :218
    // Targets per round and GPU: the targets of a round hold their lock positions together (the deterministic stand-in for the
    // reference's worker threads, :16-22). 0 = as many as the reference's own rules let be in flight: what they load must fit the
    // sliding window once the buffer has wrapped (their shared lock stands one window ahead of the loading position and loadRef
    // drops what goes beyond it, SlidingWindowSparseEMMatcher.cpp:361-378,412-417,433), and at most matcherWorkingThreads x
    // allowedTargetsOutrunFactor = 64 targets run ahead of the finalizer (MGMP.cpp:374-375,532, :16,:57) — divided by the GPUs.
    int roundSize = 0;
    static constexpr int MAX_TARGETS_IN_FLIGHT = 64;
    bool uppercaseDNA = false;                         // :196 (-U)
    bool inflateOnDevice = false;                      // mbgc-hip c --inflate device: the gzip files of a list travel compressed and are inflated in HBM (mbgc_fasta_inflate_dev)
    bool allowLossyParsing = false;                    // :213 (the reference's -L; mbgc-hip c --lossy): the files of a list are read by kseq_read_lossy
    // mbgc-hip c --bench: every round's contigs are put into HBM first, the rounds after `benchWarmup` are timed and the
    // emitted streams stay packed in HBM (what bench.py measures, from the C++ host)
    bool benchMode = false;
    // mbgc-hip c / r --checksums: the CRC-32 of every contig's bases is taken on the device where the input stage leaves them
    // (mbgc_fasta_crc_dev) and kept for <outputPrefix>.checksums; crcKernelMs / crcBytes: what the kernel ran over
    bool checksums = false;
    double crcKernelMs = 0; uint64_t crcBytes = 0;
    // mbgc-hip c --verify: every emission is decoded again on the device (SlidingWindowSparseEMMatcher::emitVerify) before the
    // reference moves on, and the run fails on the first contig that does not come back; rounds then load on the host's decision
    bool verifyEmissions = false;
    int verifyEvery = 1;                               // --verify-every K: only the emissions of every K-th target file (sequential schedule) / round
    uint64_t verifiedContigs = 0, verifiedBases = 0;
    int benchWarmup = 0;
    double benchSeconds = 0; uint64_t benchBases = 0; int benchRounds = 0;   // filled by processTargetsRounds
    // several GPUs: this process is one rank of `exchange`; a round then holds roundSize targets PER RANK
    mbgc_xchg_t *exchange = nullptr;
    int specRounds = 0;                                // rounds whose finalize ran on the ranks' device-side verdicts (diagnostics)
    int headRounds = 0;                                // rounds whose extension exchange was cut to the loadable head (diagnostics)
    static constexpr uint64_t MIN_BASIC_BLOCK_SIZE = 1 << 21;             // :48
    // single fasta file mode (`mbgc c -i`, MBGC_Encoder.cpp:775): the collection is ONE multi-FASTA file, cut into the initial
    // reference (an element of at least MIN_REF_INIT_SIZE bytes) and targets (elements of at least MIN_BASIC_BLOCK_SIZE bytes) by
    // mgmpInSplit_next — on the device here (mbgc_fasta_split_dev), window by window
    std::string inputFileName;
    uint64_t singleFileWindow = 32u << 20;             // bytes of the file read, uploaded and split at a time (mbgc-hip --window-kib)
    static constexpr uint64_t MIN_REF_INIT_SIZE = 1 << 16;                // :47
    static constexpr int SINGLEFILE_PARALLEL_MIN_TARGETS = 4;             // :19
    static constexpr uint64_t REFERENCE_LENGTH_LIMIT = (uint64_t) UINT32_MAX << 8;   // :55
    bool isContigProperForRefExtension(uint64_t len, uint64_t unmatched, int f) const { return unmatched * f > len; }      // :179-186
    bool isContigProperForRefRCExtension(uint64_t len, uint64_t unmatched, int f) const { return unmatched * f > len; }    // :188-190
};

struct MBGC_Params : MGMP_Params {                     // mbgccoder/MBGC_Params.h (only what this path reads)
    uint8_t coderMode = 1;
    bool lazyDecompressionSupport = true;              // :38
    uint64_t rcMatchMinLength = 0;                     // :99 (55 in -m3, :61,:917-918)
    bool rcMatchMinLengthFixed = false;                // :100 (set by the reference's -r, which this tool does not have)
    bool rcRedundancyRemoval = false;                  // :101
    bool kmerLengthFixed = false;                      // :71 (-k)
    bool mismatchesWithExclusionDisabled = false;      // disableMismatchesEncodingWithExclusion, :731-738: outlives a later -m
    swsem_emit_params_t emit;
    int device = 0;
    MBGC_Params() { setCompressionMode(1); }
    void setCompressionMode(int mode);                 // :886-922
    void setKmerLength(int kmerLength) { k = kmerLength; kmerLengthFixed = true; }   // :583-591
    // :924-936, on --proteins and when the probe of the initial reference fires: k = 16 unless -k was given, mismatches coded
    // without exclusion, no reverse-complement pass over the literals; "Switching to protein profile." on stderr
    void setProteinsCompressionProfile();
};

struct Contig { std::string header, seq; };
struct ResidentCollection;                             // mbgc_decoder.h: a collection that a decode left on the device (`mbgc-hip r`)
// A round's files parsed by the device input stage (include/mbgc_fasta.h: kseq_read_lossless_fasta, MGMP.cpp:349-372):
// their contigs back to back in HBM, the layout matchRound takes.
struct RoundBatch {
    uint8_t *seqDev = nullptr; size_t seqCap = 0;      // grow-only device buffer
    bool borrowed = false;                             // seqDev is a slice of the resident source's buffer: not this batch's to free
    uint64_t bytes = 0;
    std::vector<uint64_t> offsets;                     // ncont + 1
    std::vector<uint32_t> targetOf;                    // target index of every contig
    uint32_t t0 = 0, t1 = 0;                           // targets [t0, t1)
    // single fasta file mode: the records of every element found for the batch (it may hold fewer elements than asked for),
    // and whether the file ends with it
    std::vector<uint32_t> recCounts;
    bool endOfInput = false;
    // the layout `mbgc-hip d --fasta` needs, per unit of the batch (a file of the list, an element of -i): its records' headers,
    // each followed by '\n', and the line length the parser found — copied out of the staged file bytes while they are there
    std::vector<std::string> unitHeaders;
    std::vector<uint64_t> unitLineLen;
    std::vector<uint32_t> crcs;                        // --checksums: the CRC-32 of every contig
};

class MultipleGenomeMatchingProcessor {
protected:
    MGMP_Params *params;
    SlidingWindowSparseEMMatcher *matcher = nullptr;
    std::vector<std::string> fileNames;
    uint32_t filesCount = 0, targetsCount = 0;
    int64_t processedTargetsCount = 0;
    uint64_t refG0InitPos = 0, refFinalTotalLength = 0, totalFilesLength = 0, largestContigSize = 0;
    size_t resCount = 0, unmatchedCharsAll = 0, totalMatchedAll = 0, totalDestLenAll = 0;
    std::vector<size_t> matchingLocksPos;
    std::vector<uint8_t> unmatchedFractionFactors;
    int device = 0;
    bool singleFastaFileMode = false;                                                   // MGMP.h:45
    std::vector<uint32_t> seqsCounts;                                                   // records of every target (single fasta file mode)

    const size_t PROCESSING_MATCHES_SKIPPED_DUE_TO_CONTIG_DISSIMILARITY = SIZE_MAX;     // MGMP.h:97

    void loadG0Ref(const std::string &refName);                                        // MGMP.cpp:66-150
    void loadG0RefSingleFasta();                                                        // the same in single fasta file mode (:73-76, :109-129)
    void initMatcher(const char *refStr, size_t refStrSize, size_t basicRefLength);     // :152-192
    size_t refLengthLimitFor(size_t basicRefLength, bool *bit40) const;                 // :154-168
    uint32_t windowRoundSize(uint64_t window, int gpus) const;                          // MGMP_Params::roundSize == 0
    void performMatching();                                                             // :568-606
    void processTargetsWithParallelIO();                                                // :232-313  (-t1)
    void processTargetsRounds();                                                        // :340-468 as deterministic rounds
    void verifyEmission(size_t contigs, size_t bases);                                  // --verify: the selected emission through the device decoder, exit on a contig that does not come back
    void appendHeldTargets(std::vector<std::vector<EmittedStreams>> &targets);       // streams of targets that kept a round's first pass (:382-388), in target order
    void processTargetsRoundsSharded();                                                 // the rounds with their targets sharded over the ranks of params->exchange (mgmp_sharded.cpp)
    // input stage (MGMP.cpp:7-35,349-372 on the device parser)
    mbgc_fasta_t *fasta = nullptr;
    // The files of a round in page-locked host memory, read (and inflated) by several threads. The round named as "next"
    // is read, uploaded and parsed by a thread of its own while the GPU and the host work on the current one (the
    // reference reads ahead with its IO threads too, MGMP.cpp:232-313 "WithParallelIO").
    // The thread that uploads and parses round r + 1 has the files of round r + 2 read meanwhile (two staging buffers).
    struct StagedFiles {
        uint8_t *pin = nullptr; size_t cap = 0;
        std::vector<uint64_t> fileOff;
        // --inflate device: a gzip file's place among fileOff is as long as its ISIZE trailer says and stays empty on the host; its
        // compressed bytes lie at pin[gzOff, gzOff + gzLen), behind the last file's place (gzLen 0: not such a file)
        std::vector<uint64_t> gzOff, gzLen;
        std::string error;
    } staged[2];
    struct Ahead { std::future<void> done; uint32_t f0 = 0, f1 = 0; RoundBatch *B = nullptr; bool active = false; } ahead;
    struct ReadAhead { std::future<void> done; uint32_t f0 = 0, f1 = 0; int slot = 0; bool active = false; } readAhead;
    void readFiles(StagedFiles &S, uint32_t f0, uint32_t f1);
    void startReadAhead(uint32_t f0, uint32_t f1, int slot, bool bothBuffers = false);                            // files [f0, f1) into staged[slot], on a thread of its own
    // read (unless read ahead) + upload + device parse, synchronous; [afterF0, afterF1) = the files to read meanwhile
    void prepareRound(uint32_t f0, uint32_t f1, RoundBatch &B, uint32_t afterF0 = 0, uint32_t afterF1 = 0);
    // --inflate device: the staged files [0, nf) into rawDev, the gzip ones inflated there; false: one of them did not inflate to its
    // ISIZE there, and the round's bytes are in `redo` instead, that file inflated by the host, with redoOff as their fileOff
    bool uploadAndInflate(StagedFiles &S, int nf, std::string &redo, std::vector<uint64_t> &redoOff);
    void keepHeadersFromDevice(RoundBatch &B, const uint8_t *filesDev, uint64_t n, const uint64_t *fileOff, const uint64_t *recBase, const uint64_t *lineLen, int nf);
    uint8_t *rawDev = nullptr; size_t rawCap = 0;
    uint8_t *extScratch = nullptr; size_t extScratchCap = 0;                            // extension strings that are not a span of the round's buffer
    void extensionStrings(const RoundBatch &B, const std::vector<char> &ext, const std::vector<char> &rc, uint32_t ta, uint32_t tb,
                          std::vector<const uint8_t *> &extDev, std::vector<uint64_t> &extLen);
    std::vector<mbgc_fasta_record_t> records;
    // The side files of the layout (<prefix>.names / .headers / .dnaLineLengths): the units whose matching has begun wait here, in
    // target order, until their bytes are appended to the collection's streams — the thread that appends takes them from the front.
    struct LayoutUnit { std::string name, headers; uint64_t lineLen = 0; uint32_t target = 0; };   // target: checked where it is taken
    std::deque<LayoutUnit> layoutPending;
    uint32_t layoutArrived = 0;
    bool keepsLayout() const { return !params->benchMode && !params->exchange; }         // (not under --bench, not on the sharded host)
    std::mutex layoutMu;
    // --checksums: the contigs' CRC-32s — the initial reference's, and the targets' in the order their batches are taken
    std::vector<uint32_t> g0Crcs, targetCrcs;
    void crcBatch(RoundBatch &B);                                                       // B.crcs from B.seqDev, on the input stage's stream
    std::string g0Headers; uint64_t g0LineLen = 0, hostLineLen = 0;                      // the initial reference's; hostLineLen: of parseHostBytes' last file
    void noteUnitsArrived(const RoundBatch &B, uint32_t firstFile);                     // the batch's units behind those that wait
    void noteUnitArrived(LayoutUnit &&u);
    void keepHeaders(RoundBatch &B, const uint8_t *fileBytes, const uint64_t *fileOff, const uint64_t *recBase, const uint64_t *lineLen, int nf);
    void openInputStage();
    // The resident source (`mbgc-hip r`), beside the file list and single fasta file mode: the units of a collection that
    // MBGC_Decoder::decode left packed in HBM. fileNames holds their names, and nothing is read, uploaded or parsed: a round is a
    // slice of the packed buffer. Wherever a file's size in bytes counts, the unit's text size does (ResidentUnit::text).
    const ResidentCollection *resident = nullptr;
    std::vector<uint64_t> residentUnitOff;                                              // unit u's contigs start here in the packed buffer (units + 1)
    void readG0Resident(std::vector<Contig> &out, uint64_t *fileSize);                  // the first unit, down to the host once, probed where it lies
    void prepareRoundResident(uint32_t f0, uint32_t f1, RoundBatch &B);
    void readG0(const std::string &path, std::vector<Contig> &out, uint64_t *fileSize);
    // probeG0: the file is the initial reference, and its parsed records are probed for the protein profile before they come down
    void parseHostBytes(const std::string &data, const std::string &name, std::vector<Contig> &out, bool probeG0 = false);
    void probeG0Records(uint64_t nrec);                                                 // MGMP.cpp:85-87,91-98 over records[0, nrec) of the last parseHostBytes
    // Single fasta file mode: the file travels through the two staging buffers in windows of params->singleFileWindow bytes (the
    // next one is read while this one is uploaded and split) into a device buffer that starts at an element start; what a batch
    // leaves behind its last element is moved to the front of a second buffer and the two change places. Host memory is bounded
    // by the windows (a gzip file is inflated whole, as mgmpInOpen does).
    struct SingleFile {
        int fd = -1;
        bool gz = false;
        std::string inflated, error;
        uint64_t fileSize = 0, readPos = 0;                                             // readPos: behind the last window read or being read
        uint8_t *dev = nullptr, *spare = nullptr; size_t devCap = 0, spareCap = 0;
        uint64_t devBase = 0, have = 0;                                                 // dev[0, have) = bytes [devBase, devBase + have) of the file
        uint64_t scanned = 0;                                                           // dev[0, scanned): the split's streaming pass has been over it
        uint32_t nextElem = 0;
        std::future<uint64_t> reading; int readSlot = 0; bool readActive = false;
    } sf;
    std::string sfBytes;                                                                // a batch's header lines, gathered on the device
    void sfOpen(const std::string &path);
    void sfStartRead();
    bool sfExtend();                                                                    // one more window behind dev[have); false: the file has ended
    bool sfAtEnd() const { return sf.devBase + sf.have == sf.fileSize; }
    void sfConsume(uint64_t bytes);                                                     // the buffer now starts `bytes` further on
    void sfRewind();
    void sfElements(uint32_t want, uint64_t firstMin, uint64_t nextMin, std::vector<uint64_t> &ends);   // ends of the next elements, relative to sf.dev
    std::string sfFirstRecord();
    void prepareRoundSingleFasta(uint32_t f0, uint32_t f1, RoundBatch &B);
    bool settleSingleFastaRound(RoundBatch &B);                                         // what the batch really holds -> B.t1, seqsCounts, targetsCount; false: it is empty
    // files [f0, f1) parsed into B; [nextF0, nextF1) into *nextB = what will be asked for next (prepared meanwhile)
    void loadRound(uint32_t f0, uint32_t f1, RoundBatch &B, uint32_t nextF0 = 0, uint32_t nextF1 = 0, RoundBatch *nextB = nullptr);

    // hooks, MGMP.h:79-115
    virtual void setProteinsProfile() = 0;
    virtual void initStreamsForG0Ref() = 0;
    virtual void processG0RefContig(const char *seq, size_t len) = 0;
    virtual size_t processMatches(size_t destLen, int targetIdx, size_t matchingLockPos) = 0;   // consumes the handle's last match
    virtual void processAfterSequence(uint32_t targetIdx) = 0;
    virtual void processAfterTarget(uint32_t targetIdx) = 0;
    virtual void processAfterTargetWithParallelIO(size_t matcherLoaderStartPos) = 0;
    virtual void afterTargetWithParallelIO(size_t matcherLoaderStartPos) = 0;          // the same without processAfterTarget
    virtual void initParallelProcessing() = 0;
    virtual void finalizeParallelProcessingOfTarget(uint32_t targetIdx, size_t matcherLoaderStartPos) = 0;
    // the same in two halves, for the round pipeline: what is known when the target's extension has been queued (the
    // bytes of refExtSize / locksPos, refExtLoadedPosArr), and the append of its streams once they have arrived
    virtual void noteTargetLoaded(uint32_t targetIdx, size_t matcherLoaderStartPos, size_t loadedRefLengthAfter) = 0;
    virtual void appendTargetStreams(uint32_t targetIdx) = 0;
    virtual void takeRoundStreams(uint32_t targetIdx, EmittedStreams &s) = 0;           // per-target stream append in round mode
    // the same when the round's targets arrive in target order (the round loop's collection): a contig's streams straight
    // from the handle's buffer to the collection's streams, then processAfterSequence / processAfterTarget's marks
    virtual void appendContigInOrder(const swsem_streams_t &st) = 0;
    virtual void endTargetInOrder() = 0;
    virtual const swsem_emit_params_t &emitParams() const = 0;
    virtual const std::vector<size_t> &loadedPositions() const = 0;
    virtual bool lazyMode() const = 0;

public:
    explicit MultipleGenomeMatchingProcessor(MGMP_Params *p) : params(p) {}
    // the calling thread (and the threads it starts from now on) onto the CPUs of the NUMA node the device hangs on:
    // the files travel page cache -> page-locked memory -> device, and page-locked memory is allocated next to the device
    // (MBGC_HIP_NUMA=0 leaves the threads where they are)
    static void bindHostThreadsToDeviceNode(int device);
    virtual ~MultipleGenomeMatchingProcessor();
};

class MBGC_Encoder : public MultipleGenomeMatchingProcessor {
    MBGC_Params *params;
    std::vector<size_t> refExtLoadedPosArr;                                             // MBGC_Encoder.h:48
    std::vector<EmittedStreams> targetStreams;                                          // per-target streams (round mode)
    uint32_t targetsAppended = 0;                                                       // targets whose streams arrived in order
    uint32_t sequentialTargetsDone = 0;
    // <prefix>.meta (mbgc_decoder.h): per target its sequences and where its bytes start in the six streams, taken where the bytes
    // land in the collection's streams (the three places that append a target's streams)
    std::vector<uint32_t> metaSeqCounts;
    std::vector<uint64_t> metaIndex;
    uint32_t metaContigsInTarget = 0, metaG0Contigs = 0;
    void noteStreamOffsets();
    void noteTargetAppended();
    size_t backendFed[MBGC_ST_COUNT] = {};                                              // bytes of every stream the backend has been handed

    void setProteinsProfile() override { params->setProteinsCompressionProfile(); }     // ENC.cpp:20-23
    void initStreamsForG0Ref() override;                                                // ENC.cpp:25-32
    void processG0RefContig(const char *seq, size_t len) override;                      // :34-37
    size_t processMatches(size_t destLen, int targetIdx, size_t matchingLockPos) override;      // :143-308 on the device
    void processAfterSequence(uint32_t targetIdx) override;                             // :489-491
    void processAfterTarget(uint32_t targetIdx) override;                               // :493-496
    void processAfterTargetWithParallelIO(size_t matcherLoaderStartPos) override;       // :498-509
    void afterTargetWithParallelIO(size_t matcherLoaderStartPos) override;
    void initParallelProcessing() override;                                             // :516-528
    void finalizeParallelProcessingOfTarget(uint32_t targetIdx, size_t matcherLoaderStartPos) override;   // :542-564
    void noteTargetLoaded(uint32_t targetIdx, size_t matcherLoaderStartPos, size_t loadedRefLengthAfter) override;   // :557-563
    void appendTargetStreams(uint32_t targetIdx) override;                              // :543-556
    void takeRoundStreams(uint32_t targetIdx, EmittedStreams &s) override;
    void appendContigInOrder(const swsem_streams_t &st) override;
    void endTargetInOrder() override;
    const swsem_emit_params_t &emitParams() const override { return params->emit; }
    const std::vector<size_t> &loadedPositions() const override { return refExtLoadedPosArr; }
    bool lazyMode() const override { return params->lazyDecompressionSupport; }

public:
    // the streams the reference enrols at ENC.cpp:779-787 (+ the two it writes beside them)
    std::string literals, mapOff, mapOff5thByte, mapLen, gapDeltas, gapMismatchesFlags, locksPosStream, refExtSizeStream;
    std::string rcMapOff, rcMapLen;                                                     // ENC.cpp:636-638 (-m3)
    // the layout beside the streams, for `mbgc-hip d --fasta`: a name per unit ('\n' each; G0's file first — under -t1 the first file
    // is G0's and target 0's, and stands twice; -i: the one path), a header per contig ('\n' each), a u64 line length per unit.
    // Empty on the sharded host and under --bench.
    std::string namesStream, headersStream, lineLengthsStream;
    size_t extensionsMatchedCharsAll = 0, extensionsMismatchesAll = 0, removedGapBreakingMatchesAll = 0;

    explicit MBGC_Encoder(MBGC_Params *p) : MultipleGenomeMatchingProcessor(p), params(p) { device = p->device; }
    void encode(const std::vector<std::string> &files);                                 // :759-807 up to performMatching()
    // the same over a resident collection: its units are the files, in order; the encoder's input stage is the collection's from
    // here on (and is destroyed with the encoder), the packed buffer stays the caller's
    void encodeResident(const ResidentCollection &collection);
    // prepareAndCompressStreams' collective section (:641-710) for the streams this path produces — the file-name / header /
    // line-length streams belong to the part of the tool that is not rebuilt here and go in empty (eight zero bytes each) —
    // with the caller's leaf coders; what CompressionJob::writeCompressedCollectiveParallel would write for them
    // threads: the job pool of this call; numberOfThreads: what the reference's -t would be (it only decides LZMA's numThreads; 0: = threads).
    // The header-side streams (names, sequence counts, header templates, headers, line lengths) are the CLI's and go in empty:
    // the section is what the reference's reader takes for the matcher-side streams, not a complete archive. (Their facts are
    // kept beside the streams in plain form — namesStream, headersStream, lineLengthsStream below; INTEGRATION.md §11 maps them.)
    std::string compressStreams(mbgc_leaf_compress_fn leaf, void *ctx, int threads, int blocksScale = 1, int numberOfThreads = 0);
    // The backend beside the matching (include/mbgc_backend.h, the incremental form): set before encode(), the encoder hands
    // over what its streams have grown by every few targets, so that the blocks of the split streams are coded while the rounds
    // go on; finishBackendStream() hands over the rest and returns the section. The literals wait for the end under -m3 (the
    // reverse-complement pass rewrites them, ENC.cpp:636-638).
    mbgc_backend_stream_t *backendStream = nullptr;
    // called once the initial reference is loaded: the profile (k, exclusion, the RC pass) is decided by then, and a backend that
    // runs beside the matching is opened here, with the coders of the parameters as they now stand
    std::function<void()> afterG0Loaded;
    void feedBackendStream(bool everything);
    std::string finishBackendStream(uint64_t *blocksCodedEarly);
    void backendParams(mbgc_backend_params_t &bp, int blocksScale, int numberOfThreads) const;
    std::string metaBytes() const;                                                      // what `mbgc-hip d` needs beyond the streams
    bool singleFastaFile() const { return singleFastaFileMode; }
    uint32_t singleFastaElements() const { return params->sequentialMatching ? 1 : targetsCount + 1; }
    const std::vector<uint32_t> &sequenceCounts() const { return seqsCounts; }
    size_t exactMatches() const { return resCount; }
    // --checksums: per contig in the order of an unselected `mbgc-hip d` (under -t1 the initial reference is target 0's first contig again)
    std::vector<uint32_t> contigChecksums() const {
        std::vector<uint32_t> out;
        if (!params->sequentialMatching) out = g0Crcs;
        out.insert(out.end(), targetCrcs.begin(), targetCrcs.end());
        return out;
    }
    size_t finalReferenceLength() const { return refFinalTotalLength; }          // writeStats' refFinalTotalLength, ENC.cpp:734-743
    size_t droppedExtensionBytes() const { return matcher ? matcher->getDroppedBytes() : 0; }
    size_t maxReferenceLength() const { return matcher ? matcher->getMaxRefLength() : 0; }
    size_t unmatchedChars() const { return unmatchedCharsAll; }
};
