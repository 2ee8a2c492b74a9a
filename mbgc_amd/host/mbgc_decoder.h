// `mbgc-hip d`: a collection back from the raw streams `mbgc-hip c` wrote, on the device; `mbgc-hip v`: the same, compared there
// with the FASTA files on disk (the reference's `mbgc v`, main.cpp:420-445).
//   MbgcMeta       <prefix>.meta: what a decoder needs beyond the streams (the reference CLI keeps the same facts in its
//                  archive header and header-side streams: MBGC_Decoder::readParams / readStats, MBGC_Decoder.cpp:1291-1323)
//   MBGC_Decoder   mbgccoder/MBGC_Decoder.{h,cpp}: decodeTarget (:535-634) and loadRef (:651-675) restated as a load
//                  SCHEDULE — computed from the plan's lengths and unmatched counts before a base exists — and the driver
//                  that runs plan, fills and loads through the C ABI (include/mbgc_swsem.h). No HIP headers here.
// mbgc_decoder.cpp is one translation unit: the meta, the load schedule, decode() as the list of its stages, the command lines
// and the C exports of the tests. The stages are headers it includes once:
//   mbgc_decoder_streams.h    what is on disk: StreamSet (the files held to the meta, the -m 3 restore, the chain starts),
//                             Selection (--select, --select-seq), chosenUnits (THE walk over what leaves the decoder)
//   mbgc_decoder_run.h        one pass on the device: Provenance, FillUnit / partitionUnits, DecodedCollection (the handle and
//                             all it holds: plan + schedule, the closure of --select, the forward run)
//   mbgc_decoder_fasta.h      text out of a DecodedCollection: FastaLayout, FastaPlan (units and batches, shared by `d --fasta`
//                             and `v`), FastaStage (device buffers, formatBatch), writeFastaFiles (--gzip: deflateBatch)
//   mbgc_decoder_region.h     `d --region`: the specs held to the headers and the records' lengths, the pieces as outputs
//   mbgc_decoder_validate.h   `v`: Validation (read-ahead, originals to the device, compare, verdicts, --dump)
//   mbgc_decoder_find.h       `f`: the queries and their reverse complements searched in the chosen contigs, the hits named and sorted
//   mbgc_decoder_stats.h      `s`: the chosen contigs' counters and runs of N / lower case taken on the device, summed per file, N50 / L50
//   mbgc_decoder_sketch.h     `k`: FracMinHash sketches of the chosen files or records and the pairs' shared hashes taken on the device, the distances
//   mbgc_decoder_dups.h       `u`: the chosen contigs classed on the device — same sequence, forward or reverse complement —, the duplicates and the files named
//   mbgc_decoder_screen.h     `m`: the chosen files or records screened on the device for the queries' k-mers, containment per query and group, loci
// Failures travel one way: a stage returns false and leaves its message; decode() turns that into 1.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mbgc_swsem.h"
#include "../../include/mbgc_fasta.h"

struct MbgcMeta {
    static constexpr uint32_t VERSION = 1;
    bool sequentialMatching = false, rcInReference = true, contigsIndividuallyReversed = true, uppercaseDNA = false;
    bool singleFastaFile = false, rcRedundancyRemoval = false;
    uint32_t coderMode = 1, k = 32, k1 = 16;
    uint32_t g0Contigs = 0;                              // contigs at the head of the literal stream that form the initial reference
    uint64_t maxRefLength = 0, swSize = 0, finalRefLength = 0, reachedRefLengthCount = 0;
    swsem_emit_params_t emit = {};
    struct Target { uint32_t seqsCount = 0; uint8_t unmatchedFractionFactor = 0, unmatchedFractionRCFactor = 0; };
    std::vector<Target> targets;                         // the targets after G0 (-t1: every file)
    // stream index: (targets + 1) x SWSEM_NSTREAMS byte offsets — row t: where target t starts in literals, mapOff, mapOff5th,
    // mapLen, gapDelta, flags; the last row: the streams' sizes. Empty: no index.
    std::vector<uint64_t> index;

    std::string serialize() const;
    bool parse(const std::string &bytes, std::string *error);
};

// One step of the load schedule. A copy of `length` decoded bytes that start `offset` bytes into contig `contig` (G0's loads run on
// over its contigs, which lie back to back) to reference position refPos; reverseComplement: upperReverseComplement of those
// bytes. contig == SEPARATOR: the single region separator byte; contig == FROM_REF: the source is reference position `offset`
// (the per-target reverse complement of :608-616).
struct LoadSegment {
    static constexpr int64_t SEPARATOR = -1, FROM_REF = -2;
    int64_t contig;
    uint64_t offset, length, refPos;
    bool reverseComplement;
};

// `mbgc-hip r`: what a decode that ends RESIDENT hands over instead of downloading — the chosen units (the files `d --fasta` would
// write, in its order) with their names, headers, line lengths and contig lengths, and their contigs packed back to back on the
// device (mbgc_fasta_pack_dev) in a buffer of the caller's input stage, which outlives the decoder's handle: that handle, with the
// streams, the reference buffer and the decoder's sequence buffer, is gone when decode() returns.
struct ResidentUnit {
    std::string name, headers;                           // its line of <prefix>.names; its contigs' headers, '\n' behind each
    uint64_t lineLen = 0, text = 0;                      // text: the bytes of the FASTA file `d --fasta` would write at that line length
    std::vector<uint64_t> contigLen;
};
struct ResidentCollection {
    mbgc_fasta_t *fasta = nullptr;                       // in: the input stage that allocates and packs
    uint32_t packFlags = 0;                              // in: 0 or MBGC_FASTA_UPPERCASE
    bool lineLenGiven = false; uint64_t lineLen = 0;     // in: -l N, every unit's line length becomes N
    std::vector<ResidentUnit> units;
    uint8_t *packedDev = nullptr; uint64_t packedBytes = 0;   // unit u's contigs follow unit u - 1's; mbgc_fasta_dev_free(fasta, packedDev)
    uint64_t contigsDecoded = 0, contigsChosen = 0;
    double decodeMs = 0, packKernelMs = 0;
};

class MBGC_Decoder {
public:
    struct RefState {                                    // MBGC_Decoder.h: refPos, refTotalLength, reachedRefLengthCount
        uint64_t refPos = 1;                             // REF_SHIFT
        uint64_t refTotalLength = 0;
        uint64_t reachedRefLengthCount = 0;
        bool lazyDecompressionSupport = true;
        uint64_t loaded() const { return reachedRefLengthCount * (refTotalLength - 1) + (refPos - 1); }
    };
    struct ContigInfo { uint64_t length, unmatched; };
    // gzip: --gzip, the files of --fasta are written as <name>.gz, compressed on the device (mbgc_fasta_deflate_dev)
    // fastaDir: --fasta, empty = not asked for; restoreRc: --restore-rc, the -m 3 pass over the literals is inverted first
    // select: --select / --select-list, the files to bring back (a unit is chosen when its line of <prefix>.names contains one of the
    // patterns; empty = the whole collection); closureOut: --closure-out, one byte per planned contig
    // selectSeq: --select-seq / --select-seq-list, the records to bring back (a record is chosen when its header contains one of the
    // patterns — matched on the device, mbgc_fasta_match_headers_dev — and its file passes `select`); selectSeqAsked: one of the two
    // options stood on the command line; selectSeqHost: --select-seq-host, a developer switch — the match is made again by the host,
    // find by find, timed, and held against the device's
    // --region 'PATTERN:FROM-TO': pattern, a substring of the header line as in --select-seq; from / to: 1-based, inclusive
    struct RegionSpec { std::string pattern; uint64_t from = 0, to = 0; };
    // the spec is split at its last ':'; false: *why says what is wrong with it
    static bool parseRegionSpec(const std::string &text, RegionSpec &out, std::string *why);
    struct FindQuery { std::string name, seq; };
    struct PrimerPair { std::string name, fwd, rev; };
    struct Options {
        // regions: --region / --region-list, parts of records to bring back (mbgc_decoder_region.h); regionAsked: one of the two
        // options stood on the command line; regionGranule: --region-granule, bytes per granule of the closure (a power of two; a
        // knob of the measurements)
        std::vector<RegionSpec> regions; bool regionAsked = false; uint32_t regionGranule = 256;
        bool serial = false, noIndex = false, bench = false, restoreRc = false, gzip = false; int device = 0; std::string fastaDir;
        std::vector<std::string> select; std::string closureOut;
        std::vector<std::string> selectSeq; bool selectSeqAsked = false, selectSeqHost = false;
        // `mbgc-hip v`: validate — the units are formatted as for --fasta and compared on the device with the originals named by
        // <prefix>.names, nothing is downloaded or written; root / flat: where the originals lie (--root is put before relative names,
        // --flat keeps the basename `d --fasta` writes); skipCompare: decode and format only; dumpDir: the text of the first invalid
        // files is written there; batchText: text bytes per batch, 0 = the default of --fasta
        bool validate = false, flat = false, skipCompare = false, inflateOnDevice = false; std::string root, dumpDir; uint64_t batchText = 0;
        // `mbgc-hip r`: nothing is downloaded or written; the chosen units stay on the device and are described here
        ResidentCollection *resident = nullptr;
        // `d --check` / `mbgc-hip t`: the chosen contigs' CRC-32s, taken on the device, are held against <prefix>.checksums before
        // anything is written (2 = a contig or a side file differs); writeNothing: `t`, no sequence files
        bool check = false, writeNothing = false;
        // `mbgc-hip f` (mbgc_decoder_find.h): the queries (name; bases, upper case, letters only, held to the limits by the command line) are
        // searched in the chosen contigs on the device with at most findMismatches substitutions, their reverse complements too unless
        // findForwardOnly. findHitsFile: --hits (empty: stdout); findRegionsOut / findFlank: --regions-out, --flank; findHitCapacity:
        // --hit-capacity, the first size of the hit buffer (0: sized from the bases searched); findHost: --find-host, a developer switch —
        // the search is made again by the host, timed, and held against the device's. decode() then returns 0 (a hit) or 3 (none)
        bool find = false, findForwardOnly = false, findHost = false; uint32_t findMismatches = 0; uint64_t findHitCapacity = 0, findFlank = 0;
        std::vector<FindQuery> findQueries; std::string findHitsFile, findRegionsOut;
        // findIupac: --iupac, the queries are IUPAC patterns (upper case, letters of the table, U written as T) and a letter matches the
        // bases of its set. findPrimers: --primers / --primer-file (implies findIupac); findQueries then holds pair i's FWD at 2 i and
        // its REV at 2 i + 1, and the hits are paired into products of findMinAmplicon .. findMaxAmplicon bases (--min-amplicon,
        // --max-amplicon); findAmpliconsOut: --amplicons-out. decode() then returns 0 (a product) or 3 (none)
        bool findIupac = false; std::vector<PrimerPair> findPrimers; uint64_t findMinAmplicon = 0, findMaxAmplicon = 5000; std::string findAmpliconsOut;
        // `mbgc-hip s` (mbgc_decoder_stats.h): the chosen contigs are counted on the device and nothing else happens to them.
        // statsRecordsFile: --records ("-": stdout); statsGapsOut / statsMinGap: --gaps-out, --min-gap; statsMaskedOut / statsMinMasked:
        // --masked-out, --min-masked (a minimum of 0 is read as 1); statsHost: --stats-host, a developer switch — everything is
        // computed again by the host and held against the device's
        bool stats = false, statsHost = false; uint64_t statsMinGap = 1, statsMinMasked = 1;
        std::string statsRecordsFile, statsGapsOut, statsMaskedOut;
        // `mbgc-hip k` (mbgc_decoder_sketch.h): the chosen contigs are sketched on the device and nothing else happens to them. sketchK: -k
        // (1..32); sketchScale: --scale (>= 1); sketchByRecord: a group per record, not per file; sketchNoPairs: --no-pairs; sketchMinShared:
        // --min-shared; sketchPairsOut / sketchOut / sketchOrderOut: --pairs-out, --sketches-out, --order-out; sketchHost: --sketch-host, a
        // developer switch — everything is computed again by the host and held against the device's
        bool sketch = false, sketchByRecord = false, sketchNoPairs = false, sketchHost = false; uint32_t sketchK = 21; uint64_t sketchScale = 1000, sketchMinShared = 0;
        std::string sketchPairsOut, sketchOut, sketchOrderOut;
        // `mbgc-hip u` (mbgc_decoder_dups.h): the chosen contigs are classed on the device — which are the same sequence, forward or as the
        // reverse complement — and nothing else happens to them. dupsForwardOnly: --forward-only; dupsExactCase: --exact-case; dupsMinLen:
        // --min-len (0 is read as 1); dupsClustersOut / dupsUniqueFilesOut: --clusters-out, --unique-files-out; dupsHost: --dups-host, a
        // developer switch — the classes are made again by the host and held against the device's
        bool dups = false, dupsForwardOnly = false, dupsExactCase = false, dupsHost = false; uint64_t dupsMinLen = 1;
        std::string dupsClustersOut, dupsUniqueFilesOut;
        // `mbgc-hip m` (mbgc_decoder_screen.h): the chosen contigs are screened on the device for the canonical k-mers of screenQueries
        // (name; bases — the command line has held them to the limits) and nothing else happens to them. screenK: -k (1..32);
        // screenByRecord: a group per record, not per file; screenMinShared / screenMinContainment: --min-shared, --min-containment;
        // screenLociOut / screenRegionsOut / screenFlank / screenMaxGap / screenMinLocusHits: --loci-out, --regions-out, --flank, --max-gap,
        // --min-locus-hits; screenHitCapacity: --hit-capacity, the most hit rows the loci may take (0: as many as there are); screenHost:
        // --screen-host, a developer switch — everything is computed again by the host and held against the device's. decode() then
        // returns 0 (a pair was reported) or 3 (none)
        bool screen = false, screenByRecord = false, screenHost = false; uint32_t screenK = 21; uint64_t screenMinShared = 1; double screenMinContainment = 0;
        uint64_t screenFlank = 0, screenMaxGap = 500, screenMinLocusHits = 3, screenHitCapacity = 0;
        std::vector<FindQuery> screenQueries; std::string screenLociOut, screenRegionsOut;
    };

    // MBGC_Decoder::loadRef, :651-675 (the recursion as a loop). false: the schedule cannot advance (malformed input).
    static bool loadRef(RefState &st, int64_t contig, uint64_t textOffset, uint64_t seqLength, uint64_t refLockPos, bool loadRCRef,
                        std::vector<LoadSegment> &out);
    // the loads of decodeTarget, :564-620, for a target whose first contig has number firstContig
    static bool scheduleTarget(RefState &st, uint64_t firstContig, const std::vector<ContigInfo> &contigs, uint8_t unmatchedFractionFactor,
                               uint8_t unmatchedFractionRCFactor, bool rcInReference, bool contigsIndividuallyReversed, uint64_t refLockPos,
                               std::vector<LoadSegment> &out);
    // G0 as the encoder host loaded it (MultipleGenomeMatchingProcessor::initMatcher, mgmp_driver.cpp: one loadRef of the
    // contigs back to back, then their reverse complement as one text; the window's end is 0 under -t1, the buffer's end otherwise)
    static bool scheduleG0(RefState &st, uint64_t g0Bytes, bool rcInReference, bool sequentialMatching, std::vector<LoadSegment> &out);

    // streams under streamsPrefix -> outputPrefix.{seq,contigLens,seqCounts}; the message of a failure in *error.
    // opt.fastaDir: also the input FASTA files again, under that directory, from <streamsPrefix>.names / .headers / .dnaLineLengths
    // (formatted on the device: mbgc_fasta_format_dev, include/mbgc_fasta.h)
    // opt.validate: nothing is written; 0 = every file equals its original, 2 = a file differs or is missing (reported on stdout /
    // stderr in the reference's words, MBGC_Decoder.cpp:112-183, :1194-1200), 1 = a failure as above
    static int decode(const std::string &streamsPrefix, const std::string &outputPrefix, const Options &opt, std::string *error);
};

int mbgc_hip_decompress_main(int argc, char **argv);
int mbgc_hip_validate_main(int argc, char **argv);
int mbgc_hip_test_main(int argc, char **argv);
int mbgc_hip_find_main(int argc, char **argv);
int mbgc_hip_stats_main(int argc, char **argv);
int mbgc_hip_sketch_main(int argc, char **argv);
int mbgc_hip_dups_main(int argc, char **argv);
int mbgc_hip_screen_main(int argc, char **argv);
// the usage texts of `d` and `v`, without the "usage: " (or its indent) in front of the first line
extern const char *const MBGC_HIP_D_USAGE, *const MBGC_HIP_V_USAGE, *const MBGC_HIP_T_USAGE, *const MBGC_HIP_F_USAGE, *const MBGC_HIP_S_USAGE, *const MBGC_HIP_K_USAGE,
    *const MBGC_HIP_U_USAGE, *const MBGC_HIP_F_IUPAC_USAGE, *const MBGC_HIP_M_USAGE;
// The options every command over a decode shares (`d`, `v`, `r`; tool: that letter, for the messages): --serial, --no-index,
// --restore-rc, --select, --select-list, --select-seq, --select-seq-list, --region, --region-list and -d, argv[i] on. 1: taken (i stands on its last word), 0: none of them,
// -1: refused, the message is on stderr.
int mbgc_hip_decode_option(char tool, int argc, char **argv, int &i, MBGC_Decoder::Options &opt, bool &selectAsked);
// after the command line: no empty pattern, no empty list (--select and --select-seq alike); false: the message is on stderr
bool mbgc_hip_check_selection(char tool, const MBGC_Decoder::Options &opt, bool selectAsked);
// --select-list: the file's non-empty lines behind `out`; false: it cannot be opened
bool mbgc_hip_read_pattern_list(const char *path, std::vector<std::string> &out);
