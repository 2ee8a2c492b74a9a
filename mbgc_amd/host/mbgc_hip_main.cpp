// mbgc-hip: the compress hot path of `mbgc c` (file list -> match/literal byte streams) on one MI355X,
// driven by the C++ host classes that keep the reference's names. The streams are written raw, one file
// per stream, exactly what the reference's developer build dumps with `mbgc-dev v -D` (main.cpp:575-577;
// stream order of MBGC_Decoder.cpp:1085-1112): literals(13) locksPos(14) gapDelta(15) flags(16)
// mapOff(17) mapLen(18) refExtSize(19). Entropy coding (PPMd/LZMA) is the unchanged host backend of the
// reference and is not part of this tool.
//
// --gpus N: one process per GPU, forked here BEFORE anything touches a GPU; a round then holds -R targets per GPU, the
// replicas exchange the round's reference extensions and their verdicts over RCCL (include/mbgc_exchange.h) and rank 0
// takes the streams and writes them. Results equal -R (N x R) on one GPU. --exchange hostmem puts every rank on device
// -d and moves the bytes through host shared memory: a rehearsal of the protocol on a one-GPU box, not a speed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <atomic>
#include <thread>
#include <dlfcn.h>
#include <time.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include "mgmp_driver.h"
#include "mbgc_decoder.h"
#include "mbgc_checksums.h"

// what the ranks share before their exchange exists: the RCCL ids rank 0 makes, then (host-memory transport) its mapping
struct Bootstrap {
    std::atomic<uint32_t> idsReady, failed;
    uint32_t pad[14];
    uint8_t ids[2 * MBGC_XCHG_ID_BYTES];
};
// A rank that gives up (the reference's way: message + exit(EXIT_FAILURE)) must not leave the others waiting inside a
// collective: it raises the flag on its way out, the others watch it.
static Bootstrap *g_boot = nullptr;
static std::atomic<bool> g_done{false};
static void raiseFailure() { if (g_boot && !g_done.load()) g_boot->failed.store(1); }
// Cooperative only as far as it goes: a rank killed by a signal (a fault, the OOM killer) raises nothing. Rank 0 therefore polls
// its children (waitpid WNOHANG) and raises the flag for any that ended abnormally; the children watch their parent.
static void watchOtherRanks(const std::vector<pid_t> *children, pid_t parent) {
    std::thread([children, parent] {
        while (!g_boot->failed.load()) {
            usleep(50000);
            if (children)
                for (pid_t pid : *children) {
                    siginfo_t info;
                    info.si_pid = 0;                                             // (peek: finish() still reaps the child)
                    if (waitid(P_PID, (id_t) pid, &info, WEXITED | WNOHANG | WNOWAIT) == 0 && info.si_pid == pid &&
                        !(info.si_code == CLD_EXITED && info.si_status == 0) && !g_done.load())
                        g_boot->failed.store(1);
                }
            else if (parent && getppid() != parent) g_boot->failed.store(1);       // (rank 0 is gone)
        }
        if (!g_done.load()) { fprintf(stderr, "mbgc-hip: another rank failed\n"); _exit(EXIT_FAILURE); }
    }).detach();
}

static void dump(const std::string &prefix, const char *name, const std::string &data) {
    std::ofstream f(prefix + "." + name, std::ios::binary | std::ios::trunc);
    f.write(data.data(), (std::streamsize) data.size());
}

// the stream set of a finished encode under `prefix`: the seven streams (rcMapOff / rcMapLen beside them under -m 3), .meta, and —
// unless the rounds were sharded over several GPUs — .names, .headers and .dnaLineLengths (what `c` and `r` write)
static void writeStreamSet(const std::string &prefix, const MBGC_Encoder &enc, const MBGC_Params &params) {
    dump(prefix, "literals", enc.literals);
    if (params.rcRedundancyRemoval) { dump(prefix, "rcMapOff", enc.rcMapOff); dump(prefix, "rcMapLen", enc.rcMapLen); }
    dump(prefix, "locksPos", enc.locksPosStream);
    dump(prefix, "gapDelta", enc.gapDeltas);
    dump(prefix, "flags", enc.gapMismatchesFlags);
    dump(prefix, "mapOff", enc.mapOff);
    dump(prefix, "mapOff5th", enc.mapOff5thByte);
    dump(prefix, "mapLen", enc.mapLen);
    dump(prefix, "refExtSize", enc.refExtSizeStream);
    dump(prefix, "meta", enc.metaBytes());                                      // what `mbgc-hip d` needs beyond the streams
    if (!params.exchange) {                                                     // ... and `d --fasta` beyond that: names, headers, line lengths
        dump(prefix, "names", enc.namesStream);
        dump(prefix, "headers", enc.headersStream);
        dump(prefix, "dnaLineLengths", enc.lineLengthsStream);
    }
    if (params.checksums) {                                                     // --checksums: the manifest `mbgc-hip t` / `d --check` hold the set against
        mbgc_checksums::Manifest m;
        const std::string meta = enc.metaBytes();
        const std::string *side[4] = {&meta, &enc.namesStream, &enc.headersStream, &enc.lineLengthsStream};
        for (int k = 0; k < 4; k++) m.side[k] = mbgc_checksums::crc32(side[k]->data(), side[k]->size());
        m.contigs = enc.contigChecksums();
        dump(prefix, "checksums", m.serialize());
    }
}

static const char *REPACK_USAGE =
    "       mbgc-hip r [--select pattern]... [--select-list file] [--restore-rc] [--serial] [--no-index] [-m mode] [-k kmerLength] [-s samplingStep] [-t1]\n"
    "                  [-R targetsPerRound] [-U] [--proteins] [-l basesPerRow] [--verify | --verify-every K] [--ref-factor F] [-d device] [--bench]\n"
    "                  [--checksums] <inStreamsPrefix> <outputPrefix>\n"
    "  repacks the chosen files of a stream set (all of them without --select) into a new one, on the device: they are decoded as mbgc-hip d\n"
    "  decodes them (--select, --select-list, --restore-rc, --serial, --no-index: as there), packed back to back in HBM and matched again from\n"
    "  scratch as mbgc-hip c matches the files d --fasta would write (-m, -k, -s, -t1, -R, -U, --proteins, --verify, --ref-factor: as there, with\n"
    "  c's defaults, not the input set's values). No base leaves the device in between, no FASTA text is made. <outputPrefix> receives what c\n"
    "  writes; <outputPrefix>.names keeps the files' names of <inStreamsPrefix>.names. -l N: every file's line length becomes N (0: unlimited).\n"
    "  The chosen bases and the matcher's reference are resident together: the collection is not streamed through in pieces, and a device\n"
    "  allocation that fails ends the run with its message. A single-FASTA stream set (c -i) is refused; --gpus, -i, --lossy, --inflate and\n"
    "  --backend are options of c, over files. --bench: one JSON line (units, contigs decoded and chosen, bases, decode_ms, pack_kernel_ms,\n"
    "  pack_bytes, encode_s) behind the report\n"
    "  --checksums: also <outputPrefix>.checksums, as mbgc-hip c --checksums writes it — the contigs' CRC-32s are taken from the packed bases\n"
    "  in HBM; mbgc-hip t <outputPrefix> then checks the new set without the old one (--bench gains crc_kernel_ms, crc_bytes)\n";

// `mbgc-hip r`: MBGC_Decoder::decode that ends resident, then MBGC_Encoder::encodeResident over what it left
static int repackMain(int argc, char **argv) {
    MBGC_Params params;
    MBGC_Decoder::Options dopt;
    ResidentCollection coll;
    std::vector<std::string> pos;
    bool selectAsked = false, bench = false;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (const int r = mbgc_hip_decode_option('r', argc, argv, i, dopt, selectAsked)) { if (r < 0) return EXIT_FAILURE; }   // (-d: the device of both halves)
        else if (a == "-t1") params.sequentialMatching = true;
        else if (a == "-m" && i + 1 < argc) params.setCompressionMode(atoi(argv[++i]));
        else if (a == "-R" && i + 1 < argc) params.roundSize = atoi(argv[++i]);
        else if (a == "-s" && i + 1 < argc) {
            params.k1 = atoi(argv[++i]);
            if (params.k1 <= 0) { fprintf(stderr, "s - reference sampling step - should be a positive integer.\n\n"); return EXIT_FAILURE; }
        }
        else if (a == "-k" && i + 1 < argc) {
            params.setKmerLength(atoi(argv[++i]));
            if (params.k < 16 || params.k > 40) { fprintf(stderr, "k - matching kmer length - should be an integer between 16 and 40.\n\n"); return EXIT_FAILURE; }
        }
        else if (a == "-U") params.uppercaseDNA = true;
        else if (a == "--proteins") params.setProteinsCompressionProfile();
        else if (a == "-l" && i + 1 < argc) {
            const long long n = atoll(argv[++i]);
            if (n < 0) { fprintf(stderr, "l - bases per row - should be a non-negative integer (0: unlimited).\n\n"); return EXIT_FAILURE; }
            coll.lineLenGiven = true; coll.lineLen = (uint64_t) n;
        }
        else if (a == "--verify-every" && i + 1 < argc) { params.verifyEmissions = true; params.verifyEvery = atoi(argv[++i]); }
        else if (a == "--verify") params.verifyEmissions = true;
        else if (a == "--ref-factor" && i + 1 < argc) params.referenceFactor = atoi(argv[++i]);
        else if (a == "--bench") bench = true;
        else if (a == "--checksums") params.checksums = true;
        else if (a == "--gpus" || a == "-i" || a == "--lossy" || a == "--lossy-file" || a == "--inflate" || a == "--backend") {
            fprintf(stderr, "mbgc-hip r: %s is an option of mbgc-hip c, over files: r takes its input from a stream set, on one GPU, and writes raw streams\n", a.c_str());
            return EXIT_FAILURE;
        }
        else pos.push_back(a);
    }
    if (pos.size() != 2) { fprintf(stderr, "usage:\n%s", REPACK_USAGE); return EXIT_FAILURE; }
    if (pos[0] == pos[1]) { fprintf(stderr, "mbgc-hip r: the output prefix is the input prefix (%s): the input set would be overwritten while it is the only copy\n", pos[0].c_str()); return EXIT_FAILURE; }
    if (dopt.selectSeqAsked) {
        fprintf(stderr, "mbgc-hip r: --select-seq / --select-seq-list select records, and files that hold only some of their records are not repacked (an option of mbgc-hip d)\n");
        return EXIT_FAILURE;
    }
    if (dopt.regionAsked) {
        fprintf(stderr, "mbgc-hip r: --region / --region-list select parts of records, and files that hold only parts of their records are not repacked (an option of mbgc-hip d)\n");
        return EXIT_FAILURE;
    }
    if (!mbgc_hip_check_selection('r', dopt, selectAsked)) return EXIT_FAILURE;
    params.device = dopt.device;
    MultipleGenomeMatchingProcessor::bindHostThreadsToDeviceNode(params.device);
    if (mbgc_fasta_create(&coll.fasta, params.device)) { fprintf(stderr, "mbgc-hip r: input stage: %s\n", mbgc_fasta_last_error()); return EXIT_FAILURE; }
    coll.packFlags = params.uppercaseDNA ? MBGC_FASTA_UPPERCASE : 0u;
    dopt.resident = &coll;
    std::string error;
    if (MBGC_Decoder::decode(pos[0], std::string(), dopt, &error) != 0) {      // (its handle — streams, reference buffer, sequences — is gone when it returns)
        fprintf(stderr, "mbgc-hip r: %s\n", error.c_str());
        if (coll.packedDev) mbgc_fasta_dev_free(coll.fasta, coll.packedDev);
        mbgc_fasta_destroy(coll.fasta);
        return EXIT_FAILURE;
    }
    uint64_t contigs = 0;
    for (const ResidentUnit &u : coll.units) contigs += u.contigLen.size();
    printf("repacking %zu files: %llu contigs, %llu bases resident (%llu contigs decoded)\n", coll.units.size(), (unsigned long long) contigs,
           (unsigned long long) coll.packedBytes, (unsigned long long) coll.contigsDecoded);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int rc = EXIT_SUCCESS;
    {
        MBGC_Encoder enc(&params);                                               // (takes the input stage over and destroys it)
        enc.encodeResident(coll);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        writeStreamSet(pos[1], enc, params);
        if (params.verifyEmissions) {
            printf("verified on the device: %llu contigs, %llu bases decoded back to their bytes\n",
                   (unsigned long long) params.verifiedContigs, (unsigned long long) params.verifiedBases);
            if (params.verifiedContigs == 0 && coll.units.size() > 1) { fprintf(stderr, "--verify was asked for and no emission was verified\n"); rc = EXIT_FAILURE; }
        }
        if (!params.sequentialMatching)
            printf("rounds of %d targets; reference extension bytes dropped at the sliding window's end: %zu\n", params.roundSize, enc.droppedExtensionBytes());
        printf("final reference length: %zu\n", enc.finalReferenceLength());
        printf("exact matches total: %zu\n", enc.exactMatches());
        printf("final unmatched chars: %zu\n", enc.unmatchedChars() - enc.extensionsMatchedCharsAll);
        if (bench)
            printf("{\"metric\": \"repack (decode resident, pack, encode)\", \"units\": %zu, \"contigs_decoded\": %llu, \"contigs_chosen\": %llu, \"bases\": %llu, "
                   "\"decode_ms\": %.3f, \"pack_kernel_ms\": %.3f, \"pack_bytes\": %llu, \"pack_gb_per_s\": %.3f, \"encode_s\": %.6f}\n",
                   coll.units.size(), (unsigned long long) coll.contigsDecoded, (unsigned long long) coll.contigsChosen, (unsigned long long) coll.packedBytes,
                   coll.decodeMs, coll.packKernelMs, (unsigned long long) coll.packedBytes,
                   coll.packKernelMs > 0 ? coll.packedBytes / (coll.packKernelMs * 1e-3) / 1e9 : 0.0, (t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) * 1e-9);
        if (bench && params.checksums) printf("{\"crc_kernel_ms\": %.3f, \"crc_bytes\": %llu}\n", params.crcKernelMs, (unsigned long long) params.crcBytes);
        mbgc_fasta_dev_free(coll.fasta, coll.packedDev);
    }
    return rc;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "r") return repackMain(argc, argv);                 // chosen files of a stream set into a new one, resident in between
    if (argc > 1 && std::string(argv[1]) == "d") return mbgc_hip_decompress_main(argc, argv);   // the streams back to the collection (mbgc_decoder.cpp)
    if (argc > 1 && std::string(argv[1]) == "v") return mbgc_hip_validate_main(argc, argv);     // ... and compared with the files on disk, on the device
    if (argc > 1 && std::string(argv[1]) == "t") return mbgc_hip_test_main(argc, argv);         // ... or held against <prefix>.checksums, nothing written
    if (argc > 1 && std::string(argv[1]) == "f") return mbgc_hip_find_main(argc, argv);         // ... or searched for query sequences where it lies
    if (argc > 1 && std::string(argv[1]) == "s") return mbgc_hip_stats_main(argc, argv);        // ... or described: composition, N50, runs of N and lower case
    if (argc > 1 && std::string(argv[1]) == "k") return mbgc_hip_sketch_main(argc, argv);       // ... or compared: k-mer sketches and what every two of them share
    if (argc > 1 && std::string(argv[1]) == "u") return mbgc_hip_dups_main(argc, argv);         // ... or classed: which records are the same sequence, forward or reverse complement
    if (argc > 1 && std::string(argv[1]) == "m") return mbgc_hip_screen_main(argc, argv);       // ... or screened: which files hold the k-mers of a query, and where
    MBGC_Params params;
    std::vector<std::string> pos;
    int gpus = 1;
    std::string transport = "rccl";
    size_t shmMb = 64;
    std::string backend;                                                        // a library with the reference's leaf coders (mbgc_leaf_compress)
    int backendThreads = 8, backendBlocksScale = 1, coderThreads = 0;
    bool lossyList = false;                                                     // --lossy was given (the list's option; a single file takes --lossy-file)
    uint64_t backendOverlapBlock = 0;                                           // > 0: the backend runs beside the matching, blocks of this many bytes           // coderThreads: the reference's -t as the coders see it (0: the pool's size)
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "c") continue;
        if (a == "-t1") params.sequentialMatching = true;                        // like `mbgc c -t1` (MBGC_Params.h:867-869)
        else if (a == "-m" && i + 1 < argc) params.setCompressionMode(atoi(argv[++i]));
        else if (a == "-R" && i + 1 < argc) params.roundSize = atoi(argv[++i]);
        else if (a == "-s" && i + 1 < argc) {                                    // reference sampling step (MBGC_Params.h:593-600); an odd one: identity-encoded table entries
            params.k1 = atoi(argv[++i]);
            if (params.k1 <= 0) { fprintf(stderr, "s - reference sampling step - should be a positive integer.\n\n"); return EXIT_FAILURE; }
        }
        else if (a == "-k" && i + 1 < argc) {                                    // matching k-mer length (MBGC_Params.h:583-591): the matcher's L, matchTexts' minimal length, .meta's k
            params.setKmerLength(atoi(argv[++i]));                                // (fixed: the protein profile then leaves it alone)
            if (params.k < 16 || params.k > 40) { fprintf(stderr, "k - matching kmer length - should be an integer between 16 and 40.\n\n"); return EXIT_FAILURE; }
        }
        else if (a == "-i" && i + 1 < argc) params.inputFileName = argv[++i];      // single fasta file mode (MBGC_Params.h:793-803)
        else if (a == "--lossy-file" && i + 1 < argc) { params.inputFileName = argv[++i]; params.allowLossyParsing = true; }   // the reference's -L -i <fastaFile>
        else if (a == "--window-kib" && i + 1 < argc) params.singleFileWindow = (uint64_t) atoll(argv[++i]) << 10;
        else if (a == "-d" && i + 1 < argc) params.device = atoi(argv[++i]);
        else if (a == "-L") params.lazyDecompressionSupport = false;             // disable lazy decompression support
        else if (a == "-U") params.uppercaseDNA = true;                          // MBGC_Params.h: converts bases to uppercase
        else if (a == "--proteins") params.setProteinsCompressionProfile();       // the reference's developer option -P (main.cpp:332-334); where it stands among the options matters as it does there
        else if (a == "--lossy") params.allowLossyParsing = lossyList = true;                 // the reference's -L (MGMP_Params.h:213): ragged lines, CRLF, leading junk are read, not refused
        else if (a == "--inflate" && i + 1 < argc) {                             // where the gzip files of a list are inflated
            const std::string w = argv[++i];
            if (w != "host" && w != "device") { fprintf(stderr, "--inflate takes host or device\n"); return EXIT_FAILURE; }
            params.inflateOnDevice = w == "device";
        }
        else if (a == "--checksums") params.checksums = true;                     // <outputPrefix>.checksums: the CRC-32 of every contig's bases, taken on the device
        else if (a == "--bench") params.benchMode = true;                        // rounds timed with every contig resident in HBM (no streams written)
        else if (a == "--verify-every" && i + 1 < argc) { params.verifyEmissions = true; params.verifyEvery = atoi(argv[++i]); }
        else if (a == "--verify") params.verifyEmissions = true;                  // every emission decoded again on the device before the reference moves on
        else if (a == "--warmup" && i + 1 < argc) params.benchWarmup = atoi(argv[++i]);
        else if (a == "--gpus" && i + 1 < argc) gpus = atoi(argv[++i]);
        else if (a == "--exchange" && i + 1 < argc) transport = argv[++i];
        else if (a == "--shm-mb" && i + 1 < argc) shmMb = (size_t) atol(argv[++i]);
        else if (a == "--ref-factor" && i + 1 < argc) params.referenceFactor = atoi(argv[++i]);   // MGMP_Params.h:205 (tests: a buffer small enough to wrap)
        else if (a == "--backend" && i + 1 < argc) backend = argv[++i];
        else if (a == "--backend-threads" && i + 1 < argc) backendThreads = atoi(argv[++i]);
        else if (a == "--backend-blocks" && i + 1 < argc) backendBlocksScale = atoi(argv[++i]);
        else if (a == "--backend-overlap" && i + 1 < argc) backendOverlapBlock = (uint64_t) atoll(argv[++i]) << 20;
        else if (a == "--coder-threads" && i + 1 < argc) coderThreads = atoi(argv[++i]);
        else pos.push_back(a);
    }
    const bool single = !params.inputFileName.empty();
    if (single && pos.size() == 1) pos.insert(pos.begin(), std::string());      // (no list file in this mode)
    if (pos.size() != 2 || (single && !pos[0].empty())) {
        fprintf(stderr, "usage: mbgc-hip c [-t1] [-m mode] [-k kmerLength] [-s samplingStep] [-R targetsPerRound] [-d device] [-U] [--proteins] [--lossy] [--inflate host|device] [--verify | --verify-every K] [--ref-factor F] [--checksums] [--bench [--warmup rounds]] "
                        "[--gpus N [--exchange rccl|hostmem] [--shm-mb M]] [--backend coders.so [--backend-threads T] [--backend-blocks K | --backend-overlap MiB] [--coder-threads t]] <sequencesListFile> <outputPrefix>\n"
                        "       mbgc-hip c -i <fastaFile> | --lossy-file <fastaFile> [--window-kib K] [the options above, without --gpus and --lossy] <outputPrefix>\n"
                        "  -i: the collection is one multi-FASTA file (single fasta file mode): it is cut into the initial reference and targets of at least\n"
                        "  2 MiB at '>' bytes, on the device, while it travels to the GPU in windows of K KiB (default 32768; host memory is bounded by two\n"
                        "  windows, except for a gzip file, which is inflated on the host and held whole in memory); also prints `single-file elements: <n>`\n"
                        "  and writes <outputPrefix>.seqCounts (one little-endian u32 per target: its records)\n"
                        "  --proteins: the protein profile (the reference's developer option -P): k = 16 unless -k is given, mismatches coded without\n"
                        "  exclusion, no reverse-complement pass under -m 3. Without the option the first 65536 bases of the initial reference are probed on\n"
                        "  the device, as `mbgc c` probes them: record by record, the profile is switched (\"Switching to protein profile.\") at the first\n"
                        "  record behind which at least 256 bases have been seen, k is not 16 and (symbols so far outside acgtuACGTUN) * 100 / (the record's\n"
                        "  probed length) > 10; -t1 / -m 3 take only the first record's verdict. An empty record is skipped (the reference divides by zero)\n"
                        "  --lossy: the files of the list are read as `mbgc c -L` reads them (any line lengths, empty lines, CRLF, bytes in front of the first\n"
                        "  '>'; the longest line becomes the file's line length); FASTQ files are refused; not with -i\n"
                        "  --lossy-file <fastaFile>: -i <fastaFile> read by that rule (the reference's `mbgc c -L -i`): every element is read so, as a file\n"
                        "  of its own, and keeps its own longest line; under -t1 / -m 3 and for a small file the file is one stream, cut into batches on\n"
                        "  the device at lines that start with '>' or '@', and its longest line is the file's\n"
                        "  --inflate device: the gzip files of the list are uploaded compressed and inflated on the device, one wave per file, with their\n"
                        "  CRC-32 and length checked there; a file that does not inflate to the length its trailer states there (several members, a corrupt\n"
                        "  stream) is inflated by the host. The streams are the same either way. host (the default): zlib on the reader threads. The first\n"
                        "  file of the list and a gzip file given with -i are always inflated by the host\n"
                        "  --checksums: also writes <outputPrefix>.checksums — the CRC-32 of every contig's bases as the streams hold them (after -U, after the\n"
                        "  lossy rule), taken on the device where the input stage leaves the contigs, and of .meta / .names / .headers / .dnaLineLengths;\n"
                        "  mbgc-hip t <outputPrefix> and d --check hold the set against it without the FASTA files. One GPU, not with --bench\n"
                        "  --backend writes <outputPrefix>.collective: the collective section of the matcher-side streams (the header-side streams are the CLI's and\n"
                        "  go in empty); --coder-threads = the reference's -t as its coders see it (LZMA runs two threads when it is > 1)\n");
        fprintf(stderr, "       %s       %s       %s       %s       %s       %s       %s       %s%s       %s", MBGC_HIP_D_USAGE, MBGC_HIP_T_USAGE, MBGC_HIP_V_USAGE, MBGC_HIP_F_USAGE, MBGC_HIP_F_IUPAC_USAGE,
                MBGC_HIP_S_USAGE, MBGC_HIP_K_USAGE, MBGC_HIP_U_USAGE, REPACK_USAGE, MBGC_HIP_M_USAGE);
        return EXIT_FAILURE;
    }
    if (gpus < 1 || (transport != "rccl" && transport != "hostmem") || (gpus > 1 && params.sequentialMatching)) {
        fprintf(stderr, "--gpus needs a positive count, --exchange rccl or hostmem, and the round mode (not -t1 / -m 3: those match sequentially)\n");
        return EXIT_FAILURE;
    }
    if (single && (gpus > 1 || transport == "hostmem")) {
        fprintf(stderr, "-i (single fasta file mode) runs on one GPU: the rounds sharded over --gpus N take a file list\n");
        return EXIT_FAILURE;
    }
    if (single && lossyList) {
        fprintf(stderr, "--lossy reads the files of a list and is not taken with -i: a single fasta file is read by the lossy rule when it is given as --lossy-file <fastaFile> (the reference's -L -i)\n");
        return EXIT_FAILURE;
    }
    if (params.checksums && (gpus > 1 || transport == "hostmem")) {
        fprintf(stderr, "--checksums runs on one GPU: the rounds sharded over --gpus N / --exchange hostmem write no .names / .headers, and their contigs live on several ranks\n");
        return EXIT_FAILURE;
    }
    if (params.checksums && params.benchMode) {
        fprintf(stderr, "--checksums is not taken with --bench: c --bench writes no stream set, so there is nothing a manifest would describe\n");
        return EXIT_FAILURE;
    }
    if (gpus > 1 && params.verifyEmissions) {
        // (the sharded round loop has no verification step: every rank would have to decode its own emissions before the round's
        // finalize — accepted silently before, the run then ended with "verified on the device: 0 contigs" and exit code 0)
        fprintf(stderr, "--verify / --verify-every check the emissions of the one-GPU schedules; with --gpus N verify a single-GPU run of the same rounds (-R N x r writes the same streams)\n");
        return EXIT_FAILURE;
    }
    std::vector<std::string> files;
    if (!single) {
        std::ifstream lst(pos[0]);
        if (!lst) { fprintf(stderr, "cannot open sequences list file %s\n", pos[0].c_str()); return EXIT_FAILURE; }
        std::string line;
        while (std::getline(lst, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty()) files.push_back(line);
        }
    }
    // ---- the ranks: forked before the first GPU call; the parent is rank 0 and reports for all
    int rank = 0;
    std::vector<pid_t> children;
    Bootstrap *boot = nullptr;
    size_t sharedBytes = 0;
    const bool explicitExchange = gpus > 1 || transport == "hostmem";
    if (explicitExchange || getenv("MBGC_HIP_EXCHANGE")) {
        sharedBytes = sizeof(Bootstrap) + (transport == "hostmem" ? std::max<size_t>(shmMb << 20, mbgc_xchg_hostmem_min_bytes(gpus))
                                                                   : std::max<size_t>(1 << 20, mbgc_xchg_hostmem_min_bytes(gpus)));   // rccl: the hosts' control exchanges
        void *m = mmap(nullptr, sharedBytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);      // (zero-filled)
        if (m == MAP_FAILED) { perror("mmap"); return EXIT_FAILURE; }
        boot = g_boot = (Bootstrap *) m;
        atexit(raiseFailure);
        fflush(stdout); fflush(stderr);
        const pid_t parent = getpid();
        for (int r = 1; r < gpus; r++) {
            const pid_t pid = fork();
            if (pid < 0) { perror("fork"); return EXIT_FAILURE; }
            if (pid == 0) { rank = r; children.clear(); break; }
            children.push_back(pid);
        }
        static std::vector<pid_t> watched;                                      // (outlives main's frame for the detached watcher)
        watched = children;
        watchOtherRanks(rank == 0 ? &watched : nullptr, rank == 0 ? 0 : parent);
        if (transport == "rccl") {
            params.device = rank;                                                // one rank per GPU
            if (rank == 0) {
                if (mbgc_xchg_unique_ids(boot->ids)) { fprintf(stderr, "exchange: %s\n", mbgc_xchg_last_error()); return EXIT_FAILURE; }
                boot->idsReady.store(1);
            } else {
                while (!boot->idsReady.load() && !boot->failed.load()) usleep(1000);
            }
            if (mbgc_xchg_create_rccl(&params.exchange, boot->ids, rank, gpus, params.device) ||
                mbgc_xchg_set_host_control(params.exchange, (uint8_t *) m + sizeof(Bootstrap), sharedBytes - sizeof(Bootstrap))) {
                fprintf(stderr, "exchange (rank %d): %s\n", rank, mbgc_xchg_last_error());
                return EXIT_FAILURE;
            }
        } else if (mbgc_xchg_create_hostmem(&params.exchange, (uint8_t *) m + sizeof(Bootstrap), sharedBytes - sizeof(Bootstrap), rank, gpus, params.device)) {
            fprintf(stderr, "exchange (rank %d): %s\n", rank, mbgc_xchg_last_error());
            return EXIT_FAILURE;
        }
    }
    auto finish = [&](int rc) {
        g_done.store(rc == 0);
        if (params.exchange) { mbgc_xchg_destroy(params.exchange); params.exchange = nullptr; }
        if (rank != 0) { fflush(stdout); fflush(stderr); _exit(rc); }
        for (pid_t pid : children) {
            int st = 0;
            if (waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) rc = rc ? rc : EXIT_FAILURE;
        }
        return rc;
    };
    MultipleGenomeMatchingProcessor::bindHostThreadsToDeviceNode(params.device);
    MBGC_Encoder enc(&params);
    mbgc_leaf_compress_fn leaf = nullptr;
    if (!backend.empty() && rank == 0 && !params.benchMode) {
        // the reference's unchanged PPMd7 / LZMA: a library whose symbol mbgc_leaf_compress has the callback's signature
        void *lib = dlopen(backend.c_str(), RTLD_NOW | RTLD_LOCAL);
        leaf = lib ? (mbgc_leaf_compress_fn) dlsym(lib, "mbgc_leaf_compress") : nullptr;
        if (!leaf) { fprintf(stderr, "cannot load the leaf coders from %s: %s\n", backend.c_str(), dlerror()); return finish(EXIT_FAILURE); }
        if (backendOverlapBlock)
            enc.afterG0Loaded = [&] {                                            // (the probe of the initial reference may have changed k and the exclusion flag: the coders follow them)
                mbgc_backend_params_t bp;
                enc.backendParams(bp, 1, coderThreads > 0 ? coderThreads : backendThreads);
                enc.backendStream = mbgc_backend_stream_open(&bp, leaf, nullptr, backendThreads, backendOverlapBlock);
                if (!enc.backendStream) { fprintf(stderr, "%s\n", mbgc_backend_last_error()); exit(EXIT_FAILURE); }
            };
    }
    struct timespec tEnc0, tEnc1;
    clock_gettime(CLOCK_MONOTONIC, &tEnc0);
    enc.encode(files);
    clock_gettime(CLOCK_MONOTONIC, &tEnc1);
    if (rank != 0) return finish(0);
    if (params.benchMode) {
        // the C++ host's own measurement of the hot path (BASELINE.json metric): inputs resident in HBM, rounds of -R targets
        printf("{\"metric\": \"input Gbases/s (compress hot path, C++ host)\", \"value\": %.4f, \"unit\": \"Gbases/s\", \"rounds\": %d, "
               "\"warmup_rounds\": %d, \"targets_per_round\": %d, \"bases\": %llu, \"seconds\": %.6f, \"ms_per_round\": %.4f, "
               "\"n_gpus\": %d, \"exchange\": \"%s\", \"rounds_finalized_on_device_verdicts\": %d, \"extension_bytes_dropped\": %zu, "
               "\"max_ref_len\": %zu}\n",
               params.benchBases / params.benchSeconds / 1e9, params.benchRounds, params.benchWarmup, params.roundSize * gpus,
               (unsigned long long) params.benchBases, params.benchSeconds, params.benchSeconds * 1e3 / std::max(1, params.benchRounds),
               gpus, params.exchange ? transport.c_str() : "none", params.specRounds, enc.droppedExtensionBytes(), enc.maxReferenceLength());
        return finish(0);
    }
    writeStreamSet(pos[1], enc, params);
    if (enc.singleFastaFile()) {
        const std::vector<uint32_t> &counts = enc.sequenceCounts();
        dump(pos[1], "seqCounts", std::string((const char *) counts.data(), counts.size() * sizeof(uint32_t)));
        printf("single-file elements: %u\n", enc.singleFastaElements());
    }
    if (!backend.empty()) {
        // the streams through the backend's job table and container framing (include/mbgc_backend.h), entropy-coded by the
        // library given
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        uint64_t early = 0;
        const std::string section = enc.backendStream ? enc.finishBackendStream(&early)
                                                      : enc.compressStreams(leaf, nullptr, backendThreads, backendBlocksScale, coderThreads);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (enc.backendStream) { mbgc_backend_stream_close(enc.backendStream); enc.backendStream = nullptr; }
        dump(pos[1], "collective", section);
        const size_t raw = enc.literals.size() + enc.rcMapOff.size() + enc.rcMapLen.size() + enc.locksPosStream.size() + enc.gapDeltas.size() +
                           enc.gapMismatchesFlags.size() + enc.mapOff.size() + enc.mapOff5thByte.size() + enc.mapLen.size() + enc.refExtSizeStream.size();
        const double ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
        if (backendOverlapBlock)
            printf("backend: %zu stream bytes to %zu, %.0f ms after the matching's %.0f ms (%d threads, blocks of %llu MiB, %llu of them coded while the matching ran)\n",
                   raw, section.size(), ms, (tEnc1.tv_sec - tEnc0.tv_sec) * 1e3 + (tEnc1.tv_nsec - tEnc0.tv_nsec) * 1e-6, backendThreads,
                   (unsigned long long) (backendOverlapBlock >> 20), (unsigned long long) early);
        else
            printf("backend: %zu stream bytes to %zu in %.0f ms (%d threads, %d x the reference's blocks)\n", raw, section.size(), ms, backendThreads,
                   std::max(1, backendBlocksScale));
    }
    if (params.verifyEmissions) {
        printf("verified on the device: %llu contigs, %llu bases decoded back to their bytes\n",
               (unsigned long long) params.verifiedContigs, (unsigned long long) params.verifiedBases);
        if (params.verifiedContigs == 0 && (files.size() > 1 || single)) {    // (-i: the file is a target itself, or holds some)
            fprintf(stderr, "--verify was asked for and no emission was verified\n");
            return finish(EXIT_FAILURE);
        }
    }
    if (!params.sequentialMatching)
        printf("rounds of %d targets%s; reference extension bytes dropped at the sliding window's end: %zu\n", params.roundSize,
               gpus > 1 ? " per GPU" : "", enc.droppedExtensionBytes());
    printf("final reference length: %zu\n", enc.finalReferenceLength());
    printf("exact matches total: %zu\n", enc.exactMatches());
    printf("removed matches breaking gaps total: %zu\n", enc.removedGapBreakingMatchesAll);
    printf("swsMEM unmatched chars: %zu\n", enc.unmatchedChars());
    printf("extensions matched chars: %zu\n", enc.extensionsMatchedCharsAll);
    printf("final unmatched chars: %zu\n", enc.unmatchedChars() - enc.extensionsMatchedCharsAll);
    if (params.exchange) printf("rounds finalized on the ranks' device-side verdicts: %d\n", params.specRounds);
    if (params.exchange) printf("rounds whose extension exchange carried only the loadable head: %d\n", params.headRounds);
    return finish(0);
}
