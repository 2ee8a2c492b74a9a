// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_run.h): FASTA text out of a DecodedCollection. The layout
// beside the streams (<prefix>.names / .headers / .dnaLineLengths, written by mbgc-hip c), the plan of units and batches that
// `d --fasta` and `v` share, the stage that formats a batch on the device, and the writer of `d --fasta [--gzip]`.
#pragma once

namespace {
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

uint64_t recordText(uint64_t headerLen, uint64_t seqLen, uint64_t lineLen) {
    const uint64_t line = (lineLen == 0 || lineLen > seqLen) ? seqLen : lineLen;
    return 2 + headerLen + (seqLen ? seqLen + (seqLen - 1) / line + 1 : 0);
}

// the file a unit goes to: the basename of its name (the reference's ignoreFastaFilesPath: nothing is written outside the
// directory), without a .gz suffix — the text is written inflated
std::string outputName(const std::string &name) {
    std::string b = name.substr(name.find_last_of('/') == std::string::npos ? 0 : name.find_last_of('/') + 1);
    if (b.size() >= 3 && b.compare(b.size() - 3, 3, ".gz") == 0) b.resize(b.size() - 3);
    return b;
}

// the directory, with the ones above it; false: *failed = the one that could not be made
bool makeDirs(const std::string &dir, std::string *failed) {
    for (size_t at = 1; at <= dir.size(); at++)
        if (at == dir.size() || dir[at] == '/')
            if (mkdir(dir.substr(0, at).c_str(), 0777) != 0 && errno != EEXIST) { *failed = dir.substr(0, at); return false; }
    return true;
}

// the lines of L.headers, held to the collection: one per contig
bool parseHeaders(FastaLayout &L, uint64_t contigs, std::string &msg) {
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
    return true;
}
// --select-seq without a sink that needs the whole layout: <prefix>.headers alone
bool readHeaders(const std::string &prefix, uint64_t contigs, FastaLayout &L, std::string &msg) {
    if (!readFile(prefix + ".headers", L.headers)) {
        msg = "malformed stream set: cannot open " + prefix + ".headers (--select-seq needs the headers mbgc-hip c writes beside the streams)";
        return false;
    }
    return parseHeaders(L, contigs, msg);
}

// reads and checks the three side files against the meta: false and a message, or the layout
bool readFastaLayout(const std::string &prefix, const MbgcMeta &meta, uint64_t contigs, FastaLayout &L, std::string &msg) {
    std::string names, lens;
    for (const char *ext : {"names", "headers", "dnaLineLengths"})
        if (!readFile(prefix + "." + ext, ext[0] == 'n' ? names : (ext[0] == 'h' ? L.headers : lens))) {
            msg = "malformed stream set: cannot open " + prefix + "." + ext + " (--fasta needs the names, headers and line lengths mbgc-hip c writes beside the streams)";
            return false;
        }
    const size_t T = meta.targets.size();
    if (!parseNames(names, meta, L.names, msg)) return false;
    if (!parseHeaders(L, contigs, msg)) return false;
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

// ---- the FASTA files again: the chosen units (--select-seq: their runs of chosen records) in order, in batches of
// whole units of at most FASTA_BATCH_TEXT (--batch-kib) bytes of text. `d --fasta` and `v` run over the same plan.
struct FastaPlan {
    std::vector<FastaUnit> units;
    std::vector<size_t> batchEnd;                                  // batch b: units [batchEnd[b - 1], batchEnd[b])
    uint64_t maxBatch = 0, maxGz = 0;                              // the most text of a batch; --gzip: the most a batch's gzip files take
    std::vector<char> fileWanted;                                  // per output file (--select: no other file is made, empty ones included)
    bool runs = false;                                             // --select-seq: a unit is a run of chosen records, a file may have many in a batch
};
FastaPlan planFasta(const std::vector<ChosenUnit> &chosen, const MbgcMeta &meta, const FastaLayout &layout, const std::vector<uint64_t> &contigLen,
                    uint64_t batchText, bool gzip, bool runs) {
    FastaPlan P;
    P.runs = runs;
    P.fileWanted.assign(layout.outNames.size(), 0);
    for (const ChosenUnit &c : chosen) {
        FastaUnit x = {c.c0, c.c1, layout.lineLen[c.unit], 0, 0};
        x.file = meta.singleFastaFile ? 0 : c.unit - (meta.sequentialMatching ? 1 : 0);
        P.fileWanted[x.file] = 1;
        for (uint64_t k = x.c0; k < x.c1; k++) x.text += recordText(layout.hdrLen[k], contigLen[k], x.lineLen);
        P.units.push_back(x);
    }
    uint64_t cur = 0, curGz = 0;
    for (size_t u = 0; u < P.units.size(); u++) {
        if (cur && cur + P.units[u].text > (batchText ? batchText : FASTA_BATCH_TEXT)) {
            P.batchEnd.push_back(u); P.maxBatch = std::max(P.maxBatch, cur); P.maxGz = std::max(P.maxGz, curGz); cur = curGz = 0;
        }
        cur += P.units[u].text;
        if (gzip) curGz += mbgc_fasta_deflate_bound(P.units[u].text);
    }
    P.batchEnd.push_back(P.units.size()); P.maxBatch = std::max(P.maxBatch, cur); P.maxGz = std::max(P.maxGz, curGz);
    return P;
}

bool faFail(std::string &msg, const char *what) { msg = std::string(what) + ": " + mbgc_fasta_last_error(); return false; }

// ---- --select-seq: the records to bring back. The headers go to the device once, the match runs there (mbgc_fasta_match_headers_dev:
// what a header byte costs does not grow with the list), and a record is chosen when its header matched and its file passed --select
// (sel.unitSel as chooseUnits left it). Afterwards unitSel holds the units with a chosen record: the files that are written. G0's
// unit under -t1 is no file — its one contig is the first of target 0 again, and is chosen there. --bench: run twice, the second
// run is the timed one.
// the match itself: bit k of `bits` = header k contains one of the patterns (what: the option, for the message)
bool matchHeaders(const MBGC_Decoder::Options &opt, const FastaLayout &layout, uint64_t N, const std::vector<std::string> &pats, std::vector<uint32_t> &bits, double &ms,
                  const char *what, std::string &msg) {
    std::string patBytes;
    std::vector<uint64_t> patOff(1, 0);
    for (const std::string &p : pats) { patBytes += p; patOff.push_back(patBytes.size()); }
    bits.assign((N + 31) / 32, 0);
    struct Stage {                                                   // freed on every way out
        mbgc_fasta_t *fa = nullptr; uint8_t *hdrDev = nullptr;
        ~Stage() { if (hdrDev) mbgc_fasta_dev_free(fa, hdrDev); if (fa) mbgc_fasta_destroy(fa); }
    } st;
    if (mbgc_fasta_create(&st.fa, opt.device) || mbgc_fasta_dev_alloc(st.fa, layout.headers.size() + 64, &st.hdrDev) ||
        mbgc_fasta_upload(st.fa, st.hdrDev, layout.headers.data(), layout.headers.size())) return faFail(msg, what);
    for (int run = 0; run < (opt.bench ? 2 : 1); run++)
        if (mbgc_fasta_match_headers_dev(st.fa, st.hdrDev, layout.headers.size(), layout.hdrOff.data(), layout.hdrLen.data(), N, (const uint8_t *) patBytes.data(),
                                         patOff.data(), pats.size(), bits.data(), &ms)) return faFail(msg, what);
    return true;
}

bool chooseRecords(const std::string &prefix, const StreamSet &S, const MBGC_Decoder::Options &opt, const FastaLayout &layout, Selection &sel, std::string &msg) {
    const std::vector<std::string> &pats = opt.selectSeq;
    if (pats.empty()) return true;
    const uint64_t N = S.g0n + S.planned;
    std::vector<uint32_t> bits;
    if (!matchHeaders(opt, layout, N, pats, bits, sel.matchMs, "--select-seq", msg)) return false;
    if (opt.selectSeqHost) {                                         // the loop --select runs over the names, over the headers: a yardstick, and a check
        const double t0 = nowMs();
        std::vector<uint32_t> host((N + 31) / 32, 0);
        for (uint64_t c = 0; c < N; c++) {
            const std::string h(layout.headers, layout.hdrOff[c], layout.hdrLen[c]);
            for (const std::string &p : pats) if (h.find(p) != std::string::npos) { host[c >> 5] |= 1u << (c & 31); break; }
        }
        sel.matchHostMs = nowMs() - t0;
        if (host != bits) { msg = "--select-seq-host: the device and the host choose different records"; return false; }
    }
    const size_t T = S.T();
    sel.selecting = sel.selectingSeq = true;
    sel.contigSel.assign(N, 0);
    sel.selectedFiles = sel.recordsChosen = 0;
    sel.recordsAll = S.meta.sequentialMatching ? S.planned : N;
    uint64_t c = 0;
    for (size_t u = 0; u <= T; u++) {
        const uint64_t n = u == 0 ? S.g0n : S.seqCount[u - 1];
        char any = 0;
        if (sel.unitSel[u] && !(u == 0 && S.meta.sequentialMatching))
            for (uint64_t k = c; k < c + n; k++) if ((bits[k >> 5] >> (k & 31)) & 1u) { sel.contigSel[k] = any = 1; sel.recordsChosen++; }
        sel.unitSel[u] = any;
        if (!S.meta.singleFastaFile) sel.selectedFiles += any;
        c += n;
    }
    if (!sel.recordsChosen) {
        msg = "--select-seq: no record of the collection matches (" + std::to_string(pats.size()) + " patterns against " + prefix + ".headers)";
        return false;
    }
    if (S.meta.singleFastaFile) sel.selectedFiles = 1;              // its elements are no files: the one file holds what was chosen
    return true;
}

// ---- the stage that turns batches of a plan into text on the device: its handle, the headers and two text buffers in HBM (--gzip:
// two more for a batch's gzip files), two page-locked host buffers, and the record table of the batch formatted last. Freed on
// every way out, after the running writer and the running download have ended; it must go before the DecodedCollection it reads.
struct FastaStage {
    mbgc_fasta_t *fa = nullptr; uint8_t *hdrDev = nullptr, *textDev[2] = {nullptr, nullptr}; void *pin[2] = {nullptr, nullptr};
    uint8_t *gzDev[2] = {nullptr, nullptr};                        // --gzip: the gzip files of a batch (not allocated without it)
    std::future<bool> writing;
    const DecodedCollection *D = nullptr; const FastaPlan *P = nullptr; const FastaLayout *L = nullptr;
    const std::vector<uint64_t> *recOff = nullptr, *recLen = nullptr;   // where record k lies in the sequence buffer: the collection's contigs, or (--region) the pieces
    std::vector<mbgc_fasta_format_rec_t> recs;                     // the batch formatted last: its records,
    std::vector<uint64_t> textOff;                                 // and where their text starts in the batch
    FastaTimes times;

    FastaStage() = default;
    FastaStage(const FastaStage &) = delete;
    FastaStage &operator=(const FastaStage &) = delete;
    ~FastaStage() {
        if (writing.valid()) writing.wait();
        if (!fa) return;
        mbgc_fasta_download_wait(fa, nullptr);                     // (a way out between begin and wait)
        if (hdrDev) mbgc_fasta_dev_free(fa, hdrDev);
        for (uint8_t *t : textDev) if (t) mbgc_fasta_dev_free(fa, t);
        for (uint8_t *t : gzDev) if (t) mbgc_fasta_dev_free(fa, t);
        for (void *p : pin) if (p) mbgc_fasta_host_free(fa, p);
        mbgc_fasta_destroy(fa);
    }

    bool open(const DecodedCollection &d, const FastaPlan &p, const FastaLayout &l, int device, bool gzip, std::string &msg) {
        D = &d; P = &p; L = &l;
        if (!recOff) { recOff = &d.seqOff; recLen = &d.contigLen; }
        if (mbgc_fasta_create(&fa, device)) return faFail(msg, "--fasta");
        if (mbgc_fasta_dev_alloc(fa, l.headers.size() + 64, &hdrDev)) return faFail(msg, "--fasta");
        for (uint8_t *&t : textDev) if (mbgc_fasta_dev_alloc(fa, p.maxBatch + 64, &t)) return faFail(msg, "--fasta");
        if (gzip) for (uint8_t *&t : gzDev) if (mbgc_fasta_dev_alloc(fa, p.maxGz + 64, &t)) return faFail(msg, "--gzip");
        for (void *&h : pin) if (mbgc_fasta_host_alloc(fa, std::max<uint64_t>(gzip ? p.maxGz : p.maxBatch, l.headers.size()) + 64, &h)) return faFail(msg, "--fasta");
        memcpy(pin[0], l.headers.data(), l.headers.size());         // the headers go up through page-locked memory like everything else
        if (mbgc_fasta_upload(fa, hdrDev, pin[0], l.headers.size())) return faFail(msg, "--fasta");
        return true;
    }
    // units [u0, u1) formatted into dst: recs and textOff hold the batch's record table afterwards
    bool formatBatch(size_t u0, size_t u1, uint8_t *dst, uint64_t &bytes, std::string &msg) {
        recs.clear();
        for (size_t u = u0; u < u1; u++)
            for (uint64_t k = P->units[u].c0; k < P->units[u].c1; k++)
                recs.push_back({(*recOff)[k], (*recLen)[k], L->hdrOff[k], L->hdrLen[k], P->units[u].lineLen});
        textOff.assign(recs.size() + 1, 0);
        double kms = 0;
        if (mbgc_fasta_format_dev(fa, D->seqDev, D->totalBases, hdrDev, L->headers.size(), recs.data(), recs.size(), dst, P->maxBatch, textOff.data(), &kms))
            return faFail(msg, "format");
        times.format += kms;
        bytes = textOff[recs.size()];
        times.text += bytes; times.batches++;
        return true;
    }
};

// ---- the writer of `d --fasta`. Batch b: formatted into device buffer b & 1; its download into page-locked buffer b & 1 begins at
// once, on a stream of its own, and is waited for after batch b + 1 has been formatted into the other device buffer; then its
// writer starts, once the writer of batch b - 1 has ended. So the download of b and the writes of b - 1 run beside the format of
// b + 1, and page-locked buffer b & 1 is free again (writer b - 2 was waited for) before download b begins.
struct FastaPiece { size_t file; uint64_t off, len; bool first; };
struct FastaDownload {
    std::vector<FastaPiece> inFlight;                              // the pieces of the batch whose download runs
    uint8_t *host = nullptr;
    bool running = false;
};

// the running download -> its writer (writeFiles: else the bytes are dropped, the timed pass of --bench)
bool settleDownload(FastaStage &stage, FastaDownload &dl, const FastaLayout &layout, const MBGC_Decoder::Options &opt, bool writeFiles, std::string &msg) {
    if (!dl.running) return true;
    double cms = 0;
    if (mbgc_fasta_download_wait(stage.fa, &cms)) return faFail(msg, "download");
    stage.times.download += cms;
    dl.running = false;
    const double w0 = nowMs();
    const bool ok = !stage.writing.valid() || stage.writing.get();
    stage.times.write += nowMs() - w0;                             // (what the writes hold the pipeline up by)
    if (!ok) { msg = "cannot write under " + opt.fastaDir; return false; }
    if (!writeFiles) return true;
    const std::string dir = opt.fastaDir, suffix = opt.gzip ? ".gz" : "";
    const std::vector<std::string> *outNames = &layout.outNames;
    const std::vector<FastaPiece> pieces = dl.inFlight;
    const uint8_t *host = dl.host;
    stage.writing = std::async(std::launch::async, [pieces, host, dir, suffix, outNames] {
        for (const FastaPiece &p : pieces) {
            std::ofstream f(dir + "/" + (*outNames)[p.file] + suffix, std::ios::binary | (p.first ? std::ios::trunc : std::ios::app));
            f.write((const char *) host + p.off, (std::streamsize) p.len);
            f.close();                                              // (an error may only show when the last bytes leave the buffer)
            if (!f) return false;
        }
        return true;
    });
    return true;
}

// --gzip: one deflate call over batch b, a job per piece; a piece becomes one gzip member, appended to its file like the text would
// be, and only the gzip bytes travel (gzDev[b & 1]: the download of batch b - 2 has been settled). The pieces' off / len are
// rewritten to the deflate results — before the download begins — and `bytes` becomes the gzip bytes of the batch.
bool deflateBatch(FastaStage &stage, size_t b, std::vector<FastaPiece> &pieces, uint64_t &bytes, std::string &msg) {
    std::vector<mbgc_fasta_deflate_job_t> jobs;
    for (const FastaPiece &pc : pieces) jobs.push_back({pc.off, pc.len});
    std::vector<mbgc_fasta_deflate_result_t> res(jobs.size());
    uint64_t gzBytes = 0;
    double dms = 0;
    if (mbgc_fasta_deflate_dev(stage.fa, stage.textDev[b & 1], bytes, jobs.data(), jobs.size(), stage.gzDev[b & 1], stage.P->maxGz, res.data(), &gzBytes, &dms))
        return faFail(msg, "deflate");
    for (size_t k = 0; k < res.size(); k++) {
        pieces[k].off = res[k].outOff; pieces[k].len = res[k].outLen;
        stage.times.chunks += res[k].chunks; stage.times.storedChunks += res[k].storedChunks;
    }
    stage.times.deflate += dms; stage.times.gz += gzBytes;
    bytes = gzBytes;
    return true;
}

bool writeFastaFiles(const FastaPlan &plan, FastaStage &stage, const FastaLayout &layout, const MBGC_Decoder::Options &opt, bool writeFiles, std::string &msg) {
    std::vector<char> opened(layout.outNames.size(), 0);
    FastaDownload dl;
    size_t u0 = 0;
    for (size_t b = 0; b < plan.batchEnd.size(); b++) {
        const size_t u1 = plan.batchEnd[b];
        uint64_t bytes = 0;
        if (!stage.formatBatch(u0, u1, stage.textDev[b & 1], bytes, msg)) return false;
        if (!settleDownload(stage, dl, layout, opt, writeFiles, msg)) return false;   // batch b - 1: it travelled beside this batch's format
        // (the writer of b - 2, which read page-locked buffer b & 1, was waited for by that settle or the one before)
        dl.inFlight.clear();
        uint64_t at = 0;
        for (size_t u = u0; u < u1; u++) {
            const FastaUnit &x = plan.units[u];
            // --select-seq: the runs of one file that follow each other in the batch are one piece — one write, one gzip member
            if (plan.runs && !dl.inFlight.empty() && dl.inFlight.back().file == x.file) dl.inFlight.back().len += x.text;
            else dl.inFlight.push_back({x.file, at, x.text, !opened[x.file]});
            opened[x.file] = 1;
            at += x.text;
        }
        if (at != bytes) { msg = "internal error: the text of a batch is not the sum of its units"; return false; }
        const uint8_t *src = stage.textDev[b & 1];
        if (opt.gzip) {
            if (!deflateBatch(stage, b, dl.inFlight, bytes, msg)) return false;
            src = stage.gzDev[b & 1];
        }
        dl.host = (uint8_t *) stage.pin[b & 1];
        if (mbgc_fasta_download_begin(stage.fa, dl.host, src, bytes)) return faFail(msg, "download");
        dl.running = true;
        u0 = u1;
    }
    if (!settleDownload(stage, dl, layout, opt, writeFiles, msg)) return false;
    const double w0 = nowMs();
    if (stage.writing.valid() && !stage.writing.get()) { msg = "cannot write under " + opt.fastaDir; return false; }
    stage.times.write += nowMs() - w0;
    // (files of units without a record exist too, empty)
    static const unsigned char emptyGz[20] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (--gzip: the gzip file of no text)
    if (writeFiles)
        for (size_t f = 0; f < opened.size(); f++)
            if (!opened[f] && plan.fileWanted[f] && !writeFile(opt.fastaDir + "/" + layout.outNames[f] + (opt.gzip ? ".gz" : ""), opt.gzip ? (const char *) emptyGz : "", opt.gzip ? sizeof emptyGz : 0)) {
                msg = "cannot write under " + opt.fastaDir;
                return false;
            }
    return true;
}
}  // namespace
