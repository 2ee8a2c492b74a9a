// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_fasta.h): `mbgc-hip v`. The text stays on the
// device. Batch b is formatted into the first text buffer while a thread reads (and inflates) the originals of batch b + 1 into
// the page-locked buffer that batch b - 1 left; the originals of b go up into the second text buffer, one compare call runs over
// the batch with a slot per file, and a word per file comes back. A single-FASTA collection is one file over all batches: one
// piece per batch at the file's running offset, only that slice of the original is read and uploaded.
#pragma once

namespace {
static const uint64_t VALIDATION_LOG_LIMIT = 100, VALIDATION_DUMP_LIMIT = 3;   // MBGC_Params.h:121-122
// the originals of a batch as the read-ahead thread leaves them in a page-locked buffer
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
struct ValidateResult { uint64_t validFiles = 0, invalidFiles = 0, validatedFiles = 0; ValidateTimes times; };

// where a unit's original lies: its line of <prefix>.names; --flat: the basename `d --fasta` writes it under; --root before relative names
std::string originalPath(const std::string &name, const std::string &root, bool flat) {
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
ErrorLocation locateError(uint64_t first, uint64_t rec, uint64_t at, const std::vector<uint64_t> &hdrLen, const std::vector<uint64_t> &seqLen, uint64_t lineLen) {
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

// the one file of a single-FASTA collection, open over all batches, and what the batches so far have found about it
struct SingleOriginal {
    OpenOriginal file;
    std::string path;
    bool found = false, differs = false;
    ErrorLocation loc;
};

// ---- one pass of `v` over a plan: what its steps share. report: the last pass (--bench: the first pass warms up and stays quiet).
struct Validation {
    const DecodedCollection &D; const FastaPlan &P; FastaStage &stage; const FastaLayout &layout; const MbgcMeta &meta; const MBGC_Decoder::Options &opt;
    const bool report, single;
    ValidateResult res;
    uint64_t dumped = 0;
    std::vector<uint64_t> batchAt;                                 // text in front of every batch
    uint64_t totalText = 0;
    SingleOriginal one;
    uint8_t *gzDev = nullptr; uint64_t gzDevCap = 0;               // --inflate device: a batch's gzip bytes in HBM
    std::vector<mbgc_fasta_compare_piece_t> pieces;
    std::vector<uint64_t> firstDiff;

    Validation(const DecodedCollection &d, const FastaPlan &p, FastaStage &s, const FastaLayout &l, const MbgcMeta &m, const MBGC_Decoder::Options &o, bool report)
        : D(d), P(p), stage(s), layout(l), meta(m), opt(o), report(report), single(m.singleFastaFile) {}
    ~Validation() { if (gzDev) mbgc_fasta_dev_free(stage.fa, gzDev); }

    std::string nameOf(const FastaUnit &x) const { return originalPath(layout.names[single ? 0 : x.file + (meta.sequentialMatching ? 1 : 0)], opt.root, opt.flat); }
    size_t batchBegin(size_t b) const { return b ? P.batchEnd[b - 1] : 0; }
    OriginalsBatch readBatch(size_t b) const;
    bool putOriginals(size_t b, OriginalsBatch &R, std::string &msg);
    bool inflateOriginals(OriginalsBatch &R, std::string &msg);
    bool compareBatch(size_t b, uint64_t bytes, const OriginalsBatch &R, std::string &msg);
    ErrorLocation locate(const FastaUnit &x, uint64_t at, size_t rec, uint64_t pos, uint64_t firstContig) const;
    void reportInvalid(const std::string &path, bool sizeDiffer, uint64_t ours, uint64_t theirs, const ErrorLocation &loc) const;
    bool dumpText(const std::string &name, const uint8_t *src, uint64_t n, bool append, std::string &msg);
    void judgeSingleBatch(size_t b);
    bool judgeBatch(size_t b, const OriginalsBatch &R, std::string &msg);
    bool judgeSingle(std::string &msg);
    bool run(std::string &msg);
};

// the read-ahead thread's function: the originals of batch b into page-locked buffer b & 1
OriginalsBatch Validation::readBatch(size_t b) const {
    OriginalsBatch R;
    const double r0 = nowMs();
    uint8_t *dst = (uint8_t *) stage.pin[b & 1];
    if (single) {
        Original o;
        o.path = one.path; o.found = one.found; o.size = one.file.size; o.unreadable = one.file.broken;
        if (one.found && batchAt[b] < one.file.size) {
            o.n = std::min(batchAt[b + 1] - batchAt[b], one.file.size - batchAt[b]);
            if (!one.file.readAt(dst, batchAt[b], o.n)) R.error = "cannot read " + one.path;
        }
        R.bytes = o.n;
        R.files.push_back(o);
        R.ms = nowMs() - r0;
        return R;
    }
    for (size_t u = batchBegin(b); u < P.batchEnd[b] && R.error.empty(); u++) {
        Original o;
        OpenOriginal f;
        o.path = nameOf(P.units[u]);
        o.found = f.open(o.path, R.error, opt.inflateOnDevice);
        if (o.found && R.error.empty() && f.deferred) {
            // a gzip original whose trailer states the length of our text goes up compressed and is inflated into its
            // place beside the batch; any other one differs in size already and is inflated here, for its size
            if (f.size == P.units[u].text) {
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
            o.size = f.size; o.off = R.bytes; o.n = std::min(f.size, P.units[u].text);
            if (!f.readAt(dst + o.off, 0, o.n)) R.error = "cannot read " + o.path;
            R.bytes += o.n;
        }
        R.files.push_back(o);
    }
    R.ms = nowMs() - r0;
    return R;
}

// the originals of batch b into the second text buffer: one upload, or the --inflate device path
bool Validation::putOriginals(size_t b, OriginalsBatch &R, std::string &msg) {
    const double up0 = nowMs();
    if (R.gz.empty()) { if (mbgc_fasta_upload(stage.fa, stage.textDev[1], stage.pin[b & 1], R.bytes)) return faFail(msg, "upload"); }
    else {
        // --inflate device: the plain originals go up run by run, the gzip ones compressed, and those are inflated into their places
        for (size_t i = 0; i < R.files.size();) {
            size_t j = i;
            while (j < R.files.size() && !R.files[j].gzLen) j++;
            if (j > i) {
                const uint64_t a = R.files[i].off, e = R.files[j - 1].off + R.files[j - 1].n;
                if (e > a && mbgc_fasta_upload(stage.fa, stage.textDev[1] + a, (const uint8_t *) stage.pin[b & 1] + a, e - a)) return faFail(msg, "upload");
            }
            while (j < R.files.size() && R.files[j].gzLen) j++;
            i = j;
        }
        if (!inflateOriginals(R, msg)) return false;
    }
    res.times.upload += nowMs() - up0;
    return true;
}

// A job that does not end with exactly the text's length is done again by tryInflateGzip, as --inflate host does it: its verdict,
// its size and its message are the ones reported.
bool Validation::inflateOriginals(OriginalsBatch &R, std::string &msg) {
    if (R.gz.size() + 64 > gzDevCap) {
        if (gzDev && mbgc_fasta_dev_free(stage.fa, gzDev)) return faFail(msg, "upload");
        gzDev = nullptr; gzDevCap = R.gz.size() + R.gz.size() / 4 + 64;
        if (mbgc_fasta_dev_alloc(stage.fa, gzDevCap, &gzDev)) return faFail(msg, "upload");
    }
    if (mbgc_fasta_upload(stage.fa, gzDev, R.gz.data(), R.gz.size())) return faFail(msg, "upload");
    std::vector<mbgc_fasta_inflate_job_t> jobs;
    std::vector<size_t> jobFile;
    for (size_t i = 0; i < R.files.size(); i++)
        if (R.files[i].gzLen) { jobs.push_back({R.files[i].gzOff, R.files[i].gzLen, R.files[i].off, R.files[i].n}); jobFile.push_back(i); }
    std::vector<mbgc_fasta_inflate_result_t> got(jobs.size());
    double ims = 0;
    if (mbgc_fasta_inflate_dev(stage.fa, gzDev, R.gz.size(), stage.textDev[1], R.bytes, jobs.data(), jobs.size(), got.data(), &ims)) return faFail(msg, "inflate");
    res.times.inflate += ims;
    for (size_t k = 0; k < jobs.size(); k++) {
        Original &o = R.files[jobFile[k]];
        if (got[k].status == MBGC_INFLATE_OK && got[k].outLen == o.n) { res.times.inflatedOnDevice++; continue; }
        res.times.inflatedAgainOnHost++;
        std::string text;
        if (!tryInflateGzip(R.gz.substr(o.gzOff, o.gzLen), text, o.unreadable)) text.clear();
        o.size = text.size();
        o.n = std::min<uint64_t>(o.size, o.n);                      // (its place is as long as our text)
        if (o.n && mbgc_fasta_upload(stage.fa, stage.textDev[1] + o.off, text.data(), o.n)) return faFail(msg, "upload");
    }
    return true;
}

// one compare call over batch b (`bytes` of text in the first buffer): firstDiff holds a word per file afterwards
bool Validation::compareBatch(size_t b, uint64_t bytes, const OriginalsBatch &R, std::string &msg) {
    const size_t u0 = batchBegin(b), u1 = P.batchEnd[b];
    pieces.clear();
    if (single) pieces.push_back({0, 0, R.files[0].n, 0});
    else {
        uint64_t at = 0;
        for (size_t u = u0; u < u1; u++) { pieces.push_back({at, R.files[u - u0].off, R.files[u - u0].n, (uint32_t) (u - u0)}); at += P.units[u].text; }
    }
    firstDiff.assign(R.files.size(), UINT64_MAX);
    double kms = 0;
    if (mbgc_fasta_compare_dev(stage.fa, stage.textDev[0], bytes, stage.textDev[1], R.bytes, pieces.data(), pieces.size(), firstDiff.data(), (uint32_t) firstDiff.size(), &kms))
        return faFail(msg, "compare");
    res.times.compare += kms;
    for (const mbgc_fasta_compare_piece_t &pc : pieces) res.times.compared += pc.len;
    return true;
}

// the record of unit x (its text starts at `at` in the batch, its records at row `rec` of the batch's table) that holds text offset pos of the unit
ErrorLocation Validation::locate(const FastaUnit &x, uint64_t at, size_t rec, uint64_t pos, uint64_t firstContig) const {
    const std::vector<uint64_t> &textOff = stage.textOff;
    const size_t nrec = (size_t) (x.c1 - x.c0);
    if (nrec == 0) return locateError(firstContig, firstContig, 0, layout.hdrLen, D.contigLen, x.lineLen);
    const size_t j = (size_t) (std::upper_bound(textOff.begin() + rec, textOff.begin() + rec + nrec, at + pos) - (textOff.begin() + rec)) - 1;
    return locateError(firstContig, x.c0 + j, at + pos - textOff[rec + j], layout.hdrLen, D.contigLen, x.lineLen);
}

// the reference's words (MBGC_Decoder.cpp:112-183); the log ends after VALIDATION_LOG_LIMIT invalid files
void Validation::reportInvalid(const std::string &path, bool sizeDiffer, uint64_t ours, uint64_t theirs, const ErrorLocation &loc) const {
    if (!report || res.invalidFiles >= VALIDATION_LOG_LIMIT) return;
    const unsigned long long n = res.validFiles + res.invalidFiles;
    if (sizeDiffer) printf("Validation ERROR: ~%llu. %s size differ (%llu instead of %llu)\n", n, path.c_str(), (unsigned long long) ours, (unsigned long long) theirs);
    else printf("Validation ERROR: ~%llu. %s contents differ.\n", n, path.c_str());
    if (loc.kind == ErrorLocation::SEQUENCE) printf("Error location:\t\tseqIdx = %llu\tseqPos = %llu\n", (unsigned long long) loc.seqIdx, (unsigned long long) loc.seqPos);
    else if (loc.kind == ErrorLocation::HEADER) printf("Error in header:\t\tseqIdx = %llu\n", (unsigned long long) loc.seqIdx);
    else if (loc.kind == ErrorLocation::NO_SEQUENCE) printf("Error in FASTA format - no sequences found in equal part.\n");
}

// --dump: n bytes of text in HBM into <dumpDir>/<name>
bool Validation::dumpText(const std::string &name, const uint8_t *src, uint64_t n, bool append, std::string &msg) {
    std::string text(n, '\0');
    if (n && mbgc_fasta_download(stage.fa, &text[0], src, n)) return faFail(msg, "--dump");
    std::string failed;
    bool ok = makeDirs(opt.dumpDir, &failed);
    if (ok) {
        std::ofstream f(opt.dumpDir + "/" + name, std::ios::binary | (append ? std::ios::app : std::ios::trunc));
        f.write(text.data(), (std::streamsize) n);
        f.close();
        ok = (bool) f;
    }
    if (!ok) msg = "cannot write under " + opt.dumpDir;
    return ok;
}

// a single-FASTA collection, after batch b's compare: the first difference, or — sizes differ, bytes do not — the end of the shorter
// of the two, in the batch that holds it
void Validation::judgeSingleBatch(size_t b) {
    const size_t u0 = batchBegin(b), u1 = P.batchEnd[b], nb = P.batchEnd.size();
    uint64_t pos = UINT64_MAX;
    const uint64_t commonEnd = std::min(totalText, one.file.size);
    if (one.found && one.loc.kind == ErrorLocation::NONE) {
        if (firstDiff[0] != UINT64_MAX) { pos = firstDiff[0]; one.differs = true; }
        else if (one.file.size != totalText && commonEnd >= batchAt[b] && (commonEnd < batchAt[b + 1] || b + 1 == nb)) pos = commonEnd - batchAt[b];
    }
    uint64_t at = 0;
    size_t rec = 0;
    for (size_t u = u0; u < u1 && pos != UINT64_MAX; u++) {
        if (pos < at + P.units[u].text || u + 1 == u1) { one.loc = locate(P.units[u], at, rec, pos - at, P.units[0].c0); break; }
        at += P.units[u].text; rec += (size_t) (P.units[u].c1 - P.units[u].c0);
    }
}

// the verdict on every file of batch b; the text of the first VALIDATION_DUMP_LIMIT invalid ones goes to --dump
bool Validation::judgeBatch(size_t b, const OriginalsBatch &R, std::string &msg) {
    const size_t u0 = batchBegin(b), u1 = P.batchEnd[b];
    uint64_t at = 0;
    size_t rec = 0;
    for (size_t u = u0; u < u1; u++) {
        const FastaUnit &x = P.units[u];
        const Original &o = R.files[u - u0];
        if (!o.found) {
            if (report && res.invalidFiles < VALIDATION_LOG_LIMIT) fprintf(stderr, "Cannot find %s for validation.\n", o.path.c_str());
            res.invalidFiles++;
        } else if (!o.unreadable.empty()) {
            if (report && res.invalidFiles < VALIDATION_LOG_LIMIT) fprintf(stderr, "Cannot read %s for validation: %s\n", o.path.c_str(), o.unreadable.c_str());
            res.invalidFiles++;
        } else if (o.size == x.text && firstDiff[u - u0] == UINT64_MAX) res.validFiles++;
        else {
            const uint64_t pos = firstDiff[u - u0] != UINT64_MAX ? firstDiff[u - u0] : std::min(x.text, o.size);
            reportInvalid(o.path, o.size != x.text, x.text, o.size, locate(x, at, rec, pos, x.c0));
            res.invalidFiles++;
            if (report && !opt.dumpDir.empty() && dumped++ < VALIDATION_DUMP_LIMIT)
                if (!dumpText(layout.outNames[x.file], stage.textDev[0] + at, x.text, false, msg)) return false;
        }
        at += x.text; rec += (size_t) (x.c1 - x.c0);
    }
    return true;
}

// one file: its verdict, and its size, after the last batch. --dump: the text of the earlier batches is gone, so all batches are
// formatted once more; the stage's times are put back afterwards (the report counts the text once)
bool Validation::judgeSingle(std::string &msg) {
    if (!one.found) {
        if (report) fprintf(stderr, "Cannot find %s for validation.\n", one.path.c_str());
        res.invalidFiles++;
    } else if (!one.file.broken.empty()) {
        if (report) fprintf(stderr, "Cannot read %s for validation: %s\n", one.path.c_str(), one.file.broken.c_str());
        res.invalidFiles++;
    } else if (one.file.size == totalText && !one.differs) res.validFiles++;
    else {
        reportInvalid(one.path, one.file.size != totalText, totalText, one.file.size, one.loc);
        res.invalidFiles++;
        if (report && !opt.dumpDir.empty()) {
            const FastaTimes keep = stage.times;
            for (size_t b = 0; b < P.batchEnd.size(); b++) {
                uint64_t bytes = 0;
                if (!stage.formatBatch(batchBegin(b), P.batchEnd[b], stage.textDev[0], bytes, msg)) return false;
                if (!dumpText(layout.outNames[0], stage.textDev[0], bytes, b != 0, msg)) return false;
            }
            stage.times = keep;
        }
    }
    return true;
}

bool Validation::run(std::string &msg) {
    const size_t nb = P.batchEnd.size();
    res.validatedFiles = single ? 1 : P.units.size();
    if (report && !opt.skipCompare && meta.uppercaseDNA)
        printf("the streams were written with -U: the text is upper case, originals that hold lower-case bases differ from it\n");
    batchAt.assign(nb + 1, 0);
    for (size_t b = 0, u = 0; b < nb; b++) { batchAt[b + 1] = batchAt[b]; for (; u < P.batchEnd[b]; u++) batchAt[b + 1] += P.units[u].text; }
    totalText = batchAt[nb];
    one.path = single && !P.units.empty() ? nameOf(P.units[0]) : std::string();
    if (single && !opt.skipCompare) {
        const double r0 = nowMs();
        std::string e;
        one.found = one.file.open(one.path, e);
        if (!e.empty()) { msg = e; return false; }
        res.times.read += nowMs() - r0;
    }
    // (the read-ahead thread reads this object and writes the stage's page-locked buffers: `reading` ends before both, on every way out)
    std::future<OriginalsBatch> reading;
    if (!opt.skipCompare && nb) reading = std::async(std::launch::async, &Validation::readBatch, this, (size_t) 0);
    for (size_t b = 0; b < nb; b++) {
        OriginalsBatch R;
        if (!opt.skipCompare) {
            R = reading.get();
            if (b + 1 < nb) reading = std::async(std::launch::async, &Validation::readBatch, this, b + 1);
            if (!R.error.empty()) { msg = R.error; return false; }
            res.times.read += R.ms;
        }
        uint64_t bytes = 0;
        if (!stage.formatBatch(batchBegin(b), P.batchEnd[b], stage.textDev[0], bytes, msg)) return false;
        if (bytes != batchAt[b + 1] - batchAt[b]) { msg = "internal error: the text of a batch is not the sum of its units"; return false; }
        if (opt.skipCompare) continue;
        if (!putOriginals(b, R, msg) || !compareBatch(b, bytes, R, msg)) return false;
        if (single) judgeSingleBatch(b);
        else if (!judgeBatch(b, R, msg)) return false;
    }
    if (single && !opt.skipCompare && !judgeSingle(msg)) return false;
    if (report && !opt.skipCompare) {
        printf("Validation%s: correctly decoded %llu out of %llu files.\n", res.invalidFiles ? " ERROR" : "", (unsigned long long) res.validFiles, (unsigned long long) res.validatedFiles);
        if (res.invalidFiles) fprintf(stderr, "Validation ERROR: errors in contents of %llu decoded files.\n", (unsigned long long) res.invalidFiles);
    }
    return true;
}
}  // namespace
