// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_validate.h): what `d --check` / `t`, `f`, `s`, `k` and `u` share. Each of
// them puts one question to the CHOSEN contigs where the decoder left them — contigs that were decoded only because a chosen one depends
// on them are not looked at —, through a handle of the input stage of its own, once or, under --bench, six times, and its developer
// switch (--*-host) downloads the same records to ask the host.
#pragma once

namespace {
// the chosen contigs as the records of one device call over the decoder's sequence buffer, in collection order
struct ChosenRecords {
    struct Record { uint64_t contig; size_t unit; uint64_t len; };   // unit: the file's place in the layout's names (0 for a single-FASTA set)
    std::vector<mbgc_fasta_crc_rec_t> recs;                          // record r's bytes in D.seqDev
    std::vector<Record> records;                                     // record r's contig, file and length
    std::vector<size_t> units;                                       // the chosen files, one without a contig too
    uint64_t bases = 0;
    ChosenRecords() = default;
    ChosenRecords(const DecodedCollection &D, const StreamSet &S, const std::vector<ChosenUnit> &chosen) {
        for (const ChosenUnit &x : chosen) {
            const size_t unit = S.meta.singleFastaFile ? 0 : x.unit;
            if (units.empty() || units.back() != unit) units.push_back(unit);
            for (uint64_t k = x.c0; k < x.c1; k++) {
                recs.push_back(mbgc_fasta_crc_rec_t{D.seqOff[k], D.contigLen[k]});
                records.push_back({k, unit, D.contigLen[k]});
                bases += D.contigLen[k];
            }
        }
    }
    size_t size() const { return recs.size(); }
};

// a handle of the input stage that is destroyed on every way out
struct FastaHandle {
    mbgc_fasta_t *p = nullptr;
    FastaHandle() = default;
    FastaHandle(const FastaHandle &) = delete;
    FastaHandle &operator=(const FastaHandle &) = delete;
    ~FastaHandle() { mbgc_fasta_destroy(p); }
    bool open(int device, std::string &msg) { return !mbgc_fasta_create(&p, device) || faFail(msg, "input stage"); }
    operator mbgc_fasta_t *() const { return p; }
};

// fn(ms) makes the call once and leaves its N kernel times in ms, false when it failed. Run once; under --bench (timed) six times, one
// to warm up: median[i] is the median of the last five
template <size_t N, class Fn>
bool timedCalls(bool timed, double (&median)[N], Fn fn) {
    std::vector<double> all[N];
    for (int rep = 0; rep < (timed ? 6 : 1); rep++) {
        double ms[N] = {};
        if (!fn(ms)) return false;
        for (size_t i = 0; i < N && (rep || !timed); i++) all[i].push_back(ms[i]);
    }
    for (size_t i = 0; i < N; i++) { std::sort(all[i].begin(), all[i].end()); median[i] = all[i][all[i].size() / 2]; }
    return true;
}

// the bytes of one record, for a --*-host check
bool downloadRecord(const DecodedCollection &D, const mbgc_fasta_crc_rec_t &rec, std::string &text, std::string &msg) {
    text.resize(rec.len);
    return !rec.len || !swsem_dev_download(D.h, &text[0], D.seqDev + rec.off, rec.len) || hipFail(msg, "download");
}

// what stands in front of a scan: the decode, as the --bench lines of f, s, k and u state it
double decodeMs(const DecodedCollection &D, const StreamSet &S) { return D.times.plan + D.times.closure + D.times.fill + D.times.load + S.rcRestoreMs; }
}  // namespace
