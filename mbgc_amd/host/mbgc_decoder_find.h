// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_check.h): `mbgc-hip f` — query sequences searched in the decoded
// collection where it lies. The CHOSEN contigs are the records of one mbgc_fasta_find_dev call over the decoder's
// sequence buffer (contigs that were decoded only because a chosen one depends on them are not searched, as in `d --check`); the
// patterns are the queries and, unless --forward-only, their reverse complements — made on the device by the loader's own kernel
// (swsem_revcomp_dev: the reference's complement table), so a base is complemented here exactly as the decoder complements one. A
// few rows come back; the host names them (query, file, record, 1-based forward-strand coordinates, strand) and sorts them.
// --iupac: the queries are IUPAC patterns and go to mbgc_fasta_find_iupac_dev (a letter is a set of bases, a text byte without a base
// matches nothing); their reverse complements are made here, on the host, by the IUPAC complement — the loader's kernel knows bases only.
// --primers: the queries are the pairs' primers, FWD then REV; the same one search, then the host pairs the hits per record into
// products (mbgc_find_amplicons.h).
#pragma once
#include "mbgc_find_amplicons.h"

namespace {
struct FindLine { uint64_t contig, start, end; uint32_t query; char strand; uint32_t mismatches; size_t unit; };
struct AmpliconLine { uint64_t contig, start, end; uint32_t pair; char strand; uint32_t leftMismatches, rightMismatches; size_t unit; };
struct FindResult {
    std::vector<FindLine> lines;
    std::vector<AmpliconLine> amplicons;                                        // --primers: the products; ampRecords, ampFiles: those with one
    uint64_t ampRecords = 0, ampFiles = 0, tableRows = 0, rowsWalked = 0;       // --iupac: the table's rows and the rows the lanes walked
    uint64_t records = 0, files = 0, bases = 0, patterns = 0, retries = 0;      // records, files: those with a hit; bases: those searched
    double kernelMs = 0, hostMs = 0;
};

// the first word of contig k's header: what `d --region` is given to find the record again
std::string recordName(const FastaLayout &layout, uint64_t k) {
    const std::string h(layout.headers, layout.hdrOff[k], layout.hdrLen[k]);
    return h.substr(0, h.find_first_of(" \t"));
}

// --find-host: the obvious loop over the downloaded contigs — every pattern at every position, the mismatches counted byte by byte —,
// the patterns shared among a few threads; rows as the device reports them, in its order
struct HostHit { uint64_t pos; uint32_t rec, pattern, mismatches; };
std::vector<HostHit> findOnHost(const std::vector<std::string> &text, const std::vector<std::string> &patterns, uint32_t K) {
    const auto fold = [](uint8_t b) { return (uint8_t) (((b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z')) ? b & 0xDF : b); };
    const size_t threads = std::max<size_t>(1, std::min<size_t>({(size_t) 16, (size_t) std::thread::hardware_concurrency(), patterns.size()}));
    std::vector<std::future<std::vector<HostHit>>> parts;
    for (size_t w = 0; w < threads; w++)
        parts.push_back(std::async(std::launch::async, [&, w] {
            std::vector<HostHit> out;
            for (size_t q = w; q < patterns.size(); q += threads)
                for (size_t r = 0; r < text.size(); r++)
                    for (uint64_t p = 0; p + patterns[q].size() <= text[r].size(); p++) {
                        uint32_t d = 0;
                        for (size_t j = 0; j < patterns[q].size() && d <= K; j++) d += fold((uint8_t) text[r][p + j]) != fold((uint8_t) patterns[q][j]);
                        if (d <= K) out.push_back({p, (uint32_t) r, (uint32_t) q, d});
                    }
            return out;
        }));
    std::vector<HostHit> all;
    for (auto &f : parts) { const std::vector<HostHit> part = f.get(); all.insert(all.end(), part.begin(), part.end()); }
    std::sort(all.begin(), all.end(), [](const HostHit &a, const HostHit &b) { return std::tie(a.rec, a.pos, a.pattern) < std::tie(b.rec, b.pos, b.pattern); });
    return all;
}

// --iupac: the set of a letter (upper case, of the table: the command line holds the queries to it) as a mask of A 1, C 2, G 4, T 8, and
// the base of a text byte as such a mask, 0 for a byte without one — written out here, apart from the device's constants
uint32_t iupacSetOf(char c) {
    static const char *const sets[] = {"AA", "CC", "GG", "TT", "UT", "RAG", "YCT", "SCG", "WAT", "KGT", "MAC", "BCGT", "DAGT", "HACT", "VACG", "NACGT"};
    uint32_t m = 0;
    for (const char *s : sets)
        if (s[0] == c) for (const char *b = s + 1; *b; b++) m |= *b == 'A' ? 1u : *b == 'C' ? 2u : *b == 'G' ? 4u : 8u;
    return m;
}
uint32_t iupacBaseOf(uint8_t b) {
    switch (b) { case 'a': case 'A': return 1; case 'c': case 'C': return 2; case 'g': case 'G': return 4; case 't': case 'T': case 'u': case 'U': return 8; }
    return 0;
}
// the reverse complement of an IUPAC pattern (upper case, U already T): A-T, C-G, R-Y, K-M, B-V, D-H; S, W and N are their own
std::string iupacReverseComplement(const std::string &q) {
    static const char from[] = "ACGTRYKMBVDHSWN", to[] = "TGCAYRMKVBHDSWN";
    std::string r(q.rbegin(), q.rend());
    for (char &c : r) if (const char *at = strchr(from, c)) c = to[at - from];
    return r;
}

// --find-host under --iupac: the same plain loop with the rule of the sets
std::vector<HostHit> findOnHostIupac(const std::vector<std::string> &text, const std::vector<std::string> &patterns, uint32_t K) {
    const size_t threads = std::max<size_t>(1, std::min<size_t>({(size_t) 16, (size_t) std::thread::hardware_concurrency(), patterns.size()}));
    std::vector<std::future<std::vector<HostHit>>> parts;
    for (size_t w = 0; w < threads; w++)
        parts.push_back(std::async(std::launch::async, [&, w] {
            std::vector<HostHit> out;
            for (size_t q = w; q < patterns.size(); q += threads) {
                std::vector<uint32_t> sets;
                for (char c : patterns[q]) sets.push_back(iupacSetOf(c));
                for (size_t r = 0; r < text.size(); r++)
                    for (uint64_t p = 0; p + sets.size() <= text[r].size(); p++) {
                        uint32_t d = 0;
                        for (size_t j = 0; j < sets.size() && d <= K; j++) d += (sets[j] & iupacBaseOf((uint8_t) text[r][p + j])) == 0;
                        if (d <= K) out.push_back({p, (uint32_t) r, (uint32_t) q, d});
                    }
            }
            return out;
        }));
    std::vector<HostHit> all;
    for (auto &f : parts) { const std::vector<HostHit> part = f.get(); all.insert(all.end(), part.begin(), part.end()); }
    std::sort(all.begin(), all.end(), [](const HostHit &a, const HostHit &b) { return std::tie(a.rec, a.pos, a.pattern) < std::tie(b.rec, b.pos, b.pattern); });
    return all;
}

bool findQueries(const DecodedCollection &D, const StreamSet &S, const FastaLayout &layout, const std::vector<ChosenUnit> &chosen, const MBGC_Decoder::Options &opt,
                 bool timed, FindResult &R, std::string &msg) {
    R = FindResult();
    const std::vector<MBGC_Decoder::FindQuery> &Q = opt.findQueries;
    // ---- the patterns: every query, then (unless --forward-only) every reverse complement that is not its own query
    struct Pattern { uint32_t query; char strand; };
    std::vector<Pattern> what;
    std::vector<std::string> patterns;
    for (size_t q = 0; q < Q.size(); q++) { what.push_back({(uint32_t) q, '+'}); patterns.push_back(Q[q].seq); }
    if (!opt.findForwardOnly && opt.findIupac) {
        for (size_t q = 0; q < Q.size(); q++) {
            const std::string r = iupacReverseComplement(Q[q].seq);
            if (r == Q[q].seq) continue;                             // its own reverse complement: searched and reported once, as +
            what.push_back({(uint32_t) q, '-'}); patterns.push_back(r);
        }
    }
    else if (!opt.findForwardOnly) {
        // rc(q0 q1 .. qn) = rc(qn) .. rc(q1) rc(q0): one launch over the queries back to back
        std::string all;
        std::vector<uint64_t> at(1, 0);
        for (const MBGC_Decoder::FindQuery &q : Q) { all += q.seq; at.push_back(all.size()); }
        void *src = nullptr, *dst = nullptr;
        std::string rc(all.size(), '\0');
        const bool ok = !swsem_dev_malloc(D.h, all.size() + 64, &src) && !swsem_dev_malloc(D.h, all.size() + 64, &dst) && !swsem_dev_upload(D.h, src, all.data(), all.size()) &&
                        !swsem_revcomp_dev(D.h, (const uint8_t *) src, all.size(), (uint8_t *) dst) && !swsem_synchronize(D.h) && !swsem_dev_download(D.h, &rc[0], dst, all.size());
        if (!ok) hipFail(msg, "the queries' reverse complements");
        if (src) swsem_dev_free(D.h, src);
        if (dst) swsem_dev_free(D.h, dst);
        if (!ok) return false;
        for (size_t q = 0; q < Q.size(); q++) {
            const std::string r = rc.substr(all.size() - at[q + 1], Q[q].seq.size());
            if (r == Q[q].seq) continue;                             // its own reverse complement: searched and reported once, as +
            what.push_back({(uint32_t) q, '-'}); patterns.push_back(r);
        }
    }
    R.patterns = patterns.size();
    std::string blob;
    std::vector<uint64_t> patOff(1, 0);
    for (const std::string &p : patterns) { blob += p; patOff.push_back(blob.size()); }
    // ---- the records: the chosen contigs, in collection order
    const ChosenRecords in(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = in.recs;
    R.bases = in.bases;
    // ---- the search; the buffer is sized from the bases searched (--hit-capacity: the first size), and the call is made again with
    // the count it states when the hits do not fit
    std::vector<mbgc_fasta_hit_t> hits;
    uint64_t nHits = 0;
    FastaHandle fa;
    uint64_t cap = opt.findHitCapacity ? opt.findHitCapacity : 4096 + R.bases / 256;
    double median[1];
    if (!fa.open(opt.device, msg) || !timedCalls(timed, median, [&](double (&ms)[1]) {
            for (;;) {
                hits.assign(cap, mbgc_fasta_hit_t());
                const int rc = (opt.findIupac ? mbgc_fasta_find_iupac_dev : mbgc_fasta_find_dev)(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), (const uint8_t *) blob.data(),
                                                                                                 patOff.data(), patterns.size(), opt.findMismatches, hits.data(), cap, &nHits, &ms[0]);
                if (rc == -104 && nHits > cap) { cap = nHits; R.retries++; continue; }
                return !rc || faFail(msg, "find");
            }
        })) return false;
    R.kernelMs = median[0];
    hits.resize(nHits);
    if (opt.findIupac) mbgc_fasta_find_iupac_last(fa, &R.tableRows, &R.rowsWalked);
    // ---- --find-host: the same question put to the host, over the downloaded contigs; the two tables must be equal
    if (opt.findHost) {
        std::vector<std::string> text(recs.size());
        for (size_t r = 0; r < recs.size(); r++)
            if (!downloadRecord(D, recs[r], text[r], msg)) return false;
        const double t0 = nowMs();
        const std::vector<HostHit> host = opt.findIupac ? findOnHostIupac(text, patterns, opt.findMismatches) : findOnHost(text, patterns, opt.findMismatches);
        R.hostMs = nowMs() - t0;
        bool same = host.size() == hits.size();
        for (size_t i = 0; same && i < host.size(); i++)
            same = host[i].pos == hits[i].pos && host[i].rec == hits[i].rec && host[i].pattern == hits[i].pattern && host[i].mismatches == hits[i].mismatches;
        if (!same) { msg = "internal error: --find-host: the host's loop finds " + std::to_string(host.size()) + " hits, the device " + std::to_string(hits.size()) + ", or other ones"; return false; }
    }
    // ---- the lines: by file, record, start, query, + before -
    std::set<uint64_t> hitContigs;
    std::set<size_t> hitUnits;
    for (const mbgc_fasta_hit_t &h : hits) {
        const ChosenRecords::Record &w = in.records[h.rec];
        R.lines.push_back({w.contig, h.pos + 1, h.pos + patterns[h.pattern].size(), what[h.pattern].query, what[h.pattern].strand, h.mismatches, w.unit});
        hitContigs.insert(w.contig); hitUnits.insert(w.unit);
    }
    std::sort(R.lines.begin(), R.lines.end(), [](const FindLine &a, const FindLine &b) {
        return std::make_tuple(a.contig, a.start, a.query, a.strand == '-') < std::make_tuple(b.contig, b.start, b.query, b.strand == '-');
    });
    R.records = hitContigs.size(); R.files = hitUnits.size();
    // ---- --primers: query 2 i is pair i's FWD, 2 i + 1 its REV; a primer that is its own reverse complement was searched once and
    // stands on both strands wherever it stands
    if (!opt.findPrimers.empty()) {
        std::vector<bool> ownRc(Q.size(), true);
        for (const Pattern &w : what) if (w.strand == '-') ownRc[w.query] = false;
        std::vector<mbgc_amplicons::Hit> in2;
        for (const mbgc_fasta_hit_t &h : hits) {
            const Pattern &w = what[h.pattern];
            const uint32_t pair = w.query / 2, rev = w.query % 2, len = (uint32_t) patterns[h.pattern].size();
            in2.push_back({h.rec, h.pos, len, pair, 2 * rev + (w.strand == '-'), h.mismatches});
            if (ownRc[w.query]) in2.push_back({h.rec, h.pos, len, pair, 2 * rev + 1, h.mismatches});
        }
        std::set<uint64_t> contigs;
        std::set<size_t> units;
        for (const mbgc_amplicons::Product &a : mbgc_amplicons::pairHits(in2, opt.findMinAmplicon, opt.findMaxAmplicon)) {
            const ChosenRecords::Record &w = in.records[a.rec];      // (the records are the chosen contigs in collection order: sorted by rec is sorted by file, record)
            R.amplicons.push_back({w.contig, a.start + 1, a.end + 1, a.pair, a.strand, a.leftMismatches, a.rightMismatches, w.unit});
            contigs.insert(w.contig); units.insert(w.unit);
        }
        R.ampRecords = contigs.size(); R.ampFiles = units.size();
    }
    return true;
}

// the TSV (stdout, or --hits file), --regions-out, the summary and the JSON line of --bench
bool reportFind(const MBGC_Decoder::Options &opt, const FastaLayout &layout, const FindResult &R, double decodeMs, std::string &msg) {
    const bool primers = !opt.findPrimers.empty();                  // the primers' own hits are printed only with --hits file
    FILE *out = stdout;
    if (!opt.findHitsFile.empty() && !(out = fopen(opt.findHitsFile.c_str(), "w"))) { msg = "cannot write " + opt.findHitsFile; return false; }
    for (const FindLine &l : R.lines)
        if (!primers || out != stdout) fprintf(out, "%s\t%s\t%s\t%llu\t%llu\t%c\t%u\n", opt.findQueries[l.query].name.c_str(), layout.names[l.unit].c_str(), recordName(layout, l.contig).c_str(),
                (unsigned long long) l.start, (unsigned long long) l.end, l.strand, l.mismatches);
    if (out != stdout && fclose(out) != 0) { msg = "cannot write " + opt.findHitsFile; return false; }
    if (!opt.findRegionsOut.empty()) {
        std::string text;
        std::set<std::string> seen;
        for (const FindLine &l : R.lines) {
            const std::string line = recordName(layout, l.contig) + ":" + std::to_string(l.start > opt.findFlank ? l.start - opt.findFlank : 1) + "-" + std::to_string(l.end + opt.findFlank) + "\n";
            if (seen.insert(line).second) text += line;
        }
        if (!writeFile(opt.findRegionsOut, text.data(), text.size())) { msg = "cannot write " + opt.findRegionsOut; return false; }
    }
    if (primers) {
        // by file, record, start, end, pair, + before -: the order pairHits leaves
        for (const AmpliconLine &a : R.amplicons)
            printf("%s\t%s\t%s\t%llu\t%llu\t%c\t%llu\t%u\t%u\n", opt.findPrimers[a.pair].name.c_str(), layout.names[a.unit].c_str(), recordName(layout, a.contig).c_str(),
                   (unsigned long long) a.start, (unsigned long long) a.end, a.strand, (unsigned long long) (a.end - a.start + 1), a.leftMismatches, a.rightMismatches);
        if (!opt.findAmpliconsOut.empty()) {
            std::string text;
            std::set<std::string> seen;
            for (const AmpliconLine &a : R.amplicons) {
                const std::string line = recordName(layout, a.contig) + ":" + std::to_string(a.start) + "-" + std::to_string(a.end) + "\n";
                if (seen.insert(line).second) text += line;
            }
            if (!writeFile(opt.findAmpliconsOut, text.data(), text.size())) { msg = "cannot write " + opt.findAmpliconsOut; return false; }
        }
        printf("amplicons: %zu of %zu primer pairs in %llu records of %llu files; %llu bases searched\n", R.amplicons.size(), opt.findPrimers.size(),
               (unsigned long long) R.ampRecords, (unsigned long long) R.ampFiles, (unsigned long long) R.bases);
    }
    else
        printf("hits: %zu in %llu records of %llu files; %llu bases searched, %llu patterns\n", R.lines.size(), (unsigned long long) R.records, (unsigned long long) R.files,
               (unsigned long long) R.bases, (unsigned long long) R.patterns);
    if (opt.bench) {
        char hostJson[192] = "";
        int at = 0;
        if (opt.findHost) at = snprintf(hostJson, sizeof hostJson, ", \"find_host_ms\": %.3f", R.hostMs);
        if (opt.findIupac) at += snprintf(hostJson + at, sizeof hostJson - at, ", \"rows\": %llu, \"rows_walked\": %llu", (unsigned long long) R.tableRows, (unsigned long long) R.rowsWalked);
        if (primers) snprintf(hostJson + at, sizeof hostJson - at, ", \"amplicons\": %zu", R.amplicons.size());
        printf("{\"find_kernel_ms\": %.3f, \"bases_searched\": %llu, \"patterns\": %llu, \"hits\": %zu, \"retries\": %llu, \"decode_ms\": %.3f, \"find_gb_per_s\": %.3f%s}\n",
               R.kernelMs, (unsigned long long) R.bases, (unsigned long long) R.patterns, R.lines.size(), (unsigned long long) R.retries, decodeMs,
               R.kernelMs > 0 ? R.bases / (R.kernelMs * 1e-3) / 1e9 : 0.0, hostJson);
    }
    return true;
}
}  // namespace
