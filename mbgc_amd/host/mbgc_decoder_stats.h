// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_find.h): `mbgc-hip s` — what the decoded collection holds, asked
// where it lies. The CHOSEN contigs are the records of one mbgc_fasta_stats_dev call over the decoder's sequence buffer
// (contigs that were decoded only because a chosen one depends on them are not counted, as in `f`): eight counters per record and the
// runs of N — of lower case too when --masked-out asks for them — come back; the host sums them per file, takes N50 / L50 over the
// file's record lengths, names the runs by their records and writes the lines.
#pragma once

namespace {
struct StatsResult {
    ChosenRecords in;                                                // the chosen contigs; a chosen file without one has its line all the same
    std::vector<mbgc_fasta_counts_t> counts;                         // per record
    std::vector<mbgc_fasta_run_t> runs;                              // rec = an index into the records; class 0 from 1 byte on, class 1 from --min-masked on
    uint64_t edges = 0, reruns = 0;
    double kernelMs = 0;
};

// --stats-host: the obvious loop over one downloaded contig — its counters, and its runs of both classes by walking them
void statsOnHost(const std::string &text, uint32_t rec, bool lowerRuns, uint64_t minLower, mbgc_fasta_counts_t &c, std::vector<mbgc_fasta_run_t> &runs) {
    c = mbgc_fasta_counts_t{0, 0, 0, 0, 0, 0, 0, 0};
    for (const char ch : text) {
        switch (ch) {
            case 'A': case 'a': c.a++; break;
            case 'C': case 'c': c.c++; break;
            case 'G': case 'g': c.g++; break;
            case 'T': case 't': case 'U': case 'u': c.t++; break;
            case 'N': case 'n': c.n++; break;
            default: c.other++;
        }
        if (ch >= 'a' && ch <= 'z') c.lower++;
    }
    for (uint32_t cls = 0; cls < (lowerRuns ? 2u : 1u); cls++)
        for (size_t p = 0; p < text.size();) {
            const auto in = [&](size_t q) { return cls == 0 ? (text[q] == 'N' || text[q] == 'n') : (text[q] >= 'a' && text[q] <= 'z'); };
            if (!in(p)) { p++; continue; }
            size_t e = p;
            while (e < text.size() && in(e)) e++;
            if (e - p >= (cls == 0 ? 1 : std::max<uint64_t>(minLower, 1))) runs.push_back(mbgc_fasta_run_t{p, e - p, rec, cls});
            p = e;
        }
}

bool collectStats(const DecodedCollection &D, const StreamSet &S, const std::vector<ChosenUnit> &chosen, const MBGC_Decoder::Options &opt, bool timed, StatsResult &R,
                  std::string &msg) {
    R = StatsResult();
    R.in = ChosenRecords(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = R.in.recs;
    // ---- the scan. Runs of N are few and the summary counts them, so they are always asked for, from one byte on (--min-gap is applied
    // where the BED file is written); runs of lower case only for --masked-out. The call is made again with the count it states when
    // the rows do not fit
    const bool lowerRuns = !opt.statsMaskedOut.empty();
    const uint32_t flags = MBGC_FASTA_STATS_COUNTS | MBGC_FASTA_STATS_NRUNS | (lowerRuns ? MBGC_FASTA_STATS_LOWER : 0u);
    std::vector<mbgc_fasta_counts_t> &counts = R.counts;
    counts.resize(std::max<size_t>(recs.size(), 1));
    uint64_t nRuns = 0, cap = 4096;
    FastaHandle fa;
    double median[1];
    if (!fa.open(opt.device, msg) || !timedCalls(timed, median, [&](double (&ms)[1]) {
            for (;;) {
                R.runs.assign(cap, mbgc_fasta_run_t());
                const int rc = mbgc_fasta_stats_dev(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), flags, 1, opt.statsMinMasked, counts.data(), R.runs.data(), cap, &nRuns, &ms[0]);
                if (!rc || rc == -104) { uint64_t e = 0, k = 0; mbgc_fasta_stats_last(fa, &e, &k); R.edges = e; R.reruns += k; }     // (reruns: of all the calls, the first one's as a rule)
                if (rc == -104 && nRuns > cap) { cap = nRuns; continue; }
                return !rc || faFail(msg, "stats");
            }
        })) return false;
    R.kernelMs = median[0];
    R.runs.resize(nRuns);
    counts.resize(recs.size());
    // ---- --stats-host: the same questions put to the host, over the downloaded contigs; everything must be equal
    if (opt.statsHost) {
        std::vector<mbgc_fasta_run_t> hostRuns;
        std::string text;
        for (size_t r = 0; r < recs.size(); r++) {
            if (!downloadRecord(D, recs[r], text, msg)) return false;
            mbgc_fasta_counts_t c;
            statsOnHost(text, (uint32_t) r, lowerRuns, opt.statsMinMasked, c, hostRuns);
            if (memcmp(&c, &counts[r], sizeof c)) { msg = "internal error: --stats-host: the host's loop counts record " + std::to_string(r) + " otherwise than the device"; return false; }
        }
        bool same = hostRuns.size() == R.runs.size();
        for (size_t i = 0; same && i < hostRuns.size(); i++)
            same = hostRuns[i].start == R.runs[i].start && hostRuns[i].len == R.runs[i].len && hostRuns[i].rec == R.runs[i].rec && hostRuns[i].cls == R.runs[i].cls;
        if (!same) { msg = "internal error: --stats-host: the host's loop finds " + std::to_string(hostRuns.size()) + " runs, the device " + std::to_string(R.runs.size()) + ", or other ones"; return false; }
    }
    return true;
}

// a, c, g, t, n, other, lower and GC = (g + c) / (a + c + g + t), 0.000000 without one of the four
std::string statsColumns(const mbgc_fasta_counts_t &c) {
    const uint64_t acgt = c.a + c.c + c.g + c.t;
    char buf[256];
    snprintf(buf, sizeof buf, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6f", (unsigned long long) c.a, (unsigned long long) c.c, (unsigned long long) c.g, (unsigned long long) c.t,
             (unsigned long long) c.n, (unsigned long long) c.other, (unsigned long long) c.lower, acgt ? (double) (c.g + c.c) / (double) acgt : 0.0);
    return buf;
}
void statsAdd(mbgc_fasta_counts_t &sum, const mbgc_fasta_counts_t &c) { sum.a += c.a; sum.c += c.c; sum.g += c.g; sum.t += c.t; sum.n += c.n; sum.other += c.other; sum.lower += c.lower; }

// --records, the per-file lines, --gaps-out / --masked-out (BED), the summary and the JSON line of --bench
bool reportStats(const MBGC_Decoder::Options &opt, const FastaLayout &layout, const StatsResult &R, double decodeMs, std::string &msg) {
    const std::vector<ChosenRecords::Record> &records = R.in.records;
    if (!opt.statsRecordsFile.empty()) {
        std::string text;
        for (size_t r = 0; r < records.size(); r++)
            text += layout.names[records[r].unit] + "\t" + recordName(layout, records[r].contig) + "\t" + std::to_string(records[r].len) + "\t" + statsColumns(R.counts[r]) + "\n";
        if (opt.statsRecordsFile == "-") fputs(text.c_str(), stdout);
        else if (!writeFile(opt.statsRecordsFile, text.data(), text.size())) { msg = "cannot write " + opt.statsRecordsFile; return false; }
    }
    mbgc_fasta_counts_t all = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t at = 0;
    for (const size_t unit : R.in.units) {
        mbgc_fasta_counts_t sum = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<uint64_t> lens;
        uint64_t bases = 0;
        for (; at < records.size() && records[at].unit == unit; at++) { statsAdd(sum, R.counts[at]); lens.push_back(records[at].len); bases += records[at].len; }
        // N50 / L50 over the lengths in descending order: the first record at which twice the running sum reaches the file's bases
        std::sort(lens.begin(), lens.end(), std::greater<uint64_t>());
        uint64_t n50 = 0, l50 = 0, run = 0;
        for (size_t i = 0; bases && i < lens.size(); i++) {
            run += lens[i];
            if (2 * run >= bases) { n50 = lens[i]; l50 = i + 1; break; }
        }
        printf("%s\t%zu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\n", layout.names[unit].c_str(), lens.size(), (unsigned long long) bases, (unsigned long long) (lens.empty() ? 0 : lens.back()),
               (unsigned long long) (lens.empty() ? 0 : lens.front()), (unsigned long long) n50, (unsigned long long) l50, statsColumns(sum).c_str());
        statsAdd(all, sum);
    }
    // BED: record, start (0-based), end (half-open); the runs come sorted by (record, class, start), the records in collection order
    uint64_t runsN = 0;
    std::string gaps, masked;
    for (const mbgc_fasta_run_t &r : R.runs) {
        const std::string line = recordName(layout, records[r.rec].contig) + "\t" + std::to_string(r.start) + "\t" + std::to_string(r.start + r.len) + "\n";
        if (r.cls == 0) { runsN++; if (r.len >= std::max<uint64_t>(opt.statsMinGap, 1)) gaps += line; }
        else masked += line;
    }
    if (!opt.statsGapsOut.empty() && !writeFile(opt.statsGapsOut, gaps.data(), gaps.size())) { msg = "cannot write " + opt.statsGapsOut; return false; }
    if (!opt.statsMaskedOut.empty() && !writeFile(opt.statsMaskedOut, masked.data(), masked.size())) { msg = "cannot write " + opt.statsMaskedOut; return false; }
    const uint64_t acgt = all.a + all.c + all.g + all.t;
    printf("stats: %zu files, %zu records, %llu bases; GC %.6f, N %llu in %llu runs, lower-case %llu, other %llu\n", R.in.units.size(), records.size(), (unsigned long long) R.in.bases,
           acgt ? (double) (all.g + all.c) / (double) acgt : 0.0, (unsigned long long) all.n, (unsigned long long) runsN, (unsigned long long) all.lower, (unsigned long long) all.other);
    if (opt.bench)
        printf("{\"stats_kernel_ms\": %.3f, \"bases\": %llu, \"records\": %zu, \"edges\": %llu, \"edge_reruns\": %llu, \"decode_ms\": %.3f, \"stats_gb_per_s\": %.3f}\n", R.kernelMs,
               (unsigned long long) R.in.bases, records.size(), (unsigned long long) R.edges, (unsigned long long) R.reruns, decodeMs,
               R.kernelMs > 0 ? R.in.bases / (R.kernelMs * 1e-3) / 1e9 : 0.0);
    return true;
}
}  // namespace
