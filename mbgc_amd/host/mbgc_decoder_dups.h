// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_sketch.h): `mbgc-hip u` — which records of the decoded collection
// are the same sequence, read forward or as the reverse complement, asked where it lies. The CHOSEN contigs are the
// records of one mbgc_fasta_dups_dev call over the decoder's sequence buffer (contigs that were decoded only because a chosen one
// depends on them are not classed, as in `s`): per record the lowest record of its class and the strand come back, exact. The host names
// the records, writes the lines and compares the files by the classes of their records.
#pragma once

namespace {
struct DupsResult {
    ChosenRecords in;                                                // the chosen contigs and files
    std::vector<mbgc_fasta_dup_t> dup;                               // per record: rep = an index into the records
    uint64_t classes = 0, buckets = 0, verified = 0, refuted = 0;
    double kernelMs = 0, verifyMs = 0;
};

// --dups-host: the classes of the downloaded contigs by a map over canonical strings — the smaller of the folded text and its reverse
// complement —, the representative the first record with that string, the strand by comparing with the representative itself
void dupsOnHost(const std::vector<std::string> &texts, bool forwardOnly, bool exactCase, std::vector<mbgc_fasta_dup_t> &out) {
    const uint8_t *comp = mbgc_fasta_dups_comp_table();
    std::vector<std::string> folded(texts.size());
    std::map<std::string, uint32_t> first;
    out.assign(texts.size(), mbgc_fasta_dup_t{0, 0});
    for (size_t r = 0; r < texts.size(); r++) {
        std::string &f = folded[r];
        f = texts[r];
        if (!exactCase) for (char &ch : f) if ((ch >= 'a' && ch <= 'z')) ch = (char) (ch & 0xDF);
        std::string rc(f.rbegin(), f.rend());
        for (char &ch : rc) ch = (char) comp[(uint8_t) ch];
        const std::string &key = forwardOnly || f <= rc ? f : rc;
        const uint32_t rep = first.emplace(key, (uint32_t) r).first->second;
        out[r] = mbgc_fasta_dup_t{rep, f == folded[rep] ? 0u : 1u};
    }
}

bool collectDups(const DecodedCollection &D, const StreamSet &S, const std::vector<ChosenUnit> &chosen, const MBGC_Decoder::Options &opt, bool timed, DupsResult &R,
                 std::string &msg) {
    R = DupsResult();
    R.in = ChosenRecords(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = R.in.recs;
    const uint32_t flags = (opt.dupsForwardOnly ? MBGC_FASTA_DUPS_FORWARD_ONLY : 0u) | (opt.dupsExactCase ? MBGC_FASTA_DUPS_EXACT_CASE : 0u);
    R.dup.assign(std::max<size_t>(recs.size(), 1), mbgc_fasta_dup_t{0, 0});
    FastaHandle fa;
    double median[2];                                                // the scan, the exactness step
    if (!fa.open(opt.device, msg) || !timedCalls(timed, median, [&](double (&ms)[2]) {
            if (mbgc_fasta_dups_dev(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), flags, R.dup.data(), &R.classes, &ms[0])) return faFail(msg, "dups");
            mbgc_fasta_dups_last(fa, &R.buckets, &R.verified, &R.refuted, &ms[1]);
            return true;
        })) return false;
    R.kernelMs = median[0]; R.verifyMs = median[1];
    R.dup.resize(recs.size());
    // ---- --dups-host: the same question put to the host, over the downloaded contigs; every answer must be equal
    if (opt.dupsHost) {
        std::vector<std::string> texts(recs.size());
        for (size_t r = 0; r < recs.size(); r++)
            if (!downloadRecord(D, recs[r], texts[r], msg)) return false;
        std::vector<mbgc_fasta_dup_t> host;
        dupsOnHost(texts, opt.dupsForwardOnly, opt.dupsExactCase, host);
        for (size_t r = 0; r < recs.size(); r++)
            if (host[r].rep != R.dup[r].rep || host[r].strand != R.dup[r].strand) {
                msg = "internal error: --dups-host: record " + std::to_string(r) + " is (" + std::to_string(host[r].rep) + ", " + std::to_string(host[r].strand) +
                      ") by the host's map and (" + std::to_string(R.dup[r].rep) + ", " + std::to_string(R.dup[r].strand) + ") by the device";
                return false;
            }
    }
    return true;
}

// the duplicates' lines, --clusters-out, --unique-files-out, the summary and the JSON line of --bench
bool reportDups(const MBGC_Decoder::Options &opt, const FastaLayout &layout, const DupsResult &R, double decodeMs, std::string &msg) {
    const uint64_t least = std::max<uint64_t>(opt.dupsMinLen, 1);
    const std::vector<ChosenRecords::Record> &records = R.in.records;
    const auto columns = [&](size_t r) {
        const size_t rep = R.dup[r].rep;
        return recordName(layout, records[r].contig) + "\t" + layout.names[records[r].unit] + "\t" + std::to_string(records[r].len) + "\t" + (R.dup[r].strand ? "-" : "+") + "\t" +
               recordName(layout, records[rep].contig) + "\t" + layout.names[records[rep].unit];
    };
    uint64_t dups = 0, dupBases = 0, asRc = 0;
    std::vector<std::vector<size_t>> members(records.size());     // of a class, under its representative, in collection order
    for (size_t r = 0; r < records.size(); r++) {
        if (records[r].len < least) continue;
        members[R.dup[r].rep].push_back(r);
        if (R.dup[r].rep == r) continue;
        printf("%s\n", columns(r).c_str());
        dups++; dupBases += records[r].len; asRc += R.dup[r].strand;
    }
    if (!opt.dupsClustersOut.empty()) {
        std::string text;
        uint64_t number = 0;
        for (size_t rep = 0; rep < members.size(); rep++) {
            if (members[rep].size() < 2) continue;
            number++;
            for (const size_t r : members[rep]) text += columns(r) + "\t" + std::to_string(number) + "\n";
        }
        if (!writeFile(opt.dupsClustersOut, text.data(), text.size())) { msg = "cannot write " + opt.dupsClustersOut; return false; }
    }
    // a file is a duplicate of an earlier one when the sorted lists of their records' classes are equal (every record counts, whatever
    // its length and strand)
    std::map<std::vector<uint32_t>, size_t> seen;
    std::string unique;
    uint64_t dupFiles = 0;
    size_t at = 0;
    for (const size_t unit : R.in.units) {
        std::vector<uint32_t> classes;
        for (; at < records.size() && records[at].unit == unit; at++) classes.push_back(R.dup[at].rep);
        std::sort(classes.begin(), classes.end());
        if (seen.emplace(classes, unit).second) unique += layout.names[unit] + "\n"; else dupFiles++;
    }
    if (!opt.dupsUniqueFilesOut.empty() && !writeFile(opt.dupsUniqueFilesOut, unique.data(), unique.size())) { msg = "cannot write " + opt.dupsUniqueFilesOut; return false; }
    printf("dups: %zu records, %llu bases; %llu distinct sequences; %llu duplicate records, %llu bases (%llu as reverse complements); %llu of %zu files duplicate\n", records.size(),
           (unsigned long long) R.in.bases, (unsigned long long) R.classes, (unsigned long long) dups, (unsigned long long) dupBases, (unsigned long long) asRc, (unsigned long long) dupFiles,
           R.in.units.size());
    if (opt.bench)
        printf("{\"dups_kernel_ms\": %.3f, \"verify_ms\": %.3f, \"bases\": %llu, \"records\": %zu, \"buckets\": %llu, \"verified\": %llu, \"refuted\": %llu, \"decode_ms\": %.3f, "
               "\"dups_gb_per_s\": %.3f}\n", R.kernelMs, R.verifyMs, (unsigned long long) R.in.bases, records.size(), (unsigned long long) R.buckets, (unsigned long long) R.verified,
               (unsigned long long) R.refuted, decodeMs, R.kernelMs > 0 ? R.in.bases / (R.kernelMs * 1e-3) / 1e9 : 0.0);
    return true;
}
}  // namespace
