// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_dups.h): `mbgc-hip m` — which genomes of the decoded collection carry
// a query (a gene, a plasmid, a phage) in whatever allele, and where, asked where the collection lies. The queries become
// one strictly ascending list of canonical k-mers (mbgc_screen_loci.h; the command line has held them to the limits before anything was
// decoded); the CHOSEN contigs are the records of one mbgc_fasta_screen_dev call over the decoder's sequence buffer (contigs that were
// decoded only because a chosen one depends on them are not screened, as in `k`), grouped by file, or one group each under --by-record:
// per group the indices of the keys that occur in it come back, and — only when --loci-out or --regions-out asks for them — the hits as
// (position, record, key) rows. The host counts, per query and group, the query's keys among the group's (containment = shared / the
// query's keys), chains a query's hits per record into loci and writes the lines.
#pragma once
#include "mbgc_screen_loci.h"

namespace {
struct ScreenGroup { std::string name; uint64_t records = 0; };
struct ScreenResult {
    mbgc_screen::KeySet keys;
    std::vector<ScreenGroup> groups;                                 // in collection order
    std::vector<uint32_t> found;                                     // group g's keys: found[start[g], start[g + 1]), indices, ascending
    std::vector<uint64_t> start;
    std::vector<mbgc_screen::Locus> loci;                            // rec: the index among the chosen records
    std::vector<ChosenRecords::Record> records;                      // the chosen records, for the loci's names
    uint64_t bases = 0, hits = 0, passes = 0, reruns = 0, slots = 0;
    double kernelMs = 0, sortMs = 0;
};

std::vector<std::string> screenSequences(const MBGC_Decoder::Options &opt) {
    std::vector<std::string> out;
    for (const MBGC_Decoder::FindQuery &q : opt.screenQueries) out.push_back(q.seq);
    return out;
}

bool collectScreen(const DecodedCollection &D, const StreamSet &S, const std::vector<ChosenUnit> &chosen, const FastaLayout &layout, const MBGC_Decoder::Options &opt, bool timed,
                   ScreenResult &R, std::string &msg) {
    R = ScreenResult();
    R.keys = mbgc_screen::buildKeys(screenSequences(opt), opt.screenK);
    const std::vector<uint64_t> &keys = R.keys.keys;
    R.slots = 2;
    while (R.slots < 2 * keys.size()) R.slots <<= 1;                 // (the table of mbgc_fasta_screen_dev: the power of two >= 2 keys)
    // ---- the records: the chosen contigs, in collection order; a group per file (a chosen file without a contig is a group all the
    // same) or per record
    const ChosenRecords in(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = in.recs;
    std::vector<uint32_t> groupOf;
    if (!opt.screenByRecord) for (const size_t unit : in.units) R.groups.push_back(ScreenGroup{layout.names[unit]});
    size_t at = 0;
    for (const ChosenRecords::Record &rec : in.records) {
        if (opt.screenByRecord) { R.groups.push_back(ScreenGroup{recordName(layout, rec.contig)}); at = R.groups.size() - 1; }
        else while (in.units[at] != rec.unit) at++;
        groupOf.push_back((uint32_t) at);
        R.groups[at].records++;
    }
    R.records = in.records; R.bases = in.bases;
    const uint64_t ng = R.groups.size();
    if (ng >= 0xffffffffull) { msg = std::to_string(ng) + " groups in one call"; return false; }
    // ---- the scan. The hit rows are asked for only when the loci are; either call is made again with the count it states when a
    // buffer was too small, a hit buffer only as far as --hit-capacity allows
    const bool wantHits = !opt.screenLociOut.empty() || !opt.screenRegionsOut.empty();
    std::vector<mbgc_fasta_screen_hit_t> hits;
    R.start.assign(ng + 1, 0);
    uint64_t total = 0, nHits = 0, cap = 1 << 16, hitCap = wantHits ? 4096 + R.bases / 256 : 0;
    if (wantHits && opt.screenHitCapacity) hitCap = std::min(hitCap, opt.screenHitCapacity);
    FastaHandle fa;
    double median[2];                                                // the scan, the sorts
    if (!fa.open(opt.device, msg) || !timedCalls(timed, median, [&](double (&ms)[2]) {
            for (;;) {
                R.found.assign(cap, 0);
                if (wantHits) hits.assign(hitCap, mbgc_fasta_screen_hit_t());
                const int rc = mbgc_fasta_screen_dev(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), groupOf.data(), (uint32_t) ng, opt.screenK, keys.data(), keys.size(),
                                                     R.found.data(), cap, R.start.data(), &total, wantHits ? hits.data() : nullptr, hitCap, &nHits, &ms[0]);
                if (!rc || rc == -104) { uint64_t k = 0; mbgc_fasta_screen_last(fa, nullptr, &R.passes, &k, &ms[1]); R.reruns += k; }
                if (rc == -104 && total > cap) { cap = total; continue; }
                if (rc == -104 && wantHits && nHits > hitCap) {
                    if (opt.screenHitCapacity && nHits > opt.screenHitCapacity) {
                        msg = std::to_string(nHits) + " hits, --hit-capacity allows " + std::to_string(opt.screenHitCapacity) + ": raise it, or screen with fewer or shorter queries";
                        return false;
                    }
                    hitCap = nHits;
                    continue;
                }
                if (rc) return faFail(msg, "screen");
                return true;
            }
        })) return false;
    R.kernelMs = median[0]; R.sortMs = median[1];
    R.found.resize(total);
    R.hits = nHits;
    if (wantHits) hits.resize(nHits);
    // ---- --screen-host: the same questions put to the host, over the downloaded contigs; everything must be equal
    if (opt.screenHost) {
        const std::set<uint64_t> keySet(keys.begin(), keys.end());
        std::vector<std::set<uint32_t>> hostFound(ng);
        std::vector<mbgc_fasta_screen_hit_t> hostHits;
        std::string text;
        for (size_t r = 0; r < recs.size(); r++) {
            if (!downloadRecord(D, recs[r], text, msg)) return false;
            std::vector<uint64_t> positions;
            const std::vector<uint64_t> canons = mbgc_screen::canonsOf(text, opt.screenK, &positions);
            for (size_t i = 0; i < canons.size(); i++) {
                if (!keySet.count(canons[i])) continue;
                const uint32_t key = (uint32_t) (std::lower_bound(keys.begin(), keys.end(), canons[i]) - keys.begin());
                hostFound[groupOf[r]].insert(key);
                hostHits.push_back(mbgc_fasta_screen_hit_t{positions[i], (uint32_t) r, key});
            }
        }
        bool same = hostHits.size() == nHits;
        for (uint64_t g = 0; same && g < ng; g++)
            same = std::vector<uint32_t>(hostFound[g].begin(), hostFound[g].end()) == std::vector<uint32_t>(R.found.begin() + R.start[g], R.found.begin() + R.start[g + 1]);
        for (size_t i = 0; same && wantHits && i < hits.size(); i++) same = hostHits[i].pos == hits[i].pos && hostHits[i].rec == hits[i].rec && hostHits[i].key == hits[i].key;
        if (!same) {
            msg = "internal error: --screen-host: the host's loops find " + std::to_string(hostHits.size()) + " hits, the device " + std::to_string(nHits) + ", or other keys or places";
            return false;
        }
    }
    if (wantHits) {
        std::vector<mbgc_screen::Hit> in2;
        for (const mbgc_fasta_screen_hit_t &h : hits) in2.push_back({h.rec, h.pos, h.key});
        R.loci = mbgc_screen::chainLoci(in2, R.keys, opt.screenK, opt.screenMaxGap, opt.screenMinLocusHits);
    }
    return true;
}

// the pair lines, --loci-out, --regions-out, the summary and the JSON line of --bench; pairs: the lines written
bool reportScreen(const MBGC_Decoder::Options &opt, const FastaLayout &layout, const ScreenResult &R, double decodeMs, uint64_t &pairs, std::string &msg) {
    const size_t nq = opt.screenQueries.size(), ng = R.groups.size();
    // shared[q][g]: every found key of group g counts for each query that holds it
    std::vector<std::vector<uint64_t>> shared(nq, std::vector<uint64_t>(ng, 0));
    for (size_t g = 0; g < ng; g++)
        for (uint64_t i = R.start[g]; i < R.start[g + 1]; i++)
            for (uint64_t j = R.keys.start[R.found[i]]; j < R.keys.start[R.found[i] + 1]; j++) shared[R.keys.queries[j]][g]++;
    pairs = 0;
    for (size_t q = 0; q < nq; q++)
        for (size_t g = 0; g < ng; g++) {
            const uint64_t s = shared[q][g], n = R.keys.queryKeys[q];
            const double c = n ? (double) s / (double) n : 0.0;
            if (s < opt.screenMinShared || c < opt.screenMinContainment) continue;
            printf("%s\t%s\t%llu\t%llu\t%.6f\n", opt.screenQueries[q].name.c_str(), R.groups[g].name.c_str(), (unsigned long long) n, (unsigned long long) s, c);
            pairs++;
        }
    if (!opt.screenLociOut.empty()) {
        std::string text;
        for (const mbgc_screen::Locus &l : R.loci) {
            const ChosenRecords::Record &w = R.records[l.rec];
            text += opt.screenQueries[l.query].name + "\t" + layout.names[w.unit] + "\t" + recordName(layout, w.contig) + "\t" + std::to_string(l.start + 1) + "\t" + std::to_string(l.end + 1) +
                    "\t" + std::to_string(l.hits) + "\t" + std::to_string(l.distinct) + "\n";
        }
        if (!writeFile(opt.screenLociOut, text.data(), text.size())) { msg = "cannot write " + opt.screenLociOut; return false; }
    }
    if (!opt.screenRegionsOut.empty()) {
        std::string text;
        std::set<std::string> seen;
        for (const mbgc_screen::Locus &l : R.loci) {
            const std::string line = mbgc_screen::regionLine(recordName(layout, R.records[l.rec].contig), l.start, l.end, opt.screenFlank);
            if (seen.insert(line).second) text += line;
        }
        if (!writeFile(opt.screenRegionsOut, text.data(), text.size())) { msg = "cannot write " + opt.screenRegionsOut; return false; }
    }
    printf("screen: %zu queries, %zu distinct k-mers, k %u; %zu groups, %zu records, %llu bases; %llu hits, %llu pairs reported\n", nq, R.keys.keys.size(), opt.screenK, ng, R.records.size(),
           (unsigned long long) R.bases, (unsigned long long) R.hits, (unsigned long long) pairs);
    if (opt.bench)
        printf("{\"screen_kernel_ms\": %.3f, \"sort_ms\": %.3f, \"bases\": %llu, \"keys\": %zu, \"table_slots\": %llu, \"filter_passes\": %llu, \"hits\": %llu, \"hit_reruns\": %llu, "
               "\"decode_ms\": %.3f, \"screen_gb_per_s\": %.3f}\n", R.kernelMs, R.sortMs, (unsigned long long) R.bases, R.keys.keys.size(), (unsigned long long) R.slots,
               (unsigned long long) R.passes, (unsigned long long) R.hits, (unsigned long long) R.reruns, decodeMs, R.kernelMs > 0 ? R.bases / (R.kernelMs * 1e-3) / 1e9 : 0.0);
    return true;
}
}  // namespace
