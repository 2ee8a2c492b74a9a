// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_stats.h): `mbgc-hip k` — which genomes of the decoded collection
// are close to which, asked where it lies. The CHOSEN contigs are the records of one mbgc_fasta_sketch_dev call over the
// decoder's sequence buffer (contigs that were decoded only because a chosen one depends on them are not sketched, as in `s`), grouped
// by file, or one group each under --by-record: the groups' FracMinHash sketches and k-mer counts come back; one
// mbgc_fasta_sketch_pairs_dev call answers |A & B| for all pairs of groups; the host derives Jaccard, containments and distance in
// double and writes the lines. The hash is the project's own (include/mbgc_fasta.h), not Mash's or sourmash's.
#pragma once

namespace {
struct SketchGroup { std::string name; uint64_t records = 0, bases = 0, kmers = 0; };
struct SketchResult {
    std::vector<SketchGroup> groups;                                 // in collection order
    std::vector<uint64_t> hashes, start;                             // group g's sketch: hashes[start[g], start[g + 1])
    std::vector<uint32_t> shared;                                    // all pairs i < j in row-major order (empty under --no-pairs)
    uint64_t records = 0, bases = 0, rows = 0, reruns = 0;
    double kernelMs = 0, sortMs = 0, pairsMs = 0;
};

// --sketch-host: the hash of every k-mer of one downloaded contig by the obvious loop — each k-mer from scratch, its reverse complement
// by walking it backwards
void sketchOnHost(const std::string &text, uint32_t k, uint64_t maxHash, std::set<uint64_t> &kept, uint64_t &kmers) {
    const auto code = [](char ch) { switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return -1; } };
    for (size_t p = 0; p + k <= text.size(); p++) {
        uint64_t fw = 0, rc = 0;
        bool ok = true;
        for (uint32_t i = 0; i < k && ok; i++) {
            const int f = code(text[p + i]), b = code(text[p + k - 1 - i]);
            ok = f >= 0 && b >= 0;
            fw = (fw << 2) | (uint64_t) (f & 3);
            rc = (rc << 2) | (uint64_t) (3 - (b & 3));
        }
        if (!ok) continue;
        kmers++;
        uint64_t x = std::min(fw, rc) ^ 0x9E3779B97F4A7C15ull;
        x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
        if (x <= maxHash) kept.insert(x);
    }
}

bool collectSketch(const DecodedCollection &D, const StreamSet &S, const std::vector<ChosenUnit> &chosen, const FastaLayout &layout, const MBGC_Decoder::Options &opt, bool timed,
                   SketchResult &R, std::string &msg) {
    R = SketchResult();
    // ---- the records: the chosen contigs, in collection order; a group per file (a chosen file without a contig has its line all the
    // same) or per record
    const ChosenRecords in(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = in.recs;
    std::vector<uint32_t> groupOf;
    if (!opt.sketchByRecord) for (const size_t unit : in.units) R.groups.push_back(SketchGroup{layout.names[unit]});
    size_t at = 0;
    for (const ChosenRecords::Record &rec : in.records) {
        if (opt.sketchByRecord) { R.groups.push_back(SketchGroup{recordName(layout, rec.contig)}); at = R.groups.size() - 1; }
        else while (in.units[at] != rec.unit) at++;
        groupOf.push_back((uint32_t) at);
        R.groups[at].records++;
        R.groups[at].bases += rec.len;
    }
    R.records = in.size(); R.bases = in.bases;
    const uint64_t ng = R.groups.size(), npairs = opt.sketchNoPairs ? 0 : ng * (ng ? ng - 1 : 0) / 2;
    if (ng >= 0xffffffffull || npairs > ((uint64_t) 1 << 28)) {
        msg = std::to_string(ng) + " groups are " + std::to_string(npairs) + " pairs, more than 2^28: sketch without the pairs (--no-pairs) or choose fewer groups (--select)";
        return false;
    }
    const uint64_t maxHash = ~(uint64_t) 0 / opt.sketchScale;
    // ---- the scan, the sort and the pairs. The call is made again with the count it states when the hashes do not fit
    std::vector<uint64_t> kmers(std::max<uint64_t>(ng, 1));
    R.start.assign(ng + 1, 0);
    R.shared.assign(npairs, 0);
    uint64_t total = 0, cap = 1 << 16;
    FastaHandle fa;
    double median[3];                                                // the scan, the sort, the pairs
    if (!fa.open(opt.device, msg) || !timedCalls(timed, median, [&](double (&ms)[3]) {
            for (;;) {
                R.hashes.assign(cap, 0);
                const int rc = mbgc_fasta_sketch_dev(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), groupOf.data(), (uint32_t) ng, opt.sketchK, maxHash, R.hashes.data(), cap,
                                                     R.start.data(), kmers.data(), &total, &ms[0]);
                if (!rc || rc == -104) { uint64_t rows = 0, k = 0; mbgc_fasta_sketch_last(fa, &rows, &k); R.rows = rows; R.reruns += k; }     // (reruns: of all the calls, the first one's as a rule)
                if (rc == -104 && total > cap) { cap = total; continue; }
                if (rc) return faFail(msg, "sketch");
                break;
            }
            ms[1] = mbgc_fasta_sketch_sort_ms(fa);
            return !npairs || !mbgc_fasta_sketch_pairs_dev(fa, R.hashes.data(), R.start.data(), (uint32_t) ng, nullptr, npairs, R.shared.data(), &ms[2]) || faFail(msg, "pairs");
        })) return false;
    R.kernelMs = median[0]; R.sortMs = median[1]; R.pairsMs = median[2];
    R.hashes.resize(total);
    for (uint64_t g = 0; g < ng; g++) R.groups[g].kmers = kmers[g];
    // ---- --sketch-host: the same questions put to the host, over the downloaded contigs; everything must be equal
    if (opt.sketchHost) {
        std::vector<std::set<uint64_t>> kept(ng);
        std::vector<uint64_t> hostKmers(ng, 0);
        std::string text;
        for (size_t r = 0; r < recs.size(); r++) {
            if (!downloadRecord(D, recs[r], text, msg)) return false;
            sketchOnHost(text, opt.sketchK, maxHash, kept[groupOf[r]], hostKmers[groupOf[r]]);
        }
        for (uint64_t g = 0; g < ng; g++) {
            const std::vector<uint64_t> list(kept[g].begin(), kept[g].end());
            if (hostKmers[g] != kmers[g] || list != std::vector<uint64_t>(R.hashes.begin() + R.start[g], R.hashes.begin() + R.start[g + 1])) {
                msg = "internal error: --sketch-host: the host's loop sketches group " + std::to_string(g) + " (" + R.groups[g].name + ") otherwise than the device";
                return false;
            }
        }
        uint64_t q = 0;
        for (uint64_t i = 0; i < ng && npairs; i++)
            for (uint64_t j = i + 1; j < ng; j++, q++) {
                uint64_t both = 0;
                for (const uint64_t h : kept[i]) both += kept[j].count(h);
                if (both != R.shared[q]) {
                    msg = "internal error: --sketch-host: groups " + std::to_string(i) + " and " + std::to_string(j) + " share " + std::to_string(both) + " hashes on the host, " +
                          std::to_string(R.shared[q]) + " on the device";
                    return false;
                }
            }
    }
    return true;
}

// the group lines, the pair lines (stdout or --pairs-out), --sketches-out, --order-out, the summary and the JSON line of --bench
bool reportSketch(const MBGC_Decoder::Options &opt, const SketchResult &R, double decodeMs, std::string &msg) {
    const size_t ng = R.groups.size();
    const auto size = [&](size_t g) { return R.start[g + 1] - R.start[g]; };
    uint64_t kmers = 0;
    for (size_t g = 0; g < ng; g++) {
        const SketchGroup &G = R.groups[g];
        printf("%s\t%llu\t%llu\t%llu\t%llu\t%llu\n", G.name.c_str(), (unsigned long long) G.records, (unsigned long long) G.bases, (unsigned long long) G.kmers, (unsigned long long) size(g),
               (unsigned long long) (size(g) * opt.sketchScale));
        kmers += G.kmers;
    }
    // J = shared / (a + b - shared); containments shared / a, shared / b; D = 1 when J = 0, else max(0, -ln(2 J / (1 + J)) / k)
    uint64_t sharing = 0, q = 0;
    std::string pairs;
    std::vector<uint64_t> sum(ng, 0);
    for (size_t i = 0; i < ng && !opt.sketchNoPairs; i++)
        for (size_t j = i + 1; j < ng; j++, q++) {
            const uint64_t a = size(i), b = size(j), s = R.shared[q];
            sharing += s > 0;
            sum[i] += s; sum[j] += s;
            if (s < opt.sketchMinShared) continue;
            const double J = a + b - s ? (double) s / (double) (a + b - s) : 0.0;
            double dist = J > 0 ? -std::log(2 * J / (1 + J)) / opt.sketchK : 1.0;
            if (!(dist > 0)) dist = 0.0;                             // (never -0.000000)
            char buf[160];
            snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%.6f\t%.6f\t%.6f\t%.6f\n", (unsigned long long) a, (unsigned long long) b, (unsigned long long) s, J, a ? (double) s / (double) a : 0.0,
                     b ? (double) s / (double) b : 0.0, dist);
            pairs += R.groups[i].name + "\t" + R.groups[j].name + buf;
        }
    if (opt.sketchPairsOut.empty()) fputs(pairs.c_str(), stdout);
    else if (!writeFile(opt.sketchPairsOut, pairs.data(), pairs.size())) { msg = "cannot write " + opt.sketchPairsOut; return false; }
    if (!opt.sketchOut.empty()) {
        std::string text;
        char buf[24];
        for (size_t g = 0; g < ng; g++) {
            text += R.groups[g].name + "\t" + std::to_string(opt.sketchK) + "\t" + std::to_string(opt.sketchScale) + "\t" + std::to_string(size(g)) + "\t";
            for (uint64_t i = R.start[g]; i < R.start[g + 1]; i++) { snprintf(buf, sizeof buf, i == R.start[g] ? "%016llx" : ",%016llx", (unsigned long long) R.hashes[i]); text += buf; }
            text += "\n";
        }
        if (!writeFile(opt.sketchOut, text.data(), text.size())) { msg = "cannot write " + opt.sketchOut; return false; }
    }
    // --order-out: a file list for `mbgc-hip c`. First the group that shares the most with all others (the earliest of equals), then the
    // others by what they share with it, descending (collection order among equals)
    if (!opt.sketchOrderOut.empty()) {
        size_t first = 0;
        for (size_t g = 1; g < ng; g++) if (sum[g] > sum[first]) first = g;
        const auto with = [&](size_t g) { const size_t i = std::min(g, first), j = std::max(g, first); return R.shared[i * (2 * ng - i - 1) / 2 + (j - i - 1)]; };     // (row i of the pairs starts at i (2 n - i - 1) / 2)
        std::vector<size_t> order;
        for (size_t g = 0; g < ng; g++) if (g != first) order.push_back(g);
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return with(x) > with(y); });
        std::string text = ng ? R.groups[first].name + "\n" : std::string();
        for (const size_t g : order) text += R.groups[g].name + "\n";
        if (!writeFile(opt.sketchOrderOut, text.data(), text.size())) { msg = "cannot write " + opt.sketchOrderOut; return false; }
    }
    printf("sketch: %zu groups, %llu records, %llu bases; k %u, scale %llu; %zu hashes of %llu k-mers, %llu pairs, %llu share a hash\n", ng, (unsigned long long) R.records,
           (unsigned long long) R.bases, opt.sketchK, (unsigned long long) opt.sketchScale, R.hashes.size(), (unsigned long long) kmers, (unsigned long long) R.shared.size(),
           (unsigned long long) sharing);
    if (opt.bench)
        printf("{\"sketch_kernel_ms\": %.3f, \"pairs_kernel_ms\": %.3f, \"sort_ms\": %.3f, \"bases\": %llu, \"rows\": %llu, \"row_reruns\": %llu, \"hashes\": %zu, \"pairs\": %zu, "
               "\"decode_ms\": %.3f, \"sketch_gb_per_s\": %.3f}\n", R.kernelMs, R.pairsMs, R.sortMs, (unsigned long long) R.bases, (unsigned long long) R.rows, (unsigned long long) R.reruns,
               R.hashes.size(), R.shared.size(), decodeMs, R.kernelMs > 0 ? R.bases / (R.kernelMs * 1e-3) / 1e9 : 0.0);
    return true;
}
}  // namespace
