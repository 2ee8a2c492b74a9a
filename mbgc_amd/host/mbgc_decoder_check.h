// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_fasta.h): `d --check` and `t` — the decoded collection held
// against <prefix>.checksums (mbgc_checksums.h) where it lies. The CRC-32 of every CHOSEN contig is taken on the device
// (mbgc_fasta_crc_dev over the decoder's sequence buffer: one launch, nothing is downloaded) and compared with the manifest's entry;
// contigs that were decoded only because a chosen one depends on them are not looked at, so the report is a function of the selection
// alone. The four side files are a few KB and are summed on the host.
#pragma once

namespace {
struct CheckResult {
    uint64_t checked = 0, total = 0, bad = 0, bytes = 0;
    double kernelMs = 0;
    std::vector<std::string> lines;                                // the `checksum ERROR` lines, side files first
    bool differs() const { return bad != 0 || !lines.empty(); }
};

// the manifest, held to the set: false and d's message (exit 1)
bool readManifest(const std::string &prefix, const StreamSet &S, mbgc_checksums::Manifest &M, std::string &msg) {
    std::string bytes, why;
    if (!readFile(prefix + ".checksums", bytes)) { msg = prefix + ".checksums not found: write it with mbgc-hip c --checksums"; return false; }
    if (!M.parse(bytes, &why)) { msg = "malformed " + prefix + ".checksums: " + why; return false; }
    const uint64_t N = S.planned + (S.meta.sequentialMatching ? 0 : S.g0n);
    if (M.contigs.size() != N) {
        msg = "malformed " + prefix + ".checksums: it lists " + std::to_string(M.contigs.size()) + " contigs, the stream set holds " + std::to_string(N);
        return false;
    }
    return true;
}

bool checkChecksums(const std::string &prefix, const DecodedCollection &D, const StreamSet &S, const FastaLayout &layout, const std::vector<ChosenUnit> &chosen,
                    const mbgc_checksums::Manifest &M, int device, CheckResult &R, std::string &msg) {
    R = CheckResult();
    R.total = M.contigs.size();
    for (int k = 0; k < 4; k++) {
        std::string bytes;
        const bool have = readFile(prefix + "." + mbgc_checksums::SIDE_EXT[k], bytes);
        if ((have ? mbgc_checksums::crc32(bytes.data(), bytes.size()) : 0u) != M.side[k])
            R.lines.push_back("checksum ERROR: " + prefix + "." + mbgc_checksums::SIDE_EXT[k] + " differs");
    }
    const uint64_t shift = S.meta.sequentialMatching ? S.g0n : 0;   // (-t1: the initial reference has no entry of its own and is never chosen)
    const ChosenRecords in(D, S, chosen);
    const std::vector<mbgc_fasta_crc_rec_t> &recs = in.recs;
    std::vector<uint64_t> unitFirst(S.T() + 2, 0);
    unitFirst[1] = S.g0n;
    for (size_t t = 0; t < S.T(); t++) unitFirst[t + 2] = unitFirst[t + 1] + S.seqCount[t];
    R.bytes = in.bases;
    R.checked = recs.size();
    std::vector<uint32_t> got(recs.size());
    if (!recs.empty()) {
        FastaHandle fa;
        if (!fa.open(device, msg)) return false;
        if (mbgc_fasta_crc_dev(fa, D.seqDev, D.totalBases, recs.data(), recs.size(), got.data(), &R.kernelMs)) return faFail(msg, "checksums");
    }
    for (size_t i = 0; i < recs.size(); i++) {
        const uint64_t k = in.records[i].contig;
        const uint32_t want = M.contigs[k - shift];
        if (got[i] == want) continue;
        if (R.bad++ >= 100) continue;
        const size_t unit = in.records[i].unit;                      // (0 for a single-FASTA set, whose records count from the first planned contig)
        const std::string &name = layout.names[unit];
        char hex[64];
        snprintf(hex, sizeof hex, "expected %08x got %08x", want, got[i]);
        R.lines.push_back("checksum ERROR: contig " + std::to_string(k - shift) + " (file " + name + ", record " + std::to_string(S.meta.singleFastaFile ? k - shift : k - unitFirst[unit]) + ": " +
                          layout.headers.substr(layout.hdrOff[k], std::min<uint64_t>(layout.hdrLen[k], 60)) + ") " + hex);
    }
    return true;
}

void reportCheck(const CheckResult &R) {
    printf("checksums: %llu of %llu contigs checked, %llu differ\n", (unsigned long long) R.checked, (unsigned long long) R.total, (unsigned long long) R.bad);
    for (const std::string &l : R.lines) printf("%s\n", l.c_str());
}
}  // namespace
