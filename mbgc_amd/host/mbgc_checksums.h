// <prefix>.checksums: the manifest `mbgc-hip c --checksums` / `r --checksums` write beside a stream set and `d --check` / `t` hold
// it against. Little-endian: 8 bytes "MBGCCRC1", u64 contig count N, four u32 — zlib's CRC-32 of <prefix>.meta, .names, .headers,
// .dnaLineLengths as written (0 for a file the run does not write) —, then N u32: the CRC-32 of every contig's bases in the order
// of <out>.contigLens of an unselected `mbgc-hip d` (the initial reference's contigs first; under -t1 it is target 0's first contig
// again and has no entry of its own). The bases are those the streams hold: after -U, after the lossy rule.
// The contigs' CRCs come from the device (mbgc_fasta_crc_dev); the few KB of the side files are summed here.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace mbgc_checksums {
static const char MAGIC[9] = "MBGCCRC1";
static const char *const SIDE_EXT[4] = {"meta", "names", "headers", "dnaLineLengths"};

inline uint32_t crc32(const void *data, size_t n) {
    static uint32_t table[256];
    static bool ready = false;
    if (!ready) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            table[i] = c;
        }
        ready = true;
    }
    uint32_t r = 0xffffffffu;
    const uint8_t *p = (const uint8_t *) data;
    for (size_t i = 0; i < n; i++) r = table[(r ^ p[i]) & 255u] ^ (r >> 8);
    return ~r;
}

struct Manifest {
    uint32_t side[4] = {0, 0, 0, 0};
    std::vector<uint32_t> contigs;

    std::string serialize() const {
        std::string s(MAGIC, 8);
        const uint64_t n = contigs.size();
        s.append((const char *) &n, sizeof n);
        s.append((const char *) side, sizeof side);
        s.append((const char *) contigs.data(), contigs.size() * sizeof(uint32_t));
        return s;
    }
    // false: *why says what is wrong with the bytes
    bool parse(const std::string &s, std::string *why) {
        if (s.size() < 8 + sizeof(uint64_t) + sizeof side || memcmp(s.data(), MAGIC, 8) != 0) { *why = "it does not start with MBGCCRC1 and a header"; return false; }
        uint64_t n = 0;
        memcpy(&n, s.data() + 8, sizeof n);
        const size_t head = 8 + sizeof n + sizeof side;
        if (n > (s.size() - head) / sizeof(uint32_t) || s.size() != head + n * sizeof(uint32_t)) {
            *why = "it states " + std::to_string(n) + " contigs and holds " + std::to_string((s.size() - head) / sizeof(uint32_t)) + " entries";
            return false;
        }
        memcpy(side, s.data() + 8 + sizeof n, sizeof side);
        contigs.resize((size_t) n);
        if (n) memcpy(contigs.data(), s.data() + head, (size_t) n * sizeof(uint32_t));
        return true;
    }
};
}  // namespace mbgc_checksums
