// `mbgc-hip m`: the queries' k-mer keys, and the hits of one query chained into loci. Plain vectors in, plain vectors out, no decoder type
// and no device: tests/screen_loci_main.cpp compiles this header alone.
// Keys. A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3, every other byte is invalid; a k-mer with an invalid byte has no key; the key of a valid
// one is min(fw, rc), fw = the codes as a number, the first base in the highest pair of 2 k bits, rc = the same of the reverse
// complement (the canonical word of include/mbgc_fasta.h — no hash). A query's keys are its distinct ones; the call's key list is the
// strictly ascending union, and queriesOf(i) names the queries that hold key i (alleles of one gene share most keys).
// Loci. For query q and record r: the hit positions of q's keys in r, ascending (a position holds one k-mer, so they are distinct), cut
// wherever two neighbours are MORE than maxGap apart; a piece of at least minHits positions is a locus from its first position to its
// last position + k - 1 (0-based, inclusive, forward strand), with `hits` positions and `distinct` different keys among them. A
// canonical k-mer has no strand, so a locus has none.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace mbgc_screen {
struct KeySet {
    std::vector<uint64_t> keys;                                      // strictly ascending
    std::vector<uint64_t> queryKeys;                                 // per query: how many distinct keys it has
    std::vector<uint64_t> start;                                     // CSR: the queries of key i are queries[start[i], start[i + 1]), ascending
    std::vector<uint32_t> queries;
};
struct Hit { uint32_t rec; uint64_t pos; uint32_t key; };            // the k-mer at position pos of record rec is keys[key]
struct Locus { uint32_t query, rec; uint64_t start, end, hits, distinct; };      // [start, end], 0-based, inclusive

inline int codeOf(char ch) {
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return -1;
    }
}

// the keys of the valid k-mers of text, one per valid position, in position order (k: 1..32)
inline std::vector<uint64_t> canonsOf(const std::string &text, uint32_t k, std::vector<uint64_t> *positions = nullptr) {
    std::vector<uint64_t> out;
    for (size_t p = 0; p + k <= text.size(); p++) {
        uint64_t fw = 0, rc = 0;
        bool ok = true;
        for (uint32_t i = 0; i < k && ok; i++) {
            const int f = codeOf(text[p + i]), b = codeOf(text[p + k - 1 - i]);
            ok = f >= 0 && b >= 0;
            fw = (fw << 2) | (uint64_t) (f & 3);
            rc = (rc << 2) | (uint64_t) (3 - (b & 3));
        }
        if (!ok) continue;
        out.push_back(std::min(fw, rc));
        if (positions) positions->push_back(p);
    }
    return out;
}

// the key set of the queries; a query without a valid k-mer has queryKeys 0 (the command line refuses it)
inline KeySet buildKeys(const std::vector<std::string> &queries, uint32_t k) {
    KeySet S;
    std::vector<std::vector<uint64_t>> own;
    for (const std::string &q : queries) {
        std::vector<uint64_t> c = canonsOf(q, k);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        S.queryKeys.push_back(c.size());
        S.keys.insert(S.keys.end(), c.begin(), c.end());
        own.push_back(std::move(c));
    }
    std::sort(S.keys.begin(), S.keys.end());
    S.keys.erase(std::unique(S.keys.begin(), S.keys.end()), S.keys.end());
    S.start.assign(S.keys.size() + 1, 0);
    std::vector<std::vector<uint32_t>> at(own.size());                // query q's keys as indices
    for (size_t q = 0; q < own.size(); q++)
        for (const uint64_t c : own[q]) {
            const uint32_t i = (uint32_t) (std::lower_bound(S.keys.begin(), S.keys.end(), c) - S.keys.begin());
            at[q].push_back(i);
            S.start[i + 1]++;
        }
    for (size_t i = 0; i < S.keys.size(); i++) S.start[i + 1] += S.start[i];
    S.queries.resize(S.start.back());
    std::vector<uint64_t> fill(S.start.begin(), S.start.end() - 1);
    for (size_t q = 0; q < own.size(); q++) for (const uint32_t i : at[q]) S.queries[fill[i]++] = (uint32_t) q;
    return S;
}

// hits sorted by (rec, pos), each (rec, pos) once -> the loci, sorted by (query, rec, start)
inline std::vector<Locus> chainLoci(const std::vector<Hit> &hits, const KeySet &S, uint32_t k, uint64_t maxGap, uint64_t minHits) {
    std::vector<std::vector<Hit>> of(S.queryKeys.size());            // query q's hits, still sorted by (rec, pos)
    for (const Hit &h : hits)
        for (uint64_t i = S.start[h.key]; i < S.start[h.key + 1]; i++) of[S.queries[i]].push_back(h);
    std::vector<Locus> out;
    std::vector<uint32_t> seen;
    for (size_t q = 0; q < of.size(); q++) {
        const std::vector<Hit> &H = of[q];
        for (size_t a = 0; a < H.size();) {
            size_t b = a + 1;
            while (b < H.size() && H[b].rec == H[a].rec && H[b].pos - H[b - 1].pos <= maxGap) b++;
            if (b - a >= minHits && b - a > 0) {
                seen.clear();
                for (size_t i = a; i < b; i++) seen.push_back(H[i].key);
                std::sort(seen.begin(), seen.end());
                const uint64_t distinct = (uint64_t) (std::unique(seen.begin(), seen.end()) - seen.begin());
                out.push_back(Locus{(uint32_t) q, H[a].rec, H[a].pos, H[b - 1].pos + k - 1, (uint64_t) (b - a), distinct});
            }
            a = b;
        }
    }
    return out;
}

// the line of --regions-out for a locus [start, end] (0-based) of a record: NAME:FROM-TO, 1-based, widened by flank, FROM clamped at 1
inline std::string regionLine(const std::string &record, uint64_t start, uint64_t end, uint64_t flank) {
    const uint64_t from = start + 1, to = end + 1;
    return record + ":" + std::to_string(from > flank ? from - flank : 1) + "-" + std::to_string(to + flank) + "\n";
}
}  // namespace mbgc_screen
