// `mbgc-hip f --primers`: the hits of the primers paired into products (in-silico PCR). Plain vectors in, plain vectors out, no decoder
// type and no device: tests/find_amplicons_main.cpp compiles this header alone.
// A primer pair is FWD and REV, both written 5'->3'. On the forward strand of a linear record a `+` product is a `+` hit of FWD at
// [s1, e1] (0-based, inclusive) on the left and a `-` hit of REV — its reverse complement stands in the text — at [s2, e2] on the right,
// with s1 <= s2, e1 <= e2 and min <= e2 - s1 + 1 <= max; a `-` product is the same with the roles swapped, REV `+` on the left and FWD
// `-` on the right. EVERY such pair of hits is a product, not only the nearest; FWD-FWD and REV-REV are none. Nothing reaches over a
// record's end, so a product across the origin of a circular genome is not found.
#pragma once
#include <algorithm>
#include <cstdint>
#include <tuple>
#include <vector>

namespace mbgc_amplicons {
enum Role : uint32_t { FWD_PLUS = 0, FWD_MINUS = 1, REV_PLUS = 2, REV_MINUS = 3 };
struct Hit { uint32_t rec; uint64_t pos; uint32_t len, pair, role, mismatches; };        // the primer stands at [pos, pos + len) of record rec
struct Product { uint32_t rec, pair; uint64_t start, end; char strand; uint32_t leftMismatches, rightMismatches; };     // [start, end], 0-based, inclusive

// -> the products, sorted by (rec, start, end, pair, + before -); a hit of no bytes is ignored
inline std::vector<Product> pairHits(const std::vector<Hit> &hits, uint64_t minLen, uint64_t maxLen) {
    // lefts and rights of one (rec, pair, strand) side by side: sorted by that key, the rights by their end within it
    struct Side { uint32_t rec, pair, minus; uint64_t start, end; uint32_t mismatches; };
    std::vector<Side> lefts, rights;
    for (const Hit &h : hits) {
        if (h.len == 0 || h.role > REV_MINUS) continue;
        const Side s = {h.rec, h.pair, (uint32_t) (h.role == REV_PLUS || h.role == FWD_MINUS), h.pos, h.pos + h.len - 1, h.mismatches};
        (h.role == FWD_PLUS || h.role == REV_PLUS ? lefts : rights).push_back(s);
    }
    const auto key = [](const Side &s) { return std::make_tuple(s.rec, s.pair, s.minus); };
    std::sort(rights.begin(), rights.end(), [&](const Side &a, const Side &b) { return std::tuple_cat(key(a), std::make_tuple(a.end, a.start)) < std::tuple_cat(key(b), std::make_tuple(b.end, b.start)); });
    std::vector<Product> out;
    for (const Side &l : lefts) {
        // the first right of the left's group whose end is at least the left's (e1 <= e2); the ends rise from there on
        auto r = std::lower_bound(rights.begin(), rights.end(), l, [&](const Side &a, const Side &b) { return std::tuple_cat(key(a), std::make_tuple(a.end)) < std::tuple_cat(key(b), std::make_tuple(b.end)); });
        for (; r != rights.end() && key(*r) == key(l); ++r) {
            const uint64_t length = r->end - l.start + 1;            // (e2 >= e1 >= s1)
            if (length > maxLen) break;
            if (length < minLen || r->start < l.start) continue;
            out.push_back(Product{l.rec, l.pair, l.start, r->end, l.minus ? '-' : '+', l.mismatches, r->mismatches});
        }
    }
    std::sort(out.begin(), out.end(), [](const Product &a, const Product &b) {
        return std::make_tuple(a.rec, a.start, a.end, a.pair, a.strand == '-', a.leftMismatches, a.rightMismatches) <
               std::make_tuple(b.rec, b.start, b.end, b.pair, b.strand == '-', b.leftMismatches, b.rightMismatches);
    });
    return out;
}
}  // namespace mbgc_amplicons
