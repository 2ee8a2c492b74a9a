// Part of mbgc_decoder.cpp (included there once, behind mbgc_decoder_fasta.h): `d --region 'PATTERN:FROM-TO'`, parts of records.
// The specs are held to the headers (the distinct patterns matched on the device, once; which spec applies to which chosen record
// on the host, over the chosen headers only), then — once the plan has said how long every record is — to the records' lengths:
// the pieces, in output order. The closure and the fill work at the grain of granules (DecodedCollection::closure);
// what leaves the decoder is cut out of the sequence buffer here: the pieces packed back to back for <out>.seq, and for --fasta
// the format kernel run over the pieces with headers synthesized on the host.
#pragma once

namespace {
// the record's header with ":<from>-<to>" (1-based, inclusive, to clamped) behind its first whitespace-delimited word
std::string regionHeader(const std::string &header, uint64_t from1, uint64_t to1) {
    size_t w = 0;
    while (w < header.size() && isspace((unsigned char) header[w])) w++;
    while (w < header.size() && !isspace((unsigned char) header[w])) w++;
    return header.substr(0, w) + ":" + std::to_string(from1) + "-" + std::to_string(to1) + header.substr(w);
}

// ---- the specs against the headers: sel.asks, and the records that carry one as the selection (contigSel / unitSel, as --select-seq
// leaves them: a record's file must have passed --select)
bool chooseRegions(const std::string &prefix, const StreamSet &S, const MBGC_Decoder::Options &opt, const FastaLayout &layout, Selection &sel, std::string &msg) {
    if (opt.regions.empty()) return true;
    const uint64_t N = S.g0n + S.planned;
    std::vector<std::string> pats;                                   // the distinct patterns; specOf[j]: the specs of pattern j
    std::vector<std::vector<size_t>> specOf;
    for (size_t i = 0; i < opt.regions.size(); i++) {
        size_t j = (size_t) (std::find(pats.begin(), pats.end(), opt.regions[i].pattern) - pats.begin());
        if (j == pats.size()) { pats.push_back(opt.regions[i].pattern); specOf.emplace_back(); }
        specOf[j].push_back(i);
    }
    std::vector<uint32_t> bits;
    if (!matchHeaders(opt, layout, N, pats, bits, sel.matchMs, "--region", msg)) return false;
    const size_t T = S.T();
    sel.selecting = sel.selectingRegion = true;
    sel.contigSel.assign(N, 0);
    sel.asks.clear();
    uint32_t shift = 0;
    while ((1u << shift) < opt.regionGranule) shift++;
    sel.granuleShift = shift;
    uint64_t c = 0;
    for (size_t u = 0; u <= T; u++) {
        const uint64_t n = u == 0 ? S.g0n : S.seqCount[u - 1];
        char any = 0;
        if (sel.unitSel[u] && !(u == 0 && S.meta.sequentialMatching))
            for (uint64_t k = c; k < c + n; k++) {
                if (!((bits[k >> 5] >> (k & 31)) & 1u)) continue;
                // the device has narrowed the headers to this one; which of the patterns it holds is found here
                const std::string h(layout.headers, layout.hdrOff[k], layout.hdrLen[k]);
                for (size_t j = 0; j < pats.size(); j++)
                    if (h.find(pats[j]) != std::string::npos)
                        for (size_t i : specOf[j]) sel.asks.push_back({k, opt.regions[i].from, opt.regions[i].to, u});
                sel.contigSel[k] = any = 1;
            }
        sel.unitSel[u] = any;
        c += n;
    }
    if (sel.asks.empty()) {
        msg = "--region: no record of the collection matches (" + std::to_string(pats.size()) + " patterns against " + prefix + ".headers)";
        return false;
    }
    return true;
}

// ---- the asks against the records' lengths (contigLen: per contig of the collection, known once the plan has run): to is clamped,
// a region that starts behind its record's end yields nothing and is counted; identical pieces count once; the order is the
// output's: by record, then from, then to
void resolveRegions(const std::vector<uint64_t> &contigLen, bool oneFile, Selection &sel) {
    sel.pieces.clear();
    sel.regionSkipped = sel.regionBases = sel.regionRecords = sel.selectedFiles = 0;
    for (const RegionAsk &a : sel.asks) {
        if (a.from > contigLen[a.contig]) { sel.regionSkipped++; continue; }
        sel.pieces.push_back({a.contig, a.from - 1, std::min(a.to, contigLen[a.contig]) - a.from + 1, a.unit});
    }
    const auto key = [](const RegionPiece &p) { return std::make_tuple(p.contig, p.from, p.len); };
    std::sort(sel.pieces.begin(), sel.pieces.end(), [&](const RegionPiece &x, const RegionPiece &y) { return key(x) < key(y); });
    sel.pieces.erase(std::unique(sel.pieces.begin(), sel.pieces.end(), [&](const RegionPiece &x, const RegionPiece &y) { return key(x) == key(y); }), sel.pieces.end());
    for (size_t i = 0; i < sel.pieces.size(); i++) {
        sel.regionBases += sel.pieces[i].len;
        if (!i || sel.pieces[i].contig != sel.pieces[i - 1].contig) sel.regionRecords++;
        if (!i || sel.pieces[i].unit != sel.pieces[i - 1].unit) sel.selectedFiles++;
    }
    if (oneFile && !sel.pieces.empty()) sel.selectedFiles = 1;
}

// ---- the pieces as what the sinks walk: piece i lies at off[i] of the sequence buffer and is len[i] long; rows: per written file
// its run of pieces (ChosenUnit over piece numbers); layout: the original's names and line lengths with one synthesized header per
// piece (fasta: the original layout was read whole; else only its headers were)
struct RegionOutput {
    std::vector<uint64_t> off, len;
    std::vector<ChosenUnit> rows;
    FastaLayout layout;
};
RegionOutput regionOutput(const DecodedCollection &D, const Selection &sel, const FastaLayout &layout, bool fasta) {
    RegionOutput R;
    if (fasta) { R.layout.lineLen = layout.lineLen; R.layout.names = layout.names; R.layout.outNames = layout.outNames; }
    for (size_t i = 0; i < sel.pieces.size(); i++) {
        const RegionPiece &p = sel.pieces[i];
        R.off.push_back(D.seqOff[p.contig] + p.from); R.len.push_back(p.len);
        if (R.rows.empty() || R.rows.back().unit != p.unit) R.rows.push_back({p.unit, i, i});
        R.rows.back().c1 = i + 1;
        const std::string h = regionHeader(std::string(layout.headers, layout.hdrOff[p.contig], layout.hdrLen[p.contig]), p.from + 1, p.from + p.len);
        R.layout.hdrOff.push_back(R.layout.headers.size()); R.layout.hdrLen.push_back(h.size());
        R.layout.headers += h; R.layout.headers.push_back('\n');
    }
    return R;
}

// <outPrefix>.seq: the pieces back to back, packed on the device (mbgc_fasta_pack_dev) and downloaded once; .contigLens: their lengths;
// .seqCounts: the pieces per written file (oneFile: a single-FASTA set, one count); and --closure-out
bool writeRegionFiles(const DecodedCollection &D, const RegionOutput &R, uint64_t bases, int device, const std::string &closureOut, const std::string &outPrefix,
                      bool oneFile, std::string &msg) {
    std::string seq(bases, '\0');
    if (bases) {
        struct Stage {
            mbgc_fasta_t *fa = nullptr; uint8_t *dev = nullptr;
            ~Stage() { if (dev) mbgc_fasta_dev_free(fa, dev); if (fa) mbgc_fasta_destroy(fa); }
        } st;
        std::vector<mbgc_fasta_pack_piece_t> pieces;
        for (size_t i = 0; i < R.off.size(); i++) pieces.push_back({R.off[i], R.len[i]});
        std::vector<uint64_t> dstOff(pieces.size() + 1);
        double ms = 0;
        if (mbgc_fasta_create(&st.fa, device) || mbgc_fasta_dev_alloc(st.fa, bases + 64, &st.dev) ||
            mbgc_fasta_pack_dev(st.fa, D.seqDev, D.totalBases, pieces.data(), pieces.size(), 0, st.dev, bases + 64, dstOff.data(), &ms)) return faFail(msg, "--region");
        if (dstOff[pieces.size()] != bases) { msg = "internal error: the packed pieces are not the chosen regions"; return false; }
        if (swsem_dev_download(D.h, &seq[0], st.dev, bases)) return hipFail(msg, "download");
    }
    std::vector<uint32_t> counts;
    for (const ChosenUnit &x : R.rows) {
        if (oneFile && !counts.empty()) counts.back() += (uint32_t) (x.c1 - x.c0);
        else counts.push_back((uint32_t) (x.c1 - x.c0));
    }
    if (!closureOut.empty() && !writeFile(closureOut, D.mark.data(), D.mark.size())) { msg = "cannot write " + closureOut; return false; }
    if (!writeFile(outPrefix + ".seq", seq.data(), seq.size()) || !writeFile(outPrefix + ".contigLens", R.len.data(), R.len.size() * sizeof(uint64_t)) ||
        !writeFile(outPrefix + ".seqCounts", counts.data(), counts.size() * sizeof(uint32_t))) {
        msg = "cannot write " + outPrefix + ".seq / .contigLens / .seqCounts";
        return false;
    }
    return true;
}
}  // namespace
