// The way back of the input stage (included by fasta_input.hip, inside namespace fa, after CHUNK / THREADS / PER): the record table
// and the owner table mbgc_fasta_format_dev makes on the host, and k_fa_format. Kept free of HIP calls so that the same text
// compiles as plain C++: tests/fasta_format_emu.cpp runs the kernel body lane by lane on the CPU under AddressSanitizer.
// ---- the way back (mbgc_fasta_format_dev): FASTA text from contigs, headers and a line length per record — '>' header '\n', then
// the sequence in lines as the reference's writeDNA breaks them (MBGC_Decoder.cpp:76-92). The work unit is a tile of the OUTPUT:
// 4096 bytes of text, 16 per lane, so every store is one aligned 16-byte vector store whatever the records look like, and the
// loads are the side that goes unaligned. A tile finds its records through an owner table (tile -> first record that touches it)
// made on the host; a lane searches only between its tile's owner and the next tile's. Inside a sequence the byte at zone
// offset p is '\n' when p % (line + 1) == line (or p is the zone's last byte), else seq[p - p / (line + 1)]: one 64-bit division
// per lane step, then a counter. Steps that touch a header, a record's end, or lines shorter than a step walk byte by byte.
struct FmtRec {
    uint64_t textOff;         // where the record's text starts
    uint64_t seqOff, seqLen, hdrOff, hdrLen;
    uint64_t line;            // bytes per line, 1 .. seqLen (the host folds "0 = one line" and lengths beyond the sequence)
    uint64_t zone;            // bytes of the sequence with its newlines: seqLen + lines
};
constexpr uint32_t FMT_SLICE = 65535;                                // tiles per launch

__device__ __forceinline__ uint32_t fmt_find(const FmtRec *__restrict__ R, uint32_t lo, uint32_t hi, uint64_t o) {   // the last record of [lo, hi] that starts at or before o
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (R[mid].textOff <= o) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// text is the buffer's start; it stands `mis` bytes behind a 16-byte boundary, and the tiles are laid over the aligned addresses:
// tile t, lane step s covers the text offsets [t * 4096 + s * 16 - mis, ... + 16) that lie in [0, total)
__global__ void __launch_bounds__(THREADS) k_fa_format(const uint8_t *__restrict__ seq, uint64_t seqBytes, const uint8_t *__restrict__ hdr,
                                                       const FmtRec *__restrict__ R, const uint32_t *__restrict__ owner, uint32_t tile0,
                                                       uint32_t ntiles, uint32_t mis, uint64_t total, uint8_t *__restrict__ text) {
    const uint32_t tile = tile0 + blockIdx.x;
    if (tile >= ntiles) return;
    const uint64_t vs = (uint64_t) tile * CHUNK + threadIdx.x * PER, vend = total + mis;
    if (vs + PER <= mis || vs >= vend) return;
    const bool full = vs >= mis && vs + PER <= vend;
    const uint64_t o = vs >= mis ? vs - mis : 0;
    const uint32_t n = (uint32_t) ((vs + PER < vend ? vs + PER : vend) - mis - o);     // bytes of this step, 1..16
    uint32_t r = fmt_find(R, owner[tile], owner[tile + 1], o);
    FmtRec rec = R[r];
    uint64_t t = o - rec.textOff;                                   // offset in the record's text
    uint64_t zs = rec.hdrLen + 2;                                   // where its sequence zone starts
    uint64_t q = 0, rem = 0;                                        // zone offset p = q * (line + 1) + rem
    if (t >= zs && rec.zone) {
        const uint64_t p = t - zs, W = rec.line + 1;
        q = p / W; rem = p - q * W;
    }
    if (full && t >= zs && t + PER <= zs + rec.zone && rec.line >= PER) {
        const uint64_t p = t - zs;
        const uint64_t d1 = rec.line - rem, dl = rec.zone - 1 - p;  // bytes to the line's newline / to the zone's last byte (>= 15)
        if (!(dl == PER - 1 && d1 < PER - 1)) {                     // at most one newline in the step
            const uint32_t j = (uint32_t) (d1 < dl ? (d1 < PER ? d1 : PER) : (dl < PER ? dl : PER));   // its place, 16: none
            const uint64_t s0 = rec.seqOff + (p - q);
            uint8_t in[PER];
            if (s0 + PER <= seqBytes) { uint4 v; memcpy(&v, seq + s0, PER); memcpy(in, &v, PER); }
            else
#pragma unroll
                for (uint32_t i = 0; i < PER; i++) in[i] = s0 + i < seqBytes ? seq[s0 + i] : 0;
            uint8_t out[PER];
#pragma unroll
            for (uint32_t i = 0; i < PER; i++) out[i] = i < j ? in[i] : (i == j ? (uint8_t) '\n' : in[i ? i - 1 : 0]);
            uint4 v;
            memcpy(&v, out, PER);
            *(uint4 *) (text + o) = v;
            return;
        }
    }
    uint8_t out[PER];
#pragma unroll
    for (uint32_t i = 0; i < PER; i++) {
        out[i] = 0;
        if (i < n) {
            while (t >= zs + rec.zone) { rec = R[++r]; t = 0; zs = rec.hdrLen + 2; q = 0; rem = 0; }    // (a record has two bytes at least)
            uint8_t b;
            if (t == 0) b = '>';
            else if (t <= rec.hdrLen) b = hdr[rec.hdrOff + t - 1];
            else if (t + 1 == zs) b = '\n';
            else {
                const uint64_t p = t - zs;
                if (rem == rec.line || p + 1 == rec.zone) b = '\n';
                else b = seq[rec.seqOff + (p - q)];
                if (++rem == rec.line + 1) { rem = 0; q++; }
            }
            out[i] = b;
            t++;
        }
    }
    if (full) {
        uint4 v;
        memcpy(&v, out, PER);
        *(uint4 *) (text + o) = v;
    } else
#pragma unroll
        for (uint32_t i = 0; i < PER; i++) if (i < n) text[o + i] = out[i];          // the buffer's head and tail
}

// The host's half: records -> table (nrec + 1 entries, the last one a sentinel at the text's end), every record's text offset, and
// for a buffer that stands `mis` bytes behind a 16-byte boundary the tiles' owners (ntiles + 1 entries). Returns the text's size.
struct FmtIn { uint64_t seqOff, seqLen, headerOff, headerLen, lineLen; };
inline uint64_t fmt_build_table(const FmtIn *recs, uint64_t nrec, std::vector<FmtRec> &table, uint64_t *textOff) {
    table.resize(nrec + 1);
    uint64_t total = 0;
    for (uint64_t k = 0; k < nrec; k++) {
        const FmtIn &x = recs[k];
        FmtRec &f = table[k];
        f.textOff = total; f.seqOff = x.seqOff; f.seqLen = x.seqLen; f.hdrOff = x.headerOff; f.hdrLen = x.headerLen;
        f.line = (x.lineLen == 0 || x.lineLen > x.seqLen) ? x.seqLen : x.lineLen;          // 0: one line; so is a line longer than the sequence
        f.zone = x.seqLen ? x.seqLen + (x.seqLen - 1) / f.line + 1 : 0;                    // nothing for an empty sequence, not even a blank line
        if (f.line == 0) f.line = 1;
        textOff[k] = total;
        total += 2 + x.headerLen + f.zone;
    }
    textOff[nrec] = total;
    table[nrec] = FmtRec{total, 0, 0, 0, 0, 1, 0};
    return total;
}
inline void fmt_build_owner(const std::vector<FmtRec> &table, uint64_t nrec, uint32_t mis, uint32_t ntiles, std::vector<uint32_t> &owner) {
    owner.resize((size_t) ntiles + 1);
    uint32_t r = 0;
    for (uint32_t t = 0; t < ntiles; t++) {
        const uint64_t first = (uint64_t) t * CHUNK > mis ? (uint64_t) t * CHUNK - mis : 0;
        while (table[r + 1].textOff <= first) r++;
        owner[t] = r;
    }
    owner[ntiles] = (uint32_t) nrec - 1;
}
