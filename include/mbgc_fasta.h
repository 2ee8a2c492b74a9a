/* mbgc_fasta.h — C ABI of the MI355X input stage of `mbgc c`: what the reference does per
 * target file between "the file's bytes are in memory" and "its contigs are char arrays for matchTexts":
 *
 *   kseq_init + while (KSEQ_READ(seq) >= 0) { readHeader; seq->seq.s / seq->seq.l ... }   matching/MultipleGenomeMatchingProcessor.cpp:349-372
 *   KSEQ_READ = kseq_read_lossless_fasta                                                    :9-10, utils/kseq.h:233-274
 *   validate_kseq_status (-3 "expected FASTA format", -4 "inconsistent line length")         :16-35
 *   KSEQ_DNA_LINE_LENGTH                                                                     :12-14
 *   params->uppercaseDNA -> PgHelpers::upperSequence                                         :361-362, utils/helper.cpp:447-453
 *
 * The files of a round sit back to back in one device buffer (whole-file reads / inflated .gz land in pinned
 * memory and are copied up by the caller). One call strips the headers and the newlines of all of them and
 * leaves every file's contigs back to back in HBM — exactly the layout swsem_match_batch_dev takes — plus the
 * record table (header bytes, contig offsets), the detected DNA line length and the kseq status per file.
 * gzip inflate (input_with_libdeflate_wrapper.cpp) runs where the caller puts it: zlib on the host, or mbgc_fasta_inflate_dev on
 * files that were uploaded compressed. No CPU fallback. */
#ifndef MBGC_FASTA_H
#define MBGC_FASTA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbgc_fasta mbgc_fasta_t;

typedef struct {
    uint64_t headerOff, headerLen;   /* the header line without '>' and '\n' (seq->name), bytes of the FILE */
    uint64_t seqOff, seqLen;         /* the contig (seq->seq), bytes of the file's part of the output       */
} mbgc_fasta_record_t;

#define MBGC_FASTA_OK 0
#define MBGC_FASTA_ENOTFASTA (-3)    /* kseq status -3: the file does not start with '>'                     */
#define MBGC_FASTA_ELINES (-4)       /* kseq status -4: empty line / inconsistent line lengths (kseq.h:251-265) */
#define MBGC_FASTA_EFASTQ (-16)      /* lossy rule only, no kseq status: a '+' where a sequence line could start — FASTQ, not read here */

/* flags of the *2 entry points */
#define MBGC_FASTA_UPPERCASE 1u      /* params->uppercaseDNA */
#define MBGC_FASTA_LOSSY 2u          /* the rule of `mbgc c -L`: kseq_read_lossy instead of kseq_read_lossless_fasta */

int mbgc_fasta_create(mbgc_fasta_t **out, int device);
void mbgc_fasta_destroy(mbgc_fasta_t *p);
const char *mbgc_fasta_last_error(void);

/* files_dev[fileOff[f] .. fileOff[f+1]) = file f (host array of nf + 1 offsets). seq_out_dev (capacity outCap
 * bytes; fileOff[nf] - fileOff[0] always suffices) receives the contigs; file f's start at seqBase[f] and
 * seqBase[nf] is the total. records (capacity recCap; at most one per two input bytes) receives the records of
 * all files in order, file f's at [recBase[f], recBase[f+1]). status[f] is the kseq status the reference's read
 * loop ends with (0 = clean end of file); for a file with status != 0 — the reference prints its message and
 * exits there — records and sequence bytes of that file are unspecified. dnaLineLen[f] = KSEQ_DNA_LINE_LENGTH.
 * Returns 0, or a negative error of its own (capacity, HIP) with mbgc_fasta_last_error(); when the record table
 * is too small (-104) recBase[nf] holds the number of entries needed. Synchronous. */
int mbgc_fasta_parse_batch_dev(mbgc_fasta_t *p, const uint8_t *files_dev, const uint64_t *fileOff, int nf, int uppercaseDNA,
                               uint8_t *seq_out_dev, uint64_t outCap, uint64_t *seqBase,
                               mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *recBase,
                               uint64_t *dnaLineLen, int *status);

/* One file that sits in host memory and whose contigs the host needs as bytes — the first file of the list, whose
 * sequences become the initial reference and the head of the literal stream (loadG0Ref, MGMP.cpp:66-150): uploaded,
 * parsed by the same kernels, downloaded. seq_out_host has capacity n; records/recCap as above; *nrec, *seqBytes,
 * *dnaLineLen, *status as the batch call reports them for its single file. */
int mbgc_fasta_parse_host(mbgc_fasta_t *p, const uint8_t *file_host, uint64_t n, int uppercaseDNA, uint8_t *seq_out_host,
                          uint64_t *seqBytes, mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *nrec,
                          uint64_t *dnaLineLen, int *status);

/* The two calls above with flags in place of uppercaseDNA; flags = uppercaseDNA ? MBGC_FASTA_UPPERCASE : 0 is the call above.
 * MBGC_FASTA_LOSSY reads by the FASTA part of kseq_read_lossy (utils/kseq.h:282-333, selected by allowLossyParsing,
 * MultipleGenomeMatchingProcessor.cpp:9-14), one kseq_t per file:
 *   - every byte in front of the file's first '>' or '@' is skipped, wherever in a line that byte stands; a file without one has
 *     no records; afterwards a record starts at every line whose first byte is '>' or '@' (not at one that is the file's last byte);
 *   - the header is the line without its marker and '\n', and without one trailing '\r' when it is longer than one byte;
 *   - the sequence is the lines up to the next record start; empty lines are skipped; a line's trailing '\r' is dropped when the
 *     record's sequence, that line appended, is longer than one byte (ks_getuntil2, :147) — so a line that is one '\r' keeps it only
 *     as the record's first sequence byte, or as the file's last byte with no '\n' behind it (:143 returns before the strip);
 *   - dnaLineLen[f] = maxLastDnaLineLen: the longest sequence line of the file after that strip, 0 when there is none;
 *   - status[f] is 0, or MBGC_FASTA_EFASTQ when a line that could be a sequence line starts with '+' (the reference goes on to
 *     read quality strings there, :320-332; this stage does not). Never -3 or -4.
 * headerOff stays an offset in the whole file. */
int mbgc_fasta_parse_batch_dev2(mbgc_fasta_t *p, const uint8_t *files_dev, const uint64_t *fileOff, int nf, uint32_t flags,
                                uint8_t *seq_out_dev, uint64_t outCap, uint64_t *seqBase,
                                mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *recBase,
                                uint64_t *dnaLineLen, int *status);
int mbgc_fasta_parse_host2(mbgc_fasta_t *p, const uint8_t *file_host, uint64_t n, uint32_t flags, uint8_t *seq_out_host,
                           uint64_t *seqBytes, mbgc_fasta_record_t *records, uint64_t recCap, uint64_t *nrec,
                           uint64_t *dnaLineLen, int *status);

/* The protein-profile probe (MGMP_Params::probeProteinsProfile, matching/MGMP_Params.h:86-127, called for the records of the
 * initial reference by loadG0Ref, MultipleGenomeMatchingProcessor.cpp:82-105), on contigs that lie in HBM.
 * seq_dev[0..seqBytes) holds the parsed contigs; record r is seq_dev[recOff[r] .. recOff[r] + recLen[r]) (host arrays of nrec
 * entries, any offsets and alignments). k = the matching k-mer length as it stands (MGMP_Params::k). state_inout is the pair
 * the reference carries from call to call: probe_remaining starts at MBGC_FASTA_PROBE_MAX_LEN, probe_non_std_count at 0.
 * For each record in order, while probe_remaining > 0:
 *     len = min(recLen, probe_remaining); probe_remaining -= len;
 *     probe_non_std_count += the bytes among the first len that are none of a c g t u A C G T U N (a lowercase n counts);
 *     probe_len = MBGC_FASTA_PROBE_MAX_LEN - probe_remaining;
 *     pct = probe_non_std_count * 100 / len      (integers; the RUNNING count over this record's clipped length, as the reference has it)
 *     fires when probe_len >= MBGC_FASTA_PROBE_MIN_LEN && k != 16 && pct > 10, and then sets probe_remaining = 0 for good.
 * One deviation: a record whose clipped length is 0 makes the reference divide by zero; here an empty record leaves the state
 * untouched and does not fire.
 * result_out: whether the probe fired, at which record (index into recOff; 0 when it did not), and the state afterwards, which
 * is also written back to state_inout. Every record is walked, so a caller that takes only some records' verdicts (the
 * sequential schedule takes the first one's) compares `record`. At most MBGC_FASTA_PROBE_MAX_LEN bytes are read. Synchronous. */
#define MBGC_FASTA_PROBE_MIN_LEN 256
#define MBGC_FASTA_PROBE_MAX_LEN 65536
typedef struct { int32_t probe_remaining, probe_non_std_count; } mbgc_fasta_probe_state_t;
typedef struct {
    int32_t fired, reserved;
    uint64_t record;
    mbgc_fasta_probe_state_t state;
} mbgc_fasta_probe_result_t;
int mbgc_fasta_probe_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const uint64_t *recOff, const uint64_t *recLen,
                         uint64_t nrec, int k, mbgc_fasta_probe_state_t *state_inout, mbgc_fasta_probe_result_t *result_out);
/* The same for the file that mbgc_fasta_parse_host2 (or _host) parsed last on this handle: its contigs are still in the handle's
 * device buffer, and records[0..nrec) are the first nrec entries of the table that call returned (seqOff / seqLen are read). The
 * bytes are probed where they were parsed, as they are after MBGC_FASTA_UPPERCASE. */
int mbgc_fasta_probe_host(mbgc_fasta_t *p, const mbgc_fasta_record_t *records, uint64_t nrec, int k,
                          mbgc_fasta_probe_state_t *state_inout, mbgc_fasta_probe_result_t *result_out);

/* Single-FASTA input (`mbgc c -i`): the rule by which the reference cuts one multi-FASTA byte stream into the initial reference
 * and the targets, mgmpInSplit_next(iter, minSplitSize, '>') (matching/input_with_libdeflate_wrapper.cpp:150-171), on a window of
 * the file in HBM. bytes_dev[0..n) starts at an element start. Element j starts where element j - 1 ended (element 0 at 0) and
 * ends at the first byte equal to '>' at an offset >= its start + (j ? nextMin : firstMin) — any '>', also one inside a header
 * line; when its start + the minimum >= the file's size, or no such byte follows, it runs to the end of the file; an element
 * never starts at the end of the file. ends[j] (capacity maxElems) = end of element j relative to the window.
 * isFileEnd = 0: the window is not the file's end, and the call returns the elements whose end lies inside the window — *nElems
 * may be 0 (a contig longer than the window); the caller extends the window and asks again. isFileEnd != 0: the last element ends
 * at n. Synchronous, like its neighbours. */
int mbgc_fasta_split_dev(mbgc_fasta_t *p, const uint8_t *bytes_dev, uint64_t n, int isFileEnd, uint64_t firstMin, uint64_t nextMin,
                         int maxElems, uint64_t *ends, int *nElems);

/* The same for a window that grows: buf_dev[0..n) is the buffer, the elements start at `start`, ends[] are offsets in the buffer.
 * scannedBefore: the caller's promise that buf_dev[0..scannedBefore) has not changed since the last call of this handle, which
 * covered at least that much from a `start` not behind this one — the streaming pass then reads only what was appended (and the tile that was not whole). 0: none. */
int mbgc_fasta_split_buf_dev(mbgc_fasta_t *p, const uint8_t *buf_dev, uint64_t start, uint64_t n, uint64_t scannedBefore, int isFileEnd,
                             uint64_t firstMin, uint64_t nextMin, int maxElems, uint64_t *ends, int *nElems);

/* The same with a rule for what a mark is; flags = 0 is the call above (any '>'). What `mbgc-hip c --lossy-file` cuts its sequential
 * batches with: under kseq_read_lossy a record starts at a line whose first byte is '>' or '@' and nowhere else, so a cut that is a
 * mark by both flags stands between two records of the one stream — no record's state crosses it, and the byte before it is '\n'.
 *   MBGC_FASTA_SPLIT_LINE_START   a mark counts only at offset 0 of the BUFFER (not of `start`) or right behind a '\n'
 *   MBGC_FASTA_SPLIT_AT           '@' is a mark beside '>'
 * Thresholds, isFileEnd, ends and scannedBefore as above; the tile array the handle keeps holds the marks of the flags it was made
 * with, so a call whose flags differ from the last one's scans everything again. Other bits in flags are refused (-103). */
#define MBGC_FASTA_SPLIT_LINE_START 1u
#define MBGC_FASTA_SPLIT_AT 2u
int mbgc_fasta_split_buf_dev2(mbgc_fasta_t *p, const uint8_t *buf_dev, uint64_t start, uint64_t n, uint64_t scannedBefore, int isFileEnd,
                              uint64_t firstMin, uint64_t nextMin, uint32_t flags, int maxElems, uint64_t *ends, int *nElems);

/* The way back (`mbgc-hip d --fasta`): FASTA text from contigs in HBM. seq_dev[0..seqBytes) holds the contigs, headers_dev[0..
 * headerBytes) a copy of the header bytes, recs (host, nrec entries) says for every record of the text, in order, where its contig
 * and its header lie and the line length of its unit (KSEQ_DNA_LINE_LENGTH; 0: every sequence on one line). A record's text is
 * '>' header '\n', then the sequence as the reference's writeDNA breaks it (MBGC_Decoder.cpp:76-92): lineLen bytes and '\n' per
 * full line, the remainder and '\n' if bytes are left, NOTHING for an empty sequence — 2 + headerLen + seqLen + ceil(seqLen /
 * lineLen) bytes ((seqLen > 0) for the last term when lineLen is 0). textOff (host, nrec + 1 entries) receives every record's
 * offset in the text and, last, the total. text_dev has capacity textCap: when the text is longer the call writes nothing to it
 * and returns -104 with the size needed in textOff[nrec] (as the record table of the parser does). Any alignment of text_dev.
 * kernelMs (may be NULL): the kernel's time from events on the stream. Runs on the input stage's stream; synchronous. */
typedef struct {
    uint64_t seqOff, seqLen;         /* the contig, bytes of seq_dev     */
    uint64_t headerOff, headerLen;   /* its header, bytes of headers_dev */
    uint64_t lineLen;
} mbgc_fasta_format_rec_t;
int mbgc_fasta_format_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const uint8_t *headers_dev, uint64_t headerBytes,
                          const mbgc_fasta_format_rec_t *recs, uint64_t nrec, uint8_t *text_dev, uint64_t textCap, uint64_t *textOff,
                          double *kernelMs);

/* The comparison of `mbgc-hip v`: text that was formatted on the device against the originals that were uploaded beside it. Piece k
 * compares a_dev[aOff, aOff + len) with b_dev[bOff, bOff + len) (buffers of aBytes and bBytes bytes). firstDiff (host, nslots
 * entries) receives for every slot the smallest offset WITHIN ITS PIECE at which the bytes of a piece of that slot differ, taken over
 * all pieces that name the slot — the caller adds its own base — and UINT64_MAX when none differ (also for a slot no piece names).
 * Pieces of no bytes are legal. Any alignment of either side; the two sides of a piece may stand at different offsets modulo 16.
 * A piece that does not lie inside both buffers, or names a slot >= nslots, is refused (-103, message in mbgc_fasta_last_error): nothing
 * is launched and firstDiff is left as it was. kernelMs (may be NULL): the kernel's time from events on the stream. Equal bytes
 * cost no atomic: a wave that finds a difference issues one 64-bit atomicMin per piece it touches. Runs on the input stage's
 * stream; synchronous. */
typedef struct { uint64_t aOff, bOff, len; uint32_t slot; } mbgc_fasta_compare_piece_t;
int mbgc_fasta_compare_dev(mbgc_fasta_t *p, const uint8_t *a_dev, uint64_t aBytes, const uint8_t *b_dev, uint64_t bBytes,
                           const mbgc_fasta_compare_piece_t *pieces, uint64_t npieces, uint64_t *firstDiff, uint32_t nslots, double *kernelMs);

/* Pieces of a device buffer back to back in another one (`mbgc-hip r`: the chosen units' contigs out of the decoder's sequence buffer,
 * where the contigs they depend on lie among them, into the buffer the encoder's rounds are slices of). Piece k is src_dev[srcOff,
 * srcOff + len) of a buffer of srcBytes bytes; the pieces land in dst_dev in order, without a separator; pieces of no bytes are
 * legal and may overlap each other in the source. dstOff (host, n + 1 entries) receives every piece's offset in dst_dev and, last,
 * the total. When the total exceeds dstCap the call writes nothing to dst_dev and returns -104 with the size needed in dstOff[n]. A
 * piece that does not lie inside the source, or a source that overlaps dst_dev[0, dstCap), is refused (-103, message in
 * mbgc_fasta_last_error): nothing is launched. No byte outside dst_dev[0, total) is written, no byte outside a piece is read; any
 * alignment of either side (the stores are aligned 16-byte vectors, the loads go unaligned). flags: 0, or MBGC_FASTA_UPPERCASE — the
 * bytes are folded as the parser folds a base under that flag (a..z only). kernelMs (may be NULL): the kernel's time from events on
 * the stream. Runs on the input stage's stream; synchronous. */
typedef struct { uint64_t srcOff, len; } mbgc_fasta_pack_piece_t;
int mbgc_fasta_pack_dev(mbgc_fasta_t *p, const uint8_t *src_dev, uint64_t srcBytes, const mbgc_fasta_pack_piece_t *pieces, uint64_t n, uint32_t flags,
                        uint8_t *dst_dev, uint64_t dstCap, uint64_t *dstOff, double *kernelMs);

/* The record selection of `mbgc-hip d --select-seq`: which headers contain one of a list of patterns. Record r is chosen iff its header
 * bytes [hdrOff[r], hdrOff[r] + hdrLen[r]) of headers_dev (a buffer of headerBytes bytes) contain at least one pattern as a byte
 * substring (case-sensitive, as std::string::find). patterns (host): the patterns back to back, pattern k at [patOff[k], patOff[k + 1]);
 * every pattern is non-empty and holds no '\n' — one that is not is refused, as is a header outside the buffer (-103, message in
 * mbgc_fasta_last_error; nothing is launched, chosen is left as it was). chosen (host, (nrec + 31) / 32 words) receives bit r & 31 of
 * word r >> 5 per record; the bits behind the last record are 0. No pattern: no record is chosen.
 * What a header byte costs does not grow with the number of patterns: a table keyed by the first m = min(8, shortest pattern) bytes of
 * every pattern is probed once per position, and only the patterns that share those bytes are compared (the same pattern given twice
 * is one). One wave per header, 64 positions at a time, the bytes staged in LDS; a wave leaves its header at the first hit and sets
 * the record's bit with one atomic. No byte outside a record's own header is read or counted — not the line feed behind it, not the
 * next header: a pattern longer than the header cannot match, a header of no bytes matches nothing. kernelMs (may be NULL): the
 * kernel's time from events on the stream. Runs on the input stage's stream; synchronous. */
int mbgc_fasta_match_headers_dev(mbgc_fasta_t *p, const uint8_t *headers_dev, uint64_t headerBytes, const uint64_t *hdrOff, const uint64_t *hdrLen,
                                 uint64_t nrec, const uint8_t *patterns, const uint64_t *patOff, uint64_t npat, uint32_t *chosen, double *kernelMs);

/* One CRC-32 per byte range of a device buffer (`mbgc-hip c --checksums`, `d --check`, `t`: a contig's bases are checked where they
 * lie). crc_out_host[k] (host, n entries) = zlib's crc32(0, seq_dev + recs[k].off, recs[k].len): polynomial 0xEDB88320 reflected,
 * initial value and final XOR 0xffffffff; 0 for len == 0. The ranges may overlap, repeat, be unsorted and start at any byte; a range
 * with off + len > seqBytes is refused (-103, message in mbgc_fasta_last_error; nothing is launched, crc_out_host is left as it
 * was). One kernel launch per call whatever n is, none for n == 0 or ranges of no bytes only: ranges of up to 256 bytes take one lane
 * each, up to 1024 / 4096 / 16384 bytes a group of 4 / 16 / 64 lanes, longer ones are cut into pieces of 16384 bytes over as many waves
 * and folded with the arithmetic of crc32_combine. No byte outside a range is read on its behalf (aligned vector loads only where a
 * whole vector lies inside it). kernelMs (may be NULL): the kernel's time from events on the stream. Runs on the input stage's
 * stream; synchronous. */
typedef struct { uint64_t off, len; } mbgc_fasta_crc_rec_t;
int mbgc_fasta_crc_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                       uint32_t *crc_out_host, double *kernelMs);
/* the same over the records mbgc_fasta_parse_host2 has just parsed, whose sequences it left in HBM (as mbgc_fasta_probe_host reads
 * them): crc_out_host[r] is record r's. The initial reference is parsed that way; its bases are checked without a second upload. */
int mbgc_fasta_crc_host(mbgc_fasta_t *p, const mbgc_fasta_record_t *records, uint64_t nrec, uint32_t *crc_out_host, double *kernelMs);
/* host: the CRC-32 of A followed by B from crc32(A), crc32(B) and B's length (zlib's crc32_combine); needs no device */
uint32_t mbgc_fasta_crc_combine(uint32_t crcA, uint32_t crcB, uint64_t lenB);

/* The search of `mbgc-hip f`: where do query sequences stand in byte ranges of a device buffer, with at most maxMismatches
 * substitutions. Record r is seq_dev[recs[r].off, recs[r].off + recs[r].len) of a buffer of seqBytes bytes; the records may overlap,
 * repeat, be empty and come in any order. patterns_host: the patterns back to back, pattern q at [patOff[q], patOff[q + 1]); the same
 * pattern may be given twice. With fold(b) = b & 0xDF for an ASCII letter and b otherwise, a hit is (rec r, pattern q, pos p,
 * mismatches d): p + len(q) <= recs[r].len, d = the positions j with fold(seq[recs[r].off + p + j]) != fold(pattern_q[j]), d <=
 * maxMismatches. Every hit is reported exactly once, overlapping ones included; a hit never reaches over a record's end, whatever lies
 * behind it in the buffer. The call knows nothing of strands or names.
 * Refused before anything is launched (-103, message in mbgc_fasta_last_error; *nHits and hits_host are left as they were):
 * maxMismatches > 3; a pattern that holds a byte that is no ASCII letter, is shorter than 8 (maxMismatches + 1) bytes or longer than
 * 65535; a record that does not lie inside the buffer.
 * *nHits is always the exact count. When it exceeds hitCap the call returns -104 and leaves hits_host as it was: call again with that
 * capacity. Otherwise hits_host[0, *nHits) holds the hits sorted by (rec, pos, pattern). The device appends rows through one atomic
 * cursor and writes only below hitCap; the host sorts.
 * What a text byte costs does not grow with the number of patterns: a pattern is cut into maxMismatches + 1 disjoint seeds, one table
 * keyed by the seeds' first 8 folded bytes is probed once per text position, and only the patterns that share those bytes are counted
 * out. The records are cut into tiles of MBGC_FASTA_FIND_TILE positions on the 16-byte grid of the buffer's addresses, one list over
 * all records; a block of 256 lanes stages a tile and the 16 bytes behind it in LDS with aligned 16-byte loads and takes the next
 * tile of the list. The table lies in LDS up to 2048 slots, in global memory beyond. No byte outside seq_dev[0, seqBytes) is read.
 * kernelMs (may be NULL): the kernel's time from events on the stream. Runs on the input stage's stream; synchronous. */
#define MBGC_FASTA_FIND_TILE 4096
typedef struct { uint64_t pos; uint32_t rec, pattern, mismatches, reserved; } mbgc_fasta_hit_t;
int mbgc_fasta_find_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                        const uint8_t *patterns_host, const uint64_t *patOff, uint64_t npat, uint32_t maxMismatches,
                        mbgc_fasta_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs);

/* The search of `mbgc-hip f --iupac` and `--primers`: mbgc_fasta_find_dev's question, arguments, hit rows, order and refusals with
 * another matching rule — a pattern letter is an IUPAC code, a SET of bases. The set of a pattern letter, either case:
 *   A: A   C: C   G: G   T, U: T   R: AG   Y: CT   S: CG   W: AT   K: GT   M: AC   B: CGT   D: AGT   H: ACT   V: ACG   N: ACGT
 * A text byte has a base only if it is one of acgtuACGTU, u counting as T; every other byte has none — N and the ambiguity letters IN THE
 * TEXT included. Position j matches if and only if the text byte has a base and that base is in the pattern letter's set. So a text N is
 * a mismatch against everything, a pattern N included; this differs from mbgc_fasta_find_dev, where letters are compared literally and
 * an N matches an N. A hit is (rec r, pattern q, pos p, mismatches d): p + len(q) <= recs[r].len, d = the positions that do not match,
 * d <= maxMismatches. Every hit is reported exactly once, overlapping ones included; a hit never reaches over a record's end; no byte
 * outside seq_dev[0, seqBytes) is read.
 * Refused before anything is launched (-103; *nHits and hits_host are left as they were): maxMismatches > 3; a pattern shorter than
 * 8 (maxMismatches + 1) letters or longer than 65535; a letter outside the table above; a pattern with a segment that has no usable
 * seed (below; the message names the pattern and the segment); a record that does not lie inside the buffer. -104 with the exact count
 * in *nHits when the hits do not fit, as in mbgc_fasta_find_dev; otherwise hits_host[0, *nHits) sorted by (rec, pos, pattern).
 * How: a pattern is cut into maxMismatches + 1 disjoint segments of len / (maxMismatches + 1) letters, one of which an alignment
 * leaves free of mismatches. A segment's seed is the window of 8 letters inside it that stands for the fewest concrete sequences (the
 * product of the letters' set sizes; the leftmost on a tie); the host expands it into each of them — 256 at most, which four N in a
 * row reach exactly; a segment whose best window stands for more is the refusal above — and packs each into 16 bits. The 65536
 * possible grams are a bitmap of 8 KiB that a block keeps in LDS whatever the patterns are; a lane tests its 16 positions against it
 * (a text gram that holds a byte without a base is no gram) and reads the rows of a gram from global memory only on a set bit. Tiles,
 * staging, cursor and hit buffer are mbgc_fasta_find_dev's.
 * mbgc_fasta_find_iupac_last: the rows (pattern, segment, expansion) of the last call's table, and the rows its lanes walked. */
int mbgc_fasta_find_iupac_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n,
                              const uint8_t *patterns_host, const uint64_t *patOff, uint64_t npat, uint32_t maxMismatches,
                              mbgc_fasta_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs);
void mbgc_fasta_find_iupac_last(const mbgc_fasta_t *p, uint64_t *tableRows, uint64_t *rowsWalked);

/* The scan of `mbgc-hip s`: what do byte ranges of a device buffer hold, and where are their runs of N and of lower case. Record r is
 * seq_dev[recs[r].off, recs[r].off + recs[r].len), as in mbgc_fasta_find_dev: the records may overlap, touch, repeat, be empty and
 * stand at any offset. A record that does not lie inside [0, seqBytes) is refused before anything is launched (-103, message in
 * mbgc_fasta_last_error; counts_host, runs_host, *nRuns and *kernelMs are left as they were).
 * flags & MBGC_FASTA_STATS_COUNTS: counts_host[r] is filled (not touched otherwise): a, c, g, t, n counted without case, U / u as t
 * (the probe of `c` takes acgtuACGTUN for nucleotides in the same way); other = every other byte; lower = the bytes in 'a'..'z'
 * whatever the letter, so it is orthogonal to the first six; a + c + g + t + n + other == recs[r].len; reserved = 0.
 * Runs: class 0 is N / n (asked for with MBGC_FASTA_STATS_NRUNS), class 1 any byte in 'a'..'z' (MBGC_FASTA_STATS_LOWER), so n is in
 * both. A run is a MAXIMAL stretch of one class inside one record: a byte outside the record never lengthens, shortens, starts or
 * ends one, whatever its class, also where the record ends with the buffer. A run (start = its first position in the record, len,
 * rec, cls) is returned when len >= minRunN (class 0) / minRunLower (class 1); a minimum of 0 is read as 1. *nRuns is always the
 * exact number of rows that qualify. When it exceeds runCap the call returns -104 and has written nothing to runs_host (the counts
 * are filled all the same): call again with that capacity. Otherwise runs_host[0, *nRuns) holds the rows sorted by (rec, cls,
 * start), each once. -105: internal, the edges do not pair.
 * One pass of k_fa_stats over the tiles of mbgc_fasta_find_dev's kind (MBGC_FASTA_FIND_TILE positions on the 16-byte grid of the
 * buffer's addresses, one list over all records; every record with a byte has tiles). A lane reads its 16 positions as one aligned
 * vector — nothing is staged in LDS — and no byte outside seq_dev[0, seqBytes) is read. The counts are summed over the wave by
 * shuffles, over the block in LDS, and added to the record's row with at most seven 64-bit atomic adds per tile. A run is found by
 * its two edges (a position in the class whose neighbour inside the record is not) and never walked; the edges go to a device buffer
 * of the call's own through one atomic cursor, which counts the ones past its end too: the call then grows the buffer and runs the
 * kernel again. The host pairs the i-th start of a (record, class) with its i-th end and applies the minimum lengths.
 * kernelMs (may be NULL): the last run of the kernel, from events on the stream. Runs on the input stage's stream; synchronous.
 * mbgc_fasta_stats_last: the edges the last call's kernel reported and how often the kernel was run again for a larger buffer. */
#define MBGC_FASTA_STATS_COUNTS 1u   /* fill counts            */
#define MBGC_FASTA_STATS_NRUNS  2u   /* report runs of class 0 */
#define MBGC_FASTA_STATS_LOWER  4u   /* report runs of class 1 */
typedef struct { uint64_t a, c, g, t, n, other, lower, reserved; } mbgc_fasta_counts_t;
typedef struct { uint64_t start, len; uint32_t rec, cls; } mbgc_fasta_run_t;
int mbgc_fasta_stats_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint32_t flags,
                         uint64_t minRunN, uint64_t minRunLower, mbgc_fasta_counts_t *counts_host, mbgc_fasta_run_t *runs_host, uint64_t runCap,
                         uint64_t *nRuns, double *kernelMs);
void mbgc_fasta_stats_last(const mbgc_fasta_t *p, uint64_t *edges, uint64_t *reruns);

/* The two scans of `mbgc-hip k`: FracMinHash sketches of groups of records of a device buffer, and the sizes of the sketches'
 * intersections. Everything returned is an integer.
 * The hash: k is 1..32 (anything else: -103). A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3, every other byte is invalid. A k-mer is the k bytes
 * at positions i .. i + k - 1 of ONE record, 0 <= i <= len - k; one that holds an invalid byte is skipped. fw = sum of code[i + j] <<
 * 2 (k - 1 - j), rc = sum of (3 - code[i + j]) << 2 j, h = fmix64(min(fw, rc) ^ 0x9E3779B97F4A7C15), fmix64 being MurmurHash3's 64-bit
 * finaliser. This is NOT the hash of Mash or of sourmash: the sketches cannot be exchanged with theirs. h is kept when h <= maxHash
 * (maxHash = (2^64 - 1) / scale; ~0: every hash).
 * mbgc_fasta_sketch_dev: record r is seq_dev[recs[r].off, recs[r].off + recs[r].len), as in mbgc_fasta_stats_dev — the records may
 * overlap, touch, repeat, be empty or shorter than k —, and belongs to group group_host[r] < ngroups (any values, in any order; a
 * record outside the buffer or a group >= ngroups: -103, nothing launched). kmers_host[g] = the valid k-mer positions of group g's
 * records (a record listed twice counts twice). The sketch of group g = the strictly ascending list of the DISTINCT kept hashes of all
 * its records = hashes_host[groupStart_host[g], groupStart_host[g + 1]); groupStart_host has ngroups + 1 entries. *total is always the
 * exact number of hashes over all groups, = groupStart_host[ngroups]. When it exceeds cap the call returns -104: nothing in
 * hashes_host is promised, groupStart_host and kmers_host are filled — call again with that capacity.
 * One pass of k_fa_sketch over the tiles of mbgc_fasta_find_dev's kind (MBGC_FASTA_FIND_TILE k-mer starts on the 16-byte grid of the
 * buffer's addresses). A lane packs its aligned 16-byte vector into a 32-bit code word and a 16-bit invalid mask and takes those of the
 * two vectors behind it from its neighbours; no byte outside seq_dev[0, seqBytes) is read and none outside the record reaches a
 * result. The kept (hash, group) rows go to a device buffer of the call's own through one atomic cursor, taken once per wave and tile,
 * which counts the rows past the buffer's end too: the call then grows the buffer and runs the kernel again. The rows are sorted to
 * (group, hash) order by two stable radix sorts, the first of each (group, hash) is kept, and the groups' starts are read off the
 * kept rows — all on the device. kernelMs (may be NULL): the last run of k_fa_sketch. Runs on the input stage's stream; synchronous.
 * mbgc_fasta_sketch_last: the rows the last call's kernel reported and how often it was run again for a larger buffer;
 * mbgc_fasta_sketch_sort_ms: the last call's sorts, flagging and compaction, from events on the stream.
 * mbgc_fasta_sketch_pairs_dev: shared_host[q] = the number of hashes the sketches of groups pairs_host[2 q] and pairs_host[2 q + 1]
 * have in common (any ids < ngroups, repeats and (i, i) too); pairs_host == NULL: all i < j in row-major order, npairs must be ngroups
 * (ngroups - 1) / 2. The sketches (small) are uploaded; a list that does not ascend strictly, an id >= ngroups or a wrong npairs is
 * refused on the host (-103). k_fa_sketch_pairs: a wave per pair, the lanes stride over the shorter list and look each hash up in the
 * longer one by bisection; a pair with an empty side answers 0 without a search. */
int mbgc_fasta_sketch_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, const uint32_t *group_host,
                          uint32_t ngroups, uint32_t k, uint64_t maxHash, uint64_t *hashes_host, uint64_t cap, uint64_t *groupStart_host, uint64_t *kmers_host,
                          uint64_t *total, double *kernelMs);
void mbgc_fasta_sketch_last(const mbgc_fasta_t *p, uint64_t *rows, uint64_t *reruns);
double mbgc_fasta_sketch_sort_ms(const mbgc_fasta_t *p);
int mbgc_fasta_sketch_pairs_dev(mbgc_fasta_t *p, const uint64_t *hashes_host, const uint64_t *groupStart_host, uint32_t ngroups, const uint32_t *pairs_host,
                                uint64_t npairs, uint32_t *shared_host, double *kernelMs);

/* The scan of `mbgc-hip m`: which of a list of k-mers occur in which groups of records of a device buffer, and where.
 * k-mers. k, the codes, validity, fw, rc and canon = min(fw, rc) are those of mbgc_fasta_sketch_dev above; a k-mer lies inside ONE record.
 * No hash enters a result: the key of a k-mer is canon itself. keys_host[0, nkeys) is a strictly ascending list of such words.
 * Records and groups: as in mbgc_fasta_sketch_dev — the records may overlap, touch, repeat, be empty or shorter than k and stand at any
 * offset; record r belongs to group group_host[r] < ngroups.
 * A hit is (record r, position p, key index i): the k-mer at position p of record r is valid and its canon is keys_host[i].
 * found_host[groupStart_host[g], groupStart_host[g + 1]) = the strictly ascending list of the key INDICES with a hit in a record of group
 * g; groupStart_host has ngroups + 1 entries. *total is always the exact number over all groups; when it exceeds foundCap the call
 * returns -104 with groupStart_host filled and nothing promised in found_host. hits_host may be NULL; otherwise it receives the hits as
 * (pos, rec, key) rows sorted by (rec, pos), each hit once. *nHits is always their exact number; when it exceeds hitCap the call
 * returns -104 and writes no hit (mbgc_fasta_find_dev's protocol).
 * Refused with -103, nothing launched, every output left as it was: k outside 1..32; nkeys == 0 or > 2^24; a key with a bit at or above
 * 2 k; keys that do not ascend strictly; a record outside the buffer; a group >= ngroups.
 * One pass of k_fa_screen over the tiles of mbgc_fasta_sketch_dev's kind, with its packing and window, so no byte outside seq_dev[0,
 * seqBytes) is read and none outside the record reaches a result. Membership has two levels: a filter of 2^17 bits, built here from the
 * keys and copied into every block's LDS, is asked about every valid position (bit = the top 17 bits of fmix64(canon ^
 * 0x9E3779B97F4A7C15)); only a set bit leads to a table in global memory — open addressing, linear probing, a power-of-two number of
 * slots >= 2 nkeys indexed by the hash's low bits, a slot holds a key index + 1 — and a find is confirmed against the keys. The rows go
 * to a device buffer through one atomic cursor, taken once per wave and tile, which counts the rows past the buffer's end too: the call
 * then grows the buffer and runs the kernel again. The distinct (group, key) come from the rows on the device: one radix sort, the first
 * of each run flagged, an exclusive sum, a compaction; the hits by a stable sort by position and one by record. kernelMs (may be NULL):
 * the last run of k_fa_screen. Runs on the input stage's stream; synchronous.
 * mbgc_fasta_screen_last: the last call's rows (= hits), the valid positions that passed the filter, how often the kernel was run again
 * for a larger buffer, and the ms of the sorts and the compaction. Every pointer may be NULL. */
typedef struct { uint64_t pos; uint32_t rec, key; } mbgc_fasta_screen_hit_t;
int mbgc_fasta_screen_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, const uint32_t *group_host,
                          uint32_t ngroups, uint32_t k, const uint64_t *keys_host, uint64_t nkeys, uint32_t *found_host, uint64_t foundCap, uint64_t *groupStart_host,
                          uint64_t *total, mbgc_fasta_screen_hit_t *hits_host, uint64_t hitCap, uint64_t *nHits, double *kernelMs);
void mbgc_fasta_screen_last(const mbgc_fasta_t *p, uint64_t *hitRows, uint64_t *filterPasses, uint64_t *reruns, double *sortMs);

/* The scan of `mbgc-hip u`: which byte ranges of a device buffer are the same sequence, read forward or as the reverse complement.
 * Records. Record r is seq_dev[recs[r].off, recs[r].off + recs[r].len), exactly as in mbgc_fasta_stats_dev: the ranges may overlap,
 * touch, repeat, be empty and stand at any byte offset. A range outside the buffer (or a flag that is not defined) is refused with
 * -103 (message in mbgc_fasta_last_error): nothing is launched, out_host, *nClasses and *kernelMs are left as they were.
 * fold. fold(b) = b & 0xDF for an ASCII letter, and b otherwise. Under MBGC_FASTA_DUPS_EXACT_CASE, fold(b) = b.
 * comp. comp is an involution on the 256 byte values: comp[b] = b, except for the six pairs on upper case and the same pairs on lower
 * case, which keep the case:
 *     A <-> T   C <-> G   R <-> Y   K <-> M   B <-> V   D <-> H        a <-> t   c <-> g   r <-> y   k <-> m   b <-> v   d <-> h
 * Every other byte — N, S, W, U, the other letters, non-letters, the bytes >= 0x80 — maps to itself. This is deliberately NOT the
 * table of swsem_revcomp_dev (the upper reverse complement of the matcher): that one upper-cases, so it is no involution, and "is the
 * reverse complement of" would not be symmetric under it. The table is kept in one place (dups_comp_upper, mbgc_amd/csrc/fasta_dups.h);
 * mbgc_fasta_dups_comp_table returns its 256 entries.
 * The relation. Records a and b are the same sequence when either of these holds:
 *   - they have equal length and fold(a[i]) == fold(b[i]) for all i;
 *   - unless MBGC_FASTA_DUPS_FORWARD_ONLY is set, they have equal length and fold(a[i]) == comp(fold(b[len - 1 - i])) for all i.
 * This is an equivalence relation. All empty records are one class.
 * Output per record: out_host[r] = { rep, strand }. rep is the lowest index in r's class. strand is 0 when the record equals rep read
 * forward — a record that equals rep both ways, or is rep itself, also gets 0 — and 1 when it equals only the reverse complement of
 * rep. *nClasses is the number of classes. Everything is exact: no result rests on a fingerprint alone.
 * How. One pass of k_fa_dups over the tiles of mbgc_fasta_find_dev's kind (MBGC_FASTA_FIND_TILE positions on the 16-byte grid of the
 * buffer's addresses, the record of a tile by bisection): a lane reads its aligned 16-byte vector, a position outside the record
 * contributes nothing whatever memory holds there, and no byte outside seq_dev[0, seqBytes) is read. From that one read of the text a
 * tile yields the partial sums of two strand fingerprints, forward = sum T[fold(s_j)] x^(len - 1 - j) and reverse complement = sum
 * T[comp(fold(s_j))] x^j (T[b] = b + 1), each as four residues modulo four primes just below 2^31 (124 bits, every multiply 32 x 32 ->
 * 64); lanes are summed by shuffles, waves through LDS, and at most eight 64-bit atomic adds of terms below 2^31 go to the record's
 * row, which the host reduces modulo the primes. The canonical fingerprint is the smaller of (forward, reverse), the forward one
 * under FORWARD_ONLY. Records with equal (len, canonical fingerprint) form a bucket, made by a sort on the host (n counts records,
 * not bases). Every non-first member of a bucket is then verified against the bucket's first member by k_fa_dups_verify — the bytes
 * are compared under fold, or under fold and comp with the second side read backwards; forward first, then reverse, a comparison the
 * fingerprints already exclude being skipped; one ballot per step, one atomic per refuted pair —, a refuted member opens a new
 * representative inside its bucket, and the remaining members are verified against the bucket's representatives, round by round,
 * until every member has a class. MBGC_FASTA_DUPS_WEAK_HASH is a flag for tests: only the low 4 bits of a fingerprint are kept, so
 * that the exactness step runs on ordinary inputs; the result is identical with and without it.
 * kernelMs (may be NULL): k_fa_dups, from events on the stream. Runs on the input stage's stream; synchronous; n == 0 launches nothing.
 * mbgc_fasta_dups_last: the last call's buckets, the pairs k_fa_dups_verify compared, those it refuted, and its launches' time. */
#define MBGC_FASTA_DUPS_FORWARD_ONLY 1u   /* the reverse complement is not the same sequence */
#define MBGC_FASTA_DUPS_EXACT_CASE   2u   /* fold(b) = b                                     */
#define MBGC_FASTA_DUPS_WEAK_HASH    4u   /* tests: 4 bits of fingerprint                    */
typedef struct { uint32_t rep; uint32_t strand; } mbgc_fasta_dup_t;
int mbgc_fasta_dups_dev(mbgc_fasta_t *p, const uint8_t *seq_dev, uint64_t seqBytes, const mbgc_fasta_crc_rec_t *recs, uint64_t n, uint32_t flags,
                        mbgc_fasta_dup_t *out_host, uint64_t *nClasses, double *kernelMs);
void mbgc_fasta_dups_last(const mbgc_fasta_t *p, uint64_t *buckets, uint64_t *verified, uint64_t *refuted, double *verifyMs);
const uint8_t *mbgc_fasta_dups_comp_table(void);

/* gzip files that lie compressed in HBM, inflated there(mgmpInOpen's loop over libdeflate_gzip_decompress_ex, matching/
 * input_with_libdeflate_wrapper.cpp:51-124): job k reads gz_dev[inOff, inOff + inLen) — a whole file: one or more gzip members (RFC
 * 1952: magic, CM = 8, FEXTRA / FNAME / FCOMMENT skipped, FHCRC checked, the eight-byte trailer) holding DEFLATE (RFC 1951, all three
 * block types) — and writes the text to out_dev[outOff, outOff + outCap). One wave per job; no byte outside either range is touched,
 * whatever the input holds, and every input ends its job. results[k] (host, njobs entries):
 *   status   MBGC_INFLATE_OK, or what stopped the job; a job's failure is its own, the others of the call complete
 *   members  members that were decoded and checked
 *   outLen   the text's length (valid for OK only; what a failed job left in its range is unspecified)
 *   inUsed   input bytes consumed (inLen for OK)
 * Each member's CRC-32 and ISIZE are checked as zlib checks them. A job that does not lie inside both buffers, or whose output range
 * overlaps another job's, is refused before anything is launched (-103, message in mbgc_fasta_last_error; results untouched).
 * kernelMs (may be NULL): the kernel's time from events on the stream. Runs on the input stage's stream; synchronous. */
#define MBGC_INFLATE_OK      0
#define MBGC_INFLATE_ESHORT  1   /* the text does not fit outCap; nothing past the cap was written */
#define MBGC_INFLATE_EDATA   2   /* not gzip / malformed DEFLATE / input ends early */
#define MBGC_INFLATE_ECHECK  3   /* a member's CRC-32 or ISIZE does not match */
typedef struct { uint64_t inOff, inLen, outOff, outCap; } mbgc_fasta_inflate_job_t;
typedef struct { int32_t status; uint32_t members; uint64_t outLen, inUsed; } mbgc_fasta_inflate_result_t;
int mbgc_fasta_inflate_dev(mbgc_fasta_t *p, const uint8_t *gz_dev, uint64_t gzBytes, uint8_t *out_dev, uint64_t outBytes,
                           const mbgc_fasta_inflate_job_t *jobs, uint64_t njobs, mbgc_fasta_inflate_result_t *results, double *kernelMs);

/* The way back, compressed (`mbgc-hip d --fasta dir --gzip`; the reference's `mbgc d -c`, MBGC_Decoder.cpp:185-203): text that lies
 * in HBM becomes gzip files there. Job k compresses text_dev[inOff, inOff + inLen) (any alignment; inside the buffer of textBytes
 * bytes) into one gzip member: the header 1f 8b 08 00 00 00 00 00 00 ff (no name, no time: the bytes are a function of the text
 * alone), DEFLATE, CRC-32 and ISIZE. The text is cut into chunks of MBGC_DEFLATE_CHUNK bytes, max(1, ceil(inLen / CHUNK)) per job,
 * one wave each: no back-reference crosses a chunk's start, a chunk is one dynamic block (matches of 8 bytes and more, exact
 * histograms, length-limited Huffman codes, always complete code sets) or, where that is not smaller, one stored block, and ends on a
 * byte boundary (an empty stored block; the last chunk sets BFINAL) — any inflater reads the result. The files land back to back in
 * gz_dev in job order; results[k] (host, njobs entries) says where: outOff, outLen, the text's CRC-32, its chunks and how many of
 * them went out stored. *gzBytes = the total, never more than the sum of mbgc_fasta_deflate_bound(inLen). When the total exceeds
 * gzCap nothing is written to gz_dev and the call returns -104 with the size needed in *gzBytes; no byte outside gz_dev[0, *gzBytes)
 * is ever written. A job that lies outside the text is refused before anything is launched (-103, message in
 * mbgc_fasta_last_error; results untouched). The same text gives the same bytes, on every run and whatever other jobs share the
 * call. kernelMs (may be NULL): both kernels' time (the chunks, then the pack) from events on the stream. Runs on the input stage's
 * stream; synchronous. */
#define MBGC_DEFLATE_CHUNK 32768
#define MBGC_DEFLATE_OK 0
typedef struct { uint64_t inOff, inLen; } mbgc_fasta_deflate_job_t;
typedef struct { uint64_t outOff, outLen; uint32_t crc32, chunks, storedChunks, reserved; } mbgc_fasta_deflate_result_t;
uint64_t mbgc_fasta_deflate_bound(uint64_t inLen);   /* 18 + max(1, ceil(inLen / CHUNK)) * 10 + inLen */
int mbgc_fasta_deflate_dev(mbgc_fasta_t *p, const uint8_t *text_dev, uint64_t textBytes,
                           const mbgc_fasta_deflate_job_t *jobs, uint64_t njobs,
                           uint8_t *gz_dev, uint64_t gzCap, mbgc_fasta_deflate_result_t *results,
                           uint64_t *gzBytes, double *kernelMs);

/* A download that runs beside the kernels of the input stage's stream (the decoder's text batches: batch b travels while batch b + 1
 * is formatted): begin queues the copy on a stream of its own and returns; wait returns when it has arrived, with the copy's time
 * from events on that stream in *copyMs (may be NULL). One download at a time: begin before the last one's wait is refused (-103).
 * dst_host should be page-locked (mbgc_fasta_host_alloc), or the copy is not asynchronous. The caller orders the copy behind the
 * kernels that write src_dev: mbgc_fasta_format_dev has returned, so they have finished. */
int mbgc_fasta_download_begin(mbgc_fasta_t *p, void *dst_host, const uint8_t *src_dev, uint64_t bytes);
int mbgc_fasta_download_wait(mbgc_fasta_t *p, double *copyMs);

/* n pieces src_dev[off[k] .. off[k] + len[k]) of a device buffer of srcBytes bytes, packed back to back on the device, each followed
 * by the byte sep, and downloaded: out_host (capacity outCap) receives *outBytes = sum(len) + n bytes; -104 with *outBytes set when
 * it is too small. What `mbgc-hip c -i` keeps of a batch's elements: the header lines, not the elements. Synchronous. */
int mbgc_fasta_gather_dev(mbgc_fasta_t *p, const uint8_t *src_dev, uint64_t srcBytes, const uint64_t *off, const uint64_t *len, uint64_t n,
                          uint8_t sep, uint8_t *out_host, uint64_t outCap, uint64_t *outBytes);

/* Device memory for the windows of a single-FASTA input, before a matcher exists (the initial reference is cut from the first
 * window): plain allocation, a device-to-device copy and a download on the input stage's stream, each synchronous. */
int mbgc_fasta_dev_alloc(mbgc_fasta_t *p, uint64_t bytes, uint8_t **out);
int mbgc_fasta_dev_free(mbgc_fasta_t *p, uint8_t *ptr);
int mbgc_fasta_dev_copy(mbgc_fasta_t *p, uint8_t *dst_dev, const uint8_t *src_dev, uint64_t bytes);
int mbgc_fasta_download(mbgc_fasta_t *p, void *dst_host, const uint8_t *src_dev, uint64_t bytes);

/* The way into HBM ("fed by pinned-memory reads"): page-locked host memory for the reader threads to
 * read files into, and its copy to the device on the input stage's own stream — it returns when the bytes have arrived
 * and waits for nothing the matcher has queued. */
int mbgc_fasta_host_alloc(mbgc_fasta_t *p, uint64_t bytes, void **out);
int mbgc_fasta_host_free(mbgc_fasta_t *p, void *ptr);
int mbgc_fasta_upload(mbgc_fasta_t *p, uint8_t *dst_dev, const void *src_host, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
