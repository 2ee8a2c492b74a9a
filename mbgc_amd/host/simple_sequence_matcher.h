// PgTools::SimpleSequenceMatcher::rcMatchSequence with the reference's signature (matching/SimpleSequenceMatcher.h:38-39,
// .cpp:165-176) over the C ABI of include/mbgc_copmem.h: the `-m3` reverse-complement pass over the literal stream, index
// build and query scan on the device (mbgc_amd/csrc/copmem.hip); and restoreRCMatchedSequence (.h:41-42, .cpp:178-211), its
// inverse, planned and filled on the device (mbgc_amd/csrc/copmem_restore.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace PgTools {

class SimpleSequenceMatcher {
public:
    // sequence is rewritten in place (matched parts cut out, RC_MATCH_MARK left behind); rcMapOff / rcMapLen receive the maps
    static void rcMatchSequence(std::string &sequence, std::string &rcMapOff, std::string &rcMapLen, size_t targetMatchLength,
                                uint32_t minMatchLength = UINT32_MAX, int device = 0);

    struct RestoreStats { uint64_t marks = 0, restoredFromMatches = 0, maxChain = 0, minMatchLength = 0; double planMs = 0, fillMs = 0; };
    static constexpr size_t UNKNOWN_LENGTH = SIZE_MAX;
    // sequence (the cut stream) is replaced by the restored one. orgSrcLen, the uncut length, selects the width of an rcMapOff
    // entry as in the reference (4 bytes iff <= UINT32_MAX) and must be what the maps restore; UNKNOWN_LENGTH: the width follows
    // from the restored length and is checked against the stream. false (sequence untouched): malformed maps or a device
    // error, the message in *error — with error == nullptr the message is printed and the process ends, as in rcMatchSequence.
    static bool restoreRCMatchedSequence(std::string &sequence, std::string &rcMapOff, std::string &rcMapLen, size_t orgSrcLen,
                                         int device = 0, std::string *error = nullptr, RestoreStats *stats = nullptr);
};

}  // namespace PgTools
