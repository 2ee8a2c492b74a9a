// The host's gzip inflate, shared by the input stage of `mbgc-hip c` (mgmp_driver.cpp) and the originals `mbgc-hip v` reads
// (mbgc_decoder.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <zlib.h>

// mgmpInOpen (matching/input_with_libdeflate_wrapper.cpp:51-124): the whole file, and when it starts with the gzip magic,
// its members inflated one after the other (the reference: libdeflate_gzip_decompress_ex in a loop until the input is
// used up, output buffer sized by the ISIZE trailer and doubled when short; here: zlib on the host, where a round's files
// inflate while the GPU matches the round before. `mbgc-hip c --inflate device` and `mbgc-hip v --inflate device` inflate the
// files of a list, and the originals, in HBM instead (mbgc_fasta_inflate_dev) and come here only for a file that does not
// inflate to its ISIZE there)
// false, the message in error and dest as it was: the inflate failed (a corrupt or truncated file)
static bool tryInflateGzip(const std::string &gz, std::string &dest, std::string &error) {
    const size_t at = dest.size();
    uint32_t isize;
    memcpy(&isize, gz.data() + gz.size() - 4, 4);
    size_t cap = isize ? isize : gz.size() * 4, out = 0;
    dest.resize(at + cap);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) { dest.resize(at); error = "Cannot allocate decompressor."; return false; }
    auto bad = [&](int res) { inflateEnd(&z); dest.resize(at); error = "Error decompressing gz file: " + std::to_string(res) + "."; return false; };
    z.next_in = (Bytef *) gz.data();
    size_t inLeft = gz.size();
    while (true) {
        z.avail_in = (uInt) std::min<size_t>(inLeft, 1u << 30);
        const size_t inGiven = z.avail_in;
        z.next_out = (Bytef *) &dest[at + out];
        z.avail_out = (uInt) std::min<size_t>(cap - out, 1u << 30);
        const size_t outGiven = z.avail_out;
        const int res = inflate(&z, Z_NO_FLUSH);
        inLeft -= inGiven - z.avail_in;
        out += outGiven - z.avail_out;
        if (res == Z_STREAM_END) {
            if (inLeft == 0) break;
            if (inflateReset(&z) != Z_OK) return bad(res);                                                                      // the next member
        } else if (res == Z_OK || res == Z_BUF_ERROR) {
            if (out == cap) { cap *= 2; dest.resize(at + cap); }
            else if (inLeft == 0) return bad(res);                                                                              // truncated
        } else
            return bad(res);
    }
    inflateEnd(&z);
    dest.resize(at + out);
    return true;
}

// the input stage's way (the reference's: message and exit). The callers stand on reader threads and on the input thread, beside
// threads that are reading files and a main thread that has kernels in flight: exit() there runs the exit handlers and the
// destructors of static objects (the HIP runtime's among them) while those threads still use them, which the C++ standard leaves
// undefined and which has ended such a run with SIGSEGV behind its message. So: the message, the streams flushed, and _exit —
// the same status, no handlers run beside working threads.
[[maybe_unused]] static void inflateGzip(const std::string &gz, std::string &dest) {
    std::string error;
    if (!tryInflateGzip(gz, dest, error)) { fprintf(stderr, "%s\n", error.c_str()); fflush(nullptr); _exit(EXIT_FAILURE); }
}

static bool isGzip(const uint8_t *p, size_t n) { return n >= 18 && p[0] == 0x1f && p[1] == 0x8b; }     // GZIP_ID1, GZIP_ID2
