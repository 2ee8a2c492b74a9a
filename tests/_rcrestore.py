"""SimpleSequenceMatcher::restoreRCMatchedSequence (matching/SimpleSequenceMatcher.cpp:178-211) restated in Python, the whole of
complementsLUT (utils/helper.cpp:312-361) included: the sequential loop — find a mark, read an offset (4 or 8 bytes) and a
byte-frugal length, append the reverse complement of `substr(offset, length)` of what is restored so far. std::string::substr
throws when the offset lies beyond the end and silently truncates a length that runs over it; so does this."""
import numpy as np

MARK = 0xA4                                              # MBGC_Params::RC_MATCH_MARK, '$' + 128


def complements_lut():
    """indexed by the byte; the constructor's loops stop before CHAR_MAX, so entry 127 stays 0"""
    lut = np.arange(256, dtype=np.uint8)
    lut[127] = 0
    for a, b in zip(b"AaCcGgTtNnUuYyRrKkMmBbDdHhVvWwSs", b"TTGGCCAANNAARRYYMMKKVVHHDDBBSSWW"):
        lut[a] = b
    lut[ord("U")], lut[ord("u")] = ord("U"), ord("u")
    for a, b in zip(b"acgtnyrkmbdhvws", b"tgcanrymkvhdbsw"):
        lut[a] = b
    return lut


LUT = complements_lut()


def put_byte_frugal(v):
    """PgHelpers::writeUIntByteFrugal, utils/helper.cpp:217-225"""
    out = bytearray()
    while v >= 128:
        out.append(128 + v % 128)
        v //= 128
    out.append(v)
    return bytes(out)


def read_byte_frugal(buf, at):
    """PgHelpers::readUIntByteFrugal, utils/helper.h:232-241 -> (value, next position)"""
    v, base = 0, 1
    while True:
        y = buf[at]
        at += 1
        v += base * (y % 128)
        base *= 128
        if y < 128:
            return v, at


def build_maps(min_len, matches, off_bytes=4):
    """rcMapOff / rcMapLen for (source offset, length) pairs, as markAndRemoveExactMatches writes them"""
    map_off = b"".join(int(s).to_bytes(off_bytes, "little") for s, _ in matches)
    map_len = put_byte_frugal(min_len) + b"".join(put_byte_frugal(ln - min_len) for _, ln in matches)
    return map_off, map_len


def restore(cut, map_off, map_len, off_bytes=None):
    """-> the restored bytes. off_bytes None: the reference's rule cannot be applied before the length is known — 4 is taken
    (every test stream is far below 4 GiB); 8 reads the other layout."""
    cut = bytes(cut)
    w = off_bytes or 4
    out = bytearray()
    pos_dest = at_off = at_len = 0
    min_len = 0
    if map_len:
        min_len, at_len = read_byte_frugal(map_len, 0)
    while True:
        mark = cut.find(MARK, pos_dest)
        if mark < 0:
            break
        out += cut[pos_dest:mark]
        pos_dest = mark + 1
        src = int.from_bytes(map_off[at_off:at_off + w], "little")
        at_off += w
        ln, at_len = read_byte_frugal(map_len, at_len)
        ln += min_len
        if src > len(out):
            raise IndexError("substr: the offset lies beyond the end")
        piece = np.frombuffer(bytes(out[src:src + ln]), dtype=np.uint8)          # (a length over the end is truncated)
        out += LUT[piece][::-1].tobytes()
    out += cut[pos_dest:]
    return bytes(out)


CASES = ("planted", "long_copies", "manyfold", "short", "tiny")


def inputs():
    """the _rcdata cases the round trip runs on: the mark itself must not occur in an input of the forward pass, and 127 is the
    one byte complementsLUT does not map back (both replaced by 'A'); lower case, N and the stream marks stay"""
    import _rcdata
    out = {}
    for name, s in _rcdata.cases().items():
        if name in CASES:
            s = s.copy()
            s[(s == MARK) | (s == 127)] = ord("A")
            out[name] = s
    return out


CAP = 1 << 62                                            # sums beyond it are refused (mbgc_amd/csrc/copmem_restore_lane.h)
MAX_VARINT = 10


def values_of(map_len):
    """every value of rcMapLen with the number of bytes it takes -> [(value, bytes)], or None if the last value does not end"""
    vals, at = [], 0
    while at < len(map_len):
        v, k = 0, 0
        while True:
            if at + k >= len(map_len):
                return None
            y = map_len[at + k]
            v += (y % 128) << (7 * k)
            k += 1
            if y < 128:
                break
        vals.append((v, k))
        at += k
    return vals


def restore_bounded(cut, map_off, map_len, off_bytes):
    """The referee of the device's inverse pass: restore() with exactly the refusals include/mbgc_copmem.h documents for the plan
    -> (bytes, M, bytes restored from matches, deepest chain, minMatchLength), or a string that names the refusal (those of a
    source bound begin with "source"). off_bytes is 4 or 8, the width the caller states. The deepest chain is the most matches any
    byte was copied through: a literal has depth 0, a byte of a match one more than the byte it was copied from."""
    assert off_bytes in (4, 8)
    cut = np.frombuffer(bytes(cut), dtype=np.uint8)
    marks = np.flatnonzero(cut == MARK)
    m = len(marks)
    if m == 0 and len(map_off):
        return "rcMapOff: %d bytes, and no mark" % len(map_off)
    if m and len(map_off) not in (4 * m, 8 * m):
        return "rcMapOff: %d bytes for %d marks" % (len(map_off), m)
    if m and len(map_off) != off_bytes * m:
        return "rcMapOff: %d bytes for %d marks of %d bytes each" % (len(map_off), m, off_bytes)
    min_len, deltas = 0, []
    if not map_len:
        if m:
            return "rcMapLen: empty, and %d marks" % m
    else:
        vals = values_of(map_len)
        if vals is None:
            return "rcMapLen: the last value does not end"
        if len(vals) != m + 1:
            return "rcMapLen: %d values for %d marks" % (len(vals), m)
        if any(k > MAX_VARINT for _, k in vals):
            return "rcMapLen: a value of more than %d bytes" % MAX_VARINT
        min_len, deltas = vals[0][0], [v for v, _ in vals[1:]]
        if min_len > 0xFFFFFFFF:
            return "rcMapLen: a minimal length beyond 32 bits"
    lens = [v + min_len for v in deltas]
    total = sum(lens)
    if total > CAP:
        return "rcMapLen: the lengths add up beyond 2^62"
    srcs = [int.from_bytes(map_off[off_bytes * i:off_bytes * (i + 1)], "little") for i in range(m)]
    cum = 0
    for i in range(m):
        d = int(marks[i]) - i + cum
        if srcs[i] + lens[i] > d:
            return "source: match %d at %d copies [%d, %d)" % (i, d, srcs[i], srcs[i] + lens[i])
        cum += lens[i]
    out = np.empty(len(cut) - m + total, dtype=np.uint8)
    dep = np.zeros(len(out), dtype=np.uint32)
    at = prev = 0
    for i in range(m):
        k = int(marks[i]) - prev
        out[at:at + k] = cut[prev:prev + k]
        at += k
        prev = int(marks[i]) + 1
        s, ln = srcs[i], lens[i]
        out[at:at + ln] = LUT[out[s:s + ln]][::-1]
        dep[at:at + ln] = dep[s:s + ln][::-1] + 1
        at += ln
    out[at:] = cut[prev:]
    return out.tobytes(), m, total, int(dep.max()) if len(dep) else 0, min_len
