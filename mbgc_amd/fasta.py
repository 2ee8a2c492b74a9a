"""ctypes view of include/mbgc_fasta.h — the input stage (kseq_read_lossless_fasta, or kseq_read_lossy, for whole files in HBM)."""
import ctypes as C
import math

import numpy as np

from . import binding

EXPORTS = """mbgc_fasta_create mbgc_fasta_destroy mbgc_fasta_last_error mbgc_fasta_parse_batch_dev mbgc_fasta_parse_host mbgc_fasta_parse_batch_dev2 mbgc_fasta_parse_host2 mbgc_fasta_host_alloc mbgc_fasta_host_free mbgc_fasta_upload
           mbgc_fasta_split_dev mbgc_fasta_split_buf_dev mbgc_fasta_split_buf_dev2 mbgc_fasta_format_dev mbgc_fasta_download_begin mbgc_fasta_download_wait mbgc_fasta_gather_dev mbgc_fasta_dev_alloc mbgc_fasta_dev_free mbgc_fasta_dev_copy mbgc_fasta_download
           mbgc_fasta_probe_dev mbgc_fasta_probe_host mbgc_fasta_compare_dev mbgc_fasta_inflate_dev mbgc_fasta_deflate_dev mbgc_fasta_deflate_bound mbgc_fasta_pack_dev mbgc_fasta_match_headers_dev
           mbgc_fasta_crc_dev mbgc_fasta_crc_combine mbgc_fasta_find_dev mbgc_fasta_find_iupac_dev mbgc_fasta_find_iupac_last mbgc_fasta_stats_dev mbgc_fasta_stats_last
           mbgc_fasta_sketch_dev mbgc_fasta_sketch_last mbgc_fasta_sketch_sort_ms mbgc_fasta_sketch_pairs_dev
           mbgc_fasta_dups_dev mbgc_fasta_dups_last mbgc_fasta_dups_comp_table mbgc_fasta_screen_dev mbgc_fasta_screen_last""".split()


UPPERCASE, LOSSY = 1, 2              # MBGC_FASTA_UPPERCASE, MBGC_FASTA_LOSSY
EFASTQ = -16                         # MBGC_FASTA_EFASTQ
SPLIT_LINE_START, SPLIT_AT = 1, 2    # MBGC_FASTA_SPLIT_LINE_START, MBGC_FASTA_SPLIT_AT


class Record(C.Structure):
    _fields_ = [("headerOff", C.c_uint64), ("headerLen", C.c_uint64), ("seqOff", C.c_uint64), ("seqLen", C.c_uint64)]


class FormatRecord(C.Structure):
    _fields_ = [("seqOff", C.c_uint64), ("seqLen", C.c_uint64), ("headerOff", C.c_uint64), ("headerLen", C.c_uint64), ("lineLen", C.c_uint64)]


class ComparePiece(C.Structure):
    _fields_ = [("aOff", C.c_uint64), ("bOff", C.c_uint64), ("len", C.c_uint64), ("slot", C.c_uint32)]


class PackPiece(C.Structure):
    _fields_ = [("srcOff", C.c_uint64), ("len", C.c_uint64)]


class CrcRec(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint64)]


FIND_TILE = 4096                     # MBGC_FASTA_FIND_TILE: text positions per tile of find_dev
FIND_MAX_MISMATCHES, FIND_MAX_PATTERN = 3, 65535
FIND_IUPAC_MAX_EXPAND = 256          # find_iupac_dev: the concrete sequences a segment's best window of 8 letters may stand for
IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
              "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


class Hit(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("rec", C.c_uint32), ("pattern", C.c_uint32), ("mismatches", C.c_uint32), ("reserved", C.c_uint32)]


HIT_DTYPE = np.dtype([("pos", "<u8"), ("rec", "<u4"), ("pattern", "<u4"), ("mismatches", "<u4"), ("reserved", "<u4")])


class HitsTooMany(binding.SwsemError):
    """find_dev: the hits do not fit the buffer; .needed = their exact count"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


STATS_COUNTS, STATS_NRUNS, STATS_LOWER = 1, 2, 4     # MBGC_FASTA_STATS_*
COUNTS_COLUMNS = ("a", "c", "g", "t", "n", "other", "lower", "reserved")     # mbgc_fasta_counts_t
RUN_DTYPE = np.dtype([("start", "<u8"), ("len", "<u8"), ("rec", "<u4"), ("cls", "<u4")])     # mbgc_fasta_run_t


class RunsTooMany(binding.SwsemError):
    """stats_dev: the runs do not fit the buffer; .needed = their exact count"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


DUPS_FORWARD_ONLY, DUPS_EXACT_CASE, DUPS_WEAK_HASH = 1, 2, 4     # MBGC_FASTA_DUPS_*
DUP_DTYPE = np.dtype([("rep", "<u4"), ("strand", "<u4")])        # mbgc_fasta_dup_t


class SketchTooLarge(binding.SwsemError):
    """sketch_dev: the hashes do not fit the buffer; .needed = their exact count"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


SCREEN_HIT_DTYPE = np.dtype([("pos", "<u8"), ("rec", "<u4"), ("key", "<u4")])     # mbgc_fasta_screen_hit_t
SCREEN_MAX_KEYS = 1 << 24


class ScreenTooLarge(binding.SwsemError):
    """screen_dev: the found keys do not fit the buffer; .needed = their exact count"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


class PackTooSmall(binding.SwsemError):
    """pack_dev: the pieces do not fit the buffer; .needed = their size"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


NO_DIFFERENCE = 2 ** 64 - 1          # UINT64_MAX: what compare_dev leaves in a slot whose pieces are equal


INFLATE_OK, INFLATE_ESHORT, INFLATE_EDATA, INFLATE_ECHECK = 0, 1, 2, 3      # MBGC_INFLATE_*


class InflateJob(C.Structure):
    _fields_ = [("inOff", C.c_uint64), ("inLen", C.c_uint64), ("outOff", C.c_uint64), ("outCap", C.c_uint64)]


class InflateResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("members", C.c_uint32), ("outLen", C.c_uint64), ("inUsed", C.c_uint64)]


DEFLATE_CHUNK = 32768                # MBGC_DEFLATE_CHUNK


class DeflateJob(C.Structure):
    _fields_ = [("inOff", C.c_uint64), ("inLen", C.c_uint64)]


class DeflateResult(C.Structure):
    _fields_ = [("outOff", C.c_uint64), ("outLen", C.c_uint64), ("crc32", C.c_uint32), ("chunks", C.c_uint32), ("storedChunks", C.c_uint32),
                ("reserved", C.c_uint32)]


class GzipTooSmall(binding.SwsemError):
    """deflate_dev: the gzip files do not fit the buffer; .needed = their size"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


def deflate_bound(n):
    """mbgc_fasta_deflate_bound: the most a text of n bytes takes as a gzip file of deflate_dev"""
    return 18 + max(1, -(-int(n) // DEFLATE_CHUNK)) * 10 + int(n)


PROBE_MIN_LEN, PROBE_MAX_LEN = 256, 65536      # MBGC_FASTA_PROBE_MIN_LEN, MBGC_FASTA_PROBE_MAX_LEN


class ProbeState(C.Structure):
    _fields_ = [("probe_remaining", C.c_int32), ("probe_non_std_count", C.c_int32)]


class ProbeResult(C.Structure):
    _fields_ = [("fired", C.c_int32), ("reserved", C.c_int32), ("record", C.c_uint64), ("state", ProbeState)]


class TextTooSmall(binding.SwsemError):
    """format_dev: the text does not fit the buffer; .needed = its size"""
    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


def _lib():
    L = binding.lib()
    if not getattr(L, "_fasta_ready", False):
        L.mbgc_fasta_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.mbgc_fasta_destroy.argtypes = [C.c_void_p]
        L.mbgc_fasta_last_error.restype = C.c_char_p
        L.mbgc_fasta_parse_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64), C.POINTER(Record), C.c_uint64, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mbgc_fasta_parse_batch_dev2.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_uint32, C.c_void_p, C.c_uint64,
                                                  C.POINTER(C.c_uint64), C.POINTER(Record), C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        for name, second in (("mbgc_fasta_parse_host", C.c_int), ("mbgc_fasta_parse_host2", C.c_uint32)):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, second, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(Record), C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mbgc_fasta_split_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mbgc_fasta_split_buf_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mbgc_fasta_split_buf_dev2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32,
                                                C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mbgc_fasta_format_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(FormatRecord), C.c_uint64,
                                            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_gather_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.c_uint8,
                                            C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mbgc_fasta_probe_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.c_int,
                                           C.POINTER(ProbeState), C.POINTER(ProbeResult)]
        L.mbgc_fasta_probe_host.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, C.c_int, C.POINTER(ProbeState), C.POINTER(ProbeResult)]
        L.mbgc_fasta_compare_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(ComparePiece), C.c_uint64,
                                             C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_double)]
        L.mbgc_fasta_inflate_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(InflateJob), C.c_uint64,
                                             C.POINTER(InflateResult), C.POINTER(C.c_double)]
        L.mbgc_fasta_deflate_bound.argtypes = [C.c_uint64]
        L.mbgc_fasta_deflate_bound.restype = C.c_uint64
        L.mbgc_fasta_deflate_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(DeflateJob), C.c_uint64, C.c_void_p, C.c_uint64,
                                             C.POINTER(DeflateResult), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_pack_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PackPiece), C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_match_headers_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p,
                                                   C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        L.mbgc_fasta_crc_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        L.mbgc_fasta_find_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64,
                                          C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_find_iupac_dev.argtypes = L.mbgc_fasta_find_dev.argtypes
        L.mbgc_fasta_find_iupac_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mbgc_fasta_find_iupac_last.restype = None
        L.mbgc_fasta_stats_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_stats_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mbgc_fasta_stats_last.restype = None
        L.mbgc_fasta_sketch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                            C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_sketch_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mbgc_fasta_sketch_last.restype = None
        L.mbgc_fasta_sketch_sort_ms.argtypes = [C.c_void_p]
        L.mbgc_fasta_sketch_sort_ms.restype = C.c_double
        L.mbgc_fasta_sketch_pairs_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_double)]
        L.mbgc_fasta_dups_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_dups_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_dups_last.restype = None
        L.mbgc_fasta_dups_comp_table.argtypes = []
        L.mbgc_fasta_dups_comp_table.restype = C.POINTER(C.c_uint8)
        L.mbgc_fasta_screen_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(CrcRec), C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                            C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_screen_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mbgc_fasta_screen_last.restype = None
        L.mbgc_fasta_crc_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.mbgc_fasta_crc_combine.restype = C.c_uint32
        L._fasta_ready = True
    return L


def _ranges(ranges):
    """rows of (off, len) -> (the uint64 array that holds them for the call, it as mbgc_fasta_crc_rec_t *, their number)"""
    rows = np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
    return rows, rows.ctypes.data_as(C.POINTER(CrcRec)), rows.shape[0]


def _with_capacity(call, first, given, too_many, calls):
    """call(cap) -> (status, the count the call states, a function that makes the answer): made with the capacity `given`, or, when
    the caller left it open, with `first` and then with the count a -104 states, `calls` times at most (math.inf: as often as it
    takes). A -104 that is left raises too_many (.needed = the count), any other failure SwsemError"""
    cap = first if given is None else int(given)
    made = 0
    while True:
        r, needed, answer = call(cap)
        made += 1
        if r == -104 and given is None and made < calls:
            cap = needed
            continue
        if r == -104:
            raise too_many(_lib().mbgc_fasta_last_error().decode(), needed)
        if r:
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return answer()


def dups_comp_table():
    """the 256 entries of the header's comp table (mbgc_fasta_dups_comp_table), as bytes"""
    return bytes(_lib().mbgc_fasta_dups_comp_table()[:256])


class FastaParser:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        self._rec_cap = 4096
        if _lib().mbgc_fasta_create(C.byref(self.h), device):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())

    def close(self):
        if self.h:
            _lib().mbgc_fasta_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parse_batch_dev(self, files_ptr, file_offsets, out_ptr, out_cap, uppercase=False, lossy=False, flags=None):
        """files_ptr: device buffer holding the files back to back, file f at [file_offsets[f], file_offsets[f+1]).
        lossy: the rule of `mbgc c -L` (mbgc_fasta_parse_batch_dev2 with MBGC_FASTA_LOSSY); flags: that entry point with these
        flags as they are (0: the lossless rule through it).
        -> dict(seq_base [nf+1], rec_base [nf+1], records (structured array), dna_line_len [nf], status [nf])"""
        if flags is None and lossy:
            flags = LOSSY | (UPPERCASE if uppercase else 0)
        offs = np.ascontiguousarray(file_offsets, dtype=np.uint64)
        nf = offs.size - 1
        P = C.POINTER(C.c_uint64)
        seq_base, rec_base = np.zeros(nf + 1, dtype=np.uint64), np.zeros(nf + 1, dtype=np.uint64)
        line, status = np.zeros(nf, dtype=np.uint64), np.zeros(nf, dtype=np.int32)
        rec_cap = max(self._rec_cap, nf)
        while True:
            recs = (Record * rec_cap)()
            call = _lib().mbgc_fasta_parse_batch_dev if flags is None else _lib().mbgc_fasta_parse_batch_dev2
            r = call(self.h, files_ptr, offs.ctypes.data_as(P), nf, int(uppercase) if flags is None else int(flags), out_ptr, out_cap,
                     seq_base.ctypes.data_as(P), recs, rec_cap, rec_base.ctypes.data_as(P),
                     line.ctypes.data_as(P), status.ctypes.data_as(C.POINTER(C.c_int)))
            if r == -104 and int(rec_base[-1]) > rec_cap:              # the table was too small: the call says how many it needs
                rec_cap = self._rec_cap = int(rec_base[-1])
                continue
            if r:
                raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
            break
        n = int(rec_base[-1])
        arr = np.frombuffer(recs, dtype=[("headerOff", "<u8"), ("headerLen", "<u8"), ("seqOff", "<u8"), ("seqLen", "<u8")], count=n).copy()
        return dict(seq_base=seq_base, rec_base=rec_base, records=arr, dna_line_len=line, status=status)

    def parse_host(self, data, uppercase=False, lossy=False):
        """one file in host memory (mbgc_fasta_parse_host, or _host2 with MBGC_FASTA_LOSSY): uploaded, parsed, its sequences downloaded
        -> dict(status, records=[(header bytes, sequence bytes)], dna_line_len, seq=the sequences back to back)"""
        data = bytes(data)
        src = np.frombuffer(data + b"\0", dtype=np.uint8)
        out = np.zeros(max(len(data), 1), dtype=np.uint8)
        nb, nrec, line, status = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rec_cap = self._rec_cap
        while True:
            recs = (Record * rec_cap)()
            args = (src.ctypes.data_as(C.c_void_p), len(data))
            rest = (out.ctypes.data_as(C.c_void_p), C.byref(nb), recs, rec_cap, C.byref(nrec), C.byref(line), C.byref(status))
            if lossy:
                r = _lib().mbgc_fasta_parse_host2(self.h, *args, LOSSY | (UPPERCASE if uppercase else 0), *rest)
            else:
                r = _lib().mbgc_fasta_parse_host(self.h, *args, int(uppercase), *rest)
            if r == -104 and nrec.value > rec_cap:
                rec_cap = self._rec_cap = int(nrec.value)
                continue
            if r:
                raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
            break
        seq = out[: nb.value].tobytes()
        records = [(data[x.headerOff: x.headerOff + x.headerLen], seq[x.seqOff: x.seqOff + x.seqLen]) for x in recs[: nrec.value]]
        return dict(status=status.value, records=records, dna_line_len=line.value, seq=seq)

    def probe_dev(self, seq_ptr, seq_bytes, offsets, lengths, k=32, state=(PROBE_MAX_LEN, 0)):
        """probeProteinsProfile over the records seq_ptr[offsets[r] .. + lengths[r]) of a device buffer of seq_bytes bytes, from
        state = (probe_remaining, probe_non_std_count) -> (fired, record index, state afterwards)"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        assert off.size == ln.size
        st, res = ProbeState(int(state[0]), int(state[1])), ProbeResult()
        P = C.POINTER(C.c_uint64)
        if _lib().mbgc_fasta_probe_dev(self.h, seq_ptr, int(seq_bytes), off.ctypes.data_as(P), ln.ctypes.data_as(P), off.size, int(k),
                                       C.byref(st), C.byref(res)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        assert (st.probe_remaining, st.probe_non_std_count) == (res.state.probe_remaining, res.state.probe_non_std_count)
        return bool(res.fired), int(res.record), (st.probe_remaining, st.probe_non_std_count)

    def probe_host(self, data, k=32, state=(PROBE_MAX_LEN, 0), uppercase=False, records=None):
        """one file in host memory: parsed (mbgc_fasta_parse_host2), then its first `records` records (all: None) probed where the
        parse left them on the device (mbgc_fasta_probe_host) -> as probe_dev"""
        data = bytes(data)
        src = np.frombuffer(data + b"\0", dtype=np.uint8)
        out = np.zeros(max(len(data), 1), dtype=np.uint8)
        nb, nrec, line, status = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rec_cap = max(self._rec_cap, len(data) // 2 + 1)
        recs = (Record * rec_cap)()
        if _lib().mbgc_fasta_parse_host2(self.h, src.ctypes.data_as(C.c_void_p), len(data), UPPERCASE if uppercase else 0, out.ctypes.data_as(C.c_void_p),
                                         C.byref(nb), recs, rec_cap, C.byref(nrec), C.byref(line), C.byref(status)) or status.value:
            raise binding.SwsemError("parse: status %d %s" % (status.value, _lib().mbgc_fasta_last_error().decode()))
        n = nrec.value if records is None else min(int(records), nrec.value)
        st, res = ProbeState(int(state[0]), int(state[1])), ProbeResult()
        if _lib().mbgc_fasta_probe_host(self.h, recs, n, int(k), C.byref(st), C.byref(res)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return bool(res.fired), int(res.record), (st.probe_remaining, st.probe_non_std_count)

    def split_dev(self, bytes_ptr, n, is_file_end, first_min, next_min, max_elems):
        """mgmpInSplit_next over the window bytes_ptr[0..n) in HBM (it starts at an element start): the end offsets of the
        elements whose end the window decides, at most max_elems. Fewer than asked for (none, even) when the window is not the
        file's end and the search ran off it: extend the window and call again."""
        ends = np.zeros(max(int(max_elems), 1), dtype=np.uint64)
        ne = C.c_int(0)
        if _lib().mbgc_fasta_split_dev(self.h, bytes_ptr, int(n), int(bool(is_file_end)), int(first_min), int(next_min), int(max_elems),
                                       ends.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ne)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return [int(e) for e in ends[:ne.value]]

    def split_buf_dev(self, buf_ptr, start, n, scanned_before, is_file_end, first_min, next_min, max_elems):
        """split_dev for a buffer that grows: elements from `start`, ends as offsets in the buffer; buf[0..scanned_before) is
        unchanged since this parser's last call and is not read again by the streaming pass"""
        ends = np.zeros(max(int(max_elems), 1), dtype=np.uint64)
        ne = C.c_int(0)
        if _lib().mbgc_fasta_split_buf_dev(self.h, buf_ptr, int(start), int(n), int(scanned_before), int(bool(is_file_end)), int(first_min),
                                           int(next_min), int(max_elems), ends.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ne)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return [int(e) for e in ends[:ne.value]]

    def split_buf_dev2(self, buf_ptr, start, n, scanned_before, is_file_end, first_min, next_min, flags, max_elems):
        """split_buf_dev with a rule for what a mark is: SPLIT_LINE_START (only at offset 0 of the buffer or right behind a line
        feed), SPLIT_AT ('@' beside '>'); flags = 0 is split_buf_dev"""
        ends = np.zeros(max(int(max_elems), 1), dtype=np.uint64)
        ne = C.c_int(0)
        if _lib().mbgc_fasta_split_buf_dev2(self.h, buf_ptr, int(start), int(n), int(scanned_before), int(bool(is_file_end)), int(first_min),
                                            int(next_min), int(flags), int(max_elems), ends.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ne)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return [int(e) for e in ends[:ne.value]]

    def format_dev(self, seq_ptr, seq_bytes, headers_ptr, header_bytes, records, text_ptr, text_cap):
        """the inverse of parse_batch_dev: records = rows of (seqOff, seqLen, headerOff, headerLen, lineLen) -> (text offsets
        [nrec + 1], the last one the total; the kernel's ms). TextTooSmall when the text does not fit text_cap (nothing written)."""
        rows = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 5)
        n = rows.shape[0]
        offs = np.zeros(n + 1, dtype=np.uint64)
        ms = C.c_double(0)
        r = _lib().mbgc_fasta_format_dev(self.h, seq_ptr, int(seq_bytes), headers_ptr, int(header_bytes),
                                         rows.ctypes.data_as(C.POINTER(FormatRecord)), n, text_ptr, int(text_cap),
                                         offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ms))
        if r == -104:
            raise TextTooSmall(_lib().mbgc_fasta_last_error().decode(), int(offs[-1]))
        if r:
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return offs, ms.value

    def compare_dev(self, a_ptr, a_bytes, b_ptr, b_bytes, pieces, nslots, first_diff=None):
        """pieces = rows of (aOff, bOff, len, slot): a[aOff, aOff + len) against b[bOff, bOff + len) on the device -> (first differing
        offset within its piece per slot, the smallest over the slot's pieces, NO_DIFFERENCE when none differ [nslots]; the kernel's
        ms). first_diff: the uint64 array to fill (a refused call leaves it untouched and raises)."""
        rows = [tuple(int(v) for v in r) for r in pieces]
        arr = (ComparePiece * max(len(rows), 1))(*rows)
        out = np.zeros(int(nslots), dtype=np.uint64) if first_diff is None else first_diff
        assert out.dtype == np.uint64 and out.size >= int(nslots) and out.flags.c_contiguous
        ms = C.c_double(0)
        if _lib().mbgc_fasta_compare_dev(self.h, a_ptr, int(a_bytes), b_ptr, int(b_bytes), arr, len(rows), out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         int(nslots), C.byref(ms)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return out, ms.value

    def pack_dev(self, src_ptr, src_bytes, pieces, dst_ptr, dst_cap, uppercase=False):
        """pieces = rows of (srcOff, len): src[srcOff, srcOff + len) back to back in dst on the device, folded to upper case as the
        parser folds a base when `uppercase` -> (the pieces' offsets in dst [n + 1], the last one the total; the kernel's ms).
        PackTooSmall when they do not fit dst_cap (nothing written). A refused call (a piece outside the source, buffers that
        overlap) raises and launches nothing."""
        rows = np.ascontiguousarray(pieces, dtype=np.uint64).reshape(-1, 2)
        n = rows.shape[0]
        offs = np.zeros(n + 1, dtype=np.uint64)
        ms = C.c_double(0)
        r = _lib().mbgc_fasta_pack_dev(self.h, src_ptr, int(src_bytes), rows.ctypes.data_as(C.POINTER(PackPiece)), n, UPPERCASE if uppercase else 0,
                                       dst_ptr, int(dst_cap), offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ms))
        if r == -104:
            raise PackTooSmall(_lib().mbgc_fasta_last_error().decode(), int(offs[-1]))
        if r:
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return offs, ms.value

    def match_headers_dev(self, headers_ptr, header_bytes, offsets, lengths, patterns):
        """which of the headers headers_ptr[offsets[r], offsets[r] + lengths[r]) of a device buffer of header_bytes bytes contain one of
        `patterns` (bytes objects) as a substring -> (a bool per record, the kernel's ms). A refused call (an empty pattern, one with a
        line feed, a header outside the buffer) raises and launches nothing."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        assert off.size == ln.size
        pats = [bytes(x) for x in patterns]
        blob = np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8)      # (one byte more: an empty list still has an address)
        pat_off = np.concatenate([[0], np.cumsum([len(x) for x in pats], dtype=np.uint64)]).astype(np.uint64)
        words = np.zeros((off.size + 31) // 32, dtype=np.uint32)
        ms = C.c_double(0)
        P = C.POINTER(C.c_uint64)
        if _lib().mbgc_fasta_match_headers_dev(self.h, headers_ptr, int(header_bytes), off.ctypes.data_as(P), ln.ctypes.data_as(P), off.size,
                                               blob.ctypes.data_as(C.c_void_p), pat_off.ctypes.data_as(P), len(pats),
                                               words.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        bits = (words[np.arange(off.size) >> 5] >> (np.arange(off.size, dtype=np.uint32) & 31)) & 1 if off.size else np.zeros(0, dtype=np.uint32)
        return bits.astype(bool), ms.value

    def crc_dev(self, seq_ptr, seq_bytes, ranges):
        """ranges = rows of (off, len): zlib's crc32 of seq[off, off + len) of a device buffer of seq_bytes bytes, one per range, taken
        on the device in one launch -> (uint32 per range, the kernel's ms). The ranges may overlap, repeat and come in any order; one
        of no bytes gives 0. A refused call (a range outside the buffer) raises and launches nothing."""
        rows, recs, n = _ranges(ranges)                                  # (rows: held so that recs stays valid through the call)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        ms = C.c_double(0)
        if _lib().mbgc_fasta_crc_dev(self.h, seq_ptr, int(seq_bytes), recs, n, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return out[:n], ms.value

    def find_dev(self, seq_ptr, seq_bytes, ranges, patterns, max_mismatches=0, hit_cap=None):
        """ranges = rows of (off, len), the records seq[off, off + len) of a device buffer of seq_bytes bytes; patterns: bytes objects,
        ASCII letters only. Where does a pattern stand in a record with at most max_mismatches substitutions, letters compared
        without case -> (structured array of HIT_DTYPE: pos, rec, pattern, mismatches — every hit once, sorted by (rec, pos, pattern);
        the kernel's ms). hit_cap=None: the call is made again with the capacity it asks for when the hits do not fit; a given
        hit_cap: HitsTooMany (.needed = the exact count) when they do not. A refused call (a pattern that is too short for
        max_mismatches, too long or holds a non-letter, max_mismatches > 3, a record outside the buffer) raises and launches nothing."""
        rows, recs, nrec = _ranges(ranges)
        pats = [bytes(x) for x in patterns]
        blob = np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8)      # (one byte more: an empty list still has an address)
        pat_off = np.concatenate([[0], np.cumsum([len(x) for x in pats], dtype=np.uint64)]).astype(np.uint64)
        n, ms = C.c_uint64(0), C.c_double(0)

        def call(cap):
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            r = _lib().mbgc_fasta_find_dev(self.h, seq_ptr, int(seq_bytes), recs, nrec, blob.ctypes.data_as(C.c_void_p), pat_off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           len(pats), int(max_mismatches), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(ms))
            return r, int(n.value), lambda: (out[: n.value].copy(), ms.value)
        return _with_capacity(call, 4096, hit_cap, HitsTooMany, calls=math.inf)

    def find_iupac_dev(self, seq_ptr, seq_bytes, ranges, patterns, max_mismatches=0, hit_cap=None):
        """find_dev with IUPAC patterns (mbgc_fasta_find_iupac_dev): a pattern letter is a set of bases (IUPAC_SETS), a text byte has a
        base only if it is one of acgtuACGTU, and a position matches iff the text's base is in the pattern letter's set — a text N
        matches nothing. Same arguments, same answer, same HitsTooMany; a refused call (a letter outside the table, a segment whose
        best window of 8 letters stands for more than FIND_IUPAC_MAX_EXPAND sequences, and find_dev's refusals) raises and launches
        nothing."""
        rows, recs, nrec = _ranges(ranges)
        pats = [bytes(x) for x in patterns]
        blob = np.frombuffer(b"".join(pats) + b"\0", dtype=np.uint8)      # (one byte more: an empty list still has an address)
        pat_off = np.concatenate([[0], np.cumsum([len(x) for x in pats], dtype=np.uint64)]).astype(np.uint64)
        n, ms = C.c_uint64(0), C.c_double(0)

        def call(cap):
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            r = _lib().mbgc_fasta_find_iupac_dev(self.h, seq_ptr, int(seq_bytes), recs, nrec, blob.ctypes.data_as(C.c_void_p), pat_off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 len(pats), int(max_mismatches), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(ms))
            return r, int(n.value), lambda: (out[: n.value].copy(), ms.value)
        return _with_capacity(call, 4096, hit_cap, HitsTooMany, calls=math.inf)

    def find_iupac_last(self):
        """-> (the rows of the last find_iupac_dev call's table, the rows its lanes walked)"""
        rows, walked = C.c_uint64(0), C.c_uint64(0)
        _lib().mbgc_fasta_find_iupac_last(self.h, C.byref(rows), C.byref(walked))
        return int(rows.value), int(walked.value)

    def stats_dev(self, seq_ptr, seq_bytes, ranges, flags=STATS_COUNTS | STATS_NRUNS | STATS_LOWER, min_run_n=1, min_run_lower=1, run_cap=None):
        """ranges = rows of (off, len), the records seq[off, off + len) of a device buffer of seq_bytes bytes -> (counts: an (n, 8)
        uint64 array, columns COUNTS_COLUMNS — zeros without STATS_COUNTS; runs: a structured array of RUN_DTYPE (start, len, rec,
        cls: 0 = N / n with STATS_NRUNS, 1 = 'a'..'z' with STATS_LOWER), the maximal runs inside a record of at least min_run_n /
        min_run_lower bytes (0 is read as 1), sorted by (rec, cls, start); the kernel's ms). run_cap=None: the call is made once more
        with the count it states when the runs do not fit; a given run_cap: RunsTooMany (.needed = the exact count) when they do
        not. A record outside the buffer raises and launches nothing. last_stats(): the edges and the kernel's reruns of this call."""
        rows, recs, nrec = _ranges(ranges)
        counts = np.zeros((max(nrec, 1), 8), dtype=np.uint64)
        n, ms = C.c_uint64(0), C.c_double(0)

        def call(cap):
            out = np.zeros(max(cap, 1), dtype=RUN_DTYPE)
            r = _lib().mbgc_fasta_stats_dev(self.h, seq_ptr, int(seq_bytes), recs, nrec, int(flags), int(min_run_n), int(min_run_lower),
                                            counts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(ms))
            return r, int(n.value), lambda: (counts[:nrec].copy(), out[: n.value].copy(), ms.value)
        return _with_capacity(call, 4096, run_cap, RunsTooMany, calls=2)

    def last_stats(self):
        """(edges, reruns) of the last stats_dev call: the edges its kernel reported, and how often it ran again for a larger buffer"""
        e, k = C.c_uint64(0), C.c_uint64(0)
        _lib().mbgc_fasta_stats_last(self.h, C.byref(e), C.byref(k))
        return int(e.value), int(k.value)

    def sketch_dev(self, seq_ptr, seq_bytes, ranges, groups, ngroups, k=21, max_hash=(2 ** 64 - 1) // 1000, cap=None):
        """ranges = rows of (off, len), the records seq[off, off + len) of a device buffer of seq_bytes bytes; groups = a group id
        < ngroups per record -> (hashes: a uint64 array, the groups' sketches back to back, each strictly ascending; group_start: ngroups
        + 1 offsets into it; kmers: the valid k-mer positions per group; the scan kernel's ms). The hash is the header's (fmix64 of the
        canonical k-mer ^ a seed, kept when <= max_hash), not Mash's. cap=None: the call is made once more with the count it states
        when the hashes do not fit; a given cap: SketchTooLarge (.needed = the exact count) when they do not. k outside 1..32, a record
        outside the buffer or a group >= ngroups raises and launches nothing. last_sketch(): the rows, the reruns and the sort's ms."""
        rows, recs, nrec = _ranges(ranges)
        grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if grp.size != nrec:
            raise ValueError("sketch_dev: %d records, %d group ids" % (nrec, grp.size))
        start, kmers = np.zeros(int(ngroups) + 1, dtype=np.uint64), np.zeros(max(int(ngroups), 1), dtype=np.uint64)
        n, ms = C.c_uint64(0), C.c_double(0)

        def call(size):
            out = np.zeros(max(size, 1), dtype=np.uint64)
            r = _lib().mbgc_fasta_sketch_dev(self.h, seq_ptr, int(seq_bytes), recs, nrec, grp.ctypes.data_as(C.c_void_p), int(ngroups), int(k), int(max_hash),
                                             out.ctypes.data_as(C.c_void_p), size, start.ctypes.data_as(C.c_void_p), kmers.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(ms))
            return r, int(n.value), lambda: (out[: n.value].copy(), start, kmers[: int(ngroups)].copy(), ms.value)
        return _with_capacity(call, 4096, cap, SketchTooLarge, calls=2)

    def last_sketch(self):
        """(rows, reruns, sort_ms) of the last sketch_dev call: the (hash, group) rows its kernel reported, how often it ran again for a
        larger row buffer, and the ms of the sorts and the compaction behind it"""
        e, k = C.c_uint64(0), C.c_uint64(0)
        _lib().mbgc_fasta_sketch_last(self.h, C.byref(e), C.byref(k))
        return int(e.value), int(k.value), float(_lib().mbgc_fasta_sketch_sort_ms(self.h))

    def sketch_pairs_dev(self, hashes, group_start, pairs=None):
        """hashes, group_start as sketch_dev returns them; pairs = rows of (i, j), or None for all i < j in row-major order -> (shared:
        a uint32 array, |sketch i & sketch j| per pair; the kernel's ms). A list that does not ascend strictly is refused."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1)
        start = np.ascontiguousarray(group_start, dtype=np.uint64).reshape(-1)
        ngroups = start.size - 1
        if pairs is None:
            rows, npairs, ptr = None, ngroups * (ngroups - 1) // 2, None
        else:
            rows = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
            npairs, ptr = rows.shape[0], rows.ctypes.data_as(C.c_void_p)
        if start.size < 1 or int(start[-1]) > h.size:
            raise ValueError("sketch_pairs_dev: group_start reaches past the hashes")
        shared, ms = np.zeros(max(npairs, 1), dtype=np.uint32), C.c_double(0)
        r = _lib().mbgc_fasta_sketch_pairs_dev(self.h, h.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p), ngroups, ptr, npairs, shared.ctypes.data_as(C.c_void_p), C.byref(ms))
        if r:
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return shared[:npairs].copy(), ms.value

    def dups_dev(self, seq_ptr, seq_bytes, ranges, flags=0, out=None):
        """ranges = rows of (off, len), the records seq[off, off + len) of a device buffer of seq_bytes bytes -> (a structured array of
        DUP_DTYPE, one row per record: rep = the lowest index of the record's class, strand = 0 when the record equals rep read forward
        (also when it equals it both ways), 1 when it equals only rep's reverse complement; the number of classes; k_fa_dups's ms).
        Same = equal under fold (letters without case; DUPS_EXACT_CASE: as they are), forward or — unless DUPS_FORWARD_ONLY — as the
        reverse complement under the header's comp table. Exact: every duplicate is compared byte by byte on the device.
        DUPS_WEAK_HASH (tests) keeps 4 bits of the fingerprints; the answer does not change. out: an array of DUP_DTYPE to fill (a
        refused call — a record outside the buffer, an unknown flag — raises, launches nothing and leaves it as it was).
        last_dups(): the buckets, the pairs compared and refuted, the comparisons' ms."""
        rows, recs, n = _ranges(ranges)                                  # (rows: held so that recs stays valid through the call)
        if out is None:
            out = np.zeros(max(n, 1), dtype=DUP_DTYPE)
        if out.dtype != DUP_DTYPE or out.size < n or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("dups_dev: out must be a contiguous array of DUP_DTYPE with a row per record")
        classes, ms = C.c_uint64(0), C.c_double(0)
        if _lib().mbgc_fasta_dups_dev(self.h, seq_ptr, int(seq_bytes), recs, n, int(flags), out.ctypes.data_as(C.c_void_p), C.byref(classes), C.byref(ms)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return out[:n], int(classes.value), ms.value

    def last_dups(self):
        """(buckets, verified, refuted, verify_ms) of the last dups_dev call: the groups of equal (length, canonical fingerprint), the
        pairs k_fa_dups_verify compared, those it found different, and the ms of its launches"""
        b, v, r, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        _lib().mbgc_fasta_dups_last(self.h, C.byref(b), C.byref(v), C.byref(r), C.byref(ms))
        return int(b.value), int(v.value), int(r.value), float(ms.value)

    def screen_dev(self, seq_ptr, seq_bytes, ranges, groups, ngroups, keys, k=21, found_cap=None, hits=False, hit_cap=None):
        """ranges = rows of (off, len), the records seq[off, off + len) of a device buffer of seq_bytes bytes; groups = a group id
        < ngroups per record; keys = a strictly ascending uint64 list of canonical k-mers (min(fw, rc) of the header, no hash) -> (found: a
        uint32 array, per group the ascending INDICES of the keys that occur in one of its records, back to back; group_start: ngroups + 1
        offsets into it; hit rows: a structured array of SCREEN_HIT_DTYPE (pos, rec, key) sorted by (rec, pos), every hit once — None
        unless `hits`; the scan kernel's ms). found_cap=None: the call is made again with the count it states when the found keys do not
        fit; a given found_cap: ScreenTooLarge (.needed = the exact count). hit_cap likewise, with HitsTooMany. k outside 1..32, no key or
        more than SCREEN_MAX_KEYS, a key with bits above 2 k, keys that do not ascend strictly, a record outside the buffer or a group >=
        ngroups raises and launches nothing. last_screen(): the rows, the filter passes, the reruns and the sorts' ms."""
        rows, recs, nrec = _ranges(ranges)
        grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if grp.size != nrec:
            raise ValueError("screen_dev: %d records, %d group ids" % (nrec, grp.size))
        key = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        key_ptr = (key if key.size else np.zeros(1, dtype=np.uint64)).ctypes.data_as(C.c_void_p)
        start = np.zeros(int(ngroups) + 1, dtype=np.uint64)
        total, n, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        found_size = [4096 if found_cap is None else int(found_cap)]

        def call(cap):
            # (the capacity _with_capacity walks is the hits'; the found keys' is settled here, inside one of its calls)
            while True:
                out = np.zeros(max(found_size[0], 1), dtype=np.uint32)
                rows_out = np.zeros(max(cap, 1), dtype=SCREEN_HIT_DTYPE) if hits else None
                r = _lib().mbgc_fasta_screen_dev(self.h, seq_ptr, int(seq_bytes), recs, nrec, grp.ctypes.data_as(C.c_void_p), int(ngroups), int(k), key_ptr, key.size,
                                                 out.ctypes.data_as(C.c_void_p), found_size[0], start.ctypes.data_as(C.c_void_p), C.byref(total),
                                                 rows_out.ctypes.data_as(C.c_void_p) if hits else None, cap if hits else 0, C.byref(n), C.byref(ms))
                if r == -104 and int(total.value) > found_size[0]:
                    if found_cap is not None:
                        raise ScreenTooLarge(_lib().mbgc_fasta_last_error().decode(), int(total.value))
                    found_size[0] = int(total.value)
                    continue
                return r, int(n.value), lambda: (out[: total.value].copy(), start, rows_out[: n.value].copy() if hits else None, ms.value)
        return _with_capacity(call, 4096, hit_cap, HitsTooMany, calls=math.inf)

    def last_screen(self):
        """(rows, filter_passes, reruns, sort_ms) of the last screen_dev call: the hit rows its kernel reported, the valid positions that
        passed the filter in LDS, how often the kernel ran again for a larger row buffer, and the ms of the sorts and the compaction"""
        rows, passes, reruns, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        _lib().mbgc_fasta_screen_last(self.h, C.byref(rows), C.byref(passes), C.byref(reruns), C.byref(ms))
        return int(rows.value), int(passes.value), int(reruns.value), float(ms.value)

    def inflate_dev(self, gz_ptr, gz_bytes, out_ptr, out_bytes, jobs):
        """jobs = rows of (inOff, inLen, outOff, outCap): the gzip file gz[inOff, inOff + inLen) inflated on the device into
        out[outOff, outOff + outCap) -> ([(status, members, outLen, inUsed)] per job, the kernel's ms). A refused call (a job outside
        the buffers, overlapping output ranges) raises and launches nothing."""
        rows = [tuple(int(v) for v in r) for r in jobs]
        arr = (InflateJob * max(len(rows), 1))(*rows)
        res = (InflateResult * max(len(rows), 1))()
        ms = C.c_double(0)
        if _lib().mbgc_fasta_inflate_dev(self.h, gz_ptr, int(gz_bytes), out_ptr, int(out_bytes), arr, len(rows), res, C.byref(ms)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return [(r.status, r.members, r.outLen, r.inUsed) for r in res[: len(rows)]], ms.value

    def deflate_dev(self, text_ptr, text_bytes, jobs, gz_ptr, gz_cap):
        """jobs = rows of (inOff, inLen): text[inOff, inOff + inLen) compressed on the device into one gzip file each, back to back in
        gz[0, total) -> ([(outOff, outLen, crc32, chunks, storedChunks)] per job, total, both kernels' ms). GzipTooSmall when the
        files do not fit gz_cap (nothing written). A refused call (a job outside the text) raises and launches nothing."""
        rows = [tuple(int(v) for v in r) for r in jobs]
        arr = (DeflateJob * max(len(rows), 1))(*rows)
        res = (DeflateResult * max(len(rows), 1))()
        total, ms = C.c_uint64(0), C.c_double(0)
        r = _lib().mbgc_fasta_deflate_dev(self.h, text_ptr, int(text_bytes), arr, len(rows), gz_ptr, int(gz_cap), res, C.byref(total), C.byref(ms))
        if r == -104:
            raise GzipTooSmall(_lib().mbgc_fasta_last_error().decode(), int(total.value))
        if r:
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return [(x.outOff, x.outLen, x.crc32, x.chunks, x.storedChunks) for x in res[: len(rows)]], int(total.value), ms.value

    def gather_dev(self, src_ptr, src_bytes, offsets, lengths, sep=10):
        """pieces of a device buffer, each followed by the byte sep, packed on the device and downloaded -> bytes"""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        out = np.zeros(int(ln.sum()) + off.size + 1, dtype=np.uint8)
        n = C.c_uint64(0)
        P = C.POINTER(C.c_uint64)
        if _lib().mbgc_fasta_gather_dev(self.h, src_ptr, int(src_bytes), off.ctypes.data_as(P), ln.ctypes.data_as(P), off.size, sep,
                                        out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)):
            raise binding.SwsemError(_lib().mbgc_fasta_last_error().decode())
        return out[: n.value].tobytes()


def crc_combine(crc_a, crc_b, len_b):
    """mbgc_fasta_crc_combine: the CRC-32 of A followed by B from crc32(A), crc32(B) and B's length (host arithmetic; no device)"""
    return int(_lib().mbgc_fasta_crc_combine(int(crc_a), int(crc_b), int(len_b)))
