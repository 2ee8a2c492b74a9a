"""Single fasta file mode (`mbgc c -i`): a restatement of the rule by which the reference cuts one multi-FASTA byte stream into
the initial reference and the targets, mgmpInSplit_next(iter, minSplitSize, '>') (matching/input_with_libdeflate_wrapper.cpp:
150-171, called at MultipleGenomeMatchingProcessor.cpp:75 and :495), and what the tests build on it. Test infrastructure only."""
import numpy as np

MIN_REF_INIT_SIZE = 1 << 16      # MGMP_Params.h:47, element 0 (the initial reference)
MIN_BASIC_BLOCK_SIZE = 1 << 21   # MGMP_Params.h:48, every later element


def split_window(data, is_file_end=True, first_min=MIN_REF_INIT_SIZE, next_min=MIN_BASIC_BLOCK_SIZE, max_elems=None):
    """End offsets of the elements of `data`, a window that starts at an element start. An element ends at the first '>' at or
    behind its start + minimum (any '>', also one inside a header line); when start + minimum >= the file's size or no such
    byte follows, at the end of the file. A window that is not the file's end decides only the ends that lie inside it."""
    ends, s, n = [], 0, len(data)
    while s != n and (max_elems is None or len(ends) < max_elems):
        thr = s + (next_min if ends else first_min)
        e = data.find(b">", thr) if thr < n else -1
        if e < 0:
            if not is_file_end:
                break
            e = n
        ends.append(e)
        s = e
    return ends


def elements(data, first_min=MIN_REF_INIT_SIZE, next_min=MIN_BASIC_BLOCK_SIZE):
    """the file's elements as bytes: [0] is the initial reference G0, the others are the targets of the parallel schedule"""
    ends = split_window(data, True, first_min, next_min)
    return [data[a:b] for a, b in zip([0] + ends[:-1], ends)]


def parsed(elem):
    """(contigs as uint8 arrays, DNA line length) of an element, as kseq_read_lossless_fasta reads it (the C oracle)"""
    import _fasta
    r = _fasta.oracle_parse(elem)
    assert r["status"] == 0, r["status"]
    return [np.frombuffer(seq, dtype=np.uint8) for _, seq in r["records"]], r["dna_line_len"]


def multi_fasta(contigs, width=80, first_id=0, crlf=False):
    """contigs (uint8 arrays) as one multi-FASTA image"""
    from mbgc_amd import synth
    data = b"".join(synth.fasta_bytes(c, first_id + i, width) for i, c in enumerate(contigs))
    return data.replace(b"\n", b"\r\n") if crlf else data
