"""The protein-profile probe of `mbgc c`, restated in Python (MGMP_Params::probeProteinsProfile, matching/MGMP_Params.h:86-127, as
loadG0Ref calls it, MultipleGenomeMatchingProcessor.cpp:82-105), and the inputs the probe's tests share with the fixture generator
(tests/golden/make_proteins_golden.py): everything is generated from numpy.random.RandomState seeds, nothing is stored as FASTA."""
import numpy as np

MIN_PROBE_LEN, MAX_PROBE_LEN, MAX_PCT = 256, 65536, 10
STD = frozenset(b"acgtuACGTUN")                                   # (a lowercase n is NOT standard)
START = (MAX_PROBE_LEN, 0)                                        # probe_remaining, probe_non_std_count

AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)    # the 20 amino-acid letters: A C G T N are standard symbols too
NONSTD = np.frombuffer(b"DEFHIKLMPQRSVWY", dtype=np.uint8)        # those of them the probe counts
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def probe_record(seq, state, k=32):
    """one call of probeProteinsProfile -> (fired, state). An empty record (the reference divides by zero there) leaves the state
    untouched and does not fire."""
    remaining, count = state
    if remaining == 0:
        return False, state
    n = min(len(seq), remaining)
    if n == 0:
        return False, state
    remaining -= n
    count += sum(1 for c in bytes(seq[:n]) if c not in STD)
    probe_len = MAX_PROBE_LEN - remaining
    if probe_len >= MIN_PROBE_LEN and k != 16 and count * 100 // n > MAX_PCT:
        return True, (0, count)
    return False, (remaining, count)


def probe_records(records, state=START, k=32):
    """every record in order -> (fired, index of the record that fired or 0, state)"""
    fired, at = False, 0
    for i, r in enumerate(records):
        f, state = probe_record(r, state, k)
        if f and not fired:
            fired, at = True, i
    return fired, at, state


def switches(records, sequential, k=32, state=START, uppercase=False):
    """does loading these records as the initial reference switch the profile? -> (switched, state). Rounds: the first record that
    fires switches. Sequential (-t1, -m 3, a single file): the first record's verdict only; the records behind it are probed while
    fewer than MIN_PROBE_LEN bases have been seen, and their verdicts are dropped (MGMP.cpp:91-98)."""
    if uppercase:
        records = [bytes(r).upper() for r in records]
    if not sequential:
        fired, _, state = probe_records(records, state, k)
        return fired, state
    if not records:
        return False, state
    fired, state = probe_record(records[0], state, k)
    probed, i = len(records[0]), 1
    while probed < MIN_PROBE_LEN and i < len(records):
        _, state = probe_record(records[i], state, k)
        probed += len(records[i])
        i += 1
    return fired, state


# ---------------------------------------------------------------- inputs

def draw(rs, alphabet, n):
    return alphabet[rs.randint(0, alphabet.size, size=n)].tobytes()


def with_nonstd(rs, n, bad):
    """n DNA bases of which exactly `bad`, at drawn places, are letters the probe counts"""
    a = np.frombuffer(draw(rs, DNA, n), dtype=np.uint8).copy()
    at = rs.permutation(n)[:bad]
    a[at] = NONSTD[rs.randint(0, NONSTD.size, size=bad)]
    return a.tobytes()


def rule_cases():
    """name -> (records of the initial reference's file, options of `c`, sequential schedule?)"""
    rs = np.random.RandomState(20241)
    two = lambda dna: [draw(rs, NONSTD, 200), draw(rs, DNA, dna)]
    n15 = np.frombuffer(draw(rs, DNA, 4000), dtype=np.uint8).copy()
    n15[rs.permutation(4000)[:600]] = ord("n")
    prot = [draw(rs, AMINO, 3000)]
    c = {
        "pct10_of_256": ([with_nonstd(rs, 256, 26)], [], False),                       # 26 * 100 / 256 = 10: not above
        "pct11_of_256": ([with_nonstd(rs, 256, 29)], [], False),                       # 29 * 100 / 256 = 11
        "running_count_over_1500": (two(1500), [], False),                             # 200 * 100 / 1500 = 13, at record 1
        "running_count_over_2000": (two(2000), [], False),                             # 200 * 100 / 2000 = 10
        "running_count_sequential": (two(1500), ["-t1"], True),                        # the first record is shorter than 256
        "dna_65536_then_protein": ([draw(rs, DNA, 65536), draw(rs, AMINO, 5000)], [], False),
        # a record across the limit: 536 of its 1000 bytes are probed. 60 * 100 / 536 = 11 (over all 1000: 6) ...
        "straddle_clipped_divisor": ([draw(rs, DNA, 65000), with_nonstd(rs, 536, 60) + draw(rs, DNA, 464)], [], False),
        # ... and what lies behind the limit is not counted
        "straddle_clipped_count": ([draw(rs, DNA, 65000), draw(rs, DNA, 536) + draw(rs, NONSTD, 464)], [], False),
        "lowercase_n_15pct": ([n15.tobytes()], [], False),
        "lowercase_n_15pct_U": ([n15.tobytes()], ["-U"], False),
        "protein_k16": (prot, ["-k", "16"], False),
        "protein_k24": (prot, ["-k", "24"], False),
    }
    return c


def case_k(opts):
    return int(opts[opts.index("-k") + 1]) if "-k" in opts else 32


def fasta(records, tag, line=60):
    out = []
    for i, r in enumerate(records):
        out.append(b">%s_%d\n" % (tag.encode(), i))
        out.extend(r[o:o + line] + b"\n" for o in range(0, len(r), line))
    return b"".join(out)


def second_file():
    """the target beside a rule case's initial reference (a list of one file would be matched sequentially)"""
    return [draw(np.random.RandomState(20242), DNA, 3000)]


def collection():
    """4 files x 3 records x 20 000 residues over the 20 amino-acid letters; files 1 to 3 are 2 % substitutions of file 0"""
    rs = np.random.RandomState(20243)
    base = [np.frombuffer(draw(rs, AMINO, 20_000), dtype=np.uint8) for _ in range(3)]
    files = [[b.tobytes() for b in base]]
    for _ in range(3):
        recs = []
        for b in base:
            m = b.copy()
            at = rs.permutation(m.size)[: m.size // 50]
            m[at] = AMINO[(np.searchsorted(AMINO, m[at]) + rs.randint(1, AMINO.size, size=at.size)) % AMINO.size]
            recs.append(m.tobytes())
        files.append(recs)
    return files
