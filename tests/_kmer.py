"""Inputs shared by the tests of the k-mer length axis (tests/test_oracle_vs_ref.py on the CPU, tests/test_gpu_kmer_lengths.py on
the device): one matching length L per hashed k-mer length K the reference instantiates its hash for
(SlidingWindowSparseEMMatcher.cpp:57-66, initParams :74-87), and generators with fixed seeds."""
import numpy as np

from mbgc_amd import synth

LS = (16, 20, 24, 28, 32, 44, 48, 56, 64, 120)
K_OF_L = {16: 12, 20: 16, 24: 20, 28: 24, 32: 28, 44: 32, 48: 36, 56: 40, 64: 44, 120: 56}
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def assert_covered(rows, L, what=""):
    """a case that matches nothing must fail, not pass empty: at least 50 rows, one of them of length exactly L
    -> (rows, rows of length L), for the record"""
    lens = np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, 3)[:, 1] for r in rows]) if len(rows) else np.zeros(0, dtype=np.uint64)
    n, exact = int(lens.size), int((lens == L).sum())
    assert n >= 50 and exact >= 1, "%s L=%d: %d rows, %d of length L — the case does not cover what it is there for" % (what, L, n, exact)
    assert n == 0 or int(lens.min()) >= L
    return n, exact


def related(n_close, length, seed, far=0.10):
    """n_close genomes 1 % from a random base (2 % from each other) and one `far` from it"""
    base = synth.base_codes(length, seed)
    return [synth.genome(base, i, 0.01) for i in range(n_close)] + [synth.genome(base, n_close, far)]


def planted(L, seed=0, copies=128):
    """-> (reference text, query): the query holds `copies` exact copies each of L - 1, L and L + 1 bases of the reference, every
    copy between two bytes that differ from the reference's neighbours (so the match is exactly as long as the copy) and 23
    unrelated bases. The copies start 149 bases apart: every phase of the 16-base sampling grid occurs, and whether a copy
    holds a sampled K-mer at all depends on it (L - K + 1 of 16 phases for a copy of L bases)."""
    rng = np.random.default_rng(7000 + 31 * L + seed)
    ref = rng.integers(0, 4, 60_000).astype(np.uint8)
    parts = []
    for i in range(3 * copies):
        n, s = L - 1 + i % 3, 512 + 149 * i
        assert s + n + 1 < ref.size
        parts += [rng.integers(0, 4, 23).astype(np.uint8), [(ref[s - 1] + 1 + i % 3) & 3], ref[s:s + n], [(ref[s + n] + 1 + (i // 3) % 3) & 3]]
    return synth.ACGT[ref], synth.ACGT[np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])]


def hard_pair(L, K, seed):
    """-> (g0, g1): two genomes 2 % apart that share a run of one letter longer than K + 64, a run of N and a lower-case stretch"""
    base = synth.base_codes(60_000, seed)
    out = []
    for i in range(2):
        g = synth.genome(base, i, 0.01).copy()
        g[5_000:5_000 + K + 64 + 37] = ord("A")
        g[12_000:12_300] = ord("N")
        g[20_000:20_600] |= 0x20                                       # lower case
        out.append(g)
    return out


def short_contigs(g, L, K):
    """pieces of g of K - 1, K, K + 1, L - 1, L and L + 1 bases, 16 of each, their starts over every phase of the sampling grid"""
    out = []
    for j, n in enumerate((K - 1, K, K + 1, L - 1, L, L + 1)):
        for i in range(16):
            s = 30_000 + 1_000 * j + 37 * i
            out.append(g[s:s + n].copy())
    return out


def proteins(n, length, seed, div=0.01):
    """n sequences over the 20-letter amino-acid alphabet, `div` substitutions each from a common ancestor"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 20, length)
    out = []
    for i in range(n):
        g = base.copy()
        m = rng.random(length) < div
        g[m] = (g[m] + rng.integers(1, 20, int(m.sum()))) % 20
        out.append(AMINO[g])
    return out


def wrap_steps(L, seed, steps=14, rate=0.01):
    """the schedule of test_wrap_quirk_and_locks: `steps` pieces of 20 000 .. 60 000 bases of one genome, `rate` substitutions each;
    -> list of (piece, load its reverse complement, add a separator of its own)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, 60_000)
    out = []
    for step in range(steps):
        g = base.copy()
        mask = rng.random(g.size) < rate
        g[mask] = (g[mask] + 1) & 3
        out.append((synth.ACGT[g][: int(rng.integers(20_000, 60_000))], bool(step % 3 == 0), bool(step % 2)))
    return out
