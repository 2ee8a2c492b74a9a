"""processMatches and the decoder with mismatchesWithExclusion = 0 — the protein profile's setting (MBGC_Params.h:924-936), under
which a mismatch inside an extension is written as the target's byte itself, not as its code among the symbols that exclude the
reference's (MBGC_Encoder.cpp:172-176,197-201,254-258,276-280). K = 16, sampling steps 16 and 7; targets over the 20 amino-acid
letters and over ACGTN against a reference of four such contigs loaded with their reverse complements. Every stream must equal
oracle/emit_oracle.c's byte for byte, the device verification must pass, and the device decoder must give the target back.

Planted beside the drawn substitutions: the target's first and last byte (an extension to the left, to the right, then ends on a
mismatch at the contig's edge: the last byte the extension writes), two substitutions next to each other and two one byte apart
(a mismatch as the first byte of an extension, and again right behind it)."""
import numpy as np
import pytest

import _orc

pytestmark = pytest.mark.gpu
NO_LOCK = _orc.NO_LOCK
L = 16
LIM = 2_000_000
ALPHABETS = {"amino": np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8), "acgtn": np.frombuffer(b"ACGNT", dtype=np.uint8)}      # (each sorted: substitute() looks letters up)
# (target length, substitution rate, which reference contig, where in it)
TARGETS = [(3_000, 0.01, 0, 0), (7_777, 0.03, 1, 1_234), (20_000, 0.05, 2, 0), (12_001, 0.02, 3, 5_000), (4_099, 0.05, 0, 15_901)]


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    return b


def substitute(rs, a, alphabet, at):
    """another letter of the alphabet at every index of `at`"""
    cur = np.searchsorted(alphabet, a[at])
    a[at] = alphabet[(cur + rs.randint(1, alphabet.size, size=len(at))) % alphabet.size]


def inputs(name, seed):
    alphabet = ALPHABETS[name]
    rs = np.random.RandomState(seed)
    ref = [alphabet[rs.randint(0, alphabet.size, size=20_000)] for _ in range(4)]
    targets = []
    for n, rate, c, s in TARGETS:
        t = ref[c][s:s + n].copy()
        assert t.size == n
        substitute(rs, t, alphabet, rs.permutation(n)[: int(n * rate)])
        planted = np.array([0, n - 1, n // 2, n // 2 + 1, n // 3, n // 3 + 2])
        t[planted] = ref[c][s:s + n][planted]
        substitute(rs, t, alphabet, planted)
        targets.append(t)
    return ref, targets


def compare(a, b):
    for k in b:
        assert a[k] == b[k], "%s differs (%d vs %d bytes)" % (k, len(a[k]), len(b[k]))


@pytest.mark.parametrize("name,k1,lazy", [(n, k1, 1) for n in sorted(ALPHABETS) for k1 in (16, 7)] + [("amino", 16, 0)])
def test_streams_equal_the_oracle_and_decode_back(binding, name, k1, lazy):
    import torch
    ref, targets = inputs(name, 900 + k1)
    over = dict(mismatchesWithExclusion=0, lazyDecompressionSupport=lazy)
    p, po = binding.emit_params(1, **over), _orc.emit_params(1, **over)
    assert p.mismatchesWithExclusion == 0 and po.mismatchesWithExclusion == 0
    h, o = binding.SlidingWindowSparseEMMatcher(LIM, L=L, k1=k1), _orc.OracleMatcher(LIM, L=L, k1=k1)
    for m in (h, o):
        for c in ref:
            m.load_ref(c, load_rc=True)
    loaded = [h.loaded_ref_length()]
    mismatch_literals = 0
    for t, c in enumerate(targets):
        m_h, m_o = h.match(c, L), o.match(c, L)
        assert np.array_equal(m_h, m_o) and len(m_o) > 0
        un, streams, _ = h.emit(p, 0, binding.NO_LOCK, 128, t, t, loaded)
        assert h.emit_verify() == (0, -1, 2 ** 64 - 1)
        oe = _orc.OracleEmitter(o, po)
        assert oe.process(m_o, c, NO_LOCK, 128, t, t, loaded) == un
        compare(streams, oe.streams())
        # with exclusion on, the same matches give other literal bytes: the flag is not a no-op on this input
        ox = _orc.OracleEmitter(o, _orc.emit_params(1, lazyDecompressionSupport=lazy))
        ox.process(m_o, c, NO_LOCK, 128, t, t, loaded)
        with_excl = ox.streams()
        assert len(with_excl["literals"]) == len(streams["literals"])
        mismatch_literals += sum(x != y for x, y in zip(with_excl["literals"], streams["literals"]))
        bufs = [torch.from_numpy(np.frombuffer(streams[k], dtype=np.uint8).copy()).to("cuda:0") if len(streams[k]) else
                torch.empty(1, dtype=torch.uint8, device="cuda:0") for k in binding.STREAM_NAMES]
        dest = torch.zeros(c.size + 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        job = ([(b.data_ptr(), len(streams[k])) for b, k in zip(bufs, binding.STREAM_NAMES)], binding.NO_LOCK, dest.data_ptr(), c.size)
        dl, un2 = h.decode_contigs_dev(p, [job])
        back, un3 = _orc.decode_contig(h.ref(h.max_ref_length()), po, streams, NO_LOCK, c.size + 16)
        assert int(dl[0]) == c.size and np.array_equal(dest.cpu().numpy()[:c.size], c) and np.array_equal(back, c)
        assert int(un2[0]) == un3 == (un & 0xFFFFFFFF)
        for m in (h, o):
            m.load_ref(c)
            m.load_separator(0)
        loaded.append(h.loaded_ref_length())
    assert mismatch_literals > 50, mismatch_literals
    assert np.array_equal(h.ht(), o.ht())
    h.close(); o.close()
