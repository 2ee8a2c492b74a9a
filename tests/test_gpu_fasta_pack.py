"""mbgc_fasta_pack_dev (k_fa_pack: what `mbgc-hip r` packs the chosen units with) through the ctypes mirror, on torch buffers, against
numpy's concatenation of the same slices, with and without the upper-case flag: every source alignment against piece lengths around
the 16-byte lane step and the 4096-byte tile, thousands of tiny pieces in a few tiles, one piece over hundreds of tiles, a piece
that ends with the source, empty tables, the two refusals and the capacity answer. The destination stands between canaries at every
alignment: no byte outside [0, total) may change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4097]
CANARY = 0xEE


def fold(x):
    low = (x >= ord("a")) & (x <= ord("z"))
    return np.where(low, x - 32, x).astype(np.uint8)


def source(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8), max(n, 1))[:n].copy()


def pack(src, pieces, uppercase=False, src_mod=0, dst_mod=0, cap=None, slack=48):
    """-> (dstOff, the destination's bytes [0, total), total). The source stands src_mod bytes behind a 16-byte boundary and is
    declared exactly as long as it is; the destination stands dst_mod behind one, with `slack` canary bytes in front and behind."""
    import torch
    from mbgc_amd import fasta
    total = sum(int(n) for _, n in pieces)
    cap = total if cap is None else cap
    sbuf = torch.zeros(src.size + 32, dtype=torch.uint8, device="cuda:0")
    s0 = (src_mod - sbuf.data_ptr()) % 16
    sbuf[s0: s0 + src.size] = torch.from_numpy(src).to("cuda:0")
    dbuf = torch.full((cap + 2 * slack + 32,), CANARY, dtype=torch.uint8, device="cuda:0")
    d0 = slack + (dst_mod - (dbuf.data_ptr() + slack)) % 16
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        offs, ms = p.pack_dev(sbuf.data_ptr() + s0, src.size, pieces, dbuf.data_ptr() + d0, cap, uppercase)
    except Exception:
        assert (dbuf.cpu().numpy() == CANARY).all(), "a refused call wrote to the destination"
        raise
    finally:
        p.close()
    host = dbuf.cpu().numpy()
    n = int(offs[-1])
    assert (host[:d0] == CANARY).all() and (host[d0 + n:] == CANARY).all(), "bytes outside the result were written"
    return offs, host[d0: d0 + n].copy(), n


def check(src, pieces, **kw):
    want = np.concatenate([src[o: o + n] for o, n in pieces] + [np.zeros(0, dtype=np.uint8)])
    want_off = np.concatenate([[0], np.cumsum([n for _, n in pieces])]).astype(np.uint64)
    for up in (False, True):
        offs, got, total = pack(src, pieces, uppercase=up, **kw)
        assert offs.tolist() == want_off.tolist()
        assert total == want.size and np.array_equal(got, fold(want) if up else want), (up, kw, pieces[:8])


@pytest.mark.parametrize("src_mod", range(16))
def test_every_source_alignment_against_the_step_lengths(src_mod):
    """all the lengths in one call, twice over in another order: the destination's alignment of a piece follows from the running sum,
    the source's from src_mod and the gaps; the last piece ends with the source"""
    lens = LENGTHS + LENGTHS[::-1][1:] + [17, 1, 4097]
    pieces, at = [], 0
    for i, n in enumerate(lens):
        at += (3 * i) % 7                                                            # bytes no piece holds
        pieces.append((at, n))
        at += n
    src = source(at, 100 + src_mod)
    assert pieces[-1][0] + pieces[-1][1] == src.size
    check(src, pieces, src_mod=src_mod, dst_mod=(5 * src_mod + 3) % 16)


def test_many_tiny_pieces_share_a_tile():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 41, 5000)
    pieces, at = [], 0
    for n in lens:
        at += int(rng.integers(0, 9))
        pieces.append((at, int(n)))
        at += int(n)
    check(source(at, 6), pieces, src_mod=3, dst_mod=9)


def test_one_piece_spans_many_tiles():
    src = source(3_200_000, 7)
    pieces = [(5, 30), (100, 0), (40_001, 3_000_017), (3_100_000, 77), (12, 4)]      # (the pieces need not ascend in the source)
    check(src, pieces, src_mod=11, dst_mod=2)


def test_empty_tables():
    src = source(100, 8)
    for pieces in ([], [(0, 0), (100, 0), (50, 0)]):
        for up in (False, True):
            offs, got, total = pack(src, pieces, uppercase=up)
            assert total == 0 and offs.tolist() == [0] * (len(pieces) + 1)


def test_too_small_a_destination_is_left_untouched():
    from mbgc_amd import fasta
    src = source(5000, 9)
    with pytest.raises(fasta.PackTooSmall) as e:
        pack(src, [(0, 3000), (100, 1500)], cap=4499)                                # (pack() checks that every byte is still the canary)
    assert e.value.needed == 4500


def test_refusals_launch_nothing():
    import torch
    from mbgc_amd import binding, fasta
    src = source(1000, 10)
    for pieces in ([(0, 10), (990, 11)], [(1001, 0)], [(2 ** 63, 2 ** 63)]):
        with pytest.raises(binding.SwsemError, match="outside the source"):
            pack(src, pieces, cap=64)
    buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        for s, n, d, cap in ((0, 1000, 999, 100), (500, 1000, 0, 501), (0, 2000, 100, 50)):
            with pytest.raises(binding.SwsemError, match="overlap"):
                p.pack_dev(buf.data_ptr() + s, n, [(0, 10)], buf.data_ptr() + d, cap)
        offs, _ = p.pack_dev(buf.data_ptr(), 1000, [(0, 10)], buf.data_ptr() + 1000, 10)         # neighbours do not overlap
        assert offs.tolist() == [0, 10]
    finally:
        p.close()
    assert (buf.cpu().numpy() == CANARY).all()


def test_flag_folds_every_byte_as_the_parser_does():
    from mbgc_amd import fasta
    values = np.array([v for v in range(256) if v != 10], dtype=np.uint8)            # (a line feed never reaches the parser's fold)
    p = fasta.FastaParser()
    try:
        parsed = p.parse_host(b">h\nA" + values.tobytes() + b"\n", uppercase=True)
    finally:
        p.close()
    assert parsed["status"] == 0 and len(parsed["records"]) == 1
    folded = np.frombuffer(parsed["records"][0][1], dtype=np.uint8)[1:]
    assert folded.size == values.size
    src = np.arange(256, dtype=np.uint8)
    for src_mod in (0, 5):                                                           # (the vector path and, with 7-byte pieces, the byte path)
        for pieces in ([(0, 256)], [(o, min(7, 256 - o)) for o in range(0, 256, 7)]):
            _, got, total = pack(src, pieces, uppercase=True, src_mod=src_mod)
            assert total == 256 and got[10] == 10
            assert np.array_equal(np.delete(got, 10), folded)
            _, plain, _ = pack(src, pieces, uppercase=False, src_mod=src_mod)
            assert np.array_equal(plain, src)
