"""The granule closure of `d --region` swept where its arithmetic has edges (k_decode_closure_region, closure_mark_region and
rec_needed in swsem_decode.hip; Provenance::closureRegion on the host), through mbgc_decoder_region_probe. An off-by-one in a
byte range changes the granule set only when a range end falls on a granule's edge, so the sweep goes down to the 16-byte
granule, on sets whose last records read forward and reversed rows, rows of owners shorter than a granule, and a buffer that
has lapped (_regionprobe.py). The device and the host share their reasoning; the evidence that does not is the masked fill: an
under-marked granule leaves the 0xEE sentinel where a later record copies from, and `check` asks for the right byte there.

Pieces come from a seeded generator that reads the plan's own record offsets: around a record's destAt, at the contig's two ends,
around and exactly on a granule. They go in ONE PER CALL — a second piece's closure would write the bytes an under-marked first
one lacks. Then three properties that hold by the closure's definition and need no referee: it distributes over the union of two
need states, it nests when the granule grows fourfold, and its own result fed back as the request changes nothing."""
import numpy as np
import pytest

import _meta
import _regionprobe as rp

pytestmark = pytest.mark.gpu
GRANULES = (16, 64, 256, 4096)
LADDER = (16, 64, 256, 1024, 4096)
CLASSES = ("destAt-straddled", "destAt", "destAt-1", "contig-first", "contig-last", "granule-straddled", "granule-exact", "granule-and-one-each-side")
SETS = list(rp.VARIANTS)


@pytest.fixture(scope="module")
def host():
    return rp.host_lib()


class Swept:
    """a set, its plan's geometry from a first call, the contigs the pieces go to, and every closure asked for so far"""

    def __init__(self, host, s, name):
        self.host, self.s, self.name, self.memo, self.calls = host, s, name, {}, 0
        p = s.probe(host, [(0, 0, 1)], 256, "geometry")
        self.lens = p["contigLen"].astype(np.int64)
        self.g0n = self.lens.size - (p["granBase"].size - 1)
        self.rec_base, self.rec_dest = p["recBase"].astype(np.int64), p["recDest"].astype(np.int64)
        n = self.lens.size
        if name == "many-records":                                 # the b records; a piece in a short a record comes from the named cases below
            self.targets = list(range(n - rp.MANY, n))
        elif name == "wrap":                                       # the copies: contig 2 + i, i % 3 == 2
            self.targets = [2 + i for i in range(80) if i % 3 == 2]
        else:
            self.targets = [n - 1]

    def dests(self, c):
        k = c - self.g0n
        return self.rec_dest[self.rec_base[k]:self.rec_base[k + 1]]

    def closure(self, pieces, granule):
        """probe + check, once per (pieces, granule): (granule bits, contig bits, filled), device == host held by check"""
        key = (tuple(sorted(pieces)), granule)
        if key not in self.memo:
            p = self.s.probe(self.host, list(key[0]), granule)
            need, contig, filled = rp.check(p, self.s.full.seq, list(key[0]), granule)
            self.memo[key] = (need, contig, filled, p["granBase"].astype(np.int64))
            self.calls += 1
        return self.memo[key]

    def edge_pieces(self, granule, count, seed):
        """count distinct pieces, class after class in turn: [(class, (contig, from0, len))], clipped to the contig. A class that has
        no further piece to give (one contig has one first byte) passes its turn"""
        rng = np.random.default_rng(seed)
        out, seen, turn = [], set(), 0
        while len(out) < count:
            assert turn < 8 * count, "the set has no %d distinct pieces at G = %d" % (count, granule)
            cls = CLASSES[turn % len(CLASSES)]
            turn += 1
            for _ in range(40):
                c = int(self.targets[rng.integers(len(self.targets))])
                n = int(self.lens[c])
                d = self.dests(c)
                at = int(d[rng.integers(1, d.size)]) if d.size > 1 else 0          # a record's destAt, not the contig's first byte
                g = int(rng.integers(1, max(2, (n - 1) // granule))) * granule     # a granule's first byte
                a, b = {"destAt-straddled": (at - 1, at + 1), "destAt": (at, at + 1), "destAt-1": (at - 1, at), "contig-first": (0, 1), "contig-last": (n - 1, n),
                        "granule-straddled": (g - 1, g + 1), "granule-exact": (g, g + granule), "granule-and-one-each-side": (g - 1, g + granule + 1)}[cls]
                a, b = max(a, 0), min(b, n)
                if a < b and (c, a, b - a) not in seen:
                    seen.add((c, a, b - a))
                    out.append((cls, (c, a, b - a)))
                    break
        return out


_SWEPT = {}


@pytest.fixture(scope="module")
def swept(host, tmp_path_factory):
    def get(name):
        if name not in _SWEPT:
            _SWEPT[name] = Swept(host, rp.stream_set(tmp_path_factory, name), name)
        return _SWEPT[name]
    return get


def counts(name, granule):
    """single-piece calls per set and granule: 24 at 16 B and 8 elsewhere"""
    return 24 if granule == 16 else 8


@pytest.mark.parametrize("granule", GRANULES)
@pytest.mark.parametrize("name", SETS)
def test_one_piece_per_call_at_the_edges(swept, name, granule):
    """(a probe call re-reads, uploads and re-plans the set: the time of one is printed)"""
    import time
    w = swept(name)
    pieces = w.edge_pieces(granule, counts(name, granule), 100 * GRANULES.index(granule) + SETS.index(name))
    assert {cls for cls, _ in pieces} == set(CLASSES)
    t0, before = time.perf_counter(), w.calls
    for cls, piece in pieces:
        try:
            need, contig, filled, _ = w.closure([piece], granule)
        except AssertionError as e:
            raise AssertionError("%s, G = %d, %s %r: %s" % (name, granule, cls, piece, e)) from e
        assert filled >= piece[2]
    print("%s, G = %d: %d calls, %.0f ms each" % (name, granule, w.calls - before, 1e3 * (time.perf_counter() - t0) / max(1, w.calls - before)))


def test_the_wrap_set_has_lapped(swept):
    w = swept("wrap")
    assert _meta.parse(open("%s/%s.meta" % (w.s.tmp, w.s.prefix), "rb").read())["laps"] >= 2


def test_every_copy_of_the_wrap_set_whole(swept):
    """each copy in a call of its own, all of it asked for: what it reads lies two files back, which for the copies just behind a
    wrap is the lap before — the rows the split at the loader's position sends to lap - 1"""
    w = swept("wrap")
    for c in w.targets:
        need, contig, filled, _ = w.closure([(c, 0, int(w.lens[c]))], 256)
        assert contig[c - w.g0n] and filled >= int(w.lens[c]), c


@pytest.mark.parametrize("name", [n for n in SETS if n.startswith("rc-chain")])
def test_the_rc_chain_is_followed_through_its_links(swept, name):
    """a request in the last link marks at least 3 earlier links: the chain's rows, forward and reversed in turn, are what the
    sweep above walks (16 KiB of link 6 at G = 16 marks 3 earlier links of the plain set, 5 of -i; _regionprobe.write_rc_chain)"""
    w = swept(name)
    last = w.lens.size - 1
    need, contig, filled, _ = w.closure([(last, 16_384, 16_384)], 16)
    print("%s: contigs marked %s, %d bases filled" % (name, np.flatnonzero(contig).tolist(), filled))
    assert contig[-1] and int(contig[:-1].sum()) >= 3


def test_short_records_of_the_many_records_set(swept):
    """pieces inside records of 15, 16, 17, 255, 256 and 257 bases (one granule short of, exactly and one over G = 16 and 256), and
    b records whose closure reaches such records"""
    w = swept("many-records")
    lens = rp.many_lengths()
    first_a = w.lens.size - 2 * rp.MANY
    for want in rp.MANY_SHORT:
        i = lens.index(want)
        for granule in (16, 256):
            for a, n in ((0, want), (want - 1, 1)):
                w.closure([(first_a + i, a, n)], granule)
    reached = np.zeros(rp.MANY, dtype=bool)
    for c in w.targets[::25]:
        need, contig, _, _ = w.closure([(c, 0, int(w.lens[c]))], 16)
        reached |= contig[first_a - w.g0n:first_a - w.g0n + rp.MANY]
    assert {lens[i] for i in np.flatnonzero(reached)} & set(rp.MANY_SHORT[3:])       # owners of about a granule are among what is read


def pairs(w, granule, seed):
    """two pairs of pieces in different contigs, two in one contig. Where the pieces all go to the last contig, the other contig is
    the one two in front of it, itself read by what lies between"""
    e = [p for _, p in w.edge_pieces(granule, 16, seed)]
    if len(w.targets) > 1:
        other = lambda a: next(p for p in e[4:] if p[0] != a[0])
    else:
        other = lambda a: (a[0] - 2,) + e[5][1:]
    return [(e[0], other(e[0])), (e[1], other(e[1])), (e[2], (e[2][0], min(e[2][1] + 3 * granule, int(w.lens[e[2][0]]) - 1), 1)), (e[3], (e[3][0], int(w.lens[e[3][0]]) // 2, granule + 1))]


@pytest.mark.parametrize("granule", [16, 256])
@pytest.mark.parametrize("name", SETS)
def test_union(swept, name, granule):
    """closure(A u B) has exactly the bits of closure(A) | closure(B)"""
    w = swept(name)
    for a, b in pairs(w, granule, 7 + SETS.index(name)):
        na, ca, fa, _ = w.closure([a], granule)
        nb, cb, fb, _ = w.closure([b], granule)
        nu, cu, fu, _ = w.closure([a, b], granule)
        assert np.array_equal(nu, na | nb) and np.array_equal(cu, ca | cb), (name, granule, a, b)
        assert max(fa, fb) <= fu <= fa + fb


def byte_masks(w, need, base, granule):
    return [np.repeat(need[base[k]:base[k + 1]], granule)[:int(w.lens[w.g0n + k])] for k in range(w.lens.size - w.g0n)]


@pytest.mark.parametrize("name", SETS)
def test_refinement(swept, name):
    """the bytes needed at G lie among the bytes needed at 4G, 16 through 4096; the contig bits nest and filled does not decrease"""
    w = swept(name)
    e = [p for _, p in w.edge_pieces(16, 8, 31 + SETS.index(name))]
    for pieces in ([e[0]], [e[5], e[7]]):
        prev = None
        for granule in LADDER:
            need, contig, filled, base = w.closure(pieces, granule)
            cur = (byte_masks(w, need, base, granule), contig, filled)
            if prev is not None:
                assert all(not (f & ~c).any() for f, c in zip(prev[0], cur[0])), (name, granule, pieces)
                assert not (prev[1] & ~cur[1]).any() and prev[2] <= cur[2], (name, granule, pieces)
            prev = cur


@pytest.mark.parametrize("granule", [16, 256])
@pytest.mark.parametrize("name", SETS)
def test_idempotence(swept, name, granule):
    """every needed granule fed back as a piece, clipped to its contig (neighbouring granules as one piece: the same need state
    goes in): the same two bitmaps and the same filled"""
    w = swept(name)
    first = [p for _, p in w.edge_pieces(granule, 8, 53 + SETS.index(name))][4:7]
    need, contig, filled, base = w.closure(first, granule)
    back = []
    for k in range(w.lens.size - w.g0n):
        g = np.flatnonzero(need[base[k]:base[k + 1]])
        if g.size:
            runs = np.split(g, np.flatnonzero(np.diff(g) > 1) + 1)
            back += [(w.g0n + k, int(r[0]) * granule, min(int(r[-1] + 1) * granule, int(w.lens[w.g0n + k])) - int(r[0]) * granule) for r in runs]
    assert {c for c, _, _ in back} == set((w.g0n + np.flatnonzero(contig)).tolist())
    need2, contig2, filled2, _ = w.closure(back, granule)
    assert np.array_equal(need, need2) and np.array_equal(contig, contig2) and filled == filled2
