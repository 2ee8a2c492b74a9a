"""`mbgc-hip d --region` on the host, no device: the spec parser, the pieces (clamp, skip, dedup, order), the synthesized headers, and
the host restatement of the granule closure (Provenance::closureRegion through mbgc_decoder_region_closure) — a superset of a
byte-exact dependency walk this test makes itself over small hand-built plans, and the contig closure when a granule holds a
whole contig."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype([("litFrom", "<u8"), ("mark", "<u8"), ("destAt", "<u8"), ("src", "<u8"), ("leftSrcMatch", "<i8"), ("leftSrcGuard", "<i8"), ("flLeft", "<u8"),
                ("flRight", "<u8"), ("offsetDelta", "<i8"), ("guardLit", "<u8"), ("len", "<u4"), ("leftLen", "<u4"), ("leftCodes", "<u4"), ("rightLen", "<u4"),
                ("flags", "<u4"), ("pad", "<u4")])
TAIL = 16


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    P, P32, I = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    L.mbgc_region_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, P, P, C.c_char_p, C.c_uint64]
    L.mbgc_region_header.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64]
    L.mbgc_region_resolve.argtypes = [P, C.c_uint64, P, C.c_uint64, P, C.c_uint64, P, P]
    L.mbgc_decoder_region_closure.argtypes = [I, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, P, P, C.c_void_p, P, P, C.c_uint64, C.c_uint32, P, P32, P32, P, I, C.c_uint64, P]
    return L


def parse(host, text):
    pat, err = C.create_string_buffer(256), C.create_string_buffer(256)
    a, b = C.c_uint64(), C.c_uint64()
    r = host.mbgc_region_parse(text.encode(), pat, 256, C.byref(a), C.byref(b), err, 256)
    return (pat.value.decode(), a.value, b.value) if r == 0 else err.value.decode()


def test_spec_is_split_at_its_last_colon(host):
    assert parse(host, "NZ_CP0123:120000-126000") == ("NZ_CP0123", 120000, 126000)
    assert parse(host, "a:b c:1-1") == ("a:b c", 1, 1)
    assert parse(host, "x:7-7") == ("x", 7, 7)
    assert parse(host, "chr1 :5-9") == ("chr1 ", 5, 9)


@pytest.mark.parametrize("text,word", [("abc", "no ':'"), (":1-2", "empty pattern"), ("a:", "no '-'"), ("a:12", "no '-'"), ("a:-5", "decimal"), ("a:5-", "decimal"),
                                       ("a:1e3-2000", "decimal"), ("a:+1-2", "decimal"), ("a: 1-2", "decimal"), ("a:0-5", "1-based"), ("a:9-8", "behind TO"),
                                       ("a:1-2-3", "decimal"), ("a:1-99999999999999999999", "decimal"), ("a:b:c", "no '-'")])
def test_bad_specs_are_refused_with_a_reason(host, text, word):
    got = parse(host, text)
    assert isinstance(got, str) and word in got, got


def test_header_synthesis(host):
    def hdr(h, a, b):
        out = C.create_string_buffer(512)
        assert host.mbgc_region_header(h.encode(), a, b, out, 512) == 0
        return out.value.decode()
    assert hdr("NZ_CP0123.1 Listeria monocytogenes", 5, 80) == "NZ_CP0123.1:5-80 Listeria monocytogenes"
    assert hdr("lonely", 1, 1) == "lonely:1-1"
    assert hdr("tab\tseparated words", 2, 3) == "tab:2-3\tseparated words"
    assert hdr("trio:b second:of three", 8000, 9017) == "trio:b:8000-9017 second:of three"


def resolve(host, asks, lens):
    a = np.ascontiguousarray(np.asarray(asks, dtype=np.uint64).reshape(-1, 3))
    ln = np.asarray(lens, dtype=np.uint64)
    out = np.zeros((len(a) + 1, 3), dtype=np.uint64)
    n, sk = C.c_uint64(), C.c_uint64()
    P = C.POINTER(C.c_uint64)
    assert host.mbgc_region_resolve(a.ctypes.data_as(P), len(a), ln.ctypes.data_as(P), len(ln), out.ctypes.data_as(P), len(out), C.byref(n), C.byref(sk)) == 0
    return out[:n.value].tolist(), sk.value


def test_pieces_are_clamped_skipped_deduplicated_and_ordered(host):
    lens = [100, 50, 10]
    asks = [(1, 40, 60), (0, 90, 200), (0, 10, 20), (2, 11, 12), (0, 10, 20), (0, 10, 15), (1, 40, 50), (2, 10, 10), (1, 51, 51), (0, 1, 1)]
    pieces, skipped = resolve(host, asks, lens)
    # by record, then FROM, then TO; to clamped (1: 40-60 and 40-50 are the same piece then); FROM behind the end: skipped, counted
    assert pieces == [[0, 0, 1], [0, 9, 6], [0, 9, 11], [0, 89, 11], [1, 39, 11], [2, 9, 1]]
    assert skipped == 2


# ---- the granule closure against a byte-exact walk
class Plan:
    """G0 (contig 0, nobody's) and planned contigs made of literal runs and matches into what was loaded before them; every planned
    contig is loaded forward and then reverse-complemented, the loader wraps at `total`"""

    def __init__(self, total, g0, lens, seed):
        rng = np.random.default_rng(seed)
        self.total, self.segs, self.pos = total, [], 1
        self.load(0, g0, 0)
        self.recs, self.time_seg, self.lens = [], [], lens
        self.src_of = []                                           # per planned contig: per byte the reference position it is copied from, -1: a literal
        self.loaded = g0
        for c, n in enumerate(lens):
            self.time_seg.append(len(self.segs))
            rows, src_of, at, lit = [], np.full(n, -1, dtype=np.int64), 0, 0
            while at < n:
                plain = int(rng.integers(0, 12))
                ln = int(rng.integers(8, 60))
                if at + plain + ln > n:
                    break
                span = min(self.loaded, total - 1)
                src = int(rng.integers(1, max(2, span - ln)))
                r = np.zeros((), dtype=REC)
                r["litFrom"], r["mark"], r["destAt"], r["src"], r["len"] = lit, lit + plain, at, src, ln
                rows.append(r)
                src_of[at + plain:at + plain + ln] = np.arange(src, src + ln)
                lit += plain + 1
                at += plain + ln
            t = np.zeros((), dtype=REC)
            t["litFrom"], t["mark"], t["destAt"], t["flags"] = lit, lit + (n - at), at, TAIL
            rows.append(t)
            self.recs.append(np.array(rows, dtype=REC))
            self.src_of.append(src_of)
            self.load(c + 1, n, 0)
            self.load(c + 1, n, 1)
            self.loaded += 2 * n

    def load(self, contig, length, rc):
        left, done = length, 0
        while left:
            if self.pos == self.total:
                self.pos = 1
            n = min(left, self.total - self.pos)
            # (MBGC_Decoder::loadRef: a reverse complement is written from the text's end, a copy from its head)
            self.segs.append([contig, length - done - n if rc else done, n, self.pos, rc])
            self.pos += n
            done += n
            left -= n

    def owner_maps(self):
        """per planned contig: (owner, owner position) of every physical byte at the contig's time, replayed byte by byte"""
        own = np.full((self.total, 2), -1, dtype=np.int64)
        out, t = [], 0
        for c in range(len(self.lens)):
            while t < self.time_seg[c]:
                contig, off, n, pos, rc = self.segs[t]
                idx = off + (np.arange(n)[::-1] if rc else np.arange(n))
                own[pos:pos + n, 0] = contig - 1 if contig >= 1 else -1
                own[pos:pos + n, 1] = idx
                t += 1
            out.append(own.copy())
        return out

    def closure(self, host, shift, chosen):
        """chosen: [(planned contig, from0, len)] -> (granBase, granule bits, contig bits, filled)"""
        n = len(self.lens)
        segs = np.ascontiguousarray(np.asarray(self.segs, dtype=np.int64))
        lens = np.asarray(self.lens, dtype=np.uint64)
        ts = np.asarray(self.time_seg, dtype=np.uint64)
        recs = np.concatenate(self.recs)
        base = np.concatenate([[0], np.cumsum([len(r) for r in self.recs])]).astype(np.uint64)
        units = np.asarray([[c, c + 1] for c in range(n)], dtype=np.uint64)
        gb = np.zeros(n + 1, dtype=np.uint64)
        G = 1 << shift
        pre = np.concatenate([[0], np.cumsum([(x + G - 1) // G for x in self.lens])])
        need = np.zeros(int(pre[-1]) // 32 + 2, dtype=np.uint32)
        cont = np.zeros(n // 32 + 1, dtype=np.uint32)
        for c, a, ln in chosen:
            cont[c >> 5] |= np.uint32(1 << (c & 31))
            for g in range(int(pre[c]) + a // G, int(pre[c]) + (a + ln - 1) // G + 1):
                need[g >> 5] |= np.uint32(1 << (g & 31))
        filled, nrows = C.c_uint64(), C.c_uint64()
        P, P32, I = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
        r = host.mbgc_decoder_region_closure(segs.ctypes.data_as(I), len(segs), self.total, 1, n, lens.ctypes.data_as(P), ts.ctypes.data_as(P), recs.ctypes.data, base.ctypes.data_as(P),
                                             units.ctypes.data_as(P), n, shift, gb.ctypes.data_as(P), need.ctypes.data_as(P32), cont.ctypes.data_as(P32), C.byref(filled),
                                             None, 0, C.byref(nrows))
        assert r == 0 and gb.tolist() == pre.tolist()
        unpack = lambda w, k: np.unpackbits(w.view(np.uint8), bitorder="little")[:k].astype(bool)
        return pre, unpack(need, int(pre[-1])), unpack(cont, n), filled.value

    def exact_walk(self, chosen):
        """the bytes that must be right for the chosen bytes to be right, with the rule that a record runs whole: a needed byte needs
        its record, the record needs every byte its match copies, traced to (owner, position) byte by byte"""
        maps = self.owner_maps()
        needed = [np.zeros(n, dtype=bool) for n in self.lens]         # the bytes the records that run write
        read = [np.zeros(n, dtype=bool) for n in self.lens]           # the bytes that are asked for: chosen, or read by a record that runs
        todo = [(c, a, a + ln) for c, a, ln in chosen]
        while todo:
            c, a, b = todo.pop()
            read[c][a:b] = True
            dest = np.append(self.recs[c]["destAt"], self.lens[c]).astype(np.int64)
            for i in range(len(dest) - 1):
                lo, hi = int(dest[i]), int(dest[i + 1])
                if hi <= a or lo >= b or hi == lo or needed[c][lo:hi].all():
                    continue
                needed[c][lo:hi] = True
                for s in self.src_of[c][lo:hi]:
                    if s >= 0 and maps[c][s, 0] >= 0:
                        o, p = int(maps[c][s, 0]), int(maps[c][s, 1])
                        if not needed[o][p]:
                            todo.append((o, p, p + 1))
                        read[o][p] = True
        return read, needed


@pytest.mark.parametrize("total,seed", [(1 << 20, 1), (1500, 2), (1100, 3)], ids=["no-wrap", "wraps", "wraps-twice"])
@pytest.mark.parametrize("shift", [4, 6])
def test_granule_closure_is_a_superset_of_the_exact_walk(host, total, seed, shift):
    plan = Plan(total, 200, [300, 257, 311, 290, 333, 280], seed)
    chosen = [(5, 100, 40), (4, 0, 1), (5, 279, 1)]
    pre, need, cont, filled = plan.closure(host, shift, chosen)
    exact, written = plan.exact_walk(chosen)
    G = 1 << shift
    deps = 0
    for c, bytes_read in enumerate(exact):
        gran = need[int(pre[c]):int(pre[c + 1])]
        at = np.flatnonzero(bytes_read)
        assert gran[at // G].all(), c                              # never less than what is read
        assert cont[c] or not at.size, c
        deps += c < 4 and at.size > 0
    assert deps >= 2                                               # (the plan has dependencies to follow at all)
    assert filled >= sum(int(x.sum()) for x in written)
    assert not need.all()                                          # ... and the closure is no "everything"


@pytest.mark.parametrize("total,seed", [(1 << 20, 4), (1500, 5)], ids=["no-wrap", "wraps"])
def test_whole_records_with_a_granule_per_contig_give_the_contig_closure(host, total, seed):
    """a granule that holds a whole contig: a needed contig is needed whole, which is the contig closure — here made from the exact
    walk with every byte of a needed contig needed"""
    plan = Plan(total, 200, [300, 257, 311, 290, 333, 280], seed)
    chosen = [(5, 0, 280), (3, 0, 290)]
    pre, need, cont, filled = plan.closure(host, 10, chosen)
    maps = plan.owner_maps()
    want = np.zeros(6, dtype=bool)
    todo = [5, 3]
    while todo:
        c = todo.pop()
        if want[c]:
            continue
        want[c] = True
        for r in plan.recs[c]:
            if not (r["flags"] & TAIL):
                todo += [int(o) for o in set(maps[c][int(r["src"]):int(r["src"]) + int(r["len"]), 0].tolist()) if o >= 0]
    assert cont.tolist() == want.tolist() and need.tolist() == want.tolist()
    assert filled == sum(n for n, w in zip(plan.lens, want) if w)
    # at a finer grain the same selection never needs a contig the contig closure does not
    _, _, fine, fine_filled = plan.closure(host, 4, chosen)
    assert not (fine & ~want).any() and fine_filled <= filled


# ---- seeded random plans where the closure's arithmetic has edges, against a closure that works byte by byte
class EdgePlan(Plan):
    """Plan with what it lacks: contigs loaded forward only, reverse-complemented only, or both; owners shorter than a granule among
    the contigs; and, once the loader has lapped, matches placed across the loader's position and across the buffer's end's
    neighbour rows on purpose — the rest at random places, as Plan has them"""

    def __init__(self, total, g0, lens, seed):
        rng = np.random.default_rng(seed)
        self.total, self.segs, self.pos = total, [], 1
        self.load(0, g0, 0)
        self.recs, self.time_seg, self.lens, self.src_of = [], [], lens, []
        self.loaded, self.straddles, self.how = g0, 0, []
        for c, n in enumerate(lens):
            self.time_seg.append(len(self.segs))
            rows, src_of, at, lit = [], np.full(n, -1, dtype=np.int64), 0, 0
            lapped = self.loaded >= total - 1
            while at < n:
                plain = int(rng.integers(0, 12))
                ln = int(rng.integers(8, 60))
                if at + plain + ln > n:
                    break
                span = min(self.loaded, total - 1)
                kind = int(rng.integers(0, 4))
                if lapped and kind == 0 and ln < self.pos < total - ln:          # across the loader's position: this lap below it, the lap before from it on
                    src = self.pos - int(rng.integers(1, ln))
                    self.straddles += 1
                elif lapped and kind == 1:                                       # up to the buffer's last byte
                    src = total - ln
                elif kind == 2 and self.segs:                                    # from the first byte of a load on, or up to its last
                    _, _, sn, sp, _ = self.segs[int(rng.integers(len(self.segs)))]
                    src = sp if rng.integers(2) or sp + sn < ln + 1 else sp + sn - ln
                    src = min(max(src, 1), max(1, span - ln))
                else:
                    src = int(rng.integers(1, max(2, span - ln)))
                r = np.zeros((), dtype=REC)
                r["litFrom"], r["mark"], r["destAt"], r["src"], r["len"] = lit, lit + plain, at, src, ln
                rows.append(r)
                src_of[at + plain:at + plain + ln] = np.arange(src, src + ln)
                lit += plain + 1
                at += plain + ln
            t = np.zeros((), dtype=REC)
            t["litFrom"], t["mark"], t["destAt"], t["flags"] = lit, lit + (n - at), at, TAIL
            rows.append(t)
            self.recs.append(np.array(rows, dtype=REC))
            self.src_of.append(src_of)
            how = int(rng.integers(0, 3))                                        # 0: forward, 1: reverse complement, 2: both
            self.how.append(how)
            if how != 1:
                self.load(c + 1, n, 0)
            if how != 0:
                self.load(c + 1, n, 1)
            self.loaded += n * (2 if how == 2 else 1)

    def byte_closure(self, chosen, granule=1):
        """a set of needed bytes per contig: a needed byte makes its granule's bytes needed (granule = 1: itself only); a record
        runs when its destination range holds a needed byte, and every byte it copies from is needed of its owner. -> (needed, filled)"""
        maps = self.owner_maps()
        needed = [set() for _ in self.lens]
        ran = [set() for _ in self.lens]
        todo = []

        def want(c, p):
            for q in range(p // granule * granule, min((p // granule + 1) * granule, self.lens[c])):
                if q not in needed[c]:
                    needed[c].add(q)
                    todo.append((c, q))
        for c, a, ln in chosen:
            for p in range(a, a + ln):
                want(c, p)
        while todo:
            c, p = todo.pop()
            dest = self.recs[c]["destAt"].tolist() + [self.lens[c]]
            i = max(k for k in range(len(dest) - 1) if dest[k] <= p and dest[k] < dest[k + 1])
            if i in ran[c]:
                continue
            ran[c].add(i)
            for s in self.src_of[c][dest[i]:dest[i + 1]]:
                if s >= 0 and maps[c][s, 0] >= 0:
                    want(int(maps[c][s, 0]), int(maps[c][s, 1]))
        filled = 0
        for c in range(len(self.lens)):
            dest = self.recs[c]["destAt"].tolist() + [self.lens[c]]
            filled += sum(dest[i + 1] - dest[i] for i in ran[c])
        return needed, filled


EDGE_LENS = [300, 15, 257, 16, 311, 17, 290, 7, 333, 256, 255, 280, 64, 301, 1, 320]
EDGE_PLANS = [(1 << 20, 11), (1500, 12), (1100, 13), (1100, 14), (901, 15), (1500, 16)]


@pytest.fixture(scope="module")
def edge_plans():
    return {(total, seed): EdgePlan(total, 200, EDGE_LENS, seed) for total, seed in EDGE_PLANS}


def edge_chosen(plan, seed):
    """single pieces at a record's destAt, a byte before it, a contig's ends and a granule's edge, in the later contigs"""
    rng = np.random.default_rng(seed)
    out = []
    for c in (15, 13, 11, 8, 6, 12):
        n, d = plan.lens[c], plan.recs[c]["destAt"]
        at = int(d[rng.integers(1, len(d))]) if len(d) > 1 else 0
        out += [(c, max(at - 1, 0), min(2, n)), (c, at if at < n else n - 1, 1), (c, n - 1, 1), (c, 0, 1), (c, min(16 * int(rng.integers(0, 1 + n // 16)), n - 1), 1)]
    return out


def test_the_edge_plans_hold_what_they_are_for(edge_plans):
    lapped = [p for (total, _), p in edge_plans.items() if total < 2000]
    assert all(p.straddles >= 3 for p in lapped)                                  # read ranges across the loader's position on lap >= 1
    for p in edge_plans.values():
        assert {0, 1, 2} <= set(p.how)                                            # forward, reversed and both
        assert any(rc for _, _, _, _, rc in p.segs)
    for p in lapped:
        ends = [s for s in p.segs if s[3] + s[2] == p.total]
        assert len(ends) >= 2 and any(s[1] > 0 or s[2] < p.lens[s[0] - 1] for s in ends if s[0])   # loads split at the buffer's end


@pytest.mark.parametrize("shift", [4, 8])
@pytest.mark.parametrize("total,seed", EDGE_PLANS)
def test_granule_closure_against_the_byte_closure(host, edge_plans, total, seed, shift):
    """one piece per call: closureRegion covers the byte-exact closure coarsened to granules (never less than what is read), and is
    the byte closure in which a needed byte makes its granule needed — bit for bit, with the same filled"""
    plan = edge_plans[(total, seed)]
    G = 1 << shift
    followed = 0
    for piece in edge_chosen(plan, seed):
        pre, need, cont, filled = plan.closure(host, shift, [piece])
        exact, exact_filled = plan.byte_closure([piece])
        coarse, coarse_filled = plan.byte_closure([piece], G)
        for c in range(len(plan.lens)):
            gran = need[int(pre[c]):int(pre[c + 1])]
            assert all(gran[p // G] for p in exact[c]), (piece, c)
            assert sorted({p // G for p in coarse[c]}) == np.flatnonzero(gran).tolist(), (piece, c)
            assert bool(cont[c]) == bool(coarse[c]), (piece, c)
        assert exact_filled <= coarse_filled == filled, piece
        followed += sum(1 for c in range(piece[0]) if exact[c])
    assert followed >= 6                                                          # (the pieces have dependencies to follow)


def edge_closure_bytes(plan, host, shift, chosen):
    pre, need, cont, filled = plan.closure(host, shift, chosen)
    masks = [np.repeat(need[int(pre[c]):int(pre[c + 1])], 1 << shift)[:n] for c, n in enumerate(plan.lens)]
    return pre, need, cont, filled, masks


@pytest.mark.parametrize("total,seed", EDGE_PLANS)
def test_referee_union_refinement_idempotence(host, edge_plans, total, seed):
    plan = edge_plans[(total, seed)]
    e = edge_chosen(plan, seed)
    for shift in (4, 8):
        for a, b in ((e[0], e[6]), (e[1], e[3]), (e[10], e[21])):                  # different contigs, one contig, different contigs
            _, na, ca, fa = plan.closure(host, shift, [a])
            _, nb, cb, fb = plan.closure(host, shift, [b])
            _, nu, cu, fu = plan.closure(host, shift, [a, b])
            assert np.array_equal(nu, na | nb) and np.array_equal(cu, ca | cb) and max(fa, fb) <= fu <= fa + fb, (shift, a, b)
    for chosen in ([e[0]], [e[5], e[12]]):
        prev = None
        for shift in (4, 6, 8, 10, 12):
            pre, need, cont, filled, masks = edge_closure_bytes(plan, host, shift, chosen)
            if prev is not None:
                assert all(not (f & ~g).any() for f, g in zip(prev[2], masks)) and not (prev[0] & ~cont).any() and prev[1] <= filled, (shift, chosen)
            prev = (cont, filled, masks)
    for shift in (4, 8):
        G = 1 << shift
        pre, need, cont, filled = plan.closure(host, shift, [e[0], e[7], e[14]])
        back = [(c, int(g) * G, min((int(g) + 1) * G, plan.lens[c]) - int(g) * G) for c in range(len(plan.lens)) for g in np.flatnonzero(need[int(pre[c]):int(pre[c + 1])])]
        _, need2, cont2, filled2 = plan.closure(host, shift, back)
        assert np.array_equal(need, need2) and np.array_equal(cont, cont2) and filled == filled2
