"""Literal-stream-like test sequences for the -m3 reverse-complement pass: random bases with planted reverse-complement
copies (short, long, overlapping, palindromic, many-fold), stream marks among them."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def revcomp(x):
    return COMP[x][::-1]


def literal_like(n, seed, copies=40, longest=3000, marks=True, mutate=0.0):
    rng = np.random.default_rng(seed)
    s = ACGT[rng.integers(0, 4, n)].copy()
    for k in range(copies):
        ln = int(rng.integers(40, longest))
        if 2 * ln + 10 >= n:
            continue
        a = int(rng.integers(0, n - ln))
        b = int(rng.integers(0, n - ln))
        piece = revcomp(s[a:a + ln]).copy()
        if mutate:
            m = rng.random(ln) < mutate
            piece[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        s[b:b + ln] = piece
    if marks:                                          # match marks / sequence separators / a lower-case run / an N run
        for p in rng.integers(0, n, max(1, n // 5000)):
            s[p] = 0xA5 if p % 2 else 0xA2
        a = int(rng.integers(0, max(1, n - 200)))
        s[a:a + 60] = np.frombuffer(bytes(s[a:a + 60]).lower(), dtype=np.uint8)
        a = int(rng.integers(0, max(1, n - 200)))
        s[a:a + 30] = ord("N")
    return s


def cases():
    out = {
        "planted": literal_like(300_000, 1),
        "long_copies": literal_like(400_000, 2, copies=12, longest=20_000),          # matches far longer than a 256-sample block
        "mutated": literal_like(300_000, 3, copies=60, longest=2_000, mutate=0.01),
        "tiny": literal_like(54, 4, copies=0),                                         # shorter than the target length: untouched
        "short": literal_like(700, 5, copies=3, longest=200),                          # no full 256-sample block: tail loop only
    }
    # one 400-base unit planted 40 times forward and 40 times reverse-complemented: buckets beyond 13 entries
    rng = np.random.default_rng(6)
    s = ACGT[rng.integers(0, 4, 200_000)].copy()
    unit = ACGT[rng.integers(0, 4, 400)]
    for k in range(40):
        a = 1000 + k * 2300
        s[a:a + 400] = unit
        s[a + 1100:a + 1500] = revcomp(unit)
    out["manyfold"] = s
    # a palindromic region (equal to its own reverse complement) and a copy pair that overlaps itself
    s = ACGT[rng.integers(0, 4, 120_000)].copy()
    half = ACGT[rng.integers(0, 4, 900)]
    s[5000:5900] = half
    s[5900:6800] = revcomp(half)
    s[40_000:41_500] = revcomp(s[39_200:40_700]).copy()
    out["palindromes"] = s
    return out


# ---- texts whose lengths sit on the edges of the query's geometry ("edge lengths")
EDGE_TARGETS = (55, 32, 80, 120, 24)                      # what MBGC asks for (55, 32) and three other (K, k1, k2, skip)
EDGE_GROUPS = ("t", "m0", "m1", "m2")                     # lengths around the target length / around B(0), B(1), B(2)
EDGE_CONTENTS = ("none", "ends", "whole", "into_tail", "tail_only", "at", "acgt", "aatt")
QB = 256                                                  # query samples per block (MULTI, CopMEMMatcher.cpp:352)
_edge = {}


def edge_params(target):
    """(K, k1, k2) as the oracle derives them for this target length"""
    import _orc
    return _orc.rc_find_matches(np.full(target, ord("A"), dtype=np.uint8), target)[1][:3]


def edge_geometry(n, K, k2):
    """-> (whole query blocks, the tail's first query position): block b exists while b * 256 k2 + K + 256 k2 < n + 1 (:370)"""
    n_main = (n - K) // (QB * k2) if n >= K else 0
    return n_main, n_main * QB * k2


def edge_lengths(target):
    """group -> ascending lengths. B(m) = K + 256 k2 (m + 1) is the first length with m + 1 whole blocks (and a tail of one
    sample; B(m) - 1 has m blocks and a tail of 256); at B(1) + k2 the tail gains its second sample."""
    K, _, k2 = edge_params(target)
    B = [K + QB * k2 * (m + 1) for m in range(3)]
    out = {"t": [target - 1, target, target + 1]}
    for m in range(3):
        out["m%d" % m] = [B[m] - 1, B[m], B[m] + 1]
    out["m1"] = sorted(set(out["m1"] + [B[1] + k2 - 1, B[1] + k2]))
    return out


def _edge_text(content, n, target, K, k2, rng):
    """one text, or None where the content does not fit the length. Query byte j is the complement of text byte n - 1 - j,
    and a candidate is tried only while source + query position <= n (:388-390): of a reverse-complement pair the reference
    reports the one whose source lies left of its destination in the text. So a match in the query's tail has source and
    destination in the text's head, and one that reaches from the last whole block to the text's first bytes overlaps its
    own source: a region that is its own reverse complement."""
    n_main, tb = edge_geometry(n, K, k2)
    s = ACGT[rng.integers(0, 4, n)].copy()
    if content == "none":
        return s
    if content == "ends":                                  # the last ln bytes are the reverse complement of the first ln
        ln = min(n // 2 - 1, 300)
        if ln < target:
            return None
        s[n - ln:] = revcomp(s[:ln])
        return s
    if content == "whole":                                 # its own reverse complement from end to end
        h = s[:n // 2]
        mid = np.frombuffer(b"N", dtype=np.uint8) if n % 2 else s[:0]
        return np.concatenate([h, mid, revcomp(h)])
    if content == "into_tail":
        # query span [d0, e) with d0 inside the last whole block and e inside the tail, its own reverse complement; up to
        # 1500 bytes, and 400 or more wherever block and tail are wide enough (k2 = 1 at B(m): 256 + K bytes in all); the
        # centre behind the boundary where the tail is long enough, so that tail samples lie inside the carried match
        if n_main < 1:
            return None
        e = min(n - n % 3, tb + 1000)                      # (n % 3 == 0 in a short tail: the span ends on the query's last byte)
        lo = max(tb - QB * k2 + 1, e - 1500)
        d0 = max(lo, min(2 * tb - e + 2 * K, tb - 200, e - 400))
        d0 += (e - d0) % 2
        if not (d0 < tb < e) or e - d0 < 2 * (target + 2):
            return None
        a, h = n - e, (e - d0) // 2
        s[a + h:a + 2 * h] = revcomp(s[a:a + h])
        return s
    if content == "tail_only":                             # source and copy both in the text's head = the query's tail
        ln, a = target + 8, 3
        r = a + ln + 5
        if r + ln >= n - tb:                               # (the tail's span is the text's first n - tb bytes)
            return None
        s[r:r + ln] = revcomp(s[a:a + ln])
        return s
    if content == "at":
        return np.frombuffer((b"AT" * (n // 2 + 1))[:n], dtype=np.uint8).copy()
    if content == "acgt":
        return np.frombuffer((b"ACGT" * (n // 4 + 1))[:n], dtype=np.uint8).copy()
    if content == "aatt":
        return np.frombuffer(b"A" * (n // 2) + b"T" * (n - n // 2), dtype=np.uint8).copy()
    raise KeyError(content)


def edge_inputs(target):
    """[(name, uint8 array)], deterministic; name = "<group>-<content>-n<length>", every content at every length it fits"""
    if target not in _edge:
        K, _, k2 = edge_params(target)
        out = []
        for group, lengths in edge_lengths(target).items():
            for content in EDGE_CONTENTS:
                for n in lengths:
                    rng = np.random.default_rng([target, n, EDGE_CONTENTS.index(content)])
                    s = _edge_text(content, n, target, K, k2, rng)
                    if s is not None:
                        assert s.size == n and s.dtype == np.uint8
                        out.append(("%s-%s-n%d" % (group, content, n), s))
        _edge[target] = out
    return _edge[target]


# the contents that fit the lengths around the target length itself (no whole block, no room for a planted copy)
EDGE_ITEMS = [(t, g, c) for t in EDGE_TARGETS for g in EDGE_GROUPS for c in EDGE_CONTENTS
              if g != "t" or c in ("none", "whole", "at", "acgt", "aatt")]


def edge_item(target, group, content):
    """the inputs of one test item, ascending in length"""
    pre = "%s-%s-n" % (group, content)
    return [(name, s) for name, s in edge_inputs(target) if name.startswith(pre)]


def edge_expect(name, s, rows, target):
    """non-vacuity, on the oracle's rows (src, len, dest in query coordinates) of one input"""
    K, _, k2 = edge_params(target)
    n = s.size
    _, tb = edge_geometry(n, K, k2)
    content = name.split("-")[1]
    src, ln, dest = (rows[:, i].astype(np.int64) for i in range(3))
    if content == "none":
        assert len(rows) == 0, name
    elif content == "ends":
        # the left walk (:412-415) stops when it REACHES either text's first byte, without comparing it: the earliest start it
        # can report is byte 1 of both, and only a walk stopped by that limit reports it with equal bytes at 0. The planted
        # match lies on the main diagonal (query[0:ln] == text[0:ln]).
        assert s[0] == COMP[s[n - 1]] and np.any((src == 1) & (dest == 1) & (ln >= min(n // 2 - 1, 300) - 1)), name
    elif content == "whole" and n > target:
        # ... and the right walk (:409-410) runs to the last byte of both texts at once
        assert np.any((src == 1) & (dest == 1) & (ln == n - 1)), name
    elif content == "into_tail":
        assert np.any((dest < tb) & (dest + ln > tb)), name
    elif content == "tail_only":
        assert np.any((dest >= tb) & (ln >= target + 8)), name
    elif content in ("at", "acgt", "aatt") and n >= 2000:
        assert len(rows) > 1, name
