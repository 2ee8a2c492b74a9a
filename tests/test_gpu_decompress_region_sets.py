"""`mbgc-hip d --region` on the sets where the closure has work to do (_regionprobe.py: the reverse-complemented chain, plain and
through `c -t1`, `c -m 3` and `c -i`; two files of 200 records; the set whose buffer has lapped), against the Python cut of the
unselected `d` of the same streams. And `--region-granule`: the bytes that come out do not depend on it, the bases filled do not
decrease as it grows, `--bench` reports it, and what is no power of two from 16 to 2^30 is refused."""
import os
import re
import zlib

import pytest

import _regionprobe as rp

pytestmark = pytest.mark.gpu
SETS = list(rp.VARIANTS)


@pytest.fixture(scope="module")
def host():
    return rp.host_lib()


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return lambda name: rp.stream_set(tmp_path_factory, name)


def last_dependent(s, host):
    """(record, its header's first word, its length, the destAt of a plan record near its middle) of the set's last record that copies.
    Where the first file is a target as well (-t1, -m 3, -i) the probe counts the initial reference in front of the records"""
    p = s.probe(host, [(0, 0, 1)], 256, "geometry")
    g0n = p["contigLen"].size - (p["granBase"].size - 1)
    shift = p["contigLen"].size - len(s.full.headers)
    assert shift in (0, g0n)
    for c in range(p["contigLen"].size - 1, g0n - 1, -1):
        d = p["recDest"][int(p["recBase"][c - g0n]):int(p["recBase"][c - g0n + 1])]
        if d.size >= 3:
            assert p["contigLen"][c] == s.full.lens[c - shift]
            return c - shift, s.full.headers[c - shift].split()[0] + b" ", int(p["contigLen"][c]), int(d[d.size // 2])
    raise AssertionError("no record of the set copies anything")


@pytest.mark.parametrize("name", SETS)
def test_a_region_across_a_record_boundary(sets, host, name):
    """in the last record that copies: 40 bases either side of the destAt of one of its plan records; with --fasta, the text too"""
    s = sets(name)
    r, word, n, at = last_dependent(s, host)
    assert 40 <= at <= n - 40
    specs = [(word, at - 39, at + 40), (word, at, at), (word, at + 1, at + 1), (word, n, n + 7)]
    name = "edge_" + s.prefix
    out, pieces = rp.run_regions(s.full, specs, name, fasta_args=[])
    assert [p[0] for p in pieces] == [r] * 4
    path = os.path.join(s.tmp, name + "_fa", "all.fa" if s.one_file else sorted(os.listdir(os.path.join(s.tmp, name + "_fa")))[0])
    assert len(os.listdir(os.path.join(s.tmp, name + "_fa"))) == 1
    assert open(path, "rb").read() == b"".join(rp.piece_text(s.full, *p) for p in pieces)


def many_specs():
    """about 20 patterns: the 15-, 16- and 17-base records under 1-16, 16-17 and 1-9999 (16-17 starts behind the end of the 15-base
    one), records of about a granule, and b records, several pieces of one of them"""
    lens = rp.many_lengths()
    specs = []
    for want in (15, 16, 17):
        pat = b"a%03d " % lens.index(want)
        specs += [(pat, 1, 16), (pat, 16, 17), (pat, 1, 9999)]
    for want in (255, 256, 257):
        specs.append((b"a%03d " % lens.index(want), 255, 258))
    specs += [(b"b%03d " % i, 50 * k + 1, 50 * k + 333) for k, i in enumerate((0, 7, 7, 7, 64, 199, 199, 120))]
    specs.append((b"a01", 10, 12))                                 # ten records by one pattern
    return specs


def test_region_list_over_many_records(sets):
    s = sets("many-records")
    specs = many_specs()
    with open(os.path.join(s.tmp, "regions.txt"), "w") as f:
        f.write("".join("%s:%d-%d\n" % (p.decode(), a, b) for p, a, b in specs))
    out, pieces = rp.run_regions(s.full, specs, "listed", region_args=["--region-list", "regions.txt"], fasta_args=[])
    assert "1 out of range" in out and len(pieces) >= 25
    assert sorted(os.listdir(os.path.join(s.tmp, "listed_fa"))) == ["m01.fa", "m02.fa"]
    for f in (1, 2):
        want = b"".join(rp.piece_text(s.full, *p) for p in pieces if s.full.file_of[p[0]] == f)
        assert open(os.path.join(s.tmp, "listed_fa", "m%02d.fa" % f), "rb").read() == want, f


def test_fasta_gzip_over_many_records(sets):
    """several pieces of one file stand side by side in a batch"""
    s = sets("many-records")
    specs = many_specs()
    out, pieces = rp.run_regions(s.full, specs, "gz", fasta_args=["--gzip"])
    for f in (1, 2):
        data = open(os.path.join(s.tmp, "gz_fa", "m%02d.fa.gz" % f), "rb").read()
        text = b""
        while data:
            d = zlib.decompressobj(31)
            text += d.decompress(data) + d.flush()
            assert d.eof
            data = d.unused_data
        assert text == b"".join(rp.piece_text(s.full, *p) for p in pieces if s.full.file_of[p[0]] == f), f


FILLED = re.compile(r"closure: \d+ of \d+ contigs, (\d+) of \d+ bases")


def test_region_granule_changes_no_output_byte(sets, host):
    s = sets("rc-chain")
    r, word, n, at = last_dependent(s, host)
    specs = [(word, at - 39, at + 40), (word, 1, 1), (word, n, n)]
    out, _ = rp.run_regions(s.full, specs, "gdefault")
    filled = {256: int(FILLED.search(out).group(1))}
    for g in (16, 64, 4096, 65536):
        out, _ = rp.run_regions(s.full, specs, "g%d" % g, extra=["--region-granule", str(g)])
        filled[g] = int(FILLED.search(out).group(1))
        for ext in rp.OUTS:
            assert open(os.path.join(s.tmp, "g%d.%s" % (g, ext)), "rb").read() == open(os.path.join(s.tmp, "gdefault." + ext), "rb").read(), (g, ext)
    order = [filled[g] for g in sorted(filled)]
    print("filled by granule:", dict(sorted(filled.items())))
    assert order == sorted(order) and order[0] > 0 and order[0] < order[-1]
    explicit, _ = rp.run_regions(s.full, specs, "g256", extra=["--region-granule", "256"])
    assert int(FILLED.search(explicit).group(1)) == filled[256]


@pytest.mark.parametrize("granule", [16, 65536])
def test_bench_reports_the_granule_asked_for(sets, granule):
    s = sets("rc-chain")
    out = rp.tool(["d", "--bench", "--region-granule", str(granule), "--region", "link6 :1000-1999", s.prefix, "benchno"], s.tmp).stdout
    assert re.search(r'"regions": 1, "region_bases": 1000, "granule_bytes": %d\b' % granule, out), out
    assert not os.path.exists(os.path.join(s.tmp, "benchno.seq"))


@pytest.mark.parametrize("granule", ["0", "8", "24", "2147483648"])
def test_region_granule_refusals(sets, granule):
    s = sets("rc-chain")
    r = rp.tool(["d", "--region-granule", granule, "--region", "link6 :1-5", s.prefix, "no"], s.tmp, ok=False)
    assert r.returncode == 1 and "--region-granule" in r.stderr, (r.returncode, r.stderr)
    assert not [p for p in os.listdir(s.tmp) if p.startswith("no.")]
