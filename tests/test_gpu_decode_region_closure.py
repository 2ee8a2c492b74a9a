"""The granule closure of `d --region` on the device (k_decode_closure_region) against its host referee (Provenance::closureRegion),
bit for bit, and the masked fill (k_decode_fill_region) against the unmasked one, through mbgc_decoder_region_probe
(mbgc_amd/host/mbgc_decoder.cpp): the streams of a set on disk are planned and scheduled as `d` does it, chosen pieces go in as the
need state, and both closures, the plan's record offsets and the sequence buffer after a masked forward run over 0xEE bytes come
back. On the chain set of test_gpu_decompress_region.py and on a set whose circular reference buffer has wrapped twice, with
reverse-complement loads."""
import os

import numpy as np
import pytest

import _meta
import test_gpu_decompress_region as region
from mbgc_amd import synth
from _regionprobe import check, host_lib, probe, tool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return host_lib()


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("chainprobe"))
    region.write_set(tmp)
    tool(["c", "list.txt", "out"], tmp)
    tool(["d", "out", "full"], tmp)
    return tmp, open(os.path.join(tmp, "full.seq"), "rb").read()


@pytest.mark.parametrize("granule", [256, 1024, 4096])
def test_chain_set(host, chain, granule):
    tmp, full_seq = chain
    last = region.CHAIN - 1
    pieces = [(last, 30_000, 2048), (last, 0, 1), (last, region.LEN - 1, 1), (region.CHAIN + 1, 2 * granule - 1, 2), (0, 5, 10)]
    p = probe(host, tmp, "out", pieces, granule, "g%d" % granule)
    need, contig, filled = check(p, full_seq, pieces, granule)
    p2 = probe(host, tmp, "out", pieces, granule, "s%d" % granule, serial=1)
    check(p2, full_seq, pieces, granule)


def test_deep_chain_is_followed_level_by_level(host, tmp_path):
    """g_i is a 1.5 % mutation of g_(i - 1) (the shape of test_gpu_decompress_select.py's deep chain, shorter): divergent enough for
    every link to enter the reference, so the last file's records read what earlier targets loaded and the sweep has levels to follow"""
    tmp = str(tmp_path)
    codes = [synth.base_codes(64 << 10, 321)]
    for i in range(1, 7):
        codes.append(synth.genome_codes(codes[-1], i, 0.015))
    paths = []
    for i, c in enumerate(codes):
        paths.append(os.path.join(tmp, "d%02d.fa" % i))
        with open(paths[-1], "wb") as f:
            f.write(synth.fasta_bytes(synth.ACGT[c], i))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "-R", "2", "list.txt", "out"], tmp)
    tool(["d", "out", "full"], tmp)
    full_seq = open(os.path.join(tmp, "full.seq"), "rb").read()
    pieces = [(6, 30_000, 2048), (6, 1023, 2)]
    for granule in (256, 1024):
        p = probe(host, tmp, "out", pieces, granule, "deep%d" % granule)
        need, contig, filled = check(p, full_seq, pieces, granule)
        print("deep chain, G = %d: %d contigs, %d bases filled" % (granule, int(contig.sum()), filled))
        assert contig[5] and contig.sum() >= 2


def test_wrapped_buffer_with_reverse_complement_loads(host, tmp_path):
    """--ref-factor 1 (a 4 MiB buffer) and the files of test_gpu_decompress_select.py's last-lap case: a 2.4 Mbp contig fills the
    first lap, 80 files of 60 kbp the next two; every third is a 1 % mutation of the file two before it — of its reverse complement
    for every sixth, so the copy reads what a reverse-complement load wrote"""
    tmp = str(tmp_path)
    paths = []
    us = []
    big = synth.ACGT[synth.base_codes(2_400_000, 77)]
    files = [[synth.ACGT[synth.base_codes(50_000, 5)]], [big]]
    for i in range(80):
        if i % 3 == 2:
            u = synth.genome_codes(us[i - 2], 5000 + i, 0.01)
            if i % 6 == 5:
                u = (3 - u[::-1]).astype(np.uint8)
        else:
            u = synth.base_codes(60_000, 1000 + i)
        us.append(u)
        files.append([synth.ACGT[u]])
    for i, recs in enumerate(files):
        paths.append(os.path.join(tmp, "w%02d.fa" % i))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(synth.fasta_bytes(s, 100 * i + j) for j, s in enumerate(recs)))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "--ref-factor", "1", "-R", "2", "list.txt", "out"], tmp)
    assert _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())["laps"] >= 2
    tool(["d", "out", "full"], tmp)
    full_seq = open(os.path.join(tmp, "full.seq"), "rb").read()
    copy, rc_copy = 2 + 74, 2 + 77                                 # contigs of the collection: u74 copies u72, u77 the reverse complement of u75
    pieces = [(copy, 20_000, 2000), (rc_copy, 1000, 3000), (rc_copy, 59_999, 1)]
    p = probe(host, tmp, "out", pieces, 1024, "wrap")
    need, contig, filled = check(p, full_seq, pieces, 1024)
    marked = set(np.flatnonzero(contig).tolist())
    assert {copy - 1, rc_copy - 1, copy - 1 - 2, rc_copy - 1 - 2} <= marked           # planned numbers: the copies and their originals
    assert filled < 4 * 60_000
