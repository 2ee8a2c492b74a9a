"""`mbgc-hip d --fasta dir --gzip`: the FASTA files of a collection written as <name>.gz, compressed on the device. On the three
Listeria genomes of tests/golden/listeria: every .gz gunzips to its plain twin and to the original, the project's own validator reads
them (`v --flat --root`), a file that spans batches is several gzip members and still one text, -i stream sets and --select compose,
--gzip without --fasta is refused, and without --gzip nothing changes."""
import json
import lzma
import os
import zlib

import pytest

from test_gpu_decompress import LIST, tool

pytestmark = pytest.mark.gpu


def members(blob):
    """(the text of all members, their number) by walking zlib's unused_data"""
    text, n = b"", 0
    while blob:
        z = zlib.decompressobj(31)
        text += z.decompress(blob)
        assert z.eof
        blob = z.unused_data
        n += 1
    return text, n


def gunzip_dir(d):
    return {f[:-3]: members(open(os.path.join(d, f), "rb").read()) for f in sorted(os.listdir(d)) if f.endswith(".gz")}


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    """the three genomes, `c list out`, `d --fasta plain out b`, `d --fasta gz --gzip out b2`"""
    tmp = str(tmp_path_factory.mktemp("gzout"))
    names = json.load(open(os.path.join(LIST, "expected_t1.json")))["files"]
    paths = []
    for f in names:
        p = os.path.join(tmp, f)
        open(p, "wb").write(lzma.open(os.path.join(LIST, f + ".xz")).read())
        paths.append(p)
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(paths) + "\n")
    tool(["c", "list.txt", "out"], tmp)
    plain = tool(["d", "--fasta", "plain", "out", "b"], tmp)
    gz = tool(["d", "--fasta", "gz", "--gzip", "out", "b2"], tmp)
    return tmp, names, {f: open(os.path.join(tmp, f), "rb").read() for f in names}, plain, gz


def test_every_file_gunzips_to_its_plain_twin_and_the_original(lm):
    tmp, names, originals, plain, gz = lm
    assert sorted(os.listdir(os.path.join(tmp, "gz"))) == sorted(f + ".gz" for f in os.listdir(os.path.join(tmp, "plain")))
    assert sorted(os.listdir(os.path.join(tmp, "plain"))) == sorted(names)
    back = gunzip_dir(os.path.join(tmp, "gz"))
    for f in names:
        assert back[f][0] == open(os.path.join(tmp, "plain", f), "rb").read() == originals[f], f
        assert back[f][1] == 1
    assert open(os.path.join(tmp, "b2.seq"), "rb").read() == open(os.path.join(tmp, "b.seq"), "rb").read()


def test_without_gzip_nothing_changes(lm):
    tmp, names, originals, plain, gz = lm
    assert sorted(os.listdir(os.path.join(tmp, "plain"))) == sorted(names)                      # no .gz file, the same list
    for f in names:
        assert open(os.path.join(tmp, "plain", f), "rb").read() == originals[f]
    assert "gz" not in plain.stdout


def test_the_projects_validator_reads_the_projects_gzip(lm):
    tmp, names, originals, plain, gz = lm
    r = tool(["v", "--flat", "--root", "gz", "out"], tmp, ok=False)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Validation: correctly decoded %d out of %d files." % (len(names), len(names)) in r.stdout


def test_a_file_that_spans_batches_is_several_members(lm, tmp_path):
    tmp, names, originals, plain, gz = lm
    # list mode batches whole files: a file spans batches in a single-FASTA stream set
    single = os.path.join(tmp, "all.fna")
    open(single, "wb").write(b"".join(originals[f] for f in names))
    tool(["c", "-i", "all.fna", "one"], tmp)
    tool(["d", "--fasta", "gz1", "--gzip", "--batch-kib", "1024", "one", "b3"], tmp)
    assert os.listdir(os.path.join(tmp, "gz1")) == ["all.fna.gz"]
    text, n = members(open(os.path.join(tmp, "gz1", "all.fna.gz"), "rb").read())
    assert n > 1 and text == open(single, "rb").read()
    r = tool(["v", "--flat", "--root", "gz1", "one"], tmp, ok=False)
    assert r.returncode == 0 and "Validation: correctly decoded 1 out of 1 files." in r.stdout, r.stdout + r.stderr
    # list mode with small batches: the same files as with one batch
    tool(["d", "--fasta", "gz2", "--gzip", "--batch-kib", "1024", "out", "b4"], tmp)
    back = gunzip_dir(os.path.join(tmp, "gz2"))
    assert sorted(back) == sorted(names)
    for f in names:
        assert back[f][0] == originals[f]
    r = tool(["v", "--flat", "--root", "gz2", "--batch-kib", "1024", "out"], tmp, ok=False)
    assert r.returncode == 0, r.stdout + r.stderr


def test_select_writes_only_the_chosen_file(lm):
    tmp, names, originals, plain, gz = lm
    tool(["d", "--fasta", "gzsel", "--gzip", "--select", names[1], "out", "b5"], tmp)
    assert os.listdir(os.path.join(tmp, "gzsel")) == [names[1] + ".gz"]
    assert gunzip_dir(os.path.join(tmp, "gzsel"))[names[1]][0] == originals[names[1]]


def test_gzip_without_fasta_is_refused(lm):
    tmp = lm[0]
    r = tool(["d", "--gzip", "out", "b6"], tmp, ok=False)
    assert r.returncode == 1 and "--gzip needs --fasta" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "b6.seq"))
    r = tool(["v", "--gzip", "out"], tmp, ok=False)                                             # v does not take it
    assert r.returncode != 0


def test_bench_prints_the_gzip_line(lm):
    tmp, names, originals, plain, gz = lm
    r = tool(["d", "--fasta", "gzb", "--gzip", "--bench", "out", "b7"], tmp)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    plain_lines = [json.loads(l) for l in tool(["d", "--fasta", "plainb", "--bench", "out", "b8"], tmp).stdout.splitlines() if l.startswith("{")]
    assert len(lines) == len(plain_lines) + 1 and [sorted(l) for l in lines[:-1]] == [sorted(l) for l in plain_lines]
    last = lines[-1]
    assert {"text_bytes", "gz_bytes", "deflate_kernel_ms", "download_ms", "write_ms", "chunks", "stored_chunks"} <= set(last)
    assert last["gz_bytes"] == sum(os.path.getsize(os.path.join(tmp, "gz", f + ".gz")) for f in names)
    assert last["text_bytes"] == sum(len(t) for t in originals.values()) and last["deflate_kernel_ms"] > 0
