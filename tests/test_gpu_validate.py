"""`mbgc-hip v`: a stream set validated against its FASTA files on the device (decode, format, upload of the originals, one compare
call per batch; the reference's `mbgc v`): clean collections in every schedule, gzip and CRLF originals, the way round through
`d --fasta`, single-FASTA collections over several units and batches, and damaged originals — which file, what kind of damage, and
where (seqIdx / seqPos computed here from the file the test wrote)."""
import gzip
import json
import os
import re
import shutil

import pytest

from mbgc_amd import synth
from test_gpu_decompress import cut, tool, write_collection

pytestmark = pytest.mark.gpu


def validate(tmp, extra=(), prefix="out", rc=0):
    before = sorted(os.listdir(tmp))
    r = tool(["v"] + list(extra) + [prefix], tmp, ok=False)
    assert r.returncode == rc, (r.returncode, r.stdout, r.stderr)
    if "--dump" not in extra:
        assert sorted(os.listdir(tmp)) == before                                     # nothing is written
    return r


def verdict(r):
    m = re.search(r"^Validation( ERROR)?: correctly decoded (\d+) out of (\d+) files\.$", r.stdout, re.M)
    assert m, r.stdout
    return bool(m.group(1)), int(m.group(2)), int(m.group(3))


def locate(data, at):
    """the reference's report for a first difference at byte `at` of FASTA text `data` (MBGC_Decoder.cpp:157-170)"""
    head = data[:at]
    idx = head.count(b">") - 1
    rec = head[head.rindex(b">"):]
    if b"\n" not in rec:
        return "Error in header:\t\tseqIdx = %d" % idx
    body = rec[rec.index(b"\n"):]
    return "Error location:\t\tseqIdx = %d\tseqPos = %d" % (idx, len(body) - body.count(b"\n"))


CLEAN = [(["-R", "3"], [], 7), (["-t1"], [], 5), (["-m", "2", "-R", "3"], [], 7), (["-m", "3"], ["--restore-rc"], 5)]


@pytest.mark.parametrize("args,extra,n", CLEAN, ids=[" ".join(a) for a, _, _ in CLEAN])
def test_clean_collection_is_valid_in_every_schedule(tmp_path, args, extra, n):
    tmp = str(tmp_path)
    write_collection(tmp, n, 100_000 + 2000 * n)
    tool(["c"] + args + ["list.txt", "out"], tmp)
    for how in ([], ["--serial"], ["--no-index"]):
        r = validate(tmp, extra + how)
        assert verdict(r) == (False, n, n), (how, r.stdout)
        assert "Validation ERROR" not in r.stdout + r.stderr


def test_gzip_and_crlf_originals_are_valid(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 6, 100_000)
    g = [synth.genome(synth.base_codes(100_000, 55), i, 0.015) for i in range(6)]
    crlf = synth.fasta_bytes(g[2], 20, 59).replace(b"\n", b"\r\n") + synth.fasta_bytes(g[2][:7001], 21, 59).replace(b"\n", b"\r\n")
    open(paths[2], "wb").write(crlf)
    with gzip.open(paths[3] + ".gz", "wb") as f:                                     # named with .gz in the list
        f.write(open(paths[3], "rb").read())
    os.remove(paths[3])
    paths[3] += ".gz"
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    assert verdict(validate(tmp)) == (False, 6, 6)
    with gzip.open(paths[4] + ".gz", "wb") as f:                                     # named without: <path>.gz is tried when the path is gone
        f.write(open(paths[4], "rb").read())
    os.remove(paths[4])
    assert verdict(validate(tmp)) == (False, 6, 6)


def test_what_d_fasta_wrote_validates_with_flat_and_root(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 6, 100_000)
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    tool(["d", "--fasta", "back", "out", "b"], tmp)
    for p in paths:
        os.remove(p)                                                                 # (only the copies are left)
    assert verdict(validate(tmp, ["--flat", "--root", "back"])) == (False, 6, 6)
    r = validate(tmp, rc=2)                                                          # without them the names of the list are looked for
    assert verdict(r) == (True, 0, 6) and r.stderr.count("Cannot find") == 6


def test_relative_names_under_root(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 5, 100_000)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(os.path.basename(p) for p in paths) + "\n")
    tool(["c", "-R", "2", "list.txt", "out"], tmp)
    assert verdict(validate(tmp)) == (False, 5, 5)
    os.mkdir(os.path.join(tmp, "moved"))
    for p in paths:
        shutil.move(p, os.path.join(tmp, "moved"))
    assert verdict(validate(tmp, ["--root", "moved"])) == (False, 5, 5)


@pytest.fixture(scope="module")
def single_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("single"))
    base = synth.base_codes(110_000, 5)
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        for i in range(100):                                                         # 11 MB: enough elements of 2 MiB for the round schedule (a smaller file is one target)
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                f.write(synth.fasta_bytes(c, i * 10 + j))
    out = tool(["c", "-i", "all.fa", "--window-kib", "256", "out"], tmp).stdout       # (the name in out.names is relative: damaged copies are found under --root)
    assert int(re.search(r"single-file elements: (\d+)", out).group(1)) >= 3
    return tmp


@pytest.mark.parametrize("batch", [[], ["--batch-kib", "200"]], ids=["one-batch", "batches"])
def test_single_fasta_collection(single_run, tmp_path, batch):
    """one file over several units (and, with small batches, several compare calls at the file's running offset)"""
    assert verdict(validate(single_run, batch)) == (False, 1, 1)
    data = open(os.path.join(single_run, "all.fa"), "rb").read()
    root = str(tmp_path)
    at = data.index(b"\n", 3_000_000) - 11                                           # a base in the file's second unit (a batch of its own when batches are small)
    assert data[at] in b"ACGT"
    bad = bytearray(data)
    bad[at] = ord("A") if data[at] != ord("A") else ord("C")
    open(os.path.join(root, "all.fa"), "wb").write(bytes(bad))
    dump = os.path.join(root, "dump")
    r = validate(single_run, batch + ["--root", root, "--dump", dump], rc=2)
    assert verdict(r) == (True, 0, 1)
    assert "all.fa contents differ." in r.stdout and locate(data, at) in r.stdout
    assert os.listdir(dump) == ["all.fa"] and open(os.path.join(dump, "all.fa"), "rb").read() == data     # (formatted once more, batch by batch)
    open(os.path.join(root, "all.fa"), "wb").write(data[:-1000])                     # the original ends early: the location is the end of the equal part
    r = validate(single_run, batch + ["--root", root], rc=2)
    assert "all.fa size differ (%d instead of %d)" % (len(data), len(data) - 1000) in r.stdout
    assert locate(data, len(data) - 1000) in r.stdout
    r = tool(["v", "--select", "all", "out"], single_run, ok=False)                  # refused as d refuses it
    assert r.returncode == 1 and "mbgc-hip v: --select: the streams hold one FASTA file" in r.stderr


# ---- damaged originals: one compress run, the originals copied and damaged under a --root of the test's own
@pytest.fixture(scope="module")
def run8(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("damaged"))
    paths = write_collection(tmp, 8, 100_000)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(os.path.basename(p) for p in paths) + "\n")
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    return tmp


def damaged_copy(run, root, changes):
    """the originals of `run` under root, file name -> new bytes (None: the file is left out)"""
    for f in sorted(os.listdir(run)):
        if f.endswith(".fa"):
            data = changes.get(f, open(os.path.join(run, f), "rb").read())
            if data is not None:
                open(os.path.join(root, f), "wb").write(data)


def base_in_second_record(data):
    second = data.index(b">", 1)
    body = data.index(b"\n", second) + 1
    end = data.find(b">", body)
    at = (body + (end if end >= 0 else len(data))) // 2
    if data[at] == 10:
        at += 1
    return at


def flip(data, at):
    bad = bytearray(data)
    bad[at] = ord("A") if data[at] != ord("A") else ord("C")
    return bytes(bad)


@pytest.mark.parametrize("batch", [[], ["--batch-kib", "150"]], ids=["one-batch", "batches"])
def test_one_base_changed(run8, tmp_path, batch):
    data = open(os.path.join(run8, "g05.fa"), "rb").read()
    at = base_in_second_record(data)
    damaged_copy(run8, str(tmp_path), {"g05.fa": flip(data, at)})
    r = validate(run8, ["--root", str(tmp_path)] + batch, rc=2)
    assert verdict(r) == (True, 7, 8)
    assert re.search(r"^Validation ERROR: ~5\. %s contents differ\.$" % re.escape(os.path.join(str(tmp_path), "g05.fa")), r.stdout, re.M), r.stdout
    want = locate(data, at)
    assert want.startswith("Error location:\t\tseqIdx = 1\tseqPos = ") and want in r.stdout
    assert r.stdout.count("Validation ERROR: ~") == 1
    assert "Validation ERROR: errors in contents of 1 decoded files." in r.stderr


def test_one_header_byte_changed(run8, tmp_path):
    data = open(os.path.join(run8, "g04.fa"), "rb").read()
    at = data.index(b">", 1) + 5
    bad = bytearray(data)
    bad[at] ^= 1
    damaged_copy(run8, str(tmp_path), {"g04.fa": bytes(bad)})
    r = validate(run8, ["--root", str(tmp_path)], rc=2)
    assert verdict(r) == (True, 7, 8)
    assert "g04.fa contents differ." in r.stdout and "Error in header:\t\tseqIdx = 1\n" in r.stdout
    assert locate(data, at) == "Error in header:\t\tseqIdx = 1"


def test_one_byte_appended(run8, tmp_path):
    data = open(os.path.join(run8, "g01.fa"), "rb").read()
    damaged_copy(run8, str(tmp_path), {"g01.fa": data + b"\n"})
    r = validate(run8, ["--root", str(tmp_path)], rc=2)
    assert verdict(r) == (True, 7, 8)
    assert "g01.fa size differ (%d instead of %d)" % (len(data), len(data) + 1) in r.stdout
    assert "contents differ" not in r.stdout


def test_one_file_removed(run8, tmp_path):
    damaged_copy(run8, str(tmp_path), {"g06.fa": None})
    r = validate(run8, ["--root", str(tmp_path)], rc=2)
    assert verdict(r) == (True, 7, 8)
    assert "Cannot find %s for validation." % os.path.join(str(tmp_path), "g06.fa") in r.stderr
    assert "Validation ERROR: ~" not in r.stdout


def test_two_files_damaged(run8, tmp_path):
    d2, d7 = (open(os.path.join(run8, f), "rb").read() for f in ("g02.fa", "g07.fa"))
    damaged_copy(run8, str(tmp_path), {"g02.fa": flip(d2, len(d2) - 2), "g07.fa": flip(d7, d7.index(b"\n") + 1)})
    r = validate(run8, ["--root", str(tmp_path)], rc=2)
    assert verdict(r) == (True, 6, 8)
    assert re.findall(r"^Validation ERROR: ~(\d+)\. \S+/(g\d+\.fa) contents differ\.$", r.stdout, re.M) == [("2", "g02.fa"), ("7", "g07.fa")]
    assert locate(d2, len(d2) - 2) in r.stdout and locate(d7, d7.index(b"\n") + 1) in r.stdout
    assert locate(d7, d7.index(b"\n") + 1) == "Error location:\t\tseqIdx = 0\tseqPos = 0"
    assert "errors in contents of 2 decoded files" in r.stderr


def test_select_validates_the_chosen_file_only(run8, tmp_path):
    data = open(os.path.join(run8, "g05.fa"), "rb").read()
    damaged_copy(run8, str(tmp_path), {"g05.fa": flip(data, base_in_second_record(data))})
    assert verdict(validate(run8, ["--root", str(tmp_path), "--select", "g03"])) == (False, 1, 1)      # the damaged file is outside the selection
    r = validate(run8, ["--root", str(tmp_path), "--select", "g03", "--select", "g05"], rc=2)
    assert verdict(r) == (True, 1, 2) and "g05.fa contents differ." in r.stdout


def test_dump_writes_the_decoded_text_of_the_damaged_file(run8, tmp_path):
    data = open(os.path.join(run8, "g05.fa"), "rb").read()
    root = os.path.join(str(tmp_path), "root")
    os.mkdir(root)
    damaged_copy(run8, root, {"g05.fa": flip(data, base_in_second_record(data))})
    dump = os.path.join(str(tmp_path), "dumped", "here")
    validate(run8, ["--root", root, "--dump", dump], rc=2)
    assert os.listdir(dump) == ["g05.fa"]
    assert open(os.path.join(dump, "g05.fa"), "rb").read() == data                   # the text as decoded: the undamaged original
    assert sorted(os.listdir(str(tmp_path))) == ["dumped", "root"]


def test_uppercase_streams_over_lowercase_originals(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 5, 100_000)
    for p in paths:
        data = open(p, "rb").read()
        first = data.index(b"\n") + 1
        open(p, "wb").write(data[:first + 3] + data[first + 3: first + 9].lower() + data[first + 9:])
    tool(["c", "-U", "-R", "2", "list.txt", "out"], tmp)
    r = validate(tmp, rc=2)
    assert verdict(r) == (True, 0, 5)
    assert r.stdout.count("contents differ.") == 5 and r.stdout.count("Error location:\t\tseqIdx = 0\tseqPos = 3\n") == 5
    notice = r.stdout.index("written with -U")
    assert notice < r.stdout.index("Validation ERROR")


def test_skip_compare_and_bench(run8):
    r = validate(run8, ["--skip-compare"])
    assert "Validation" not in r.stdout + r.stderr and "decoded:" in r.stdout
    r = validate(run8, ["--bench"])
    assert verdict(r) == (False, 8, 8) and r.stdout.count("correctly decoded") == 1
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert r.stdout.index("correctly decoded") < r.stdout.index('{"metric"')
    total = sum(os.path.getsize(os.path.join(run8, f)) for f in os.listdir(run8) if f.endswith(".fa"))
    assert line["compared_bytes"] == total == line["text_bytes"] and line["files"] == 8 and line["valid"] == 8
    for key in ("compare_kernel_ms", "upload_ms", "read_inflate_ms", "plan_ms", "fill_ms", "load_ms", "value", "bases"):
        assert line[key] > 0, key


def test_refusals_are_those_of_d(run8, tmp_path):
    tmp = str(tmp_path)
    for f in os.listdir(run8):
        if f.startswith("out."):
            data = open(os.path.join(run8, f), "rb").read()
            open(os.path.join(tmp, f), "wb").write(data[data.index(b"\n") + 1:] if f == "out.headers" else data)
    r = validate(tmp, rc=1)
    assert "mbgc-hip v: malformed .headers" in r.stderr and "Validation" not in r.stdout
    os.remove(os.path.join(tmp, "out.names"))
    r = validate(tmp, rc=1)
    assert "mbgc-hip v: malformed stream set: cannot open" in r.stderr and ".names" in r.stderr
    assert tool(["v", "--gpus", "2", "out"], tmp, ok=False).returncode == 1


def test_m3_without_restore_rc_is_refused(tmp_path):
    tmp = str(tmp_path)
    write_collection(tmp, 5, 100_000)
    tool(["c", "-m", "3", "list.txt", "out"], tmp)
    r = validate(tmp, rc=1)
    assert "mbgc-hip v: " in r.stderr and "-m 3" in r.stderr and "--restore-rc" in r.stderr


def test_four_damaged_files_are_reported_and_the_first_three_dumped(run8, tmp_path):
    """VALIDATION_DUMP_LIMIT = 3: every invalid file is logged, only the first three are downloaded and written"""
    names = ["g01.fa", "g03.fa", "g04.fa", "g06.fa"]
    whole = {f: open(os.path.join(run8, f), "rb").read() for f in names}
    root = os.path.join(str(tmp_path), "root")
    os.mkdir(root)
    damaged_copy(run8, root, {f: flip(d, base_in_second_record(d) if d.count(b">") > 1 else len(d) // 2) for f, d in whole.items()})
    dump = os.path.join(str(tmp_path), "dumped")
    r = validate(run8, ["--root", root, "--dump", dump], rc=2)
    assert verdict(r) == (True, 4, 8)
    assert re.findall(r"^Validation ERROR: ~\d+\. \S+/(g\d+\.fa) contents differ\.$", r.stdout, re.M) == names
    assert sorted(os.listdir(dump)) == names[:3]
    for f in names[:3]:
        assert open(os.path.join(dump, f), "rb").read() == whole[f]


def test_a_gzip_original_that_does_not_inflate_is_an_invalid_file(run8, tmp_path):
    root = str(tmp_path)
    damaged_copy(run8, root, {"g02.fa": None})
    packed = gzip.compress(open(os.path.join(run8, "g02.fa"), "rb").read())
    open(os.path.join(root, "g02.fa.gz"), "wb").write(packed[: len(packed) // 2])     # truncated
    r = validate(run8, ["--root", root], rc=2)
    assert verdict(r) == (True, 7, 8)
    assert "Cannot read %s for validation: Error decompressing gz file" % os.path.join(root, "g02.fa") in r.stderr
    open(os.path.join(root, "g02.fa.gz"), "wb").write(packed)
    assert verdict(validate(run8, ["--root", root])) == (False, 8, 8)


def test_at_most_100_invalid_files_are_logged(tmp_path):
    """VALIDATION_LOG_LIMIT = 100: 104 small files, every original gone, then every original damaged"""
    tmp = str(tmp_path)
    base = synth.base_codes(20_000, 9)
    names = ["s%03d.fa" % i for i in range(104)]
    for i, f in enumerate(names):
        open(os.path.join(tmp, f), "wb").write(synth.fasta_bytes(synth.genome(base, i, 0.01), i))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    tool(["c", "-R", "8", "list.txt", "out"], tmp)
    assert verdict(validate(tmp)) == (False, 104, 104)
    os.mkdir(os.path.join(tmp, "empty"))
    r = validate(tmp, ["--root", "empty"], rc=2)
    assert verdict(r) == (True, 0, 104) and r.stderr.count("Cannot find") == 100
    assert "errors in contents of 104 decoded files" in r.stderr
    os.mkdir(os.path.join(tmp, "bad"))
    for f in names:
        d = open(os.path.join(tmp, f), "rb").read()
        open(os.path.join(tmp, "bad", f), "wb").write(flip(d, len(d) - 2))
    r = validate(tmp, ["--root", "bad"], rc=2)
    assert verdict(r) == (True, 0, 104)
    assert r.stdout.count("contents differ.") == 100 and r.stdout.count("Error location:") == 100
    assert "s099.fa contents differ." in r.stdout and "s100.fa" not in r.stdout
