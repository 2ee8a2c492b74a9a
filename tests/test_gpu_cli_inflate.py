"""`mbgc-hip c --inflate device`: the gzip files of a list uploaded compressed and inflated in HBM. Every file `c` writes is
byte-identical to `c --inflate host` on the same list, and — but for the side file that holds the files' names — to `c` on the plain
files, in the sequential schedule and in rounds. A file of two members and a file whose CRC is wrong go the host's way: the first
compresses identically, the second ends the run with the message and the exit status of --inflate host. `v --inflate device` against
gzip originals: a good set, one altered original, one that does not inflate — the report of --inflate host, line for line."""
import gzip
import os
import re

import pytest

from test_gpu_decompress import tool, write_collection

pytestmark = pytest.mark.gpu
N = 6


def untimed(text):
    """the tool's output without the times it prints"""
    return re.sub(r"[\d.]+ (\[ms\]|ms\b)", "T", text)


def outputs(tmp, prefix):
    return {f[len(prefix):]: open(os.path.join(tmp, f), "rb").read() for f in sorted(os.listdir(tmp)) if f.startswith(prefix + ".")}


def gzip_copies(tmp, paths, make=None):
    """list_gz.txt: G0 plain, every other file as <path>.gz (make(i, data) -> the gzip bytes; default: one member, level 6)"""
    names = [paths[0]]
    for i, p in enumerate(paths[1:], 1):
        data = open(p, "rb").read()
        blob = make(i, data) if make else None
        open(p + ".gz", "wb").write(blob if blob is not None else gzip.compress(data, 6))
        names.append(p + ".gz")
    with open(os.path.join(tmp, "list_gz.txt"), "w") as f:
        f.write("\n".join(names) + "\n")


@pytest.mark.parametrize("args", [["-t1"], ["-R", "2"], ["-R", "3", "-m", "2"]], ids=" ".join)
def test_streams_are_those_of_the_host_path(tmp_path, args):
    tmp = str(tmp_path)
    paths = write_collection(tmp, N, 100_000)
    gzip_copies(tmp, paths)
    tool(["c"] + args + ["list.txt", "plain"], tmp)
    tool(["c"] + args + ["--inflate", "host", "list_gz.txt", "host"], tmp)
    r = tool(["c"] + args + ["--inflate", "device", "list_gz.txt", "dev"], tmp)
    plain, host, dev = outputs(tmp, "plain"), outputs(tmp, "host"), outputs(tmp, "dev")
    assert host and sorted(dev) == sorted(host) == sorted(plain)
    for ext in host:
        assert dev[ext] == host[ext], ext
        if ext != ".names":
            assert dev[ext] == plain[ext], ext
    assert "decompress" not in r.stderr


def test_two_members_and_a_mixed_list_go_through(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, N, 100_000)

    def make(i, data):
        if i == 2:                                                     # two members: ISIZE is the second one's length
            return gzip.compress(data[:len(data) // 3], 6) + gzip.compress(data[len(data) // 3:], 9)
        return None
    gzip_copies(tmp, paths, make)
    names = open(os.path.join(tmp, "list_gz.txt")).read().split()
    names[4] = paths[4]                                                # one plain file between gzip files
    open(os.path.join(tmp, "list_gz.txt"), "w").write("\n".join(names) + "\n")
    tool(["c", "-R", "3", "--inflate", "host", "list_gz.txt", "host"], tmp)
    tool(["c", "-R", "3", "--inflate", "device", "list_gz.txt", "dev"], tmp)
    host, dev = outputs(tmp, "host"), outputs(tmp, "dev")
    assert host and sorted(dev) == sorted(host)
    for ext in host:
        assert dev[ext] == host[ext], ext


def test_a_wrong_crc_ends_the_run_with_the_host_paths_message(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, N, 100_000)

    def make(i, data):
        if i == 3:
            blob = bytearray(gzip.compress(data, 6))
            blob[-6] ^= 0x10                                           # a bit of the CRC-32
            return bytes(blob)
        return None
    gzip_copies(tmp, paths, make)
    host = tool(["c", "-R", "3", "--inflate", "host", "list_gz.txt", "host"], tmp, ok=False)
    dev = tool(["c", "-R", "3", "--inflate", "device", "list_gz.txt", "dev"], tmp, ok=False)
    assert host.returncode == 1 and host.stderr == "Error decompressing gz file: -3.\n", (host.returncode, host.stderr)
    assert (dev.returncode, dev.stdout, dev.stderr) == (host.returncode, host.stdout, host.stderr)


def test_gzip_g0_empty_gzip_file_and_an_all_plain_round(tmp_path):
    """G0 as a gzip file (inflated by the host under either switch), a gzip file of no bytes (ISIZE 0) and, with -R 2, a round whose
    files are all plain: whatever --inflate host does with the list, --inflate device does"""
    tmp = str(tmp_path)
    paths = write_collection(tmp, 8, 100_000)
    gzip_copies(tmp, paths)
    names = open(os.path.join(tmp, "list_gz.txt")).read().split()
    open(paths[0] + ".gz", "wb").write(gzip.compress(open(paths[0], "rb").read(), 6))
    names[0] = paths[0] + ".gz"
    names[3], names[4] = paths[3], paths[4]                              # -R 2: targets 3 and 4 are a round of their own
    for with_empty in (False, True):
        if with_empty:
            open(os.path.join(tmp, "empty.fna.gz"), "wb").write(gzip.compress(b""))
            names.append(os.path.join(tmp, "empty.fna.gz"))
        open(os.path.join(tmp, "list_gz.txt"), "w").write("\n".join(names) + "\n")
        host = tool(["c", "-R", "2", "--inflate", "host", "list_gz.txt", "host"], tmp, ok=False)
        dev = tool(["c", "-R", "2", "--inflate", "device", "list_gz.txt", "dev"], tmp, ok=False)
        assert (dev.returncode, untimed(dev.stderr)) == (host.returncode, untimed(host.stderr))
        assert host.returncode == 0 or with_empty
        assert outputs(tmp, "dev") == outputs(tmp, "host")


# ---- mbgc-hip v
def v_lines(r):
    return (r.returncode, untimed(r.stdout).splitlines(), untimed(r.stderr).splitlines())


@pytest.fixture(scope="module")
def gz_set(tmp_path_factory):
    """a stream set of six files whose originals (but G0's) exist as <path>.gz only"""
    tmp = str(tmp_path_factory.mktemp("vgz"))
    paths = write_collection(tmp, N, 100_000)
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    for p in paths[1:]:
        open(p + ".gz", "wb").write(gzip.compress(open(p, "rb").read(), 6))
        os.remove(p)
    return tmp, paths


@pytest.mark.parametrize("extra", [[], ["--batch-kib", "150"]], ids=["one batch", "several batches"])
def test_v_good_set(gz_set, extra):
    tmp, paths = gz_set
    host = tool(["v", "--inflate", "host"] + extra + ["out"], tmp, ok=False)
    dev = tool(["v", "--inflate", "device", "--bench"] + extra + ["out"], tmp, ok=False)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    assert "Validation: correctly decoded %d out of %d files." % (N, N) in dev.stdout
    assert host.stdout.splitlines()[-1] in dev.stdout.splitlines()
    assert '"inflated_on_device": %d, "inflated_again_on_host": 0' % (N - 1) in dev.stdout              # (--bench: the counts of the timed pass)


def test_v_one_altered_original_and_one_that_does_not_inflate(gz_set, tmp_path):
    tmp, paths = gz_set
    keep = {p: open(p + ".gz", "rb").read() for p in (paths[2], paths[3], paths[4])}
    try:
        text = bytearray(gzip.decompress(keep[paths[2]]))
        at = len(text) // 2
        while text[at] not in b"ACGT":
            at += 1
        text[at] = ord("A") if text[at] != ord("A") else ord("C")           # one base, the size stays
        open(paths[2] + ".gz", "wb").write(gzip.compress(bytes(text), 6))
        longer = gzip.decompress(keep[paths[4]]) + b"ACGT\n"                # another size: its trailer says so
        open(paths[4] + ".gz", "wb").write(gzip.compress(longer, 6))
        host, dev = (tool(["v", "--inflate", how, "out"], tmp, ok=False) for how in ("host", "device"))
        assert host.returncode == 2 and v_lines(dev) == v_lines(host)
        assert "contents differ" in host.stdout and "size differ" in host.stdout
        assert "Validation ERROR: correctly decoded %d out of %d files." % (N - 2, N) in dev.stdout
        broken = bytearray(keep[paths[3]])
        broken[len(broken) // 2] ^= 0x40                                    # does not inflate (or not to its CRC)
        open(paths[3] + ".gz", "wb").write(bytes(broken))
        host, dev = (tool(["v", "--inflate", how, "out"], tmp, ok=False) for how in ("host", "device"))
        assert host.returncode == 2 and v_lines(dev) == v_lines(host)
        assert any(l.startswith("Cannot read %s for validation: Error decompressing gz file: " % paths[3]) for l in dev.stderr.splitlines()), dev.stderr
    finally:
        for p, blob in keep.items():
            open(p + ".gz", "wb").write(blob)


def test_v_switch_takes_two_words(tmp_path):
    r = tool(["v", "--inflate", "gpu", "out"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "--inflate takes host or device" in r.stderr


def test_the_switch_takes_two_words(tmp_path):
    tmp = str(tmp_path)
    r = tool(["c", "--inflate", "gpu", "list.txt", "out"], tmp, ok=False)                 # (refused before the list is opened)
    assert r.returncode != 0 and "--inflate takes host or device" in r.stderr
