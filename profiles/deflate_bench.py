"""gzip output end to end (MEASUREMENTS §3i): N synthetic 5 Mbp genomes (the collection of §3b: BASELINE configs[2]'s generator, 99 %
identity) compressed once with `mbgc-hip c`, then three runs each of
  (a) `mbgc-hip d --fasta dir --gzip --bench`                      the files compressed on the device
  (b) `d --fasta dir`, then zlib level 1 over the written files    what a user does without --gzip, at the cheapest setting
  (c) the same with level 6
(b) and (c) run zlib on a pool of 16 threads (zlib releases the GIL); --parent names the tool of (b) and (c) when it is another build.
One JSON line per run: wall seconds, the .gz bytes, and what --bench prints.
    python profiles/deflate_bench.py [--files 129] [--parent path/to/mbgc-hip] [--dir scratch]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mbgc_amd import synth  # noqa: E402

TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")


def gzip_file(job):
    path, level = job
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    data = open(path, "rb").read()
    blob = c.compress(data) + c.flush()
    with open(path + ".gz", "wb") as f:
        f.write(blob)
    os.remove(path)
    return len(blob)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=129)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    tmp = a.dir or tempfile.mkdtemp(prefix="deflate_bench_")
    os.makedirs(tmp, exist_ok=True)
    base = synth.base_codes(5_000_000)
    ids = list(range(a.files))
    paths = []
    for i, g in zip(ids, synth.genomes(base, ids)):
        p = os.path.join(tmp, "g%04d.fna" % i)
        open(p, "wb").write(synth.fasta_bytes(g, i))
        paths.append(p)
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(paths) + "\n")
    subprocess.run([TOOL, "c", "list.txt", "out"], cwd=tmp, check=True, capture_output=True, timeout=1800)
    plain_tool = os.path.abspath(a.parent) if a.parent else TOOL
    for rep in range(a.repeats):
        for tag, level in (("a device", None), ("b zlib 1", 1), ("c zlib 6", 6)):
            d = os.path.join(tmp, "fa")
            shutil.rmtree(d, ignore_errors=True)
            t0 = time.perf_counter()
            if level is None:
                r = subprocess.run([TOOL, "d", "--fasta", "fa", "--gzip", "--bench", "out", "b"], cwd=tmp, capture_output=True, text=True, timeout=1800)
            else:
                r = subprocess.run([plain_tool, "d", "--fasta", "fa", "out", "b"], cwd=tmp, capture_output=True, text=True, timeout=1800)
                if r.returncode == 0:
                    with ThreadPoolExecutor(16) as pool:
                        list(pool.map(gzip_file, [(os.path.join(d, f), level) for f in os.listdir(d)]))
            wall = time.perf_counter() - t0
            out = {"run": "%s #%d" % (tag, rep), "rc": r.returncode, "wall_s": round(wall, 3),
                   "gz_bytes": sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".gz")) if os.path.isdir(d) else 0}
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    j = json.loads(line)
                    out.update({k: j[k] for k in ("text_bytes", "format_kernel_ms", "deflate_kernel_ms", "download_ms", "write_ms", "chunks", "stored_chunks") if k in j})
            print(json.dumps(out), flush=True)
            if r.returncode:
                sys.exit("%s failed: %s" % (tag, r.stderr[-500:]))


if __name__ == "__main__":
    main()
