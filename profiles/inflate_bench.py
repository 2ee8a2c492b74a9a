"""gzip input end to end (MEASUREMENTS §8): N synthetic 5 Mbp genomes (BASELINE configs[2]'s generator, 99 % identity) written once as
gzip level 6, then `mbgc-hip c` three times in every configuration — a tool of another build given with --parent (no --inflate switch),
--inflate host, --inflate device — and `mbgc-hip v --bench` against the gzip originals with either switch. One JSON line per run: wall
time and what MBGC_HIP_TIMES=1 / v --bench print.
    python profiles/inflate_bench.py [--files 200] [--parent path/to/mbgc-hip] [--dir scratch]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mbgc_amd import synth  # noqa: E402

TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")


def _write(job):
    path, data = job
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "wb") as f:
        f.write(c.compress(data) + c.flush())
    return len(data)


def run(tool, args, cwd, tag):
    env = dict(os.environ, MBGC_HIP_TIMES="1")
    t0 = time.perf_counter()
    r = subprocess.run([tool] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    out = {"run": tag, "cmd": " ".join(["mbgc-hip"] + args), "rc": r.returncode, "wall_s": round(wall, 3)}
    text = r.stderr + r.stdout
    for key, pat in (("reading_files_ms", r"reading files (\d+) ms"), ("waiting_for_readers_ms", r"waiting for them (\d+) ms"), ("upload_parse_ms", r"upload \+ parse (\d+) ms"),
                     ("inflate_kernel_ms", r"inflate kernel ran (\d+) ms"), ("main_waiting_for_input_ms", r"main thread: waiting for it (\d+) ms")):
        m = re.search(pat, text)
        if m:
            out[key] = int(m.group(1))
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            out.update({k: j[k] for k in ("upload_ms", "read_inflate_ms", "compare_kernel_ms", "inflate_kernel_ms", "inflated_on_device", "inflated_again_on_host", "valid", "files") if k in j})
    print(json.dumps(out), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    tmp = a.dir or tempfile.mkdtemp(prefix="inflate_bench_")
    os.makedirs(tmp, exist_ok=True)
    base = synth.base_codes(5_000_000)
    ids = list(range(a.files))
    t0 = time.perf_counter()
    jobs, paths, text_bytes = [], [], 0
    with Pool(16) as pool:
        pending = []
        for i, g in zip(ids, synth.genomes(base, ids)):
            p = os.path.join(tmp, "g%04d.fna.gz" % i)
            paths.append(p)
            pending.append(pool.apply_async(_write, ((p, synth.fasta_bytes(g, i)),)))
        text_bytes = sum(x.get() for x in pending)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    gz_bytes = sum(os.path.getsize(p) for p in paths)
    print(json.dumps({"files": a.files, "text_bytes": text_bytes, "gz_bytes": gz_bytes, "generated_in_s": round(time.perf_counter() - t0, 1)}), flush=True)
    configs = ([("parent", os.path.abspath(a.parent), [])] if a.parent else []) + [("host", TOOL, ["--inflate", "host"]), ("device", TOOL, ["--inflate", "device"])]
    for rep in range(a.repeats):
        for tag, tool, extra in configs:
            r = run(tool, ["c"] + extra + ["list.txt", "out_" + tag], tmp, "c %s #%d" % (tag, rep))
            if r.returncode:
                sys.exit("c %s failed: %s" % (tag, r.stderr[-500:]))
    same = all(open(os.path.join(tmp, f), "rb").read() == open(os.path.join(tmp, "out_device" + f[len("out_host"):]), "rb").read()
               for f in os.listdir(tmp) if f.startswith("out_host."))
    print(json.dumps({"device_streams_identical_to_host": same}), flush=True)
    for rep in range(a.repeats):
        for how in ("host", "device"):
            run(TOOL, ["v", "--bench", "--inflate", how, "out_host"], tmp, "v %s #%d" % (how, rep))


if __name__ == "__main__":
    main()
