"""Per-range CRC-32 on the device (MEASUREMENTS: the section on mbgc_fasta_crc_dev): the kernel's rate on three shapes — one 250 MB
range, 1000 ranges of 5 MB, 2 000 000 ranges of 20-2000 bytes — with the table lookup in use (the 1 KiB byte table)
and with nibble tables, one copy per LDS bank (MBGC_HIP_CRC_LOOKUP=nibble; the switch is read once per process, so every lookup runs in a child of its
own), beside what the kernel replaces: mbgc_fasta_download of the same bytes and zlib.crc32 over them on 16 host threads. Then what
--check adds to `mbgc-hip d --bench` on a synthetic collection. One JSON line per measurement.
    python profiles/crc_bench.py [--scale 1.0] [--files 12] > profiles/crc_bench.jsonl"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
HOST_THREADS = 16


def shapes(scale):
    import numpy as np
    rng = np.random.default_rng(1)
    small = rng.integers(20, 2001, int(2_000_000 * scale)).astype(np.uint64)
    return [("one_250MB", np.array([int(250_000_000 * scale)], dtype=np.uint64)),
            ("1000x5MB", np.full(1000, int(5_000_000 * scale), dtype=np.uint64)),
            ("2M_20_2000B", small)]


def kernel_child(scale):
    """the three shapes with the lookup the environment names; the host alternative once (it does not depend on the lookup)"""
    import numpy as np
    import torch
    from mbgc_amd import binding, fasta
    p = fasta.FastaParser()
    L = binding.lib()
    lookup = os.environ.get("MBGC_HIP_CRC_LOOKUP", "byte")
    for name, lens in shapes(scale):
        total = int(lens.sum())
        buf = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        ranges = np.stack([off, lens], axis=1)
        ms = []
        for _ in range(6):
            got, t = p.crc_dev(buf.data_ptr(), total, ranges)
            ms.append(t)
        best = min(ms[1:])
        row = {"shape": name, "lookup": lookup, "ranges": int(lens.size), "bytes": total, "crc_kernel_ms": round(best, 3),
               "crc_kernel_ms_all": [round(x, 3) for x in ms], "crc_gb_per_s": round(total / (best * 1e-3) / 1e9, 2)}
        if lookup == "byte":
            host = np.empty(total, dtype=np.uint8)
            t0 = time.perf_counter()
            rc = L.mbgc_fasta_download(p.h, C.c_void_p(host.ctypes.data), C.c_void_p(buf.data_ptr()), C.c_uint64(total))
            t1 = time.perf_counter()
            assert rc == 0
            view = memoryview(host)
            ends = (off + lens).astype(np.int64)
            starts = off.astype(np.int64)
            parts = np.array_split(np.arange(lens.size), HOST_THREADS) if lens.size >= HOST_THREADS else [np.arange(lens.size)]

            def work(idx):
                return [zlib.crc32(view[starts[k]:ends[k]]) for k in idx]
            if lens.size == 1:                                       # one range: 16 slices, joined with crc32_combine
                cut = np.linspace(0, total, HOST_THREADS + 1).astype(np.int64)
                with ThreadPoolExecutor(HOST_THREADS) as ex:
                    crcs = list(ex.map(lambda i: zlib.crc32(view[cut[i]:cut[i + 1]]), range(HOST_THREADS)))
                acc = crcs[0]
                for i in range(1, HOST_THREADS):
                    acc = fasta.crc_combine(acc, crcs[i], int(cut[i + 1] - cut[i]))
                want = [acc]
            else:
                with ThreadPoolExecutor(HOST_THREADS) as ex:
                    want = sum(ex.map(work, parts), [])
            t2 = time.perf_counter()
            assert [int(x) for x in got] == want, "the device's CRCs differ from zlib's"
            row.update({"download_ms": round((t1 - t0) * 1e3, 1), "zlib_16_threads_ms": round((t2 - t1) * 1e3, 1),
                        "host_gb_per_s": round(total / (t2 - t0) / 1e9, 2)})
        print(json.dumps(row), flush=True)
        del buf
        torch.cuda.empty_cache()
    p.close()


def check_cost(files, tmp):
    import numpy as np
    from mbgc_amd import synth
    base = synth.base_codes(2_000_000, 7)
    paths = []
    for i in range(files):
        path = os.path.join(tmp, "g%02d.fa" % i)
        with open(path, "wb") as f:
            f.write(synth.fasta_bytes(synth.genome(base, i, 0.01), i))
        paths.append(path)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    subprocess.run([TOOL, "c", "--checksums", "list.txt", "out"], cwd=tmp, check=True, capture_output=True, timeout=600)
    for tag, args in (("d --bench", ["d", "--bench", "out", "back"]), ("d --check --bench", ["d", "--check", "--bench", "out", "back"]), ("t --bench", ["t", "--bench", "out"])):
        r = subprocess.run([TOOL] + args, cwd=tmp, capture_output=True, text=True, timeout=600)
        row = {"run": tag, "rc": r.returncode}
        for line in r.stdout.splitlines():
            if line.startswith("{") and "decompress" in line:
                j = json.loads(line)
                row["decode_ms"] = round(j["plan_ms"] + j["fill_ms"] + j["load_ms"], 3)
                row.update({k: j[k] for k in ("bases", "plan_ms", "fill_ms", "load_ms", "crc_kernel_ms", "crc_bytes", "crc_gb_per_s") if k in j})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        kernel_child(a.scale)
        return
    for lookup in ("byte", "nibble"):
        env = dict(os.environ, MBGC_HIP_CRC_LOOKUP=lookup)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scale", str(a.scale)], env=env, check=True, timeout=900)
    with tempfile.TemporaryDirectory() as tmp:
        check_cost(a.files, tmp)


if __name__ == "__main__":
    main()
