"""mbgc_fasta_stats_dev beside its yardstick (MEASUREMENTS §11): k_fa_stats and k_fa_crc over the SAME records of the same device
buffer, in one process, interleaved — the CRC reads every byte once and writes a word per record, which is what a streaming read of
the records costs here. Shapes: the three Listeria genomes of tests/golden/listeria (their 62 records back to back), crc_bench.py's
one range of 250 MB and its 1000 ranges of 5 MB. The synthetic text is random ACGT with a run of N and a lower-case stretch every
~100 kB. Per shape one warm-up of each kernel, then five rounds; the medians. One JSON line per shape.
    python profiles/stats_bench.py [--scale 1.0] > profiles/stats_bench.jsonl"""
import argparse
import json
import lzma
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIST = os.path.join(ROOT, "tests", "golden", "listeria")


def listeria():
    seqs = []
    for f in sorted(os.listdir(LIST)):
        if f.endswith(".xz"):
            for block in lzma.open(os.path.join(LIST, f)).read().split(b">")[1:]:
                seqs.append(block.partition(b"\n")[2].replace(b"\n", b""))
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), np.array([len(s) for s in seqs], dtype=np.uint64)


def synthetic(lens):
    rng = np.random.default_rng(2)
    n = int(lens.sum())
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for at in range(50_000, n - 2000, 100_000):
        text[at:at + 500] = ord("N")
        text[at + 1000:at + 1700] |= 0x20
    return text, lens


def main():
    import torch
    from mbgc_amd import fasta
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    shapes = [("listeria_62_records",) + listeria(),
              ("one_250MB",) + synthetic(np.array([int(250_000_000 * a.scale)], dtype=np.uint64)),
              ("1000x5MB",) + synthetic(np.full(1000, int(5_000_000 * a.scale), dtype=np.uint64))]
    p = fasta.FastaParser()
    for name, text, lens in shapes:
        dev = torch.from_numpy(text).to("cuda:0")
        torch.cuda.synchronize()
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        ranges = np.stack([off, lens], axis=1)
        arms = {"stats_counts_nruns": lambda: p.stats_dev(dev.data_ptr(), text.size, ranges, flags=3)[2],
                "stats_all": lambda: p.stats_dev(dev.data_ptr(), text.size, ranges, flags=7)[2],
                "stats_runs_only": lambda: p.stats_dev(dev.data_ptr(), text.size, ranges, flags=6)[2],
                "crc": lambda: p.crc_dev(dev.data_ptr(), text.size, ranges)[1]}
        for f in arms.values():
            f()
        edges = p.last_stats()                                       # (of the warm-up's last stats call: runs only, both classes)
        ms = {k: [] for k in arms}
        for _ in range(5):
            for k, f in arms.items():
                ms[k].append(f())
        line = {"shape": name, "bytes": int(text.size), "records": int(lens.size), "edges_both_classes": edges[0], "edge_reruns_warmup": edges[1]}
        for k, v in ms.items():
            line[k + "_ms"] = round(float(np.median(v)), 4)
            line[k + "_ms_min"] = round(float(np.min(v)), 4)
            line[k + "_gb_per_s"] = round(text.size / (float(np.median(v)) * 1e-3) / 1e9, 1)
        print(json.dumps(line), flush=True)
        del dev
    p.close()


if __name__ == "__main__":
    main()
