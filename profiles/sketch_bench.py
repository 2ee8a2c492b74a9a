"""mbgc_fasta_sketch_dev beside its yardstick (MEASUREMENTS §12): k_fa_sketch and k_fa_stats (counts only: the same tile walk, no
neighbour window, no rows) over the SAME records of the same device buffer, in one process, interleaved; then the sort behind the scan
and k_fa_sketch_pairs over all pairs of groups. Shapes: stats_bench.py's — the three Listeria genomes of tests/golden/listeria (their
62 records back to back, a group per genome), one range of 250 MB and 1000 ranges of 5 MB (a group per 100 ranges) of random ACGT with
a run of N every ~100 kB. k = 21; scale 1000 (the default) and, on the shapes of up to 300 MB, scale 1 (every position emits a row).
Per shape and scale one warm-up of each kernel, then five rounds; the medians. One JSON line per shape and scale.
    python profiles/sketch_bench.py [--scale 1.0] > profiles/sketch_bench.jsonl"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stats_bench import listeria, synthetic  # noqa: E402


def main():
    import torch
    from mbgc_amd import fasta
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    text, lens = listeria()
    per_file = np.repeat(np.arange(3), [19, 27, 16]) if lens.size == 62 else np.arange(lens.size) * 3 // lens.size
    shapes = [("listeria_62_records", text, lens, per_file),
              ("one_250MB",) + synthetic(np.array([int(250_000_000 * a.scale)], dtype=np.uint64)) + (np.zeros(1, dtype=np.uint32),),
              ("1000x5MB",) + synthetic(np.full(1000, int(5_000_000 * a.scale), dtype=np.uint64)) + (np.arange(1000) // 100,)]
    p = fasta.FastaParser()
    for name, text, lens, groups in shapes:
        dev = torch.from_numpy(text).to("cuda:0")
        torch.cuda.synchronize()
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        ranges = np.stack([off, lens], axis=1)
        ngroups = int(groups.max()) + 1
        for scale in (1000, 1):
            if scale == 1 and text.size > 300_000_000:                # (a row per base: 32 bytes of device memory each, and the hashes come down to the host)
                continue
            max_hash = (2 ** 64 - 1) // scale
            hashes, start, kmers, _ = p.sketch_dev(dev.data_ptr(), text.size, ranges, groups, ngroups, k=21, max_hash=max_hash)      # (warm-up; the row buffer grows here)
            cap = int(hashes.size)
            p.stats_dev(dev.data_ptr(), text.size, ranges, flags=1)
            if ngroups > 1:
                p.sketch_pairs_dev(hashes, start)
            ms = {"sketch": [], "sort": [], "stats_counts": [], "pairs": []}
            for _ in range(5):
                ms["sketch"].append(p.sketch_dev(dev.data_ptr(), text.size, ranges, groups, ngroups, k=21, max_hash=max_hash, cap=cap)[3])
                rows, reruns, sort_ms = p.last_sketch()
                ms["sort"].append(sort_ms)
                ms["stats_counts"].append(p.stats_dev(dev.data_ptr(), text.size, ranges, flags=1)[2])
                ms["pairs"].append(p.sketch_pairs_dev(hashes, start)[1] if ngroups > 1 else 0.0)
            line = {"shape": name, "bytes": int(text.size), "records": int(lens.size), "groups": ngroups, "k": 21, "scale": scale, "rows": rows, "row_reruns_timed": reruns,
                    "hashes": cap, "pairs": ngroups * (ngroups - 1) // 2}
            for k, v in ms.items():
                line[k + "_ms"] = round(float(np.median(v)), 4)
                line[k + "_ms_min"] = round(float(np.min(v)), 4)
            for k in ("sketch", "stats_counts"):
                line[k + "_gb_per_s"] = round(text.size / (float(np.median(ms[k])) * 1e-3) / 1e9, 1)
            line["sketch_over_stats"] = round(float(np.median(ms["sketch"])) / float(np.median(ms["stats_counts"])), 2)
            print(json.dumps(line), flush=True)
        del dev
    p.close()


if __name__ == "__main__":
    main()
