"""mbgc_fasta_dups_dev beside its yardstick (MEASUREMENTS §13): k_fa_dups and k_fa_stats (counts only — the same tile walk, no
arithmetic) over the SAME records of one device buffer, in one process, interleaved; and the share of the exactness step
(k_fa_dups_verify, from mbgc_fasta_dups_last). Shapes: few long records (40 of 5 MB, every fourth a copy or a reverse complement of
the one before it) and many short ones (200 000 of 1 kB, the same planting). Random ACGT. Per shape one warm-up of each arm, then five
rounds; the medians. One JSON line per shape.
    python profiles/dups_bench.py [--scale 1.0] > profiles/dups_bench.jsonl"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COMP = np.arange(256, dtype=np.uint8)
for a, b in (b"AT", b"CG"):
    COMP[a], COMP[b] = b, a


def planted(nrec, ln):
    rng = np.random.default_rng(3)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, nrec * ln, dtype=np.uint8)].reshape(nrec, ln)
    for r in range(3, nrec, 4):
        text[r] = text[r - 1] if r % 8 == 3 else COMP[text[r - 1][::-1]]
    return text.reshape(-1), np.full(nrec, ln, dtype=np.uint64)


def main():
    import torch
    from mbgc_amd import fasta
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    shapes = [("40x5MB",) + planted(40, int(5_000_000 * a.scale)), ("200000x1kB",) + planted(int(200_000 * a.scale), 1000)]
    p = fasta.FastaParser()
    for name, text, lens in shapes:
        dev = torch.from_numpy(text).to("cuda:0")
        torch.cuda.synchronize()
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        ranges = np.stack([off, lens], axis=1)
        last = {}

        def dups():
            out, classes, ms = p.dups_dev(dev.data_ptr(), text.size, ranges)
            last["classes"], last["last"] = classes, p.last_dups()
            return ms
        arms = {"dups": dups, "stats_counts": lambda: p.stats_dev(dev.data_ptr(), text.size, ranges, flags=1)[2]}
        for f in arms.values():
            f()
        ms, verify = {k: [] for k in arms}, []
        for _ in range(5):
            for k, f in arms.items():
                ms[k].append(f())
            verify.append(last["last"][3])
        line = {"shape": name, "bytes": int(text.size), "records": int(lens.size), "classes": last["classes"], "buckets": last["last"][0], "verified": last["last"][1],
                "refuted": last["last"][2], "verify_ms": round(float(np.median(verify)), 4)}
        for k, v in ms.items():
            line[k + "_ms"] = round(float(np.median(v)), 4)
            line[k + "_ms_min"] = round(float(np.min(v)), 4)
            line[k + "_gb_per_s"] = round(text.size / (float(np.median(v)) * 1e-3) / 1e9, 1)
        line["dups_over_stats"] = round(line["dups_ms"] / line["stats_counts_ms"], 2)
        line["verify_share"] = round(line["verify_ms"] / (line["verify_ms"] + line["dups_ms"]), 3)
        print(json.dumps(line), flush=True)
        del dev
    p.close()


if __name__ == "__main__":
    main()
