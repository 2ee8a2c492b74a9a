"""mbgc_fasta_screen_dev beside its yardstick (MEASUREMENTS §15): k_fa_screen and k_fa_sketch at scale 1000 over the SAME records of the
same device buffer, in one process, interleaved — both read the same text and form the same canonical k-mers; one asks `hash <=
maxHash`, the other asks a filter in LDS and a table in global memory. Shapes: dups_bench.py's, 40 records of 5 MB and 200 000 records
of 1 kB, 40 groups each. The text is a collection of related genomes — every 5 MB a copy of one random base genome with 1 % of its
bases substituted — so that a whole genome as the query hits most positions of every other one. Key sets, k = 21: one gene (1 500 bases
of the first genome), 2 000 genes (that one and 1 999 random kilobases: about 2 M keys, nearly all of them k-mers of nothing), and the
whole first genome. Per shape and key set one warm-up of each kernel (the row buffer grows there), then five rounds; the medians. The
hit rows are not asked for: the found lists alone. One JSON line per shape and key set.
    python profiles/screen_bench.py [--scale 1.0] > profiles/screen_bench.jsonl"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _screen  # noqa: E402  (the keys of a query: canonical 2-bit words)

K = 21


def collection(genomes, length):
    rng = np.random.default_rng(3)
    base = rng.integers(0, 4, length, dtype=np.uint8)
    out = np.empty(genomes * length, dtype=np.uint8)
    for g in range(genomes):
        codes = base.copy()
        if g:
            at = rng.integers(0, length, length // 100)
            codes[at] = (codes[at] + rng.integers(1, 4, at.size, dtype=np.uint8)) & 3
        out[g * length:(g + 1) * length] = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return out


def main():
    import torch
    from mbgc_amd import fasta
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    length = int(5_000_000 * a.scale)
    text = collection(40, length)
    rng = np.random.default_rng(4)
    gene = text[length // 2:length // 2 + 1500].tobytes()
    genes = [gene] + [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1000)].tobytes() for _ in range(1999)]
    key_sets = [("one_gene", _screen.key_set([gene], K)[0]), ("2000_genes", _screen.key_set(genes, K)[0]), ("whole_genome", _screen.key_set([text[:length].tobytes()], K)[0])]
    dev = torch.from_numpy(text).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    max_hash = (2 ** 64 - 1) // 1000
    for name, lens in (("40x5MB", np.full(40, length, dtype=np.uint64)), ("200000x1kB", np.full(text.size // 1000, 1000, dtype=np.uint64))):
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        ranges = np.stack([off, lens], axis=1)
        groups = (np.arange(lens.size) * 40 // lens.size).astype(np.uint32)
        hashes = p.sketch_dev(dev.data_ptr(), text.size, ranges, groups, 40, k=K, max_hash=max_hash)[0]      # (warm-up)
        for label, keys in key_sets:
            found = p.screen_dev(dev.data_ptr(), text.size, ranges, groups, 40, keys, k=K)[0]                # (warm-up; the row buffer grows here)
            ms = {"screen": [], "screen_sort": [], "sketch": []}
            for _ in range(5):
                ms["screen"].append(p.screen_dev(dev.data_ptr(), text.size, ranges, groups, 40, keys, k=K, found_cap=int(found.size))[3])
                rows, passes, reruns, sort_ms = p.last_screen()
                ms["screen_sort"].append(sort_ms)
                ms["sketch"].append(p.sketch_dev(dev.data_ptr(), text.size, ranges, groups, 40, k=K, max_hash=max_hash, cap=int(hashes.size))[3])
            positions = int(np.maximum(lens.astype(np.int64) - K + 1, 0).sum())
            slots = 2
            while slots < 2 * keys.size:
                slots *= 2
            line = {"shape": name, "bytes": int(text.size), "records": int(lens.size), "groups": 40, "k": K, "key_set": label, "keys": int(keys.size), "table_slots": slots,
                    "positions": positions, "filter_passes": passes, "filter_passes_per_position": round(passes / positions, 4), "rows": rows, "row_reruns_timed": reruns,
                    "found": int(found.size)}
            for k, v in ms.items():
                line[k + "_ms"] = round(float(np.median(v)), 4)
                line[k + "_ms_min"] = round(float(np.min(v)), 4)
            for k in ("screen", "sketch"):
                line[k + "_gb_per_s"] = round(text.size / (float(np.median(ms[k])) * 1e-3) / 1e9, 1)
            line["screen_over_sketch"] = round(float(np.median(ms["screen"])) / float(np.median(ms["sketch"])), 2)
            print(json.dumps(line), flush=True)
    p.close()


if __name__ == "__main__":
    main()
