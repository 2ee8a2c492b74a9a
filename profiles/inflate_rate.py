"""k_fa_inflate's rate: N copies of one gzip stream (5 MB of FASTA text, level 6) in one call, the kernel's ms from events"""
import json, sys, time, zlib
import numpy as np
import torch
sys.path.insert(0, ".")
from mbgc_amd import fasta

rng = np.random.default_rng(1)
base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 5_000_000)
lines = base.reshape(-1, 80)
text = b">genome\n" + b"".join(l.tobytes() + b"\n" for l in lines)
c = zlib.compressobj(6, zlib.DEFLATED, 31)
gz = c.compress(text) + c.flush()
t0 = time.perf_counter(); zlib.decompress(gz, 31); host_ms = (time.perf_counter() - t0) * 1e3
print(json.dumps({"text_bytes": len(text), "gz_bytes": len(gz), "zlib_one_thread_ms": round(host_ms, 2)}), flush=True)
p = fasta.FastaParser()
for n in (1, 8, 31, 64, 256, 1024):
    g = np.frombuffer(gz, dtype=np.uint8)
    pad = (-len(gz)) % 16
    one = np.concatenate([g, np.zeros(pad, dtype=np.uint8)])
    gz_dev = torch.from_numpy(np.tile(one, n)).to("cuda:0")
    cap = len(text) + (-len(text)) % 16
    out_dev = torch.zeros(cap * n, dtype=torch.uint8, device="cuda:0")
    jobs = [(k * one.size, len(gz), k * cap, len(text)) for k in range(n)]
    torch.cuda.synchronize()
    runs = []
    for rep in range(3):
        res, ms = p.inflate_dev(gz_dev.data_ptr(), gz_dev.numel(), out_dev.data_ptr(), out_dev.numel(), jobs)
        assert all(r[0] == 0 and r[2] == len(text) for r in res), res[:3]
        runs.append(round(ms, 2))
    assert out_dev[(n - 1) * cap:(n - 1) * cap + len(text)].cpu().numpy().tobytes() == text
    print(json.dumps({"jobs": n, "kernel_ms": runs, "text_GB_per_s": round(n * len(text) / min(runs) / 1e6, 3), "MB_per_s_per_wave": round(len(text) / min(runs) / 1e3, 1)}), flush=True)
    del gz_dev, out_dev
p.close()
