"""Regenerates tests/golden/listeria/expected_lossy_single.json: the three bundled Listeria genomes, each written again in a
damaged style of its own (CRLF, ragged lines with empty ones, '@' headers) and concatenated behind a leading comment
(tests/_singlefasta_lossy.damaged_listeria), through the reference CLI's lossy single fasta file mode under the sequential schedule
(`mbgc-dev c -L -t1 -i`, deterministic) and its developer build's `v -D`. Format and stream order: make_single_fasta_golden.py.

    python tests/golden/make_single_fasta_lossy_golden.py        (needs oracle/_ref/mbgc-dev)"""
import hashlib
import json
import lzma
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _singlefasta_lossy as sfl  # noqa: E402

LIST = os.path.join(HERE, "listeria")
DEV = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "mbgc-dev")
FILES = ["GCA_000585755.1_Lm1823_genomic.fna", "GCA_000585775.1_Lm1824_genomic.fna", "GCA_000585795.1_Lm1840_genomic.fna"]
ORDER = ["literals", "locksPos", "gapDelta", "flags", "mapOff", "mapLen"]


def damaged():
    return sfl.damaged_listeria([lzma.open(os.path.join(LIST, f + ".xz")).read() for f in FILES])


def reference_streams(workdir):
    data = damaged()
    path = os.path.join(workdir, "all.fna")
    with open(path, "wb") as f:
        f.write(data)
    arc = os.path.join(workdir, "lossy.mbgc")
    subprocess.run([DEV, "c", "-L", "-t1", "-i", path, arc], check=True, capture_output=True)
    subprocess.run([DEV, "v", "-t1", "-D", arc], check=True, capture_output=True, cwd=workdir)
    dump = lambda i: "%s_dump_%02d" % (arc, i)
    names = [i for i in range(1, 30) if os.path.exists(dump(i)) and open(dump(i), "rb").read() == b"all.fna\xbb"]
    assert len(names) == 1
    out = {}
    for i, name in enumerate(ORDER):
        b = open(dump(names[0] + 6 + i), "rb").read()
        out[name] = {"bytes": len(b), "md5": hashlib.md5(b).hexdigest()}
    assert not os.path.exists(dump(names[0] + 6 + len(ORDER)))
    counts = open(dump(names[0] + 1), "rb").read()
    lines = open(dump(names[0] + 4), "rb").read()
    return dict(command="mbgc-dev c -L -t1 -i all.fna x.mbgc && mbgc-dev v -t1 -D x.mbgc  (all.fna: _singlefasta_lossy.damaged_listeria of the files below)",
                files=FILES, input_bytes=len(data), input_md5=hashlib.md5(data).hexdigest(),
                sequence_counts=list(struct.unpack("<%dI" % (len(counts) // 4), counts)),
                dna_line_lengths=list(struct.unpack("<%dQ" % (len(lines) // 8), lines)), streams=out)


if __name__ == "__main__":
    if not os.path.exists(DEV):
        sys.exit("oracle/_ref/mbgc-dev is not built")
    with tempfile.TemporaryDirectory() as d:
        res = reference_streams(d)
    with open(os.path.join(LIST, "expected_lossy_single.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print({k: v["bytes"] for k, v in res["streams"].items()}, res["sequence_counts"], res["dna_line_lengths"])
