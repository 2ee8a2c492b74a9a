"""Regenerates tests/golden/listeria/expected_t1_single.json and expected_m3_single.json: the three bundled Listeria genomes
concatenated into ONE multi-FASTA file, through the reference CLI's single fasta file mode (`mbgc-dev c -t1 -i` / `-m 3 -t1 -i`,
both deterministic) and its developer build's `v -D`, which dumps the raw streams in the order of MBGC_Decoder.cpp:1085-1112.
A single-file archive is written without lazy decompression support (MBGC_Encoder.cpp:462-466): there is no refExtSize stream.

    python tests/golden/make_single_fasta_golden.py        (needs oracle/_ref/mbgc-dev)"""
import hashlib
import json
import lzma
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LIST = os.path.join(HERE, "listeria")
DEV = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "mbgc-dev")
FILES = ["GCA_000585755.1_Lm1823_genomic.fna", "GCA_000585775.1_Lm1824_genomic.fna", "GCA_000585795.1_Lm1840_genomic.fna"]
ORDER = {"t1": ["literals", "locksPos", "gapDelta", "flags", "mapOff", "mapLen"],
         "m3": ["literals", "rcMapOff", "rcMapLen", "locksPos", "gapDelta", "flags", "mapOff", "mapLen"]}
ARGS = {"t1": ["-t1"], "m3": ["-m", "3", "-t1"]}


def concatenated():
    return b"".join(lzma.open(os.path.join(LIST, f + ".xz")).read() for f in FILES)


def reference_streams(kind, workdir):
    path = os.path.join(workdir, "all.fna")
    with open(path, "wb") as f:
        f.write(concatenated())
    arc = os.path.join(workdir, kind + ".mbgc")
    subprocess.run([DEV, "c"] + ARGS[kind] + ["-i", path, arc], check=True, capture_output=True)
    subprocess.run([DEV, "v", "-t1", "-D", arc], check=True, capture_output=True, cwd=workdir)
    # the dumps are numbered as the coders meet them: the collective section starts with the names stream (here the file's name
    # and a separator), then sequence counts, header templates, headers, line lengths, factors, and the streams of ORDER
    dump = lambda i: "%s_dump_%02d" % (arc, i)
    names = [i for i in range(1, 30) if os.path.exists(dump(i)) and open(dump(i), "rb").read() == b"all.fna\xbb"]
    assert len(names) == 1
    out = {}
    for i, name in enumerate(ORDER[kind]):
        b = open(dump(names[0] + 6 + i), "rb").read()
        out[name] = {"bytes": len(b), "md5": hashlib.md5(b).hexdigest()}
    assert not os.path.exists(dump(names[0] + 6 + len(ORDER[kind])))
    counts = open(dump(names[0] + 1), "rb").read()
    return dict(command="mbgc-dev c %s -i all.fna x.mbgc && mbgc-dev v -t1 -D x.mbgc  (all.fna: the files below, concatenated)" % " ".join(ARGS[kind]),
                files=FILES, input_bytes=len(concatenated()), sequence_counts=list(struct.unpack("<%dI" % (len(counts) // 4), counts)), streams=out)


if __name__ == "__main__":
    if not os.path.exists(DEV):
        sys.exit("oracle/_ref/mbgc-dev is not built")
    for kind in ("t1", "m3"):
        with tempfile.TemporaryDirectory() as d:
            res = reference_streams(kind, d)
        with open(os.path.join(LIST, "expected_%s_single.json" % kind), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(kind, {k: v["bytes"] for k, v in res["streams"].items()})
