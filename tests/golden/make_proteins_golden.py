"""Regenerates tests/golden/proteins/*.json from the reference CLI (oracle/_ref/mbgc-dev): what `mbgc c` decides about the protein
profile, and the streams it then writes.

  rule_cases.json               per case of tests/_probe.py's rule_cases(): did stderr hold "Switching to protein profile."?
  expected_t1.json / _m3.json   the protein collection of _probe.collection() through `mbgc-dev c -t1` / `c -m 3` (both
                                deterministic) and `mbgc-dev v -D`, which dumps the raw streams in the order of
                                MBGC_Decoder.cpp:1085-1112; sizes and digests as in tests/golden/listeria/expected_t1.json

The inputs are generated (numpy.random.RandomState, a frozen stream) and are not stored; only these results are.

    python tests/golden/make_proteins_golden.py        (needs oracle/_ref/mbgc-dev)"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "proteins")
DEV = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "mbgc-dev")
LINE = "Switching to protein profile."
# the matcher-side streams are the last the reader meets; with the profile switched there is no rcMapOff / rcMapLen under -m 3 either
ORDER = ["literals", "locksPos", "gapDelta", "flags", "mapOff", "mapLen", "refExtSize"]
ARGS = {"t1": ["-t1"], "m3": ["-m", "3"]}

import _probe  # noqa: E402


def write_list(workdir, files, tag):
    names = []
    for i, recs in enumerate(files):
        name = "%s%d.fa" % (tag, i)
        with open(os.path.join(workdir, name), "wb") as f:
            f.write(_probe.fasta(recs, "%s%d" % (tag, i)))
        names.append(name)
    with open(os.path.join(workdir, "list.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return names


def compress(workdir, args, arc):
    r = subprocess.run([DEV, "c"] + args + ["list.txt", arc], cwd=workdir, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return LINE in r.stderr


def rule_case(records, opts):
    with tempfile.TemporaryDirectory() as d:
        write_list(d, [records, _probe.second_file()], "r")
        return compress(d, opts, "r.mbgc")


def collection_streams(kind):
    files = _probe.collection()
    with tempfile.TemporaryDirectory() as d:
        names = write_list(d, files, "p")
        switched = compress(d, ARGS[kind], "p.mbgc")
        subprocess.run([DEV, "v", "-t1", "-D", "p.mbgc"], check=True, capture_output=True, cwd=d)
        dumps = sorted(f for f in os.listdir(d) if re.fullmatch(r"p\.mbgc_dump_\d+", f))
        assert len(dumps) >= len(ORDER)
        out = {}
        for name, f in zip(ORDER, dumps[-len(ORDER):]):
            b = open(os.path.join(d, f), "rb").read()
            out[name] = {"bytes": len(b), "md5": hashlib.md5(b).hexdigest()}
            if name == "literals":                      # (the dumps are the ones meant: the literals start with the initial reference)
                assert b.startswith(files[0][0] + b"\xa2"), f
    return dict(command="mbgc-dev c %s list.txt p.mbgc && mbgc-dev v -t1 -D p.mbgc  (the files of tests/_probe.py collection())" % " ".join(ARGS[kind]),
                files=names, switched=switched, streams=out)


if __name__ == "__main__":
    if not os.path.exists(DEV):
        sys.exit("oracle/_ref/mbgc-dev is not built")
    os.makedirs(OUT, exist_ok=True)
    rules = {}
    for name, (records, opts, sequential) in _probe.rule_cases().items():
        rules[name] = dict(options=opts, record_lengths=[len(r) for r in records], switched=rule_case(records, opts))
        print(name, rules[name]["switched"])
    with open(os.path.join(OUT, "rule_cases.json"), "w") as f:
        json.dump(rules, f, indent=1)
        f.write("\n")
    for kind in ("t1", "m3"):
        res = collection_streams(kind)
        with open(os.path.join(OUT, "expected_%s.json" % kind), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(kind, res["switched"], {k: v["bytes"] for k, v in res["streams"].items()})
