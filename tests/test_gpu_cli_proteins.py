"""The protein profile through the tool. `mbgc-hip c` probes the initial reference on the device as `mbgc c` probes it
(tests/_probe.py; tests/test_protein_probe_rule.py holds that restatement to the reference's decisions) and, when the probe fires —
or under --proteins — goes on with k = 16 (unless -k is given), mismatches coded without exclusion and no reverse-complement pass.
  * the protein collection of _probe.collection(): `c -t1` and `c -m 3` against the reference CLI's dumps
    (tests/golden/proteins/expected_{t1,m3}.json, written by tests/golden/make_proteins_golden.py);
  * rounds against the oracle-driven reference loop (tests/_driver.py) at k = 16 with exclusion off;
  * `d --fasta` gives the files back; the rule's edge cases decide as the reference decided; --proteins; two ranks; a DNA list."""
import hashlib
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _driver
import _meta
import _orc
import _probe
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "proteins")
LISTERIA = os.path.join(ROOT, "tests", "golden", "listeria")
LINE = "Switching to protein profile."
STREAMS = ("literals", "mapOff", "mapOff5th", "mapLen", "gapDelta", "flags", "locksPos", "refExtSize")
EXCLUSION = 1                                                         # index of mismatchesWithExclusion in .meta's emission parameters


def run_tool(args, cwd):
    """-> (stdout, stderr)"""
    r = subprocess.run(["timeout", "-k", "10", "280", TOOL] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout, r.stderr


def write_list(tmp, files, tag):
    """the files as tests/golden/make_proteins_golden.py writes them -> {name: bytes}"""
    written = {}
    for i, recs in enumerate(files):
        name = "%s%d.fa" % (tag, i)
        written[name] = _probe.fasta(recs, "%s%d" % (tag, i))
        (tmp / name).write_bytes(written[name])
    (tmp / "list.txt").write_text("\n".join(written) + "\n")
    return written


def meta_of(tmp, prefix):
    return _meta.parse((tmp / (prefix + ".meta")).read_bytes())


def dumps(tmp, prefix):
    return {k: (tmp / (prefix + "." + k)).read_bytes() for k in STREAMS}


def as_arrays(files):
    return [[np.frombuffer(r, dtype=np.uint8) for r in recs] for recs in files]


def oracle_rounds(files, rs, k, exclusion, mode=1):
    """the reference's round loop on the oracle -> the tool's eight streams"""
    lim, _ = _driver.ref_length_limit(len(files), sum(c.size for c in files[0]), mode=mode)
    o = _orc.OracleMatcher(lim, L=k, skip_margin=24 if mode >= 2 else 16)
    p = _orc.emit_params(mode, mismatchesWithExclusion=exclusion)
    res = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o, p), files[0], files[1:], rs, _driver.Policy(mode), min_len=k)
    out = dict(res["streams"])
    out["literals"] = b"".join(c.tobytes() + b"\xa2" for c in files[0]) + out["literals"]
    out["locksPos"], out["refExtSize"] = res["locks"], res["refExtSize"]
    o.close()
    return out


def files_of(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(str(d)))}


@pytest.fixture(scope="module")
def collection(tmp_path_factory):
    """the protein collection compressed three ways: -t1, -m 3 and -R 2"""
    tmp = tmp_path_factory.mktemp("proteins")
    written = write_list(tmp, _probe.collection(), "p")
    err = {}
    for prefix, args in (("t1", ["-t1"]), ("m3", ["-m", "3"]), ("r2", ["-R", "2"])):
        err[prefix] = run_tool(["c"] + args + ["list.txt", prefix], tmp)[1]
    return tmp, written, err


@pytest.mark.parametrize("kind", ["t1", "m3"])
def test_collection_streams_equal_reference_cli(collection, kind):
    """(fails without the probe: the tool then matches with k = 32 and codes mismatches with exclusion)"""
    tmp, _, err = collection
    exp = json.load(open(os.path.join(GOLDEN, "expected_%s.json" % kind)))
    assert exp["switched"] and err[kind].count(LINE) == 1, err[kind]
    for name, e in exp["streams"].items():
        b = (tmp / (kind + "." + name)).read_bytes()
        assert len(b) == e["bytes"], (name, len(b), e["bytes"])
        assert hashlib.md5(b).hexdigest() == e["md5"], name
    assert (tmp / (kind + ".mapOff5th")).read_bytes() == b""
    assert not (tmp / (kind + ".rcMapOff")).exists() and not (tmp / (kind + ".rcMapLen")).exists()     # -m 3: the RC pass is off
    m = meta_of(tmp, kind)
    assert m["k"] == 16 and m["emit"][EXCLUSION] == 0 and m["sequential"] and not m["rc_redundancy_removal"]


def test_collection_rounds_equal_oracle_driver(collection):
    tmp, _, err = collection
    assert err["r2"].count(LINE) == 1
    want, got = oracle_rounds(as_arrays(_probe.collection()), 2, 16, 0), dumps(tmp, "r2")
    for k in STREAMS:
        assert got[k] == want[k], k
    assert len(got["mapLen"]) > 1000                                   # (the targets were matched, not copied out as literals)
    m = meta_of(tmp, "r2")
    assert m["k"] == 16 and m["emit"][EXCLUSION] == 0 and not m["sequential"]


@pytest.mark.parametrize("prefix", ["t1", "m3", "r2"])
def test_collection_comes_back_as_fasta(collection, prefix):
    """.meta carries k and the exclusion flag: `d` needs no option of its own"""
    tmp, written, _ = collection
    run_tool(["d", "--fasta", "back_" + prefix, prefix, "seq_" + prefix], tmp)
    assert files_of(tmp / ("back_" + prefix)) == written


RULES = _probe.rule_cases()
RECORDED = json.load(open(os.path.join(GOLDEN, "rule_cases.json")))


@pytest.mark.parametrize("name", sorted(RULES))
def test_rule_cases_decide_as_the_reference(tmp_path, name):
    records, opts, _ = RULES[name]
    write_list(tmp_path, [records, _probe.second_file()], "r")
    _, err = run_tool(["c"] + opts + ["list.txt", "out"], tmp_path)
    switched = RECORDED[name]["switched"]
    assert (LINE in err) == switched, err
    m = meta_of(tmp_path, "out")
    assert m["k"] == (_probe.case_k(opts) if "-k" in opts or not switched else 16)
    assert m["emit"][EXCLUSION] == (0 if switched else 1)


def dna_files():
    base = synth.base_codes(70_000, 58)
    gs = [synth.genome(base, i, 0.015) for i in range(7)]
    return [[g[:30_011], g[30_011:]] for g in gs]


def write_dna(tmp):
    paths = []
    for i, contigs in enumerate(dna_files()):
        p = tmp / ("g%02d.fa" % i)
        p.write_bytes(b"".join(synth.fasta_bytes(c, i * 10 + j) for j, c in enumerate(contigs)))
        paths.append(str(p))
    (tmp / "list.txt").write_text("\n".join(paths) + "\n")


def test_proteins_option(tmp_path):
    """--proteins on DNA: k = 16 and no exclusion, whatever the probe would say (its k != 16 guard keeps it silent); with -k the
    length stays"""
    write_dna(tmp_path)
    _, err = run_tool(["c", "--proteins", "-R", "3", "list.txt", "p"], tmp_path)
    assert err.count(LINE) == 1
    want, got = oracle_rounds(dna_files(), 3, 16, 0), dumps(tmp_path, "p")
    for k in STREAMS:
        assert got[k] == want[k], k
    m = meta_of(tmp_path, "p")
    assert m["k"] == 16 and m["emit"][EXCLUSION] == 0
    for args in (["--proteins", "-k", "20"], ["-k", "20", "--proteins"]):
        _, err = run_tool(["c"] + args + ["-R", "3", "list.txt", "q"], tmp_path)
        assert err.count(LINE) == 1
        m = meta_of(tmp_path, "q")
        assert m["k"] == 20 and m["emit"][EXCLUSION] == 0
        want, got = oracle_rounds(dna_files(), 3, 20, 0), dumps(tmp_path, "q")
        for k in STREAMS:
            assert got[k] == want[k], (args, k)


def test_two_ranks_decide_alike(collection):
    """--gpus 2 -R 1: both ranks probe their copy of the initial reference before the exchange starts; the streams are -R 2's"""
    tmp, _, _ = collection
    _, err = run_tool(["c", "--gpus", "2", "--exchange", "hostmem", "--shm-mb", "1", "-R", "1", "list.txt", "many"], tmp)
    assert err.count(LINE) == 1                                        # (rank 0 reports for all)
    a, b = dumps(tmp, "r2"), dumps(tmp, "many")
    for k in STREAMS:
        assert a[k] == b[k], k
    assert meta_of(tmp, "many")["k"] == 16


def test_dna_list_is_left_alone(tmp_path):
    """the Listeria genomes under -t1 (their bytes are pinned by tests/test_gpu_cli.py): no switch"""
    exp = json.load(open(os.path.join(LISTERIA, "expected_t1.json")))
    names = []
    for f in exp["files"]:
        (tmp_path / f).write_bytes(lzma.open(os.path.join(LISTERIA, f + ".xz")).read())
        names.append(str(tmp_path / f))
    (tmp_path / "seqlist.txt").write_text("\n".join(names) + "\n")
    _, err = run_tool(["c", "-t1", "seqlist.txt", "lm"], tmp_path)
    assert LINE not in err
    m = meta_of(tmp_path, "lm")
    assert m["k"] == 32 and m["emit"][EXCLUSION] == 1
