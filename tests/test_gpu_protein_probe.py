"""mbgc_fasta_probe_dev (the protein-profile probe on contigs in HBM) against its restatement, tests/_probe.py — which
tests/test_protein_probe_rule.py holds to the reference CLI's own decisions. Fired flag, record index and the carried state."""
import numpy as np
import pytest

import _probe
from mbgc_amd import fasta

pytestmark = pytest.mark.gpu
CASES = _probe.rule_cases()


@pytest.fixture(scope="module")
def parser():
    p = fasta.FastaParser(0)
    yield p
    p.close()


def on_device(parser, records, k=32, state=_probe.START, lead=0, gap=0):
    """the records laid out in one device buffer, `lead` bytes in front and `gap` bytes between them (bytes the probe must not
    count: all non-standard) -> what the kernel says"""
    import torch
    blob, offs = bytearray(b"#" * lead), []
    for r in records:
        offs.append(len(blob))
        blob += r + b"#" * gap
    dev = torch.from_numpy(np.frombuffer(bytes(blob) + b"#", dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return parser.probe_dev(dev.data_ptr(), len(blob), offs, [len(r) for r in records], k=k, state=state)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("lead,gap", [(0, 0), (3, 5)])
def test_rule_cases(parser, name, lead, gap):
    records, opts, _ = CASES[name]
    if "-U" in opts:
        records = [r.upper() for r in records]
    k = _probe.case_k(opts)
    assert on_device(parser, records, k, lead=lead, gap=gap) == _probe.probe_records(records, k=k)


def odd_records(seed, lengths, bad=0.3):
    rs = np.random.RandomState(seed)
    return [_probe.with_nonstd(rs, n, int(n * bad)) for n in lengths]


EXTRA = {
    "empty_record_in_front": [b""] + odd_records(1, [300]),
    "empty_records_between": odd_records(2, [100]) + [b"", b""] + odd_records(3, [100, 100]),
    "only_empty_records": [b"", b""],
    "one_byte_records": [bytes([c]) for c in _probe.draw(np.random.RandomState(4), _probe.AMINO, 700)],
    "one_byte_dna_then_protein": [bytes([c]) for c in _probe.draw(np.random.RandomState(5), _probe.DNA, 300)] + odd_records(6, [17]),
    "lengths_not_multiples_of_16": odd_records(7, [15, 17, 1, 31, 33, 63, 65, 1023, 1025, 4097], bad=0.05),
    "exactly_the_limit": odd_records(8, [65536], bad=0.0) + odd_records(9, [500]),
    "exactly_the_limit_fires_at_its_end": odd_records(10, [65000], bad=0.0) + odd_records(11, [536], bad=0.5) + odd_records(12, [40]),
    "running_count_over_a_tiny_record": odd_records(13, [3000, 2999, 7], bad=0.02),
    "all_byte_values": [bytes(range(256)) * 2, bytes(range(255, -1, -1))],
}


@pytest.mark.parametrize("name", sorted(EXTRA))
@pytest.mark.parametrize("lead", [0, 1, 7])
def test_shapes(parser, name, lead):
    records = EXTRA[name]
    for k in (32, 16):
        assert on_device(parser, records, k, lead=lead, gap=lead) == _probe.probe_records(records, k=k), k


def test_record_of_exactly_probe_remaining(parser):
    records = odd_records(14, [1000, 77], bad=0.04)
    state = (1000, 3)
    got = on_device(parser, records, state=state, lead=5)
    assert got == _probe.probe_records(records, state) and got[2][0] == 0


def test_state_carried_across_two_calls(parser):
    prot = CASES["protein_k24"][0][0]
    first, second = [prot[:120], prot[120:200]], [prot[200:230], prot[230:300], prot[300:900]]
    a = on_device(parser, first, lead=1)
    assert a == _probe.probe_records(first) and not a[0]
    b = on_device(parser, second, state=a[2], lead=2)
    assert b == _probe.probe_records(second, a[2]) and b[:2] == (True, 1)       # 256 bases are reached inside the second call's record 1
    assert on_device(parser, second, state=b[2]) == (False, 0, b[2])            # spent
    # over a whole file the two calls decide what one call decides
    assert _probe.probe_records(first + second)[0] and _probe.probe_records(first + second)[2] == b[2]


def test_host_call_probes_what_the_parse_left_on_the_device(parser):
    for name in ("running_count_over_1500", "lowercase_n_15pct", "lowercase_n_15pct_U", "straddle_clipped_divisor"):
        records, opts, _ = CASES[name]
        upper = "-U" in opts
        want = _probe.probe_records([r.upper() for r in records] if upper else records)
        assert parser.probe_host(_probe.fasta(records, "x"), uppercase=upper) == want, name
    records = CASES["running_count_over_1500"][0]
    assert parser.probe_host(_probe.fasta(records, "x"), records=1) == _probe.probe_records(records[:1])


def test_records_outside_the_buffer_are_refused(parser):
    import torch
    from mbgc_amd import binding
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(binding.SwsemError):
        parser.probe_dev(dev.data_ptr(), 64, [60], [5])
    with pytest.raises(binding.SwsemError):
        parser.probe_dev(dev.data_ptr(), 64, [0], [10], state=(70000, 0))
