"""mbgc_fasta_inflate_dev (k_fa_inflate: gzip files inflated where they lie in HBM) through the ctypes mirror, on torch buffers, over
the corpus of tests/_inflate_cases.py — the same streams tests/test_inflate_kernel_cpu.py has already run through the decoder's text
on the CPU under AddressSanitizer. Expected bytes are zlib's. Every job's output range stands at an odd offset between guard bands of
a known pattern, which must come back untouched whatever the job's status; a failing job leaves the other jobs of its call alone."""
import numpy as np
import pytest

import _inflate_cases as cases

pytestmark = pytest.mark.gpu
GUARD = 16
PATTERN = 0xA5


def run_jobs(selected, odd=True):
    """selected: corpus rows -> (results [(status, members, outLen, inUsed)], the output buffer as numpy, jobs [(inOff, inLen, outOff, outCap)])"""
    import torch
    from mbgc_amd import fasta
    jobs, gz_parts, in_at, out_at = [], [], 0, GUARD
    for k, (name, stream, cap, status, want) in enumerate(selected):
        lead = (1 + k % 5) if odd else 0                       # bytes between the streams: every alignment of the input too
        gz_parts.append(b"\x1f" * lead + stream)
        in_at += lead
        if odd and (out_at % 2 == 0):
            out_at += 1
        jobs.append((in_at, len(stream), out_at, cap))
        in_at += len(stream)
        out_at += cap + GUARD
    gz = np.frombuffer(b"".join(gz_parts), dtype=np.uint8)
    assert gz.size == in_at
    gz_dev = torch.from_numpy(gz.copy()).to("cuda:0")
    out_dev = torch.full((out_at,), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        results, ms = p.inflate_dev(gz_dev.data_ptr(), gz.size, out_dev.data_ptr(), out_at, jobs)
    finally:
        p.close()
    out = out_dev.cpu().numpy()
    return results, out, jobs


def check(selected, odd=True):
    results, out, jobs = run_jobs(selected, odd)
    covered = np.zeros(out.size, dtype=bool)
    for (name, stream, cap, status, want), (st, members, out_len, in_used), (in_off, in_len, out_off, out_cap) in zip(selected, results, jobs):
        if status == cases.NOT_OK:
            assert st != cases.OK, name
        else:
            assert st == status, (name, st, status)
        if st == cases.OK:
            assert out_len == len(want) and in_used == in_len and members >= 1, (name, out_len, len(want), in_used, in_len, members)
            assert out[out_off: out_off + out_len].tobytes() == want, name
            assert (out[out_off + out_len: out_off + out_cap] == PATTERN).all(), name     # nothing behind the text
            covered[out_off: out_off + out_len] = True
        else:
            covered[out_off: out_off + out_cap] = True                                    # (unspecified inside its own range)
    assert (out[~covered] == PATTERN).all(), "a byte outside every job's range was written"
    return results


def by_status(ok):
    return [c for c in cases.corpus() if (c[3] == cases.OK) == ok]


@pytest.mark.parametrize("case", by_status(True), ids=lambda c: c[0])
def test_valid_stream(case):
    (status, members, out_len, in_used), = check([case])
    assert members == {"two_members": 2, "three_members_one_empty": 3, "member_after_stored": 2}.get(case[0], 1)


@pytest.mark.parametrize("case", by_status(False), ids=lambda c: c[0])
def test_failing_stream_beside_good_ones(case):
    good = [c for c in cases.corpus() if c[0] in ("dna_70x80", "z_fixed")]
    check([good[0], case, good[1]])


def test_aligned_ranges():
    check([c for c in cases.corpus() if c[0] in ("dna_70x80", "level0_stored_blocks", "level6")], odd=False)


def test_64_jobs_at_odd_offsets():
    small = [c for c in cases.corpus() if len(c[1]) < 60_000]
    check([small[k % len(small)] for k in range(64)])


def test_200_jobs_mixed():
    rows = cases.corpus()
    check([rows[(7 * k) % len(rows)] for k in range(200) if rows[(7 * k) % len(rows)][0] != "random_acgt_1mib"] + [r for r in rows if r[0] == "random_acgt_1mib"])


def test_job_outside_the_buffers_is_refused():
    import torch
    from mbgc_amd import binding, fasta
    row = [c for c in cases.corpus() if c[0] == "dna_70x80"][0]
    gz = np.frombuffer(row[1], dtype=np.uint8)
    gz_dev = torch.from_numpy(gz.copy()).to("cuda:0")
    out_dev = torch.full((row[2] + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        for jobs in ([(0, gz.size + 1, 0, row[2])], [(1, gz.size, 0, row[2])], [(0, gz.size, 65, row[2])], [(0, gz.size, 2 ** 63, 2 ** 63)],
                     [(0, gz.size, 0, row[2]), (0, gz.size, row[2] - 1, 32)]):              # the last: two output ranges that overlap
            with pytest.raises(binding.SwsemError):
                p.inflate_dev(gz_dev.data_ptr(), gz.size, out_dev.data_ptr(), row[2] + 64, jobs)
        assert (out_dev.cpu().numpy() == PATTERN).all()                                    # nothing was launched
        (st, members, out_len, in_used), = p.inflate_dev(gz_dev.data_ptr(), gz.size, out_dev.data_ptr(), row[2] + 64, [(0, gz.size, 3, row[2])])[0]
        assert (st, members, out_len, in_used) == (cases.OK, 1, row[2], gz.size)
    finally:
        p.close()


def test_input_inside_an_output_range_of_the_same_buffer_is_refused():
    """gz_dev and out_dev may be one buffer (the round's file buffer of `c` holds both); a job's input where a job's output is written is not"""
    import torch
    from mbgc_amd import binding, fasta
    row = [c for c in cases.corpus() if c[0] == "dna_70x80"][0]
    n, cap = len(row[1]), row[2]
    at = (cap + 15) // 16 * 16
    buf = torch.full((at + n + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    buf[at: at + n] = torch.from_numpy(np.frombuffer(row[1], dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        for out_off, out_cap in ((at - 8, cap), (at + n - 1, 8), (at + 5, 1)):
            with pytest.raises(binding.SwsemError):
                p.inflate_dev(buf.data_ptr(), buf.numel(), buf.data_ptr(), buf.numel(), [(at, n, out_off, out_cap)])
        res, _ = p.inflate_dev(buf.data_ptr(), buf.numel(), buf.data_ptr(), buf.numel(), [(at, n, 0, cap)])       # apart: inflated in place
        assert res[0] == (cases.OK, 1, cap, n)
        assert buf[:cap].cpu().numpy().tobytes() == row[4]
    finally:
        p.close()
