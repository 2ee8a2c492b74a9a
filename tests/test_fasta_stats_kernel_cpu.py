"""k_fa_stats without a GPU: the lane steps (mbgc_amd/csrc/fasta_stats.h holds no HIP call) compiled as plain C++ with AddressSanitizer
and UBSan and run as a program of its own, tile by tile, lane by lane, the wave's shuffles emulated by arrays, over random texts over
ACGTNacgtnRYU>\\0 and record lists that overlap, touch and are empty, against a byte loop written the obvious way
(tests/fasta_stats_emu.cpp): the counters of every record and the paired runs of both classes. The text is exactly seqBytes long: a
read outside the buffer ends the run. The program says how many runs of each class it compared, and at least 1 000 of each are asked
for here, so that "ok" cannot mean "nothing to compare". Says nothing about the compiled device code, the shuffles, the sums in LDS
or the atomics — that is tests/test_gpu_fasta_stats.py's job."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_the_byte_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_stats_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.match(r"ok: 400 calls, runs compared: class 0 (\d+), class 1 (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 1000 and int(m.group(2)) >= 1000, r.stdout
