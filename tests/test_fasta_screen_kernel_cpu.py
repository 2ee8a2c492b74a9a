"""k_fa_screen without a GPU: the lane steps and the host's builders of the filter and the table (mbgc_amd/csrc/fasta_screen.h holds no
HIP call) compiled as plain C++ with AddressSanitizer and UBSan and run as a program of its own, tile by tile, lane by lane, the wave's
shuffles emulated by arrays, over texts over ACGTNacgtnRYU>\\0 and records that start at every offset mod 16, have 0, k - 1, k and k + 1
bytes and end on the buffer's last byte, around a tile's edge and around a wave's edge, against a byte loop that builds every k-mer
from scratch, its reverse complement by reversing the string, and looks the smaller one up in a std::set
(tests/fasta_screen_emu.cpp). k = 1, 2, 15, 16, 17, 31, 32. The text, the keys, the filter and the table are exactly as long as they
are said to be: a read outside one ends the run. The program says per k how many positions it compared, how many hit, how many filter
passes the table refuted and how long the longest probe chain was; asked for here: at least 10 000 compared and 1 000 hits at every k,
and at least one refuted pass and a chain of more than one slot at every k from 15 on, so that "ok" cannot mean "nothing exercised".
At k = 1 and k = 2 there are 2 and 10 canonical words in all, far fewer than the filter has bits: a word that is no key and still
passes the filter would need two of them on one of 2^17 bits, so no refuted pass is asked for there. Says nothing about the compiled
device code, the shuffles, the cursor or the sorts — that is tests/test_gpu_fasta_screen.py's job."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_and_builders_equal_the_byte_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_screen_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), r.stdout[-3000:] + r.stderr[-3000:]
    seen = {int(m[0]): tuple(int(x) for x in m[1:]) for m in
            re.findall(r"^k (\d+): (\d+) positions compared, (\d+) hits, (\d+) filter passes, (\d+) refuted by the table, longest probe chain (\d+)", r.stdout, flags=re.M)}
    assert sorted(seen) == [1, 2, 15, 16, 17, 31, 32], r.stdout
    for k, (compared, hits, passes, refuted, chain) in seen.items():
        assert compared >= 10_000 and hits >= 1_000 and passes == hits + refuted, r.stdout
        assert k < 15 or (refuted >= 1 and chain > 1), r.stdout
