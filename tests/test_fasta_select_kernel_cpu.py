"""k_fa_match_headers without a GPU: the two lane steps and the host's table builder (mbgc_amd/csrc/fasta_select.h hold no HIP call)
compiled as plain C++ with AddressSanitizer and run tile by tile, lane by lane, over random header blobs and pattern lists against
a memmem loop written the obvious way (tests/fasta_select_emu.cpp). Every header stands in an allocation exactly as long as itself,
the patterns and the staging buffer are exactly as long as declared: a read outside a record's own header ends the run. Says
nothing about the compiled device code, the barrier, the ballot or the atomic — that is tests/test_gpu_fasta_select.py's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_plain_memmem_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(HERE, "fasta_select_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: 1500 calls"
