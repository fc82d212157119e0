"""rayzath_amd/csrc/hiprz_u8_div.hpp — a byte over 255 in two fmas (RZ_U8_SHORT_DIV: from_u8 and fetch_r8 on the device) — run WITHOUT
a GPU.  The header and tests/u8_division_main.cpp are compiled with g++ -ffp-contract=off (the device build's setting: only the fmas the
header spells are fused) into a program of their own.  Inside it all 256 bytes go through the short form and through `/`: the bits must
be equal.  The same program counts the bytes for which the bare product n * y misses the quotient: 126, which is why the refinement is
there.  Built with the switch on and off: u8_over_255 equals the division under both.  On the device hiprz_selftest repeats the comparison
(tests/test_mirror_lobe_gpu.py).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


@pytest.mark.parametrize("switch", [1, 0])
def test_all_256_bytes_equal_the_division(tmp_path, switch):
    out = str(tmp_path / "u8_division")
    cmd = ["g++", *FLAGS, f"-DRZ_U8_SHORT_DIV={switch}", "-I", CSRC, os.path.join(ROOT, "tests", "u8_division_main.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    proc = subprocess.run([out], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    checked, bad, bare_bad = (int(x) for x in proc.stdout.split()[-3:])
    assert checked == 256 and bad == 0
    assert bare_bad == 126, "the bare product misses the quotient for 126 bytes: one refinement is needed, and it is enough"


def test_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "hiprz_u8_div.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
