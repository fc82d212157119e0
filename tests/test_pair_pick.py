"""rayzath_amd/csrc/hiprz_pair_pick.hpp — how the one-leaf walk settles two triangles tested in one iteration — run WITHOUT a GPU.  The
header and tests/pair_pick_shim.cpp are compiled with g++ under ASan and UBSan into a program of their own (nothing built with a
sanitizer is loaded into this process).  Inside it pair_pick is set against the one-by-one loop over the two triangles (tri_hit's range
test, the far end moving between them): all four hit masks x three classes of draws of the two distances and the range ends (special
values: equal values, +-0, +-inf, NaN; small finite values with a distance put ON the near end, the far end or the other distance;
random bit patterns), DRAWS draws each: winner and the bits of the new far end are equal.  The program itself checks that the draws
reached every winner, equal distances won by the first triangle, distances on either range end, NaNs and zeros.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
DRAWS = 200000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_pick") / "pair_pick_shim")
    cmd = ["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "pair_pick_shim.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return out


def test_pair_pick_equals_the_one_by_one_loop(program):
    proc = subprocess.run([program, str(DRAWS)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert int(proc.stdout) == 4 * 3 * DRAWS


def test_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "hiprz_pair_pick.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
