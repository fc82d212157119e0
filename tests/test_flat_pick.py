"""rayzath_amd/csrc/hiprz_flat_pick.hpp — the one-leaf walk's candidate pick and its packed 8-bin prefix — run WITHOUT a GPU.  The header
and tests/flat_pick_shim.cpp are compiled with g++ under ASan and UBSan into a program of their own (nothing built with a sanitizer is
loaded into this process).  Inside it:

1. flat_pick against the candidate loop it replaced, restated literally: all 256 masks x flat_next 0..8 x three classes of draws of
   tm[8] and far (special values: equal values, tm[k] == far, +-0, +-inf, NaN; small finite values with far taken from tm; random bit
   patterns), DRAWS draws each: candidate, new flat_next and new flat_mask are equal.
2. flat_prefix8 / flat_round / flat_item_slot against three plain prefix sums over random bin counts of at most 256 visits (wide bins in
   multiples of 8 lanes), with wide + narrow == 256 and == 257 among the fixed cases: every field of every bin, the totals, and every
   visit's item slots, which together cover [0, n_items) once.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
DRAWS, ROUNDS = 2000, 200000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("flat_pick") / "flat_pick_shim")
    cmd = ["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "flat_pick_shim.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return out


def test_pick_and_prefix_equal_the_loops_they_replace(program):
    proc = subprocess.run([program, str(DRAWS), str(ROUNDS)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    picks, prefixes = (int(x) for x in proc.stdout.split())
    assert picks == 256 * 9 * 3 * DRAWS
    assert prefixes >= ROUNDS + 2


def test_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "hiprz_flat_pick.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
