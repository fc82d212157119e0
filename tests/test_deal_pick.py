"""rayzath_amd/csrc/hiprz_deal_pick.hpp — the integer half of dealing a leaf's later triangle pairs over a wave's lanes — run WITHOUT a
GPU.  The header and tests/deal_pick_shim.cpp are compiled with g++ under ASan and UBSan into a program of their own (nothing built
with a sanitizer is loaded into this process).  Inside it a wave of 64 lanes with a visit of some pairs per lane is settled twice: by
"every owner walks its pairs 1 .. in order" and by the dealing (owner search, pair index, trip and lane of a work item, the merge in
pair order and in a shuffled order).  Inputs: every rem in 0 .. 3 on lanes 0, 15, 16 and 63; totals T = 0, 1, 63, 64, 65, 128 and 320
with uniform and non-uniform rem; DRAWS random waves.  Distances come from six values, so equal distances found by different lanes are
common: the lower triangle index must win.  Every pair must be assigned exactly once and no lane gets two work items in one trip.  The
program itself checks that the draws reached a tie across lanes, a taken and a declined wave and an owner whose items straddle two trips.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
DRAWS = 20000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("deal_pick") / "deal_pick_shim")
    cmd = ["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "deal_pick_shim.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return out


def test_dealing_equals_every_owner_walking_its_pairs(program):
    proc = subprocess.run([program, str(DRAWS)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert int(proc.stdout) == 64 * (256 * 8 + 7 * 200 + DRAWS)


def test_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "hiprz_deal_pick.hpp")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
