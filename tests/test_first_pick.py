"""flat_pick_first of rayzath_amd/csrc/hiprz_flat_pick.hpp — the pick of the visit a ray of the one-leaf walk makes in place, ahead of the
binned rounds — run WITHOUT a GPU.  The header and tests/first_pick_shim.cpp are compiled with g++ under ASan and UBSan into a program
of their own (nothing built with a sanitizer is loaded into this process).  Inside it, against a literal restatement (the one-by-one
chain on copies of mask and next, committed iff there is no candidate or the candidate's bit in `small` is set): all 256 verdict masks x
all 256 `small` masks x next 0..8 x three classes of draws of tm[8] and far (equal values, tm[k] == far, +-0, +-inf, NaN; small finite
values with far taken from tm; random bit patterns), DRAWS draws each.  Candidate, mask and next are equal; a committed pick is
flat_pick's; a ray without a candidate is finished as flat_pick finishes it; a declined pick leaves mask and next untouched and
flat_pick called after it yields what flat_pick alone yields."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]
DRAWS = 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("first_pick") / "first_pick_shim")
    cmd = ["g++", *FLAGS, "-I", CSRC, os.path.join(ROOT, "tests", "first_pick_shim.cpp"), "-o", out]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return out


def test_first_pick_equals_its_restatement(program):
    proc = subprocess.run([program, str(DRAWS)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    picks, committed, declined, finished = (int(x) for x in proc.stdout.split())
    assert picks == 256 * 256 * 9 * 3 * DRAWS
    assert committed + declined + finished == picks
    assert min(committed, declined, finished) > 0
