"""The packer's pair section (rayzath_amd/csrc/hiprz_scene_host.cpp: PackedScene::pair_section — what the one-leaf walk's triangle loop
reads) WITHOUT a GPU: tests/pair_records_main.cpp, a program of its own, is compiled with the packer under AddressSanitizer and UBSan and
run as a child process.  It packs worlds with single-leaf meshes of 1, 2, 3, 4, 5, 8, 9, 12, 31 and 32 triangles and checks that every
pair record equals triangles 2p and 2p + 1 of its leaf bit for bit (an odd leaf's last record repeating a in b), that the table points
every instance at its mesh's records (two instances of one mesh share them, a mesh with an inner root has none while its neighbours
do), that the section is empty for a world of 9 instances, a world that is not one leaf, a world without a single-leaf mesh and trees
rebuilt at upload, and that the blob and its seven offsets are byte-identical with and without the section, the total being blob +
section."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_ASSERTIONS"]


def test_pair_section_of_the_packer(tmp_path):
    exe = str(tmp_path / "pair_records")
    subprocess.run(["g++", *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "hiprz_scene_host.cpp"),
                    os.path.join(CSRC, "hiprz_host.cpp"), os.path.join(ROOT, "tests", "pair_records_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "pair records: 10 scenes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
