"""Pipelined frame delivery (hiprz_present / hiprz_read_frame) at the C-ABI level, without a GPU: both calls are exported and refuse a
null context, and the Python mirror of hiprz_frame has the layout the header gives it — as the library was compiled, and as a C
compiler lays it out from include/hiprz.h."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from rayzath_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_present_and_read_frame_are_exported_and_refuse_a_null_context(built):
    lib = _lib.load()
    for name in ("hiprz_present", "hiprz_read_frame", "hiprz_frame_layout"):
        assert hasattr(lib, name), name
        assert name in _abi.ENTRY_POINTS, name
    assert lib.hiprz_present(None, 0, 0) == _abi.ERR_INVALID
    frame = _abi.Frame()
    assert lib.hiprz_read_frame(None, 0, C.byref(frame)) == _abi.ERR_INVALID
    assert lib.hiprz_read_frame(None, 1, None) == _abi.ERR_INVALID


def test_frame_layout_matches_the_library(built):
    lib = _lib.load()
    out = (C.c_uint32 * 3)()
    lib.hiprz_frame_layout(out)
    assert list(out) == [C.sizeof(_abi.Frame), _abi.Frame.ray_count.offset, _abi.Frame.hit.offset]
    assert C.sizeof(_abi.Frame) == 56 and C.sizeof(_abi.RayCast) == 16


def test_frame_layout_matches_a_c_compiler(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hiprz.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu\\n\", sizeof(hiprz_frame), offsetof(hiprz_frame, depth),"
                   " offsetof(hiprz_frame, width), offsetof(hiprz_frame, sequence), offsetof(hiprz_frame, ray_count),"
                   " offsetof(hiprz_frame, hit)); return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    F = _abi.Frame
    assert got == [C.sizeof(F), F.depth.offset, F.width.offset, F.sequence.offset, F.ray_count.offset, F.hit.offset]
