"""The denoiser at the C-ABI level, without a GPU: the entry points are exported, the records have the layout the header gives them — as
the library was compiled, as a C compiler lays them out, and in the Python mirror —, the default parameters are sane and every call
refuses a null context."""
import ctypes as C
import os
import shutil
import subprocess

from rayzath_amd import _abi, _lib
from rayzath_amd.engine import denoise_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hiprz_render_guides", "hiprz_read_guides", "hiprz_guides_device", "hiprz_denoise_default_params", "hiprz_denoise",
         "hiprz_read_denoised", "hiprz_read_denoised_rgba8", "hiprz_denoise_image", "hiprz_set_denoise", "hiprz_denoise_layout")


def test_the_entry_points_are_exported_and_bound(built):
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _abi.ENTRY_POINTS, name


def test_record_sizes_agree_between_library_and_mirror(built):
    lib = _lib.load()
    out = (C.c_uint32 * 4)()
    lib.hiprz_denoise_layout(out)
    assert list(out) == [C.sizeof(_abi.Guide), C.sizeof(_abi.DenoiseParams), _abi.Guide.albedo.offset, _abi.Guide.instance.offset]
    assert C.sizeof(_abi.Guide) == _abi.guide_dtype.itemsize == 32 and C.sizeof(_abi.DenoiseParams) == 20
    for name in ("normal", "depth", "albedo", "instance"):
        assert _abi.guide_dtype.fields[name][1] == getattr(_abi.Guide, name).offset, name
    sizes = (C.c_uint32 * 13)()
    lib.hiprz_abi_sizes(sizes)  # stays at 13 entries
    assert all(v > 0 for v in sizes)


def test_record_sizes_agree_with_a_c_compiler(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler (the build itself needs one)"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hiprz.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(hiprz_guide), offsetof(hiprz_guide, depth),"
                   " offsetof(hiprz_guide, albedo), offsetof(hiprz_guide, instance), sizeof(hiprz_denoise_params),"
                   " offsetof(hiprz_denoise_params, sigma_color), offsetof(hiprz_denoise_params, flags)); return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G, P = _abi.Guide, _abi.DenoiseParams
    assert got == [C.sizeof(G), G.depth.offset, G.albedo.offset, G.instance.offset, C.sizeof(P), P.sigma_color.offset, P.flags.offset]


def test_default_params_are_sane(built):
    p = denoise_params()
    assert 1 <= p.iterations <= 6
    assert p.sigma_normal > 0 and 0 < p.sigma_depth < 10 and 0 <= p.sigma_color <= 10
    assert p.flags == _abi.DENOISE_DEMODULATE
    q = denoise_params(iterations=2, sigma_color=0.0, demodulate=False)
    assert (q.iterations, q.sigma_color, q.flags, q.sigma_normal) == (2, 0.0, 0, p.sigma_normal)
    _lib.load().hiprz_denoise_default_params(None)  # tolerated


def test_calls_on_a_null_context_fail_cleanly(built):
    lib = _lib.load()
    p = denoise_params()
    buf = (C.c_uint8 * 64)()
    ptr = C.c_void_p()
    assert lib.hiprz_render_guides(None) == _abi.ERR_INVALID
    assert lib.hiprz_read_guides(None, buf, 64) == _abi.ERR_INVALID
    assert lib.hiprz_guides_device(None, C.byref(ptr)) == _abi.ERR_INVALID and not ptr
    assert lib.hiprz_denoise(None, C.byref(p)) == _abi.ERR_INVALID
    assert lib.hiprz_denoise(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_read_denoised(None, buf, 64) == _abi.ERR_INVALID
    assert lib.hiprz_read_denoised_rgba8(None, buf, 64) == _abi.ERR_INVALID
    assert lib.hiprz_denoise_image(None, buf, None, None, buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_set_denoise(None, C.byref(p)) == _abi.ERR_INVALID
    assert lib.hiprz_set_denoise(None, None) == _abi.ERR_INVALID
