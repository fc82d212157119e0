"""The noise meter at the C-ABI level, without a GPU: libhiprz_noise.so loads and exports every symbol include/hiprz_noise.h declares, its
layouts agree with the Python mirror, it refuses to come up without a device, the pure-host summary equals the numpy restatement
(tests/noise_reference.py) — also as a process of its own under sanitizers — and every host stub of the new library has its gfx950 kernel."""
import ctypes as C
import importlib.util
import os
import re
import struct
import subprocess

import numpy as np

import noise_reference as nref
from rayzath_amd import _abi, _lib, noise
from rayzath_amd.engine import Context, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_noise.h")


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hiprz_noise_[a-z0-9_]+)\s*\(", text)))


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tile_maps(rng, tx, ty, empty=0.3):
    """random tile records of a tx x ty grid: integer counts, empty tiles, a tie for the worst tile between two non-adjacent tiles"""
    n = rng.integers(1, 257, (ty, tx)).astype(np.float32)
    n[rng.uniform(size=(ty, tx)) < empty] = 0
    tiles = np.zeros((ty, tx, 4), np.float32)
    mean_sq = rng.gamma(2.0, 1.0e-4, (ty, tx)).astype(np.float32)
    tiles[..., 0] = mean_sq * n
    tiles[..., 1] = np.sqrt(mean_sq) * rng.uniform(1.0, 3.0, (ty, tx)) * (n > 0)
    tiles[..., 2] = n
    tiles[..., 3] = np.floor(n * rng.uniform(0.0, 1.0, (ty, tx)))
    live = np.flatnonzero(n.reshape(-1) > 0)
    if len(live) >= 2:  # the same (sum, n) in two tiles, larger than all others: the first one is the worst
        a, b = sorted(rng.choice(live, 2, replace=False))
        flat = tiles.reshape(-1, 4)
        flat[a, 0] = flat[b, 0] = 64.0
        flat[a, 2] = flat[b, 2] = 16.0
        flat[a, 3] = flat[b, 3] = 3.0
    return tiles


_GRIDS = ((1, 1, 1, 1), (2, 3, 45, 20), (6, 13, 173, 99), (3, 8, 96, 64), (60, 135, 1920, 1080))


def test_library_exports_every_declared_symbol_and_the_mirror_binds_them(built):
    lib = noise.load()
    names = _declared_symbols()
    assert len(names) == 7, names
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_noise.h but not exported"
    assert set(names) == set(noise.ENTRY_POINTS)
    assert os.path.dirname(noise.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ, "the library sits next to libhiprz.so"


def test_accum_device_is_an_entry_point_of_the_context_library(built):
    assert "hiprz_accum_device" in _abi.ENTRY_POINTS
    lib = _lib.load()
    assert hasattr(lib, "hiprz_accum_device")
    assert re.search(r"\bint\s+hiprz_accum_device\(", open(os.path.join(ROOT, "include", "hiprz.h")).read())
    ptr = C.c_void_p()
    assert lib.hiprz_accum_device(None, C.byref(ptr)) == _abi.ERR_INVALID and not ptr
    for name in ("accum_device", "noise"):
        assert callable(getattr(Context, name)), name
    assert callable(Engine.render_until)


def test_layouts_match_the_mirror(built):
    out = (C.c_uint32 * 4)()
    noise.load().hiprz_noise_layout(out)
    assert out[0] == C.sizeof(noise.Params) == 16
    assert out[1] == C.sizeof(noise.Summary) == 56
    assert out[2] == noise.Summary.estimated.offset == 24
    assert out[3] == noise.Summary.tiles_x.offset == 48
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+HIPRZ_NOISE_TILE_W\s+(\d+)u", header).group(1)) == noise.TILE_W == nref.TILE_W
    assert int(re.search(r"#define\s+HIPRZ_NOISE_TILE_H\s+(\d+)u", header).group(1)) == noise.TILE_H == nref.TILE_H


def test_create_fails_loudly_without_a_gpu(built):
    import torch
    lib = noise.load()
    assert lib.hiprz_noise_create(None, 0) == _abi.ERR_INVALID
    assert lib.hiprz_noise_destroy(None) == _abi.ERR_INVALID
    if torch.cuda.is_available():
        return
    meter = C.c_void_p()
    assert lib.hiprz_noise_create(C.byref(meter), 0) == _abi.ERR_DEVICE and not meter
    assert b"HIP device" in lib.hiprz_noise_last_error(None)


def test_calls_without_a_meter_are_refused(built):
    lib = noise.load()
    p, s, buf = noise.Params(0.02, 1.0 / 60.0, 1.0 / 255.0, 8), noise.Summary(), (C.c_uint8 * 64)()
    assert lib.hiprz_noise_tiles(None, buf, buf, 1, 1, C.byref(p), buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_noise_measure(None, buf, buf, 1, 1, C.byref(p), None, C.byref(s), None) == _abi.ERR_INVALID
    assert b"null meter" in lib.hiprz_noise_last_error(None)


def test_summarise_reports_argument_errors(built):
    lib = noise.load()
    tiles = np.zeros((3, 2, 4), np.float32)
    out = noise.Summary()
    ok = (tiles.ctypes.data, 2, 3, 45, 20)
    assert lib.hiprz_noise_summarise(*ok, C.byref(out)) == _abi.OK
    assert lib.hiprz_noise_summarise(None, 2, 3, 45, 20, C.byref(out)) == _abi.ERR_INVALID
    assert lib.hiprz_noise_summarise(*ok, None) == _abi.ERR_INVALID
    for bad in ((2, 3, 0, 20), (2, 3, 45, 0), (0, 3, 45, 20), (2, 0, 45, 20), (3, 2, 45, 20), (2, 3, 65, 20), (2, 3, 45, 25), (1, 3, 45, 20)):
        assert lib.hiprz_noise_summarise(tiles.ctypes.data, *bad, C.byref(out)) == _abi.ERR_INVALID, bad


def _assert_same(got, want, what):
    for name in ("estimated", "above", "pixels", "tiles_x", "tiles_y", "worst_tile"):
        assert got[name] == want[name], (what, name, got[name], want[name])
    for name in ("rms", "tile_rms_max", "max"):  # the same float64 operations in the same order
        assert got[name] == want[name], (what, name, got[name], want[name])


def test_summarise_equals_the_numpy_summary(built):
    rng = np.random.default_rng(11)
    for tx, ty, W, H in _GRIDS:
        for empty in (0.3, 1.0):
            tiles = _tile_maps(rng, tx, ty, empty)
            got = noise.summarise(tiles, W, H).as_dict()
            want = nref.summary(tiles, W, H)
            _assert_same(got, want, (tx, ty, empty))
            if empty == 1.0:
                assert got["estimated"] == 0 and got["rms"] == 0 and got["tile_rms_max"] == 0 and got["worst_tile"] == 0
            elif tx * ty >= 6:
                flat = tiles.reshape(-1, 4)
                ties = np.flatnonzero((flat[:, 0] == 64.0) & (flat[:, 2] == 16.0))
                assert len(ties) == 2 and got["worst_tile"] == ties[0] and got["tile_rms_max"] == 2.0


def test_every_host_stub_of_the_noise_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "noise", "hiprz_noise.o"), noise.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 1 and "rz_noise_tiles_kernel" in next(iter(found[lib]))
    assert ck.host_stubs(os.path.join(CSRC, "noise", "hiprz_noise_host.o")) == set(), "the summary half is pure host code"
    assert not any("rz_noise_tiles" in name for name in ck.device_kernels(_lib.LIB_PATH)), "the kernel entered libhiprz.so, whose kernel set is pinned"


def test_the_summary_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "noise_summary_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "noise_summary_main.cpp"), os.path.join(CSRC, "noise", "hiprz_noise_host.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(12)
    cases = []
    with open(tmp_path / "maps.bin", "wb") as f:
        for tx, ty, W, H in _GRIDS:
            for empty in (0.3, 1.0):
                tiles = _tile_maps(rng, tx, ty, empty)
                f.write(struct.pack("<4I", tx, ty, W, H) + tiles.tobytes())
                cases.append((_abi.OK, nref.summary(tiles, W, H)))
        tiles = _tile_maps(rng, 2, 3)
        f.write(struct.pack("<4I", 2, 3, 70, 20) + tiles.tobytes())  # not the frame's grid: refused, nothing is read
        cases.append((_abi.ERR_INVALID, None))
    r = subprocess.run([exe, str(tmp_path / "maps.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"records {len(cases)}" and lines[-2] == "layout 16 56 24 48"
    for line, (rc, want) in zip(lines, cases):
        f_ = line.split()
        assert int(f_[0]) == rc
        if want is None:
            continue
        got = dict(rms=float(f_[1]), tile_rms_max=float(f_[2]), max=float(np.float32(float(f_[3]))), worst_tile=int(f_[4]), estimated=int(f_[5]), above=int(f_[6]),
                   pixels=int(f_[7]), tiles_x=int(f_[8]), tiles_y=int(f_[9]))
        _assert_same(got, want, line)
