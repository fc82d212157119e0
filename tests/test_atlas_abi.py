"""Bake atlases at the C-ABI level, without a GPU: libhiprz_atlas.so loads and exports exactly the symbols include/hiprz_atlas.h declares,
atlas.ENTRY_POINTS binds them, null arguments are refused, begin applies its size rule, the library does not come up without a device,
every host stub of the new library has its gfx950 kernel — four of them, none in the five libraries whose kernel sets are pinned — and
the pure-host unit runs as a process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from rayzath_amd import _abi, _lib, atlas, bake, order, query, scene
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_atlas.h")
KERNELS = ("rz_atlas_clear_kernel", "rz_atlas_cover_kernel", "rz_atlas_points_kernel", "rz_atlas_dilate_kernel")
NAMES = ["hiprz_atlas_" + n for n in ("add", "add_host", "begin", "create", "destroy", "dilate", "dilate_host", "last_error", "layout", "points_device", "read_host",
                                     "read_records_host", "records_device", "samples_device")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = atlas.load()
    names = sorted(set(re.findall(r"\b(hiprz_atlas_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_atlas.h but not exported"
    assert set(names) == set(atlas.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", atlas.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    assert os.path.dirname(atlas.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ or "HIPRZ_ATLAS_LIB" in os.environ
    # the point is the bake library's, not restated; the rules are written out in the header
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_bake.h"' in header and "typedef struct hiprz_bake_point" not in header
    assert "e(p) = (B.x - A.x) * (p.y - A.y) - (B.y - A.y) * (p.x - A.x)" in text, "the edge value is part of the contract"
    assert "a_i = (u_i * float(W) - 0.5f, v_i * float(H) - 0.5f)" in text and "p = (p1 * b1 + p2 * bx) + p3 * by" in text
    assert "(x-1, y) (x+1, y) (x, y-1) (x, y+1) (x-1, y-1) (x+1, y-1) (x-1, y+1) (x+1, y+1)" in text, "the neighbour order is part of the contract"
    assert re.search(r"#define\s+HIPRZ_ATLAS_NONE\s+0xFFFFFFFFu", header) and atlas.NONE == 0xFFFFFFFF
    assert re.search(r"#define\s+HIPRZ_ATLAS_MAX_SIZE\s+16384u", header) and re.search(r"#define\s+HIPRZ_ATLAS_MAX_RINGS\s+64u", header)
    assert (atlas.MAX_SIZE, atlas.MAX_RINGS) == (16384, 64)


def test_the_layout_is_the_mirrors(built):
    out = (C.c_uint32 * 8)()
    atlas.load().hiprz_atlas_layout(out)
    t, s = atlas.tri_dtype, atlas.sample_dtype
    assert list(out) == [t.itemsize, s.itemsize, bake.point_dtype.itemsize, t.fields["n1"][1], t.fields["v3"][1], s.fields["bx"][1], s.fields["by"][1],
                         s.fields["zero"][1]] == [96, 16, 32, 48, 92, 4, 8, 12]
    assert [t.fields[k][1] for k in ("p1", "u1", "p2", "u2", "p3", "u3", "n1", "v1", "n2", "v2", "n3", "v3")] == [0, 12, 16, 28, 32, 44, 48, 60, 64, 76, 80, 92]
    # charts(): one record per triangle in the mesh's order, its own UVs or a second set, zeros where a mesh has no normals
    cube, sphere = scene.generate_cube(), scene.generate_sphere(8)
    c, sp = atlas.charts(cube), atlas.charts(sphere)
    assert c.dtype == t and c.shape == (12,) and sp.shape == (48,)
    assert not c["n1"].any() and not c["n2"].any() and not c["n3"].any(), "the cube has no normals: the face normal is used"
    assert np.array_equal(sp["n2"], sphere.normals[sphere.tri_normals[:, 1]]) and np.array_equal(sp["p3"], sphere.vertices[sphere.tri_vertices[:, 2]])
    assert np.array_equal(c["u1"], cube.texcrds[cube.tri_texcrds[:, 0], 0]) and np.array_equal(c["v3"], cube.texcrds[cube.tri_texcrds[:, 2], 1])
    second = np.linspace(0.1, 0.9, 16, dtype=np.float32).reshape(8, 2)
    c2 = atlas.charts(cube, texcrds=second, tri_texcrds=cube.tri_vertices)
    assert np.array_equal(c2["u2"], second[cube.tri_vertices[:, 1], 0]) and np.array_equal(c2["p1"], c["p1"])
    try:
        atlas.charts(scene.Mesh(cube.vertices, cube.tri_vertices))
    except ValueError as e:
        assert "no texture coordinates" in str(e)
    else:
        raise AssertionError("a mesh without UVs made charts")


def test_null_arguments_are_refused(built):
    lib = atlas.load()
    buf = (C.c_uint8 * 96)()
    assert lib.hiprz_atlas_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_atlas_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_atlas_begin(None, 4, 4) == _abi.ERR_INVALID and b"atlas_begin: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_add(None, buf, 1, 0, 0, 1e-3, 1.0, None) == _abi.ERR_INVALID and b"atlas_add: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_add(None, buf, 0, 0, 0, 1e-3, 1.0, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    assert lib.hiprz_atlas_add_host(None, buf, 1, 0, 0, 1e-3, 1.0) == _abi.ERR_INVALID and b"atlas_add_host: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_read_host(None, buf, buf) == _abi.ERR_INVALID and b"atlas_read_host: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_read_records_host(None, buf, buf) == _abi.ERR_INVALID and b"atlas_read_records_host: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_dilate(None, buf, 1, None, None) == _abi.ERR_INVALID and b"atlas_dilate: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_dilate_host(None, buf, 1, None) == _abi.ERR_INVALID and b"atlas_dilate_host: null atlas" in lib.hiprz_atlas_last_error(None)
    assert lib.hiprz_atlas_points_device(None) is None and lib.hiprz_atlas_samples_device(None) is None and lib.hiprz_atlas_records_device(None) is None
    lib.hiprz_atlas_layout(None)         # nothing to write to: returns
    for name in ("atlas", "atlas_points", "bake_atlas"):
        assert callable(getattr(Context, name)), name
    for name in ("begin", "add", "add_device", "points_device", "samples_device", "read", "dilate", "dilate_device"):
        assert callable(getattr(atlas.Atlas, name)), name


def test_create_fails_loudly_without_a_gpu(built):
    lib = atlas.load()
    a = C.c_void_p(1)
    rc = lib.hiprz_atlas_create(C.byref(a), None)
    assert not a
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_atlas_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_atlas_last_error(None)


def test_every_host_stub_of_the_atlas_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; four kernels,
    and none of them in the libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "atlas", "hiprz_atlas.o"), atlas.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 4
    for kernel in KERNELS:
        assert sum(kernel in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "atlas", "hiprz_atlas_host.o")) == set(), "the refusals, the size rule and the layout report are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others), "a kernel of the atlas library is in a library whose kernel set is pinned"
    assert not any("rz_atlas" in name for name in others)
    assert all("N5hiprz" in name for name in found[lib]), "the atlas kernels live in namespace hiprz"


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "atlas", "hiprz_atlas.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_session.hpp"' in code and "struct hiprz_atlas : Session" in code, "the handle is built on the shared session"
    assert code.count("__global__") == 4 and "__shared__" not in code, "four kernels, no LDS"
    assert len(re.findall(r"\batomic\w*\(", code)) == 1 and "atomicMin(&owner[" in code, "one vector atomic: the owner of a texel"
    assert len(re.findall(r"\bfloat edge_value\(", code)) == 1 and len(re.findall(r"\bedge_value\(", code)) == 7, "the edge value is written once: area, 3 in cover, 2 in points"
    assert "__launch_bounds__(RZ_ATLAS_WG)" in code and re.search(r"#define\s+RZ_ATLAS_WG\s+64\b", code)
    host = open(os.path.join(CSRC, "atlas", "hiprz_atlas_host.cpp")).read() + open(os.path.join(CSRC, "atlas", "hiprz_atlas_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_atlas\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*atlas/\*\.o.*\blibhiprz_atlas\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_atlas") == 2, "libhiprz_host.so and hip_engine_test link the atlas library"


def test_begin_applies_the_size_rule_and_needs_no_device(built):
    """begin is host only, so its rule is checked on a handle where there is a device to make one on, and through the host unit below
    everywhere"""
    if not os.path.exists("/dev/kfd"):
        return
    ctx = Context(0)
    try:
        a = ctx.atlas()
        lib, h = a.lib, a._atlas
        for w, hh in ((0, 4), (4, 0), (16385, 4), (4, 16385), (2**32 - 1, 1)):
            assert lib.hiprz_atlas_begin(h, w, hh) == _abi.ERR_INVALID and b"atlas_begin: " in lib.hiprz_atlas_last_error(h), (w, hh)
        assert lib.hiprz_atlas_points_device(h) is None
        assert lib.hiprz_atlas_begin(h, 16384, 16384) == _abi.OK and lib.hiprz_atlas_begin(h, 1, 1) == _abi.OK     # nothing is allocated by a begin
        assert lib.hiprz_atlas_points_device(h) is None and lib.hiprz_atlas_records_device(h) is None, "no arrays before the first add"
    finally:
        ctx.close()


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/atlas/hiprz_atlas_host.cpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 6 * 0xFFFFFFFF)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**28, 2**28 + 1), (65536, 65537), (1, 60000),
          (6 * 0xFFFFFFFF - 1, 6 * 0xFFFFFFFF), (2**34, 2**34 + 1)]
_SIZES = [("1 1", "none"), ("16384 16384", "none"), ("0 4", "width is not in 1..16384"), ("4 0", "height is not in 1..16384"), ("16385 4", "width is not in 1..16384"),
          ("4 16385", "height is not in 1..16384"), ("4294967295 1", "width is not in 1..16384"), ("7 5", "none")]
_NULL, _BEGIN, _IDS = "null pointer", "no atlas has been begun", "triangle_base + n is 0xFFFFFFFF or more"
_FINITE, _NEAR, _FAR = "near_ or far_ is not finite: every point would be invalid", "near_ < 0: every point would be invalid", "far_ <= near_: every point would be invalid"
_ADDS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _BEGIN), (_abi.ERR_STATE, _BEGIN), (_abi.OK, "none"), (_abi.ERR_INVALID, _IDS),
         (_abi.ERR_INVALID, _IDS), (_abi.OK, "none"), (_abi.ERR_INVALID, _IDS), (_abi.ERR_INVALID, _IDS), (_abi.ERR_INVALID, _IDS), (_abi.ERR_INVALID, _FINITE),
         (_abi.ERR_INVALID, _FINITE), (_abi.ERR_INVALID, _FINITE), (_abi.ERR_INVALID, _NEAR), (_abi.OK, "none"), (_abi.ERR_INVALID, _FAR), (_abi.ERR_INVALID, _FAR)]
_INSTANCES = [("0 of 1", "none"), ("0 of 0", "the scene has no such instance"), ("3 of 3", "the scene has no such instance"), ("2 of 3", "none"),
              ("4294967295 of 4294967295", "the scene has no such instance")]
_BUILT, _RINGS = "nothing has been added since the atlas was begun", "more than 64 rings"
_DILATIONS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _RINGS), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _BUILT), (_abi.ERR_STATE, _BUILT),
              (_abi.ERR_INVALID, _RINGS)]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "atlas_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "atlas"), os.path.join(ROOT, "tests", "atlas_host_main.cpp"), os.path.join(CSRC, "atlas", "hiprz_atlas_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}"
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
    at = len(_PAIRS)
    for prefix, want, fmt in (("size", _SIZES, "size {}: {}"), ("add", _ADDS, "add: {} {}"), ("instance", _INSTANCES, "instance {}: {}"), ("dilate", _DILATIONS, "dilate: {} {}")):
        assert lines[at:at + len(want)] == [fmt.format(a, b) for a, b in want], prefix
        at += len(want)
    assert lines[at:-1] == ["layout 96 16 32 48 92 4 8 12"]
