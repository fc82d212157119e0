"""Occlusion baking at the C-ABI level, without a GPU: libhiprz_bake.so loads and exports exactly the symbols include/hiprz_bake.h declares,
bake.ENTRY_POINTS binds them, null arguments are refused, the library does not come up without a device, every host stub of the new
library has its gfx950 kernel — two of them, none in libhiprz.so, libhiprz_query.so or libhiprz_order.so — the kernel unit takes the ray
rule from the query's device header, and the pure-host unit runs as a process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from rayzath_amd import _abi, _lib, bake, order, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_bake.h")
KERNELS = ("rz_bake_occlusion_kernel", "rz_bake_rays_kernel")
NAMES = ["hiprz_bake_" + n for n in ("cosine_directions", "create", "destroy", "last_error", "layout", "occlusion", "occlusion_host", "rays", "set_directions",
                                    "set_of")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = bake.load()
    names = sorted(set(re.findall(r"\b(hiprz_bake_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_bake.h but not exported"
    assert set(names) == set(bake.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", bake.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    assert os.path.dirname(bake.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ or "HIPRZ_BAKE_LIB" in os.environ
    # the ray is the query library's, not restated; the hash is written out in the header
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_query.h"' in header and "typedef struct hiprz_ray" not in header
    assert "x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;" in text
    assert "d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z" in text, "the parenthesisation of the rotation is part of the contract"
    assert re.search(r"#define\s+HIPRZ_BAKE_INVALID\s+0x80000000u", header) and bake.INVALID == 0x80000000


def test_the_layout_is_the_mirrors(built):
    out = (C.c_uint32 * 6)()
    bake.load().hiprz_bake_layout(out)
    p, t = bake.point_dtype, bake.texel_dtype
    assert list(out) == [p.itemsize, t.itemsize, p.fields["normal"][1], p.fields["far"][1], t.fields["bent"][1], t.fields["occluded"][1]] == [32, 16, 16, 28, 0, 12]
    r = query.ray_dtype                 # a point is the ray along its normal
    assert [p.fields[a][1] for a in ("position", "near", "normal", "far")] == [r.fields[b][1] for b in ("origin", "near", "direction", "far")]
    pts = bake.points([[1, 2, 3], [4, 5, 6]], [0, 0, 1], far=9.0)
    assert pts.dtype == p and pts.shape == (2,) and pts["near"].tolist() == [np.float32(1e-3)] * 2 and pts["normal"][1].tolist() == [0, 0, 1]


def test_null_arguments_are_refused(built):
    lib = bake.load()
    buf = (C.c_uint8 * 96)()
    assert lib.hiprz_bake_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_bake_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_bake_occlusion(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert b"bake_occlusion: null bake" in lib.hiprz_bake_last_error(None)
    assert lib.hiprz_bake_rays(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert b"bake_rays: null bake" in lib.hiprz_bake_last_error(None)
    assert lib.hiprz_bake_occlusion_host(None, buf, 1, 0, buf) == _abi.ERR_INVALID
    assert b"bake_occlusion_host: null bake" in lib.hiprz_bake_last_error(None)
    assert lib.hiprz_bake_set_directions(None, buf, 16, 1) == _abi.ERR_INVALID
    assert b"bake_set_directions: null bake" in lib.hiprz_bake_last_error(None)
    assert lib.hiprz_bake_occlusion(None, buf, 0, 0, buf, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    assert lib.hiprz_bake_cosine_directions(16, 1, None) == _abi.ERR_INVALID
    lib.hiprz_bake_layout(None)         # nothing to write to: returns
    for name in ("bake", "bake_occlusion", "bake_rays"):
        assert callable(getattr(Context, name)), name
    for name in ("set_directions", "occlusion", "occlusion_device", "rays_device"):
        assert callable(getattr(bake.Bake, name)), name


def test_create_fails_loudly_without_a_gpu(built):
    lib = bake.load()
    b = C.c_void_p(1)
    rc = lib.hiprz_bake_create(C.byref(b), None)
    assert not b
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_bake_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_bake_last_error(None)


def test_every_host_stub_of_the_bake_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; two kernels, and
    none of them in the three libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "bake", "hiprz_bake.o"), bake.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 2
    for kernel in KERNELS:
        assert sum(kernel in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "bake", "hiprz_bake_host.o")) == set(), "the refusals, the table check and the host-only calls are pure host code"
    others = ck.device_kernels(_lib.LIB_PATH) | ck.device_kernels(query.LIB_PATH) | ck.device_kernels(order.LIB_PATH)
    assert not (found[lib] & others), "a kernel of the bake library is in a library whose kernel set is pinned"
    assert not any("rz_bake" in name for name in others)
    assert all("N5hiprz" in name for name in found[lib]), "the bake kernels live in namespace hiprz"


def test_the_kernel_unit_takes_the_ray_rule_from_the_query(built):
    body = open(os.path.join(CSRC, "bake", "hiprz_bake.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_query_device.hpp"' in code and "bool take_ray(" not in code and "isfinite" not in code, "the invalid-ray rule exists once"
    assert "take_ray(" in code and "occluded_word(s, r0, r1, 0u)" in code and "HIPRZ_QUERY_NORMALIZE" in code
    assert code.count("__global__") == 2 and "__shared__" not in code and "atomic" not in code, "two kernels, no LDS, no atomics"
    assert len(re.findall(r"\bbake_ray\(", code)) == 3, "the device function that makes a ray is written once and called by both kernels"
    host = open(os.path.join(CSRC, "bake", "hiprz_bake_host.cpp")).read() + open(os.path.join(CSRC, "bake", "hiprz_bake_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/bake/hiprz_bake_host.cpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 2**27)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**26, 2**26 + 1), (2**27, 2**27),
          (2**26 + 5, 2**27), (2**27 - 1, 2**27), (3, 2**27), (65536, 65537), (1, 60000)]
_NULL, _TABLE, _SIZE = "null pointer", "no direction table has been set", "n*K is 2^31 or more"
_REFUSALS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _TABLE),
             (_abi.ERR_STATE, _TABLE), (_abi.ERR_STATE, _TABLE), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE),
             (_abi.ERR_INVALID, _SIZE), (_abi.ERR_INVALID, _SIZE)]
_FINITE, _UNIT = "a direction is not finite", "a direction is not of unit length (squared length outside [0.999, 1.001])"
_K, _S = "K is not one of 16, 32, 64, 128, 256, 512, 1024", "S is not in 1..64"
_TABLES = [("good", "none"), ("nan", _FINITE), ("inf", _FINITE), ("nan in w", "none"), ("squared length 1.002", _UNIT), ("squared length 0.998", _UNIT),
           ("length 1.002", _UNIT), ("length 0.998", _UNIT), ("length 1.0004 downwards", "none"), ("zero", _UNIT), ("K = 48", _K), ("K = 8", _K),
           ("K = 1024", "none"), ("K = 2048", _K), ("S = 0", _S), ("S = 65", _S), ("S = 64", "none"), ("null", "null pointer")]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "bake_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "bake"), os.path.join(ROOT, "tests", "bake_host_main.cpp"), os.path.join(CSRC, "bake", "hiprz_bake_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}"
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
    at = len(_PAIRS)
    assert lines[at:at + len(_REFUSALS)] == [f"refusal: {code} {why}" for code, why in _REFUSALS]
    at += len(_REFUSALS)
    assert lines[at:at + len(_TABLES)] == [f"table {name}: {why}" for name, why in _TABLES]
    at += len(_TABLES)
    want = bake.set_of(1, 0, 64), bake.set_of(0, 1, 7), bake.set_of(9, 9, 5), 0
    assert lines[at:-1] == ["cosine 1024 64: 0, behind 7", "table cosine: none", "cosine 48 1: %d, wrote 0" % _abi.ERR_INVALID, "layout 32 16 16 28 0 12",
                            "set_of %d %d %d %d" % want]
