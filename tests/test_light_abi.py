"""Light baking at the C-ABI level, without a GPU: libhiprz_light.so loads and exports exactly the symbols include/hiprz_light.h declares,
light.ENTRY_POINTS binds them, null arguments are refused, the library does not come up without a device, every host stub of the new
library has its gfx950 kernel — two of them, none in the six other libraries — the kernel unit takes the ray rule and the walk from the
query's device header and makes a sample in one function, the library links against libhiprz.so alone, and the pure-host unit runs as a
process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from rayzath_amd import _abi, _lib, atlas, bake, light, order, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_light.h")
KERNELS = ("rz_light_bake_kernel", "rz_light_rays_kernel")
NAMES = ["hiprz_light_" + n for n in ("bake", "bake_host", "count", "create", "destroy", "disk_samples", "last_error", "layout", "rays", "set_of", "set_samples")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = light.load()
    names = sorted(set(re.findall(r"\b(hiprz_light_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_light.h but not exported"
    assert set(names) == set(light.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", light.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    assert os.path.dirname(light.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ or "HIPRZ_LIGHT_LIB" in os.environ
    # the point and the ray are the bake's and the query's, not restated; the hash is written out in the header, and so is what is left out
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_bake.h"' in header and "typedef struct hiprz_ray" not in header and "typedef struct hiprz_bake_point" not in header
    assert "x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;" in text
    assert "q.c = lpos.c + ((t.c * x + bt.c * y) * size)" in text and "d.c = (t.c * (x * g) + bt.c * (y * g)) + a.c * z" in text, "the parenthesisation is part of the contract"
    for left_out in ("radiance < 1e-4", "scattering factor", "coloured shadow mask", "BRDF-sampled term Se"):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    assert re.search(r"#define\s+HIPRZ_LIGHT_INVALID\s+0x80000000u", header) and light.INVALID == 0x80000000
    assert re.search(r"#define\s+HIPRZ_LIGHT_TO_END\s+0xFFFFFFFFu", header) and light.TO_END == 0xFFFFFFFF


def test_the_library_links_against_libhiprz_alone(built):
    needed = subprocess.run(["readelf", "-d", light.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_light\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*light/\*\.o.*\blibhiprz_light\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_light") == 2, "libhiprz_host.so and hip_engine_test link the light library"


def test_the_layout_is_the_mirrors(built):
    out = (C.c_uint32 * 6)()
    light.load().hiprz_light_layout(out)
    p, t, r = bake.point_dtype, light.texel_dtype, light.range_dtype
    assert list(out) == [p.itemsize, t.itemsize, r.itemsize, t.fields["light"][1], t.fields["shadowed"][1], r.fields["direct_first"][1]] == [32, 16, 16, 0, 12, 8]
    assert light.point_dtype is bake.point_dtype
    assert light.light_range(None) is None and light.light_range((1, None, 2, 3)).tolist() == [(1, 0xFFFFFFFF, 2, 3)]


def test_null_arguments_are_refused(built):
    lib = light.load()
    buf = (C.c_uint8 * 96)()
    assert lib.hiprz_light_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_light_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_light_bake(None, buf, 1, 0, None, buf, None) == _abi.ERR_INVALID
    assert b"light_bake: null light" in lib.hiprz_light_last_error(None)
    assert lib.hiprz_light_rays(None, buf, 1, 0, None, buf, buf, None) == _abi.ERR_INVALID
    assert b"light_rays: null light" in lib.hiprz_light_last_error(None)
    assert lib.hiprz_light_bake_host(None, buf, 1, 0, None, buf) == _abi.ERR_INVALID
    assert b"light_bake_host: null light" in lib.hiprz_light_last_error(None)
    assert lib.hiprz_light_set_samples(None, buf, 16, 1) == _abi.ERR_INVALID
    assert b"light_set_samples: null light" in lib.hiprz_light_last_error(None)
    spots, directs = C.c_uint32(7), C.c_uint32(7)
    assert lib.hiprz_light_count(None, None, C.byref(spots), C.byref(directs)) == _abi.ERR_INVALID and (spots.value, directs.value) == (7, 7)
    assert b"light_count: null light" in lib.hiprz_light_last_error(None)
    assert lib.hiprz_light_bake(None, buf, 0, 0, None, buf, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    assert lib.hiprz_light_disk_samples(16, 1, None) == _abi.ERR_INVALID
    lib.hiprz_light_layout(None)         # nothing to write to: returns
    for name in ("light", "bake_light", "light_rays", "bake_light_atlas"):
        assert callable(getattr(Context, name)), name
    for name in ("set_samples", "count", "bake", "bake_device", "rays_device", "rays"):
        assert callable(getattr(light.Light, name)), name
    assert callable(atlas.bake_light)


def test_create_fails_loudly_without_a_gpu(built):
    lib = light.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_light_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_light_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_light_last_error(None)


def test_every_host_stub_of_the_light_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; two kernels, and
    none of them in the six libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "light", "hiprz_light.o"), light.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 2
    for kernel in KERNELS:
        assert sum(kernel in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "light", "hiprz_light_host.o")) == set(), "the refusals, the table check, the range rule and the host-only calls are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others), "a kernel of the light library is in a library whose kernel set is pinned"
    assert not any("rz_light" in name for name in others)
    assert all("N5hiprz" in name for name in found[lib]), "the light kernels live in namespace hiprz"


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "light", "hiprz_light.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_query_device.hpp"' in code and "bool take_ray(" not in code, "the invalid-ray rule exists once"
    assert '#include "query/hiprz_session.hpp"' in code and "struct hiprz_light : Session" in code, "the handle is built on the shared session"
    assert "take_ray(" in code and "occluded_word(s, r0, r1, 0u)" in code and "HIPRZ_QUERY_NORMALIZE" in code
    assert code.count("__global__") == 2 and "__shared__" not in code and "atomic" not in code, "two kernels, no LDS, no atomics"
    assert "__launch_bounds__(RZ_LIGHT_WG)" in code and re.search(r"#define\s+RZ_LIGHT_WG\s+64\b", code)
    assert len(re.findall(r"\blight_sample\(", code)) == 3, "the device function that makes a sample is written once and called by both kernels"
    for f in ("sinf(", "cosf(", "acosf(", "expf(", "RZ_SINCOSF", "RZ_EXPF", "RZ_ACOSF", "__fmaf", "fmaf("):
        assert f not in code, f"{f} in the kernel unit: the rules are plain float32 with true / and sqrtf"
    assert "bake/" not in code and "atlas/" not in code and "hiprz_atlas" not in code, "nothing of the bake or atlas libraries but the point's layout"
    host = open(os.path.join(CSRC, "light", "hiprz_light_host.cpp")).read() + open(os.path.join(CSRC, "light", "hiprz_light_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in make and re.search(r"light/hiprz_light\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\)", make)


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/light/hiprz_light_host.cpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 2**31)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**30, 2**30 + 1), (2**31, 2**31),
          (2**30 + 5, 2**31), (2**31 - 1, 2**31), (3, 2**31), (65536, 65537), (1, 60000)]
_NULL, _TABLE, _SIZE = "null pointer", "no sample table has been set", "n*K is 2^31 or more"
_REFUSALS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _TABLE),
             (_abi.ERR_STATE, _TABLE), (_abi.ERR_STATE, _TABLE), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE),
             (_abi.ERR_INVALID, _SIZE), (_abi.ERR_INVALID, _SIZE)]
_MANY = "n*L*K is 2^31 or more"
_RAYS = ["none", "none", "none", _MANY, "none", "none", _MANY, "none", _MANY, _MANY, "none", _MANY]
_FINITE, _DISK = "a sample is not finite", "a sample lies outside the unit disk"
_K, _S = "K is not a power of two in 1..1024", "S is not in 1..64"
_TABLES = [("good", "none"), ("nan", _FINITE), ("inf", _FINITE), ("just outside", _DISK), ("on the rim", "none"), ("behind the rim", _DISK), ("centre", "none"),
           ("K = 1", "none"), ("K = 48", _K), ("K = 0", _K), ("K = 1024", "none"), ("K = 2048", _K), ("S = 0", _S), ("S = 65", _S), ("S = 64", "none"),
           ("null", "null pointer")]
_RANGES = [("null", "0 3 0 2"), ("all", "0 3 0 2"), ("one", "1 1 0 0"), ("tail", "2 1 1 1"), ("none", "3 0 2 0"), ("no lights", "0 0 0 0"),
           ("behind", "the range starts behind the last spot light"), ("long", "the range ends behind the last spot light"),
           ("direct behind", "the range starts behind the last direct light"), ("direct long", "the range ends behind the last direct light"),
           ("wrap", "the range ends behind the last spot light")]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "light_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "light"), os.path.join(ROOT, "tests", "light_host_main.cpp"), os.path.join(CSRC, "light", "hiprz_light_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}"
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
    at = len(_PAIRS)
    assert lines[at:at + len(_REFUSALS)] == [f"refusal: {code} {why}" for code, why in _REFUSALS]
    at += len(_REFUSALS)
    assert lines[at:at + len(_RAYS)] == [f"rays: {why}" for why in _RAYS]
    at += len(_RAYS)
    assert lines[at:at + len(_TABLES)] == [f"table {name}: {why}" for name, why in _TABLES]
    at += len(_TABLES)
    assert lines[at:at + len(_RANGES)] == [f"range {name}: {what}" for name, what in _RANGES]
    at += len(_RANGES)
    want = light.set_of(1, 0, 64), light.set_of(0, 1, 7), light.set_of(9, 9, 5), 0
    assert lines[at:-1] == ["disk 1024 64: 0, behind 7", "table disk: none", "disk 1 1: 0, %.9g 0" % np.float32(np.sqrt(0.5)), "disk 48 1: %d, wrote 0" % _abi.ERR_INVALID,
                            "disk null: %d" % _abi.ERR_INVALID, "layout 32 16 16 0 12 8", "set_of %d %d %d %d" % want]
