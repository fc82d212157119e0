"""Probe baking at the C-ABI level, without a GPU: libhiprz_probe.so loads and exports exactly the symbols include/hiprz_probe.h declares,
probe.ENTRY_POINTS binds them, null arguments are refused, the library does not come up without a device, every host stub of the new
library has its gfx950 kernel — three of them, none in the eight other libraries — the kernel unit takes the ray rule and the walks from
the query's device header, makes a ray and a sample in one function each and keeps a lane's running sums where the build says, the library
links against libhiprz.so alone, and the pure-host unit runs as a process of its own under sanitizers: every refusal in the header's order,
the sphere table and the evaluation."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

import bake_reference as BR
from rayzath_amd import _abi, _lib, atlas, bake, gather, light, order, probe, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_probe.h")
KERNELS = ("rz_probe_gather_kernel", "rz_probe_light_kernel", "rz_probe_samples_kernel")
NAMES = ["hiprz_probe_" + n for n in ("create", "destroy", "gather", "gather_host", "irradiance", "last_error", "layout", "light", "light_host", "samples", "set_charts",
                                      "set_directions", "set_samples", "sphere_directions")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = probe.load()
    names = sorted(set(re.findall(r"\b(hiprz_probe_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_probe.h but not exported"
    assert set(names) == set(probe.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", probe.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_gather.h"' in header and '#include "hiprz_light.h"' in header and "typedef struct hiprz_bake_point" not in header
    assert "x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;" in text
    for rule in ("d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z", "u  = (u1 * b1 + u2 * bx) + u3 * by", "b1 = (1.0f - bx) - by", "B6 = (3.0f*(d.z*d.z)) - 1.0f",
                 "acc[b].c = acc[b].c + (L.c * B_b)", "acc[b].c = acc[b].c + (P.c * B_b(w3))", "P.c = ((colour.c * emission) * w) * 0.25f",
                 "out.sh[b].c = base.sh[b].c + light[b].c", "e = e + ((w_b * sh[b].c) * B_b(n))", "w = {1, 2, 2, 2, 15/4, 15/4, 5/16, 15/4, 15/16}"):
        assert rule in text, f"the parenthesisation is part of the contract: {rule}"
    for left_out in ("bands above 2", "ringing windowing", "probe placement and visibility", "glossy transport", "transmission", "scattering medium",
                     "device-side evaluation kernel"):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    assert re.search(r"#define\s+HIPRZ_PROBE_INVALID\s+0x%08Xu" % probe.INVALID, header)
    assert probe.INVALID == gather.INVALID == light.INVALID == bake.INVALID


def test_the_library_links_against_libhiprz_alone(built):
    needed = subprocess.run(["readelf", "-d", probe.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_probe\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*probe/\*\.o.*\blibhiprz_probe\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_probe") == 2, "libhiprz_host.so and hip_engine_test link the probe library"
    assert re.search(r"^hip_engine_test:.*\blibhiprz_probe\.so\b", make, flags=re.M) and re.search(r"^libhiprz_host\.so:.*\blibhiprz_probe\.so\b", make, flags=re.M)
    assert re.search(r"^PROBE_DEFS \?=\s*$", make, flags=re.M)
    assert "-ffp-contract=off" in make and re.search(r"probe/hiprz_probe\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\) \$\(PROBE_DEFS\)", make)


def test_the_layout_is_the_mirrors(built):
    out = (C.c_uint32 * 6)()
    probe.load().hiprz_probe_layout(out)
    assert list(out) == [bake.point_dtype.itemsize, probe.sh_dtype.itemsize, gather.sample_dtype.itemsize, gather.chart_dtype.itemsize, 12, 28]
    assert list(out) == [32, 144, 16, 32, 12, 28]
    rec = np.zeros(1, probe.sh_dtype)
    rec["sh"][0, 0, 3], rec["sh"][0, 1, 3] = np.array([7, 9], np.uint32).view(np.float32)
    assert rec.view(np.uint32)[[3, 7]].tolist() == [7, 9] and [int(v[0]) for v in probe.words(rec)] == [7, 9]


def test_null_arguments_are_refused(built):
    lib = probe.load()
    buf = (C.c_uint8 * 288)()
    err = lambda: lib.hiprz_probe_last_error(None)
    assert lib.hiprz_probe_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_probe_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_probe_gather(None, buf, 1, 0, buf, 4, 4, buf, buf, None) == _abi.ERR_INVALID and b"probe_gather: null probe" in err()
    assert lib.hiprz_probe_samples(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID and b"probe_samples: null probe" in err()
    assert lib.hiprz_probe_light(None, buf, 1, 0, None, None, buf, None) == _abi.ERR_INVALID and b"probe_light: null probe" in err()
    assert lib.hiprz_probe_gather_host(None, buf, 1, 0, buf, 4, 4, buf, buf) == _abi.ERR_INVALID and b"probe_gather_host: null probe" in err()
    assert lib.hiprz_probe_light_host(None, buf, 1, 0, None, None, buf) == _abi.ERR_INVALID and b"probe_light_host: null probe" in err()
    assert lib.hiprz_probe_set_directions(None, buf, 16, 1) == _abi.ERR_INVALID and b"probe_set_directions: null probe" in err()
    assert lib.hiprz_probe_set_samples(None, buf, 1, 1) == _abi.ERR_INVALID and b"probe_set_samples: null probe" in err()
    assert lib.hiprz_probe_set_charts(None, buf, 1, buf, 1) == _abi.ERR_INVALID and b"probe_set_charts: null probe" in err()
    assert lib.hiprz_probe_gather(None, buf, 0, 0, buf, 4, 4, buf, buf, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    lib.hiprz_probe_layout(None)          # nothing to write to: returns
    assert lib.hiprz_probe_sphere_directions(16, 1, None) == _abi.ERR_INVALID
    for name in ("prober", "bake_probes", "probe_samples", "bake_probe_field", "bake_bounce_atlas"):
        assert callable(getattr(Context, name)), name
    for name in ("set_directions", "set_samples", "set_charts", "gather", "light", "gather_device", "light_device", "samples_device", "samples", "bake_device", "bake"):
        assert callable(getattr(probe.Probe, name)), name
    assert callable(probe.sphere_directions) and callable(probe.irradiance) and callable(probe.grid) and callable(probe.Field)


def test_create_fails_loudly_without_a_gpu(built):
    lib = probe.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_probe_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_probe_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_probe_last_error(None)


def test_every_host_stub_of_the_probe_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; three kernels, and
    none of them in the eight libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "probe", "hiprz_probe.o"), probe.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 3
    for kernel in KERNELS:
        assert sum(kernel + "E" in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "probe", "hiprz_probe_host.o")) == set(), "the refusals, the checks, the table and the evaluation are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, light.LIB_PATH, gather.LIB_PATH, os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others), "a kernel of the probe library is in a library whose kernel set is pinned"
    assert not any("rz_probe" in name for name in others)
    assert all("N5hiprz" in name for name in found[lib]), "the probe kernels live in namespace hiprz"


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "probe", "hiprz_probe.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_query_device.hpp"' in code and "bool take_ray(" not in code, "the invalid-ray rule exists once"
    assert '#include "query/hiprz_session.hpp"' in code and "struct hiprz_probe : Session" in code, "the handle is built on the shared session"
    assert "take_ray(" in code and "closest_hit_skip<false, false, true>(" in code and "occluded_word(" in code and "HIPRZ_QUERY_NORMALIZE" in code
    assert "analyze_intersection" not in code and "closest_record" not in code, "no material, texture or normal is fetched for a hit"
    assert code.count("__global__") == 3 and "atomic" not in code and "__syncthreads" not in code, "three kernels, no atomics, no barrier"
    assert code.count("__shared__") == 1 and "RZ_PROBE_GATHER_IN_LDS" in code and "RZ_PROBE_LIGHT_IN_LDS" in code and re.search(r"#define\s+RZ_PROBE_SUMS\s+27\b", code), "one LDS array, in the kernels built to use it"
    assert "__launch_bounds__(RZ_PROBE_WG" in code and re.search(r"#define\s+RZ_PROBE_WG\s+64\b", code)
    assert len(re.findall(r"\bprobe_walk\(", code)) == 3 and len(re.findall(r"\bprobe_ray\(", code)) == 3, "the ray and the sample are each made by one function that both kernels call"
    assert len(re.findall(r"\bprobe_add\(", code)) == 3, "one step of the running sums for both terms and both placements"
    for f in ("sinf(", "cosf(", "acosf(", "expf(", "RZ_SINCOSF", "RZ_EXPF", "RZ_ACOSF", "__fmaf", "fmaf("):
        assert f not in code, f"{f} in the kernel unit: the rules are plain float32 with true / and sqrtf"
    for other in ("bake/", "atlas/", "light/", "gather/", "hiprz_atlas", "gather_walk(", "take_light_point("):
        assert other not in code, "nothing of the other libraries but their records' layouts: what it needs it restates"
    host = open(os.path.join(CSRC, "probe", "hiprz_probe_host.cpp")).read() + open(os.path.join(CSRC, "probe", "hiprz_probe_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"


_NULL, _TABLE, _MAP, _SIZE, _DISK = "null pointer", "no direction table has been set", "no chart map has been set", "n*K is 2^31 or more", "no sample table has been set"
_GATHERS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _TABLE), (_abi.ERR_STATE, _TABLE), (_abi.ERR_STATE, _MAP),
            (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE)]
_LIGHTS = [(_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _DISK), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE), (_abi.ERR_INVALID, _SIZE)]
_FINITE, _UNIT = "a direction is not finite", "a direction is not of unit length (squared length outside [0.999, 1.001])"
_K, _S = "K is not one of 16, 32, 64, 128, 256, 512, 1024", "S is not in 1..64"
_TABLES = [("good", "none"), ("nan", _FINITE), ("inf", _FINITE), ("nan w", "none"), ("long", _UNIT), ("below", "none"), ("K = 8", _K), ("K = 2048", _K), ("S = 0", _S), ("S = 65", _S),
           ("null", _NULL)]
_LK = "K is not a power of two in 1..1024"
_SAMPLES = [("good", "none"), ("K = 1", "none"), ("outside", "a sample lies outside the unit disk"), ("nan", "a sample is not finite"), ("K = 3", _LK), ("K = 2048", _LK), ("S = 0", _S),
            ("null", _NULL)]
_UV = "a chart's UV is not finite"
_CHARTS = [("good", "none"), ("empty", "none"), ("null base", _NULL), ("null uv", _NULL), ("too many", "more charts than there are ids below the codes"), ("inf", _UV), ("nan padding", "none")]
_WH = "W or H is not in 1..16384"
_SIZES = [("1 1", "none"), ("16384 16384", "none"), ("0 4", _WH), ("4 0", _WH), ("16385 1", _WH), ("1 16385", _WH), ("4294967295 4294967295", _WH)]
_RANGES = ["range null: none 0 3 0 2", "range: none 0 3 0 2", "range: none 1 2 2 0", "range: none 3 0 0 1", "range: the range starts behind the last spot light",
           "range: the range ends behind the last spot light", "range: the range starts behind the last direct light", "range: the range ends behind the last direct light"]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "probe_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "probe"), os.path.join(ROOT, "tests", "probe_host_main.cpp"), os.path.join(CSRC, "probe", "hiprz_probe_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    at = 0
    for expected in ([f"gather: {code} {why}" for code, why in _GATHERS], [f"light: {code} {why}" for code, why in _LIGHTS], [f"table {name}: {why}" for name, why in _TABLES],
                     [f"sphere refusals: {_abi.ERR_INVALID} {_abi.ERR_INVALID} {_abi.ERR_INVALID}", "sphere worst: ok"], [f"samples {name}: {why}" for name, why in _SAMPLES],
                     [f"charts {name}: {why}" for name, why in _CHARTS], [f"size {name}: {why}" for name, why in _SIZES], _RANGES):
        assert lines[at:at + len(expected)] == expected, (lines[at:at + len(expected)], expected)
        at += len(expected)
    # the evaluation: the module's vectorised float32 rule on the program's record and normal, bit for bit
    rec = np.zeros(1, probe.sh_dtype)
    for b in range(9):
        for c in range(3):
            rec["sh"][0, b, c] = np.float32(0.25) * np.float32(b + 1) - np.float32(0.5) * np.float32(c)
    want = probe.irradiance(rec, np.array([0.48, 0.6, 0.64], np.float32))[0]
    got = np.array([float.fromhex(v) for v in lines[at].split()[1:]], np.float32)
    assert lines[at].startswith("irradiance ") and got.tobytes() == want.tobytes(), (got, want)
    assert lines[at + 1] == "irradiance invalid 0x0p+0 0x0p+0 0x0p+0"
    want_hash = tuple(int(BR.hash32(x)[0]) for x in (0, 1, 0xFFFFFFFF))
    assert lines[at + 2:] == ["layout 32 144 16 32 12 28", "hash %d %d %d" % want_hash, "capacity 4096 8192 100"]
