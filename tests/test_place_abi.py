"""Probe placement at the C-ABI level, without a GPU: libhiprz_place.so loads and exports exactly the symbols include/hiprz_place.h declares,
place.ENTRY_POINTS binds them, the header writes the rule out, the layout is the mirrors', hiprz_place_check_params refuses case by case,
null arguments are refused, the library does not come up without a device, every host stub of the new library has its gfx950 kernel — one
kernel, in none of the eleven other libraries —, the library links against libhiprz.so alone, and the pure-host unit runs as a process of
its own under sanitizers: the table check, the params check, every refusal in the header's order."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bake_reference as BR
from rayzath_amd import _abi, _lib, atlas, bake, field, gather, light, order, place, probe, query, smooth
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_place.h")
NAMES = ["hiprz_place_" + n for n in ("check_params", "create", "destroy", "last_error", "layout", "probes", "probes_host", "set_directions")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = place.load()
    names = sorted(set(re.findall(r"\b(hiprz_place_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_place.h but not exported"
    assert set(names) == set(place.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", place.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_bake.h"' in header and "typedef struct hiprz_bake_point" not in header
    for rule in ("r = min(t, reach)", "r = reach", "INSIDE (2)   when n_back > max_back", "NEAR (1)     otherwise, when F exists and r_F < min_front", "ties going to the LOWEST k",
                 "s = r_B + (0.5f * min_front)", "m.a = d_B.a * s", "(d_O.x*d_F.x + d_O.y*d_F.y) + d_O.z*d_F.z <= 0.5f", "s = min(min_front - r_F, 0.5f * r_O)", "m.a = d_O.a * s",
                 "o'.a = o.a + m.a", "|o'.a| > max_offset[a]", "P.a = H.a + o.a", "d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z", "hiprz_bake_hash(i ^ seed) % S",
                 "(bits of r << 32) | k", "(~bits of r << 32) | k", "at most iterations + 1 evaluations", "the bytes of H when no move was made"):
        assert rule in text, f"the rule is part of the contract: {rule}"
    for left_out in ("a search over several directions", "moving a probe across cells", "re-baking", 'classified "off"'):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    for name, value in (("CLEAR", place.CLEAR), ("NEAR", place.NEAR), ("INSIDE", place.INSIDE), ("MAX_ITERATIONS", place.MAX_ITERATIONS)):
        assert re.search(r"#define\s+HIPRZ_PLACE_%s\s+%du" % (name, value), header), name
    assert re.search(r"#define\s+HIPRZ_PLACE_STUCK\s+0x%xu" % place.STUCK, header) and re.search(r"#define\s+HIPRZ_PLACE_INVALID\s+0x%08xu" % place.INVALID, header)
    assert re.search(r"#define\s+HIPRZ_PLACE_STATE_MASK\s+0x%xu" % place.STATE_MASK, header)
    # the field and the probe header point here
    for other in ("hiprz_field.h", "hiprz_probe.h"):
        assert "hiprz_place.h" in open(os.path.join(ROOT, "include", other)).read(), other


def test_the_library_links_against_libhiprz_alone(built):
    needed = subprocess.run(["readelf", "-d", place.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_place\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*place/\*\.o.*\blibhiprz_place\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_place") == 2, "libhiprz_host.so and hip_engine_test link the placement library"
    assert re.search(r"^hip_engine_test:.*\blibhiprz_place\.so\b", make, flags=re.M) and re.search(r"^libhiprz_host\.so:.*\blibhiprz_place\.so\b", make, flags=re.M)
    assert re.search(r"^PLACE_DEFS \?=\s*$", make, flags=re.M)
    assert "-ffp-contract=off" in make and re.search(r"place/hiprz_place\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\) \$\(PLACE_DEFS\)", make)
    host = subprocess.run(["readelf", "-d", os.path.join(CSRC, "libhiprz_host.so")], check=True, capture_output=True, text=True).stdout
    assert "libhiprz_place.so" in host


def test_the_layout_is_the_mirrors(built):
    fields = place.params_dtype.fields, place.record_dtype.fields
    assert place.layout() == [bake.point_dtype.itemsize, place.params_dtype.itemsize, place.record_dtype.itemsize, fields[0]["max_offset"][1], fields[0]["iterations"][1],
                              fields[0]["max_back"][1], fields[1]["word"][1], fields[1]["front"][1]] == [32, 32, 32, 8, 20, 24, 12, 16]
    assert list(place.params_dtype.names) == ["min_front", "reach", "max_offset", "iterations", "max_back", "reserved"]
    assert list(place.record_dtype.names) == ["offset", "word", "front", "back", "n_back", "n_front"]
    p = place.params(0.25, 4.0, (0.1, 0.2, 0.3), 3, 7)
    assert p.tobytes() == np.array([0.25, 4.0, 0.1, 0.2, 0.3], np.float32).tobytes() + np.array([3, 7, 0], np.uint32).tobytes()
    assert place.params(0.25, 4.0, 0.5, 3, 7)["max_offset"].tolist() == [0.5, 0.5, 0.5]
    assert place._params(p, 64) is not None and place._params(place.params(0.25, 4.0, 0.5), 512)["max_back"] == 128
    with pytest.raises(TypeError):
        place._params(np.zeros(2, place.params_dtype), 64)
    with pytest.raises(TypeError):
        place._probes(np.zeros(2, np.float32))


def test_check_params_case_by_case(built):
    lib = place.load()
    assert lib.hiprz_place_check_params(None) == _abi.ERR_INVALID
    good = place.params(0.2, 4.0, (0.36, 0.0, 3.0e38), 16, 2 ** 32 - 1)
    assert lib.hiprz_place_check_params(good.ctypes.data) == _abi.OK

    def verdict(**changes):
        p = good.copy()
        for k, v in changes.items():
            p[k] = v
        return lib.hiprz_place_check_params(p.ctypes.data)

    for name in ("min_front", "reach"):
        for v in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            assert verdict(**{name: v}) == _abi.ERR_INVALID, (name, v)
        assert verdict(**{name: 1.0e-30}) == _abi.OK and verdict(**{name: 3.0e38}) == _abi.OK
    for a in range(3):
        for v in (-1.0e-30, np.nan, np.inf):
            offset = good["max_offset"].copy()
            offset[a] = v
            assert verdict(max_offset=offset) == _abi.ERR_INVALID, (a, v)
    assert verdict(max_offset=(0.0, -0.0, 0.0)) == _abi.OK, "a box of nothing is a box: every move is STUCK"
    assert verdict(iterations=0) == _abi.OK and verdict(iterations=16) == _abi.OK and verdict(iterations=17) == _abi.ERR_INVALID and verdict(iterations=2 ** 32 - 1) == _abi.ERR_INVALID
    assert verdict(max_back=0) == _abi.OK
    assert verdict(reserved=1) == _abi.ERR_INVALID and verdict(reserved=2 ** 31) == _abi.ERR_INVALID
    for bad in (dict(min_front=np.nan), dict(reach=0.0), dict(max_offset=-1.0), dict(iterations=17), dict(iterations=-1), dict(max_back=-1)):
        with pytest.raises(ValueError):
            place.params(**{**dict(min_front=0.2, reach=4.0, max_offset=0.1), **bad})


def test_null_arguments_are_refused(built):
    lib = place.load()
    buf = (C.c_uint8 * 64)()
    err = lambda: lib.hiprz_place_last_error(None)
    assert lib.hiprz_place_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_place_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_place_set_directions(None, buf, 64, 1) == _abi.ERR_INVALID and b"place_set_directions: null place" in err()
    assert lib.hiprz_place_probes(None, buf, 1, 0, buf, buf, buf, None) == _abi.ERR_INVALID and b"place_probes: null place" in err()
    assert lib.hiprz_place_probes_host(None, buf, 1, 0, buf, buf, buf) == _abi.ERR_INVALID and b"place_probes_host: null place" in err()
    lib.hiprz_place_layout(None)          # nothing to write to: returns
    for name in ("placer", "place_probes", "bake_probe_field"):
        assert callable(getattr(Context, name)), name
    for name in ("set_directions", "probes", "probes_device", "probes_through_device"):
        assert callable(getattr(place.Placer, name)), name
    assert inspect.signature(Context.bake_probe_field).parameters["place"].default is None
    assert list(inspect.signature(Context.bake_probe_field).parameters)[-2:] == ["visibility", "place"], "the new keyword comes last: no caller's positions move"
    assert inspect.signature(Context.place_probes).parameters["directions"].default == (256, 4)
    assert inspect.signature(place.params).parameters["iterations"].default == 4 and inspect.signature(place.params).parameters["max_back"].default is None


def test_create_fails_loudly_without_a_gpu(built):
    lib = place.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_place_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_place_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_place_last_error(None)


def test_every_host_stub_of_the_place_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; one kernel, and
    not in the eleven libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "place", "hiprz_place.o"), place.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 1
    assert "rz_place_kernel" in next(iter(found[lib])), found[lib]
    assert ck.host_stubs(os.path.join(CSRC, "place", "hiprz_place_host.o")) == set(), "the refusals, the checks and the layout are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, light.LIB_PATH, gather.LIB_PATH, probe.LIB_PATH, smooth.LIB_PATH, field.LIB_PATH,
                 os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others) and not any("rz_place" in name for name in others)


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "place", "hiprz_place.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_session.hpp"' in code and '#include "query/hiprz_query_device.hpp"' in code and "struct hiprz_place : Session" in code
    assert code.count("__global__") == 1 and "atomic" not in code and "__shared__" not in code and "__syncthreads" not in code, "one kernel, no atomics, no LDS"
    assert code.count("closest_hit_skip<false, false, true>") == 1 and "take_ray(r0, r1, 0u, ray)" in code, "the query's closest-hit walk without NORMALIZE"
    assert "__shfl_xor(key, off, RZ_PLACE_WG)" in code and code.count("__ballot(") == 2, "the selections by a butterfly, the counts by ballots"
    kernel = code[code.index("__global__"):code.index("using namespace hiprz;")]
    assert "return" not in kernel[:kernel.index("if (!inside || lane != 0u) return;")], "nothing returns before the last ballot and shuffle"
    for f in ("expf(", "powf(", "sinf(", "cosf(", "acosf(", "__fmaf", "fmaf(", "__fdividef", "__frcp", "rsqrtf("):
        assert f not in code, f"{f} in the kernel unit: the rule is plain float32"
    for other in ("bake/", "atlas/", "light/", "gather/", "probe/", "smooth/", "field/", "hiprz_field", "hiprz_probe_host", "field_walk", "field_probe"):
        assert other not in code, "what the library needs of the probe's frame, hash and ray it restates"
    assert code.count("hiprz_device_view") == 0 and len(re.findall(r"\bview\(h, what, s\)", code)) == 2, "both calls take a view, on every call"
    host = open(os.path.join(CSRC, "place", "hiprz_place_host.cpp")).read() + open(os.path.join(CSRC, "place", "hiprz_place_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"
    # the hash is the bake's
    assert [int(BR.hash32(x)[0]) for x in (0, 1, 0xFFFFFFFF)] == [0, 1753845952, 1734902346]


_K = "K is not one of 64, 128, 256, 512, 1024"
_S = "S is not in 1..64"
_UNIT = "a direction is not of unit length (squared length outside [0.999, 1.001])"
_FRONT = "min_front is not a finite number > 0"
_REACH = "reach is not a finite number > 0"
_OFFSET = "a max_offset is not a finite number >= 0"
_BAD = _abi.ERR_INVALID
_EXPECTED = (["table: none", "table: null pointer"] + [f"table K {K}: {_K}" for K in (0, 16, 32, 63, 96, 2048)] + [f"table S {S}: {_S}" for S in (0, 65)]
             + ["table: a direction is not finite", f"table: {_UNIT}", "table: none"]
             + [f"params: {_abi.OK} none", f"params: {_BAD} null params"] + [f"min_front: {_BAD} {_FRONT}"] * 5 + [f"reach: {_BAD} {_REACH}"] * 4
             + [f"max_offset {a}: {_BAD} {_OFFSET}" for a in range(3) for _ in range(3)]
             + [f"params: {_abi.OK} none", f"iterations: {_BAD} iterations is above 16", f"reserved: {_BAD} reserved is not 0", f"params: {_BAD} {_FRONT}"]
             + [f"place: {code} {why}" for code, why in [(_abi.OK, "none")] * 2 + [(_BAD, "null pointer"), (_abi.ERR_STATE, "no direction table has been set"),
                                                                                     (_BAD, "n*K is 2^31 or more"), (_BAD, _REACH), (_abi.OK, "none"), (_BAD, "null params")]]
             + ["hash 0 1753845952 1734902346", "allowed 1 1 0 0 1 0", "capacity 4096 8192 100 2147483648", "layout 32 32 32 8 20 24 12 16"])


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "place_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "place"), os.path.join(ROOT, "tests", "place_host_main.cpp"), os.path.join(CSRC, "place", "hiprz_place_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines == _EXPECTED, [(a, b) for a, b in zip(lines, _EXPECTED) if a != b]
