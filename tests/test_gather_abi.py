"""Bounce baking at the C-ABI level, without a GPU: libhiprz_gather.so loads and exports exactly the symbols include/hiprz_gather.h declares,
gather.ENTRY_POINTS binds them, null arguments are refused, the library does not come up without a device, every host stub of the new
library has its gfx950 kernel — three of them, none in the seven other libraries — the kernel unit takes the ray rule and the walk from
the query's device header and makes a sample in one function, the library links against libhiprz.so alone, the chart tables of an atlas's
parts are what the header says, and the pure-host unit runs as a process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import bake_reference as BR
from rayzath_amd import _abi, _lib, atlas, bake, gather, light, order, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_gather.h")
KERNELS = ("rz_gather_kernel", "rz_gather_samples_kernel", "rz_gather_compose_kernel")
NAMES = ["hiprz_gather_" + n for n in ("compose", "compose_host", "create", "destroy", "last_error", "layout", "samples", "set_charts", "set_directions", "texels", "texels_host")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = gather.load()
    names = sorted(set(re.findall(r"\b(hiprz_gather_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_gather.h but not exported"
    assert set(names) == set(gather.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", gather.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_bake.h"' in header and "typedef struct hiprz_bake_point" not in header
    assert "x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;" in text
    assert "d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z" in text and "u  = (u1 * b1 + u2 * bx) + u3 * by" in text and "b1 = (1.0f - bx) - by" in text, "the parenthesisation is part of the contract"
    assert "out.c = (albedo.c * (direct.c + indirect.c)) + emission.c" in text
    for left_out in ("glossy transport", "transmission", "scattering medium"):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    for name, value in (("INVALID", gather.INVALID), ("NONE", gather.NONE), ("MISS", gather.MISS), ("UNMAPPED", gather.UNMAPPED), ("BACK", gather.BACK),
                        ("INVALID_RAY", gather.INVALID_RAY), ("MAX_CHARTS", gather.MAX_CHARTS)):
        assert re.search(r"#define\s+HIPRZ_GATHER_%s\s+0x%08Xu" % (name, value), header), name
    assert gather.INVALID == light.INVALID == bake.INVALID, "light and bake texels are sources as they are"
    assert min(gather.MISS, gather.UNMAPPED, gather.BACK, gather.INVALID_RAY) == gather.MAX_CHARTS, "chart ids lie below the codes"


def test_the_library_links_against_libhiprz_alone(built):
    needed = subprocess.run(["readelf", "-d", gather.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_gather\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*gather/\*\.o.*\blibhiprz_gather\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_gather") == 2, "libhiprz_host.so and hip_engine_test link the gather library"


def test_the_layout_is_the_mirrors(built):
    out = (C.c_uint32 * 8)()
    gather.load().hiprz_gather_layout(out)
    p, t, s, c = bake.point_dtype, gather.texel_dtype, gather.sample_dtype, gather.chart_dtype
    assert list(out) == [p.itemsize, t.itemsize, s.itemsize, c.itemsize, t.fields["counts"][1], s.fields["bx"][1], s.fields["t"][1], c.fields["u3"][1]]
    assert list(out) == [32, 16, 16, 32, 12, 4, 12, 16]
    assert gather.record_dtype.fields["word"][1] == 12 == light.texel_dtype.fields["shadowed"][1]


def test_null_arguments_are_refused(built):
    lib = gather.load()
    buf = (C.c_uint8 * 96)()
    err = lambda: lib.hiprz_gather_last_error(None)
    assert lib.hiprz_gather_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_gather_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_gather_texels(None, buf, 1, 0, buf, 4, 4, buf, buf, None) == _abi.ERR_INVALID and b"gather_texels: null gather" in err()
    assert lib.hiprz_gather_samples(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID and b"gather_samples: null gather" in err()
    assert lib.hiprz_gather_texels_host(None, buf, 1, 0, buf, 4, 4, buf, buf) == _abi.ERR_INVALID and b"gather_texels_host: null gather" in err()
    assert lib.hiprz_gather_compose(None, buf, buf, buf, buf, buf, 1, None) == _abi.ERR_INVALID and b"gather_compose: null gather" in err()
    assert lib.hiprz_gather_compose_host(None, buf, buf, buf, buf, buf, 1) == _abi.ERR_INVALID and b"gather_compose_host: null gather" in err()
    assert lib.hiprz_gather_set_directions(None, buf, 16, 1) == _abi.ERR_INVALID and b"gather_set_directions: null gather" in err()
    assert lib.hiprz_gather_set_charts(None, buf, 1, buf, 1) == _abi.ERR_INVALID and b"gather_set_charts: null gather" in err()
    assert lib.hiprz_gather_texels(None, buf, 0, 0, buf, 4, 4, buf, buf, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    lib.hiprz_gather_layout(None)         # nothing to write to: returns
    for name in ("gatherer", "gather", "gather_samples", "bake_bounce_atlas"):
        assert callable(getattr(Context, name)), name
    for name in ("set_directions", "set_charts", "texels", "texels_device", "samples_device", "samples", "compose_device", "compose"):
        assert callable(getattr(gather.Gather, name)), name
    assert callable(atlas.bake_bounce) and callable(gather.chart_tables)


def test_create_fails_loudly_without_a_gpu(built):
    lib = gather.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_gather_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_gather_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_gather_last_error(None)


def test_every_host_stub_of_the_gather_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; three kernels, and
    none of them in the seven libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "gather", "hiprz_gather.o"), gather.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 3
    for kernel in KERNELS:
        assert sum(kernel + "E" in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "gather", "hiprz_gather_host.o")) == set(), "the refusals, the checks and the layout are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, light.LIB_PATH, os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others), "a kernel of the gather library is in a library whose kernel set is pinned"
    assert not any("rz_gather" in name for name in others)
    assert all("N5hiprz" in name for name in found[lib]), "the gather kernels live in namespace hiprz"


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "gather", "hiprz_gather.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_query_device.hpp"' in code and "bool take_ray(" not in code, "the invalid-ray rule exists once"
    assert '#include "query/hiprz_session.hpp"' in code and "struct hiprz_gather : Session" in code, "the handle is built on the shared session"
    assert "take_ray(" in code and "closest_hit_skip<false, false, true>(" in code and "HIPRZ_QUERY_NORMALIZE" in code
    assert "analyze_intersection" not in code and "closest_record" not in code, "no material, texture or normal is fetched for a hit"
    assert code.count("__global__") == 3 and "__shared__" not in code and "atomic" not in code, "three kernels, no LDS, no atomics"
    assert "__launch_bounds__(RZ_GATHER_WG)" in code and re.search(r"#define\s+RZ_GATHER_WG\s+64\b", code)
    assert len(re.findall(r"\bgather_walk\(", code)) == 3 and len(re.findall(r"\bgather_ray\(", code)) == 3, "the ray and the sample are each made by one function that both kernels call"
    for f in ("sinf(", "cosf(", "acosf(", "expf(", "RZ_SINCOSF", "RZ_EXPF", "RZ_ACOSF", "__fmaf", "fmaf("):
        assert f not in code, f"{f} in the kernel unit: the rules are plain float32 with true / and sqrtf"
    for other in ("bake/", "atlas/", "light/", "hiprz_atlas", "hiprz_light"):
        assert other not in code, "nothing of the bake, atlas or light libraries but the point's layout"
    host = open(os.path.join(CSRC, "gather", "hiprz_gather_host.cpp")).read() + open(os.path.join(CSRC, "gather", "hiprz_gather_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in make and re.search(r"gather/hiprz_gather\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\)", make)


def test_chart_tables_follow_the_parts(built):
    rng = np.random.default_rng(3)

    def tris(n):
        t = np.zeros(n, atlas.tri_dtype)
        for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
            t[name] = rng.random(n)
        return t

    a, b = tris(5), tris(3)
    base, uv = gather.chart_tables([(2, a), (0, b)], 4)
    assert base.tolist() == [5, gather.NONE, 0, gather.NONE] and uv.dtype == gather.chart_dtype and len(uv) == 8
    for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
        assert np.array_equal(uv[name], np.concatenate([a[name], b[name]]))
    assert not uv["zero"].any()
    base, uv = gather.chart_tables([], 2)
    assert base.tolist() == [gather.NONE, gather.NONE] and len(uv) == 0
    with pytest.raises(ValueError):
        gather.chart_tables([(0, a), (0, b)], 1)
    with pytest.raises(ValueError):
        gather.chart_tables([(1, a)], 1)
    with pytest.raises(TypeError):
        gather.chart_tables([(0, np.zeros(3, np.float32))], 1)
    rec = gather.records((1.0, 0.5, 0.25), (2, 3))
    assert rec.dtype == gather.record_dtype and rec.shape == (2, 3) and rec["rgb"][1, 2].tolist() == [1.0, 0.5, 0.25] and not rec["word"].any()
    assert gather.records(rec, (2, 3)) is rec or gather.records(rec, (2, 3)).tobytes() == rec.tobytes()


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/gather/hiprz_gather_host.cpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 2**27)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**26, 2**26 + 1), (2**27, 2**27),
          (2**26 + 5, 2**27), (2**27 - 1, 2**27), (3, 2**27), (65536, 65537), (1, 60000)]
_NULL, _TABLE, _MAP, _SIZE = "null pointer", "no direction table has been set", "no chart map has been set", "n*K is 2^31 or more"
_REFUSALS = [(_abi.OK, "none"), (_abi.OK, "none"), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_INVALID, _NULL), (_abi.ERR_STATE, _TABLE),
             (_abi.ERR_STATE, _TABLE), (_abi.ERR_STATE, _MAP), (_abi.ERR_STATE, _MAP), (_abi.OK, "none"), (_abi.ERR_INVALID, _SIZE), (_abi.OK, "none"),
             (_abi.ERR_INVALID, _SIZE), (_abi.ERR_INVALID, _SIZE), (_abi.ERR_INVALID, _SIZE)]
_FINITE, _UNIT = "a direction is not finite", "a direction is not of unit length (squared length outside [0.999, 1.001])"
_K, _S = "K is not one of 16, 32, 64, 128, 256, 512, 1024", "S is not in 1..64"
_TABLES = [("good", "none"), ("nan", _FINITE), ("inf", _FINITE), ("nan w", "none"), ("long", _UNIT), ("short", _UNIT), ("below", "none"), ("K = 8", _K), ("K = 48", _K),
           ("K = 1024", "none"), ("K = 2048", _K), ("S = 0", _S), ("S = 65", _S), ("null", "null pointer")]
_UV = "a chart's UV is not finite"
_CHARTS = [("good", "none"), ("empty", "none"), ("no charts", "none"), ("no instances", "none"), ("null base", _NULL), ("null uv", _NULL),
           ("too many", "more charts than there are ids below the codes"), ("nan", _UV), ("inf", _UV), ("nan padding", "none")]
_WH = "W or H is not in 1..16384"
_SIZES = [("1 1", "none"), ("16384 16384", "none"), ("0 4", _WH), ("4 0", _WH), ("16385 1", _WH), ("1 16385", _WH), ("4294967295 4294967295", _WH)]
_COMPOSES = ["none", _NULL, "none", "2^31 texels or more", _NULL]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "gather_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "gather"), os.path.join(ROOT, "tests", "gather_host_main.cpp"), os.path.join(CSRC, "gather", "hiprz_gather_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}"
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
    at = len(_PAIRS)
    for expected in ([f"refusal: {code} {why}" for code, why in _REFUSALS], [f"table {name}: {why}" for name, why in _TABLES],
                     [f"charts {name}: {why}" for name, why in _CHARTS], [f"size {name}: {why}" for name, why in _SIZES], [f"compose: {why}" for why in _COMPOSES]):
        assert lines[at:at + len(expected)] == expected
        at += len(expected)
    want = tuple(int(BR.hash32(x)[0]) for x in (0, 1, 0xFFFFFFFF))
    assert lines[at:-1] == ["layout 32 16 16 32 12 4 12 16", "hash %d %d %d" % want]
    # the hash is the bake's: a point uses the same set in both libraries
    assert [bake.set_of(i, 77, 5) for i in range(40)] == [int(BR.hash32(i ^ 77)[0]) % 5 for i in range(40)]
