"""Probe fields at the C-ABI level, without a GPU: libhiprz_field.so loads and exports exactly the symbols include/hiprz_field.h declares,
field.ENTRY_POINTS binds them, the header writes the rules out, the layout is the mirrors', the pure host calls answer, null arguments are
refused, the library does not come up without a device, every host stub of the new library has its gfx950 kernel — two kernels, in none
of the ten other libraries —, the library links against libhiprz.so alone, and the pure-host unit runs as a process of its own under
sanitizers: the table check, every refusal in the header's order, the grid and params checks, the texel directions."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bake_reference as BR
from rayzath_amd import _abi, _lib, atlas, bake, field, gather, light, order, probe, query, smooth
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_field.h")
NAMES = ["hiprz_field_" + n for n in ("check_grid", "check_params", "create", "destroy", "last_error", "layout", "lookup", "lookup_host", "set_directions", "texel_directions",
                                      "visibility", "visibility_host")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = field.load()
    names = sorted(set(re.findall(r"\b(hiprz_field_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_field.h but not exported"
    assert set(names) == set(field.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", field.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_probe.h"' in header and "typedef struct hiprz_bake_point" not in header and "typedef struct hiprz_probe_sh" not in header
    for rule in ("c  = max(0, (o.x*d.x + o.y*d.y) + o.z*d.z)", "w = c*c; w = w*w; w = w*w; w = w*w; w = w*w", "sw = sw + w", "s1 = s1 + (w * r)", "s2 = s2 + (w * (r * r))",
                 "r = min(t, reach)", "e = ((ix + 0.5) / 4 - 1, (iy + 0.5) / 4 - 1)", "g = (p.a - lo.a) / step.a", "i = min(int(floorf(g)), n[a] - 2)", "tri = (wx * wy) * wz",
                 "q.c = p.c + (bias * n.c)", "dist = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)", "wb = (b * b) + 0.2f", "s = (|x| + |y|) + |z|",
                 "fx = (1.0f - |ey|) * copysignf(1, ex)", "var = fabsf(mean2 - mean*mean)", "ch = var / (var + dd*dd)", "ch = (ch*ch)*ch", "w = max(wb * ch, 1e-6f)",
                 "w = w * ((w*w) * 25.0f)", "acc.c = acc.c + (w * E.c)", "(i * n[1] + j) * n[2] + k"):
        assert rule in text, f"the parenthesisation is part of the contract: {rule}"
    for left_out in ("probe placement", "a bilinear tap", "an irregular or sparse grid", "blending the coefficients"):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    assert re.search(r"#define\s+HIPRZ_FIELD_INVALID\s+0x%08Xu" % field.INVALID, header) and field.INVALID == probe.INVALID
    assert re.search(r"#define\s+HIPRZ_FIELD_TEXELS\s+%du" % field.TEXELS, header)
    # the probe header points here, and still says what its own library leaves out
    probe_text = open(os.path.join(ROOT, "include", "hiprz_probe.h")).read()
    assert probe_text.count("hiprz_field.h") >= 2 and "probe placement and visibility" in probe_text and "device-side evaluation kernel" in probe_text


def test_the_library_links_against_libhiprz_alone(built):
    needed = subprocess.run(["readelf", "-d", field.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_field\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*field/\*\.o.*\blibhiprz_field\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_field") == 2, "libhiprz_host.so and hip_engine_test link the field library"
    assert re.search(r"^hip_engine_test:.*\blibhiprz_field\.so\b", make, flags=re.M) and re.search(r"^libhiprz_host\.so:.*\blibhiprz_field\.so\b", make, flags=re.M)
    assert re.search(r"^FIELD_DEFS \?=\s*$", make, flags=re.M)
    assert "-ffp-contract=off" in make and re.search(r"field/hiprz_field\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\) \$\(FIELD_DEFS\)", make)
    host = subprocess.run(["readelf", "-d", os.path.join(CSRC, "libhiprz_host.so")], check=True, capture_output=True, text=True).stdout
    assert "libhiprz_field.so" in host


def test_the_layout_is_the_mirrors(built):
    out = field.layout()
    assert out[:7] == [bake.point_dtype.itemsize, probe.sh_dtype.itemsize, field.vis_dtype.itemsize, field.grid_dtype.itemsize, field.params_dtype.itemsize,
                       field.result_dtype.itemsize, field.vis_dtype.fields["words"][1]] == [32, 144, 528, 40, 16, 16, 512]
    assert out[7] in (64, 256)
    p = field.params(bias=0.25, max_back=7)
    assert p.tobytes() == np.array([0.25], np.float32).tobytes() + np.array([7, 0, 0], np.uint32).tobytes()
    assert field._params(None)["max_back"] == 0 and field._params(dict(bias=0.5))["bias"] == 0.5 and field._params(p) is not None
    g = field.grid_of((-2.0, 0.25, -2.0), (2.0, 2.25, 2.0), (5, 3, 5))
    assert g.tobytes() == np.array([-2.0, 0.25, -2.0, 1.0, 1.0, 1.0], np.float32).tobytes() + np.array([5, 3, 5, 0], np.uint32).tobytes()
    flat = field.grid_of((0, 0, 0), (1, 0, 0), (3, 1, 1))
    assert flat["step"].tolist() == [0.5, 0.0, 0.0]
    with pytest.raises(TypeError):
        field._params(np.zeros(2, field.params_dtype))
    with pytest.raises(TypeError):
        field._grid(np.zeros(2, field.grid_dtype))


def test_the_pure_host_calls(built):
    lib = field.load()
    assert lib.hiprz_field_texel_directions(None) == _abi.ERR_INVALID
    t = field.texel_directions()
    assert t.shape == (64, 4) and np.abs(np.linalg.norm(t[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6 and not t[:, 3].any()
    assert lib.hiprz_field_check_params(None) == _abi.ERR_INVALID and lib.hiprz_field_check_grid(None, 1) == _abi.ERR_INVALID
    for bias in (np.nan, -1.0, -1e-30, np.inf):
        with pytest.raises(ValueError):
            field.params(bias=bias)
    with pytest.raises(ValueError):
        field.params(max_back=-1)
    for lo, hi, shape in (((0, 0, 0), (1, 1, 1), (2, 0, 2)), ((0, 0, 0), (0, 1, 1), (2, 2, 2)), ((0, 0, 0), (-1, 1, 1), (2, 2, 2)), ((0, 0, 0), (np.inf, 1, 1), (2, 2, 2)),
                          ((np.nan, 0, 0), (1, 1, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1), (2 ** 11, 2 ** 10, 2 ** 10))):
        with pytest.raises(ValueError):
            field.grid_of(lo, hi, shape)
    g = field.grid_of((0, 0, 0), (1, 1, 1), (2, 3, 4))
    assert lib.hiprz_field_check_grid(g.ctypes.data, 24) == _abi.OK and lib.hiprz_field_check_grid(g.ctypes.data, 23) == _abi.ERR_INVALID


def test_null_arguments_are_refused(built):
    lib = field.load()
    buf = (C.c_uint8 * 64)()
    err = lambda: lib.hiprz_field_last_error(None)
    assert lib.hiprz_field_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_field_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_field_set_directions(None, buf, 64, 1) == _abi.ERR_INVALID and b"field_set_directions: null field" in err()
    assert lib.hiprz_field_visibility(None, buf, 1, 0, 1.0, buf, None) == _abi.ERR_INVALID and b"field_visibility: null field" in err()
    assert lib.hiprz_field_visibility_host(None, buf, 1, 0, 1.0, buf) == _abi.ERR_INVALID and b"field_visibility_host: null field" in err()
    assert lib.hiprz_field_lookup(None, buf, buf, buf, None, 1, buf, buf, 1, buf, None) == _abi.ERR_INVALID and b"field_lookup: null field" in err()
    assert lib.hiprz_field_lookup_host(None, buf, buf, buf, None, 1, buf, buf, 1, buf) == _abi.ERR_INVALID and b"field_lookup_host: null field" in err()
    lib.hiprz_field_layout(None)          # nothing to write to: returns
    for name in ("fielder", "bake_visibility", "lookup_field", "bake_probe_field"):
        assert callable(getattr(Context, name)), name
    for name in ("set_directions", "visibility", "visibility_device", "lookup", "lookup_device"):
        assert callable(getattr(field.Fielder, name)), name
    assert inspect.signature(Context.bake_probe_field).parameters["visibility"].default is None
    assert inspect.signature(Context.bake_visibility).parameters["directions"].default == (256, 4)


def test_create_fails_loudly_without_a_gpu(built):
    lib = field.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_field_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_field_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_field_last_error(None)


def test_every_host_stub_of_the_field_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; two kernels, and
    neither in the ten libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "field", "hiprz_field.o"), field.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 2
    assert sorted(re.search(r"rz_field_\w+?_kernel", name).group(0) for name in found[lib]) == ["rz_field_lookup_kernel", "rz_field_visibility_kernel"], found[lib]
    assert ck.host_stubs(os.path.join(CSRC, "field", "hiprz_field_host.o")) == set(), "the refusals, the checks and the layout are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, light.LIB_PATH, gather.LIB_PATH, probe.LIB_PATH, smooth.LIB_PATH,
                 os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others) and not any("rz_field" in name for name in others)


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "field", "hiprz_field.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_session.hpp"' in code and '#include "query/hiprz_query_device.hpp"' in code and "struct hiprz_field : Session" in code
    assert code.count("__global__") == 2 and "atomic" not in code, "two kernels, no atomics"
    assert code.count("__shared__") == 1 and "__shared__ float4 rows[RZ_FIELD_WG]" in code, "one LDS array: a float4 per lane, 1 KB per wave"
    assert code.count("__syncthreads()") == 2, "the rows are written, read by every lane, and only then overwritten"
    assert code.count("closest_hit_skip<false, false, true>") == 1 and "take_ray(r0, r1, 0u, ray)" in code, "the query's closest-hit walk without NORMALIZE"
    lookup = code[code.index("rz_field_lookup_kernel"):code.index("using namespace hiprz;")]
    assert "__shared__" not in lookup and "__syncthreads" not in lookup and "__ballot" not in lookup, "the lookup shares nothing"
    for f in ("expf(", "powf(", "sinf(", "cosf(", "acosf(", "__fmaf", "fmaf(", "__fdividef", "__frcp", "rsqrtf("):
        assert f not in code, f"{f} in the kernel unit: the rule is plain float32 with true division and sqrtf"
    for other in ("bake/", "atlas/", "light/", "gather/", "probe/", "smooth/", "hiprz_probe_host", "probe_point", "probe_ray"):
        assert other not in code, "what the library needs of the probe's frame, hash and ray it restates"
    assert code.count("hiprz_device_view") == 0 and len(re.findall(r"\bview\(h, what, s\)", code)) == 2, "the bake takes a view on every call, the lookup none"
    host = open(os.path.join(CSRC, "field", "hiprz_field_host.cpp")).read() + open(os.path.join(CSRC, "field", "hiprz_field_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"
    assert "RZ_FIELD_LOOKUP_WG" in host
    # the hash is the bake's
    assert [int(BR.hash32(x)[0]) for x in (0, 1, 0xFFFFFFFF)] == [0, 1753845952, 1734902346]


_K = "K is not one of 64, 128, 256, 512, 1024"
_S = "S is not in 1..64"
_UNIT = "a direction is not of unit length (squared length outside [0.999, 1.001])"
_REACH = "reach is not a finite number > 0"
_STEP = "a grid step is not a finite number > 0"
_MANY = "the grid has 2^31 probes or more"
_BIAS = "bias is not a finite number >= 0"
_EXPECTED = (["table: none", "table: null pointer"] + [f"table K {K}: {_K}" for K in (0, 16, 32, 63, 96, 2048)] + [f"table S {S}: {_S}" for S in (0, 65)]
             + ["table: a direction is not finite", f"table: {_UNIT}", "table: none"]
             + [f"bake: {code} {why}" for code, why in [(_abi.OK, "none")] * 2 + [(_abi.ERR_INVALID, "null pointer"), (_abi.ERR_STATE, "no direction table has been set"),
                                                                                    (_abi.ERR_INVALID, "n*K is 2^31 or more"), (_abi.OK, "none")] + [(_abi.ERR_INVALID, _REACH)] * 4]
             + [f"grid: {_abi.OK} none", f"grid: {_abi.ERR_INVALID} the grid's counts do not multiply to the number of probes", f"grid: {_abi.ERR_INVALID} null grid",
                "grid: a grid count is 0", f"grid: {_MANY}", f"grid: {_MANY}", "grid: none"] + [f"grid step: {_STEP}"] * 4 + ["grid: none", "grid: the grid's corner is not finite"]
             + [f"params: {_abi.OK} none"] * 4 + [f"params: {_abi.ERR_INVALID} {_BIAS}"] * 3 + [f"params null: {_abi.ERR_INVALID}"]
             + [f"lookup: {why}" for why in ("none", "none", "null pointer", _STEP, _BIAS, "2^31 points or more", "none")]
             + [f"texels: {_abi.OK} {_abi.ERR_INVALID}", "texels: 24 up 24 down unit 1", "hash 0 1753845952 1734902346", "allowed 1 1 0 0 1 0",
                "capacity 4096 8192 100 2147483648", "layout 32 144 528 40 16 16 512"])


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "field_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "field"), os.path.join(ROOT, "tests", "field_host_main.cpp"), os.path.join(CSRC, "field", "hiprz_field_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines == _EXPECTED, [(a, b) for a, b in zip(lines, _EXPECTED) if a != b]
