"""The baked view at the C-ABI level, without a GPU: libhiprz_view.so loads and exports exactly the symbols include/hiprz_view.h declares,
view.ENTRY_POINTS binds them, the header writes the rule out, the layout is the mirrors', hiprz_view_check_params refuses case by case,
null arguments are refused, the library does not come up without a device, every host stub of the new library has its gfx950 kernel — two
kernels, in none of the twelve other libraries —, the library links against libhiprz.so alone, the Makefile builds it with VIEW_DEFS, and
the pure-host unit runs as a process of its own under sanitizers: the chart check, the params check, every refusal in the header's order."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from rayzath_amd import _abi, _lib, atlas, bake, field, gather, light, order, place, probe, query, smooth, view
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_view.h")
NAMES = ["hiprz_view_" + n for n in ("check_params", "create", "destroy", "last_error", "layout", "pixels", "pixels_host", "samples", "set_charts")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = view.load()
    names = sorted(set(re.findall(r"\b(hiprz_view_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_view.h but not exported"
    assert set(names) == set(view.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", view.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    header, text = _header(), open(HEADER).read()
    assert '#include "hiprz_gather.h"' in header and '#include "hiprz_field.h"' in header
    assert "typedef struct hiprz_gather_chart" not in header and "typedef struct hiprz_field_grid" not in header
    for rule in ("hiprz_query_pixel_rays", "WITHOUT HIPRZ_QUERY_NORMALIZE", "b1 = (1.0f - bx) - by", "u  = (u1 * b1 + u2 * bx) + u3 * by",
                 "x = clamp(int(floorf(u * float(W))), 0, W - 1)", "gx = u * float(W) - 0.5f", "x0 = int(floorf(gx))", "fx = gx - floorf(gx)", "clamped to [-1, W]",
                 "(x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1)", "w = wx * wy", "wx = 1.0f - fx for x0 and fx for x0 + 1", "is LEFT OUT", "acc.c = acc.c + (w * rgb.c)",
                 "sw = sw + w", "acc.c / sw when sw > 0", "0x80000000", "p.c = o.c + (t * d.c)", "hiprz_hit::normal", "hiprz_field_lookup writes", "rgb.c = color.c * E.c",
                 "rgb.c = (color.c * E.c) + (color.c * emission)", "A hit on a mapped id fetches no material", "kind SKY", "kind BACK", "word = kind << 28 | count",
                 "(r, g, b, 1.0f)", "hiprz_tonemap_image", "hiprz_denoise_image", "8 x 8", "VIEW_DEFS=-DRZ_VIEW_ROWS", "no LDS, no atomics"):
        assert rule in text, f"the rule is part of the contract: {rule}"
    for left_out in ("supersampling and depth of field", "glossy, transmissive and scattering", "shadows cast by unmapped objects onto the atlas", "mip-mapping of the atlas",
                     "a headless task key"):
        assert left_out in text, f"the header does not say that it leaves out: {left_out}"
    for name, value in (("NEAREST", view.NEAREST), ("BILINEAR", view.BILINEAR), ("NONE", view.NONE), ("ATLAS", view.ATLAS), ("FIELD", view.FIELD), ("SKY", view.SKY),
                        ("BACK", view.BACK), ("KIND_SHIFT", view.KIND_SHIFT)):
        assert re.search(r"#define\s+HIPRZ_VIEW_%s\s+%du" % (name, value), header), name
    assert re.search(r"#define\s+HIPRZ_VIEW_COUNT_MASK\s+0x%08Xu" % view.COUNT_MASK, header)
    # the refusals stand in the header in the order the calls make them
    order_ = [text.index(s) for s in ("a null handle or pointer —", "no chart map set (HIPRZ_ERR_STATE)", "a W or H outside 1 .. HIPRZ_GATHER_MAX_SIZE", "params hiprz_view_check_params refuses",
                                      "a grid hiprz_field_check_grid refuses", "hiprz_field_check_params refuses (HIPRZ_ERR_INVALID)", "whatever hiprz_device_view refuses",
                                      "more than 2^31 - 1 pixels", "a chart map for another number")]
    assert order_ == sorted(order_)


def test_the_library_links_against_libhiprz_alone_and_the_makefile_builds_it(built):
    needed = subprocess.run(["readelf", "-d", view.LIB_PATH], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(libhiprz[^\]]*)\]", needed)
    assert libs == ["libhiprz.so"], libs
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\blibhiprz_view\.so\b", make, flags=re.M) and re.search(r"^\trm -f .*view/\*\.o.*\blibhiprz_view\.so\b", make, flags=re.M)
    assert make.count("-lhiprz_view") == 2, "libhiprz_host.so and hip_engine_test link the view library"
    assert re.search(r"^hip_engine_test:.*\blibhiprz_view\.so\b", make, flags=re.M) and re.search(r"^libhiprz_host\.so:.*\blibhiprz_view\.so\b", make, flags=re.M)
    assert re.search(r"^VIEW_DEFS \?=\s*$", make, flags=re.M)
    assert "-ffp-contract=off" in make and re.search(r"view/hiprz_view\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(HIPFLAGS\) \$\(VIEW_DEFS\)", make)
    assert re.search(r"view/hiprz_view_host\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(VIEW_DEFS\)", make), "the layout reports the build: the host unit sees VIEW_DEFS too"
    assert re.search(r"^libhiprz_view\.so:.*\n\t.*-L\. -lhiprz -Wl,-rpath,'\$\$ORIGIN'\n\tmv -f \$@\.tmp \$@", make, flags=re.M), "linked under another name and renamed into place"
    host = subprocess.run(["readelf", "-d", os.path.join(CSRC, "libhiprz_host.so")], check=True, capture_output=True, text=True).stdout
    assert "libhiprz_view.so" in host


def test_the_layout_is_the_mirrors(built):
    assert view.layout() == [view.pixel_dtype.itemsize, view.params_dtype.itemsize, C.sizeof(view.FieldStruct), gather.sample_dtype.itemsize, gather.chart_dtype.itemsize,
                             view.pixel_dtype.fields["word"][1], view.KIND_SHIFT, 0] == [16, 16, 48, 16, 32, 12, 28, 0], "the shipped build maps a wave to an 8 x 8 block"
    assert list(view.pixel_dtype.names) == ["rgb", "word"] and list(view.params_dtype.names) == ["filter", "reserved"]
    assert [f[0] for f in view.FieldStruct._fields_] == ["grid", "probes", "sh", "vis", "n_probes", "params"]
    assert view.params().tobytes() == np.array([0, 0, 0, 0], np.uint32).tobytes() and view.params("bilinear").tobytes() == np.array([1, 0, 0, 0], np.uint32).tobytes()
    assert view._params("bilinear")["filter"] == view.BILINEAR and view._params(dict(filter="nearest"))["filter"] == view.NEAREST and view._params(None)["filter"] == view.NEAREST
    assert view._params(view.params(view.BILINEAR))["filter"] == view.BILINEAR
    with pytest.raises(TypeError):
        view._params(np.zeros(2, view.params_dtype))
    records = np.zeros(3, view.pixel_dtype)
    records["word"] = [(view.ATLAS << 28) | 4, (view.FIELD << 28) | 8, view.SKY << 28]
    assert view.kind(records).tolist() == [view.ATLAS, view.FIELD, view.SKY] and view.count(records).tolist() == [4, 8, 0]
    assert (view.NONE, view.ATLAS, view.FIELD, view.SKY, view.BACK) == (0, 1, 2, 3, 4)


def test_check_params_case_by_case(built):
    lib = view.load()
    assert lib.hiprz_view_check_params(None) == _abi.ERR_INVALID
    p = view.params("bilinear").copy()
    assert lib.hiprz_view_check_params(p.ctypes.data) == _abi.OK
    for f, want in ((0, _abi.OK), (1, _abi.OK), (2, _abi.ERR_INVALID), (2 ** 32 - 1, _abi.ERR_INVALID)):
        p["filter"] = f
        assert lib.hiprz_view_check_params(p.ctypes.data) == want, f
    p["filter"] = 0
    for k in range(3):
        q = p.copy()
        q["reserved"][k] = 1
        assert lib.hiprz_view_check_params(q.ctypes.data) == _abi.ERR_INVALID, k
    for bad in ("trilinear", 2, -1):
        with pytest.raises(ValueError):
            view.params(bad)


def test_null_arguments_are_refused(built):
    lib = view.load()
    buf = (C.c_uint8 * 64)()
    err = lambda: lib.hiprz_view_last_error(None)
    assert lib.hiprz_view_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_view_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_view_set_charts(None, buf, 1, buf, 1) == _abi.ERR_INVALID and b"view_set_charts: null view" in err()
    assert lib.hiprz_view_pixels(None, buf, 1, 1, None, buf, None, buf, buf, None) == _abi.ERR_INVALID and b"view_pixels: null view" in err()
    assert lib.hiprz_view_pixels_host(None, buf, 1, 1, None, buf, None, buf, buf) == _abi.ERR_INVALID and b"view_pixels_host: null view" in err()
    assert lib.hiprz_view_samples(None, buf, None) == _abi.ERR_INVALID and b"view_samples: null view" in err()
    lib.hiprz_view_layout(None)          # nothing to write to: returns
    for name in ("viewer", "view", "view_samples", "lit_source"):
        assert callable(getattr(Context, name)), name
    for name in ("set_charts", "pixels", "pixels_device", "samples", "samples_device"):
        assert callable(getattr(view.View, name)), name
    sig = inspect.signature(Context.view).parameters
    assert list(sig) == ["self", "source", "width", "height", "charts", "field", "sky", "params", "rgba8"]
    assert sig["field"].default is None and sig["params"].default is None and sig["rgba8"].default is False
    assert inspect.signature(Context.view_samples).parameters["charts"].default is None
    assert inspect.signature(Context.lit_source).parameters["emission"].default is None
    assert inspect.signature(view.params).parameters["filter"].default == "nearest"


def test_create_fails_loudly_without_a_gpu(built):
    lib = view.load()
    h = C.c_void_p(1)
    rc = lib.hiprz_view_create(C.byref(h), None)
    assert not h
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_view_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_view_last_error(None)


def test_every_host_stub_of_the_view_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; two kernels, and
    not in the twelve libraries whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "view", "hiprz_view.o"), view.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 2
    assert sorted(re.search(r"rz_view\w*?kernel", name).group(0) for name in found[lib]) == ["rz_view_kernel", "rz_view_samples_kernel"], found[lib]
    assert ck.host_stubs(os.path.join(CSRC, "view", "hiprz_view_host.o")) == set(), "the refusals, the checks and the layout are pure host code"
    others = set()
    for path in (_lib.LIB_PATH, query.LIB_PATH, order.LIB_PATH, bake.LIB_PATH, atlas.LIB_PATH, light.LIB_PATH, gather.LIB_PATH, probe.LIB_PATH, smooth.LIB_PATH, field.LIB_PATH,
                 place.LIB_PATH, os.path.join(CSRC, "libhiprz_noise.so")):
        others |= ck.device_kernels(path)
    assert not (found[lib] & others) and not any("rz_view" in name for name in others)


def test_the_kernel_unit_and_the_host_unit_keep_to_their_halves(built):
    body = open(os.path.join(CSRC, "view", "hiprz_view.hip")).read()
    code = re.sub(r"//[^\n]*", "", body)
    assert '#include "query/hiprz_session.hpp"' in code and '#include "query/hiprz_query_device.hpp"' in code and "struct hiprz_view : Session" in code
    assert code.count("__global__") == 2 and "atomic" not in code and "__shared__" not in code and "__syncthreads" not in code, "two kernels, no atomics, no LDS"
    assert code.count("closest_hit_skip<false, false, true>") == 1 and code.count("take_ray(r0, r1, 0u, ray)") == 1, "one walk, the query's closest-hit walk without NORMALIZE"
    assert code.count("generate_simple_ray(") == 1 and code.count("view_walk(s, cam, map, x, y, ray, hit)") == 2, "both kernels call the one device function that makes the sample"
    assert code.count("analyze_intersection<false, true>(") == 1 and "hiprz_kernels.hpp" not in code, "the renderer's surface, without the renderer's kernels"
    for f in ("expf(", "powf(", "sinf(", "cosf(", "acosf(", "__fmaf", "fmaf(", "__fdividef", "__frcp", "rsqrtf("):
        assert f not in code, f"{f} in the kernel unit: the rule is plain float32"
    for other in ("bake/", "atlas/", "light/", "gather/", "probe/", "smooth/", "field/", "place/", "hiprz_field_host", "hiprz_gather_host", "gather_walk", "gather_lookup", "field_visible",
                  "field_irradiance"):
        assert other not in code, "what the library needs of the gather's and the field's lookups it restates"
    assert code.count("hiprz_device_view") == 0 and len(re.findall(r"\bview_and_map\(h, what, s, cam\)", code)) == 3, "all three calls take a view, on every call"
    assert "#if RZ_VIEW_ROWS_BUILD" in code
    host = open(os.path.join(CSRC, "view", "hiprz_view_host.cpp")).read() + open(os.path.join(CSRC, "view", "hiprz_view_host.hpp")).read()
    assert "hip/" not in host and "__global__" not in host and "__device__" not in host, "the pure-host unit has no HIP include"


_NULL = "null pointer"
_CHARTS = "no chart map has been set"
_SIZE = "W or H is not in 1..16384"
_FILTER = "filter is neither NEAREST nor BILINEAR"
_STEP = "a grid step is not a finite number > 0"
_BIAS = "bias is not a finite number >= 0"
_BAD = _abi.ERR_INVALID
_EXPECTED = (["charts: none", "charts: none", f"charts: {_NULL}", f"charts: {_NULL}", "charts: more charts than there are ids below the codes", "charts: a chart's UV is not finite",
              "charts: none"]
             + [f"params: {_abi.OK} none", f"params: {_BAD} null params", f"filter 0: {_abi.OK} none", f"filter 1: {_abi.OK} none", f"filter 2: {_BAD} {_FILTER}",
                f"filter 4294967295: {_BAD} {_FILTER}"] + [f"reserved {k}: {_BAD} reserved is not 0" for k in range(3)]
             + ["grid: none", "grid: null grid", "grid: the grid's counts do not multiply to the number of probes", "grid: a grid count is 0", "grid: the grid has 2^31 probes or more",
                "grid: the grid's corner is not finite"] + [f"grid step: {_STEP}"] * 4 + ["grid: none"]
             + ["field params: none", "field params: null params"] + [f"field params: {_BIAS}"] * 3
             + [f"view: {code} {why}" for code, why in [(_abi.OK, "none")] * 3 + [(_BAD, _NULL)] * 3 + [(_abi.ERR_STATE, _CHARTS), (_BAD, _SIZE), (_BAD, _SIZE), (_BAD, _FILTER),
                                                                                                 (_BAD, _STEP), (_BAD, _BIAS)]]
             + ["pixels: none | none | more than 2^31 - 1 pixels | more than 2^31 - 1 pixels", "groups 12 15 1 12 10 1", "capacity 4096 8192 100 2147483647",
                "layout 16 16 48 16 32 12 28 0"])


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "view_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "view"), os.path.join(ROOT, "tests", "view_host_main.cpp"), os.path.join(CSRC, "view", "hiprz_view_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines == _EXPECTED, [(a, b) for a, b in zip(lines, _EXPECTED) if a != b]
