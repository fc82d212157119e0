"""The ray queries at the C-ABI level, without a GPU: libhiprz_query.so loads and exports every symbol include/hiprz_query.h declares, its
record layouts agree with the header and the numpy dtypes, null arguments are refused, it does not come up without a device,
hiprz_device_view is declared, bound and refuses a null context (its size guard needs a context: tests/test_query_gpu.py::test_device_view_guards),
every host stub of the new library has its gfx950 kernel while libhiprz.so's kernel set is what it
was, and the pure-host unit runs as a process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

import query_reference as QR
from rayzath_amd import _abi, _lib, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_query.h")
KERNELS = ("rz_query_closest_kernel", "rz_query_occluded_kernel", "rz_query_pixel_rays_kernel")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _struct_fields(name):
    """[(field, C type, count)] of `typedef struct name { ... } name;` in the header"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(float|uint32_t|int32_t)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", n)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    return fields


def test_library_exports_every_declared_symbol_and_the_mirror_binds_them(built):
    lib = query.load()
    names = sorted(set(re.findall(r"\b(hiprz_query_[a-z0-9_]+)\s*\(", _header())))
    assert len(names) == 9, names
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_query.h but not exported"
    assert set(names) == set(query.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", query.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(s for s in re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    assert os.path.dirname(query.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ or "HIPRZ_QUERY_LIB" in os.environ


def test_layouts_match_the_header_and_the_dtypes(built):
    out = (C.c_uint32 * 7)()
    query.load().hiprz_query_layout(out)
    r, h = query.ray_dtype, query.hit_dtype
    assert list(out) == [r.itemsize, h.itemsize, r.fields["direction"][1], h.fields["flags"][1], h.fields["instance"][1], h.fields["normal"][1],
                         h.fields["scene_triangle"][1]] == [32, 48, 16, 12, 16, 32, 44]
    ctype = {"float": "<f4", "uint32_t": "<u4", "int32_t": "<i4"}
    for struct, dtype in (("hiprz_ray", r), ("hiprz_hit", h)):
        fields = _struct_fields(struct)
        assert [n.rstrip("_") for n, _, _ in fields] == list(dtype.names), struct
        offset = 0
        for (name, ct, count), key in zip(fields, dtype.names):
            sub, at = dtype.fields[key][:2]
            assert at == offset and sub.base == np.dtype(ctype[ct]) and int(np.prod(sub.shape, dtype=int)) == count, (struct, name)
            offset += 4 * count
        assert offset == dtype.itemsize
    header = _header()
    for name, value in (("HIPRZ_HIT_FOUND", query.HIT_FOUND), ("HIPRZ_HIT_EXTERNAL", query.HIT_EXTERNAL), ("HIPRZ_HIT_INVALID", query.HIT_INVALID),
                        ("HIPRZ_QUERY_NORMALIZE", query.NORMALIZE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, header).group(1)) == value
    assert query.rays([[0, 0, 0]], [[0, 0, 1], [1, 0, 0]], 0.5, 9.0).tobytes() == np.array(
        [([0, 0, 0], 0.5, [0, 0, 1], 9.0), ([0, 0, 0], 0.5, [1, 0, 0], 9.0)], query.ray_dtype).tobytes()


def test_null_arguments_are_refused(built):
    lib = query.load()
    buf = (C.c_uint8 * 96)()
    assert lib.hiprz_query_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_query_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_query_closest(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert b"null query" in lib.hiprz_query_last_error(None)
    assert lib.hiprz_query_occluded(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_query_closest_host(None, buf, 1, 0, buf) == _abi.ERR_INVALID
    assert lib.hiprz_query_occluded_host(None, buf, 1, 0, buf) == _abi.ERR_INVALID
    assert lib.hiprz_query_pixel_rays(None, buf, None) == _abi.ERR_INVALID
    assert b"query_pixel_rays: null query" in lib.hiprz_query_last_error(None)
    for name in ("trace", "occluded", "pixel_rays", "query"):
        assert callable(getattr(Context, name)), name


def _has_gpu():
    """whether this machine has an AMD GPU, asked of the kernel driver and not of a HIP runtime: torch brings a second copy of the runtime into
    the process, and the copy that comes up second finds no device — a test that asked torch first would take the GPU from every test after it"""
    return os.path.exists("/dev/kfd")


def test_create_fails_loudly_without_a_gpu(built):
    lib = query.load()
    q = C.c_void_p(1)
    rc = lib.hiprz_query_create(C.byref(q), None)
    assert not q
    if _has_gpu():
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_query_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_query_last_error(None)


def test_device_view_is_declared_and_refuses_a_null_context(built):
    """only what can be asked without a context; the size guard, the order of the refusals and the state rules run on the GPU
    (tests/test_query_gpu.py::test_device_view_guards)"""
    assert "hiprz_device_view" in _abi.ENTRY_POINTS
    lib = _lib.load()
    assert re.search(r"\bint\s+hiprz_device_view\(", open(os.path.join(ROOT, "include", "hiprz.h")).read())
    scene_bytes, camera_bytes = QR.device_view_sizes()
    assert (scene_bytes, camera_bytes) == (256, 84)      # as hiprz_device.hpp declares them today: DScene is pinned there by a static_assert
    scene, camera = (C.c_uint8 * scene_bytes)(), (C.c_uint8 * camera_bytes)()
    assert lib.hiprz_device_view(None, scene, scene_bytes, camera, camera_bytes) == _abi.ERR_INVALID


def test_every_host_stub_of_the_query_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; and the three
    kernels stay out of libhiprz.so, whose kernel set is pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "query", "hiprz_query.o"), query.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 3
    for kernel in KERNELS:
        assert sum(kernel in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "query", "hiprz_query_host.o")) == set(), "the staging rule and the layouts are pure host code"
    main = ck.device_kernels(_lib.LIB_PATH)
    assert not any("rz_query" in name for name in main), "a query kernel entered libhiprz.so, whose kernel set is pinned"
    assert not (found[lib] & main), "a kernel of libhiprz.so is duplicated in the query library"


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/query/hiprz_query_staging.hpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 2**31 - 1)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**30, 2**30 + 1), (2**31 - 1, 2**31 - 1),
          (2**30 + 5, 2**31 - 1), (2**31 - 2, 2**31 - 1), (3, 2**31 - 1), (65536, 65537), (1, 60000)]
# of the calls tests/order_host_main.cpp lists, under the query's limit: 2^30 + 1 rays are taken, a null pointer is looked at before the flags
_REFUSALS = ["none", "none", "null pointer", "unknown flag", "unknown flag", "none", "none", "null pointer", "more than 2^31 - 1 rays"]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "query_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "query"), os.path.join(ROOT, "tests", "query_host_main.cpp"), os.path.join(CSRC, "query", "hiprz_query_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}" and lines[-2] == "layout 32 48 16 12 16 32 44"
    assert lines[len(_PAIRS):-2] == ["refusal: " + w for w in _REFUSALS]
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
