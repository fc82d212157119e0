"""The ordered ray queries at the C-ABI level, without a GPU: libhiprz_order.so loads and exports exactly the symbols include/hiprz_order.h
declares, order.ENTRY_POINTS binds them, hiprz_sort_u32_device is declared, bound and refuses a null context, null arguments are refused,
the library does not come up without a device, every host stub of the new library has its gfx950 kernel — three of them, none in
libhiprz.so or libhiprz_query.so — and the pure-host unit runs as a process of its own under sanitizers."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from rayzath_amd import _abi, _lib, order, query
from rayzath_amd.engine import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hiprz_order.h")
KERNELS = ("rz_order_keys_kernel", "rz_order_closest_kernel", "rz_order_occluded_kernel")
NAMES = ["hiprz_order_" + n for n in ("closest", "closest_by", "closest_host", "create", "destroy", "last_error", "occluded", "occluded_by", "occluded_host",
                                     "permutation")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _check_kernels():
    spec = importlib.util.spec_from_file_location("check_kernels", os.path.join(ROOT, "tools", "check_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_exactly_the_declared_symbols_and_the_mirror_binds_them(built):
    lib = order.load()
    names = sorted(set(re.findall(r"\b(hiprz_order_[a-z0-9_]+)\s*\(", _header())))
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in include/hiprz_order.h but not exported"
    assert set(names) == set(order.ENTRY_POINTS)
    exported = subprocess.run(["nm", "-D", "--defined-only", order.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bhiprz_\w+", exported)) == names, "the library exports hiprz_ symbols the header does not declare"
    assert os.path.dirname(order.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) or "HIPRZ_LIB" in os.environ or "HIPRZ_ORDER_LIB" in os.environ
    # the records and the flag are the query library's, not restated
    header = _header()
    assert '#include "hiprz_query.h"' in header and "typedef struct hiprz_ray" not in header and "#define HIPRZ_QUERY_NORMALIZE" not in header
    assert order.NORMALIZE == query.NORMALIZE and order.ray_dtype is query.ray_dtype and order.hit_dtype is query.hit_dtype


def test_the_sort_entry_point_is_declared_bound_and_refuses_a_null_context(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprz.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hiprz_sort_u32_device\(hiprz_ctx\*\s*ctx,\s*uint32_t\*\s*keys_device,\s*uint32_t\s+n,\s*int\s+key_bits,\s*uint32_t\*\s*perm_out_device,\s*void\*\s*stream\)", text)
    assert "hiprz_sort_u32_device" in _abi.ENTRY_POINTS
    buf = (C.c_uint32 * 4)()
    assert _lib.load().hiprz_sort_u32_device(None, buf, 4, 24, buf, None) == _abi.ERR_INVALID


def test_null_arguments_are_refused(built):
    lib = order.load()
    buf = (C.c_uint8 * 96)()
    assert lib.hiprz_order_create(None, None) == _abi.ERR_INVALID
    assert lib.hiprz_order_destroy(None) == _abi.ERR_INVALID
    assert lib.hiprz_order_closest(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert b"order_closest: null order" in lib.hiprz_order_last_error(None)
    assert lib.hiprz_order_occluded(None, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_order_closest_by(None, buf, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert lib.hiprz_order_occluded_by(None, buf, buf, 1, 0, buf, None) == _abi.ERR_INVALID
    assert b"order_occluded_by: null order" in lib.hiprz_order_last_error(None)
    assert lib.hiprz_order_closest_host(None, buf, 1, 0, buf) == _abi.ERR_INVALID
    assert lib.hiprz_order_occluded_host(None, buf, 1, 0, buf) == _abi.ERR_INVALID
    assert lib.hiprz_order_permutation(None, buf, 1, 0, None, buf, None) == _abi.ERR_INVALID
    assert b"order_permutation: null order" in lib.hiprz_order_last_error(None)
    assert lib.hiprz_order_closest(None, buf, 0, 0, buf, None) == _abi.ERR_INVALID, "a null handle is refused before n == 0 is looked at"
    for name in ("trace", "occluded", "ray_order", "order"):
        assert callable(getattr(Context, name)), name


def test_create_fails_loudly_without_a_gpu(built):
    lib = order.load()
    o = C.c_void_p(1)
    rc = lib.hiprz_order_create(C.byref(o), None)
    assert not o
    if os.path.exists("/dev/kfd"):       # asked of the kernel driver, not of a HIP runtime (tests/test_query_abi.py: _has_gpu)
        assert rc == _abi.ERR_INVALID and b"null context" in lib.hiprz_order_last_error(None)
    else:
        assert rc == _abi.ERR_DEVICE and b"HIP device" in lib.hiprz_order_last_error(None)


def test_every_host_stub_of_the_order_library_has_its_gfx950_kernel(built):
    """the missing-symbol abort tools/check_kernels.py exists for, for the object and the library that tool does not walk; three kernels, and
    none of them in libhiprz.so or libhiprz_query.so, whose kernel sets are pinned"""
    ck = _check_kernels()
    obj, lib = os.path.join(CSRC, "order", "hiprz_order.o"), order.LIB_PATH
    found = {}
    for path in (obj, lib):
        stubs, kernels = ck.host_stubs(path), ck.device_kernels(path)
        assert stubs == kernels, (path, stubs ^ kernels)
        found[path] = stubs
    assert found[obj] == found[lib] and len(found[lib]) == 3
    for kernel in KERNELS:
        assert sum(kernel in name for name in found[lib]) == 1, kernel
    assert ck.host_stubs(os.path.join(CSRC, "order", "hiprz_order_host.o")) == set(), "the refusals and the growth rule are pure host code"
    main, asked = ck.device_kernels(_lib.LIB_PATH), ck.device_kernels(query.LIB_PATH)
    # by mangled name: libhiprz.so has a kernel of its own called rz_order_keys_kernel (hiprz_api.hip, global namespace, three arguments: the
    # launch order of the resident kernels), another symbol than hiprz::rz_order_keys_kernel here
    assert not (found[lib] & (main | asked)), "a kernel of the order library is in a library whose kernel set is pinned"
    assert not any("rz_order_closest" in name or "rz_order_occluded" in name or "N5hiprz20rz_order_keys_kernel" in name for name in main | asked)
    assert all("N5hiprz" in name for name in found[lib]), "the order kernels live in namespace hiprz"
    assert len(asked) == 3, "the query library keeps its three kernels"


def test_the_shared_device_header_defines_no_kernel():
    text = open(os.path.join(CSRC, "query", "hiprz_query_device.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "__global__" not in code and "take_ray" in code
    for unit in (os.path.join("query", "hiprz_query.hip"), os.path.join("order", "hiprz_order.hip")):
        body = open(os.path.join(CSRC, unit)).read()
        assert "hiprz_query_device.hpp" in body and "bool take_ray(" not in body and "HIPRZ_HIT_FOUND |" not in body, f"{unit}: the ray rule and the hit layout exist once"


def _capacity(have, need):
    """the rule of rayzath_amd/csrc/order/hiprz_order_host.cpp, restated"""
    if need <= have:
        return have
    return min(max(need, 2 * have, 4096), 2**30)


_PAIRS = [(0, 0), (0, 1), (0, 4096), (0, 4097), (4096, 4096), (4096, 4097), (8192, 8193), (8192, 20000), (100, 50), (2**29, 2**29 + 1), (2**30, 2**30),
          (2**29 + 5, 2**30), (2**30 - 1, 2**30), (3, 2**30), (65536, 65537), (1, 60000)]
_REFUSALS = ["none", "none", "null pointer", "unknown flag", "unknown flag", "none", "more than 2^30 rays", "null pointer", "more than 2^30 rays"]


def test_the_host_unit_as_a_process_of_its_own_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "order_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(CSRC, "order"), os.path.join(ROOT, "tests", "order_host_main.cpp"), os.path.join(CSRC, "order", "hiprz_order_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(f"{h} {n}\n" for h, n in _PAIRS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"pairs {len(_PAIRS)}"
    assert lines[len(_PAIRS):-1] == ["refusal: " + w for w in _REFUSALS]
    assert [int(v) for v in lines[:len(_PAIRS)]] == [_capacity(h, n) for h, n in _PAIRS]
