"""Lightmap smoothing on the GPU (include/hiprz_smooth.h: libhiprz_smooth.so, Context.smooth_texels and the `smooth` keyword of the atlas
bakes).  Every record the device writes is held to the numpy float32 restatement (tests/smooth_reference.py), every byte.

THE INPUTS are tests/smooth_reference.py's atlas(W, H) — tests/test_smooth_reference.py shows that they tell every mutant of the rule apart
— and the real atlas points of tests/gather_world.py's room with what the light bake and the gather leave on them.

  1 bytes            atlases of 1 x 1, 1 x 7, 5 x 3, 16 x 16, 17 x 33, 64 x 64 and 67 x 131; iterations 1 .. 5; all stops on, each one off,
                     all off; host calls; device-pointer calls with out == records and out != records (what lies behind the atlas is not
                     written).
  2 the room         the device's light bake (K = 4) and gather (K = 16) of the room's atlas, smoothed: == the restatement.
  3 both builds      the other build of the kernel (SMOOTH_DEFS: direct for staged) writes the bytes of the shipped one on the cases of 1.
  4 pipeline         smooth=None changes no byte of bake_light_atlas, bake_bounce_atlas and bake_probe_field; with params they are their
                     steps made by hand through the host; Engine::smoothTexels, bakeLightAtlas and bakeBounceAtlas deliver Context's bytes.
  5 refusals         in the header's order, and nothing is launched: the output keeps its bytes.

MEASURED ON MI355X: the twelve cases in 4.8 s beside the session's build fixture; slowest the two builds' comparison (2.2 s: it compiles the
other build and starts two processes) and the C++ host (0.7 s: it compiles a program), every other case below 0.2 s.  Every byte of every
case equal on the first run, with the staged form shipped at every step and the direct form as the other build."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gather_world as GW
import smooth_reference as SR
from rayzath_amd import _abi, _hiprt, gather, light, probe, scene_io, smooth
from rayzath_amd.engine import Context
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
F = np.float32
SIZES = ((1, 1), (1, 7), (5, 3), (16, 16), (17, 33), (64, 64), (67, 131))
ITERATIONS = (1, 2, 3, 4, 5)
OFF = dict(radius=0.0, plane=0.0, sigma_colour=0.0)
STOPS = [SR.PARAMS] + [dict(SR.PARAMS, **{name: 0.0}) for name in SR.PARAMS] + [OFF]      # all on, each one off, all off
NEAR, FAR = 1e-3, 1e3


@pytest.fixture(scope="module")
def ctx(built):
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every case of 1, computed once: (W, H, iterations, index into STOPS) -> record bytes"""
    out = {}
    for W, H in SIZES:
        points, records = SR.atlas(W, H)
        for it in ITERATIONS:
            for k, stops in enumerate(STOPS):
                out[W, H, it, k] = SR.smooth(points, records, iterations=it, **stops).tobytes()
    return out


@pytest.mark.parametrize("size", SIZES)
def test_device_bytes_are_the_restatements(ctx, wanted, size):
    W, H = size
    points, records = SR.atlas(W, H)
    s = ctx.smoother()
    for it in ITERATIONS:
        for k, stops in enumerate(STOPS):
            got = ctx.smooth_texels(points, records, smooth.params(it, **stops))
            assert got.dtype == records.dtype and got.shape == records.shape
            assert got.tobytes() == wanted[W, H, it, k], (size, it, stops, int((got.view(np.uint32) != np.frombuffer(wanted[W, H, it, k], np.uint32).reshape(H, W, 4)).any(-1).sum()))
    # the device-pointer call, in place and not, with guard records behind the atlas
    ctx.sync()
    n, guard = W * H, np.full((3, 4), 0xABABABAB, np.uint32)
    padded = np.concatenate([records.reshape(-1).view(np.uint32).reshape(n, 4), guard])
    d_points = _hiprt.DeviceBuffer.of(points)
    try:
        for it in ITERATIONS:
            d_records, d_out = _hiprt.DeviceBuffer.of(padded), _hiprt.DeviceBuffer.of(np.concatenate([np.zeros((n, 4), np.uint32), guard]))
            try:
                s.texels_device(d_points.ptr, d_records.ptr, W, H, smooth.params(it, **SR.PARAMS), d_out.ptr)
                ctx.sync()
                apart, kept = d_out.download(padded.shape, np.uint32), d_records.download(padded.shape, np.uint32)
                assert apart[:n].tobytes() == wanted[W, H, it, 0] and (apart[n:] == guard).all(), (size, it, "out != records")
                assert kept.tobytes() == padded.tobytes(), "the input of a call with an output of its own is not written"
                s.texels_device(d_points.ptr, d_records.ptr, W, H, smooth.params(it, **SR.PARAMS))
                ctx.sync()
                in_place = d_records.download(padded.shape, np.uint32)
                assert in_place[:n].tobytes() == wanted[W, H, it, 0] and (in_place[n:] == guard).all(), (size, it, "out == records")
            finally:
                d_records.free(), d_out.free()
    finally:
        d_points.free()


def _room(tree=0):
    c = Context(0)
    if tree:
        c.set_tree(tree)
    world = GW.world()
    flat = flatten(world)
    c.upload_scene(flat), c.upload_camera(camera_struct(world.camera))
    return c, world, flat


def test_the_rooms_own_bakes_are_smoothed_as_the_restatement_smooths_them(built):
    c, world, flat = _room()
    try:
        parts = GW.parts(world)
        points, _ = c.atlas_points(parts, GW.W, GW.H, NEAR, FAR)
        direct = c.bake_light(points, (4, 4), 7)
        source = gather.records((0.7, 0.6, 0.5), (GW.H, GW.W))
        source["rgb"] *= direct["light"]
        source["word"] = direct["shadowed"]
        gathered = c.gather(points, source, GW.W, GW.H, gather.chart_tables(parts, len(flat.instances)), (16, 4), 7, (0.05, 0.08, 0.12))
        on = SR.takes_part(points, direct)
        normals = np.unique(points["normal"][on], axis=0)
        assert 500 < on.sum() < on.size and len(normals) >= 3 and ((normals != 0).sum(-1) == 3).any(), "floor, wall and a face of the turned cube, with gutters between"
        changed = 0
        for records in (direct, gathered):
            for it in ITERATIONS:
                for stops in (dict(radius=0.5, plane=0.02, sigma_colour=2.0), dict(radius=0.0, plane=0.05, sigma_colour=0.0), OFF):
                    got = c.smooth_texels(points, records, smooth.params(it, **stops))
                    want = SR.smooth(points, records, iterations=it, **stops)
                    assert got.dtype == records.dtype and got.tobytes() == want.tobytes(), (records.dtype.names, it, stops)
                    changed += int((got.view(np.uint32) != records.view(np.uint32)).sum())
        assert changed > 10000
        defaults = c.smooth_texels(points, direct)
        kw = {k: smooth.params()[k].item() for k in smooth.params_dtype.names}
        assert defaults.tobytes() == SR.smooth(points, direct, **kw).tobytes(), "params=None are smooth.params()'s defaults"
    finally:
        c.close()


_CHILD = r"""
import sys
import numpy as np
import smooth_reference as SR
from rayzath_amd import smooth
from rayzath_amd.engine import Context
ctx = Context(0)
out = []
for W, H in %r:
    points, records = SR.atlas(W, H)
    for it in %r:
        for stops in (SR.PARAMS, dict(radius=0.0, plane=0.0, sigma_colour=0.0)):
            out.append(ctx.smooth_texels(points, records, smooth.params(it, **stops)).reshape(-1))
ctx.close()
np.save(sys.argv[1], np.concatenate(out))
print(smooth.layout()[6], smooth.layout()[7], smooth.LIB_PATH)
""" % (SIZES, ITERATIONS)


def test_both_builds_of_the_kernel_write_the_same_bytes(built, wanted, tmp_path):
    """the shipped library against the other build of the same source (the direct form where the staged one ships and the other way
    round, at s = 1 and at s > 1), each in a process of its own through HIPRZ_SMOOTH_LIB"""
    make = open(os.path.join(CSRC, "Makefile")).read()
    cxxflags = re.search(r"^CXXFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(INC)", f"-I{os.path.join(ROOT, 'include')} -I{CSRC}")
    hipflags = re.search(r"^HIPFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    shipped = smooth.layout()[6:8]
    flipped = [f"-DRZ_SMOOTH_STAGED_S1={1 - shipped[0]}", f"-DRZ_SMOOTH_STAGED_SN={1 - shipped[1]}"]
    other = str(tmp_path / "libhiprz_smooth_other.so")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, *cxxflags.split(), *hipflags.split(), *flipped, "-Wno-undefined-inline", "-I", os.path.join(CSRC, "smooth"),
                    "-shared", os.path.join(CSRC, "smooth", "hiprz_smooth.hip"), os.path.join(CSRC, "smooth", "hiprz_smooth_host.cpp"), "-L", CSRC, "-lhiprz", f"-Wl,-rpath,{CSRC}", "-o", other],
                   check=True, capture_output=True, timeout=600)
    results = {}
    for name, lib in (("shipped", None), ("other", other)):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
        env.pop("HIPRZ_SMOOTH_LIB", None)
        if lib:
            env["HIPRZ_SMOOTH_LIB"] = lib
        path = str(tmp_path / f"{name}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        forms = r.stdout.strip().splitlines()[-1].split()
        assert forms[2] == (lib or smooth.LIB_PATH) and [int(forms[0]), int(forms[1])] == (shipped if lib is None else [1 - shipped[0], 1 - shipped[1]])
        results[name] = np.load(path)
    assert results["shipped"].dtype == SR.record_dtype and len(results["shipped"]) == 2 * len(ITERATIONS) * sum(w * h for w, h in SIZES)
    assert results["shipped"].tobytes() == results["other"].tobytes(), "the two forms of the kernel differ in some byte"
    want = b"".join(wanted[W, H, it, k] for W, H in SIZES for it in ITERATIONS for k in (0, len(STOPS) - 1))
    assert results["other"].tobytes() == want, "the other build differs from the restatement"


def _by_hand(c, parts, charts, albedo, emission, bounces, directions, samples, seed, rings, sky, params):
    """(direct, indirect, ring, the source of the last gather) of a smoothed bounce bake, step by step through the host"""
    W, H = GW.W, GW.H
    points, _ = c.atlas_points(parts, W, H, NEAR, FAR)
    a = c.atlas()
    direct = c.smooth_texels(points, c.bake_light(points, samples, seed), params)
    indirect = None
    for _ in range(bounces):
        source = a.dilate(c.gatherer().compose(direct, indirect, albedo, emission, c.sync), rings)[0].reshape(H, W)
        indirect = c.smooth_texels(points, c.gather(points, source, W, H, charts, directions, seed, sky), params)
    dilated, ring = a.dilate(indirect, rings)
    return a.dilate(direct, rings)[0], dilated, ring, source


def test_the_pipeline_calls_are_their_steps(built):
    W, H = GW.W, GW.H
    seed, rings, directions, samples, sky = 4, 2, (16, 3), (4, 3), (0.01, 0.02, 0.03)
    params = smooth.params(3, radius=0.5, plane=0.02, sigma_colour=2.0)
    c, world, flat = _room(3)
    try:
        parts = GW.parts(world)
        charts = gather.chart_tables(parts, len(flat.instances))
        albedo, emission = gather.records((0.7, 0.6, 0.5), (H, W)), gather.records((0.0, 0.0, 0.0), (H, W))
        emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)
        # smooth=None: the bytes of the call without the keyword, and no smoothing handle is made
        plain_light = c.bake_light_atlas(parts, W, H, samples, seed, rings, NEAR, FAR)
        none_light = c.bake_light_atlas(parts, W, H, samples, seed, rings, NEAR, FAR, smooth=None)
        plain_bounce = c.bake_bounce_atlas(parts, W, H, albedo, emission, 2, directions, samples, seed, rings, sky, NEAR, FAR)
        none_bounce = c.bake_bounce_atlas(parts, W, H, albedo, emission, 2, directions, samples, seed, rings, sky, NEAR, FAR, smooth=None)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain_light, none_light)) and all(a.tobytes() == b.tobytes() for a, b in zip(plain_bounce, none_bounce))
        assert getattr(c, "_smooth", None) is None, "smooth=None runs no smoothing code"
        # the light atlas: atlas points -> bake -> smooth_texels -> dilate
        points, samples_map = c.atlas_points(parts, W, H, NEAR, FAR)
        want, want_ring = c.atlas().dilate(c.smooth_texels(points, c.bake_light(points, samples, seed), params), rings)
        got, got_samples, got_ring = c.bake_light_atlas(parts, W, H, samples, seed, rings, NEAR, FAR, smooth=params)
        assert got.dtype == light.texel_dtype and got.tobytes() == want.tobytes() and got_ring.tobytes() == want_ring.tobytes() and got_samples.tobytes() == samples_map.tobytes()
        assert got.tobytes() != plain_light[0].tobytes() and got_ring.tobytes() == plain_light[2].tobytes()
        as_dict = c.bake_light_atlas(parts, W, H, samples, seed, rings, NEAR, FAR, smooth=dict(iterations=3, radius=0.5, plane=0.02, sigma_colour=2.0))
        assert as_dict[0].tobytes() == got.tobytes()
        # the bounce atlas and the probe field
        probes = probe.grid((-2.0, 0.25, -2.0), (2.0, 2.25, 2.0), (3, 2, 3))
        for bounces in (1, 2):
            direct, indirect, ring, source = _by_hand(c, parts, charts, albedo, emission, bounces, directions, samples, seed, rings, sky, params)
            got = c.bake_bounce_atlas(parts, W, H, albedo, emission, bounces, directions, samples, seed, rings, sky, NEAR, FAR, smooth=params)
            assert got[0].tobytes() == direct.tobytes(), f"{bounces} bounces: direct"
            assert got[1].tobytes() == indirect.tobytes(), f"{bounces} bounces: indirect"
            assert got[2].tobytes() == ring.tobytes(), f"{bounces} bounces: ring"
            field = c.bake_probe_field(parts, W, H, albedo, emission, bounces, probes, directions, samples, seed, rings, sky, NEAR, FAR, None, (16, 2), smooth=params)
            assert all(f.tobytes() == g.tobytes() for f, g in zip(field[:3], got))
            assert field[3].tobytes() == c.bake_probes(probes, source, W, H, charts, (16, 2), samples, seed, sky).tobytes(), f"{bounces} bounces: the probes"
        assert got[1].tobytes() != plain_bounce[1].tobytes()
        plain_field = c.bake_probe_field(parts, W, H, albedo, emission, 2, probes, directions, samples, seed, rings, sky, NEAR, FAR, None, (16, 2))
        assert all(f.tobytes() == g.tobytes() for f, g in zip(plain_field[:3], plain_bounce)), "smooth=None changes no byte of bake_probe_field"
    finally:
        c.close()


def test_cpp_engine_smooths(built, tmp_path):
    exe = str(tmp_path / "smooth_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "smooth_delivery_check.cpp"), "-o", exe,
                    "-L", CSRC, "-lhiprz_host", "-lhiprz_smooth", "-lhiprz", "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "room.json")
    world = GW.world()
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, LK, LS, seed, bounces = 16, 3, 4, 4, 20261021, 2
    it, stops = 3, dict(radius=0.5, plane=0.02, sigma_colour=2.0)
    params = smooth.params(it, **stops)
    parts = GW.parts(world)
    W, H = 67, 131
    points, records = SR.atlas(W, H)
    c = Context(0)
    try:
        want = c.smooth_texels(points, records, params)
        c.upload_scene(loaded.flat), c.upload_camera(loaded.camera)
        albedo = gather.records((0.7, 0.6, 0.5), (GW.H, GW.W))
        lit = c.bake_light_atlas(parts, GW.W, GW.H, (LK, LS), seed, 2, smooth=params)
        bounced = c.bake_bounce_atlas(parts, GW.W, GW.H, albedo, None, bounces, (K, S), (LK, LS), seed, 2, (0.01, 0.02, 0.03), smooth=params)
    finally:
        c.close()
        loaded.close()
    files = {name: str(tmp_path / (name + ".bin")) for name in ("points", "records", "out")}
    points.tofile(files["points"]), records.tofile(files["records"])
    part_args = []
    for instance, tris in parts:
        path = str(tmp_path / f"charts{instance}.bin")
        tris.tofile(path)
        part_args += [str(instance), path]
    r = subprocess.run([exe, scene_path, files["points"], files["records"], str(W), str(H), files["out"], str(it), repr(stops["radius"]), repr(stops["plane"]), repr(stops["sigma_colour"]),
                        str(K), str(S), str(LK), str(LS), str(seed), str(bounces)] + part_args, capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "SMOOTH DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    read = lambda suffix: open(files["out"] + suffix, "rb").read()
    assert read("") == want.tobytes() == SR.smooth(points, records, iterations=it, **stops).tobytes(), "Engine::smoothTexels differs from Context.smooth_texels"
    assert read(".lit") == lit[0].tobytes() and read(".lit_ring") == lit[2].tobytes(), "Engine::bakeLightAtlas with smoothing differs from Context.bake_light_atlas"
    assert read(".direct") == bounced[0].tobytes() and read(".indirect") == bounced[1].tobytes() and read(".ring") == bounced[2].tobytes(), "Engine::bakeBounceAtlas with smoothing differs"


def test_refusals_come_in_order_and_launch_nothing(ctx):
    lib, s = smooth.load(), ctx.smoother()
    W, H = 5, 3
    points, records = SR.atlas(W, H)
    ctx.sync()
    guard = np.full((W * H, 4), 0xCDCDCDCD, np.uint32)
    bufs = [_hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer.of(records), _hiprt.DeviceBuffer.of(guard)]
    good = smooth.params(2, **SR.PARAMS)
    bad = np.array([(0, np.nan, 0.0, 0.0)], smooth.params_dtype)
    handle = s._smooth

    def refused(text, *args):
        assert lib.hiprz_smooth_texels(*args) == _abi.ERR_INVALID
        assert text in lib.hiprz_smooth_last_error(handle if args[0] else None), (text, lib.hiprz_smooth_last_error(handle if args[0] else None))

    try:
        p, r, o = (b.ptr for b in bufs)
        refused(b"null smooth", None, p, r, W, H, good.ctypes.data, o, None)
        for args in ((None, r, 0, 0, bad.ctypes.data, o), (p, None, 0, 0, bad.ctypes.data, o), (p, r, 0, 0, None, o), (p, r, 0, 0, bad.ctypes.data, None)):
            refused(b"null pointer", handle, *args, None)                       # before the params and the size are looked at
        refused(b"iterations is not in 1..8", handle, p, r, 0, 0, bad.ctypes.data, o, None)          # the params before the size
        for field, name in ((1, b"radius"), (2, b"plane"), (3, b"sigma_colour")):
            for value in (np.nan, -1.0, np.inf):
                v = [2, 0.5, 0.5, 0.5]
                v[field] = value
                refused(name + b" is not a finite number >= 0", handle, p, r, 0, H, np.array([tuple(v)], smooth.params_dtype).ctypes.data, o, None)
        for w, h in ((0, H), (W, 0), (16385, 1), (1, 16385), (0xFFFFFFFF, 0xFFFFFFFF)):
            refused(b"W or H is not in 1..16384", handle, p, r, w, h, good.ctypes.data, o, None)
        host_out = guard.copy()
        assert lib.hiprz_smooth_texels_host(handle, points.ctypes.data, records.ctypes.data, W, H, bad.ctypes.data, host_out.ctypes.data) == _abi.ERR_INVALID
        assert lib.hiprz_smooth_texels_host(handle, points.ctypes.data, None, W, H, good.ctypes.data, host_out.ctypes.data) == _abi.ERR_INVALID
        assert lib.hiprz_smooth_texels_host(handle, points.ctypes.data, records.ctypes.data, W, 0, good.ctypes.data, host_out.ctypes.data) == _abi.ERR_INVALID
        assert (host_out == guard).all()
        with pytest.raises(ValueError):
            ctx.smooth_texels(points, records, dict(iterations=9))
        with pytest.raises(TypeError):
            ctx.smooth_texels(points, records[:, :-1], good)
        ctx.sync()
        assert (bufs[2].download(guard.shape, np.uint32) == guard).all(), "a refused call wrote its output"
        s.texels_device(p, r, W, H, good, o)
        ctx.sync()
        assert bufs[2].download(guard.shape, np.uint32).tobytes() == SR.smooth(points, records, iterations=2, **SR.PARAMS).tobytes(), "and the handle still works"
    finally:
        for b in bufs:
            b.free()
