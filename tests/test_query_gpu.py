"""Ray queries on the GPU (include/hiprz_query.h: libhiprz_query.so, hiprz_device_view, Context.trace / occluded / pixel_rays,
Engine::castRays) held to the CPU oracle's first hit (tests/query_reference.py; tests/test_query_oracle.py is the reference's own proof).
Trees 0 (reference) and 3 (device SAH) unless said otherwise; one Context per chunk of 8 of the 118 scenes of tests/guide_scenes.py.

  1 sweep       pixel_rays() read back and traced WITHOUT NORMALIZE against rzo_first_hit_frame on every pixel: the geometric fields
                (found, t bits, instance, scene_triangle, triangle, slot, material, external) must be equal, normal / u / v are held
                under guide_scenes' far rule with its caps (2 per scene, 1 per sweep: the one-ulp libm stand-ins show 0); misses read
                +0 / -1 / far; on the 12 x 8 lattice after one pass the four hiprz_raycast fields of every hit equal Context.ray_cast,
                and on EVERY lattice pixel they equal it for the ray hiprz_ray_cast really walks, the pixel's between 0.99 and 1.01 of
                its depth: on a pixel that misses the depth is the camera's far, and the ray cast then reaches 1 % beyond it (scene 10,
                pixel (8, 8): a triangle between far and 1.01 far, met by hiprz_ray_cast and rzo_ray_cast alike, not by the pixel's ray).
  2 pixel rays  origin = the camera's position bit for bit, direction within 1e-6 per component of normalized(pixel_d0) in float64
                (about ten float32 roundings of a unit vector); (position, pixel_d0) under NORMALIZE gives case 1's bytes.
  3 arbitrary   query_reference.scene_rays under NORMALIZE against oracle_ray, same rule, internal hits included.  Of the 16 sparse
                scenes the 3 empty worlds miss on every ray (asserted); the 12 one-pixel frames' frustum rays cover the pixel's footprint
                and 66 of the 128 hit — all are held to the oracle like every other ray.
  4 occlusion   occluded(r) == found(trace(r)) on the rays of 1 and 3; for every hit the ray cut to [near, 0.5 t] reads 0, cut to
                [near, min(2 t, far)] reads 1, started at 1.5 t it agrees with trace on the same ray.
  5 invalid     NaN, +-inf, zero direction, far <= near, near < 0 and (without NORMALIZE) a direction of length 2 at lanes 0, 31, 63, 64
                and the last of 257: each reads INVALID / the miss fields / t = far's bits / occlusion 0, every valid ray reads what it
                reads without them; n in {0, 1, 63, 64, 65, 257} through device pointers with a sentinel behind n, byte-equal to the
                host-pointer calls.  Host-pointer calls of 1, 4096, 4097, 8193 and 1 rays on one handle of its own (its staging is made,
                kept, grown twice, kept), closest and occluded by turns, byte-equal to the device-pointer calls.
  6 staleness  one Context: after upload_scene(other), after update_instances with a moved instance, after update_triangles + refit and
                after rebuild_trees, trace of fixed rays equals a fresh context's on the changed scene and differs from before.  A
                refitted context numbers scene_triangle by the order IT was given (the first upload's), a fresh one by the changed
                scene's: compared through the permutation between the two orders.
  7 off = off   with and without queries between every two render calls accumulator, RGBA8, depth, ray count, pass count, graph
                captures and guides are equal — on one part, on a two-part [0, 0] context and under set_shard(1, 4), where the query
                answers for the whole scene.  hiprz_device_view's refusal of a part of a multi-device context is a guard no caller can
                reach today (no call hands a part's handle out): it has no test.
  refusals      hiprz_device_view's guards with a context (test_device_view_guards): a wrong scene size, a wrong camera size, a null
                camera with bytes and a camera with none are HIPRZ_ERR_INVALID before the state is looked at; the right sizes give
                HIPRZ_ERR_STATE before a scene and, for the camera half, before a camera.  Null pointers, an unknown flag, no scene,
                no camera through the query's calls (test_refusals).
  8 C++         Engine::castRays / ::occluded through tests/query_delivery_check.cpp, byte-equal to Context.trace / occluded.

MEASURED ON MI355X (trees 0 and 3 gave the same figures): sweep 126 885 pixels on 118 scenes, all 48 bytes of every hit equal to the
oracle's record (exact 126 885, far 0, discrete 0); ray cast lattice 9 306 pixels, 7 082 met an instance, 10 of them on a pixel whose own ray
misses within the camera's range; largest direction error of a pixel ray 1.05e-7; recipe 3 392 rays, 2 307 hit, 1 067 from the inside, exact
3 392; occlusion consistent on every ray and on three cut rays per hit (3 961 hits in the first chunk alone); off = off: every buffer and
counter equal on the three kinds of context, the traced frame (3 840 rays) exact on each; C++ host byte-equal (1 536 rays, 1 535 hit, one
invalid).  No fault was found in the three kernels.  Run time: 151 cases in 7 s beside the session's build fixture, slowest case 0.6 s.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guide_scenes as GS
import oracle
import query_reference as QR
from rayzath_amd import _abi, _hiprt, _lib, query, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, HIT_INVALID, hit_dtype, ray_dtype
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
THREADS = 8
CHUNK = 8
CHUNKS = [GS.SCENES[i:i + CHUNK] for i in range(0, len(GS.SCENES), CHUNK)]
TREES = (0, 3)
_RESULTS = {}


def _context(tree=0, devices=0):
    ctx = Context(devices)
    if tree:
        ctx.set_tree(tree)
    return ctx


def _upload(ctx, key):
    flat, cam, cfg = GS.flat_scene(key)[:3]
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    return flat, cam, cfg


def _found(hits):
    return (hits["flags"] & HIT_FOUND) != 0


def _lattice(cam):
    xs = sorted(set(np.linspace(0, cam.width - 1, 12).astype(int).tolist()))
    ys = sorted(set(np.linspace(0, cam.height - 1, 8).astype(int).tolist()))
    return [(x, y) for y in ys for x in xs]


def _cut_rays(rays, hits):
    """the three cut rays of every hit: (rays of the found ones, [near, 0.5 t], [near, min(2 t, far)], [1.5 t, far])"""
    found = _found(hits)
    r, t = rays[found], hits["t"][found]
    half, double, behind = r.copy(), r.copy(), r.copy()
    half["far"] = np.float32(0.5) * t
    double["far"] = np.minimum(np.float32(2.0) * t, r["far"])
    behind["near"] = np.float32(1.5) * t
    return half, double, behind


def _occlusion(ctx, rays, hits, normalize):
    """case 4 on one batch: failures as strings"""
    rays, hits = rays.reshape(-1), hits.reshape(-1)
    out = []
    occ = ctx.occluded(rays, normalize)
    if not np.array_equal(occ, _found(hits).astype(np.uint32)):
        out.append(f"occluded != found on {int((occ != _found(hits)).sum())} of {len(rays)} rays")
    half, double, behind = _cut_rays(rays, hits)
    if len(half):
        if ctx.occluded(half, normalize).any():
            out.append("a ray cut to [near, 0.5 t] is occluded")
        if not ctx.occluded(double, normalize).all():
            out.append("a ray cut to [near, min(2 t, far)] is not occluded")
        if not np.array_equal(ctx.occluded(behind, normalize), _found(ctx.trace(behind, normalize)).astype(np.uint32)):
            out.append("occluded != found on rays started at 1.5 t")
    return out, len(half)


def run_chunk(tree, chunk):
    """one context, the chunk's scenes uploaded one after the other: {scene: dict of comparisons}; computed once per (tree, chunk)"""
    at = (tree, chunk)
    if at in _RESULTS:
        return _RESULTS[at]
    out, ctx = {}, _context(tree)
    for key in CHUNKS[chunk]:
        flat, cam, cfg = _upload(ctx, key)
        assert ctx.tree() == (tree if len(flat.instances) else 0), (key, ctx.tree())
        r = {}
        # 1: the sweep
        rays = ctx.pixel_rays()
        hits = ctx.trace(rays)
        ref = QR.as_hits(GS.records(key, 0, threads=THREADS))
        r["sweep"] = QR.compare(hits, ref)
        r["sweep_misses"] = QR.misses_read_as_specified(hits, rays)
        r["invalid"] = int(((hits["flags"] & HIT_INVALID) != 0).sum())
        # 2: the pixel rays
        d0 = QR.frame_d0(cam).astype(np.float64)
        unit = d0 / np.linalg.norm(d0, axis=-1, keepdims=True)
        r["origin_bits"] = bool((rays["origin"].view(np.uint32) == np.array(cam.position[:], np.float32).view(np.uint32)).all())
        r["range_bits"] = bool((rays["near"] == np.float32(cam.near_far[0])).all() and (rays["far"] == np.float32(cam.near_far[1])).all())
        r["direction_error"] = float(np.abs(rays["direction"].astype(np.float64) - unit).max())
        r["normalize_bytes"] = ctx.trace(QR.pixel_rays_d0(cam), normalize=True).tobytes() == hits.tobytes()
        # 3: arbitrary rays
        recipe, dense = QR.scene_rays(key)
        got = ctx.trace(recipe, normalize=True)
        want = QR.scene_reference(key)
        r["recipe"] = QR.compare(got, want)
        r["recipe_misses"] = QR.misses_read_as_specified(got, recipe)
        r["recipe_found"], r["recipe_internal"] = int(_found(got).sum()), int((_found(got) & ((got["flags"] & HIT_EXTERNAL) == 0)).sum())
        r["dense"], r["empty"] = dense, not len(flat.instances)
        # 4: occlusion
        a, na = _occlusion(ctx, rays, hits, False)
        b, nb = _occlusion(ctx, recipe, got, True)
        r["occlusion"], r["cut_rays"] = a + b, na + nb
        # 1, last part: the ray cast of the rendered frame
        ctx.render(1)
        lattice = _lattice(cam)
        fields = ("instance", "material_slot", "material", "triangle")
        depth = ctx.read_depth()
        window = np.array([rays[y, x] for x, y in lattice])      # the ray hiprz_ray_cast walks: the pixel's, between 0.99 and 1.01 of its depth
        window["near"] = np.array([depth[y, x] for x, y in lattice], np.float32) * np.float32(0.99)
        window["far"] = np.array([depth[y, x] for x, y in lattice], np.float32) * np.float32(1.01)
        windowed = ctx.trace(window)
        r["ray_cast"] = [(x, y, ctx.ray_cast(x, y), tuple(int(windowed[k][f]) for f in fields), tuple(int(hits[y, x][f]) for f in fields), bool(_found(hits)[y, x]))
                         for k, (x, y) in enumerate(lattice)]
        out[key] = r
    ctx.close()
    _RESULTS[at] = out
    return out


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("tree", TREES)
def test_sweep(built, tree, chunk):
    failures = []
    for key, r in run_chunk(tree, chunk).items():
        s, cap = r["sweep"], GS.scene_cap(key, 0)
        print(f"sweep tree {tree} {key!r}: {s['rays']} pixels, exact {s['exact']}, far {s['far']}, discrete {s['discrete']}, cap {cap}")
        assert r["sweep_misses"], key
        assert r["invalid"] == 0, key
        if s["discrete"]:
            failures.append(f"{key!r}: {s['discrete']} rays differ in a geometric field\n" + "\n".join(s["worst"]))
        elif s["far"] > cap:
            failures.append(f"{key!r}: {s['far']} far rays, cap {cap}\n" + "\n".join(s["worst"]))
        differ = [(x, y, cast, windowed, traced) for x, y, cast, windowed, traced, found in r["ray_cast"] if cast != windowed or (found and cast != traced)]
        if differ:
            failures.append(f"{key!r}: ray_cast != trace on the lattice: {differ[:4]}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tree", TREES)
def test_sweep_totals(built, tree):
    results = {}
    for chunk in range(len(CHUNKS)):
        results.update(run_chunk(tree, chunk))
    assert len(results) == 118
    total = {k: sum(r["sweep"][k] for r in results.values()) for k in ("rays", "exact", "far", "discrete")}
    lattice = sum(len(r["ray_cast"]) for r in results.values())
    met = sum(cast[0] >= 0 for r in results.values() for _, _, cast, *_ in r["ray_cast"])
    beyond = sum(cast[0] >= 0 and not found for r in results.values() for _, _, cast, _, _, found in r["ray_cast"])
    cap = GS.sweep_cap(GS.SCENES, 0)
    print(f"sweep tree {tree}: {total['rays']} pixels on {len(results)} scenes, exact {total['exact']} ({total['exact'] / total['rays']:.4%}), far {total['far']}, "
          f"discrete {total['discrete']}, sweep cap {cap}; ray cast lattice {lattice} pixels, {met} met an instance, {beyond} of them on a pixel whose ray misses within the camera's range")
    assert total["rays"] == 126885 and total["discrete"] == 0 and total["far"] <= cap
    assert met > 5000


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("tree", TREES)
def test_pixel_rays(built, tree, chunk):
    for key, r in run_chunk(tree, chunk).items():
        print(f"pixel rays tree {tree} {key!r}: largest direction error {r['direction_error']:.3e}")
        assert r["origin_bits"] and r["range_bits"], key
        assert r["direction_error"] <= 1e-6, (key, r["direction_error"])
        assert r["normalize_bytes"], f"{key!r}: (position, pixel_d0) under NORMALIZE is not byte-equal to the traced pixel rays"


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("tree", TREES)
def test_arbitrary_rays(built, tree, chunk):
    failures = []
    for key, r in run_chunk(tree, chunk).items():
        s = r["recipe"]
        print(f"recipe tree {tree} {key!r}: {s['rays']} rays, {r['recipe_found']} hit ({r['recipe_internal']} from the inside), exact {s['exact']}, far {s['far']}, discrete {s['discrete']}")
        assert r["recipe_misses"], key
        if r["empty"]:
            assert r["recipe_found"] == 0, key
        if s["discrete"]:
            failures.append(f"{key!r}: {s['discrete']} rays differ in a geometric field\n" + "\n".join(s["worst"]))
        elif s["far"] > GS.scene_cap(key, 0):
            failures.append(f"{key!r}: {s['far']} far rays\n" + "\n".join(s["worst"]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tree", TREES)
def test_arbitrary_rays_totals(built, tree):
    results = {}
    for chunk in range(len(CHUNKS)):
        results.update(run_chunk(tree, chunk))
    total = {k: sum(r["recipe"][k] for r in results.values()) for k in ("rays", "exact", "far", "discrete")}
    found, internal = sum(r["recipe_found"] for r in results.values()), sum(r["recipe_internal"] for r in results.values())
    print(f"recipe tree {tree}: {total['rays']} rays, {found} hit, {internal} from the inside, exact {total['exact']}, far {total['far']}, discrete {total['discrete']}")
    assert total["rays"] >= 3000 and internal >= 500 and total["discrete"] == 0 and total["far"] <= GS.sweep_cap(GS.SCENES, 0)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
@pytest.mark.parametrize("tree", TREES)
def test_occlusion(built, tree, chunk):
    failures, cut = [], 0
    for key, r in run_chunk(tree, chunk).items():
        failures += [f"{key!r}: {f}" for f in r["occlusion"]]
        cut += r["cut_rays"]
    print(f"occlusion tree {tree} chunk {chunk}: {cut} hits, three cut rays each")
    assert not failures, "\n".join(failures)


# =====================================================================================================================
# 5. invalid rays and shapes
# =====================================================================================================================
_LANES = (0, 31, 63, 64, 256)


def _spoil(ray, kind):
    r = ray.copy()
    if kind == "nan origin":
        r["origin"][1] = np.nan
    elif kind == "inf direction":
        r["direction"][0] = np.inf
    elif kind == "-inf origin":
        r["origin"][2] = -np.inf
    elif kind == "nan far":
        r["far"] = np.nan
    elif kind == "inf far":
        r["far"] = np.inf
    elif kind == "zero direction":
        r["direction"] = 0
    elif kind == "far <= near":
        r["far"] = r["near"]
    elif kind == "near < 0":
        r["near"] = -1e-3
    elif kind == "length 2":
        r["direction"] = r["direction"] * np.float32(2)
    else:
        raise KeyError(kind)
    return r


@pytest.fixture(scope="module")
def shapes_context(built):
    ctx = _context(0)
    _upload(ctx, "inside_sphere")           # every valid ray hits: an invalid one cannot pass for a miss
    rays = ctx.pixel_rays().reshape(-1)[:257].copy()
    yield ctx, rays
    ctx.close()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", ["nan origin", "inf direction", "-inf origin", "nan far", "inf far", "zero direction", "far <= near", "near < 0", "length 2"])
def test_invalid_rays(shapes_context, kind, normalize):
    ctx, rays = shapes_context
    clean, clean_occ = ctx.trace(rays, normalize), ctx.occluded(rays, normalize)
    assert _found(clean).all() and clean_occ.all()
    batch = rays.copy()
    for lane in _LANES:
        batch[lane] = _spoil(rays[lane], kind)
    hits, occ = ctx.trace(batch, normalize), ctx.occluded(batch, normalize)
    spoiled = np.zeros(len(rays), bool)
    spoiled[list(_LANES)] = True
    assert hits[~spoiled].tobytes() == clean[~spoiled].tobytes() and np.array_equal(occ[~spoiled], clean_occ[~spoiled]), "a valid ray reads otherwise beside invalid ones"
    if kind == "length 2" and normalize:         # a valid ray under NORMALIZE: the same unit direction (a power of two scales exactly)
        assert hits.tobytes() == clean.tobytes() and np.array_equal(occ, clean_occ)
        return
    bad = hits[spoiled]
    assert (bad["flags"] == HIT_INVALID).all(), bad["flags"]
    assert (bad["t"].view(np.uint32) == batch["far"][spoiled].view(np.uint32)).all(), "t is not the input far's bits"
    for name, value in (("instance", -1), ("material_slot", -1), ("material", -1), ("triangle", 0), ("scene_triangle", -1)):
        assert (bad[name] == value).all(), name
    assert (bad["u"].view(np.uint32) == 0).all() and (bad["v"].view(np.uint32) == 0).all() and (bad["normal"].view(np.uint32) == 0).all()
    assert not occ[spoiled].any()


@pytest.mark.parametrize("normalize", [False, True])
def test_shapes_and_device_pointers(shapes_context, normalize):
    ctx, rays = shapes_context
    q, pad = ctx.query(), 8
    for n in (0, 1, 63, 64, 65, 257):
        host_hits, host_occ = ctx.trace(rays[:n], normalize), ctx.occluded(rays[:n], normalize)
        assert host_hits.shape == (n,) and host_occ.shape == (n,)
        d_rays = _hiprt.DeviceBuffer.of(rays) if n else _hiprt.DeviceBuffer(32)
        d_hits = _hiprt.DeviceBuffer.of(np.full((n + pad) * hit_dtype.itemsize, 0xAB, np.uint8))
        d_occ = _hiprt.DeviceBuffer.of(np.full(n + pad, 0xABABABAB, np.uint32))
        try:
            q.closest_device(d_rays.ptr, n, d_hits.ptr, normalize)
            q.occluded_device(d_rays.ptr, n, d_occ.ptr, normalize)
            ctx.sync()
            hits, occ = d_hits.download(((n + pad) * hit_dtype.itemsize,), np.uint8), d_occ.download((n + pad,), np.uint32)
        finally:
            d_rays.free(), d_hits.free(), d_occ.free()
        assert hits[:n * hit_dtype.itemsize].tobytes() == host_hits.tobytes(), n
        assert (hits[n * hit_dtype.itemsize:] == 0xAB).all(), f"n = {n}: a record behind n was written"
        assert np.array_equal(occ[:n], host_occ) and (occ[n:] == 0xABABABAB).all(), n


def test_device_view_guards(built):
    """the guard against a query library built from other headers: byte counts that are not sizeof(DScene) / sizeof(DCamera) as libhiprz.so was
    compiled are refused, before the state is looked at and with nothing written; then the state rules"""
    lib = _lib.load()
    S, K = QR.device_view_sizes()
    scene, camera = (C.c_uint8 * (S + 16))(), (C.c_uint8 * (K + 16))()
    untouched = lambda: not any(scene) and not any(camera)
    ctx = Context(0)
    try:
        for state in ("nothing", "scene", "scene and camera"):
            C.memset(scene, 0, len(scene)), C.memset(camera, 0, len(camera))
            if state == "scene":
                ctx.upload_scene(GS.flat_scene("slots")[0])
            if state == "scene and camera":
                ctx.upload_camera(GS.flat_scene("slots")[1])
            for sizes in ((S - 1, K), (S + 1, K), (S + 16, K), (0, K), (S, K - 4), (S, K + 4), (K, S), (0, 0)):
                assert lib.hiprz_device_view(ctx._ctx, scene, sizes[0], camera, sizes[1]) == _abi.ERR_INVALID, (state, sizes)
                assert b"device_view" in lib.hiprz_last_error(ctx._ctx)
            assert lib.hiprz_device_view(ctx._ctx, scene, S, camera, 0) == _abi.ERR_INVALID, state      # a camera with no bytes
            assert lib.hiprz_device_view(ctx._ctx, scene, S, None, K) == _abi.ERR_INVALID, state        # no camera with bytes
            assert lib.hiprz_device_view(ctx._ctx, None, S, camera, K) == _abi.ERR_INVALID, state
            assert lib.hiprz_device_view(ctx._ctx, scene, S - 1, None, 0) == _abi.ERR_INVALID, state
            assert untouched(), state
            both, alone = lib.hiprz_device_view(ctx._ctx, scene, S, camera, K), lib.hiprz_device_view(ctx._ctx, scene, S, None, 0)
            assert (both, alone) == {"nothing": (_abi.ERR_STATE, _abi.ERR_STATE), "scene": (_abi.ERR_STATE, _abi.OK), "scene and camera": (_abi.OK, _abi.OK)}[state], state
        assert any(scene[:S]) and any(camera[:K]) and not any(scene[S:]) and not any(camera[K:]), "the views are copied, and nothing behind them"
        width = int.from_bytes(bytes(camera[48:52]), "little")      # DCamera::width follows position and the three axes
        assert width == GS.flat_scene("slots")[1].width
    finally:
        ctx.close()


def test_refusals(built):
    ctx = _context(0)
    try:
        rays = query.rays([[0, 0, 0]], [[0, 0, 1]], 0.0, 1.0)
        with pytest.raises(HiprzError) as e:
            ctx.trace(rays)
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value), e.value
        assert ctx.trace(rays[:0]).shape == (0,)                                     # n == 0: HIPRZ_OK, nothing is launched
        flat = _upload(ctx, "slots")[0]
        q = ctx.query()
        assert q.lib.hiprz_query_closest(q._query, None, 1, 0, None, None) != 0 and b"null pointer" in q.lib.hiprz_query_last_error(q._query)
        assert q.lib.hiprz_query_closest_host(q._query, rays.ctypes.data, 1, 2, rays.ctypes.data) != 0 and b"unknown flag" in q.lib.hiprz_query_last_error(q._query)
        assert len(flat.instances) and ctx.trace(rays).shape == (1,)
        fresh = Context(0)                    # no camera: pixel rays are refused, a trace is not
        try:
            fresh.upload_scene(flat)
            assert fresh.trace(rays).tobytes() == ctx.trace(rays).tobytes()
            with pytest.raises(HiprzError) as e:
                fresh.query().pixel_rays_device(1)
            assert e.value.code == _abi.ERR_STATE and "no camera" in str(e.value)
        finally:
            fresh.close()
    finally:
        ctx.close()


# =====================================================================================================================
# 6. staleness
# =====================================================================================================================
def _sphere_world(moved=False, deformed=False):
    world = scenes.textured_sphere_scene(48, 32, resolution=24, map_size=32)
    inst = next(i for i in world.instances if i.name == "bugatti stand-in")
    if deformed:
        v = inst.mesh.vertices
        inst.mesh.vertices = np.ascontiguousarray(v * np.array([1.0, 1.25, 0.9], np.float32) + np.sin(v[:, [1, 2, 0]] * 7.0).astype(np.float32) * np.float32(0.03), dtype=np.float32)
    if moved:
        inst.position = (np.asarray(inst.position, np.float32) + np.array([0.25, -0.1, 0.2], np.float32)).astype(np.float32)
        inst.rotation = (np.asarray(inst.rotation, np.float32) + np.array([0.1, 0.4, 0.0], np.float32)).astype(np.float32)
    return world


def _uploaded_order(world0, flat0, new):
    """position in flat0's triangle order -> flat `new`'s record of the same triangle (meshes keep their ranges: same meshes, same counts)"""
    order, done, seen = np.empty(len(flat0.tris), np.int64), 0, set()
    for inst in world0.instances:
        if inst.mesh is None or id(inst.mesh) in seen:
            continue
        seen.add(id(inst.mesh))
        T = len(inst.mesh.tri_vertices)
        where = np.empty(T, np.int64)
        where[new.tris["source_index"][done:done + T]] = np.arange(T)
        order[done:done + T] = done + where[flat0.tris["source_index"][done:done + T]]
        done += T
    assert done == len(flat0.tris)
    return order


def _fresh_trace(flat, rays):
    ctx = Context(0)
    try:
        ctx.upload_scene(flat)
        return ctx.trace(rays)
    finally:
        ctx.close()


def test_a_query_sees_every_update(built):
    worlds = dict(plain=_sphere_world(), moved=_sphere_world(moved=True), changed=_sphere_world(moved=True, deformed=True))
    flats = {k: flatten(w) for k, w in worlds.items()}
    cam = camera_struct(worlds["plain"].camera)
    other = GS.flat_scene("slots")[0]
    ctx = _context(3)
    try:
        ctx.upload_scene(other), ctx.upload_camera(cam)
        rays = ctx.pixel_rays().reshape(-1)
        want = {k: _fresh_trace(f, rays) for k, f in flats.items()}
        before = ctx.trace(rays)
        assert before.tobytes() == _fresh_trace(other, rays).tobytes()
        ctx.upload_scene(flats["plain"])
        got = ctx.trace(rays)
        assert got.tobytes() == want["plain"].tobytes() and got.tobytes() != before.tobytes(), "after upload_scene"
        assert _found(got).sum() > 500
        assert np.array_equal(flats["moved"].tris, flats["plain"].tris)        # only the instance records change
        ctx.update_instances(flats["moved"].instances)
        moved = ctx.trace(rays)
        assert moved.tobytes() == want["moved"].tobytes() and moved.tobytes() != got.tobytes(), "after update_instances"
        order = _uploaded_order(worlds["plain"], flats["plain"], flats["changed"])
        ctx.update_triangles(0, flats["changed"].tris[order], flats["changed"].tri_attrs[order])

        def same_as_fresh(hits, what):
            as_fresh = hits.copy()           # scene_triangle counts in the order this context was given: into the changed scene's order
            found = _found(hits)
            as_fresh["scene_triangle"][found] = order[hits["scene_triangle"][found]]
            assert as_fresh.tobytes() == want["changed"].tobytes(), what
        refitted = ctx.trace(rays)
        same_as_fresh(refitted, "after update_triangles")
        assert refitted.tobytes() != moved.tobytes()
        assert (refitted["t"] != moved["t"]).sum() > 100
        ctx.rebuild_trees(3)
        same_as_fresh(ctx.trace(rays), "after rebuild_trees")
        assert np.array_equal(ctx.occluded(rays), _found(want["changed"]).astype(np.uint32))
    finally:
        ctx.close()


# =====================================================================================================================
# 7. off means off
# =====================================================================================================================
_CALLS = (1, 3, 8, 2, 8)


def _frame_context(kind):
    ctx = Context([0, 0]) if kind == "two-streams" else Context(0)
    if kind == "shard":
        ctx.set_shard(1, 4)
    return ctx


@pytest.mark.parametrize("kind", ["single", "two-streams", "shard"])
def test_querying_changes_nothing_else(built, kind):
    world = scenes.shading_inputs_scene(80, 48, lights=True)
    flat, cam = flatten(world), camera_struct(world.camera)
    results, traced = [], None
    for ask in (True, False):
        ctx = _frame_context(kind)
        try:
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(None, Tracing(6, 4)).struct())
            for k, n in enumerate(_CALLS):
                ctx.render(n)
                if ask and k + 1 < len(_CALLS):
                    rays = ctx.pixel_rays()
                    traced = ctx.trace(rays)
                    assert np.array_equal(ctx.occluded(rays), _found(traced).astype(np.uint32))
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.ray_count(), ctx.pass_count(),
                            ctx.graph_captures(), ctx.read_guides().tobytes()))
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "ray_count", "pass_count", "graph_captures", "guides"), *results):
        assert a == b, f"{kind}: {name} differs once rays are queried between the render calls"
    # the query answers for the whole scene, whatever share of the frame the context renders
    want = QR.as_hits(oracle.first_hits(flat, cam, 0, threads=THREADS))
    r = QR.compare(traced, want)
    print(f"{kind}: {r}")
    assert r["discrete"] == 0 and r["far"] <= 2 and _found(traced).sum() > 1000


# =====================================================================================================================
# 8. the C++ host
# =====================================================================================================================
@pytest.mark.parametrize("normalize", [0, 1])
def test_cpp_engine_casts_rays(built, tmp_path, normalize):
    exe = str(tmp_path / "query_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "query_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "sphere.json")
    scene_io.save_scene_json(scenes.textured_sphere_scene(48, 32, resolution=24, map_size=32), scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        rays = ctx.pixel_rays().reshape(-1)
        if normalize:
            rays = rays.copy()
            rays["direction"] *= np.linspace(0.5, 3.0, len(rays), dtype=np.float32)[:, None]
        rays["far"][5] = 0.0            # an invalid ray travels through the C++ host as well
        want_hits, want_occ = ctx.trace(rays, bool(normalize)), ctx.occluded(rays, bool(normalize))
    finally:
        ctx.close()
        loaded.close()
    assert want_hits[5]["flags"] == HIT_INVALID and _found(want_hits).sum() > 500
    rays.tofile(str(tmp_path / "rays.bin"))
    r = subprocess.run([exe, scene_path, str(tmp_path / "rays.bin"), str(tmp_path / "out.bin"), str(normalize)], capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "QUERY DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = open(tmp_path / "out.bin", "rb").read()
    n = len(rays)
    assert len(out) == n * (hit_dtype.itemsize + 4)
    assert out[:n * hit_dtype.itemsize] == want_hits.tobytes(), "Engine::castRays differs from Context.trace"
    assert out[n * hit_dtype.itemsize:] == want_occ.tobytes(), "Engine::occluded differs from Context.occluded"


GROWTH = (1, 4096, 4097, 8193, 1)      # on one new handle: a staging of 4096 made, kept, grown to 8192, grown to 16 384, kept


def test_one_handle_grows_its_staging_twice(shapes_context):
    """Host-pointer calls of GROWTH's sizes on one handle of its own, closest and occluded taking turns to go first (the out side of the
    staging is sized for hits; the occlusion words share it): every result equals, byte for byte, the device-pointer call over the same
    rays.  The rays leave the camera of `inside_sphere` in 8 193 directions of their own, so every one hits."""
    ctx, pixel = shapes_context
    d = np.random.default_rng(22).normal(size=(max(GROWTH), 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(-1, dtype=np.float32))[:, None]
    rays = query.rays(pixel["origin"][0], d, pixel["near"][0], pixel["far"][0])
    q = query.Query(ctx._ctx)
    ctx.sync()      # (makes the head device the current one for the buffers)
    d_rays, d_hits, d_occ = _hiprt.DeviceBuffer.of(rays), _hiprt.DeviceBuffer(rays.size * hit_dtype.itemsize), _hiprt.DeviceBuffer(rays.size * 4)
    try:
        for turn, n in enumerate(GROWTH):
            got = {}
            for call in (q.closest, q.occluded)[::1 if turn % 2 == 0 else -1]:
                got[call.__name__] = call(rays[:n])
            q.closest_device(d_rays.ptr, n, d_hits.ptr)
            q.occluded_device(d_rays.ptr, n, d_occ.ptr)
            ctx.sync()
            hits, occ = d_hits.download((n,), hit_dtype), d_occ.download((n,), np.uint32)
            assert _found(hits).all() and occ.all(), n
            assert got["closest"].tobytes() == hits.tobytes(), f"turn {turn}, n = {n}: closest through the staging"
            assert got["occluded"].tobytes() == occ.tobytes(), f"turn {turn}, n = {n}: occluded through the staging"
    finally:
        d_rays.free(), d_hits.free(), d_occ.free()
        q.close()
