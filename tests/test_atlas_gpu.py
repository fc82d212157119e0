"""Bake atlases on the GPU (include/hiprz_atlas.h: libhiprz_atlas.so, Context.atlas_points / bake_atlas, Engine::bakeAtlas).  The owner
map, the samples and the points of an atlas are held to the numpy float32 restatement (tests/atlas_reference.py, itself held to answers
worked by hand by tests/test_atlas_reference.py) in every byte; a baked atlas to Context.bake_occlusion on the points read back; the
dilation to the restatement in every byte.

THE WORLD of every case (_world): a floor (generate_plane(4), scale 4) with a sphere (generate_sphere(16), scale (2, 0.5, 3), rotated)
and a cube (mirrored scale (-1, 1, 1.5), rotated) resting on it, and one more sphere at unit scale: the three kinds of placement.

  1 bytes        samples (their `triangle` is the owner map) and points == the restatement in every byte: the charts of the count table
                 of tests/test_atlas_reference.py, a mirrored copy, and sphere 8 with five triangles spoiled (NaN, infinity, zero area,
                 UVs wholly and partly outside [0, 1]); atlases 1x1, 7x5, 8x8, 9x9, 64x64, 65x33, 256x1; every placement; through host
                 and device pointers; guard words behind the handle's points, samples and records (written through the device
                 addresses while the handle holds a larger atlas, read back behind W*H afterwards).
  2 adds         two parts with disjoint id ranges in either order == one add of both; a second begin forgets the first; n == 0 clears.
  3 bake         bake_atlas texels == Context.bake_occlusion on the points read back, byte for byte, K = 16 and 64, trees 0 and 3; rings = 0
                 there, and with rings = 2 the dilation of those texels by the restatement.  THE SCENE CONDITION, checked with the oracle
                 on the CPU when the test was written (tests/query_reference.oracle_rays over tests/bake_reference.rays of the floor's
                 points in a 32x32 atlas, K = 16): 369 of the floor's 484 covered texels, 76.2 %, have 0 < occluded < K (113 lie under the
                 sphere and the cube with all 16 rays occluded, 2 see the open sky); asserted again on the device's texels, at least a tenth.
  4 dilation     texels and ring map == the restatement for rings 0, 1, 2 and 64 on the sphere atlases, on an atlas with no covered texel
                 and on a fully covered one, with guard words behind the records and the ring map; the host-pointer call equals the
                 device-pointer call.
  5 staleness    after update_instances a new begin/add equals the restatement under the new placement and differs from the atlas before.
  6 off = off    renders with atlas builds and dilations between the render calls equal renders without.
  7 refusals     each refusal of hiprz_atlas_add, and of the calls that need an add.
  8 C++          Engine::bakeAtlas through tests/atlas_delivery_check.cpp, byte-equal to Context.bake_atlas.

MEASURED ON MI355X: 19 cases in 2.3 s beside the session's build fixture, slowest case 0.6 s (the C++ host: it compiles a program), then
0.3 s (case 6 on two streams).  Case 1: 96 960 covered texels compared over the seven atlases (18, 507, 963, 1 203, 59 067, 30 816, 4 386),
six chart sets and three placements, every byte equal.  Case 3: 369 of the floor's 484 texels partly occluded at K = 16 — the oracle's
figure — and 421 at K = 64, on both trees.  Case 8: 65x33, 1 881 covered, 264 filled by 2 rings, 0 empty.  No fault was found in the four
kernels.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atlas_reference as AR
from rayzath_amd import _abi, _hiprt, atlas, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.atlas import NONE, sample_dtype
from rayzath_amd.bake import INVALID, point_dtype, texel_dtype
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, World, camera_struct, flatten, generate_cube, generate_plane, generate_sphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
ATLASES = ((1, 1), (7, 5), (8, 8), (9, 9), (64, 64), (65, 33), (256, 1))
FLOOR, SCALED, MIRRORED, UNIT = 0, 1, 2, 3          # instance indices of _world
PAD, GUARD = 8, 0xABABABAB
NEAR, FAR = 1e-3, 1e3
F = np.float32


def _world(moved=False):
    world = World()
    grey = world.add(Material((200, 200, 200, 255), 0.0, 0.8, name="grey"))
    plane, sphere, cube = world.add(generate_plane(4)), world.add(generate_sphere(16)), world.add(generate_cube())
    world.add(Instance(plane, [grey], position=(0, 0, 0), scale=(4, 1, 4), name="floor"))
    world.add(Instance(sphere, [grey], position=(0.6, 0.5, 0.4) if not moved else (-0.9, 0.7, 1.1), rotation=(0, 0.6, 0) if not moved else (0.2, 1.4, 0.1),
                       scale=(2, 0.5, 3), name="scaled sphere"))
    world.add(Instance(cube, [grey], position=(-1.6, 0.5, -1.2), rotation=(0, 0.4, 0), scale=(-1, 1, 1.5), name="mirrored cube"))
    world.add(Instance(sphere, [grey], position=(0.5, 3.0, -2.5), name="unit sphere"))
    world.camera = Camera(position=(0, 3, -8), resolution=(48, 32))
    world.camera.look_at((0, 0, 0))
    return world


def _mirrored(t):
    """the same charts with vertices 2 and 3 exchanged: every orientation flips"""
    m = t.copy()
    for a in "punv":
        m[a + "2"], m[a + "3"] = t[a + "3"], t[a + "2"]
    return m


def _spoiled(t):
    """sphere 8 with triangles 3, 11, 19, 27 and 35 spoiled: NaN, infinity, zero area, UVs wholly outside, UVs partly outside"""
    s = t.copy()
    s["p2"][3, 1] = np.nan
    s["n1"][11, 0] = np.inf
    s["u3"][19], s["v3"][19] = s["u2"][19], s["v2"][19]
    for k in "123":
        s["u" + k][27] += F(2.0)
    s["u2"][35] += F(0.75)
    s["v3"][35] -= F(0.5)
    return s


def _charts():
    sphere16, sphere8 = atlas.charts(generate_sphere(16)), atlas.charts(generate_sphere(8))
    return dict(cube=atlas.charts(generate_cube()), sphere16=sphere16, sphere8=sphere8, plane4=atlas.charts(generate_plane(4)), mirrored=_mirrored(sphere16),
                spoiled=_spoiled(sphere8))


CHARTS = _charts()


@pytest.fixture(scope="module")
def scene(built):
    world = _world()
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(None, Tracing(4, 2)).struct())
    yield ctx, flat
    ctx.close()


def _copy_to(ptr, array):
    _hiprt._check(_hiprt.runtime().hipMemcpy(ptr, array.ctypes.data, array.nbytes, 1), "hipMemcpy (host to device)")


def _copy_from(ptr, offset, words):
    out = np.zeros(words, np.uint32)
    _hiprt._check(_hiprt.runtime().hipMemcpy(out.ctypes.data, C.c_void_p(ptr + offset), out.nbytes, 2), "hipMemcpy (device to host)")
    return out


def _guarded_build(ctx, a, W, H, add):
    """begin(W, H) + add(a) on a handle whose arrays hold W*H + PAD texels and GUARD words everywhere; (points, samples) read back, the
    words behind W*H asserted"""
    n = W * H
    a.begin(n + PAD, 1)
    a.add(CHARTS["cube"][:0])                       # allocates and clears
    ctx.sync()
    arrays = ((a.points_device(), 8), (a.samples_device(), 4), (a.records_device(), 4))
    for ptr, words in arrays:
        _copy_to(ptr, np.full((n + PAD) * words, GUARD, np.uint32))
    a.begin(W, H)
    add(a)
    ctx.sync()
    assert [a.points_device(), a.samples_device(), a.records_device()] == [p for p, _ in arrays], "a smaller atlas keeps the arrays"
    for (ptr, words), name in zip(arrays, ("points", "samples", "records")):
        behind = _copy_from(ptr, n * words * 4, PAD * words)
        assert (behind == GUARD).all(), f"{W}x{H}: {name} behind W*H were written"
    assert (_copy_from(arrays[2][0], 0, n * 4) == GUARD).all(), "the library never writes the records"
    return a.read()


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        differ = (got.reshape(-1).view(np.uint32).reshape(got.size, -1) != want.reshape(-1).view(np.uint32).reshape(want.size, -1)).any(-1)
        at = int(np.argmax(differ))
        raise AssertionError(f"{what}: {int(differ.sum())} of {got.size} differ, first at texel {at}: {got.reshape(-1)[at]} != {want.reshape(-1)[at]}")


# =====================================================================================================================
# 1. bytes
# =====================================================================================================================
@pytest.mark.parametrize("W,H", ATLASES, ids=lambda v: str(v))
def test_the_atlas_is_the_restated_atlas(scene, W, H):
    ctx, flat = scene
    a = ctx.atlas()
    covered = 0
    for name, tris in CHARTS.items():
        owner = AR.cover(tris, W, H, 5)[0]
        for instance in (SCALED, MIRRORED, UNIT):
            want_owner, want_samples, want_points = AR.build([(AR.placement_of(flat.instances[instance]), tris)], W, H, NEAR, FAR)
            assert np.array_equal(want_owner, np.where(owner == NONE, owner, owner - 5))
            points, samples = _guarded_build(ctx, a, W, H, lambda h: h.add(tris, 0, instance, NEAR, FAR))
            _same(samples, want_samples, f"{name} {W}x{H} instance {instance}: samples")
            _same(points, want_points, f"{name} {W}x{H} instance {instance}: points")
            assert np.array_equal(samples["triangle"], want_owner)
            covered += int((want_owner != NONE).sum())
        # the same through a device pointer, with a base: the ids move, nothing else
        ctx.sync()
        d_tris = _hiprt.DeviceBuffer.of(tris)
        try:
            a.begin(W, H)
            a.add_device(d_tris.ptr, len(tris), 5, UNIT, NEAR, FAR)
            points, samples = a.read()
        finally:
            d_tris.free()
        _same(samples["triangle"], owner, f"{name} {W}x{H}: owner through a device pointer")
        _same(points, want_points, f"{name} {W}x{H}: points through a device pointer")
        assert np.array_equal(samples["bx"].view(np.uint32), want_samples["bx"].view(np.uint32)) and not samples["zero"].any()
    if W * H > 1:
        assert covered > 0
    spoiled_owner = AR.cover(CHARTS["spoiled"], W, H)[0]
    assert not np.isin(spoiled_owner, (3, 11, 19, 27)).any(), "a degenerate triangle or one outside the atlas owns a texel"
    print(f"{W}x{H}: {covered} covered texels compared over {len(CHARTS)} charts and 3 placements")


def test_the_normals_of_the_placements(scene):
    """what the bytes of case 1 mean: on the unit sphere the normal of a point is its direction from the centre (scaled: perpendicular to
    the ellipsoid), the cube's face normals survive the mirrored scale as unit vectors, and every covered texel is a valid point"""
    ctx, flat = scene
    points, samples = ctx.atlas_points([(UNIT, CHARTS["sphere16"])], 64, 64, NEAR, FAR)
    has = samples["triangle"] != NONE
    assert has.sum() == 3584 and points.dtype == point_dtype and samples.dtype == sample_dtype and points.shape == (64, 64)
    centre = flat.instances[UNIT]["position"]
    radial = points["position"][has] - centre
    radial /= np.linalg.norm(radial, axis=-1, keepdims=True)
    assert (np.einsum("ij,ij->i", radial, points["normal"][has]) > 0.97).all()
    points, samples = ctx.atlas_points([(MIRRORED, CHARTS["cube"])], 9, 9, NEAR, FAR)
    assert (samples["triangle"] < 2).all() and np.abs(np.linalg.norm(points["normal"], axis=-1) - 1).max() < 1e-6
    assert np.abs(points["normal"][..., 1]).min() > 0.999, "triangles 0 and 1 are the cube's top face: the normal is +-y under a rotation about y"
    assert (points["near"] == F(NEAR)).all() and (points["far"] == F(FAR)).all()


# =====================================================================================================================
# 2. adds
# =====================================================================================================================
def test_adds_in_either_order_are_one_add(scene):
    ctx, flat = scene
    a = ctx.atlas()
    cube, sphere = CHARTS["cube"][:1], CHARTS["sphere16"]          # one triangle: half the atlas, with the lowest id
    for W, H in ((65, 33), (7, 5), (64, 64)):
        parts = [(AR.placement_of(flat.instances[MIRRORED]), cube), (AR.placement_of(flat.instances[SCALED]), sphere)]
        want_owner, want_samples, want_points = AR.build(parts, W, H, NEAR, FAR)
        assert (want_owner < len(cube)).any() and ((want_owner >= len(cube)) & (want_owner != NONE)).any(), "both parts own texels"
        results = []
        for order in ((0, 1), (1, 0)):
            a.begin(W, H)
            for k in order:
                a.add((cube, sphere)[k], (0, len(cube))[k], (MIRRORED, SCALED)[k], NEAR, FAR)
            results.append(a.read())
        for points, samples in results:
            _same(samples, want_samples, f"{W}x{H}: samples of two parts")
            _same(points, want_points, f"{W}x{H}: points of two parts")
        # the sphere in two halves with ids of their own == the sphere at once
        a.begin(W, H)
        a.add(sphere[100:], 100, SCALED, NEAR, FAR), a.add(sphere[:100], 0, SCALED, NEAR, FAR)
        halves = a.read()
        a.begin(W, H)
        a.add(sphere, 0, SCALED, NEAR, FAR)
        whole = a.read()
        _same(halves[0], whole[0], "points of two halves"), _same(halves[1], whole[1], "samples of two halves")
        # a second begin forgets the first; n == 0 clears
        a.begin(W, H)
        a.add(cube[:0], 0, UNIT, NEAR, FAR)
        points, samples = a.read()
        assert (samples["triangle"] == NONE).all() and not points.view(np.uint32).any() and not samples["bx"].view(np.uint32).any() and not samples["zero"].any()
        a.add(sphere, 0, SCALED, NEAR, FAR)                                         # a later add on the cleared atlas
        _same(a.read()[0], whole[0], "an add after an empty first add")
        a.add(cube[:0], 900, UNIT, NEAR, FAR)                                       # a later empty add changes nothing
        _same(a.read()[1], whole[1], "an empty later add")


# =====================================================================================================================
# 3. bake composition
# =====================================================================================================================
@pytest.mark.parametrize("tree", (0, 3))
def test_a_baked_atlas_is_the_bake_of_its_points(built, tree):
    world = _world()
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx = Context(0)
    try:
        if tree:
            ctx.set_tree(tree)
        ctx.upload_scene(flat), ctx.upload_camera(cam)
        W = H = 32
        parts = [(FLOOR, CHARTS["plane4"]), (SCALED, CHARTS["sphere16"])]
        points, samples = ctx.atlas_points(parts, W, H, NEAR, FAR)
        floor = samples["triangle"] < 2
        assert floor.sum() == 484 and ((samples["triangle"] >= 2) & (samples["triangle"] != NONE)).any() and (samples["triangle"] == NONE).any()
        for K in (16, 64):
            want = ctx.bake_occlusion(points, (K, 4), 20261020)
            texels, got_samples, ring = ctx.bake_atlas(parts, W, H, (K, 4), 20261020, rings=0, near=NEAR, far=FAR)
            _same(texels, want, f"tree {tree} K {K}: texels")
            _same(got_samples, samples, "samples")
            assert np.array_equal(ring == 0, samples["triangle"] != NONE) and (ring[ring != 0] == NONE).all()
            assert (want["occluded"][samples["triangle"] == NONE] == INVALID).all(), "an uncovered texel is an invalid point"
            assert (want["occluded"][samples["triangle"] != NONE] <= K).all(), "a covered texel is a valid point"
            partial = (want["occluded"][floor] > 0) & (want["occluded"][floor] < K)
            print(f"tree {tree} K {K}: {int(partial.sum())} of {int(floor.sum())} floor texels partly occluded")
            assert partial.sum() * 10 >= floor.sum(), "the scene condition: a tenth of the floor is partly shadowed"
            texels2, _, ring2 = ctx.bake_atlas(parts, W, H, (K, 4), 20261020, rings=2, near=NEAR, far=FAR)
            want2, want_ring2 = AR.dilate(want, samples, 2)
            _same(texels2, want2, f"tree {tree} K {K}: dilated texels")
            assert np.array_equal(ring2, want_ring2) and (ring2 == 1).any()
    finally:
        ctx.close()


# =====================================================================================================================
# 4. dilation
# =====================================================================================================================
def _dilation_case(ctx, a, records, samples, rings):
    W, H = a.width, a.height
    n = W * H
    want, want_ring = AR.dilate(records, samples, rings)
    ctx.sync()
    d_rec = _hiprt.DeviceBuffer.of(np.concatenate([records.reshape(-1).view(np.uint32), np.full(PAD * 4, GUARD, np.uint32)]))
    d_ring = _hiprt.DeviceBuffer.of(np.full(n + PAD, GUARD, np.uint32))
    try:
        a.dilate_device(d_rec.ptr, rings, d_ring.ptr)
        ctx.sync()
        rec, ring = d_rec.download(((n + PAD) * 4,), np.uint32), d_ring.download((n + PAD,), np.uint32)
        assert (rec[n * 4:] == GUARD).all() and (ring[n:] == GUARD).all(), "a record or a ring word behind W*H was written"
        _same(rec[:n * 4].view(texel_dtype).reshape(H, W), want, f"{W}x{H} rings {rings}: records")
        assert np.array_equal(ring[:n].reshape(H, W), want_ring), f"{W}x{H} rings {rings}: ring map"
        a.dilate_device(d_rec.ptr, 0, None)            # without a ring map and without rings: nothing to write
        ctx.sync()
        assert d_rec.download(((n + PAD) * 4,), np.uint32).tobytes() == rec.tobytes()
    finally:
        d_rec.free(), d_ring.free()
    host, host_ring = a.dilate(records, rings)
    _same(host, want, f"{W}x{H} rings {rings}: host-pointer call")
    assert np.array_equal(host_ring, want_ring)
    return want_ring


@pytest.mark.parametrize("W,H", ((64, 64), (65, 33), (7, 5)), ids=lambda v: str(v))
def test_dilation_is_the_restated_dilation(scene, W, H):
    ctx, flat = scene
    a = ctx.atlas()
    rng = np.random.default_rng(W * 100 + H)
    records = rng.integers(0, 2**32, (H, W, 4), dtype=np.uint32).view(texel_dtype).reshape(H, W)        # any 16 bytes: NaN patterns included
    cases = (("sphere", CHARTS["sphere16"]), ("mirrored", CHARTS["mirrored"]), ("none", CHARTS["cube"][:0]), ("full", CHARTS["cube"]))
    for name, tris in cases:
        a.begin(W, H)
        a.add(tris, 0, UNIT, NEAR, FAR)
        samples = a.read(points=False)[1]
        has = samples["triangle"] != NONE
        assert dict(sphere=0 < has.sum() < W * H, mirrored=0 < has.sum() < W * H, none=not has.any(), full=has.all())[name]
        for rings in (0, 1, 2, 64):
            ring = _dilation_case(ctx, a, records, samples, rings)
            if name == "none":
                assert (ring == NONE).all()
            elif name == "full":
                assert not ring.any()
            elif rings == 64:
                assert (ring != NONE).all() and ring.max() >= 1, "64 rings fill these atlases"


# =====================================================================================================================
# 5. staleness
# =====================================================================================================================
def test_an_atlas_sees_update_instances(built):
    worlds = _world(), _world(moved=True)
    flats = [flatten(w) for w in worlds]
    ctx = Context(0)
    try:
        ctx.set_tree(3)
        ctx.upload_scene(flats[0]), ctx.upload_camera(camera_struct(worlds[0].camera))
        tris = CHARTS["sphere16"]
        before = ctx.atlas_points([(SCALED, tris)], 65, 33, NEAR, FAR)
        _same(before[0], AR.build([(AR.placement_of(flats[0].instances[SCALED]), tris)], 65, 33, NEAR, FAR)[2], "before the update")
        ctx.update_instances(flats[1].instances)
        after = ctx.atlas_points([(SCALED, tris)], 65, 33, NEAR, FAR)
        _same(after[0], AR.build([(AR.placement_of(flats[1].instances[SCALED]), tris)], 65, 33, NEAR, FAR)[2], "after update_instances")
        assert after[0].tobytes() != before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), "the placement moves the points, not the samples"
        _same(ctx.atlas_points([(FLOOR, CHARTS["plane4"])], 65, 33, NEAR, FAR)[0],
              AR.build([(AR.placement_of(flats[0].instances[FLOOR]), CHARTS["plane4"])], 65, 33, NEAR, FAR)[2], "an instance that did not move")
    finally:
        ctx.close()


# =====================================================================================================================
# 6. nothing else changes
# =====================================================================================================================
_CALLS = (1, 3, 8, 2, 8)


@pytest.mark.parametrize("kind", ["single", "two-streams"])
def test_atlases_change_nothing_else(built, kind):
    world = scenes.shading_inputs_scene(80, 48, lights=True)
    flat, cam = flatten(world), camera_struct(world.camera)
    results = []
    for ask in (True, False):
        ctx = Context([0, 0]) if kind == "two-streams" else Context(0)
        try:
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(None, Tracing(6, 4)).struct())
            for k, n in enumerate(_CALLS):
                ctx.render(n)
                if ask and k + 1 < len(_CALLS):
                    texels, samples, ring = ctx.bake_atlas([(k % len(flat.instances), CHARTS["sphere16"])], 65, 33, (16, 2), k, rings=k, near=NEAR, far=FAR)
                    points = ctx.atlas_points([(0, CHARTS["cube"])], 9, 9)[0]
            if ask:
                assert (samples["triangle"] != NONE).sum() == 1881 and (ring != NONE).all() and ring.max() == 2, "the sphere atlas is full after two of the three rings"
                assert np.abs(np.linalg.norm(points["normal"], axis=-1) - 1).max() < 1e-5
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.ray_count(), ctx.pass_count(),
                            ctx.graph_captures(), ctx.read_guides().tobytes()))
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "ray_count", "pass_count", "graph_captures", "guides"), *results):
        assert a == b, f"{kind}: {name} differs once atlases are built between the render calls"


# =====================================================================================================================
# 7. refusals
# =====================================================================================================================
def test_refusals(built):
    world = _world()
    flat = flatten(world)
    ctx = Context(0)
    try:
        a = ctx.atlas()
        lib, h = a.lib, a._atlas
        tris = CHARTS["cube"]
        p = tris.ctypes.data                       # (every call below is refused before a pointer is used)
        err = lambda: lib.hiprz_atlas_last_error(h)
        add = lambda n=12, base=0, instance=0, near=NEAR, far=FAR, ptr=p: lib.hiprz_atlas_add(h, ptr, n, base, instance, near, far, None)
        add_host = lambda n=12, base=0, instance=0, near=NEAR, far=FAR, ptr=p: lib.hiprz_atlas_add_host(h, ptr, n, base, instance, near, far)
        for call in (add, add_host):
            assert call() == _abi.ERR_STATE and b"no atlas has been begun" in err()
            assert call(n=0) == _abi.ERR_STATE, "no begin is refused before n == 0 is looked at"
        assert lib.hiprz_atlas_read_host(h, p, p) == _abi.ERR_STATE and lib.hiprz_atlas_dilate(h, p, 1, None, None) == _abi.ERR_STATE
        a.begin(8, 8)
        for call in (add, add_host):
            assert call() == _abi.ERR_STATE and b"before a scene" in err(), err()     # a context without a scene
            assert call(ptr=None) == _abi.ERR_INVALID and b"null pointer" in err()
        assert lib.hiprz_atlas_points_device(h) is None and lib.hiprz_atlas_dilate_host(h, p, 1, None) == _abi.ERR_STATE and b"nothing has been added" in err()
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
        for call in (add, add_host):
            assert call(instance=len(flat.instances)) == _abi.ERR_INVALID and b"no such instance" in err()
            assert call(instance=2**32 - 1) == _abi.ERR_INVALID
            assert call(n=1, base=2**32 - 2) == _abi.ERR_INVALID and b"0xFFFFFFFF or more" in err()
            assert call(n=2**32 - 1) == _abi.ERR_INVALID and call(n=2**64 - 1, base=7) == _abi.ERR_INVALID and call(n=0, base=2**32 - 1) == _abi.ERR_INVALID
            assert call(near=float("nan")) == _abi.ERR_INVALID and b"not finite" in err()
            assert call(far=float("inf")) == _abi.ERR_INVALID and call(near=-1.0) == _abi.ERR_INVALID and b"near_ < 0" in err()
            assert call(near=1.0, far=1.0) == _abi.ERR_INVALID and b"far_ <= near_" in err() and call(near=2.0, far=1.0) == _abi.ERR_INVALID
        assert lib.hiprz_atlas_points_device(h) is None and lib.hiprz_atlas_read_host(h, p, p) == _abi.ERR_STATE, "a refused add is no add"
        with pytest.raises(HiprzError) as e:
            ctx.atlas_points([(9, tris)], 8, 8)
        assert e.value.code == _abi.ERR_INVALID
        with pytest.raises(TypeError):
            ctx.atlas_points([(0, np.zeros(3, np.float32))], 8, 8)
        with pytest.raises(HiprzError):
            ctx.atlas_points([(0, tris)], 0, 8)
        # and after all that it builds; the calls that need an add take their own refusals
        points, samples = ctx.atlas_points([(MIRRORED, tris)], 8, 8, NEAR, FAR)
        _same(points, AR.build([(AR.placement_of(flat.instances[MIRRORED]), tris)], 8, 8, NEAR, FAR)[2], "after the refusals")
        rec = np.zeros((8, 8), texel_dtype)
        assert lib.hiprz_atlas_dilate(h, None, 1, None, None) == _abi.ERR_INVALID and lib.hiprz_atlas_dilate_host(h, None, 1, None) == _abi.ERR_INVALID
        assert lib.hiprz_atlas_dilate_host(h, rec.ctypes.data, 65, None) == _abi.ERR_INVALID and b"more than 64 rings" in err()
        assert lib.hiprz_atlas_read_host(h, None, None) == _abi.ERR_INVALID and lib.hiprz_atlas_read_records_host(h, None, None) == _abi.ERR_INVALID
        ring = np.zeros((8, 8), np.uint32)
        assert lib.hiprz_atlas_read_records_host(h, None, ring.ctypes.data) == _abi.ERR_STATE and b"nothing has been dilated" in err()
        assert lib.hiprz_atlas_dilate_host(h, rec.ctypes.data, 64, None) == _abi.OK
    finally:
        ctx.close()


# =====================================================================================================================
# 8. the C++ host
# =====================================================================================================================
def test_cpp_engine_bakes_an_atlas(built, tmp_path):
    exe = str(tmp_path / "atlas_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "atlas_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "world.json")
    scene_io.save_scene_json(_world(), scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    W, H, K, S, seed, rings = 65, 33, 64, 4, 20261020, 2
    parts = [(FLOOR, CHARTS["plane4"]), (SCALED, CHARTS["sphere16"])]
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        texels, samples, ring = ctx.bake_atlas(parts, W, H, (K, S), seed, rings, NEAR, FAR)
    finally:
        ctx.close()
        loaded.close()
    floor = samples["triangle"] < 2
    assert ((texels["occluded"][floor] > 0) & (texels["occluded"][floor] < K)).sum() * 10 >= floor.sum() and (ring == 1).any()
    names = []
    for k, (instance, tris) in enumerate(parts):
        names += [str(instance), str(tmp_path / f"part{k}.bin")]
        tris.tofile(names[-1])
    r = subprocess.run([exe, scene_path, str(tmp_path / "out.bin"), str(W), str(H), str(K), str(S), str(seed), str(rings)] + names, capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "ATLAS DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = open(tmp_path / "out.bin", "rb").read()
    assert out == texels.tobytes() + samples.tobytes() + ring.tobytes(), "Engine::bakeAtlas differs from Context.bake_atlas"
