"""Bounce baking on the GPU (include/hiprz_gather.h: libhiprz_gather.so, Context.gather / gather_samples / bake_bounce_atlas, Engine::gather).
The samples of a gather are held to the query library's own closest hits on the rays of Context.bake_rays (libhiprz_query.so and
libhiprz_bake.so, themselves held to the CPU oracle and to a numpy restatement by their tests), the texel under a hit to a float64
reconstruction of the hit, and a texel of the result to the numpy float32 restatement (tests/gather_reference.py) over the emitted
samples, bit for bit.  Trees 0 (reference) and 3 (device SAH).

THE WORLD (tests/gather_world.py): the floor, cube and sphere of tests/test_light_gpu.py plus one wall, seen by a 32 x 24 camera.  POINTS: the
first hits of its pixel rays, position = o + t * d in float32, the normal the hit's, near_ 1e-3, far_ 1e3.  THE ATLAS: 64 x 48, the mesh UVs
of floor, cube and wall scaled into a rectangle each; the sphere is in no part.

  1 rays, walk   K in 16, 64, 128, S in 1, 3, two seeds, two points spoiled: samples.t == Context.trace(Context.bake_rays(...)).t in every
                 byte, the ids are gather_reference.ids of those hits (instance, triangle and side decoded), bx and by are +0 without a hit.
  2 barycentrics the texel from the emitted bx, by == the texel from float64 barycentrics of the same ray on the same triangle, rays whose
                 float64 UV lies within 1e-3 texel of a texel boundary left out, at most 1 % of them.
  3 texels       mean and counts == gather_reference.texels over the emitted samples and a source that differs per texel, bit for bit.
                 The four mutants of the restatement are each caught: `back` by 1, `swap` and `rint` by 2 (and 3), `order` by 3.
  4 physics      a closed room whose source is 1.0 everywhere: exactly 1.0 and K rays read; an empty world: exactly sky and K rays
                 missed; a point centred under a radiant square: the closed-form form factor (test's docstring).
  5 sizes        n in 1, 3, 4, 5, 63, 64, 65, 257 with guard words behind texels and samples, n == 0, host-pointer == device-pointer calls,
                 the nine spoiled-point kinds at the first and last slot of a wave's group, 257 copies of one point.
  6 staleness    after update_instances moves the cube the gather equals a fresh context's and differs from before.
  7 compose      == gather_reference.compose in every byte, with and without indirect and emission.
  8 end to end   bake_bounce_atlas with 1 and 2 bounces == the same steps done one by one, ring map included; a red wall reddens the
                 floor before it; a zero albedo gathers +0.
  9 refusals, C++  in their order; Engine::gather and Engine::bakeBounceAtlas byte-equal to Context's.

MEASURED ON MI355X: 53 cases in 3.0 s beside the session's build fixture, slowest case 0.8 s (cases 1 - 3 on tree 0, which also makes the
points), then 0.7 s (the C++ host: it compiles a program).  Per tree, cases 1 - 3: 574 080 rays byte-equal in t and id to the query's hits,
2 884 of them back-face hits, 131 223 texels equal to the float64 reconstruction and 520 (0.39 %) on a boundary left out, every texel
bit-equal to the restatement, all four mutants caught; identical figures on trees 0 and 3.  Case 4: 35 of 64 and 567 of 1 024 rays reach
the square, the float64 estimator's counts exactly.  Case 8: 12 floor texels before the wall gather R 0.064 G 0.004 from the red wall,
R 0.057 G 0.055 from a grey one (the cube's faces in cells of their own: its sides no longer send on the top face's light).  C++: 690 points, one invalid, 2 282 rays read a texel, 8 006 missed.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bake_reference as BR
import gather_reference as GR
import gather_world as GW
from rayzath_amd import _abi, _hiprt, atlas, bake, gather, light, scene_io
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context
from rayzath_amd.gather import INVALID, record_dtype, sample_dtype, texel_dtype
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, HIT_INVALID, ray_dtype
from rayzath_amd.scene import Instance, Material, World, camera_struct, flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
SIZES = (1, 3, 4, 5, 63, 64, 65, 257)
KINDS = ("nan origin", "inf direction", "-inf origin", "nan far", "inf far", "zero direction", "far <= near", "near < 0", "length 2")
NEAR, FAR = 1e-3, 1e3
PAD, GUARD = 8, 0xABABABAB
F = np.float32
W, H = GW.W, GW.H
SKY = (0.25, 0.5, 2.0)


def _context(tree=0, world=None):
    """(context with the world uploaded, the world, its flat scene)"""
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    world = GW.world() if world is None else world
    flat = flatten(world)
    ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
    return ctx, world, flat


_ONCE = {}


def _points():
    """the first hits of the camera's pixel rays as surface points, computed once and never changed"""
    if "points" not in _ONCE:
        ctx, _, _ = _context(0)
        try:
            rays = ctx.pixel_rays().reshape(-1)
            hits = ctx.trace(rays)
        finally:
            ctx.close()
        found = (hits["flags"] & HIT_FOUND) != 0
        r, h = rays[found], hits[found]
        assert len(h) > 300 and set(np.unique(h["instance"])) == {0, 1, 2, 3}, "the camera sees all four instances"
        position = r["origin"] + h["t"][:, None] * r["direction"]
        assert position.dtype == F
        _ONCE["points"] = bake.points(position, h["normal"], NEAR, F(FAR))
        _ONCE["points"].setflags(write=False)
    return _ONCE["points"]


def _charts():
    """(base, uv) of the atlas, computed once"""
    if "charts" not in _ONCE:
        w = GW.world()
        _ONCE["charts"] = gather.chart_tables(GW.parts(w), len(w.instances))
        assert _ONCE["charts"][0].tolist() == [0, 2, gather.NONE, 14] and len(_ONCE["charts"][1]) == 16
    return _ONCE["charts"]


def _source(seed=1):
    """a W x H source whose values differ per texel; one texel in eleven has no value"""
    rng = np.random.default_rng(seed)
    source = np.zeros((H, W), record_dtype)
    source["rgb"] = rng.uniform(0.0, 4.0, (H, W, 3))
    source["word"] = rng.integers(0, 100, (H, W))
    source["word"][rng.random((H, W)) < 1.0 / 11.0] = INVALID
    return source


def _spoil(points, at, kind):
    from test_query_gpu import _spoil as spoil      # the nine kinds are that test's, applied to the point as a ray
    as_rays = points.view(ray_dtype)
    as_rays[at] = spoil(as_rays[at], kind)


def _guarded(entries, words_per_entry):
    return _hiprt.DeviceBuffer.of(np.full((entries + PAD) * words_per_entry, GUARD, np.uint32))


def _device_calls(ctx, points, n, source, seed, sky=SKY):
    """hiprz_gather_texels and hiprz_gather_samples on the first n of `points` through device pointers: (texels (n,), samples (n, K)); the
    guard words behind both are asserted"""
    g = ctx.gatherer()
    K = g.K
    ctx.sync()
    d_points = _hiprt.DeviceBuffer.of(points) if len(points) else _hiprt.DeviceBuffer(32)
    d_source, d_texels, d_samples = _hiprt.DeviceBuffer.of(source), _guarded(n, 4), _guarded(n * K, 4)
    try:
        g.texels_device(d_points.ptr, n, d_source.ptr, W, H, d_texels.ptr, seed, sky)
        g.samples_device(d_points.ptr, n, d_samples.ptr, seed)
        ctx.sync()
        texels, samples = d_texels.download(((n + PAD) * 4,), np.uint32), d_samples.download(((n * K + PAD) * 4,), np.uint32)
    finally:
        d_points.free(), d_source.free(), d_texels.free(), d_samples.free()
    assert (texels[n * 4:] == GUARD).all(), f"n = {n}, K = {K}: a texel behind n was written"
    assert (samples[n * K * 4:] == GUARD).all(), f"n = {n}, K = {K}: a sample behind n*K was written"
    return texels[:n * 4].view(texel_dtype), samples[:n * K * 4].view(sample_dtype).reshape(n, K)


# =====================================================================================================================
# 1. the rays and the walk are the bake's and the query's;  2. the barycentrics find the texel;  3. the texels are the restatement's
# =====================================================================================================================
@pytest.mark.parametrize("tree", TREES)
def test_samples_barycentrics_and_texels(built, tree):
    ctx, world, flat = _context(tree)
    try:
        points = _points().copy()
        _spoil(points, 5, "nan origin"), _spoil(points, len(points) - 1, "zero direction")
        base, uv = _charts()
        source = _source()
        triangles = GW.world_triangles(world, flat)
        rays_seen = back = left_out = kept = 0
        caught = {m: False for m in GR.MUTANTS}
        first = True
        for K in (16, 64, 128):
            for S in (1, 3):
                table = bake.cosine_directions(K, S)
                for seed in (0, 20261020):
                    texels = ctx.gather(points, source, W, H, (base, uv) if first else None, table, seed, SKY)
                    first = False
                    samples = ctx.gather_samples(points, seed)
                    rays = ctx.bake_rays(points, seed, table)
                    hits = ctx.trace(rays.reshape(-1)).reshape(rays.shape)
                    what = f"tree {tree} K {K} S {S} seed {seed}"
                    assert samples.shape == hits.shape == (len(points), K)
                    # 1: t in every byte, ids from the hits
                    assert samples["t"].tobytes() == hits["t"].tobytes(), f"{what}: t differs on {int((samples['t'].view(np.uint32) != hits['t'].view(np.uint32)).sum())} of {samples.size} rays"
                    want_ids = GR.ids(hits["flags"], hits["instance"], hits["triangle"], base, len(uv))
                    assert np.array_equal(samples["id"], want_ids), f"{what}: the ids differ on {int((samples['id'] != want_ids).sum())} rays"
                    found = (hits["flags"] & HIT_FOUND) != 0
                    assert np.array_equal(samples["id"] == gather.BACK, found & ((hits["flags"] & HIT_EXTERNAL) == 0))
                    assert np.array_equal(samples["id"] == gather.MISS, hits["flags"] == 0) and np.array_equal(samples["id"] == gather.INVALID_RAY, (hits["flags"] & HIT_INVALID) != 0)
                    assert np.array_equal(samples["id"] == gather.UNMAPPED, found & ((hits["flags"] & HIT_EXTERNAL) != 0) & (hits["instance"] == GW.SPHERE))
                    mapped = samples["id"] < gather.MAX_CHARTS
                    inst = np.searchsorted(np.array([0, 2, 14]), samples["id"][mapped], side="right") - 1        # decode: floor, cube, wall
                    inst = np.array([GW.FLOOR, GW.CUBE, GW.WALL])[inst]
                    assert np.array_equal(inst, hits["instance"][mapped]) and np.array_equal(samples["id"][mapped] - base[inst], hits["triangle"][mapped])
                    assert (samples["bx"][~found].view(np.uint32) == 0).all() and (samples["by"][~found].view(np.uint32) == 0).all()
                    assert (samples["id"][[5, -1]] == gather.INVALID_RAY).all() and samples["t"][5].tobytes() == F(FAR).tobytes() * K
                    caught["back"] |= not np.array_equal(samples["id"], GR.ids(hits["flags"], hits["instance"], hits["triangle"], base, len(uv), "back"))
                    # 2: the texel from bx, by against float64 barycentrics of the same ray on the same triangle
                    tri = np.stack([triangles[i][t] for i, t in zip(inst, hits["triangle"][mapped])])
                    _, bx, by, _ = GW.barycentrics(tri, rays["origin"][mapped].astype(np.float64), rays["direction"][mapped].astype(np.float64))
                    c = uv[samples["id"][mapped]]
                    b1 = (1.0 - bx) - by
                    u64 = c["u1"] * b1 + c["u2"] * bx + c["u3"] * by
                    v64 = c["v1"] * b1 + c["v2"] * bx + c["v3"] * by
                    edge = GW.on_a_boundary(u64, v64, 1e-3)
                    assert edge.mean() <= 0.01, f"{what}: {edge.mean():.2%} of the rays lie on a texel boundary"
                    x64, y64, _ = GR.texel_of(u64, v64, W, H)
                    u32, v32, _ = GR.uv(samples[mapped], uv)
                    x32, y32, _ = GR.texel_of(u32, v32, W, H)
                    wrong = ((x32 != x64) | (y32 != y64)) & ~edge
                    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {int((~edge).sum())} texels differ from the float64 reconstruction"
                    for mutant in ("swap", "rint"):
                        mu, mv, _ = GR.uv(samples[mapped], uv, F, mutant)
                        mx, my, _ = GR.texel_of(mu, mv, W, H, mutant)
                        caught[mutant] |= bool((((mx != x64) | (my != y64)) & ~edge).any())
                    # 3: the texels
                    want = GR.texels(points, samples, uv, source, W, H, SKY)
                    assert np.array_equal(texels["counts"], want["counts"]), f"{what}: the counts differ on {int((texels['counts'] != want['counts']).sum())} points"
                    assert texels.tobytes() == want.tobytes(), f"{what}: the mean differs on {int((texels['mean'].view(np.uint32) != want['mean'].view(np.uint32)).any(-1).sum())} points"
                    caught["order"] |= GR.texels(points, samples, uv, source, W, H, SKY, "order").tobytes() != texels.tobytes()
                    rays_seen += samples.size
                    back += int((samples["id"] == gather.BACK).sum())
                    left_out += int(edge.sum())
                    kept += int((~edge).sum())
        assert texels["counts"][5] == INVALID and texels["counts"][-1] == INVALID and (texels["mean"][[5, -1]].view(np.uint32) == 0).all()
        print(f"tree {tree}: {rays_seen} rays byte-equal in t and id to the query's hits, {back} back-face hits, {kept} texels equal to the float64 reconstruction, "
              f"{left_out} on a boundary left out; mutants caught: {caught}")
        assert back > 0 and all(caught.values()), caught
    finally:
        ctx.close()


# =====================================================================================================================
# 4. exact physics
# =====================================================================================================================
def test_a_closed_room_and_an_empty_world(built):
    rng = np.random.default_rng(4)
    points = bake.points(rng.uniform(-0.4, 0.4, size=(131, 3)), rng.normal(size=(131, 3)), NEAR, FAR)
    _spoil(points, 64, "nan far")
    ok = np.arange(131) != 64
    room = World()
    grey = room.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    box = room.add(GW.inward_box())
    room.add(Instance(box, [grey], position=(0.1, -0.2, 0.05), rotation=(0.2, 0.4, 0.1), scale=(3.0, 2.0, 2.5), name="room"))
    room.camera = GW.world().camera
    charts = gather.chart_tables([(0, atlas.charts(box))], 1)
    ones = gather.records((1.0, 1.0, 1.0), (5, 7))
    for tree in TREES:
        ctx, _, _ = _context(tree, room)
        try:
            for K in (16, 64, 256):
                texels = ctx.gather(points, ones, 7, 5, charts, (K, 3), 9, SKY)
                assert (texels["counts"][ok] == K).all(), f"tree {tree} K {K}: not every ray of a closed room reads a texel: {np.unique(texels['counts'][ok])}"
                assert (texels["mean"][ok] == 1.0).all() and texels["counts"][64] == INVALID and not texels["mean"][64].view(np.uint32).any()
        finally:
            ctx.close()
    ctx, _, flat = _context(0, GW.world(geometry=False))
    try:
        assert not len(flat.instances)
        nothing = gather.chart_tables([], 0)
        for K in (16, 64, 256):
            texels = ctx.gather(points, ones, 7, 5, nothing, (K, 3), 9, SKY)
            assert (texels["counts"][ok] == K << 16).all() and texels["mean"][ok].tobytes() == np.asarray(SKY, F).tobytes() * 130, f"K {K}: an empty world is not the sky"
            assert texels["counts"][64] == INVALID
            samples = ctx.gather_samples(points, 9)
            assert (samples["id"][ok] == gather.MISS).all() and (samples["id"][64] == gather.INVALID_RAY).all() and (samples["t"][ok] == F(FAR)).all()
    finally:
        ctx.close()


def _form_factor(a, h):
    """of a differential element to a parallel square of side 2a centred h above it: four corner rectangles (Howell, A Catalog of Radiation
    Heat Transfer Configuration Factors, B-4)"""
    x = a / h
    r = np.sqrt(1.0 + x * x)
    return 4.0 * (2.0 * (x / r) * np.arctan(x / r)) / (2.0 * np.pi)


def test_the_form_factor_of_a_radiant_square(built):
    """A point at the origin, normal +y, under a square of side 2 at height 1 whose source is 1.0: with cosine-weighted directions the mean
    is the form factor, 0.554126 in closed form.  The K-sample estimator with the library's table (set 0) evaluated in float64 on the CPU
    misses it by 7.25e-3 at K = 64 (35 of 64 rays) and by 4.15e-4 at K = 1024 (567 of 1024); no ray of either table passes within 1e-4 of
    the square's edge.  The device is allowed that error plus (rays within 1e-4 of the edge) / K, and the error must fall from 64 to 1024."""
    a, h = 1.0, 1.0
    exact = _form_factor(a, h)
    assert abs(exact - 0.5541264239795719) < 1e-12
    world = World()
    grey = world.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    square = world.add(GW.square_below(a, h))
    world.add(Instance(square, [grey], name="square"))
    world.camera = GW.world().camera
    charts = gather.chart_tables([(0, atlas.charts(square))], 1)
    ones = gather.records((1.0, 1.0, 1.0), (4, 4))
    point = bake.points([[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]], NEAR, FAR)
    ctx, _, _ = _context(3, world)
    try:
        errors = {}
        for K in (64, 1024):
            l = bake.cosine_directions(K, 1)[0].astype(np.float64)
            x, z = h * l[:, 0] / l[:, 2], -h * l[:, 1] / l[:, 2]          # d = (l.x, l.z, -l.y) under the frame of (0, 1, 0)
            inside = (np.abs(x) <= a) & (np.abs(z) <= a)
            edge = ((np.abs(np.abs(x) - a) < 1e-4) & (np.abs(z) <= a + 1e-4)) | ((np.abs(np.abs(z) - a) < 1e-4) & (np.abs(x) <= a + 1e-4))
            estimator = abs(inside.mean() - exact)
            texel = ctx.gather(point, ones, 4, 4, charts, (K, 1), 0, (0.0, 0.0, 0.0))[0]
            errors[K] = abs(float(texel["mean"][0]) - exact)
            print(f"K {K}: device {texel['mean'][0]!r} ({texel['counts'] & 0xFFFF} rays read), float64 estimator {inside.mean()!r}, exact {exact!r}, {int(edge.sum())} rays at the edge")
            assert texel["counts"] >> 16 == K - (texel["counts"] & 0xFFFF), "what does not hit the square misses"
            assert texel["mean"][0] == texel["mean"][1] == texel["mean"][2] == F(texel["counts"] & 0xFFFF) / F(K)
            assert errors[K] <= estimator + edge.sum() / K, f"K {K}: the device misses the form factor by {errors[K]:.3e}, the float64 estimator by {estimator:.3e}"
        assert errors[1024] < errors[64]
    finally:
        ctx.close()


# =====================================================================================================================
# 5. sizes, spoiled points, copies — on one context per tree
# =====================================================================================================================
@pytest.fixture(scope="module", params=TREES)
def lit(built, request):
    ctx, world, flat = _context(request.param)
    ctx.gatherer().set_charts(*_charts())
    yield ctx, _points()[:257].copy(), _source(2)
    ctx.close()


@pytest.mark.parametrize("K", (16, 64, 128))
def test_sizes_at_the_edges_of_a_wave(lit, K):
    ctx, points, source = lit
    seed = 11
    want = ctx.gather(points, source, W, H, None, (K, 3), seed, SKY)
    want_samples = ctx.gather_samples(points, seed)
    assert want.tobytes() == GR.texels(points, want_samples, _charts()[1], source, W, H, SKY).tobytes()
    assert (want["counts"] & 0xFFFF).any() and (want["counts"] >> 16).any() and want["mean"].any()
    for n in SIZES:
        texels, samples = _device_calls(ctx, points, n, source, seed)
        assert texels.tobytes() == want[:n].tobytes(), f"K {K} n {n}: the texels differ from the first n of a larger gather"
        assert samples.tobytes() == want_samples[:n].tobytes(), f"K {K} n {n}"
        assert ctx.gather(points[:n], source, W, H, None, None, seed, SKY).tobytes() == want[:n].tobytes(), f"host-pointer call, K {K} n {n}"
    texels, samples = _device_calls(ctx, points, 0, source, seed)          # n == 0: the guards (asserted inside) are all there is
    assert len(texels) == 0 and samples.size == 0
    assert ctx.gather(points[:0], source, W, H, None, None, seed).shape == (0,) and ctx.gather_samples(points[:0], seed).shape == (0, K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n,spoiled", [(16, 130, (0, 3, 4, 63, 129)), (128, 5, (0, 4))], ids=["K16", "K128"])
def test_invalid_points(lit, K, n, spoiled, kind):
    ctx, points, source = lit
    clean = points[:n].copy()
    want = ctx.gather(clean, source, W, H, None, (K, 3), 5, SKY)
    batch = clean.copy()
    for at in spoiled:
        _spoil(batch, at, kind)
    got, got_samples = _device_calls(ctx, batch, n, source, 5)
    assert got.tobytes() == ctx.gather(batch, source, W, H, None, None, 5, SKY).tobytes()
    mask = np.zeros(n, bool)
    mask[list(spoiled)] = True
    assert got[~mask].tobytes() == want[~mask].tobytes(), "a valid point reads otherwise beside invalid ones"
    assert np.array_equal(BR.valid(batch), ~mask | (kind == "length 2"))
    if kind == "length 2":          # a valid point: the normal is normalised first, and a power of two scales exactly
        assert got.tobytes() == want.tobytes()
        return
    assert (got["counts"][mask] == INVALID).all(), got["counts"][mask]
    assert (got["mean"][mask].view(np.uint32) == 0).all(), "the mean of an invalid point is not +0"
    assert got.tobytes() == GR.texels(batch, got_samples, _charts()[1], source, W, H, SKY).tobytes()
    assert (got_samples["id"][mask] == gather.INVALID_RAY).all() and (got_samples["bx"][mask].view(np.uint32) == 0).all()


def test_one_point_many_times(lit):
    ctx, points, source = lit
    texels = ctx.gather(points, source, W, H, None, (64, 1), 3, SKY)
    reads = texels["counts"] & 0xFFFF
    at = int(np.argmax((reads > 8) & (reads < 56)))
    assert 8 < reads[at] < 56
    batch = np.repeat(points[at:at + 1], 257)
    for K in (16, 64):
        one = ctx.gather(batch[:1], source, W, H, None, (K, 1), 3, SKY)          # one set: the texel of a point does not depend on its index
        got = _device_calls(ctx, batch, 257, source, 3)[0]
        assert got.tobytes() == one.tobytes() * 257, f"K {K}: copies of one point under one set differ"
    assert one.tobytes() == texels[at:at + 1].tobytes()


# =====================================================================================================================
# 6. staleness: the scene is read from the view of the call
# =====================================================================================================================
def test_a_gather_sees_update_instances(built):
    points, source, seed = _points()[::3].copy(), _source(3), 13
    ctx, world, flat = _context(3)
    moved_world = GW.world(moved=True)
    moved = flatten(moved_world)
    try:
        before = ctx.gather(points, source, W, H, _charts(), (16, 3), seed, SKY)
        assert moved.instances[GW.CUBE].tobytes() != flat.instances[GW.CUBE].tobytes() and moved.instances[GW.WALL].tobytes() == flat.instances[GW.WALL].tobytes()
        ctx.update_instances(moved.instances)
        after = ctx.gather(points, source, W, H, None, None, seed, SKY)
        samples = ctx.gather_samples(points, seed)
        assert after.tobytes() != before.tobytes(), "the gather does not see the moved cube"
        assert after.tobytes() == GR.texels(points, samples, _charts()[1], source, W, H, SKY).tobytes()
    finally:
        ctx.close()
    fresh, _, _ = _context(3, moved_world)
    try:
        assert fresh.gather(points, source, W, H, _charts(), (16, 3), seed, SKY).tobytes() == after.tobytes(), "a gather after update_instances differs from a fresh context's"
    finally:
        fresh.close()


# =====================================================================================================================
# 7. compose
# =====================================================================================================================
def test_compose_is_the_restatement(built):
    rng = np.random.default_rng(7)
    shape = (33, 17)
    direct, indirect, albedo, emission = (np.zeros(shape, record_dtype) for _ in range(4))
    for a in (direct, indirect, albedo, emission):
        a["rgb"], a["word"] = rng.uniform(0.0, 3.0, shape + (3,)), rng.integers(0, 2**32, shape)
    direct["word"][::5, ::3] = INVALID
    direct["rgb"][1, 1], albedo["rgb"][2, 2] = (-0.0, 0.0, 1.0e30), 0.0
    ctx, _, _ = _context(0)
    try:
        g = ctx.gatherer()
        for ind, emi in ((indirect, emission), (None, emission), (indirect, None), (None, None)):
            got = g.compose(direct, ind, albedo, emi, ctx.sync)
            assert got.tobytes() == GR.compose(direct, ind, albedo, emi).tobytes(), f"indirect {ind is not None}, emission {emi is not None}"
        assert got["word"].tobytes() == direct["word"].tobytes()
        n = direct.size
        ctx.sync()
        bufs = [_hiprt.DeviceBuffer.of(a) for a in (direct, indirect, albedo)] + [_guarded(n, 4)]
        try:
            g.compose_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, bufs[3].ptr, n - 3)       # the last three texels and the guards stay
            g.compose_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, bufs[3].ptr, 0)
            ctx.sync()
            out = bufs[3].download(((n + PAD) * 4,), np.uint32)
        finally:
            for b in bufs:
                b.free()
        assert (out[(n - 3) * 4:] == GUARD).all() and out[:(n - 3) * 4].tobytes() == GR.compose(direct, indirect, albedo, None).reshape(-1)[:n - 3].tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 8. end to end
# =====================================================================================================================
def _albedo(red_wall):
    """per texel of the atlas: 0.8 grey, the wall's rectangle red"""
    albedo = gather.records((0.8, 0.8, 0.8), (H, W))
    if red_wall:
        u0, v0, u1, v1 = GW.RECTS[GW.WALL]
        albedo["rgb"][int(v0 * H) - 1:int(v1 * H) + 2, int(u0 * W) - 1:int(u1 * W) + 2] = (0.9, 0.05, 0.05)
    return albedo


def test_a_bounce_atlas_is_its_steps(built):
    seed, rings, directions, samples = 4, 2, (64, 3), (16, 3)
    ctx, world, flat = _context(3)
    try:
        parts = GW.parts(world)
        albedo = _albedo(True)
        emission = gather.records((0.0, 0.0, 0.0), (H, W))
        emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)          # a patch of the floor glows green
        sky = (0.01, 0.02, 0.03)
        results = {}
        for bounces in (1, 2):
            results[bounces] = ctx.bake_bounce_atlas(parts, W, H, albedo, emission, bounces, directions, samples, seed, rings, sky, NEAR, FAR)
        # the same, one step at a time through the host
        points, atlas_samples = ctx.atlas_points(parts, W, H, NEAR, FAR)
        a = ctx.atlas()
        direct = ctx.bake_light(points, samples, seed)
        indirect = None
        for bounces in (1, 2):
            source = a.dilate(ctx.gatherer().compose(direct, indirect, albedo, emission, ctx.sync), rings)[0].reshape(H, W)
            indirect = ctx.gather(points, source, W, H, gather.chart_tables(parts, len(flat.instances)), directions, seed, sky)
            want_direct, want_ring = a.dilate(direct, rings)
            want_indirect, _ = a.dilate(indirect, rings)
            got_direct, got_indirect, got_ring = results[bounces]
            assert got_direct.shape == got_indirect.shape == got_ring.shape == (H, W) and got_indirect.dtype == texel_dtype and got_direct.dtype == light.texel_dtype
            assert got_ring.tobytes() == want_ring.tobytes() and got_direct.tobytes() == want_direct.reshape(H, W).tobytes(), f"{bounces} bounces: direct or ring"
            assert got_indirect.tobytes() == want_indirect.reshape(H, W).tobytes(), f"{bounces} bounces: bake_bounce_atlas differs from its steps done one by one"
        assert results[1][1].tobytes() != results[2][1].tobytes() and results[1][0].tobytes() == results[2][0].tobytes(), "a second bounce adds light, to the indirect only"
        # the physics: floor texels before the red wall gather more red than green (no emission here: the green patch is out)
        _, red, ring = ctx.bake_bounce_atlas(parts, W, H, albedo, None, 1, directions, samples, seed, rings, (0.0, 0.0, 0.0), NEAR, FAR)
        _, grey, _ = ctx.bake_bounce_atlas(parts, W, H, _albedo(False), None, 1, directions, samples, seed, rings, (0.0, 0.0, 0.0), NEAR, FAR)
        p = points["position"]
        before_wall = (atlas_samples["triangle"] < 2) & (np.abs(p[..., 0] + 1.0) < 0.8) & (p[..., 2] > 0.3) & (p[..., 2] < 0.9)
        assert before_wall.sum() >= 4, int(before_wall.sum())
        r, g_ = red["mean"][before_wall][:, 0].mean(), red["mean"][before_wall][:, 1].mean()
        print(f"{int(before_wall.sum())} floor texels before the wall gather R {r:.4f} G {g_:.4f} from a red wall, R {grey['mean'][before_wall][:, 0].mean():.4f} "
              f"G {grey['mean'][before_wall][:, 1].mean():.4f} from a grey one")
        gr, gg = grey["mean"][before_wall][:, 0].mean(), grey["mean"][before_wall][:, 1].mean()
        assert r > g_ > 0.0, "a red wall does not redden the floor before it"
        assert r / g_ > gr / gg and g_ < gg, "... more than a grey wall does under the same lights: the wall's green is what went missing"
        # a zero albedo everywhere: nothing is sent on
        _, dark, _ = ctx.bake_bounce_atlas(parts, W, H, (0.0, 0.0, 0.0), None, 2, directions, samples, seed, rings, (0.0, 0.0, 0.0), NEAR, FAR)
        assert not dark["mean"].view(np.uint32).any() and (dark["counts"][ring == 0] != INVALID).all()
        with pytest.raises(ValueError):
            ctx.bake_bounce_atlas(parts, W, H, albedo, None, 0)
    finally:
        ctx.close()


# =====================================================================================================================
# 9. refusals, in their order
# =====================================================================================================================
def test_refusals(built):
    ctx = Context(0)
    try:
        points = bake.points([[0, 3, 0]], [[0, 1, 0]], NEAR, 10.0)          # above the cube, looking up
        source = gather.records((1.0, 1.0, 1.0), (H, W))
        g = ctx.gatherer()
        lib, hd, p = g.lib, g._gather, points.ctypes.data           # (every call below is refused before a pointer is used)
        err = lambda: lib.hiprz_gather_last_error(hd)
        texels = lambda n=1, pts=p, src=p, w=W, h=H, sky=p, out=p: lib.hiprz_gather_texels(hd, pts, n, 0, src, w, h, sky, out, None)
        host = lambda n=1, pts=p, src=p, w=W, h=H, sky=p, out=p: lib.hiprz_gather_texels_host(hd, pts, n, 0, src, w, h, sky, out)
        smp = lambda n=1, pts=p, out=p: lib.hiprz_gather_samples(hd, pts, n, 0, out, None)
        # 1. a null pointer, before the missing table
        for call in (texels, host):
            for kw in (dict(pts=None), dict(src=None), dict(sky=None), dict(out=None)):
                assert call(**kw) == _abi.ERR_INVALID and b"null pointer" in err(), kw
        assert smp(pts=None) == _abi.ERR_INVALID and smp(out=None) == _abi.ERR_INVALID and b"gather_samples: null pointer" in err()
        # 2. no table, then no chart map, before the size and before n == 0
        assert texels() == _abi.ERR_STATE and b"gather_texels: no direction table" in err()
        assert smp(n=2**40) == _abi.ERR_STATE and host(n=0) == _abi.ERR_STATE
        with pytest.raises(HiprzError) as e:
            ctx.gather(points, source, W, H, None, None)
        assert e.value.code == _abi.ERR_STATE
        table = bake.cosine_directions(16, 2)
        bad = table.copy()
        bad[1, 15, :3] = (0.8, 0.7, 0.0)
        with pytest.raises(HiprzError) as e:
            g.set_directions(bad)
        assert e.value.code == _abi.ERR_INVALID and "not of unit length" in str(e.value)
        assert lib.hiprz_gather_set_directions(hd, table.ctypes.data, 48, 1) == _abi.ERR_INVALID and b"K is not one of" in err()
        assert lib.hiprz_gather_set_directions(hd, None, 16, 2) == _abi.ERR_INVALID and texels() == _abi.ERR_STATE and b"no direction table" in err()
        g.set_directions(table)
        assert texels() == _abi.ERR_STATE and b"no chart map" in err() and smp(n=0) == _abi.ERR_STATE and host(n=2**40) == _abi.ERR_STATE
        base, uv = _charts()
        nan = uv.copy()
        nan["v3"][-1] = np.nan
        with pytest.raises(HiprzError) as e:
            g.set_charts(base, nan)
        assert e.value.code == _abi.ERR_INVALID and "not finite" in str(e.value) and texels() == _abi.ERR_STATE
        assert lib.hiprz_gather_set_charts(hd, None, 4, uv.ctypes.data, len(uv)) == _abi.ERR_INVALID and lib.hiprz_gather_set_charts(hd, base.ctypes.data, 4, None, 1) == _abi.ERR_INVALID
        g.set_charts(base, uv)
        # 3. n*K >= 2^31, then W and H, before 4. the view: a table and a map, no scene yet
        assert texels(n=2**27) == _abi.ERR_INVALID and b"2^31" in err() and smp(n=2**64 - 1) == _abi.ERR_INVALID and host(n=2**60 + 1) == _abi.ERR_INVALID
        assert texels(w=0) == _abi.ERR_INVALID and b"W or H" in err() and host(h=16385) == _abi.ERR_INVALID and texels(n=0, w=0) == _abi.ERR_INVALID
        assert texels(n=2**27, w=0) == _abi.ERR_INVALID and b"2^31" in err()
        with pytest.raises(HiprzError) as e:
            ctx.gather(points, source, W, H, None, None)
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value), e.value
        with pytest.raises(HiprzError) as e:
            ctx.gather_samples(points)
        assert e.value.code == _abi.ERR_STATE
        assert ctx.gather(points[:0], source, W, H, None, None).shape == (0,) and texels(n=0) == _abi.OK and smp(n=0) == _abi.OK          # n == 0: no view, no launch
        # compose needs neither table, map nor scene; its refusals
        comp = lambda d=p, i=p, a=p, e=p, o=p, n=1: lib.hiprz_gather_compose(hd, d, i, a, e, o, n, None)
        assert comp(d=None) == _abi.ERR_INVALID and comp(a=None) == _abi.ERR_INVALID and comp(o=None) == _abi.ERR_INVALID and b"gather_compose: null pointer" in err()
        assert comp(n=2**31) == _abi.ERR_INVALID and b"2^31 texels" in err() and comp(n=0, i=None, e=None) == _abi.OK
        # 5. the chart map is for another number of instances than the scene
        world = GW.world()
        flat = flatten(world)
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
        g.set_charts(base[:3], uv)
        with pytest.raises(HiprzError) as e:
            ctx.gather(points, source, W, H, None, None)
        assert e.value.code == _abi.ERR_INVALID and "another number of instances" in str(e.value)
        assert smp() == _abi.ERR_INVALID and host() == _abi.ERR_INVALID and texels(n=0) == _abi.OK
        with pytest.raises(TypeError):
            ctx.gather(np.zeros(3, np.float32), source, W, H, None, None)
        with pytest.raises(TypeError):
            ctx.gather(points, source[:3], W, H, None, None)
        # and after all that it gathers: the table set before the scene
        first = ctx.gather(points, source, W, H, (base, uv), None, 1, SKY)
        assert first.tobytes() == ctx.gather(points, source, W, H, None, (16, 2), 1, SKY).tobytes() and (first["counts"][0] >> 16) + (first["counts"][0] & 0xFFFF) <= 16
        assert first["counts"][0] >> 16 > 0, "a point above the scene looking up misses"
    finally:
        ctx.close()


# =====================================================================================================================
# 9 (continued). the C++ host
# =====================================================================================================================
def test_cpp_engine_gathers(built, tmp_path):
    exe = str(tmp_path / "gather_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "gather_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "bounce.json")
    world = GW.world()
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, seed, bounces = 16, 4, 20261020, 2
    parts = GW.parts(world)
    source, albedo = _source(9), _albedo(True)
    emission = gather.records((0.0, 0.0, 0.0), (H, W))
    emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        assert len(loaded.flat.instances) == 4
        rays = ctx.pixel_rays().reshape(-1)
        hits = ctx.trace(rays)
        found = (hits["flags"] & HIT_FOUND) != 0
        points = bake.points(rays["origin"][found] + hits["t"][found][:, None] * rays["direction"][found], hits["normal"][found], NEAR, F(FAR))
        _spoil(points, 5, "far <= near")            # an invalid point travels through the C++ host as well
        want = ctx.gather(points, source, W, H, gather.chart_tables(parts, 4), (K, S), seed, SKY)
        want_direct, want_indirect, want_ring = ctx.bake_bounce_atlas(parts, W, H, albedo, emission, bounces, (K, S), (16, 4), seed, 2, SKY, NEAR, FAR)
    finally:
        ctx.close()
        loaded.close()
    assert want["counts"][5] == INVALID and want["mean"].any() and (want["counts"][want["counts"] != INVALID] & 0xFFFF).any()
    files = {name: str(tmp_path / (name + ".bin")) for name in ("points", "source", "albedo", "emission", "out")}
    for name, array in (("points", points), ("source", source), ("albedo", albedo), ("emission", emission)):
        array.tofile(files[name])
    part_args = []
    for instance, tris in parts:
        path = str(tmp_path / f"charts{instance}.bin")
        tris.tofile(path)
        part_args += [str(instance), path]
    r = subprocess.run([exe, scene_path, files["points"], files["source"], str(W), str(H), files["out"], str(K), str(S), str(seed), files["albedo"], files["emission"],
                        str(bounces)] + part_args, capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "GATHER DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(files["out"], "rb").read() == want.tobytes(), "Engine::gather differs from Context.gather"
    assert (want_ring == 0).sum() > 100 and want_indirect["mean"].any() and want_direct["light"].any()
    assert open(files["out"] + ".ring", "rb").read() == want_ring.tobytes()
    assert open(files["out"] + ".direct", "rb").read() == want_direct.tobytes(), "Engine::bakeBounceAtlas: the direct light differs from Context.bake_bounce_atlas"
    assert open(files["out"] + ".indirect", "rb").read() == want_indirect.tobytes(), "Engine::bakeBounceAtlas: the indirect light differs from Context.bake_bounce_atlas"
