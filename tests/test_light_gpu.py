"""Light baking on the GPU (include/hiprz_light.h: libhiprz_light.so, Context.bake_light / light_rays / bake_light_atlas, Engine::bakeLight).
The rays and weights of a bake are held to the numpy float32 restatement (tests/light_reference.py) in every byte; a texel is held to the
restatement's fixed-order sum over the query library's own verdicts on those rays (libhiprz_query.so, itself held to the CPU oracle by
tests/test_query_gpu.py), bit for bit.  Trees 0 (reference) and 3 (device SAH).

THE WORLD: a floor of two triangles, a cube above it and a small sphere beside it (12 + 48 triangles), seen by a 32 x 24 camera.  POINTS: the
first hits of its pixel rays (Context.trace(ctx.pixel_rays())), position = o + t * d in float32, the normal the hit's, near_ 1e-3, far_ 1e3.
LIGHT SETS: none, one spot, two spots, one direct, two directs, mixed (two spots, two directs), `edges`: the lights without light of
tests/test_light_reference.py beside one of each kind that shines, and the two at their upper clamps, and `at a point`: a spot light whose
position is that of one of the baked points, beside a spot and a direct light.

  1 rays       hiprz_light_rays == light_reference.rays in every byte, weights included: K in 1, 16, 64, 128, S in 1, 3, two seeds, every
               light set, two points spoiled.
  2 texels     shadowed and light == light_reference.texels over hiprz_query_occluded's words on the emitted rays, bit for bit; the four
               mutants of the restatement are each caught by case 1 or case 2.
  3 sizes      n in 1, 3, 4, 5, 63, 64, 65, 257 at K in 1, 16, 64, 128 through device pointers with guard words behind texels, rays and
               weights; n == 0 writes nothing; host-pointer calls equal them.
  4 invalid    the nine kinds of test_query_gpu._spoil at the first and last slot of a wave's group.
  5 empty      an empty world (the unshadowed sum, shadowed 0), no lights, an empty range.
  6 ranges     a one-light range equals the restatement for that light alone; the ranges of all lights one by one add up to the whole.
  7 copies     257 copies of one point under one set give 257 equal texels.
  8 staleness  after update_shading moves and recolours a light, the bake equals a fresh context's, byte for byte, and differs from before;
               after it changes the NUMBER of lights, count, rays and texels follow.
  9 refusals   in their order: null, no table, n*K, no scene, a bad range, n*L*K.
 10 atlas      bake_light_atlas at 33 x 17 equals atlas points -> bake_light -> dilation done separately, ring map included.
 11 C++        Engine::bakeLight and Engine::bakeLightAtlas through tests/light_delivery_check.cpp, byte-equal to Context.bake_light and
               Context.bake_light_atlas.

MEASURED ON MI355X: 87 cases in 37 s beside the session's build fixture, slowest case 0.6 s (the C++ host: it compiles a program), then
0.4 s (cases 1 and 2 on `edges`).  Per tree, cases 1 and 2: 214 852 rays and weights byte-equal to the restatement per light (4 726 744 in
all; `edges` 1 933 668, `at a point` 644 556), 32 040 (one direct) to 228 229 (at a point) rays shadowed, 435 to 2 780 texels in a
penumbra, every texel bit-equal; identical figures on trees 0 and 3.  Mutants: `mixed`,
`two spots`, `edges` and `at a point` catch all four; one light cannot catch `order`, direct lights alone cannot catch `angle` and `far`.  Case 11: 648
points, one invalid, 647 lit, 4 332 rays shadowed.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import light_reference as LR
from rayzath_amd import _abi, _hiprt, atlas, bake, light, scene_io
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context
from rayzath_amd.light import INVALID, texel_dtype
from rayzath_amd.query import HIT_FOUND, ray_dtype
from rayzath_amd.scene import (Camera, DirectLight, Instance, Material, SpotLight, World, camera_struct, flatten, generate_cube, generate_plane,
                               generate_sphere)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
KS = (1, 16, 64, 128)
SIZES = (1, 3, 4, 5, 63, 64, 65, 257)
KINDS = ("nan origin", "inf direction", "-inf origin", "nan far", "inf far", "zero direction", "far <= near", "near < 0", "length 2")
NEAR, FAR = 1e-3, 1e3
PAD, GUARD = 8, 0xABABABAB
F = np.float32

SPOT_A = dict(position=(1.5, 4.0, -1.0), direction=(-0.3, -1.0, 0.25), color=(255, 210, 120, 255), size=0.35, emission=60.0, beam_angle=0.8)
SPOT_B = dict(position=(-2.5, 1.5, 1.5), direction=(1.0, -0.4, -0.6), color=(40, 120, 255, 255), size=0.05, emission=25.0, beam_angle=2.2)
DIRECT_A = dict(direction=(0.3, -1.0, 0.2), color=(255, 255, 240, 255), emission=4.0, angular_size=0.15)
DIRECT_B = dict(direction=(-1.0, -0.35, -0.5), color=(255, 90, 60, 200), emission=1.5, angular_size=1.1)
LIGHT_SETS = {
    "none": ((), ()),
    "one spot": ((SPOT_A,), ()),
    "two spots": ((SPOT_A, SPOT_B), ()),
    "one direct": ((), (DIRECT_A,)),
    "two directs": ((), (DIRECT_A, DIRECT_B)),
    "mixed": ((SPOT_A, SPOT_B), (DIRECT_A, DIRECT_B)),
    # lights of size / angle / emission 0 or at their upper clamp, as tests/generated_scenes.py draws them, beside one of each kind that shines
    "edges": ((dict(SPOT_A, size=0.0), dict(SPOT_A, beam_angle=0.0), SPOT_B, dict(SPOT_A, beam_angle=3.14159), dict(SPOT_A, emission=0.0)),
              (dict(DIRECT_A, angular_size=0.0), DIRECT_A, dict(DIRECT_B, angular_size=np.pi), dict(DIRECT_A, emission=0.0))),
    # a spot light at the position of one of the baked points (put in by _world: the points come from the device) beside two that cast shadows
    "at a point": ((SPOT_A,), (DIRECT_A,)),
}
AT_A_POINT = dict(direction=(0.2, -1.0, 0.1), color=(120, 255, 160, 255), size=0.2, emission=30.0, beam_angle=3.14159)


def _world(lights="mixed", geometry=True):
    world = World()
    if geometry:
        grey = world.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
        world.add(Instance(world.add(generate_plane(4, 1.0, 1.0)), [grey], position=(0, 0, 0), scale=(5, 1, 5), name="floor"))
        world.add(Instance(world.add(generate_cube()), [grey], position=(0.2, 1.2, 0.0), rotation=(0.3, 0.5, 0.1), scale=(1.2, 0.6, 1.2), name="cube"))
        world.add(Instance(world.add(generate_sphere(8)), [grey], position=(-1.6, 0.5, -0.8), scale=(0.5, 0.5, 0.5), name="sphere"))
    spots, directs = LIGHT_SETS[lights]
    if lights == "at a point":      # a light AT a baked point: its position is that point's float32 position, bit for bit
        spots = (dict(AT_A_POINT, position=tuple(_points()[_on_the_cube()]["position"])),) + spots
    for kw in spots:
        world.add(SpotLight(**kw))
    for kw in directs:
        world.add(DirectLight(**kw))
    world.camera = Camera(position=(0.5, 3.5, -6.0), resolution=(32, 24), fov=1.0, near_far=(1e-2, 1e3))
    world.camera.look_at((0.0, 0.5, 0.0))
    return world


def _context(tree=0, lights="mixed", geometry=True):
    """(context with the world uploaded, its flat scene)"""
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    world = _world(lights, geometry)
    flat = flatten(world)
    ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
    return ctx, flat


def _surface_points(ctx):
    rays = ctx.pixel_rays().reshape(-1)
    hits = ctx.trace(rays)
    found = (hits["flags"] & HIT_FOUND) != 0
    r, h = rays[found], hits[found]
    assert len(h) > 300, len(h)
    position = r["origin"] + h["t"][:, None] * r["direction"]
    assert position.dtype == F
    return bake.points(position, h["normal"], NEAR, F(FAR))


_POINTS = {}


def _points():
    """the surface points of the world, computed once (they do not depend on the tree or the lights) and never changed"""
    if "points" not in _POINTS:
        ctx, _ = _context(0, "none")
        try:
            _POINTS["points"] = _surface_points(ctx)
        finally:
            ctx.close()
        _POINTS["points"].setflags(write=False)
    return _POINTS["points"]


def _on_the_cube():
    """the index into _points() of a point on the cube's upper face (the floor lies below it and is lit from there); even and below 514, so
    that the point is in the batch of cases 1 and 2 (every other point, 257 of them), and neither of the two that batch spoils"""
    p = _points()
    at = [i for i in range(12, 512, 2) if p["position"][i][1] > 0.9 and p["normal"][i][1] > 0.8]
    assert at, "no point of the batch lies on the cube's upper face"
    return at[len(at) // 2]


def _spoil(points, at, kind):
    from test_query_gpu import _spoil as spoil      # the nine kinds are that test's, applied to the point as a ray
    as_rays = points.view(ray_dtype)
    as_rays[at] = spoil(as_rays[at], kind)


def _reconstruct(ctx, flat, points, rays, weights, lights=None, mutant=None):
    """case 2's reconstruction: the restatement's texels from the query's verdicts on the emitted rays"""
    words = ctx.occluded(rays.reshape(-1)).reshape(rays.shape) if rays.size else np.zeros(rays.shape, np.uint32)
    spots, directs = LR.select(flat.spot_lights, flat.direct_lights, lights)
    return LR.texels(points, weights, words, LR.colour_emission(spots, directs), mutant), words


def _guarded(entries, words_per_entry):
    return _hiprt.DeviceBuffer.of(np.full((entries + PAD) * words_per_entry, GUARD, np.uint32))


def _device_calls(ctx, points, n, L, seed, lights=None):
    """hiprz_light_bake and hiprz_light_rays on the first n of `points` through device pointers: (texels (n,), rays (n, L, K), weights);
    the guard words behind all three are asserted"""
    h = ctx.light()
    K = h.K
    ctx.sync()
    d_points = _hiprt.DeviceBuffer.of(points) if len(points) else _hiprt.DeviceBuffer(32)
    d_texels, d_rays, d_weights = _guarded(n, 4), _guarded(n * L * K, 8), _guarded(n * L * K, 1)
    try:
        h.bake_device(d_points.ptr, n, d_texels.ptr, seed, lights)
        h.rays_device(d_points.ptr, n, d_rays.ptr, d_weights.ptr, seed, lights)
        ctx.sync()
        texels, rays = d_texels.download(((n + PAD) * 4,), np.uint32), d_rays.download(((n * L * K + PAD) * 8,), np.uint32)
        weights = d_weights.download((n * L * K + PAD,), np.uint32)
    finally:
        d_points.free(), d_texels.free(), d_rays.free(), d_weights.free()
    assert (texels[n * 4:] == GUARD).all(), f"n = {n}, K = {K}: a texel behind n was written"
    assert (rays[n * L * K * 8:] == GUARD).all(), f"n = {n}, K = {K}: a ray behind n*L*K was written"
    assert (weights[n * L * K:] == GUARD).all(), f"n = {n}, K = {K}: a weight behind n*L*K was written"
    return texels[:n * 4].view(texel_dtype), rays[:n * L * K * 8].view(ray_dtype).reshape(n, L, K), weights[:n * L * K].view(F).reshape(n, L, K)


# =====================================================================================================================
# 1. the rays and weights are the restatement's, in every byte;  2. the texels are its fixed-order sum over the query's verdicts
# =====================================================================================================================
@pytest.mark.parametrize("lights", list(LIGHT_SETS), ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("tree", TREES)
def test_rays_weights_and_texels_are_the_restatements(built, tree, lights):
    ctx, flat = _context(tree, lights)
    try:
        points = _points()[::2][:257].copy()
        _spoil(points, 5, "nan origin"), _spoil(points, len(points) - 1, "zero direction")
        L = len(flat.spot_lights) + len(flat.direct_lights)
        compared, shadowed, partial, caught = 0, 0, 0, {m: False for m in LR.MUTANTS}
        for K in KS:
            for S in (1, 3):
                table = light.disk_samples(K, S)
                for seed in (0, 20261020):
                    texels = ctx.bake_light(points, table, seed)
                    rays, weights = ctx.light_rays(points, seed)
                    want_rays, want_weights = LR.rays(points, flat.spot_lights, flat.direct_lights, table, seed)
                    assert rays.shape == want_rays.shape == (len(points), L, K) and weights.shape == want_weights.shape
                    assert rays.tobytes() == want_rays.tobytes(), f"{lights} K {K} S {S} seed {seed}: {int((rays != want_rays).sum())} of {rays.size} rays differ"
                    assert weights.tobytes() == want_weights.tobytes(), f"{lights} K {K} S {S} seed {seed}: {int((weights.view(np.uint32) != want_weights.view(np.uint32)).sum())} of {weights.size} weights differ"
                    want, words = _reconstruct(ctx, flat, points, rays, weights)
                    assert np.array_equal(texels["shadowed"], want["shadowed"]), f"{lights} K {K} S {S} seed {seed}: shadowed differs on {int((texels['shadowed'] != want['shadowed']).sum())} points"
                    assert texels.tobytes() == want.tobytes(), f"{lights} K {K} S {S} seed {seed}: light differs on {int((texels['light'].view(np.uint32) != want['light'].view(np.uint32)).any(-1).sum())} points"
                    assert not words[weights == 0].any(), "a skipped ray is an invalid ray: never occluded"
                    compared += rays.size
                    ok = texels["shadowed"] != INVALID
                    shadowed += int(texels["shadowed"][ok].sum())
                    walked = (weights > 0).sum((1, 2))
                    partial += int(((texels["shadowed"] > 0) & (texels["shadowed"] < walked) & ok).sum())
                    if seed == 0 and S == 3 and L:          # the harness has teeth: each mutant of the restatement differs from the device somewhere
                        for mutant in LR.MUTANTS:
                            m_rays, m_weights = LR.rays(points, flat.spot_lights, flat.direct_lights, table, seed, mutant=mutant)
                            m_texels = LR.texels(points, weights, words, LR.colour_emission(flat.spot_lights, flat.direct_lights), mutant)
                            caught[mutant] |= m_rays.tobytes() != rays.tobytes() or m_weights.tobytes() != weights.tobytes() or m_texels.tobytes() != texels.tobytes()
        assert texels["shadowed"][5] == INVALID and texels["shadowed"][-1] == INVALID and (texels["light"][[5, -1]].view(np.uint32) == 0).all()
        print(f"tree {tree} {lights}: {compared} rays and weights byte-equal to the restatement, {shadowed} rays shadowed, {partial} texels in a penumbra; mutants caught: {caught}")
        if lights == "none":
            assert compared == 0 and shadowed == 0 and not texels["light"].any()
        else:
            assert shadowed > 0 and partial > 0, "the scene condition: the lights cast shadows with soft edges on these points"
        if lights in ("mixed", "edges"):     # both kinds, more than one light and skipped samples: every mutant has something to get wrong
            assert all(caught.values()), caught
        if lights == "one spot":
            assert caught["far"] and caught["skipped"]
        if lights == "at a point":     # light 0 sits at point `at` of the batch: vOP = 0, normalized(0) is NaN, and so is everything made from it
            at = _on_the_cube() // 2
            assert points["position"][at].tobytes() == flat.spot_lights[0]["position"].tobytes()
            assert (weights[at, 0].view(np.uint32) == 0).all() and (rays["direction"][at, 0].view(np.uint32) == 0).all(), "a light at the point is skipped"
            assert (rays["far"][at, 0] == points["far"][at]).all() and (weights[at, 1:] > 0).any(), "... with the point's far_, and the other lights still reach the point"
            others = np.arange(len(points)) != at
            assert (weights[others, 0] > 0).any(-1).sum() > 50, "the light at the point lights other points"
            assert texels["shadowed"][at] != INVALID and np.isfinite(texels["light"]).all()
        if lights == "edges":
            dark = [0, 1, 4, 5, 8]          # size 0, beam angle 0, emission 0 (spot); angular size 0, emission 0 (direct)
            assert (weights[:, dark].view(np.uint32) == 0).all() and (rays["direction"][:, dark].view(np.uint32) == 0).all(), "a light without light walks nothing"
            assert (weights[:, [2, 3, 6, 7]] > 0).any((0, 2)).all(), "the lights that shine, the two at their upper clamps among them, reach some point"
    finally:
        ctx.close()


# =====================================================================================================================
# 3, 4, 6, 7 on one context per tree
# =====================================================================================================================
@pytest.fixture(scope="module", params=TREES)
def lit(built, request):
    ctx, flat = _context(request.param, "mixed")
    yield ctx, flat, _points()[:257].copy()
    ctx.close()


@pytest.mark.parametrize("K", KS)
def test_sizes_at_the_edges_of_a_wave(lit, K):
    ctx, flat, points = lit
    seed, L = 11, 4
    want = ctx.bake_light(points, (K, 3), seed)
    want_rays, want_weights = ctx.light_rays(points, seed)
    assert want.tobytes() == _reconstruct(ctx, flat, points, want_rays, want_weights)[0].tobytes()
    assert want["shadowed"].any() and want["light"].any()
    for n in SIZES:
        texels, rays, weights = _device_calls(ctx, points, n, L, seed)
        assert texels.tobytes() == want[:n].tobytes(), f"K {K} n {n}: the texels differ from the first n of a larger bake"
        assert rays.tobytes() == want_rays[:n].tobytes() and weights.tobytes() == want_weights[:n].tobytes(), f"K {K} n {n}"
        assert ctx.bake_light(points[:n], None, seed).tobytes() == want[:n].tobytes(), f"host-pointer call, K {K} n {n}"
    texels, rays, weights = _device_calls(ctx, points, 0, L, seed)          # n == 0: the guards (asserted inside) are all there is
    assert len(texels) == 0 and rays.size == 0 and weights.size == 0
    assert ctx.bake_light(points[:0], None, seed).shape == (0,) and ctx.light_rays(points[:0], seed)[0].shape == (0, L, K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n,spoiled", [(1, 130, (0, 63, 64, 127, 129)), (16, 130, (0, 3, 4, 63, 129)), (128, 5, (0, 4))], ids=["K1", "K16", "K128"])
def test_invalid_points(lit, K, n, spoiled, kind):
    ctx, flat, points = lit
    clean = points[:n].copy()
    want = ctx.bake_light(clean, (K, 3), 5)
    batch = clean.copy()
    for at in spoiled:
        _spoil(batch, at, kind)
    got, got_rays, got_weights = _device_calls(ctx, batch, n, 4, 5)
    assert got.tobytes() == ctx.bake_light(batch, None, 5).tobytes()
    mask = np.zeros(n, bool)
    mask[list(spoiled)] = True
    assert got[~mask].tobytes() == want[~mask].tobytes(), "a valid point reads otherwise beside invalid ones"
    assert np.array_equal(LR.valid(batch), ~mask | (kind == "length 2"))
    if kind == "length 2":          # a valid point: the normal is normalised first, and a power of two scales exactly
        assert got.tobytes() == want.tobytes()
        return
    assert (got["shadowed"][mask] == INVALID).all(), got["shadowed"][mask]
    assert (got["light"][mask].view(np.uint32) == 0).all(), "light of an invalid point is not +0"
    assert got.tobytes() == _reconstruct(ctx, flat, batch, got_rays, got_weights)[0].tobytes()
    assert (got_rays[mask]["direction"].view(np.uint32) == 0).all() and (got_weights[mask].view(np.uint32) == 0).all()
    assert not ctx.occluded(got_rays[mask].reshape(-1)).any()


def test_ranges_select_their_lights(lit):
    ctx, flat, points = lit
    K, seed = 16, 9
    table = light.disk_samples(K, 2)
    whole = ctx.bake_light(points, table, seed)
    rays, weights = ctx.light_rays(points, seed)
    shadowed = np.zeros(len(points), np.uint64)
    total = np.zeros((len(points), 3), np.float64)
    for l, lights in enumerate(((0, 1, 0, 0), (1, 1, 2, 0), (2, 0, 0, 1), (0, 0, 1, None))):
        alone = ctx.bake_light(points, None, seed, lights)
        a_rays, a_weights = ctx.light_rays(points, seed, lights=lights)
        want_rays, want_weights = LR.rays(points, flat.spot_lights, flat.direct_lights, table, seed, lights)
        assert a_rays.shape == (len(points), 1, K) and a_rays.tobytes() == want_rays.tobytes() == rays[:, l:l + 1].tobytes()
        assert a_weights.tobytes() == want_weights.tobytes() == weights[:, l:l + 1].tobytes()
        assert alone.tobytes() == _reconstruct(ctx, flat, points, a_rays, a_weights, lights)[0].tobytes(), f"light {l} alone"
        assert alone["light"].any(), f"light {l} reaches no point: the range says nothing"
        shadowed += alone["shadowed"]
        total += alone["light"]
    assert np.array_equal(shadowed, whole["shadowed"]), "the per-light maps count the shadowed rays of the whole"
    assert np.abs(total - whole["light"]).max() <= 1e-5 * np.abs(whole["light"]).max(), "the per-light maps add up to the whole (another order of sums)"
    pair = ctx.bake_light(points, None, seed, (1, None, 0, 1))          # two lights of a range: spot 1, then direct 0
    p_rays, p_weights = ctx.light_rays(points, seed, lights=(1, None, 0, 1))
    assert p_rays.tobytes() == rays[:, 1:3].tobytes() and pair.tobytes() == _reconstruct(ctx, flat, points, p_rays, p_weights, (1, None, 0, 1))[0].tobytes()
    empty = ctx.bake_light(points, None, seed, (2, None, 2, 0))          # an empty range
    assert empty.tobytes() == bytes(16 * len(points)) and ctx.light_rays(points, seed, lights=(2, 0, 0, 0))[0].shape == (len(points), 0, K)


def test_one_point_many_times(lit):
    ctx, flat, points = lit
    texels = ctx.bake_light(points, (64, 1), 3)
    rays, weights = ctx.light_rays(points, 3)
    walked = (weights > 0).sum((1, 2))
    at = int(np.argmax((texels["shadowed"] > 0) & (texels["shadowed"] < walked)))
    assert 0 < texels["shadowed"][at] < walked[at]
    batch = np.repeat(points[at:at + 1], 257)
    for K in (1, 16, 64):
        one = ctx.bake_light(batch[:1], (K, 1), 3)          # one set: the texel of a point does not depend on its index
        got = _device_calls(ctx, batch, 257, 4, 3)[0]
        assert got.tobytes() == one.tobytes() * 257, f"K {K}: copies of one point under one set differ"
        assert got.tobytes() == ctx.bake_light(batch, None, 3).tobytes()
    assert one.tobytes() == texels[at:at + 1].tobytes()


# =====================================================================================================================
# 5. empty cases
# =====================================================================================================================
def test_an_empty_world_and_no_lights(built):
    rng = np.random.default_rng(6)
    points = bake.points(rng.uniform(-1.0, 1.0, size=(131, 3)), rng.normal(size=(131, 3)), NEAR, FAR)
    points["normal"][:3] = [[0, 1, 0], [0, -1, 0], [1, 0, -0.0]]
    _spoil(points, 64, "nan far")
    ctx, flat = _context(0, "mixed", geometry=False)
    try:
        assert not len(flat.instances) and len(flat.spot_lights) == 2
        for K in KS:
            table = light.disk_samples(K, 3)
            texels = ctx.bake_light(points, table, 9)
            rays, weights = ctx.light_rays(points, 9)
            want_rays, want_weights = LR.rays(points, flat.spot_lights, flat.direct_lights, table, 9)
            assert rays.tobytes() == want_rays.tobytes() and weights.tobytes() == want_weights.tobytes()
            want = LR.texels(points, weights, np.zeros(weights.shape, np.uint32), LR.colour_emission(flat.spot_lights, flat.direct_lights))
            assert texels.tobytes() == want.tobytes(), f"K {K}: light is not the unshadowed sum"
            assert (texels["shadowed"][np.arange(131) != 64] == 0).all() and texels["shadowed"][64] == INVALID and texels["light"].any()
    finally:
        ctx.close()
    ctx, flat = _context(3, "none")
    try:
        texels = ctx.bake_light(points, (16, 2), 1)
        assert (texels["shadowed"][np.arange(131) != 64] == 0).all() and texels["shadowed"][64] == INVALID and not texels["light"].view(np.uint32).any()
        rays, weights = ctx.light_rays(points, 1)
        assert rays.shape == weights.shape == (131, 0, 16)
    finally:
        ctx.close()


# =====================================================================================================================
# 8. staleness: the lights are read from the view of the call
# =====================================================================================================================
def test_a_bake_sees_update_shading(built):
    points = _points()[::3].copy()
    K, seed = 16, 13
    ctx, flat = _context(3, "mixed")
    try:
        before = ctx.bake_light(points, (K, 3), seed)
        world = _world("mixed")
        world.spot_lights[0].position = np.array((-1.0, 3.0, 2.0), F)
        world.spot_lights[0].color = (20, 255, 90, 255)
        world.direct_lights[1].direction = np.array((0.6, -1.0, 0.1), F)
        changed = flatten(world)
        assert changed.spot_lights.tobytes() != flat.spot_lights.tobytes() and len(changed.materials) == len(flat.materials)
        ctx._check(ctx.lib.hiprz_update_shading(ctx._ctx, changed.materials.ctypes.data, len(changed.materials), changed.spot_lights.ctypes.data, len(changed.spot_lights),
                                                changed.direct_lights.ctypes.data, len(changed.direct_lights)))
        after = ctx.bake_light(points, None, seed)
        rays, weights = ctx.light_rays(points, seed)
        assert after.tobytes() != before.tobytes(), "the bake does not see the moved light"
        assert after.tobytes() == _reconstruct(ctx, changed, points, rays, weights)[0].tobytes()
        assert rays.tobytes() == LR.rays(points, changed.spot_lights, changed.direct_lights, light.disk_samples(K, 3), seed)[0].tobytes()
        # the NUMBER of lights changes too, past Context: the arrays of light_rays are sized by the library's count of this call's view
        fewer = changed.direct_lights[:1].copy()
        ctx._check(ctx.lib.hiprz_update_shading(ctx._ctx, changed.materials.ctypes.data, len(changed.materials), changed.spot_lights.ctypes.data, len(changed.spot_lights),
                                                fewer.ctypes.data, 1))
        assert ctx.light().count() == (2, 1)
        rays3, weights3 = ctx.light_rays(points, seed)
        assert rays3.shape == (len(points), 3, K) and rays3.tobytes() == rays[:, :3].tobytes() and weights3.tobytes() == weights[:, :3].tobytes()
        texels3 = ctx.bake_light(points, None, seed)
        assert texels3.tobytes() == LR.texels(points, weights3, ctx.occluded(rays3.reshape(-1)).reshape(rays3.shape), LR.colour_emission(changed.spot_lights, fewer)).tobytes()
        ctx._check(ctx.lib.hiprz_update_shading(ctx._ctx, changed.materials.ctypes.data, len(changed.materials), changed.spot_lights.ctypes.data, len(changed.spot_lights),
                                                changed.direct_lights.ctypes.data, len(changed.direct_lights)))
        assert ctx.light().count() == (2, 2) and ctx.bake_light(points, None, seed).tobytes() == after.tobytes()
    finally:
        ctx.close()
    fresh = Context(0)
    try:
        fresh.set_tree(3)
        fresh.upload_scene(changed), fresh.upload_camera(camera_struct(world.camera))
        assert fresh.bake_light(points, (K, 3), seed).tobytes() == after.tobytes(), "a bake after update_shading differs from a fresh context's"
    finally:
        fresh.close()


# =====================================================================================================================
# 9. refusals, in their order
# =====================================================================================================================
def test_refusals(built):
    ctx = Context(0)
    try:
        points = bake.points([[0, 1, 0]], [[0, 1, 0]], NEAR, 10.0)
        h = ctx.light()
        lib, hd, p = h.lib, h._light, points.ctypes.data           # (every call below is refused before a pointer is used)
        err = lambda: lib.hiprz_light_last_error(hd)
        bad = light.light_range((0, 100, 0, 0)).ctypes.data
        # 1. a null pointer, before the missing table
        assert lib.hiprz_light_bake(hd, None, 1, 0, None, p, None) == _abi.ERR_INVALID and b"light_bake: null pointer" in err()
        assert lib.hiprz_light_rays(hd, p, 1, 0, None, p, None, None) == _abi.ERR_INVALID and lib.hiprz_light_rays(hd, p, 1, 0, None, None, p, None) == _abi.ERR_INVALID
        assert lib.hiprz_light_bake_host(hd, p, 1, 0, None, None) == _abi.ERR_INVALID
        # 2. no table, before the size and before n == 0
        assert lib.hiprz_light_bake(hd, p, 1, 0, None, p, None) == _abi.ERR_STATE and b"light_bake: no sample table" in err()
        assert lib.hiprz_light_rays(hd, p, 2**40, 0, None, p, p, None) == _abi.ERR_STATE and lib.hiprz_light_bake_host(hd, p, 0, 0, None, p) == _abi.ERR_STATE
        with pytest.raises(HiprzError) as e:
            ctx.bake_light(points, None)
        assert e.value.code == _abi.ERR_STATE
        # a bad table leaves the handle without one
        table = light.disk_samples(16, 2)
        outside = table.copy()
        outside[1, 15] = (0.8, 0.7)
        with pytest.raises(HiprzError) as e:
            h.set_samples(outside)
        assert e.value.code == _abi.ERR_INVALID and "outside the unit disk" in str(e.value)
        outside[1, 15] = (np.nan, 0.0)
        assert lib.hiprz_light_set_samples(hd, outside.ctypes.data, 16, 2) == _abi.ERR_INVALID and b"not finite" in err()
        assert lib.hiprz_light_set_samples(hd, table.ctypes.data, 48, 1) == _abi.ERR_INVALID and b"K is not a power of two" in err()
        assert lib.hiprz_light_set_samples(hd, None, 16, 2) == _abi.ERR_INVALID
        assert lib.hiprz_light_bake(hd, p, 1, 0, None, p, None) == _abi.ERR_STATE
        # 3. n*K >= 2^31 before 4. the view: a table, no scene yet
        h.set_samples(table)
        assert lib.hiprz_light_bake(hd, p, 2**27, 0, None, p, None) == _abi.ERR_INVALID and b"2^31" in err()
        assert lib.hiprz_light_rays(hd, p, 2**64 - 1, 0, None, p, p, None) == _abi.ERR_INVALID and lib.hiprz_light_bake_host(hd, p, 2**60 + 1, 0, None, p) == _abi.ERR_INVALID
        with pytest.raises(HiprzError) as e:
            ctx.bake_light(points, None)
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value), e.value
        assert lib.hiprz_light_bake(hd, p, 1, 0, bad, p, None) == _abi.ERR_STATE, "the view refuses before the range is looked at"
        with pytest.raises(HiprzError) as e:
            ctx.light_rays(points)
        assert e.value.code == _abi.ERR_STATE
        with pytest.raises(HiprzError) as e:
            h.count()
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value)
        assert ctx.bake_light(points[:0], None).shape == (0,)                      # n == 0: HIPRZ_OK without a view or a launch
        assert lib.hiprz_light_bake(hd, p, 0, 0, bad, p, None) == _abi.OK
        world = _world("mixed")
        flat = flatten(world)
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
        # 5. a bad range
        for lights in ((3, 0, 0, 0), (0, 3, 0, 0), (0, 0, 3, None), (0, 0, 1, 2), (2, 0xFFFFFFFE, 0, 0)):
            r = light.light_range(lights).ctypes.data
            assert lib.hiprz_light_bake(hd, p, 1, 0, r, p, None) == _abi.ERR_INVALID and b"light_bake: the range" in err(), lights
            assert lib.hiprz_light_rays(hd, p, 1, 0, r, p, p, None) == _abi.ERR_INVALID and lib.hiprz_light_bake_host(hd, p, 1, 0, r, p) == _abi.ERR_INVALID
        with pytest.raises(HiprzError) as e:
            ctx.light_rays(points, lights=(3, 0, 0, 0))
        assert e.value.code == _abi.ERR_INVALID and "light_count: the range" in str(e.value)
        assert h.count() == (2, 2) and h.count((1, None, 0, 1)) == (1, 1) and h.count((2, None, 2, 0)) == (0, 0)
        one = C.c_uint32()
        assert lib.hiprz_light_count(hd, None, None, C.byref(one)) == _abi.ERR_INVALID and lib.hiprz_light_count(hd, None, C.byref(one), None) == _abi.ERR_INVALID
        # ... and n*L*K >= 2^31 for the rays alone: L = 4, K = 16
        assert lib.hiprz_light_rays(hd, p, 2**25, 0, None, p, p, None) == _abi.ERR_INVALID and b"n*L*K" in err()
        with pytest.raises(TypeError):
            ctx.bake_light(np.zeros(3, np.float32), None)
        # and after all that it bakes: the table set before the scene, then the library's through Context
        first = ctx.bake_light(points, None, 1)
        assert first.tobytes() == ctx.bake_light(points, (16, 2), 1).tobytes() and first["shadowed"][0] <= 4 * 16
    finally:
        ctx.close()


# =====================================================================================================================
# 10. the atlas
# =====================================================================================================================
def test_an_atlas_is_the_three_steps(built):
    W, H, K, seed, rings = 33, 17, 16, 4, 2
    ctx, flat = _context(3, "mixed")
    try:
        world = _world("mixed")
        floor = atlas.charts(world.meshes[0])
        for k in (1, 2, 3):         # the floor's own UVs, shrunk into the middle of the atlas: gutters all round
            floor[f"u{k}"], floor[f"v{k}"] = 0.15 + 0.7 * floor[f"u{k}"], 0.2 + 0.6 * floor[f"v{k}"]
        parts = [(0, floor)]
        texels, samples, ring = ctx.bake_light_atlas(parts, W, H, (K, 3), seed, rings, NEAR, FAR)
        assert texels.shape == samples.shape == ring.shape == (H, W) and texels.dtype == texel_dtype
        points, want_samples = ctx.atlas_points(parts, W, H, NEAR, FAR)
        baked = ctx.bake_light(points, None, seed)
        want, want_ring = ctx.atlas().dilate(baked, rings)
        assert samples.tobytes() == want_samples.tobytes() and ring.tobytes() == want_ring.tobytes()
        assert texels.tobytes() == want.reshape(H, W).tobytes(), "bake_light_atlas differs from atlas points -> bake_light -> dilation"
        covered = ring == 0
        assert covered.sum() > 100 and (ring == 1).any() and (ring == atlas.NONE).any(), "charts, gutters and empty texels"
        assert texels["light"][covered].any() and texels["shadowed"][covered].any(), "the cube's shadow falls on the floor"
        one = ctx.bake_light_atlas(parts, W, H, None, seed, rings, NEAR, FAR, lights=(0, 1, 0, 0))[0]
        assert one.tobytes() == ctx.atlas().dilate(ctx.bake_light(points, None, seed, (0, 1, 0, 0)), rings)[0].reshape(H, W).tobytes() and one.tobytes() != texels.tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 11. the C++ host
# =====================================================================================================================
def test_cpp_engine_bakes_light(built, tmp_path):
    exe = str(tmp_path / "light_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "light_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "lit.json")
    scene_io.save_scene_json(_world("mixed"), scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, seed = 16, 4, 20261020
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        assert len(loaded.flat.spot_lights) == 2 and len(loaded.flat.direct_lights) == 2
        points = _surface_points(ctx).copy()
        _spoil(points, 5, "far <= near")            # an invalid point travels through the C++ host as well
        want = ctx.bake_light(points, (K, S), seed)
        want_spot0 = ctx.bake_light(points, None, seed, (0, 1, 0, 0))
        floor = atlas.charts(_world("mixed").meshes[0])
        for k in (1, 2, 3):
            floor[f"u{k}"], floor[f"v{k}"] = 0.15 + 0.7 * floor[f"u{k}"], 0.2 + 0.6 * floor[f"v{k}"]
        want_atlas, _, want_ring = ctx.bake_light_atlas([(0, floor)], 33, 17, None, seed, 2, NEAR, FAR)
    finally:
        ctx.close()
        loaded.close()
    assert want["shadowed"][5] == INVALID and want["light"].any() and want["shadowed"][want["shadowed"] != INVALID].any()
    points.tofile(str(tmp_path / "points.bin"))
    floor.tofile(str(tmp_path / "charts.bin"))
    r = subprocess.run([exe, scene_path, str(tmp_path / "points.bin"), str(tmp_path / "out.bin"), str(K), str(S), str(seed), str(tmp_path / "charts.bin"), "33", "17"],
                       capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "LIGHT DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(tmp_path / "out.bin", "rb").read() == want.tobytes(), "Engine::bakeLight differs from Context.bake_light"
    assert open(str(tmp_path / "out.bin") + ".spot0", "rb").read() == want_spot0.tobytes(), "Engine::bakeLight over a range differs from Context.bake_light"
    assert (want_ring == 0).sum() > 100 and want_atlas["light"].any()
    assert open(str(tmp_path / "out.bin") + ".atlas", "rb").read() == want_atlas.tobytes(), "Engine::bakeLightAtlas differs from Context.bake_light_atlas"
    assert open(str(tmp_path / "out.bin") + ".ring", "rb").read() == want_ring.tobytes()
