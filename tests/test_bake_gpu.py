"""Occlusion baking on the GPU (include/hiprz_bake.h: libhiprz_bake.so, Context.bake_occlusion / bake_rays, Engine::bakeOcclusion).  The
rays of a bake are held to the numpy float32 restatement (tests/bake_reference.py) in every byte; a texel is held to the query library's
own verdicts on those rays (libhiprz_query.so, itself held to the CPU oracle by tests/test_query_gpu.py) exactly, and its bent normal to
the restated butterfly sum bit for bit; the verdicts are held to the oracle directly on a sample.  Trees 0 (reference) and 3 (device SAH).

POINTS of a scene: the first hits of its pixel rays (Context.trace(ctx.pixel_rays())), position = o + t * d in float32, the normal the
hit's, near_ 1e-3, far_ 1e3 or the scene's median hit distance.

SCENES: test_order_gpu.SUBSET's eight.  Chosen with the oracle on the CPU (query_reference.oracle_rays over bake_reference.rays of 64
points per scene, K = 16): every one of them has points with 0 < occluded < K — `0` 52 of 64 points, `1` 29, `2` 53, big_leaf_9 64,
big_leaf_12 61, big_leaf_13 63, slots 11 at either far_; inside_sphere 30 at far_ 1e3 (994 of 1 024 rays occluded) and 64 at the median.
All eight were kept; case 3 asserts the condition again on the points it samples.

  1 rays         hiprz_bake_rays == bake_reference.rays in every byte: K in 16, 32, 64, 128, S in 1, 3, two seeds, at most 257 points of both
                 far_ values, two of them spoiled; the set of every point is set_of(i, seed, S).
  2 counts       occluded == the per-point sum of hiprz_query_occluded over the emitted rays, bent == the butterfly sum over those
                 verdicts bit for bit: every point of the scene, both far_, K in 16, 64, 128.
  3 oracle       at most 64 points per scene and far_, K = 16: the oracle's "found" on every emitted ray == the verdict the count is made of.
  4 shapes       n in 1, 3, 4, 5, 63, 64, 65, 257 at K in 16, 32, 64, 128 through device pointers with guard words behind the texels and
                 the rays; n == 0 writes nothing.  Host-pointer calls of 1, 4096, 4097, 8193 and 1 points at K = 16 on one handle of its
                 own (its staging is made, kept, grown twice, kept), byte-equal to the device-pointer calls.
  5 invalid      the nine kinds of test_query_gpu._spoil on the point as a ray: K = 16, n = 130 at points 0, 3, 4, 63, 129; K = 128, n = 5
                 at points 0 and 4.
  6 empty world  occluded 0 and bent = the sum of the whole table; 257 copies of one point under S = 1 give 257 equal texels.
  7 staleness    after upload, update_instances, refit and rebuild a bake equals case 2's reconstruction from a query asked afresh, and
                 differs from the bake before; after the first two also a fresh context's (the test's docstring has why not after a refit).
  8 off = off    renders with bakes between the render calls equal renders without: one part, two streams.
  9 refusals     no table, n*K >= 2^31, a context without a scene, null pointers.
 10 C++          Engine::bakeOcclusion through tests/bake_delivery_check.cpp, byte-equal to Context.bake_occlusion.

MEASURED ON MI355X: 76 cases in 3.4 s beside the session's build fixture, slowest case 0.6 s (the C++ host: it compiles a program), then
0.4 s (case 1 on scene `0`).  Case 1: 1 970 880 rays byte-equal to the restatement (246 720 per scene, 243 840 on scene `1`, which has 127
hit pixels).  Case 2: 127 to 1 536 points per scene, both far_, K in 16, 64, 128, on both trees: every count the query's, every bent
bit-equal; 440 to 9 205 partially occluded texels per scene and tree.  Case 3: 32 768 rays compared with the oracle (2 048 per scene and
tree), every verdict equal; per scene 28 to 1 384 occluded and 664 to 2 020 clear, 16 to 126 sampled points with 0 < occluded < K.  Case 7:
after update_triangles 5 of 512 texels differ from a fresh context's (the query's own difference, see the test).  Case 10: 1 536 points, one
invalid, 47 181 of 98 240 rays occluded.  No fault was found in the two kernels.
"""
import os
import subprocess

import numpy as np
import pytest

import bake_reference as BR
import guide_scenes as GS
import query_reference as QR
from rayzath_amd import _abi, _hiprt, bake, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.bake import INVALID, texel_dtype
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.query import HIT_FOUND, HIT_INVALID, ray_dtype
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
SUBSET = GS.SCENES[:3] + GS.SCENES[60:63] + ("inside_sphere", "slots")      # test_order_gpu.SUBSET: all eight meet the scene condition (docstring)
KS = (16, 32, 64, 128)
SIZES = (1, 3, 4, 5, 63, 64, 65, 257)
KINDS = ("nan origin", "inf direction", "-inf origin", "nan far", "inf far", "zero direction", "far <= near", "near < 0", "length 2")
NEAR, FAR = 1e-3, 1e3
PAD, GUARD = 8, 0xABABABAB
F = np.float32


def _context(tree=0):
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    return ctx


def _upload(ctx, key):
    flat, cam, cfg = GS.flat_scene(key)[:3]
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
    return flat, cam


def _found(hits):
    return (hits["flags"] & HIT_FOUND) != 0


def _surface_points(ctx):
    """(points at far_ 1e3, points at the median hit distance): the first hits of the pixel rays"""
    rays = ctx.pixel_rays().reshape(-1)
    hits = ctx.trace(rays)
    r, h = rays[_found(hits)], hits[_found(hits)]
    assert len(h) > 100
    position = r["origin"] + h["t"][:, None] * r["direction"]
    assert position.dtype == F
    return tuple(bake.points(position, h["normal"], NEAR, far) for far in (F(FAR), F(np.median(h["t"]))))


def _reconstruct(ctx, points, rays):
    """case 2's reconstruction: (texels from the query's verdicts on the emitted rays, the verdicts as (n, K) words)"""
    words = ctx.occluded(rays.reshape(-1)).reshape(rays.shape)
    return BR.texels(points, rays, words), words


def _spoil(points, at, kind):
    from test_query_gpu import _spoil as spoil      # the nine kinds are that test's, applied to the point as a ray
    as_rays = points.view(ray_dtype)
    as_rays[at] = spoil(as_rays[at], kind)


def _guarded(entries, words_per_entry):
    return _hiprt.DeviceBuffer.of(np.full((entries + PAD) * words_per_entry, GUARD, np.uint32))


def _device_calls(ctx, points, n, K, seed):
    """hiprz_bake_occlusion and hiprz_bake_rays on the first n of `points` through device pointers: (texels (n,), rays (n, K)); the guard
    words behind both are asserted"""
    b = ctx.bake()
    ctx.sync()
    d_points = _hiprt.DeviceBuffer.of(points) if len(points) else _hiprt.DeviceBuffer(32)
    d_texels, d_rays = _guarded(n, 4), _guarded(n * K, 8)
    try:
        b.occlusion_device(d_points.ptr, n, d_texels.ptr, seed)
        b.rays_device(d_points.ptr, n, d_rays.ptr, seed)
        ctx.sync()
        texels, rays = d_texels.download(((n + PAD) * 4,), np.uint32), d_rays.download(((n * K + PAD) * 8,), np.uint32)
    finally:
        d_points.free(), d_texels.free(), d_rays.free()
    assert (texels[n * 4:] == GUARD).all(), f"n = {n}, K = {K}: a texel behind n was written"
    assert (rays[n * K * 8:] == GUARD).all(), f"n = {n}, K = {K}: a ray behind n*K was written"
    return texels[:n * 4].view(texel_dtype), rays[:n * K * 8].view(ray_dtype).reshape(n, K)


# =====================================================================================================================
# 1. the rays are the restatement's, in every byte
# =====================================================================================================================
@pytest.mark.parametrize("key", SUBSET, ids=repr)
def test_rays_are_the_restated_rays(built, key):
    ctx = _context(0)
    try:
        _upload(ctx, key)
        far, median = _surface_points(ctx)
        points = np.concatenate([far[:129], median[:128]])
        _spoil(points, 5, "nan origin"), _spoil(points, len(points) - 1, "zero direction")
        compared = 0
        for K in KS:
            for S in (1, 3):
                table = bake.cosine_directions(K, S)
                for seed in (0, 20261020):
                    got = ctx.bake_rays(points, seed, directions=table)
                    want = BR.rays(points, table, seed)
                    assert got.shape == want.shape == (len(points), K)
                    assert got.tobytes() == want.tobytes(), f"{key!r} K {K} S {S} seed {seed}: {int((got != want).sum())} of {got.size} rays differ"
                    compared += got.size
                    sets = BR.set_of(np.arange(len(points)), seed, S)
                    assert sets[:16].tolist() == [bake.set_of(i, seed, S) for i in range(16)]
                    if S == 3:          # the set shows in the bytes: another seed deals other sets
                        assert len(np.unique(sets)) == 3 and ctx.bake_rays(points, seed + 1).tobytes() != got.tobytes()
        bad = got[[5, len(points) - 1]]
        assert (bad["direction"].view(np.uint32) == 0).all() and (bad["origin"].view(np.uint32) == points["position"][[5, -1]].view(np.uint32)[:, None]).all()
        assert (ctx.trace(bad.reshape(-1))["flags"] == HIT_INVALID).all(), "the rays of an invalid point are invalid rays"
        print(f"{key!r}: {compared} rays byte-equal to the restatement")
    finally:
        ctx.close()


# =====================================================================================================================
# 2. counts are the query's, bent is the butterfly sum over its verdicts;  3. the verdicts are the oracle's
# =====================================================================================================================
@pytest.mark.parametrize("key", SUBSET, ids=repr)
@pytest.mark.parametrize("tree", TREES)
def test_counts_are_the_querys_and_the_oracles(built, tree, key):
    ctx = _context(tree)
    try:
        flat, cam = _upload(ctx, key)
        partial, sampled = 0, dict(rays=0, occluded=0, clear=0, partial=0)
        for which, points in zip(("far 1e3", "median"), _surface_points(ctx)):
            for K in (16, 64, 128):
                seed = 7 * K
                texels = ctx.bake_occlusion(points, (K, 3), seed)
                rays = ctx.bake_rays(points, seed)
                want, words = _reconstruct(ctx, points, rays)
                assert texels.dtype == texel_dtype and texels.shape == points.shape and rays.shape == points.shape + (K,)
                assert np.array_equal(texels["occluded"], words.sum(-1)), f"{key!r} {which} K {K}: counts differ from the query's on {int((texels['occluded'] != words.sum(-1)).sum())} points"
                assert texels.tobytes() == want.tobytes(), f"{key!r} {which} K {K}: bent differs on {int((texels['bent'].view(np.uint32) != want['bent'].view(np.uint32)).any(-1).sum())} points"
                assert (texels["occluded"] <= K).all()
                partial += int(((texels["occluded"] > 0) & (texels["occluded"] < K)).sum())
                if K == 16:         # case 3 on a sample: every emitted ray through the oracle
                    pick = np.linspace(0, len(points) - 1, min(64, len(points))).astype(int)
                    oracle_found = _found(QR.oracle_rays(flat, cam, rays[pick].reshape(-1))).reshape(len(pick), K)
                    assert np.array_equal(oracle_found, words[pick] != 0), f"{key!r} {which}: {int((oracle_found != (words[pick] != 0)).sum())} of {oracle_found.size} verdicts differ from the oracle's"
                    count = oracle_found.sum(-1)
                    sampled["rays"] += oracle_found.size
                    sampled["occluded"] += int(oracle_found.sum())
                    sampled["clear"] += int((~oracle_found).sum())
                    sampled["partial"] += int(((count > 0) & (count < K)).sum())
        print(f"tree {tree} {key!r}: {len(points)} points, {partial} partially occluded texels; oracle: {sampled['rays']} rays compared, {sampled['occluded']} occluded, "
              f"{sampled['clear']} clear, {sampled['partial']} sampled points with 0 < occluded < K")
        assert sampled["partial"] > 0, "the scene condition: the oracle alone finds a point with 0 < occluded < K"
    finally:
        ctx.close()


# =====================================================================================================================
# 4 - 6 on one context per tree
# =====================================================================================================================
@pytest.fixture(scope="module", params=TREES)
def sphere(built, request):
    """inside_sphere at the median distance: about a third of the rays of a point are occluded, so count and bent both say something"""
    ctx = _context(request.param)
    _upload(ctx, "inside_sphere")
    points = _surface_points(ctx)[1][:257].copy()
    yield ctx, points
    ctx.close()


@pytest.mark.parametrize("K", KS)
def test_shapes_at_the_edges_of_a_wave(sphere, K):
    ctx, points = sphere
    seed = 11
    want = ctx.bake_occlusion(points, (K, 3), seed)
    want_rays = ctx.bake_rays(points, seed)
    assert want.tobytes() == _reconstruct(ctx, points, want_rays)[0].tobytes()
    assert 0 < int(want["occluded"].sum()) < K * len(points) and ((want["occluded"] > 0) & (want["occluded"] < K)).any()
    for n in SIZES:
        texels, rays = _device_calls(ctx, points, n, K, seed)
        assert texels.tobytes() == want[:n].tobytes(), f"K {K} n {n}: the texels differ from the first n of a larger bake"
        assert rays.tobytes() == want_rays[:n].tobytes(), f"K {K} n {n}"
        assert ctx.bake_occlusion(points[:n], None, seed).tobytes() == want[:n].tobytes(), f"host-pointer call, K {K} n {n}"
    texels, rays = _device_calls(ctx, points, 0, K, seed)          # n == 0: the guards (asserted inside) are all there is
    assert len(texels) == 0 and rays.size == 0
    assert ctx.bake_occlusion(points[:0], None, seed).shape == (0,) and ctx.bake_rays(points[:0], seed).shape == (0, K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n,spoiled", [(16, 130, (0, 3, 4, 63, 129)), (128, 5, (0, 4))], ids=["K16", "K128"])
def test_invalid_points(sphere, K, n, spoiled, kind):
    ctx, points = sphere
    clean = points[:n].copy()
    want = ctx.bake_occlusion(clean, (K, 3), 5)
    assert (want["occluded"] <= K).all() and want["occluded"].any()
    batch = clean.copy()
    for at in spoiled:
        _spoil(batch, at, kind)
    got, got_rays = _device_calls(ctx, batch, n, K, 5)
    assert got.tobytes() == ctx.bake_occlusion(batch, None, 5).tobytes()
    mask = np.zeros(n, bool)
    mask[list(spoiled)] = True
    assert got[~mask].tobytes() == want[~mask].tobytes(), "a valid point reads otherwise beside invalid ones"
    assert np.array_equal(BR.valid(batch), ~mask | (kind == "length 2"))
    if kind == "length 2":          # a valid point: the normal is normalised first, and a power of two scales exactly
        assert got.tobytes() == want.tobytes()
        return
    assert (got["occluded"][mask] == INVALID).all(), got["occluded"][mask]
    assert (got["bent"][mask].view(np.uint32) == 0).all(), "bent of an invalid point is not +0"
    assert got.tobytes() == _reconstruct(ctx, batch, got_rays)[0].tobytes()
    assert (got_rays[mask]["direction"].view(np.uint32) == 0).all() and not ctx.occluded(got_rays[mask].reshape(-1)).any()


def test_one_point_many_times(sphere):
    ctx, points = sphere
    occluded = ctx.bake_occlusion(points, (64, 1), 3)["occluded"]
    at = int(np.argmax((occluded > 0) & (occluded < 64)))
    assert 0 < occluded[at] < 64
    batch = np.repeat(points[at:at + 1], 257)
    for K in (16, 64):
        one = ctx.bake_occlusion(batch[:1], (K, 1), 3)          # one set: the texel of a point does not depend on its index
        texels = _device_calls(ctx, batch, 257, K, 3)[0]
        assert texels.tobytes() == one.tobytes() * 257, f"K {K}: copies of one point under one set differ"
        assert texels.tobytes() == ctx.bake_occlusion(batch, None, 3).tobytes()
    assert one.tobytes() == ctx.bake_occlusion(points, None, 3)[at:at + 1].tobytes()


def test_an_empty_world(built):
    empty = GS._world(0)[0]
    GS._camera(empty)
    flat = flatten(empty)
    assert not len(flat.instances)
    rng = np.random.default_rng(6)
    points = bake.points(rng.normal(size=(131, 3)), rng.normal(size=(131, 3)), NEAR, FAR)
    points["normal"][:3] = [[0, 0, 1], [0, 0, -1], [1, 0, -0.0]]
    _spoil(points, 64, "nan far")
    ctx = _context(0)
    try:
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(empty.camera))
        for K in KS:
            table = bake.cosine_directions(K, 3)
            texels = ctx.bake_occlusion(points, table, 9)
            rays = BR.rays(points, table, 9)
            want = BR.texels(points, rays, np.zeros(rays.shape, np.uint32))
            assert texels.tobytes() == want.tobytes(), f"K {K}: bent is not the butterfly sum of the whole table"
            assert (texels["occluded"][np.arange(131) != 64] == 0).all() and texels["occluded"][64] == INVALID
            # the sum of a cosine table leans along the normal: its length is K * mean(z) = 2K/3 up to the stratification
            along = (texels["bent"].astype(np.float64) * BR.normalized(points["normal"]).astype(np.float64)).sum(-1)[np.arange(131) != 64]
            assert np.abs(along / K - 2.0 / 3.0).max() < 1.0 / K + 1e-5
    finally:
        ctx.close()


# =====================================================================================================================
# 7. staleness: the scene is read from the view of the call
# =====================================================================================================================
def test_a_bake_sees_every_update(built):
    """After every kind of update the bake equals case 2's reconstruction from a query asked afresh of the same context, and differs from
    the bake before.  After upload_scene and update_instances it also equals the reconstruction from a FRESH context's query on the
    changed scene.  Not so after update_triangles: there the context's own closest hit and occlusion already differ from a fresh
    context's on 9 of these 16 384 rays (measured on MI355X, equally against fresh trees 0 and 3, and unchanged by rebuild_trees) — rays
    that start on the old surface and graze the deformed one; tests/test_query_gpu.py compares the two on pixel rays, where they agree.
    That difference is the renderer's and the query's, upstream of this library, and is not held against the bake."""
    from test_query_gpu import _fresh_trace, _sphere_world, _uploaded_order
    worlds = dict(plain=_sphere_world(), moved=_sphere_world(moved=True), changed=_sphere_world(moved=True, deformed=True))
    flats = {k: flatten(w) for k, w in worlds.items()}
    cam = camera_struct(worlds["plain"].camera)
    other = GS.flat_scene("slots")[0]
    K, seed = 32, 13
    ctx = _context(3)
    try:
        ctx.upload_scene(flats["plain"]), ctx.upload_camera(cam)
        points = _surface_points(ctx)[0][::3].copy()           # on the sphere as first uploaded; they stay where they are
        ctx.bake().set_directions((K, 3))
        rays = ctx.bake_rays(points, seed)
        assert rays.tobytes() == BR.rays(points, bake.cosine_directions(K, 3), seed).tobytes()

        def fresh(flat):
            words = _found(_fresh_trace(flat, rays.reshape(-1))).astype(np.uint32)      # occluded == found on the same ray (test_query_gpu case 4)
            return BR.texels(points, rays, words)

        def asked_afresh():
            return _reconstruct(ctx, points, rays)[0]
        ctx.upload_scene(other)
        before = ctx.bake_occlusion(points, None, seed)
        assert before.tobytes() == asked_afresh().tobytes() == fresh(other).tobytes()
        ctx.upload_scene(flats["plain"])
        got = ctx.bake_occlusion(points, None, seed)
        assert got.tobytes() == asked_afresh().tobytes() == fresh(flats["plain"]).tobytes() and got.tobytes() != before.tobytes(), "after upload_scene"
        ctx.update_instances(flats["moved"].instances)
        moved = ctx.bake_occlusion(points, None, seed)
        assert moved.tobytes() == asked_afresh().tobytes() == fresh(flats["moved"]).tobytes() and moved.tobytes() != got.tobytes(), "after update_instances"
        order = _uploaded_order(worlds["plain"], flats["plain"], flats["changed"])
        ctx.update_triangles(0, flats["changed"].tris[order], flats["changed"].tri_attrs[order])
        refitted = ctx.bake_occlusion(points, None, seed)
        assert refitted.tobytes() == asked_afresh().tobytes() and refitted.tobytes() != moved.tobytes(), "after update_triangles"
        differ = int((refitted["occluded"] != fresh(flats["changed"])["occluded"]).sum())
        print(f"after update_triangles: {differ} of {len(points)} texels differ from a fresh context's on the changed scene (the query's own difference)")
        assert differ <= len(points) // 50, "the refitted scene is not the changed scene at all"
        ctx.rebuild_trees(3)
        assert ctx.bake_occlusion(points, None, seed).tobytes() == asked_afresh().tobytes() == refitted.tobytes(), "after rebuild_trees"
        assert ctx.bake_rays(points, seed).tobytes() == rays.tobytes(), "the rays read no scene"
    finally:
        ctx.close()


# =====================================================================================================================
# 8. nothing else changes
# =====================================================================================================================
_CALLS = (1, 3, 8, 2, 8)


@pytest.mark.parametrize("kind", ["single", "two-streams"])
def test_bakes_change_nothing_else(built, kind):
    world = scenes.shading_inputs_scene(80, 48, lights=True)
    flat, cam = flatten(world), camera_struct(world.camera)
    results, baked = [], None
    for ask in (True, False):
        ctx = Context([0, 0]) if kind == "two-streams" else Context(0)
        try:
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(None, Tracing(6, 4)).struct())
            for k, n in enumerate(_CALLS):
                ctx.render(n)
                if ask and k + 1 < len(_CALLS):
                    points = _surface_points(ctx)[k % 2]
                    baked = ctx.bake_occlusion(points, (16 << k, 2), k)
                    rays = ctx.bake_rays(points, k)
            if ask:
                assert baked.tobytes() == _reconstruct(ctx, points, rays)[0].tobytes() and ((baked["occluded"] > 0) & (baked["occluded"] < 128)).any()
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.ray_count(), ctx.pass_count(),
                            ctx.graph_captures(), ctx.read_guides().tobytes()))
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "ray_count", "pass_count", "graph_captures", "guides"), *results):
        assert a == b, f"{kind}: {name} differs once bakes run between the render calls"


# =====================================================================================================================
# 9. refusals
# =====================================================================================================================
def test_refusals(built):
    ctx = _context(0)
    try:
        points = bake.points([[0, 0, 0]], [[0, 0, 1]], NEAR, 1.0)
        b = ctx.bake()
        lib, h, p = b.lib, b._bake, points.ctypes.data           # (every call below is refused before a pointer is used)
        err = lambda: lib.hiprz_bake_last_error(h)
        # no table
        assert lib.hiprz_bake_occlusion(h, p, 1, 0, p, None) == _abi.ERR_STATE and b"bake_occlusion: no direction table" in err()
        assert lib.hiprz_bake_rays(h, p, 1, 0, p, None) == _abi.ERR_STATE and lib.hiprz_bake_occlusion_host(h, p, 1, 0, p) == _abi.ERR_STATE
        assert lib.hiprz_bake_occlusion(h, p, 0, 0, p, None) == _abi.ERR_STATE, "no table is refused before n == 0 is looked at"
        with pytest.raises(HiprzError) as e:
            ctx.bake_occlusion(points, None)
        assert e.value.code == _abi.ERR_STATE
        # a bad table leaves the handle without one
        table = bake.cosine_directions(16, 2)
        bad = table.copy()
        bad[1, 15, 2] = np.nan
        with pytest.raises(HiprzError) as e:
            b.set_directions(bad)
        assert e.value.code == _abi.ERR_INVALID and "not finite" in str(e.value)
        assert lib.hiprz_bake_set_directions(h, table.ctypes.data, 48, 1) == _abi.ERR_INVALID and b"K is not one of" in err()
        assert lib.hiprz_bake_set_directions(h, None, 16, 2) == _abi.ERR_INVALID
        assert lib.hiprz_bake_rays(h, p, 1, 0, p, None) == _abi.ERR_STATE
        # a table, no scene: the table may be set before a scene is uploaded
        b.set_directions(table)
        with pytest.raises(HiprzError) as e:
            ctx.bake_occlusion(points, None)
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value), e.value
        with pytest.raises(HiprzError) as e:
            ctx.bake_rays(points)
        assert e.value.code == _abi.ERR_STATE
        assert ctx.bake_occlusion(points[:0], None).shape == (0,)                      # n == 0: HIPRZ_OK without a view or a launch
        assert lib.hiprz_bake_occlusion(h, p, 0, 0, p, None) == _abi.OK
        _upload(ctx, "slots")
        # n*K >= 2^31, with a dummy pointer: refused before use
        for call in (lambda n: lib.hiprz_bake_occlusion(h, p, n, 0, p, None), lambda n: lib.hiprz_bake_rays(h, p, n, 0, p, None),
                     lambda n: lib.hiprz_bake_occlusion_host(h, p, n, 0, p)):
            assert call(2**27) == _abi.ERR_INVALID and b"2^31" in err()
            assert call(2**64 - 1) == _abi.ERR_INVALID and call(2**60 + 1) == _abi.ERR_INVALID
        assert lib.hiprz_bake_occlusion(h, None, 1, 0, p, None) == _abi.ERR_INVALID and b"null pointer" in err()
        assert lib.hiprz_bake_occlusion(h, p, 1, 0, None, None) == _abi.ERR_INVALID and lib.hiprz_bake_rays(h, p, 1, 0, None, None) == _abi.ERR_INVALID
        assert lib.hiprz_bake_occlusion_host(h, None, 1, 0, p) == _abi.ERR_INVALID and lib.hiprz_bake_occlusion_host(h, p, 1, 0, None) == _abi.ERR_INVALID
        with pytest.raises(TypeError):
            ctx.bake_occlusion(np.zeros(3, np.float32), None)
        # and after all that it bakes: the table set before the scene, then the library's through Context
        first = ctx.bake_occlusion(points, None, 1)
        assert first.tobytes() == ctx.bake_occlusion(points, (16, 2), 1).tobytes() and first["occluded"][0] <= 16
    finally:
        ctx.close()


# =====================================================================================================================
# 10. the C++ host
# =====================================================================================================================
def test_cpp_engine_bakes(built, tmp_path):
    exe = str(tmp_path / "bake_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "bake_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "sphere.json")
    scene_io.save_scene_json(scenes.textured_sphere_scene(48, 32, resolution=24, map_size=32), scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, seed = 64, 4, 20261020
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        points = _surface_points(ctx)[1].copy()
        _spoil(points, 5, "far <= near")            # an invalid point travels through the C++ host as well
        want = ctx.bake_occlusion(points, (K, S), seed)
    finally:
        ctx.close()
        loaded.close()
    assert want["occluded"][5] == INVALID and ((want["occluded"] > 0) & (want["occluded"] < K)).sum() > 100
    points.tofile(str(tmp_path / "points.bin"))
    r = subprocess.run([exe, scene_path, str(tmp_path / "points.bin"), str(tmp_path / "out.bin"), str(K), str(S), str(seed)], capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "BAKE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = open(tmp_path / "out.bin", "rb").read()
    assert out == want.tobytes(), "Engine::bakeOcclusion differs from Context.bake_occlusion"


GROWTH = (1, 4096, 4097, 8193, 1)      # on one new handle: a staging of 4096 made, kept, grown to 8192, grown to 16 384, kept


def test_one_handle_grows_its_staging_twice(sphere):
    """Host-pointer calls of GROWTH's sizes at K = 16 on one handle of its own: every result equals, byte for byte, the device-pointer call
    over the same points (the surface points of `inside_sphere`, repeated to 8 193: point i uses set_of(i), so a repeat is another case)."""
    ctx = sphere[0]
    points = np.resize(_surface_points(ctx)[1], max(GROWTH))
    b = bake.Bake(ctx._ctx)
    ctx.sync()      # (makes the head device the current one for the buffers)
    d_points, d_texels = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(points.size * texel_dtype.itemsize)
    try:
        b.set_directions((16, 3))
        for turn, n in enumerate(GROWTH):
            got = b.occlusion(points[:n], 7)
            b.occlusion_device(d_points.ptr, n, d_texels.ptr, 7)
            ctx.sync()
            want = d_texels.download((n,), texel_dtype)
            assert (want["occluded"] <= 16).all() and (n == 1 or 0 < int(want["occluded"].sum()) < 16 * n), n
            assert got.tobytes() == want.tobytes(), f"turn {turn}, n = {n}: the bake through the staging"
    finally:
        d_points.free(), d_texels.free()
        b.close()
