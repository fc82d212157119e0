"""Ordered ray queries on the GPU (include/hiprz_order.h: libhiprz_order.so, hiprz_sort_u32_device, Context.trace / occluded with
ordered=True, Context.ray_order, Engine::castRays(..., ordered)).  Every ray is independent, so the ordered walk is held to the BYTES of the
caller-order walk (libhiprz_query.so, itself held to the CPU oracle by tests/test_query_gpu.py), and on the recipe rays to the oracle
directly.  Trees 0 (reference) and 3 (device SAH).

  1 bytes        per scene of SUBSET: the pixel rays in a seeded random permutation followed by the scene's recipe rays, with and without
                 NORMALIZE: order.closest == query.closest and order.occluded == query.occluded in every byte; the recipe rays under
                 NORMALIZE against query_reference.scene_reference under test_query_gpu's rule (no discrete difference, far within the cap).
  2 sizes        n in 1, 63, 64, 65, 4095, 4096, 4097, 8193 (the wave is 64, the sort's tile 4096 keys) through device pointers with guard
                 words behind hits, occlusion words, keys and permutation; n == 0 writes nothing.
  3 permutation  perm is a permutation, equals numpy's stable argsort of the keys read back, keys < 2^24, invalid rays have key 0, and on the
                 permuted pixel rays it moves more than half of the rays.
  4 one bucket   8193 copies of one ray: perm == arange, 8193 equal records.
  5 invalid      the nine kinds of test_query_gpu.test_invalid_rays at positions 0, 31, 63, 64 and 129 of 130.
  6 _by          the library's own order, the reversal, and an order with one index >= n.
  7 staleness    after upload, update_instances, refit and rebuild an ordered query equals a fresh caller-order query.
  8 off = off    renders with ordered queries between the render calls equal renders without: one part, two streams, and the split
                 pipeline with ray sorting on (the frame's own sort workspace).
  9 the sort     hiprz_sort_u32_device on seeded keys of 8, 16, 24, 32 bits at 1, 4096, 4097 keys: numpy's stable argsort; refusals.
 10 refusals     of the order calls; an empty world misses on every ray.
 11 C++          Engine::castRays / ::occluded with ordered = true through tests/order_delivery_check.cpp.

MEASURED ON MI355X: 113 cases in 3.4 s beside the session's build fixture, slowest case 0.7 s (the C++ host: it compiles a program).  Case 1:
729 to 1 568 rays per scene and tree, byte-equal to the caller-order walk under both flags; the 32 recipe rays of each of the 8 scenes on both
trees equal the oracle in all 48 bytes (far 0, discrete 0).  Case 3: the 1 089 shuffled pixel rays of `inside_sphere` have 96 distinct keys and
the order moves all 1 089.  No fault was found in the three kernels or in hiprz_sort_u32_device.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guide_scenes as GS
import query_reference as QR
from rayzath_amd import _abi, _hiprt, query, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.query import HIT_FOUND, HIT_INVALID, hit_dtype
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
SUBSET = GS.SCENES[:3] + GS.SCENES[60:63] + ("inside_sphere", "slots")      # generated, tree shapes, hand-made: the first of each kind
SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
KINDS = ("nan origin", "inf direction", "-inf origin", "nan far", "inf far", "zero direction", "far <= near", "near < 0", "length 2")
HIT, PAD, GUARD = hit_dtype.itemsize, 8, 0xABABABAB


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


def _shuffled_pixel_rays(ctx, seed):
    rays = ctx.pixel_rays().reshape(-1)
    return rays[np.random.default_rng(seed).permutation(len(rays))].copy()


def _tiled(rays, n):
    return np.tile(rays, -(-n // len(rays)))[:n].copy()


def _spoil(ray, kind):
    from test_query_gpu import _spoil as spoil      # the nine kinds are that test's, not restated
    return spoil(ray, kind)


def _guarded(n, words_per_entry):
    return _hiprt.DeviceBuffer.of(np.full((n + PAD) * words_per_entry, GUARD, np.uint32))


def _device_calls(ctx, rays, n, normalize, perm=None):
    """the device-pointer calls on the first n of `rays` (fused, or _by the order `perm`): (hits, occlusion) of n entries; the guard words
    behind them are asserted"""
    o = ctx.order()
    ctx.sync()
    d_rays = _hiprt.DeviceBuffer.of(rays) if len(rays) else _hiprt.DeviceBuffer(32)
    d_hits, d_occ = _guarded(n, HIT // 4), _guarded(n, 1)
    d_perm = _hiprt.DeviceBuffer.of(np.ascontiguousarray(perm, np.uint32)) if perm is not None else None
    try:
        o.closest_device(d_rays.ptr, n, d_hits.ptr, normalize, perm_ptr=d_perm.ptr if d_perm else None)
        o.occluded_device(d_rays.ptr, n, d_occ.ptr, normalize, perm_ptr=d_perm.ptr if d_perm else None)
        ctx.sync()
        hits, occ = d_hits.download(((n + PAD) * HIT // 4,), np.uint32), d_occ.download((n + PAD,), np.uint32)
    finally:
        d_rays.free(), d_hits.free(), d_occ.free()
        if d_perm:
            d_perm.free()
    assert (hits[n * HIT // 4:] == GUARD).all(), f"n = {n}: a hit behind n was written"
    assert (occ[n:] == GUARD).all(), f"n = {n}: an occlusion word behind n was written"
    return hits[:n * HIT // 4].view(hit_dtype), occ[:n]


def _device_order(ctx, rays, n, normalize):
    """hiprz_order_permutation on the first n of `rays` through guarded buffers: (perm, keys)"""
    o = ctx.order()
    ctx.sync()
    d_rays = _hiprt.DeviceBuffer.of(rays) if len(rays) else _hiprt.DeviceBuffer(32)
    d_perm, d_keys = _guarded(n, 1), _guarded(n, 1)
    try:
        o.permutation_device(d_rays.ptr, n, d_perm.ptr, d_keys.ptr, normalize)
        ctx.sync()
        perm, keys = d_perm.download((n + PAD,), np.uint32), d_keys.download((n + PAD,), np.uint32)
    finally:
        d_rays.free(), d_perm.free(), d_keys.free()
    assert (perm[n:] == GUARD).all() and (keys[n:] == GUARD).all(), f"n = {n}: a word behind n was written"
    return perm[:n], keys[:n]


# =====================================================================================================================
# 1. byte equality with the caller-order walk, and the oracle on the recipe rays
# =====================================================================================================================
@pytest.mark.parametrize("key", SUBSET, ids=repr)
@pytest.mark.parametrize("tree", TREES)
def test_ordered_bytes_are_the_caller_order_bytes(built, tree, key):
    ctx = _context(tree)
    try:
        flat = _upload(ctx, key)[0]
        shuffled = _shuffled_pixel_rays(ctx, QR.seed_of(key))
        recipe = QR.scene_rays(key)[0]
        batch = np.concatenate([shuffled, recipe])
        for normalize in (False, True):
            plain, plain_occ = ctx.trace(batch, normalize), ctx.occluded(batch, normalize)
            got, got_occ = ctx.trace(batch, normalize, ordered=True), ctx.occluded(batch, normalize, ordered=True)
            assert got.tobytes() == plain.tobytes(), f"{key!r} normalize {normalize}: {int((got != plain).sum())} of {len(batch)} ordered hits differ"
            assert got_occ.tobytes() == plain_occ.tobytes(), f"{key!r} normalize {normalize}: ordered occlusion differs"
            assert np.array_equal(got_occ, _found(got).astype(np.uint32))
        if len(flat.instances):
            assert not (got["flags"][:len(shuffled)] & HIT_INVALID).any()
        ordered = ctx.trace(recipe, normalize=True, ordered=True)
        r = QR.compare(ordered, QR.scene_reference(key))
        print(f"tree {tree} {key!r}: {len(batch)} rays, {int(_found(got).sum())} hit; recipe against the oracle: {r['rays']} rays, exact {r['exact']}, far {r['far']}, discrete {r['discrete']}")
        assert QR.misses_read_as_specified(ordered, recipe)
        assert r["discrete"] == 0, "\n".join(r["worst"])
        assert r["far"] <= GS.scene_cap(key, 0), "\n".join(r["worst"])
    finally:
        ctx.close()


# =====================================================================================================================
# 2 - 6 on one context: a world whose every valid ray hits, so an unwritten or invalid record cannot pass for a miss
# =====================================================================================================================
@pytest.fixture(scope="module", params=TREES)
def sphere(built, request):
    ctx = _context(request.param)
    _upload(ctx, "inside_sphere")
    rays = _shuffled_pixel_rays(ctx, 20261019)
    yield ctx, rays
    ctx.close()


@pytest.mark.parametrize("normalize", [False, True])
def test_batch_sizes_at_the_edges_of_both_kernels(sphere, normalize):
    ctx, rays = sphere
    big = _tiled(rays, max(SIZES))
    want, want_occ = ctx.trace(big, normalize), ctx.occluded(big, normalize)
    assert _found(want).all()
    for n in SIZES:
        hits, occ = _device_calls(ctx, big, n, normalize)
        assert hits.tobytes() == want[:n].tobytes(), n
        assert np.array_equal(occ, want_occ[:n]), n
        assert ctx.trace(big[:n], normalize, ordered=True).tobytes() == want[:n].tobytes(), f"host-pointer call, n = {n}"
        assert np.array_equal(ctx.occluded(big[:n], normalize, ordered=True), want_occ[:n]), f"host-pointer call, n = {n}"
    hits, occ = _device_calls(ctx, big, 0, normalize)        # n == 0: the guards (asserted inside) are all there is
    assert len(hits) == 0 and len(occ) == 0
    perm, keys = _device_order(ctx, big, 0, normalize)
    assert len(perm) == 0 and len(keys) == 0
    assert ctx.trace(big[:0], normalize, ordered=True).shape == (0,) and ctx.occluded(big[:0], normalize, ordered=True).shape == (0,)


@pytest.mark.parametrize("n", SIZES)
def test_the_permutation_is_the_stable_order_of_the_keys(sphere, n):
    ctx, rays = sphere
    batch = _tiled(rays, n)
    spoiled = sorted({0, n // 2, n - 1})
    for k, at in enumerate(spoiled):
        batch[at] = _spoil(batch[at], KINDS[k])
    perm, keys = _device_order(ctx, batch, n, False)
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), "not a permutation of 0..n-1"
    assert (keys < 2**24).all()
    assert (keys[spoiled] == 0).all(), "an invalid ray's key is not 0"
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32)), "not the stable order of the keys"
    host_perm, host_keys = ctx.ray_order(batch)
    assert np.array_equal(host_perm, perm) and np.array_equal(host_keys, keys)


def test_the_permutation_moves_the_shuffled_pixel_rays(sphere):
    ctx, rays = sphere
    n = len(rays)
    perm, keys = ctx.ray_order(rays)
    assert perm.dtype == np.uint32 and perm.shape == (n,) == keys.shape
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32)) and (keys < 2**24).all()
    moved = int((perm != np.arange(n)).sum())
    print(f"{n} shuffled pixel rays: {len(np.unique(keys))} distinct keys, {moved} rays moved")
    assert moved > n // 2, "the input is in key order already: the byte equalities above would hold for an identity order"
    assert ctx.trace(rays, ordered=True).tobytes() == ctx.trace(rays).tobytes()
    normalized = ctx.ray_order(rays, normalize=True)          # unit directions: the normalised direction differs in the last bits at most
    assert np.array_equal(np.sort(normalized[0]), np.arange(n, dtype=np.uint32))


def test_one_bucket(sphere):
    ctx, rays = sphere
    n = 8193
    batch = np.repeat(rays[:1], n)
    perm, keys = _device_order(ctx, batch, n, False)
    assert (keys == keys[0]).all() and np.array_equal(perm, np.arange(n, dtype=np.uint32)), "equal keys do not keep their order"
    hits, occ = _device_calls(ctx, batch, n, False)
    one = ctx.trace(batch[:1])
    assert _found(one).all() and hits.tobytes() == one.tobytes() * n and (occ == 1).all()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_invalid_rays(sphere, kind, normalize):
    ctx, rays = sphere
    n, lanes = 130, [0, 31, 63, 64, 129]
    clean = rays[:n].copy()
    want, want_occ = ctx.trace(clean, normalize, ordered=True), ctx.occluded(clean, normalize, ordered=True)
    assert _found(want).all() and want_occ.all() and want.tobytes() == ctx.trace(clean, normalize).tobytes()
    batch = clean.copy()
    for lane in lanes:
        batch[lane] = _spoil(clean[lane], kind)
    hits, occ = ctx.trace(batch, normalize, ordered=True), ctx.occluded(batch, normalize, ordered=True)
    assert hits.tobytes() == ctx.trace(batch, normalize).tobytes() and np.array_equal(occ, ctx.occluded(batch, normalize))
    spoiled = np.zeros(n, bool)
    spoiled[lanes] = True
    assert hits[~spoiled].tobytes() == want[~spoiled].tobytes() and np.array_equal(occ[~spoiled], want_occ[~spoiled]), "a valid ray reads otherwise beside invalid ones"
    keys = ctx.ray_order(batch, normalize)[1]
    if kind == "length 2" and normalize:         # a valid ray under NORMALIZE: the same unit direction (a power of two scales exactly)
        assert hits.tobytes() == want.tobytes() and np.array_equal(occ, want_occ)
        return
    bad = hits[spoiled]
    assert (keys[spoiled] == 0).all()
    assert (bad["flags"] == HIT_INVALID).all(), bad["flags"]
    assert (bad["t"].view(np.uint32) == batch["far"][spoiled].view(np.uint32)).all(), "t is not the input far's bits"
    for name, value in (("instance", -1), ("material_slot", -1), ("material", -1), ("triangle", 0), ("scene_triangle", -1)):
        assert (bad[name] == value).all(), name
    assert (bad["u"].view(np.uint32) == 0).all() and (bad["v"].view(np.uint32) == 0).all() and (bad["normal"].view(np.uint32) == 0).all()
    assert not occ[spoiled].any()


@pytest.mark.parametrize("normalize", [False, True])
def test_a_kept_permutation(sphere, normalize):
    ctx, rays = sphere
    n = 4097
    batch = _tiled(rays, n)
    want, want_occ = ctx.trace(batch, normalize), ctx.occluded(batch, normalize)
    fused, fused_occ = _device_calls(ctx, batch, n, normalize)
    assert fused.tobytes() == want.tobytes() and np.array_equal(fused_occ, want_occ)
    own = _device_order(ctx, batch, n, normalize)[0]
    for name, perm in (("the library's own order", own), ("the reversal", np.arange(n, dtype=np.uint32)[::-1])):
        hits, occ = _device_calls(ctx, batch, n, normalize, perm)
        assert hits.tobytes() == fused.tobytes() and np.array_equal(occ, fused_occ), name
    # one index >= n: that thread does nothing — its record keeps the guard, every other record is written, nothing outside [0, n) is
    # touched (the guards behind n are asserted in _device_calls)
    for outside in (n, n + 3, 0xFFFFFFFF):
        perm = own.copy()
        skipped = int(perm[100])
        perm[100] = outside
        hits, occ = _device_calls(ctx, batch, n, normalize, perm)
        others = np.arange(n) != skipped
        assert hits[others].tobytes() == fused[others].tobytes() and np.array_equal(occ[others], fused_occ[others]), outside
        assert (hits[skipped:skipped + 1].view(np.uint32) == GUARD).all() and occ[skipped] == GUARD, outside


# =====================================================================================================================
# 7. staleness: the key reads the world box from the view of the call
# =====================================================================================================================
def test_an_ordered_query_sees_every_update(built):
    from test_query_gpu import _fresh_trace, _sphere_world, _uploaded_order
    worlds = dict(plain=_sphere_world(), moved=_sphere_world(moved=True), changed=_sphere_world(moved=True, deformed=True))
    flats = {k: flatten(w) for k, w in worlds.items()}
    cam = camera_struct(worlds["plain"].camera)
    other = GS.flat_scene("slots")[0]
    ctx = _context(3)
    try:
        ctx.upload_scene(other), ctx.upload_camera(cam)
        rays = _shuffled_pixel_rays(ctx, 7)
        want = {k: _fresh_trace(f, rays) for k, f in flats.items()}
        before = ctx.trace(rays, ordered=True)
        keys_before = ctx.ray_order(rays)[1]
        assert before.tobytes() == _fresh_trace(other, rays).tobytes()
        ctx.upload_scene(flats["plain"])
        got = ctx.trace(rays, ordered=True)
        assert got.tobytes() == want["plain"].tobytes() and got.tobytes() != before.tobytes(), "after upload_scene"
        assert _found(got).sum() > 500
        assert not np.array_equal(ctx.ray_order(rays)[1], keys_before), "the keys still read the first scene's world box"
        ctx.update_instances(flats["moved"].instances)
        moved = ctx.trace(rays, ordered=True)
        assert moved.tobytes() == want["moved"].tobytes() and moved.tobytes() != got.tobytes(), "after update_instances"
        order = _uploaded_order(worlds["plain"], flats["plain"], flats["changed"])
        ctx.update_triangles(0, flats["changed"].tris[order], flats["changed"].tri_attrs[order])

        def same_as_fresh(hits, what):
            as_fresh = hits.copy()           # scene_triangle counts in the order this context was given: into the changed scene's order
            found = _found(hits)
            as_fresh["scene_triangle"][found] = order[hits["scene_triangle"][found]]
            assert as_fresh.tobytes() == want["changed"].tobytes(), what
        refitted = ctx.trace(rays, ordered=True)
        same_as_fresh(refitted, "after update_triangles")
        assert refitted.tobytes() != moved.tobytes() and refitted.tobytes() == ctx.trace(rays).tobytes()
        ctx.rebuild_trees(3)
        same_as_fresh(ctx.trace(rays, ordered=True), "after rebuild_trees")
        assert np.array_equal(ctx.occluded(rays, ordered=True), _found(want["changed"]).astype(np.uint32))
    finally:
        ctx.close()


# =====================================================================================================================
# 8. nothing else changes
# =====================================================================================================================
_CALLS = (1, 3, 8, 2, 8)


def _frame_context(kind):
    ctx = Context([0, 0]) if kind == "two-streams" else Context(0)
    if kind == "split-sorted":             # the trace kernel follows the frame's own sort, in the frame's own sort workspace
        ctx.set_pipeline(1), ctx.set_ray_sort(1)
    return ctx


@pytest.mark.parametrize("kind", ["single", "two-streams", "split-sorted"])
def test_ordered_queries_change_nothing_else(built, kind):
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
                    rays = _shuffled_pixel_rays(ctx, k)
                    traced = ctx.trace(rays, ordered=True)
                    assert np.array_equal(ctx.occluded(rays, ordered=True), _found(traced).astype(np.uint32))
                    assert len(ctx.ray_order(rays)[0]) == rays.size
            if ask:
                assert traced.tobytes() == ctx.trace(rays).tobytes() and _found(traced).sum() > 1000
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.ray_count(), ctx.pass_count(),
                            ctx.graph_captures(), ctx.read_guides().tobytes()))
            if kind == "split-sorted":
                assert ctx.pipeline() == 1
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "ray_count", "pass_count", "graph_captures", "guides"), *results):
        assert a == b, f"{kind}: {name} differs once ordered queries run between the render calls"


# =====================================================================================================================
# 9. hiprz_sort_u32_device
# =====================================================================================================================
@pytest.mark.parametrize("n", [1, 4096, 4097])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_the_sort_entry_point(sphere, bits, n):
    ctx = sphere[0]
    keys = np.random.default_rng(1000 * bits + n).integers(0, 2**bits, size=n, dtype=np.uint64).astype(np.uint32)
    keys[n // 2:] = keys[:n - n // 2]          # repeated keys: stability shows
    ctx.sync()
    d_keys, d_perm = _hiprt.DeviceBuffer.of(np.concatenate([keys, np.full(PAD, GUARD, np.uint32)])), _guarded(n, 1)
    try:
        assert ctx.lib.hiprz_sort_u32_device(ctx._ctx, d_keys.ptr, n, bits, d_perm.ptr, None) == _abi.OK
        ctx.sync()
        perm, left = d_perm.download((n + PAD,), np.uint32), d_keys.download((n + PAD,), np.uint32)
    finally:
        d_keys.free(), d_perm.free()
    assert (perm[n:] == GUARD).all() and (left[n:] == GUARD).all(), "a word behind n was written"
    assert np.array_equal(perm[:n], np.argsort(keys, kind="stable").astype(np.uint32))


def test_the_sort_entry_point_refuses(sphere):
    ctx = sphere[0]
    lib, c = ctx.lib, ctx._ctx
    ctx.sync()
    buf = _guarded(4, 1)
    try:
        assert lib.hiprz_sort_u32_device(None, buf.ptr, 4, 24, buf.ptr, None) == _abi.ERR_INVALID
        assert lib.hiprz_sort_u32_device(c, None, 4, 24, buf.ptr, None) == _abi.ERR_INVALID and b"null pointer" in lib.hiprz_last_error(c)
        assert lib.hiprz_sort_u32_device(c, buf.ptr, 4, 24, None, None) == _abi.ERR_INVALID
        for bits in (0, -1, 33):
            assert lib.hiprz_sort_u32_device(c, buf.ptr, 4, bits, buf.ptr, None) == _abi.ERR_INVALID and b"key_bits" in lib.hiprz_last_error(c), bits
        assert lib.hiprz_sort_u32_device(c, buf.ptr, 2**30 + 1, 24, buf.ptr, None) == _abi.ERR_INVALID and b"2^30" in lib.hiprz_last_error(c)
        assert lib.hiprz_sort_u32_device(c, buf.ptr, 0, 24, buf.ptr, None) == _abi.OK           # nothing is launched
        ctx.sync()
        assert (buf.download((4 + PAD,), np.uint32) == GUARD).all(), "a refused or empty sort wrote"
    finally:
        buf.free()


# =====================================================================================================================
# 10. refusals, an empty world
# =====================================================================================================================
def test_refusals_and_an_empty_world(built):
    ctx = _context(0)
    try:
        rays = query.rays([[0, 0, 0]], [[0, 0, 1]], 0.0, 1.0)
        with pytest.raises(HiprzError) as e:
            ctx.trace(rays, ordered=True)
        assert e.value.code == _abi.ERR_STATE and "before a scene" in str(e.value), e.value
        with pytest.raises(HiprzError) as e:
            ctx.ray_order(rays)
        assert e.value.code == _abi.ERR_STATE
        assert ctx.trace(rays[:0], ordered=True).shape == (0,)                         # n == 0: HIPRZ_OK without a view or a launch
        _upload(ctx, "slots")
        o = ctx.order()
        lib, h, p = o.lib, o._order, rays.ctypes.data           # (every call below is refused before a pointer is used)
        err = lambda: lib.hiprz_order_last_error(h)
        assert lib.hiprz_order_closest(h, None, 1, 0, p, None) == _abi.ERR_INVALID and b"null pointer" in err()
        assert lib.hiprz_order_closest(h, p, 1, 0, None, None) == _abi.ERR_INVALID and b"null pointer" in err()
        assert lib.hiprz_order_occluded(h, p, 1, 0, None, None) == _abi.ERR_INVALID
        assert lib.hiprz_order_closest_by(h, p, None, 1, 0, p, None) == _abi.ERR_INVALID and b"order_closest_by: null pointer" in err()
        assert lib.hiprz_order_occluded_by(h, p, None, 1, 0, p, None) == _abi.ERR_INVALID
        assert lib.hiprz_order_permutation(h, p, 1, 0, None, None, None) == _abi.ERR_INVALID and b"null pointer" in err()
        assert lib.hiprz_order_closest_host(h, p, 1, 0, None) == _abi.ERR_INVALID
        for flags in (2, 3, 0x80000000):
            assert lib.hiprz_order_closest(h, p, 1, flags, p, None) == _abi.ERR_INVALID and b"unknown flag" in err(), flags
            assert lib.hiprz_order_occluded_host(h, p, 1, flags, p) == _abi.ERR_INVALID and b"unknown flag" in err(), flags
            assert lib.hiprz_order_permutation(h, p, 1, flags, None, p, None) == _abi.ERR_INVALID
        for call in (lambda n: lib.hiprz_order_closest(h, p, n, 0, p, None), lambda n: lib.hiprz_order_occluded_by(h, p, p, n, 0, p, None),
                     lambda n: lib.hiprz_order_permutation(h, p, n, 0, None, p, None), lambda n: lib.hiprz_order_closest_host(h, p, n, 0, p)):
            assert call(2**30 + 1) == _abi.ERR_INVALID and b"2^30" in err()
        assert ctx.trace(rays, ordered=True).tobytes() == ctx.trace(rays).tobytes()
        # an empty world: every ray misses, nothing faults
        empty = GS._world(0)[0]
        GS._camera(empty)
        flat = flatten(empty)
        assert not len(flat.instances)
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(empty.camera))
        batch = _shuffled_pixel_rays(ctx, 3)
        hits = ctx.trace(batch, ordered=True)
        assert not _found(hits).any() and not (hits["flags"] & HIT_INVALID).any() and QR.misses_read_as_specified(hits, batch)
        assert hits.tobytes() == ctx.trace(batch).tobytes() and not ctx.occluded(batch, ordered=True).any()
        perm = ctx.ray_order(batch)[0]
        assert np.array_equal(np.sort(perm), np.arange(len(batch), dtype=np.uint32))
    finally:
        ctx.close()


# =====================================================================================================================
# 11. the C++ host
# =====================================================================================================================
@pytest.mark.parametrize("normalize", [0, 1])
def test_cpp_engine_casts_rays_in_order(built, tmp_path, normalize):
    exe = str(tmp_path / "order_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "order_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "sphere.json")
    scene_io.save_scene_json(scenes.textured_sphere_scene(48, 32, resolution=24, map_size=32), scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        rays = _shuffled_pixel_rays(ctx, 11)
        if normalize:
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
    assert r.returncode == 0 and "ORDER DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    out = open(tmp_path / "out.bin", "rb").read()
    n = len(rays)
    assert len(out) == n * (HIT + 4)
    assert out[:n * HIT] == want_hits.tobytes(), "Engine::castRays(ordered = true) differs from Context.trace"
    assert out[n * HIT:] == want_occ.tobytes(), "Engine::occluded(ordered = true) differs from Context.occluded"
