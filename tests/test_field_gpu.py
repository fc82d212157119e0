"""Probe fields on the GPU (include/hiprz_field.h: libhiprz_field.so, Context.bake_visibility / lookup_field / bake_probe_field(visibility=)).
A visibility record is held to the numpy float32 restatement (tests/field_reference.py) over the rays of Context.bake_rays and the hits of
Context.trace, a lookup result to the restatement over the same records, bit for bit.  Trees 0 (reference) and 3 (device SAH).

THE WORLD is tests/gather_world.py's.  PROBES: tests/test_probe_gpu.py's 67 points of free space with random frame axes, the middle one
spoiled.

  1 visibility       K in 64 (one round), 128 (the order across rounds), S in 1, 3, n in 1, 5, 67: every record == the restatement, the
                     words == the flag counts, records past n untouched, every mutant caught.
  2 known answers    a closed room: K front hits, no miss, every mean <= reach; an empty world: K misses, every mean within
                     (2K + 2) 2^-24 reach of reach; a probe inside a closed cube: K back hits.
  3 lookup           random records, no scene uploaded; grids (3, 2, 3), (2, 1, 1), (1, 1, 1); 257 points inside, outside, on nodes, a
                     NaN, a zero normal; with and without visibility; invalid probes, a probe inside geometry, a dead cell; == the
                     restatement in every byte, the plain lookup within 1e-5 relative of probe.Field.irradiance; every mutant caught.
  4 two rooms        baked end to end: the plain blend leaks >= 0.15, the weighted one <= 1/100 of it; inside a room both agree to 1e-3.
  5 equality         bake_probe_field(visibility=) == its steps; a bake after update_instances == a fresh context's; host-pointer ==
                     device-pointer calls; the refusals in the header's order; the C++ Engine delivers Python's bytes.

MEASURED ON MI355X: the twelve cases in 1.9 s beside the session's build fixture.  Per tree, case 1: 28 032 rays, 2 989 hits capped at the
reach, every record bit-equal to the restatement, the three mutants caught.  Case 4, both trees alike: plain 0.19997 and 0.34995, weighted
9.04e-6 and 4.88e-5 at K = 64, 2.36e-6 and 2.82e-5 at K = 256 (ratios 1.2e-5 .. 1.4e-4 against the bar of 1/100)."""
import os
import subprocess

import numpy as np
import pytest

import bake_reference as BR
import field_reference as FR
import gather_world as GW
from rayzath_amd import _abi, _hiprt, atlas, bake, field, gather, probe, scene_io
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context
from rayzath_amd.scene import Instance, Material, World, camera_struct, flatten, generate_cube

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
NEAR, FAR = 1e-3, 1e3
F = np.float32
W, H = GW.W, GW.H
N = 67
REACH = 2.0          # below the world's size: some hits lie beyond it and are capped


def _context(tree=0, world=None):
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    world = GW.world() if world is None else world
    flat = flatten(world)
    ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
    return ctx, world, flat


def _probes(n=N, spoil=True):
    """tests/test_probe_gpu.py's probes: n points over the floor, the same ones every time; with `spoil` the middle one is invalid"""
    rng = np.random.default_rng(7)
    out = bake.points(rng.uniform((-2.4, 0.1, -2.4), (2.4, 2.4, 2.4), size=(N, 3)), rng.normal(size=(N, 3)), NEAR, FAR)[:n].copy()
    if spoil and n >= 3:
        out["normal"][n // 2] = 0.0
    return out


# =====================================================================================================================
# 1. a visibility record is the restatement's over the device's own rays and hits
# =====================================================================================================================
@pytest.mark.parametrize("tree", TREES)
def test_visibility_bit_for_bit(built, tree):
    ctx, world, flat = _context(tree)
    try:
        caught = {m: False for m in FR.VIS_MUTANTS}
        rays_seen = capped = 0
        for K in (64, 128):
            for S in (1, 3):
                table = probe.sphere_directions(K, S)
                for n in (1, 5, N):
                    probes, seed = _probes(n), 20261021 + K
                    what = f"tree {tree} K {K} S {S} n {n}"
                    rays = ctx.bake_rays(probes, seed, table)
                    assert rays.tobytes() == BR.rays(probes, table, seed).tobytes()
                    hits = ctx.trace(rays)
                    got = ctx.bake_visibility(probes, table, seed, REACH)
                    ref = FR.visibility_records(probes, rays, hits, REACH)
                    assert got.dtype == field.vis_dtype and got.shape == (n,)
                    assert got.tobytes() == ref.tobytes(), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words of {got.view(np.uint32).size} differ from the restatement"
                    ok = BR.valid(probes)
                    found = (hits["flags"] & 1) != 0
                    front = found & ((hits["flags"] & 2) != 0)
                    assert np.array_equal(got["words"][ok], np.stack([front.sum(1), (found & ~front).sum(1), (~found).sum(1), np.full(n, K)], -1)[ok]), f"{what}: the words are not the flag counts"
                    if n >= 3:
                        assert got["words"][n // 2].tolist() == [0, 0, 0, field.INVALID] and not got["moments"][n // 2].view(np.uint32).any()
                    rays_seen += rays.size
                    if n == N:
                        capped += int((found & (hits["t"] > REACH)).sum())
                        assert front.any() and (found & ~front).any() and (~found[ok]).any(), "the probes see fronts, backs and the sky"
                        for m in caught:
                            caught[m] |= FR.visibility_records(probes, rays, hits, REACH, m).tobytes() != got.tobytes()
                        # records past n are untouched: the device-pointer call into a guarded buffer
                        ctx.sync()
                        guard = np.full((n + 2) * 132, 0xABABABAB, np.uint32)
                        bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(guard)]
                        try:
                            ctx.fielder().visibility_device(bufs[0].ptr, n, bufs[1].ptr, seed, REACH)
                            ctx.sync()
                            back = bufs[1].download(guard.shape, np.uint32)
                        finally:
                            for b in bufs:
                                b.free()
                        assert back[:n * 132].tobytes() == got.tobytes() and (back[n * 132:] == 0xABABABAB).all(), f"{what}: the device-pointer call"
        assert all(caught.values()), caught
        assert capped > 0, "no hit beyond the reach: the cap is not exercised"
        print(f"tree {tree}: {rays_seen} rays, {capped} hits capped at the reach, every record bit-equal to the restatement, mutants caught: {sorted(caught)}")
    finally:
        ctx.close()


# =====================================================================================================================
# 2. known answers
# =====================================================================================================================
def test_known_answers(built):
    rng = np.random.default_rng(4)
    probes = bake.points(rng.uniform(-0.4, 0.4, size=(21, 3)), rng.normal(size=(21, 3)), NEAR, FAR)
    probes["far"][10] = np.nan
    ok = np.arange(21) != 10
    placed = dict(position=(0.1, -0.2, 0.05), rotation=(0.2, 0.4, 0.1), scale=(3.0, 2.0, 2.5))
    reach = 2.5
    for mesh, column, name in ((GW.inward_box(), 0, "room"), (generate_cube(), 1, "solid")):
        w = World()
        grey = w.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
        w.add(Instance(w.add(mesh), [grey], name=name, **placed))
        w.camera = GW.world().camera
        for tree in TREES:
            ctx, _, _ = _context(tree, w)
            try:
                for K in (64, 256):
                    got = ctx.bake_visibility(probes, (K, 3), 9, reach)
                    assert (got["words"][ok, column] == K).all() and (got["words"][ok, 3] == K).all(), f"{name} tree {tree} K {K}: not every ray hits the {('front', 'back')[column]} of a closed mesh"
                    assert not got["words"][ok, 2].any() and not got["words"][ok, 1 - column].any()
                    assert (got["moments"][ok, :, 0] <= reach).all() and (got["moments"][ok, :, 0] > 0).all()
                    assert got["words"][10].tolist() == [0, 0, 0, field.INVALID]
            finally:
                ctx.close()
    ctx, _, flat = _context(0, GW.world(geometry=False))
    try:
        assert not len(flat.instances)
        for K in (64, 256):
            got = ctx.bake_visibility(probes, (K, 3), 9, reach)
            assert (got["words"][ok] == (0, 0, K, K)).all(), f"K {K}: an empty world is not all misses"
            bound = (2 * K + 2) * 2.0 ** -24 * reach          # two K-term float32 sums and one division
            assert (np.abs(got["moments"][ok, :, 0].astype(np.float64) - reach) <= bound).all(), np.abs(got["moments"][ok, :, 0] - reach).max()
    finally:
        ctx.close()


# =====================================================================================================================
# 3. the lookup, with no scene uploaded
# =====================================================================================================================
LO, HI = (-1.0, 0.0, 0.5), (1.0, 1.0, 2.5)


def _field_of(rng, shape):
    n = int(np.prod(shape))
    hi = [LO[a] if shape[a] == 1 else HI[a] for a in range(3)]
    probes = probe.grid(LO, hi, shape)
    sh = np.zeros(n, probe.sh_dtype)
    sh["sh"][:, 0, :3] = rng.uniform(1.0, 2.0, (n, 3))                 # band 0 of the order of 1, the others small: E(n) stays away from 0,
    sh["sh"][:, 1:, :3] = rng.uniform(-0.05, 0.05, (n, 8, 3))          # which a RELATIVE comparison with probe.Field needs
    sh["sh"][:, :, 3] = rng.integers(0, 2 ** 31, (n, 9)).astype(np.uint32).view(F)
    vis = np.zeros(n, field.vis_dtype)
    mean = rng.uniform(0.2, 1.5, (n, 64)).astype(F)
    vis["moments"][..., 0], vis["moments"][..., 1] = mean, mean * mean + rng.uniform(0.0, 0.2, (n, 64)).astype(F)
    vis["words"][:] = (60, 1, 3, 64)
    return field.grid_of(LO, hi, shape), probes, hi, sh, vis


def _points(rng, probes):
    flat = probes.reshape(-1)
    pos = rng.uniform((-1.6, -0.6, -0.1), (1.6, 1.6, 3.1), (257, 3))                  # inside and outside (clamped)
    pos[:120] = rng.uniform(LO, HI, (120, 3))
    pos[200:200 + min(len(flat), 40)] = flat["position"][:40]                          # exactly on nodes ...
    pos[240] = flat["position"][-1]                                                    # ... the last one included
    points = bake.points(pos, BR.normalized(rng.normal(size=(257, 3))))
    points["position"][250, 1] = np.nan
    points["normal"][251] = 0.0
    points["normal"][252] *= 1.2                                                       # not a unit normal
    return points


@pytest.mark.parametrize("shape", [(3, 2, 3), (2, 1, 1), (1, 1, 1)])
def test_lookup_bit_for_bit_without_a_scene(built, shape):
    rng = np.random.default_rng(sum(shape))
    grid, probes, hi, sh, vis = _field_of(rng, shape)
    n = len(sh)
    if n > 4:
        sh["sh"][n - 1, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]        # one invalid probe
        vis["words"][3, 3] = field.INVALID                                             # one whose visibility record is invalid
    if n > 1:
        vis["words"][n // 2, 1] = 9                                                    # one inside geometry: back > max_back
    points = _points(rng, probes)
    params = field.params(bias=0.02, max_back=4)
    ctx = Context(0)
    try:
        caught = {m: False for m in FR.LOOKUP_MUTANTS}
        for v in (None, vis):
            what = f"grid {shape} {'with' if v is not None else 'without'} visibility"
            got = ctx.lookup_field(grid, probes, sh, points, v, params)
            ref = FR.lookup(grid, probes, sh, v, params, points)
            assert got.dtype == field.result_dtype and got.shape == (257,)
            assert got.tobytes() == ref.tobytes(), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words differ from the restatement"
            for bad in (250, 251, 252):
                assert got["word"][bad] == field.INVALID and not got["rgb"][bad].view(np.uint32).any()
            good = got["word"] != field.INVALID
            assert good.sum() >= 200 and (got["word"][good] >= 1).all() and (got["word"][good] <= 8).all()
            # the device-pointer call gives the same bytes
            assert ctx.fielder().lookup_through_device(grid, probes, sh, points, v, params, ctx.sync).tobytes() == got.tobytes(), f"{what}: device pointers"
            if v is None:
                want = probe.Field(LO, hi, shape, sh).irradiance(points["position"][good], points["normal"][good])
                assert (np.abs(got["rgb"][good] - want) <= 1e-5 * np.abs(want)).all(), f"{what}: {np.abs(got['rgb'][good] / want - 1).max():.2e} from probe.Field.irradiance"
            else:
                for m in caught:
                    caught[m] |= FR.lookup(grid, probes, sh, v, params, points, m).tobytes() != got.tobytes()
        if shape == (3, 2, 3):
            assert all(caught.values()), caught
            # a cell whose eight probes are all invalid reads INVALID, its neighbours do not
            dead = sh.copy().reshape(shape)
            dead["sh"][:2, :, :2, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]
            inside = bake.points([(-0.5, 0.5, 1.0), (-0.9, 0.1, 0.6), (0.5, 0.5, 1.0), (-0.5, 0.5, 2.0)], (0.0, 1.0, 0.0))
            for v in (None, vis):
                got = ctx.lookup_field(grid, probes, dead, inside, v, params)
                assert got.tobytes() == FR.lookup(grid, probes, dead, v, params, inside).tobytes()
                assert (got["word"][:2] == field.INVALID).all() and not got["rgb"][:2].view(np.uint32).any() and (got["word"][2:] != field.INVALID).all()
    finally:
        ctx.close()


# =====================================================================================================================
# 4. the two rooms, baked end to end
# =====================================================================================================================
def _two_room_world():
    w = World()
    grey = w.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    box = w.add(GW.inward_box())
    for k, (lo, hi) in enumerate(FR.ROOMS):
        lo, hi = np.asarray(lo), np.asarray(hi)
        w.add(Instance(box, [grey], position=tuple((lo + hi) / 2), scale=tuple(hi - lo), name=f"room {k}"))
    w.camera = GW.world().camera
    parts = []
    for k, (u0, u1) in enumerate(((0.05, 0.45), (0.55, 0.95))):          # a chart rectangle per room: the left and the right half of the atlas
        tris = atlas.charts(box)
        for c in (1, 2, 3):
            tris[f"u{c}"], tris[f"v{c}"] = F(u0) + F(u1 - u0) * tris[f"u{c}"], F(0.1) + F(0.8) * tris[f"v{c}"]
        parts.append((k, tris))
    source = gather.records((0.0, 0.0, 0.0), (8, 16))
    source["rgb"][:, :8] = 1.0                                           # the first room's half holds 1, gutters included
    return w, parts, source


@pytest.mark.parametrize("tree", TREES)
def test_the_two_rooms_end_to_end(built, tree):
    world, parts, source = _two_room_world()
    ctx, _, flat = _context(tree, world)
    try:
        probes = probe.grid(FR.ROOM_LO, FR.ROOM_HI, FR.ROOM_SHAPE, near=NEAR, far=FAR)
        grid = field.grid_of(FR.ROOM_LO, FR.ROOM_HI, FR.ROOM_SHAPE)
        sh = ctx.bake_probes(probes, source, 16, 8, gather.chart_tables(parts, 2), (64, 1), None, 0, direct=False)
        lit = probes["position"][..., 0] < 0
        assert (probe.words(sh)[0] == 64).all(), "every ray of a probe in a closed room reads a texel"
        assert (sh["sh"][lit][:, 0, :3] == 1.0).all() and not sh["sh"][~lit][..., :3].any()
        leak = bake.points(FR.LEAK_POINTS, (0.0, 1.0, 0.0))
        inside = bake.points([(-1.0, 1.0, 0.0), (-1.2, 0.8, 0.3), (1.0, 1.0, 0.0), (1.3, 1.2, -0.2)], (0.0, 1.0, 0.0))
        for K in (64, 256):
            vis = ctx.bake_visibility(probes, (K, 1), 0, 4.0)
            assert (vis["words"] == (K, 0, 0, K)).all()
            plain = ctx.lookup_field(grid, probes, sh, leak)["rgb"][:, 0]
            weighted = ctx.lookup_field(grid, probes, sh, leak, vis, field.params(bias=0.0))["rgb"][:, 0]
            for i, p in enumerate(FR.LEAK_POINTS):
                print(f"tree {tree} K {K} point {p}: plain {plain[i]:.6f} weighted {weighted[i]:.3e} ratio {weighted[i] / plain[i]:.3e}")
            assert (plain >= 0.15).all(), "the plain blend leaks the lit room's light through the wall"
            assert (weighted <= plain / 100.0).all(), "the weighted blend leaks more than 1/100 of the plain one"
            both = [ctx.lookup_field(grid, probes, sh, inside, v)["rgb"] for v in (None, vis)]
            assert np.abs(both[0] - both[1]).max() <= 1e-3, "inside a room, away from the wall, the two blends differ"
            assert (both[0][:2] > 0.9).all() and not both[0][2:].any()
    finally:
        ctx.close()


# =====================================================================================================================
# 5. equality and delivery
# =====================================================================================================================
def test_a_probe_field_with_visibility_is_its_steps(built):
    seed, rings, directions, samples, sky = 4, 2, (64, 3), (16, 3), (0.01, 0.02, 0.03)
    ctx, world, flat = _context(3)
    try:
        parts = GW.parts(world)
        albedo = gather.records((0.7, 0.6, 0.5), (H, W))
        emission = gather.records((0.0, 0.0, 0.0), (H, W))
        emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)
        probes = probe.grid((-2.0, 0.25, -2.0), (2.0, 2.25, 2.0), (5, 3, 5))
        args = (parts, W, H, albedo, emission, 1, probes, directions, samples, seed, rings, sky, NEAR, FAR, None, (64, 2))
        want = ctx.bake_probe_field(*args)
        vis = ctx.bake_visibility(probes, (64, 2), seed, REACH)
        got = ctx.bake_probe_field(*args, visibility=REACH)
        assert len(want) == 4 and len(got) == 5
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:4], want)), "the first four items change with visibility="
        assert got[4].shape == (5, 3, 5) and got[4].dtype == field.vis_dtype and got[4].tobytes() == vis.tobytes(), "bake_probe_field(visibility=) differs from bake_visibility"
        assert (vis["words"][..., 3] == 64).all() and vis["words"][..., 0].any()
    finally:
        ctx.close()


def test_a_bake_sees_update_instances(built):
    probes, seed = _probes(), 13
    ctx, world, flat = _context(3)
    moved_world = GW.world(moved=True)
    try:
        before = ctx.bake_visibility(probes, (64, 3), seed, REACH)
        ctx.update_instances(flatten(moved_world).instances)
        after = ctx.bake_visibility(probes, None, seed, REACH)
        assert after.tobytes() != before.tobytes(), "the bake does not see the moved cube"
    finally:
        ctx.close()
    fresh, _, _ = _context(3, moved_world)
    try:
        assert fresh.bake_visibility(probes, (64, 3), seed, REACH).tobytes() == after.tobytes(), "a bake after update_instances differs from a fresh context's"
    finally:
        fresh.close()


def test_refusals_in_the_headers_order(built):
    ctx = Context(0)
    try:
        probes = _probes(5)
        f = ctx.fielder()
        dev = 16          # a device address that is never read: every call below is refused or empty

        def refused(code, text, call, *args, **kwargs):
            with pytest.raises(HiprzError) as e:
                call(*args, **kwargs)
            assert e.value.code == code and text in str(e.value), (code, text, str(e.value))

        refused(_abi.ERR_INVALID, "null pointer", f.visibility_device, None, 1, dev, 0, 1.0)
        refused(_abi.ERR_STATE, "no direction table", f.visibility, probes, 0, 1.0)
        with pytest.raises(HiprzError):
            f.set_directions(probe.sphere_directions(32, 2))                          # K < 64
        with pytest.raises(ValueError):
            f.set_directions((16, 2))
        with pytest.raises(HiprzError):
            f.set_directions(np.zeros((1, 64, 4), F))
        refused(_abi.ERR_STATE, "no direction table", f.visibility, probes, 0, 1.0)  # what was set before stays: nothing
        f.set_directions((64, 2))
        refused(_abi.ERR_INVALID, "n*K is 2^31 or more", f.visibility_device, dev, 2 ** 25, dev, 0, np.nan)
        for reach in (0.0, -1.0, np.nan, np.inf):
            refused(_abi.ERR_INVALID, "reach", f.visibility, probes, 0, reach)
        assert f.visibility(probes[:0], 0, 1.0).shape == (0,), "n == 0 is OK without a scene"
        refused(_abi.ERR_STATE, "", f.visibility, probes, 0, 1.0)                     # no scene: whatever hiprz_device_view refuses
        # the lookup: a null pointer, then the grid, then the params, then m
        rng = np.random.default_rng(2)
        grid, fprobes, hi, sh, vis = _field_of(rng, (3, 2, 3))
        bad_grid, bad_params = grid.copy(), field.params().copy()
        bad_grid["step"][1], bad_params["bias"] = 0.0, -1.0
        refused(_abi.ERR_INVALID, "null pointer", f.lookup_device, bad_grid, None, dev, None, 18, dev, 1, dev, bad_params)
        refused(_abi.ERR_INVALID, "grid step", f.lookup_device, bad_grid, dev, dev, None, 18, dev, 1, dev, bad_params)
        refused(_abi.ERR_INVALID, "do not multiply", f.lookup_device, grid, dev, dev, None, 17, dev, 1, dev, bad_params)
        refused(_abi.ERR_INVALID, "bias", f.lookup_device, grid, dev, dev, None, 18, dev, 2 ** 31, dev, bad_params)
        refused(_abi.ERR_INVALID, "2^31 points", f.lookup_device, grid, dev, dev, None, 18, dev, 2 ** 31, dev)
        assert ctx.lookup_field(grid, fprobes, sh, bake.points(np.zeros((0, 3)), (0.0, 1.0, 0.0)), vis).shape == (0,)
    finally:
        ctx.close()


def test_cpp_engine_bakes_and_looks_up(built, tmp_path):
    exe = str(tmp_path / "field_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "field_delivery_check.cpp"), "-o", exe,
                    "-L", CSRC, "-lhiprz_host", "-lhiprz_field", "-lhiprz", "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "field.json")
    world = GW.world()
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, seed, reach, bias, max_back = 128, 3, 20261021, REACH, 0.02, 40
    lo, hi, shape = (-2.0, 0.25, -2.0), (2.0, 2.25, 2.0), (5, 3, 5)
    probes = probe.grid(lo, hi, shape, near=NEAR, far=FAR)
    probes["normal"][2, 1, 2] = 0.0
    grid = field.grid_of(lo, hi, shape)
    rng = np.random.default_rng(8)
    sh = _field_of(rng, (5, 3, 5))[3]
    points = bake.points(rng.uniform((-2.5, 0.0, -2.5), (2.5, 2.5, 2.5), (300, 3)), BR.normalized(rng.normal(size=(300, 3))))
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        vis = ctx.bake_visibility(probes, (K, S), seed, reach)
        params = field.params(bias=bias, max_back=max_back)
        weighted, plain = ctx.lookup_field(grid, probes, sh, points, vis, params), ctx.lookup_field(grid, probes, sh, points, None, params)
    finally:
        ctx.close()
        loaded.close()
    assert vis["words"][2, 1, 2, 3] == field.INVALID and weighted.tobytes() != plain.tobytes()
    files = {name: str(tmp_path / (name + ".bin")) for name in ("probes", "grid", "sh", "points", "out")}
    probes.tofile(files["probes"]), grid.tofile(files["grid"]), sh.tofile(files["sh"]), points.tofile(files["points"])
    r = subprocess.run([exe, scene_path, files["probes"], files["grid"], files["sh"], files["points"], files["out"], str(K), str(S), str(seed), repr(reach), repr(bias), str(max_back)],
                       capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "FIELD DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(files["out"], "rb").read() == vis.tobytes(), "Engine::bakeVisibility differs from Context.bake_visibility"
    assert open(files["out"] + ".lookup", "rb").read() == weighted.tobytes(), "Engine::lookupField differs from Context.lookup_field"
    assert open(files["out"] + ".plain", "rb").read() == plain.tobytes(), "Engine::lookupField without visibility differs from Context.lookup_field"
