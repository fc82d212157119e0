"""Probe baking on the GPU (include/hiprz_probe.h: libhiprz_probe.so, Context.bake_probes / probe_samples / bake_probe_field).  The samples
of a probe are held to the gather library's own samples for the same points, table, seed and chart map (themselves held to the query's
hits by tests/test_gather_gpu.py), a record of either term to the numpy float32 restatement (tests/probe_reference.py) over the emitted
samples and over rays whose verdicts are Context.occluded's, bit for bit.  Trees 0 (reference) and 3 (device SAH).

THE WORLD is tests/gather_world.py's with its 64 x 48 atlas.  PROBES: 67 points of free space drawn from the box over the floor, with
random frame axes; one in the middle is spoiled.

  1 samples, gather  K in 16, 64, 128, S in 1, 3, n in 1, 5, 67: probe_samples == gather_samples in every byte; every record == the
                     restatement over those samples and the rays of bake_rays.  No ray is left out.
  2 light            K in 1, 16, 128; spot only, direct only, both, an empty range; with and without `base`, `out` aliasing `base` and not:
                     every record == the restatement over probe_reference.light_rays and Context.occluded's verdicts.
  3 known answers    a closed room whose source is 1.0: sh[0] exactly 1.0, K rays READ, sh[b] the table's own float32 mean of B_b; an empty
                     world: the same with the sky and K MISSED; lights without geometry: 0 shadowed; a probe inside a closed mesh: +0.
  4 meaning          E(n) of probes 1e-3 above floor points against bake_light + gather at those points, within the discrepancy of the
                     float64 estimators of both (same rays, K = 1024) plus the float32 summation bound.
  5 equality         the build that holds the sums in registers writes the bytes of the shipped one; bake_probe_field == its steps; a bake
                     after update_instances == a fresh context's.
  6 refusals, C++    in the header's order, n == 0, the host-pointer calls == the device-pointer calls; Engine::bakeProbes delivers the bytes
                     of Context.bake_probes, Engine::probeIrradiance is hiprz_probe_irradiance.

MEASURED ON MI355X: the first eleven cases in 4.1 s beside the session's build fixture (the twelfth, the C++ host, compiles a program),
slowest the two builds' comparison (2.7 s: it compiles the other build and starts two processes), every other case below 0.4 s.  Per tree, case 1: 30 368 samples byte-equal to the gather's, every record bit-equal to the restatement,
the mutants swap, b6 and order caught.  Case 2: 256, 4 081 and 32 637 shadow rays walked at K = 1, 16, 128 with both lights, 11, 181 and
1 446 shadowed.  Case 4: the device's E(n) within 1.7e-7 and its light + mean within 7e-8 of their float64 estimators."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bake_reference as BR
import gather_reference as GR
import gather_world as GW
import light_reference as LR
import probe_reference as PR
from rayzath_amd import _abi, _hiprt, atlas, bake, gather, probe, scene_io
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
SKY = (0.25, 0.5, 2.0)
N = 67
INVALID_WORD = np.array([probe.INVALID], np.uint32).view(F)[0]


def _context(tree=0, world=None):
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    world = GW.world() if world is None else world
    flat = flatten(world)
    ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
    return ctx, world, flat


def _probes(n=N, spoil=True):
    """n probes over the floor, the same ones every time; with `spoil` the middle one (of three or more) is invalid: its axis is 0"""
    rng = np.random.default_rng(7)
    out = bake.points(rng.uniform((-2.4, 0.1, -2.4), (2.4, 2.4, 2.4), size=(N, 3)), rng.normal(size=(N, 3)), NEAR, FAR)[:n].copy()
    if spoil and n >= 3:
        out["normal"][n // 2] = 0.0
    return out


def _charts():
    w = GW.world()
    return gather.chart_tables(GW.parts(w), len(w.instances))


def _source(seed=1):
    rng = np.random.default_rng(seed)
    source = np.zeros((H, W), gather.record_dtype)
    source["rgb"] = rng.uniform(0.0, 4.0, (H, W, 3))
    source["word"] = rng.integers(0, 100, (H, W))
    source["word"][rng.random((H, W)) < 1.0 / 11.0] = gather.INVALID
    return source


# =====================================================================================================================
# 1. the samples are the gather's; the gathered term is the restatement's
# =====================================================================================================================
@pytest.mark.parametrize("tree", TREES)
def test_samples_and_the_gathered_term(built, tree):
    ctx, world, flat = _context(tree)
    try:
        charts, source = _charts(), _source()
        rays_seen, caught = 0, {m: False for m in ("swap", "b6", "order")}
        for K in (16, 64, 128):
            for S in (1, 3):
                table = probe.sphere_directions(K, S)
                for n in (1, 5, N):
                    probes, seed = _probes(n), 20261021 + K
                    what = f"tree {tree} K {K} S {S} n {n}"
                    samples = ctx.probe_samples(probes, seed, table, charts)
                    want = ctx.gather_samples(probes, seed, table, charts)
                    assert samples.shape == (n, K) and samples.tobytes() == want.tobytes(), f"{what}: probe_samples differs from gather_samples"
                    rays = ctx.bake_rays(probes, seed, table)
                    assert rays.tobytes() == BR.rays(probes, table, seed).tobytes()
                    got = ctx.bake_probes(probes, source, W, H, None, None, None, seed, SKY, direct=False)
                    ref = PR.gather_records(probes, samples, rays, charts[1], source, W, H, SKY)
                    assert got.dtype == probe.sh_dtype and got.shape == (n,)
                    assert got.tobytes() == ref.tobytes(), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words of {got.view(np.uint32).size} differ from the restatement"
                    if n >= 3:
                        assert got["sh"][n // 2, 0, 3].tobytes() == INVALID_WORD.tobytes() and not got["sh"][n // 2, :, :3].view(np.uint32).any()
                        assert (samples["id"][n // 2] == gather.INVALID_RAY).all()
                    rays_seen += samples.size
                    if n == N:
                        counts = probe.words(got)[0][np.arange(n) != n // 2]
                        assert ((counts & 0xFFFF) > 0).any() and ((counts >> 16) > 0).all(), "probes over an open floor see the sky, and some of them a chart"
                        assert (samples["id"] == gather.BACK).any() and (samples["id"] == gather.UNMAPPED).any()
                        for m in caught:
                            caught[m] |= PR.gather_records(probes, samples, rays, charts[1], source, W, H, SKY, m).tobytes() != got.tobytes()
        assert all(caught.values()), caught
        print(f"tree {tree}: {rays_seen} samples byte-equal to the gather's, every record bit-equal to the restatement, mutants caught: {sorted(caught)}")
    finally:
        ctx.close()


# =====================================================================================================================
# 2. the light term
# =====================================================================================================================
RANGES = {"spot only": (0, None, 0, 0), "direct only": (0, 0, 0, None), "both": None, "empty": (1, 0, 1, 0)}


def _light_reference(ctx, flat, probes, table, seed, lights, base=None, mutant=None):
    rays, weights = PR.light_rays(probes, flat.spot_lights, flat.direct_lights, table, seed, lights, mutant)
    words = ctx.occluded(rays.reshape(-1)).reshape(rays.shape) if rays.size else np.zeros(rays.shape, np.uint32)
    spots, directs = LR.select(flat.spot_lights, flat.direct_lights, lights)
    return PR.light_records(probes, rays["direction"], weights, words, LR.colour_emission(spots, directs), base, mutant), words, weights


@pytest.mark.parametrize("K", [1, 16, 128])
def test_the_light_term(built, K):
    ctx, world, flat = _context(3)
    try:
        assert len(flat.spot_lights) == 1 and len(flat.direct_lights) == 1
        p = ctx.prober()
        probes, seed = _probes(), 5 + K
        rng = np.random.default_rng(K)
        base = np.zeros(N, probe.sh_dtype)
        base["sh"][..., :3] = rng.uniform(-1.0, 1.0, (N, 9, 3))
        base["sh"][:, 0, 3] = rng.integers(0, 2 ** 31, N).astype(np.uint32).view(F)
        base["sh"][:, 1:, 3] = 5.0                                        # of a base only sh[0].w is carried over
        base["sh"][11, 0, 3] = INVALID_WORD
        shadowed = walked = 0
        caught = {m: False for m in ("swap", "b6", "quarter", "cosine")}
        for S in (1, 3):
            table = LR.disk_table(K, S)
            p.set_samples(table)
            for name, lights in RANGES.items():
                what = f"K {K} S {S} {name}"
                ref, words, weights = _light_reference(ctx, flat, probes, table, seed, lights)
                got = p.light(probes, seed, lights)
                assert got.tobytes() == ref.tobytes(), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words differ from the restatement"
                ok = PR.valid(probes)
                assert not probe.words(got)[0][ok].any() and probe.words(got)[0][N // 2] == probe.INVALID
                if name == "empty":
                    assert not got["sh"][ok].view(np.uint32).any(), "no light selected: +0 and nothing shadowed"
                # with a base: the sum per component and the copied word; the host call aliases out and base on the device
                ref_based, _, _ = _light_reference(ctx, flat, probes, table, seed, lights, base)
                based = p.light(probes, seed, lights, base)
                assert based.tobytes() == ref_based.tobytes(), f"{what}: with a base"
                good = ok & (np.arange(N) != 11)
                assert based["sh"][good][..., :3].tobytes() == (base["sh"][good][..., :3] + got["sh"][good][..., :3]).tobytes()
                assert np.array_equal(probe.words(based)[0][good], probe.words(base)[0][good]) and np.array_equal(probe.words(based)[1][good], probe.words(got)[1][good])
                assert probe.words(based)[0][11] == probe.INVALID and not based["sh"][11, :, :3].view(np.uint32).any()
                assert not based["sh"][:, 2:, 3].view(np.uint32).any()
                # device pointers, out apart from base: the same bytes, and the base is left as it was
                ctx.sync()
                bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(base), _hiprt.DeviceBuffer(N * 144)]
                try:
                    p.light_device(bufs[0].ptr, N, bufs[2].ptr, seed, lights, bufs[1].ptr)
                    ctx.sync()
                    assert bufs[2].download((N,), probe.sh_dtype).tobytes() == based.tobytes() and bufs[1].download((N,), probe.sh_dtype).tobytes() == base.tobytes()
                finally:
                    for b in bufs:
                        b.free()
                if name == "both":
                    shadowed += int(probe.words(got)[1][ok].sum())
                    walked += int((weights > 0).sum())
                    assert np.array_equal(probe.words(got)[1][ok], ((words != 0) & (weights > 0)).sum((1, 2))[ok])
                    for m in caught:
                        caught[m] |= _light_reference(ctx, flat, probes, table, seed, lights, None, m)[0].tobytes() != got.tobytes()
        assert all(caught.values()), caught
        assert 0 < shadowed < walked, "some probes lie in the shadow of the cube or the wall, some do not"
        print(f"K {K}: {walked} shadow rays walked, {shadowed} shadowed; every record bit-equal to the restatement")
    finally:
        ctx.close()


# =====================================================================================================================
# 3. known answers
# =====================================================================================================================
def test_known_answers(built):
    rng = np.random.default_rng(4)
    probes = bake.points(rng.uniform(-0.4, 0.4, size=(21, 3)), rng.normal(size=(21, 3)), NEAR, FAR)
    probes["far"][10] = np.nan
    ok = np.arange(21) != 10
    room = World()
    grey = room.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    box = room.add(GW.inward_box())
    room.add(Instance(box, [grey], position=(0.1, -0.2, 0.05), rotation=(0.2, 0.4, 0.1), scale=(3.0, 2.0, 2.5), name="room"))
    room.camera = GW.world().camera
    ones = gather.records((1.0, 1.0, 1.0), (5, 7))
    for tree in TREES:
        ctx, _, _ = _context(tree, room)
        try:
            charts = gather.chart_tables([(0, atlas.charts(box))], 1)
            for K in (16, 64, 256):
                table = probe.sphere_directions(K, 3)
                got = ctx.bake_probes(probes, ones, 7, 5, charts, table, None, 9, SKY, direct=False)
                assert (probe.words(got)[0][ok] == K).all(), f"tree {tree} K {K}: not every ray of a closed room reads a texel"
                assert (got["sh"][ok][:, 0, :3] == 1.0).all() and probe.words(got)[0][10] == probe.INVALID
                directions = BR.rays(probes, table, 9)["direction"]
                want = PR.project(np.ones((21, K, 3), F), directions)
                assert got["sh"][ok][..., :3].tobytes() == want[ok].tobytes(), "sh[b] is the table's own float32 mean of B_b under the fixed order"
        finally:
            ctx.close()
    # a closed mesh seen from inside: back faces only
    solid = World()
    grey = solid.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    cube = solid.add(generate_cube())
    solid.add(Instance(cube, [grey], position=(0.1, -0.2, 0.05), rotation=(0.2, 0.4, 0.1), scale=(3.0, 2.0, 2.5), name="solid"))
    solid.camera = GW.world().camera
    ctx, _, _ = _context(3, solid)
    try:
        charts = gather.chart_tables([(0, atlas.charts(cube))], 1)
        got = ctx.bake_probes(probes, ones, 7, 5, charts, (64, 3), None, 9, SKY, direct=False)
        assert not got[ok].view(np.uint32).any(), "a probe all of whose rays hit back faces reads +0 and counts nothing"
        assert (ctx.probe_samples(probes, 9)[ok]["id"] == gather.BACK).all()
    finally:
        ctx.close()
    # an empty world, with and without lights
    ctx, _, flat = _context(0, GW.world(geometry=False))
    try:
        assert not len(flat.instances) and len(flat.spot_lights) + len(flat.direct_lights) == 2
        nothing = gather.chart_tables([], 0)
        for K in (16, 64, 256):
            table = probe.sphere_directions(K, 3)
            got = ctx.bake_probes(probes, ones, 7, 5, nothing, table, None, 9, SKY, direct=False)
            assert (probe.words(got)[0][ok] == K << 16).all() and got["sh"][ok][:, 0, :3].tobytes() == np.asarray(SKY, F).tobytes() * 20, f"K {K}: an empty world is not the sky"
            want = PR.project(np.broadcast_to(np.asarray(SKY, F), (21, K, 3)), BR.rays(probes, table, 9)["direction"])
            assert got["sh"][ok][..., :3].tobytes() == want[ok].tobytes()
        lit = ctx.bake_probes(probes, ones, 7, 5, None, None, (16, 3), 9, SKY)
        assert not probe.words(lit)[1][ok].any() and np.array_equal(probe.words(lit)[0], probe.words(got)[0]), "lights without geometry: nothing is shadowed"
        alone = ctx.prober().light(probes, 9)
        assert (alone["sh"][ok][:, 0, :3] > 0).all() and lit["sh"][ok][..., :3].tobytes() == (got["sh"][ok][..., :3] + alone["sh"][ok][..., :3]).tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 4. the meaning: E(n) of a probe just above a surface point is what a lightmap texel holds there
# =====================================================================================================================
K_MEANING = 1024
FLOOR_POINTS = [(-2.0, -2.0), (0.3, -1.9), (1.8, -0.7), (-0.9, 0.45), (2.1, 2.0), (-2.2, 1.7)]


def _region_source():
    """an atlas whose value depends on the chart's rectangle alone (floor, cube, wall: tests/gather_world.py RECTS), gutters included: a
    ray that lands a texel aside reads the same value in float32 and in float64"""
    source = np.zeros((H, W), gather.record_dtype)
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    left, low = (u < 0.5)[None, :], (v < 0.5)[:, None]
    source["rgb"] = np.where(left[..., None], (0.8, 0.7, 0.6), np.where((~left & low)[..., None], (0.9, 0.3, 0.2), (0.2, 0.4, 0.9)))
    return source


def _walk64(triangles, origin, direction, near, far):
    """the float64 closest hit within (near, far) of rays over the world's triangles: (instance (-1: none), triangle, bx, by, front)"""
    n = len(origin)
    best = np.asarray(far, np.float64) * np.ones(n)
    inst, tri_id, bx, by, front = np.full(n, -1), np.zeros(n, np.int64), np.zeros(n), np.zeros(n), np.zeros(n, bool)
    for i, tris in enumerate(triangles):
        for k, tri in enumerate(tris):
            t, b1, b2, det = GW.barycentrics(np.broadcast_to(tri, (n, 3, 3)), origin, direction)
            with np.errstate(invalid="ignore"):
                hit = (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t > near) & (t < best)
            best = np.where(hit, t, best)
            inst[hit], tri_id[hit], bx[hit], by[hit], front[hit] = i, k, b1[hit], b2[hit], (det > 0)[hit]
    return inst, tri_id, bx, by, front


def _radiance64(triangles, charts, source, rays, sky):
    """what every ray of `rays` ((n, K) query.ray_dtype) contributes by the gather's rule, walked and looked up in float64: (n, K, 3)"""
    base, uv = charts
    shape = rays.shape
    r = rays.reshape(-1)
    inst, tri, bx, by, front = _walk64(triangles, r["origin"].astype(np.float64), r["direction"].astype(np.float64), r["near"].astype(np.float64), r["far"].astype(np.float64))
    mapped = (inst >= 0) & front & (base[np.maximum(inst, 0)] != gather.NONE)
    c = uv[np.where(mapped, base[np.maximum(inst, 0)] + tri, 0)]
    b1 = (1.0 - bx) - by
    u, v = c["u1"] * b1 + c["u2"] * bx + c["u3"] * by, c["v1"] * b1 + c["v2"] * bx + c["v3"] * by
    x, y = np.clip(np.floor(u * W), 0, W - 1).astype(int), np.clip(np.floor(v * H), 0, H - 1).astype(int)
    L = np.where(mapped[:, None], source["rgb"][y, x].astype(np.float64), 0.0)
    L = np.where((inst < 0)[:, None], np.asarray(sky, np.float64), L)
    return L.reshape(shape + (3,))


def _shadowed64(triangles, position, near, w3, far):
    n, Ln, K = far.shape
    origin = np.broadcast_to(position[:, None, None, :], w3.shape).reshape(-1, 3)
    inst = _walk64(triangles, origin, w3.reshape(-1, 3), np.broadcast_to(near[:, None, None], far.shape).reshape(-1), far.reshape(-1))[0]
    return (inst >= 0).reshape(n, Ln, K)


def float64_estimators(K=K_MEANING, seed=3, sky=(0.05, 0.08, 0.12)):
    """Both sides of "THE MEANING" estimated in float64 on the host with the rays the device walks, for FLOOR_POINTS: (probes, surface points,
    source, E64, S64, eps_E, eps_S) — E(n) of the probes 1e-3 above the floor, light + mean of the floor points under them, and the float32
    summation bounds of either side: K * 2^-24 * mean|term| per sum (L * K terms for the lights), carried through the evaluation's weights,
    plus the evaluation's own ten roundings.  No device is asked anything."""
    world = GW.world()
    flat = flatten(world)
    triangles, charts, source = GW.world_triangles(world, flat), _charts(), _region_source()
    xz = np.array(FLOOR_POINTS)
    surface = bake.points(np.stack([xz[:, 0], np.zeros(len(xz)), xz[:, 1]], -1), (0.0, 1.0, 0.0), NEAR, FAR)
    probes = bake.points(np.stack([xz[:, 0], np.full(len(xz), 1e-3), xz[:, 1]], -1), (0.0, 1.0, 0.0), NEAR, FAR)
    normal = np.array([0.0, 1.0, 0.0])
    sphere, cosine, disk = PR.sphere_table(K, 1), BR.cosine_table(K, 1), LR.disk_table(K, 1)
    ce = LR.colour_emission(flat.spot_lights, flat.direct_lights, np.float64)
    # the probe
    rays = BR.rays(probes, sphere, seed)
    L = _radiance64(triangles, charts, source, rays, sky)
    terms = L[:, :, None, :] * PR.basis(rays["direction"].astype(np.float64))[:, :, :, None]
    w3, far, w, kept = PR.light_samples(probes, flat.spot_lights, flat.direct_lights, disk, seed, np.float64)
    occluded = _shadowed64(triangles, probes["position"].astype(np.float64), probes["near"].astype(np.float64), w3, far) & kept
    P = np.where((kept & ~occluded)[..., None], ce[None, :, None, :] * w[..., None] * 0.25, 0.0)
    sh64 = terms.mean(1) + PR.light_term(w3, w, occluded, ce, np.float64)
    E64 = PR.irradiance(sh64, normal)
    # the surface point
    srays = BR.rays(surface, cosine, seed)
    Ls = _radiance64(triangles, charts, source, srays, sky)
    sw3, sfar, sw, skept = LR.samples(surface, flat.spot_lights, flat.direct_lights, disk, seed, np.float64)
    socc = _shadowed64(triangles, surface["position"].astype(np.float64), surface["near"].astype(np.float64), sw3, sfar) & skept
    direct = np.where((skept & ~socc)[..., None], ce[None, :, None, :] * sw[..., None], 0.0)
    S64 = Ls.mean(1) + direct.sum((1, 2)) / K
    n_lights = len(ce)
    Bn = np.abs(PR.basis(normal)) * np.asarray(PR.WEIGHTS)
    magnitude = np.abs(terms).mean(1) + n_lights * (np.abs(P)[:, :, :, None, :] * np.abs(PR.basis(w3))[..., None]).sum((1, 2)) / K
    eps_E = K * 2.0 ** -24 * (Bn[None, :, None] * magnitude).sum(1) + 10 * 2.0 ** -24 * (Bn[None, :, None] * np.abs(sh64)).sum(1)
    eps_S = K * 2.0 ** -24 * (np.abs(Ls).mean(1) + n_lights * np.abs(direct).sum((1, 2)) / K)
    return probes, surface, source, E64, S64, eps_E, eps_S


def test_the_irradiance_of_a_probe_is_what_a_lightmap_texel_holds(built):
    """Both sides are first estimated in float64 on the host with the rays the device walks (K = 1024 for the directions and the disks), so
    the discrepancy D between E(n) and light + mean — the band-2 truncation of the clamped cosine (the lights' overshoot, whatever the
    probe sees below the surface's horizon) and the two tables' different sampling — is known before the device is looked at.  The
    device's two sides may then differ by D plus their float32 summation bounds, all taken from the float64 run.

    MEASURED in float64 (DESIGN.md §6 "Probe baking"): D is between 0.3 % and 4.8 % of the texel's largest component over the six floor
    points; this test prints both sides per point."""
    K, seed, sky = K_MEANING, 3, (0.05, 0.08, 0.12)
    probes, surface, source, E64, S64, eps_E, eps_S = float64_estimators(K, seed, sky)
    D = np.abs(E64 - S64)
    for i in range(len(FLOOR_POINTS)):
        print(f"floor point {FLOOR_POINTS[i]}: float64 E(n) {np.round(E64[i], 4)} light + mean {np.round(S64[i], 4)} |difference| {np.round(D[i], 4)} "
              f"({100 * D[i].max() / S64[i].max():.1f} % of the texel's largest component); float32 bounds {eps_E[i].max():.1e} and {eps_S[i].max():.1e}")
    assert (S64 > 0).all()
    normal = np.array([0.0, 1.0, 0.0], F)
    ctx, _, _ = _context(3)
    try:
        charts = _charts()
        sh = ctx.bake_probes(probes, source, W, H, charts, (K, 1), (K, 1), seed, sky)
        E = probe.irradiance(sh, normal).astype(np.float64)
        S = ctx.bake_light(surface, (K, 1), seed)["light"].astype(np.float64) + ctx.gather(surface, source, W, H, charts, (K, 1), seed, sky)["mean"].astype(np.float64)
    finally:
        ctx.close()
    for i in range(len(FLOOR_POINTS)):
        print(f"floor point {FLOOR_POINTS[i]}: device E(n) {np.round(E[i], 4)} light + mean {np.round(S[i], 4)}; |E - E64| {np.abs(E - E64)[i].max():.1e} |S - S64| {np.abs(S - S64)[i].max():.1e}")
    assert (np.abs(E - S) <= D + eps_E + eps_S).all(), (np.abs(E - S) - (D + eps_E + eps_S)).max()


# =====================================================================================================================
# 5. equality and freshness
# =====================================================================================================================
_CHILD = r"""
import sys
import numpy as np
import gather_world as GW
import test_probe_gpu as T
from rayzath_amd import probe
ctx, world, flat = T._context(3)
out = []
for K, LK in ((16, 1), (64, 16), (128, 128)):
    out.append(ctx.bake_probes(T._probes(), T._source(), T.W, T.H, T._charts(), (K, 3), (LK, 3), 77, T.SKY))
    out.append(ctx.bake_probes(T._probes(5), T._source(), T.W, T.H, None, None, None, 78, T.SKY, direct=False))
ctx.close()
np.save(sys.argv[1], np.concatenate(out))
print(probe.LIB_PATH)
"""


def test_both_placements_of_the_running_sums_write_the_same_bytes(built, tmp_path):
    """the shipped library against the other build of the same source (each kernel's sums the other way round: registers for LDS, LDS for
    registers), each in a process of its own through HIPRZ_PROBE_LIB"""
    make = open(os.path.join(CSRC, "Makefile")).read()
    cxxflags = re.search(r"^CXXFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(INC)", f"-I{os.path.join(ROOT, 'include')} -I{CSRC}")
    hipflags = re.search(r"^HIPFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    body = open(os.path.join(CSRC, "probe", "hiprz_probe.hip")).read()
    flipped = []
    for kernel in ("GATHER", "LIGHT"):
        in_lds = int(re.search(r"#define RZ_PROBE_%s_IN_LDS (\d)" % kernel, body).group(1))
        flipped += [f"-DRZ_PROBE_{kernel}_IN_LDS={1 - in_lds}", f"-DRZ_PROBE_{kernel}_WAVES={4 if in_lds else 5}"]
    other = str(tmp_path / "libhiprz_probe_other.so")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, *cxxflags.split(), *hipflags.split(), *flipped, "-Wno-undefined-inline", "-I", os.path.join(CSRC, "probe"),
                    "-shared", os.path.join(CSRC, "probe", "hiprz_probe.hip"), os.path.join(CSRC, "probe", "hiprz_probe_host.cpp"), "-L", CSRC, "-lhiprz", f"-Wl,-rpath,{CSRC}", "-o", other],
                   check=True, capture_output=True, timeout=600)
    results = {}
    for name, lib in (("shipped", None), ("other", other)):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
        env.pop("HIPRZ_PROBE_LIB", None)
        if lib:
            env["HIPRZ_PROBE_LIB"] = lib
        path = str(tmp_path / f"{name}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.strip().splitlines()[-1] == (lib or probe.LIB_PATH)
        results[name] = np.load(path)
    assert results["shipped"].dtype == probe.sh_dtype and len(results["shipped"]) == 3 * (N + 5)
    assert results["shipped"].tobytes() == results["other"].tobytes(), "the two placements of the running sums differ in some byte"
    assert np.abs(results["shipped"]["sh"][..., :3]).max() > 0


def test_a_probe_field_is_its_steps(built):
    seed, rings, directions, samples, sky = 4, 2, (64, 3), (16, 3), (0.01, 0.02, 0.03)
    ctx, world, flat = _context(3)
    try:
        parts = GW.parts(world)
        albedo = gather.records((0.7, 0.6, 0.5), (H, W))
        emission = gather.records((0.0, 0.0, 0.0), (H, W))
        emission["rgb"][2:20, 2:10] = (0.0, 0.5, 0.0)
        lo, hi, shape = (-2.0, 0.25, -2.0), (2.0, 2.25, 2.0), (5, 3, 5)          # a spacing of 1: every node is a float
        probes = probe.grid(lo, hi, shape)
        charts = gather.chart_tables(parts, len(flat.instances))
        for bounces in (1, 2):
            want = ctx.bake_bounce_atlas(parts, W, H, albedo, emission, bounces, directions, samples, seed, rings, sky, NEAR, FAR)
            got = ctx.bake_probe_field(parts, W, H, albedo, emission, bounces, probes, directions, samples, seed, rings, sky, NEAR, FAR, None, (64, 2))
            assert len(got) == 4 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), f"{bounces} bounces: the atlas of bake_probe_field is not bake_bounce_atlas's"
            # the steps one by one through the host: the source of the last gather, then both terms of the probes
            points, _ = ctx.atlas_points(parts, W, H, NEAR, FAR)
            a = ctx.atlas()
            direct = ctx.bake_light(points, samples, seed)
            indirect = None
            for _ in range(bounces):
                source = a.dilate(ctx.gatherer().compose(direct, indirect, albedo, emission, ctx.sync), rings)[0].reshape(H, W)
                indirect = ctx.gather(points, source, W, H, charts, directions, seed, sky)
            sh = ctx.bake_probes(probes, source, W, H, charts, (64, 2), samples, seed, sky)
            assert got[3].shape == shape and got[3].dtype == probe.sh_dtype and got[3].tobytes() == sh.tobytes(), f"{bounces} bounces: bake_probe_field differs from its steps"
        field = probe.Field(lo, hi, shape, got[3])
        up = field.irradiance(probes["position"].reshape(-1, 3), np.array([0.0, 1.0, 0.0], F))
        assert up.tobytes() == probe.irradiance(got[3].reshape(-1), np.array([0.0, 1.0, 0.0], F)).tobytes() and (up.max(-1) > 0).any()
        unlit = ctx.bake_probe_field(parts, W, H, albedo, emission, 1, probes, directions, samples, seed, rings, sky, NEAR, FAR, None, (64, 2), direct=False)[3]
        assert not probe.words(unlit)[1].any() and unlit.tobytes() == ctx.bake_probes(probes, a.dilate(ctx.gatherer().compose(direct, None, albedo, emission, ctx.sync), rings)[0].reshape(H, W),
                                                                                     W, H, charts, (64, 2), None, seed, sky, direct=False).tobytes()
    finally:
        ctx.close()


def test_a_bake_sees_update_instances(built):
    probes, source, seed = _probes(), _source(3), 13
    ctx, world, flat = _context(3)
    moved_world = GW.world(moved=True)
    moved = flatten(moved_world)
    try:
        before = ctx.bake_probes(probes, source, W, H, _charts(), (16, 3), (16, 3), seed, SKY)
        ctx.update_instances(moved.instances)
        after = ctx.bake_probes(probes, source, W, H, None, None, None, seed, SKY)
        assert after.tobytes() != before.tobytes(), "the bake does not see the moved cube"
    finally:
        ctx.close()
    fresh, _, _ = _context(3, moved_world)
    try:
        assert fresh.bake_probes(probes, source, W, H, _charts(), (16, 3), (16, 3), seed, SKY).tobytes() == after.tobytes(), "a bake after update_instances differs from a fresh context's"
    finally:
        fresh.close()


# =====================================================================================================================
# 6. refusals in their order, n == 0, host-pointer and device-pointer calls
# =====================================================================================================================
def test_refusals_and_the_two_kinds_of_calls(built):
    ctx = Context(0)
    try:
        probes, source = _probes(5), _source()
        p = ctx.prober()

        def refused(code, text, call, *args, **kwargs):
            with pytest.raises(HiprzError) as e:
                call(*args, **kwargs)
            assert e.value.code == code and text in str(e.value), (code, text, str(e.value))

        refused(_abi.ERR_STATE, "no direction table", p.gather, probes, source, W, H)
        refused(_abi.ERR_STATE, "no sample table", p.light, probes)
        p.set_directions((16, 2))
        refused(_abi.ERR_STATE, "no chart map", p.gather, probes, source, W, H)
        refused(_abi.ERR_STATE, "no chart map", ctx.probe_samples, probes)
        p.set_charts(*_charts())
        p.set_samples((4, 2))
        refused(_abi.ERR_INVALID, "W or H", p.gather_device, 16, 1, 16, 0, H, 16)
        assert p.gather(probes[:0], source, W, H).shape == (0,) and p.light(probes[:0]).shape == (0,), "n == 0 is OK without a scene"
        refused(_abi.ERR_STATE, "", p.gather, probes, source, W, H)            # no scene: whatever hiprz_device_view refuses
        refused(_abi.ERR_STATE, "", p.light, probes)
        refused(_abi.ERR_INVALID, "null pointer", p.gather_device, None, 1, 16, W, H, 16)
        refused(_abi.ERR_INVALID, "n*K is 2^31 or more", p.gather_device, 16, 2 ** 27, 16, W, H, 16)
        refused(_abi.ERR_INVALID, "n*K is 2^31 or more", p.light_device, 16, 2 ** 29, 16)
        with pytest.raises(HiprzError):
            p.set_directions(np.zeros((1, 16, 4), F))
        with pytest.raises(HiprzError):
            p.set_samples(np.full((1, 4, 2), 0.9, F))
        world = GW.world()
        flat = flatten(world)
        ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
        refused(_abi.ERR_INVALID, "the range", p.light, probes, 0, (2, 0, 0, 0))
        p.set_charts(*gather.chart_tables([], 2))
        refused(_abi.ERR_INVALID, "another number of instances", p.gather, probes, source, W, H)
        p.set_charts(*_charts())
        # the host-pointer calls are the device-pointer calls; records behind n are not written
        hosted = p.light(probes, 3, None, p.gather(probes, source, W, H, 3, SKY))
        assert hosted.tobytes() == ctx.bake_probes(probes, source, W, H, None, None, None, 3, SKY).tobytes()
        ctx.sync()
        guard = np.full((5 + 2) * 36, 0xABABABAB, np.uint32)
        bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(source), _hiprt.DeviceBuffer.of(guard)]
        try:
            p.bake_device(bufs[0].ptr, 5, bufs[1].ptr, W, H, bufs[2].ptr, 3, SKY)
            ctx.sync()
            back = bufs[2].download(guard.shape, np.uint32)
        finally:
            for b in bufs:
                b.free()
        assert back[:5 * 36].tobytes() == hosted.tobytes() and (back[5 * 36:] == 0xABABABAB).all()
    finally:
        ctx.close()


def test_cpp_engine_bakes_probes(built, tmp_path):
    exe = str(tmp_path / "probe_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "probe_delivery_check.cpp"), "-o", exe,
                    "-L", CSRC, "-lhiprz_host", "-lhiprz_probe", "-lhiprz", "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "probes.json")
    world = GW.world()
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    K, S, LK, LS, seed = 64, 3, 16, 4, 20261021
    parts, probes, source = GW.parts(world), _probes(), _source(9)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        assert len(loaded.flat.instances) == 4
        charts = gather.chart_tables(parts, 4)
        want = ctx.bake_probes(probes, source, W, H, charts, (K, S), (LK, LS), seed, SKY)
        gathered = ctx.bake_probes(probes, source, W, H, charts, (K, S), None, seed, SKY, direct=False)
    finally:
        ctx.close()
        loaded.close()
    assert probe.words(want)[0][N // 2] == probe.INVALID and probe.words(want)[1].any() and want.tobytes() != gathered.tobytes()
    files = {name: str(tmp_path / (name + ".bin")) for name in ("probes", "source", "out")}
    probes.tofile(files["probes"]), source.tofile(files["source"])
    part_args = []
    for instance, tris in parts:
        path = str(tmp_path / f"charts{instance}.bin")
        tris.tofile(path)
        part_args += [str(instance), path]
    r = subprocess.run([exe, scene_path, files["probes"], files["source"], str(W), str(H), files["out"], str(K), str(S), str(LK), str(LS), str(seed)] + part_args,
                       capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "PROBE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(files["out"], "rb").read() == want.tobytes(), "Engine::bakeProbes differs from Context.bake_probes"
    assert open(files["out"] + ".gathered", "rb").read() == gathered.tobytes(), "Engine::bakeProbes without the light term differs from Context.bake_probes"
