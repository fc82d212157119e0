"""The CPU oracle's CUDA-compat mode (rzo_render_pass_mode, oracle/rz_oracle.c) on its own, no GPU: the texture fetch of the CUDA engine
against a numpy restatement at the edges, the analytic micro-scenes of test_cuda_compat_gpu.py against the same analytic expectations the
GPU meets there, flags that no scene element can trigger against the default mode bit for bit, and the grouping and early-out of the
coloured shadow mask (cuda_bvh.cuh:172-232, cuda_instance.cuh:92-164) through the texel-fetch counter."""
import math
import zlib

import numpy as np
import pytest

import oracle
from compat_common import compat_showcase, fetch_numpy, open_sky, fog_scene, map_panel, panel_hits, quad, sample_numpy, shadow_scene, slab_scene
from rayzath_amd import scenes
from rayzath_amd.engine import (COMPAT_BEER_LAMBERT, COMPAT_FILTERING, COMPAT_SCATTERING, COMPAT_SHADOW_COLOR, COMPAT_TEXTURE_MULT,
                                LightSampling, RenderConfig, Tracing)
from rayzath_amd.scene import Camera, Instance, Material, Mesh, SpotLight, TextureBuffer, World, camera_struct, flatten

FILTERS = ["point", "linear"]
ADDRESS_MODES = ["wrap", "clamp", "mirror", "border"]


def _oracle(world, flags, passes, max_depth, samples=(1, 1), counted=False):
    flat, cam = flatten(world), camera_struct(world.camera)
    ref = oracle.OracleRenderer(flat, cam, RenderConfig(LightSampling(*samples), Tracing(max_depth, passes)).struct(), mode=flags)
    first = ref.render(1, counted=counted)
    ref.render(passes - 1)
    out = ref.accum, ref.depth, ref.state, first
    ref.close()
    return out


# ---- TextureBuffer::fetch (cuda_buffer.cuh:427-438) ----
def _texture_world(bitmaps, **sampling):
    world = World()
    for i, bm in enumerate(bitmaps):
        world.add(Material((255, 255, 255, 255), texture=TextureBuffer(bm, **sampling), name=f"m{i}"))
    world.add(Instance(world.add(Mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)])), [world.materials[-1]], name="anchor"))
    world.camera = Camera(resolution=(4, 4))
    return flatten(world)


def _bitmaps(rng, h, w):
    return [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8),
            rng.uniform(-3.0, 7.0, size=(h, w)).astype(np.float32)]


_EDGE = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1e-7, -1e-7, 1 - 2 ** -24, 0.999, 7.3, -7.3, 123.456, -123.456, 1e4, -1e4,
                  3e7, -3e7, 1e9, -1e9, 5e12, -5e12, 3e38, -3e38], np.float32)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 2), (8, 8)])
@pytest.mark.parametrize("filter_mode", FILTERS)
@pytest.mark.parametrize("address_mode", ADDRESS_MODES)
@pytest.mark.parametrize("transform", ["identity", "rotated"])
def test_compat_fetch_equals_the_numpy_restatement(shape, filter_mode, address_mode, transform):
    """Every filter x address mode x texel kind, 1x1, odd and even maps; texcoords exactly 0 and 1, negative, just inside / outside,
    far outside [0, 1] up to 3e38 (clamped at 2^30 texels, D4), under the identity and under rotation + translation + a negative scale."""
    rng = np.random.default_rng(zlib.crc32(repr((shape, filter_mode, address_mode, transform)).encode()))
    sampling = dict(filter_mode=filter_mode, address_mode=address_mode)
    if transform == "rotated":
        sampling.update(scale=(2.5, -1.75), rotation=0.7, translation=(0.3, -1.2))
    flat = _texture_world(_bitmaps(rng, *shape), **sampling)
    grid_u, grid_v = np.meshgrid(_EDGE, _EDGE)
    rand = rng.uniform(-3.0, 4.0, size=(2, 300)).astype(np.float32)
    u = np.concatenate([grid_u.ravel(), rand[0]])
    v = np.concatenate([grid_v.ravel(), rand[1]])
    for tex in range(3):
        got, fetches = oracle.compat_fetch(flat, tex, u, v)
        want = fetch_numpy(flat, tex, u, v)
        assert fetches == u.size                                   # one TextureBuffer::fetch per call, whatever the filter
        assert np.array_equal(got, want), (tex, np.argwhere(got != want)[:4])
        assert np.isfinite(got).all()
    if shape == (1, 1) and address_mode != "border":               # a 1x1 map is a constant under every filter
        got, _ = oracle.compat_fetch(flat, 2, u, v)
        assert np.allclose(got[:, 0], flat.texels.view(np.float32)[-1], rtol=1e-6)


@pytest.mark.parametrize("filter_mode", FILTERS)
@pytest.mark.parametrize("address_mode", ADDRESS_MODES)
def test_compat_fetch_agrees_with_the_float64_restatement(filter_mode, address_mode):
    """The independent float64 restatement of the GPU test (R32F, scale only) away from texel and tap boundaries, where float32 and
    float64 round to the same texel."""
    em = np.array([[1.0, 2.0, 5.0], [3.0, 4.0, 7.0]], dtype=np.float32)
    scale = (2.5, -1.75)
    world = map_panel(TextureBuffer(em, scale=scale, filter_mode=filter_mode, address_mode=address_mode))
    flat = flatten(world)
    u, v = np.meshgrid(np.linspace(-1.3, 2.1, 53), np.linspace(-0.9, 1.7, 47))
    got, _ = oracle.compat_fetch(flat, 0, u, v)
    want = sample_numpy(em.astype(np.float64), u, v, scale, filter_mode, address_mode)
    assert np.allclose(got[..., 0], want, rtol=1e-5, atol=1e-5)


# ---- the analytic micro-scenes (test_cuda_compat_gpu.py) in the oracle ----
def test_beer_lambert_through_a_slab():
    thickness = 0.5
    cpu, _, _, _ = _oracle(slab_scene(thickness), 0, 6, 3)
    compat, _, _, _ = _oracle(slab_scene(thickness), COMPAT_BEER_LAMBERT, 6, 3)
    assert np.array_equal(cpu[..., 3], compat[..., 3]) and cpu[..., 3].min() >= 1
    opacity = np.array([200, 150, 100]) / 255.0
    alpha = 1.0 - 128 / 255.0
    lit = cpu[..., :3].min(-1) > 0
    assert lit.mean() > 0.99
    ratio = compat[..., :3][lit] / cpu[..., :3][lit]
    for ch in range(3):
        expected = opacity[ch] * alpha ** thickness
        assert abs(ratio[:, ch].mean() / expected - 1.0) < 0.01, (ch, ratio[:, ch].mean(), expected)
        assert ratio[:, ch].std() < 0.01 * expected


def test_medium_scattering_follows_the_exponential_law():
    sigma, distance = 0.5, 4.0
    _, depth_cpu, _, _ = _oracle(fog_scene(sigma, distance), 0, 1, 4)
    _, depth, state, _ = _oracle(fog_scene(sigma, distance), COMPAT_SCATTERING, 1, 4)
    assert depth_cpu.min() > distance - 1e-3
    scattered = (depth < distance - 1e-3).mean()
    expected = 1.0 - math.exp(-sigma * distance) + 1e-4
    assert abs(scattered - expected) < 0.03, (scattered, expected)
    free = depth[depth < distance - 1e-3]
    trunc_mean = 1 / sigma - distance * math.exp(-sigma * distance) / (1 - math.exp(-sigma * distance))
    assert abs(free.mean() - trunc_mean) < 0.05
    assert (state["material"][depth < distance - 1e-3] == 0).all()


def test_coloured_shadows():
    open_, _, _, _ = _oracle(shadow_scene(False), COMPAT_SHADOW_COLOR, 1, 1)
    opaque, _, _, _ = _oracle(shadow_scene(True), 0, 1, 1)
    tinted, depth, _, _ = _oracle(shadow_scene(True), COMPAT_SHADOW_COLOR, 1, 1)
    under = (opaque[..., :3].max(-1) == 0) & (open_[..., :3].min(-1) > 0) & (depth < 50)
    assert under.sum() > 200
    mask = np.array([255, 64, 64]) / 255.0 * (1.0 - 128 / 255.0)
    ratio = tinted[..., :3][under] / open_[..., :3][under]
    assert np.allclose(ratio, mask[None, :], rtol=2e-3), (ratio.mean(0), mask)
    lit = opaque[..., :3].min(-1) > 0
    assert np.allclose(tinted[..., :3][lit], opaque[..., :3][lit], rtol=1e-5)


def test_texture_and_emission_map_multiply():
    rng = np.random.default_rng(5)
    tex = rng.integers(30, 256, size=(8, 8, 4), dtype=np.uint8)
    tex[..., 3] = 255
    em = rng.uniform(0.5, 2.0, size=(4, 4)).astype(np.float32)
    world = map_panel(TextureBuffer(em), TextureBuffer(tex), color=(128, 255, 64, 255), emission=2.0)
    cpu, depth, _, _ = _oracle(world, 0, 1, 2)
    compat, _, _, _ = _oracle(world, COMPAT_TEXTURE_MULT, 1, 2)
    on_panel = depth < 50
    assert on_panel.mean() > 0.3
    factor = np.array([128, 255, 64], dtype=np.float32) / np.float32(255) * np.float32(2.0)
    assert np.allclose(compat[..., :3][on_panel], cpu[..., :3][on_panel] * factor[None, :], rtol=1e-5)


@pytest.mark.parametrize("filter_mode", FILTERS)
@pytest.mark.parametrize("address_mode", ADDRESS_MODES)
def test_filter_and_address_modes(filter_mode, address_mode):
    em = np.array([[1.0, 2.0, 5.0], [3.0, 4.0, 7.0]], dtype=np.float32)
    scale = (2.5, -1.75)
    world = map_panel(TextureBuffer(em, scale=scale, filter_mode=filter_mode, address_mode=address_mode))
    acc, depth, _, _ = _oracle(world, COMPAT_FILTERING, 1, 2)
    hit_x, hit_y = panel_hits(world.camera)
    on_panel = depth < 50
    assert np.array_equal(on_panel, (np.abs(hit_x) < 1) & (np.abs(hit_y) < 1))
    expected = sample_numpy(em.astype(np.float64), (hit_x + 1) / 2, (hit_y + 1) / 2, scale, filter_mode, address_mode)
    ok = np.abs(acc[..., 0] - expected) <= 1e-3 * np.maximum(np.abs(expected), 1.0)
    assert ok[on_panel].mean() > (0.97 if filter_mode == "point" else 0.999), ok[on_panel].mean()
    cpu, _, _, _ = _oracle(world, 0, 1, 2)
    assert np.array_equal(cpu, _oracle(map_panel(TextureBuffer(em, scale=scale)), 0, 1, 2)[0])


# ---- flags with nothing to act on ----
def test_flags_that_nothing_triggers_give_the_default_frame_bit_for_bit():
    """Opaque materials, no maps, no scattering, a world medium whose opacityColor is (1, 1, 1, 1): Beer multiplies by 1 * 1^d, the mask
    of a crossed opaque triangle has alpha 0 like the CPU engine's, no medium draws a distance.  Every one of the 32 flag combinations (and
    63, reprojection being no integrator flag) renders the default mode's frame, state and non-shadow counters bit for bit."""
    world = scenes.cornell_box(40, 24)
    world.material = Material((255, 255, 255, 0), 0.0, 0.0, 0.0, 1.0, 0.0, name="clear air")
    assert all(m.color[3] == 255 and m.scattering == 0 and m.texture is None and m.emission_map is None for m in world.materials)
    world.add(SpotLight(position=(0.3, 0.9, -0.2), direction=(0, -1, 0), color=(255, 255, 255, 255), size=0.1, emission=80.0, beam_angle=1.0))
    base_acc, base_depth, base_state, base_cnt = _oracle(world, 0, 6, 4, samples=(1, 2), counted=True)
    assert base_acc[..., 3].max() >= 1 and base_cnt["shadow_rays"] > 0
    for flags in list(range(1, 32)) + [63]:
        acc, depth, state, cnt = _oracle(world, flags, 6, 4, samples=(1, 2), counted=True)
        assert np.array_equal(acc, base_acc), flags
        assert np.array_equal(depth, base_depth), flags
        for k in base_state:
            assert np.array_equal(state[k], base_state[k]), (flags, k)
        for k in ("segments", "hits", "light_samples", "texel_fetches", "finished", "shadow_rays"):
            assert cnt[k] == base_cnt[k], (flags, k)


# ---- the coloured mask's grouping and early-out ----
def _sheet_stack(n_sheets, tex_alpha=230, tints=None):
    """Floor under a spot light, camera below the sheets: every pixel sees the floor, every shadow ray crosses every sheet.  The sheets
    are 1x1-textured (one texel fetch per crossing), grouped in instances of the sizes in n_sheets."""
    world = World()
    floor = world.add(Material((255, 255, 255, 255), 0.0, 1.0, name="floor"))
    world.add(Instance(world.add(quad(6.0)), [floor], position=(0, -1, 0), rotation=(-math.pi / 2, 0, 0), name="floor"))
    k = 0
    for g, n in enumerate(n_sheets):
        verts, tris, uv, tri_uv = [], [], [(0.5, 0.5)], []
        for i in range(n):
            y = 1.0 + 0.1 * k
            k += 1
            b = len(verts)
            verts += [(-4, y, -4), (4, y, -4), (4, y, 4), (-4, y, 4)]
            tris += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
            tri_uv += [(0, 0, 0), (0, 0, 0)]
        texel = np.array([[[*(tints[g] if tints else (255, 255, 255)), tex_alpha]]], np.uint8)
        m = world.add(Material((255, 255, 255, 0), 0.0, 0.5, texture=TextureBuffer(texel), name=f"sheets {g}"))
        world.add(Instance(world.add(Mesh(verts, tris, texcrds=uv, tri_texcrds=tri_uv, name=f"stack {g}")), [m], name=f"stack {g}"))
    world.add(SpotLight(position=(0, 4.0, 0), direction=(0, -1, 0), color=(255, 255, 255, 255), size=0.05, emission=200.0, beam_angle=1.4))
    world.camera = Camera(position=(0, 0.0, -0.5), rotation=(-1.2, 0, 0), resolution=(16, 12), fov=0.3, near_far=(1e-2, 1e3),
                          focal_distance=1.0, aperture=1e-6, exposure_time=1.0 / 60.0)
    return world


def _world_visit_order(flat):
    root = flat.nodes[flat.tlas_root]
    assert root["meta"] & 0x80000000, "the test assumes a world tree of one leaf"
    begin, count = int(root["begin"]), int(root["meta"]) & 0x7FFFFFFF
    return [int(i) for i in flat.tlas_order[begin:begin + count]]


@pytest.mark.parametrize("groups", [(7,), (2, 5), (5, 2), (1, 1, 1, 1, 1, 1)])
def test_mask_early_out_per_instance_and_per_world(groups):
    """opacity alpha of one sheet = 25/255 ~ 0.098, 0.098^4 < 1e-4 < 0.098^3.  An instance stops its own walk at the crossing that takes
    ITS mask below 1e-4; the world stops after the instance that takes the RUNNING mask below 1e-4 (cuda_bvh.cuh:186-187, 212-213;
    cuda_instance.cuh:112-113, 144-145).  (2, 5): 2 crossings in the first, the running alpha 0.0096, then the second instance crosses 4
    sheets of its own (its own alpha reaches 9.2e-5), not 2 — 6 fetches per shadow ray; a single running mask would stop after 4."""
    a = np.float32(1) - np.float32(230) / np.float32(255)
    world = _sheet_stack(groups)
    flat = flatten(world)
    order = [i for i in _world_visit_order(flat) if i != 0]  # instance 0 is the floor
    # expected crossings per shadow ray, in the reference's grouping
    running, crossings = np.float32(1), 0
    sizes = {i: groups[i - 1] for i in range(1, len(groups) + 1)}
    for inst in order:
        own = np.float32(1)
        for _ in range(sizes[inst]):
            own = own * a
            crossings += 1
            if own < np.float32(1e-4):
                break
        running = running * own
        if running < np.float32(1e-4):
            break
    mask = running
    acc, depth, _, cnt = _oracle(world, COMPAT_SHADOW_COLOR, 1, 1, counted=True)
    open_acc, open_depth, _, open_cnt = _oracle(_sheet_stack(()), COMPAT_SHADOW_COLOR, 1, 1, counted=True)
    assert (depth < 50).all() and np.array_equal(depth, open_depth)
    assert cnt["shadow_rays"] == open_cnt["shadow_rays"] == depth.size
    assert cnt["texel_fetches"] == crossings * cnt["shadow_rays"], (cnt["texel_fetches"] / cnt["shadow_rays"], crossings)
    lit = open_acc[..., 0] > 0
    assert lit.all()
    ratio = acc[..., :3][lit] / open_acc[..., :3][lit]
    assert np.allclose(ratio, mask, rtol=1e-4), (ratio.mean(), mask)   # V_PL * V_PL.alpha: white sheets, rgb 1


def test_mask_is_the_product_in_reference_order():
    """Coloured sheets in three instances: the mask is the product of the instances' own masks, each the product of its sheets'
    opacityColor in the walk's order, as float32 — rgb * alpha of it is the ratio of the tinted to the open floor."""
    tints = [(250, 120, 60), (90, 240, 200), (200, 200, 70)]
    groups = (1, 2, 1)
    world = _sheet_stack(groups, tex_alpha=64, tints=tints)
    flat = flatten(world)
    order = [i for i in _world_visit_order(flat) if i != 0]
    mask = np.ones(4, np.float32)
    for inst in order:
        t = tints[inst - 1]
        c = np.array([*t, 0], np.float32) / np.float32(255)            # opacityColor: white material of alpha 0 x the texel
        c[3] = np.float32(1) - np.float32(64) / np.float32(255)
        own = np.ones(4, np.float32)
        for _ in range(groups[inst - 1]):
            own = own * c
        mask = mask * own
    acc, _, _, cnt = _oracle(world, COMPAT_SHADOW_COLOR, 1, 1, counted=True)
    open_acc, _, _, _ = _oracle(_sheet_stack(()), COMPAT_SHADOW_COLOR, 1, 1, counted=True)
    assert cnt["texel_fetches"] == 4 * cnt["shadow_rays"]
    ratio = acc[..., :3] / open_acc[..., :3]
    assert np.allclose(ratio, (mask[:3] * mask[3])[None, None, :], rtol=1e-5), (ratio.reshape(-1, 3).mean(0), mask)


# ---- non-vacuity: every flag changes the showcase's oracle frame ----
SHARES = (0.95, 0.85, 0.45, 0.95, 0.95)   # measured: 0.9870, 0.8964, 0.5188, 0.9946, 0.9868
@pytest.mark.parametrize("flag,share", [(COMPAT_BEER_LAMBERT, SHARES[0]), (COMPAT_SCATTERING, SHARES[1]), (COMPAT_SHADOW_COLOR, SHARES[2]),
                                        (COMPAT_TEXTURE_MULT, SHARES[3]), (COMPAT_FILTERING, SHARES[4])])
def test_every_flag_changes_the_showcase(flag, share):
    """The oracle's showcase frame (the scene of test_cuda_compat_oracle_gpu.py, 1 + 8 + 3 passes at depth 5, the GPU comparison's run) with
    one flag differs from its mode-0 frame, by the GPU comparison's own measure (rgb beyond 1e-3 relative, or the finished-path count), on
    at least `share` of the pixels, and `share` is far above what that comparison lets through (1 - 0.988): a kernel that ignored a flag
    cannot meet its bars."""
    world = compat_showcase(160, 96)
    base, _, _, _ = _oracle(world, 0, 12, 5)
    with_flag, _, _, _ = _oracle(world, flag, 12, 5)
    close = (np.abs(with_flag[..., :3] - base[..., :3]) <= 1e-3 * np.maximum(np.abs(base[..., :3]), 1.0)).all(-1)
    differs = 1.0 - (close & (with_flag[..., 3] == base[..., 3])).mean()
    print(f"flag {flag}: oracle frame differs from mode 0 on {differs:.4f} of the pixels")
    assert differs >= share and share > 3 * (1 - 0.988)


def test_a_sky_outside_the_root_box_is_sampled_at_its_texcrd():
    """Compat mode samples the sky at calculateTexcrd(direction) on EVERY miss (cuda_world.cuh:86-88), also when the ray misses the world's
    root box; the default mode keeps texcrd (0, 0) there (cpu_engine_kernel.cpp:279-298).  First pass, depth 1, flags 24 (texture x colour,
    filtering): a pixel that sees the sky = texture(uv).rgb * emission map(uv), against rzo_compat_fetch at the uv of the pixel's ray."""
    world = open_sky(96, 64)
    flat, cam = flatten(world), camera_struct(world.camera)
    acc, depth, _, _ = _oracle(world, COMPAT_TEXTURE_MULT | COMPAT_FILTERING, 1, 1)
    cpu, _, _, _ = _oracle(world, 0, 1, 1)
    sky = depth > 100
    assert sky.mean() > 0.7
    F = np.float32
    px, py = np.meshgrid(np.arange(cam.width, dtype=F), np.arange(cam.height, dtype=F))
    tana = F(cam.tan_half_fov)
    d = np.stack([((px + F(0.5)) / F(cam.width) - F(0.5)) * tana, ((py + F(0.5)) / F(cam.height) - F(0.5)) * (-tana / F(cam.aspect_ratio)),
                  np.ones_like(px)], -1)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    u = -(F(0.5) + np.arctan2(d[..., 2], d[..., 0]) / (F(np.pi) * F(2)))
    v = F(0.5) + np.arcsin(d[..., 1]) / F(np.pi)
    tex, _ = oracle.compat_fetch(flat, 0, u, v)
    em, _ = oracle.compat_fetch(flat, 1, u, v)
    want = tex[..., :3] * em[..., :1]
    ok = np.abs(acc[..., :3] - want).max(-1) <= 1e-4 * np.maximum(want.max(-1), 1.0)
    print(f"sky pixels {sky.mean():.3f}, equal to the texcrd restatement {ok[sky].mean():.4f}")
    assert ok[sky].mean() > 0.99
    assert np.unique(acc[..., 0][sky]).size > 100                            # the map varies over the sky: not one texel
    assert np.unique(cpu[..., 0][sky]).size <= 2                             # the CPU engine's (0, 0) where the root box is missed
