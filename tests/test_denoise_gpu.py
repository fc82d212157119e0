"""The denoiser on the GPU: first-hit guide buffers against the renderer's own answers (depth, ray cast, snapshot), the a-trous filter
against the numpy restatement of include/hiprz.h (tests/denoise_reference.py), its quality against long renders, and its delivery
through hiprz_present, both Engine hosts and the headless runner.  Every figure a bound is compared with is printed before the assert
(pytest -s shows them; DESIGN.md "Denoising" quotes them)."""
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as ref
from rayzath_amd import _abi, _hiprt, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import (SHARD_SAMPLES, TREE_DEVICE_SAH, Context, Engine, LightSampling, RenderConfig, Tracing,
                                denoise_params)
from rayzath_amd.scene import camera_struct, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")

pytestmark = pytest.mark.gpu

_SCENES = {
    "cornell": lambda: scenes.cornell_box(250, 150),                                   # frame edges inside tiles
    "textured": lambda: scenes.textured_sphere_scene(240, 136, resolution=40, map_size=256),  # texture + normal map, 8 instances of 4 meshes
}


def _context(kind="single", tree=None):
    ctx = Context(0) if kind == "single" else Context([0, 0])
    if kind == "samples":
        ctx.set_shard_mode(SHARD_SAMPLES)
    if tree is not None:
        ctx.set_tree(tree)
    return ctx


def _setup(ctx, world, depth=6, rpp=4, seed=20240501):
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(depth, rpp), seed=seed).struct())
    return flat, cam


def _mesh_triangles(flat, root):
    """indices into flat.tris of the mesh tree rooted at node `root`"""
    out, stack = [], [int(root)]
    while stack:
        node = flat.nodes[stack.pop()]
        begin, meta = int(node["begin"]), int(node["meta"])
        if meta & _abi.NODE_LEAF:
            out.extend(range(begin, begin + (meta & _abi.NODE_COUNT_MASK)))
        else:
            stack.extend((begin, begin + 1))
    return out


def _pixel_ray_direction(cam, x, y):
    """generateSimpleRay's direction through the centre of pixel (x, y), float64"""
    tana = float(cam.tan_half_fov)
    dx = ((x + 0.5) / cam.width - 0.5) * tana
    dy = ((y + 0.5) / cam.height - 0.5) * (-tana / float(cam.aspect_ratio))
    d = np.array(cam.x_axis[:], float) * dx + np.array(cam.y_axis[:], float) * dy + np.array(cam.z_axis[:], float)
    return d / np.linalg.norm(d)


# =====================================================================================================================
# guides
# =====================================================================================================================
@pytest.mark.parametrize("scene", sorted(_SCENES))
def test_guides_agree_with_depth_ray_cast_and_snapshot(built, scene):
    world = _SCENES[scene]()
    ctx = _context()
    try:
        flat, cam = _setup(ctx, world)
        W, H = cam.width, cam.height
        ctx.render(1)
        depth = ctx.read_depth()
        g = ctx.read_guides()
        assert g.shape == (H, W)
        assert np.array_equal(g["depth"].view(np.uint32), depth.view(np.uint32)), "guide depth is not the first pass's depth, bit for bit"
        hit = g["instance"] != _abi.GUIDE_MISS
        assert hit.mean() > 0.5
        assert np.all(g["normal"][~hit] == 0) and np.all(g["albedo"][~hit] == 1)
        length = np.linalg.norm(g["normal"][hit].astype(np.float64), axis=-1)
        print(f"\n{scene}: |normal| - 1 on {hit.sum()} hit pixels: max {np.abs(length - 1).max():.3e}")
        assert np.abs(length - 1).max() < 4 * 2.0 ** -23, "normals of hit pixels are not unit vectors"
        assert g["instance"][hit].max() < len(flat.instances)

        # a lattice of 16 x 17 = 272 pixels against hiprz_ray_cast and the snapshot
        xs, ys = np.linspace(1, W - 2, 16).astype(int), np.linspace(1, H - 2, 17).astype(int)
        mesh_of = {}
        flat_checked = untextured_checked = emissive_checked = 0
        worst_normal = 0.0
        for y in ys:
            for x in xs:
                inst, slot, mat, tri = ctx.ray_cast(int(x), int(y))
                rec = g[y, x]
                assert (int(rec["instance"]) == inst) if inst >= 0 else (rec["instance"] == _abi.GUIDE_MISS), f"pixel ({x}, {y})"
                if inst < 0:
                    continue
                m = flat.materials[mat if mat >= 0 else _abi.MATERIAL_DEFAULT]
                if m["texture"] < 0 and m["emission_map"] < 0:
                    want = np.ones(3, np.float32) if m["emission"] > 0 else m["color"][:3].astype(np.float32) / np.float32(255)
                    assert np.array_equal(rec["albedo"], want), f"pixel ({x}, {y}): albedo {rec['albedo']} != {want}"
                    untextured_checked += 1
                    emissive_checked += bool(m["emission"] > 0)
                record = flat.instances[inst]
                if inst not in mesh_of:
                    mesh_of[inst] = _mesh_triangles(flat, record["blas_root"])
                index = next(t for t in mesh_of[inst] if flat.tris[t]["source_index"] == tri)
                if (flat.tris[index]["material_flags"] & _abi.TRI_HAS_NORMALS) or m["normal_map"] >= 0:
                    continue
                local = flat.tri_attrs[index]["face_normal"].astype(np.float64) / record["scale"].astype(np.float64)
                n = record["x_axis"].astype(np.float64) * local[0] + record["y_axis"].astype(np.float64) * local[1] + record["z_axis"].astype(np.float64) * local[2]
                n /= np.linalg.norm(n)
                if np.dot(n, _pixel_ray_direction(cam, x, y)) > 0:
                    n = -n
                worst_normal = max(worst_normal, float(np.abs(rec["normal"].astype(np.float64) - n).max()))
                flat_checked += 1
        print(f"{scene}: lattice of {len(xs) * len(ys)} pixels: {flat_checked} flat-shaded normals, worst component error {worst_normal:.3e} "
              f"({worst_normal * 2 ** 23:.2f} ulp of 1); {untextured_checked} untextured albedos ({emissive_checked} emissive)")
        assert flat_checked >= 100 and untextured_checked >= 100
        # divide by the scale, three multiply-adds per component, a dot product, a square root and a division: six roundings in a chain
        assert worst_normal <= 6 * 2.0 ** -23
    finally:
        ctx.close()


@pytest.mark.parametrize("scene", sorted(_SCENES))
def test_guides_do_not_depend_on_parts_trees_or_passes(built, scene):
    world = _SCENES[scene]()
    images = {}
    for name, kind, tree, passes in (("one part", "single", None, 3), ("two streams", "two-streams", None, 3),
                                     ("device SAH trees", "single", TREE_DEVICE_SAH, 3), ("before any pass", "single", None, 0)):
        ctx = _context(kind, tree)
        try:
            _setup(ctx, world)
            if passes:
                ctx.render(passes)
            ctx.render_guides()
            images[name] = ctx.read_guides().tobytes()
        finally:
            ctx.close()
    for name, data in images.items():
        assert data == images["one part"], f"guides under '{name}' differ from the one-part context's"


def test_rendering_guides_leaves_the_frame_alone_and_restarts_make_them_stale(built):
    world = _SCENES["cornell"]()
    ctx = _context()
    try:
        flat, cam = _setup(ctx, world)
        for call in (ctx.render_guides, ctx.read_guides, ctx.guides_device, ctx.denoise):  # all usable before any pass
            call()
        ctx.render(3)
        before = (ctx.read_accum(), ctx.read_state(), ctx.ray_count(), ctx.pass_count(), ctx.read_depth())
        ctx.render_guides()
        g0 = ctx.read_guides()
        after = (ctx.read_accum(), ctx.read_state(), ctx.ray_count(), ctx.pass_count(), ctx.read_depth())
        assert np.array_equal(before[0], after[0]) and before[2:4] == after[2:4] and np.array_equal(before[4], after[4])
        for key in before[1]:
            assert np.array_equal(before[1][key], after[1][key]), key
        ctx.render(2)  # more passes: the accumulation goes on, the guides stay
        assert ctx.read_guides().tobytes() == g0.tobytes()
        # a moved camera restarts accumulation: hiprz_denoise renders the guides again by itself
        cam.position[0] += 0.4
        ctx.upload_camera(cam)
        ctx.render(2)
        ctx.denoise()
        g1 = ctx.read_guides()
        assert g1.tobytes() != g0.tobytes()
        assert np.array_equal(g1["depth"].view(np.uint32), ctx.read_depth().view(np.uint32))
        # new materials restart it too
        flat.materials["color"][2] = (10, 20, 30, 255)
        ctx.update_shading(flat)
        g2 = ctx.read_guides()
        assert g2.tobytes() != g1.tobytes() and np.array_equal(g2["depth"], g1["depth"])
    finally:
        ctx.close()


def test_calls_before_scene_and_camera_are_state_errors(built):
    ctx = _context()
    try:
        for call in (ctx.render_guides, ctx.read_guides, ctx.guides_device, ctx.denoise, ctx.read_denoised, ctx.read_denoised_rgba8,
                     lambda: ctx.denoise_image(1, None, None, 2)):
            with pytest.raises(HiprzError) as e:
                call()
            assert e.value.code == _abi.ERR_STATE
        world = _SCENES["cornell"]()
        _setup(ctx, world)
        with pytest.raises(HiprzError) as e:
            ctx.read_denoised()  # nothing denoised yet
        assert e.value.code == _abi.ERR_STATE
        with pytest.raises(HiprzError) as e:
            ctx.denoise(denoise_params(iterations=7))
        assert e.value.code == _abi.ERR_INVALID
    finally:
        ctx.close()


def test_denoise_on_a_shard_of_a_frame_is_a_state_error_with_a_message(built):
    ctx = _context()
    try:
        _setup(ctx, _SCENES["cornell"]())
        ctx.set_shard(1, 2)
        ctx.render(2)
        with pytest.raises(HiprzError) as e:
            ctx.denoise()
        assert e.value.code == _abi.ERR_STATE and "shard 1 of 2" in str(e.value)
    finally:
        ctx.close()


# =====================================================================================================================
# the filter against the restatement
# =====================================================================================================================
def _device_filter(ctx, accum, guides, params):
    """hiprz_denoise_image on host arrays: (H, W, 4) float32"""
    a, g = _hiprt.DeviceBuffer.of(accum.astype(np.float32)), _hiprt.DeviceBuffer.of(guides)
    d = _hiprt.DeviceBuffer(accum.shape[0] * accum.shape[1] * 16)
    try:
        ctx.denoise_image(a.ptr, g.ptr, params, d.ptr)
        ctx.sync()
        return d.download(accum.shape, np.float32)
    finally:
        a.free(), g.free(), d.free()


def _compare_with_restatement(ctx, cam, accum, guides, params, what, pooled=None):
    """device against the float64 restatement; the bound is four times the float32 restatement's own deviation from it.  `pooled`: a list
    that collects (what, float32 deviation, device deviation) instead — the caller holds the device to the largest float32 deviation of
    the whole pool (_hold_to_the_pooled_bar)"""
    r64 = ref.atrous(accum, guides, params, cam.aperture, cam.exposure_time, np.float64)
    r32 = ref.atrous(accum, guides, params, cam.aperture, cam.exposure_time, np.float32)
    got = _device_filter(ctx, accum, guides, params)
    dev32 = float(np.abs(r32.astype(np.float64) - r64).max())
    dev_gpu = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"\n{what}: float32 restatement deviates from float64 by {dev32:.3e}, the device by {dev_gpu:.3e} "
          f"(ratio {dev_gpu / dev32 if dev32 else float('inf'):.2f}, values up to {np.abs(r64[..., :3]).max():.3g})")
    assert np.all(got[..., 3] == 1)
    if pooled is not None:
        pooled.append((what, dev32, dev_gpu))
    else:
        assert dev_gpu <= 4 * dev32, what
    return got, r64, dev32


def _hold_to_the_pooled_bar(pooled, what):
    """the same bar over a pool of frames: every frame's device deviation <= 4 x the largest float32 deviation of the pool, so that a frame
    on which float32 happens to be exact (one pixel, one tap) does not set a bound of zero"""
    dev32 = max(d for _, d, _ in pooled)
    worst = max(pooled, key=lambda r: r[2])
    print(f"{what}: pooled float32 deviation {dev32:.3e} over {len(pooled)} frames, largest device deviation {worst[2]:.3e} ({worst[0]})")
    assert dev32 > 0, what
    assert not [r for r in pooled if r[2] > 4 * dev32], what


def _synthetic(H, W, seed):
    rng = np.random.default_rng(seed)
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., 3] = rng.integers(0, 9, (H, W))               # some pixels have no finished path
    accum[..., :3] = rng.gamma(2.0, 0.5, (H, W, 3)) * np.maximum(accum[..., 3:4], 1)
    g = np.zeros((H, W), _abi.guide_dtype)
    blocks = rng.integers(0, 5, (H // 12 + 1, W // 20 + 1))
    inst = np.kron(blocks, np.ones((12, 20), int))[:H, :W]
    g["instance"] = np.where(inst == 4, _abi.GUIDE_MISS, inst)
    n = rng.normal(size=(5, 3)) * 0.15 + np.array([0.0, 0.0, -1.0])
    normal = n[inst] + rng.normal(size=(H, W, 3)) * 0.02
    g["normal"] = normal / np.linalg.norm(normal, axis=-1, keepdims=True)
    g["normal"][inst == 4] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    g["depth"] = np.where(inst == 4, 1000.0, 2.0 + 0.01 * xx + 0.02 * yy + inst)
    g["albedo"] = rng.uniform(0.0, 1.0, (H, W, 3))
    g["albedo"][rng.uniform(size=(H, W)) < 0.05] = (0.0, 0.004, 0.5)  # below the 0.01 floor
    g["albedo"][inst == 4] = 1
    return accum, g


@pytest.mark.parametrize("scene", sorted(_SCENES))
def test_filter_equals_the_restatement_on_a_real_frame(built, scene):
    world = _SCENES[scene]()
    ctx = _context()
    try:
        _, cam = _setup(ctx, world)
        ctx.render(8)
        accum, guides = ctx.read_accum(), ctx.read_guides()
        for params in (denoise_params(), denoise_params(iterations=6, sigma_color=0.0), denoise_params(iterations=1, demodulate=False)):
            what = f"{scene} iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
            _compare_with_restatement(ctx, cam, accum, guides, params, what)
    finally:
        ctx.close()


def test_filter_equals_the_restatement_on_synthetic_inputs(built):
    world = scenes.cornell_box(173, 99)  # odd sizes: every step leaves partial sub-lattice tiles
    ctx = _context()
    try:
        _, cam = _setup(ctx, world)
        accum, guides = _synthetic(99, 173, 17)
        for params in (denoise_params(), denoise_params(iterations=6, sigma_normal=8.0, sigma_depth=0.02, sigma_color=0.2),
                       denoise_params(iterations=3, sigma_color=0.0, demodulate=False)):
            what = f"synthetic iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
            got, _, _ = _compare_with_restatement(ctx, cam, accum, guides, params, what)
            again = _device_filter(ctx, accum, guides, params)
            assert got.tobytes() == again.tobytes(), "two calls gave different bits"
    finally:
        ctx.close()


# Frames smaller than the filter's reach.  At step s = 2^i the kernel tiles the s x s residue classes of the frame; on these sizes whole
# classes hold no pixel from step 2, 4 or 8 on (1x1: from the first), every tile is a halo, and at 5 and 6 iterations the step (16, 32)
# exceeds one or both sides of every frame but 64x3 / 3x64 / 17x41 / 33x33, whose long side it still fits.
SMALL_FRAMES = ((1, 1), (64, 3), (3, 64), (17, 41), (33, 33), (5, 3))          # width x height


@pytest.mark.parametrize("sigma_color", [0.0, None])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("iterations", [1, 5, 6])
def test_filter_equals_the_restatement_on_small_frames(built, iterations, demodulate, sigma_color):
    ctx = _context()
    try:
        params = denoise_params(iterations=iterations, demodulate=demodulate, sigma_color=sigma_color)
        pooled = []
        for k, (W, H) in enumerate(SMALL_FRAMES):
            _, cam = _setup(ctx, scenes.cornell_box(W, H))
            accum, guides = _synthetic(H, W, 31 + k)
            what = f"{W}x{H} iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
            got, _, _ = _compare_with_restatement(ctx, cam, accum, guides, params, what, pooled)
            assert got.shape == (H, W, 4) and np.isfinite(got).all(), what
            again = _device_filter(ctx, accum, guides, params)
            assert got.tobytes() == again.tobytes(), f"{what}: two calls gave different bits"
        _hold_to_the_pooled_bar(pooled, f"small frames iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}")
    finally:
        ctx.close()


def test_demodulation_preserves_texture_and_instances_do_not_mix(built):
    world = scenes.cornell_box(160, 96)
    ctx = _context()
    try:
        _, cam = _setup(ctx, world)
        H, W = 96, 160
        yy, xx = np.mgrid[0:H, 0:W]
        # constant irradiance times a checkerboard albedo, colour term off
        guides = ref.make_guides(H, W)
        guides["albedo"] = np.where((((xx // 3) + (yy // 3)) % 2)[..., None] == 0, np.float32(0.9), np.float32(0.15))
        accum = np.ones((H, W, 4), np.float32) * 4
        accum[..., :3] = np.float32(0.7) * guides["albedo"] * 4
        params = denoise_params(sigma_color=0.0)
        got, _, dev32 = _compare_with_restatement(ctx, cam, accum, guides, params, "checkerboard albedo")
        radiance = accum[..., :3].astype(np.float64) / 4
        err = float(np.abs(got[..., :3] - radiance).max())
        print(f"checkerboard: device output differs from the input radiance by {err:.3e} (bound {4 * dev32:.3e})")
        assert err <= 4 * dev32
        # the same without demodulation blurs the texture: the check above is not vacuous
        blurred = _device_filter(ctx, accum, guides, denoise_params(sigma_color=0.0, demodulate=False))
        assert np.abs(blurred[..., :3] - radiance).max() > 0.1

        # a step image over two instances comes back unchanged
        guides = ref.make_guides(H, W)
        guides["instance"][:, W // 2:] = 1
        accum = np.ones((H, W, 4), np.float32)
        accum[:, : W // 2, :3], accum[:, W // 2:, :3] = (1.0, 0.5, 0.25), (100.0, 40.0, 70.0)
        params = denoise_params()
        got = _device_filter(ctx, accum, guides, params)
        rel = float((np.abs(got[..., :3] - accum[..., :3]) / accum[..., :3]).max())
        # a normalised sum of up to 25 equal values: 25 products, 24 + 24 additions along two chains and a division — at most 27 roundings
        # of relative size 2^-24 in a chain per iteration; leakage across the step would be of order 1
        bound = params.iterations * 27 * 2.0 ** -24
        print(f"two-instance step: relative change {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["single", "two-streams", "samples"])
def test_denoise_equals_denoise_image_on_the_read_accumulator(built, kind):
    world = _SCENES["cornell"]()
    ctx = _context(kind)
    try:
        _, cam = _setup(ctx, world)
        ctx.render(1), ctx.render(5)
        for params in (None, denoise_params(iterations=2, sigma_color=0.1)):
            ctx.denoise(params)
            got, got8 = ctx.read_denoised(), ctx.read_denoised_rgba8()
            accum = ctx.read_accum()
            if kind == "samples":
                assert ctx.ray_count() == 2 * 6 * cam.width * cam.height  # the accumulator is the sum of two parts' frames
            want = _device_filter(ctx, accum, ctx.read_guides(), params)
            assert got.tobytes() == want.tobytes(), f"{kind}: hiprz_denoise differs from hiprz_denoise_image on hiprz_read_accum's image"
            # ... and its RGBA8 is the tone map of that image
            d, out8 = _hiprt.DeviceBuffer.of(want), _hiprt.DeviceBuffer(want.shape[0] * want.shape[1] * 4)
            ctx.tonemap_image(d.ptr, out8.ptr)
            ctx.sync()
            assert np.array_equal(out8.download(got8.shape, np.uint8), got8)
            d.free(), out8.free()
    finally:
        ctx.close()


# =====================================================================================================================
# quality
# =====================================================================================================================
# 960 x 540: the five default iterations reach 62 pixels to every side, a filter for frames of the flagship's size (1920 x 1080) — on a
# thumbnail its support is a quarter of the picture and what it measures is not what a user sees
_QUALITY = {
    "cornell": (lambda: scenes.cornell_box(960, 540), LightSampling()),
    "lights and maps": (lambda: scenes.shading_inputs_scene(960, 540, lights=True), LightSampling(2, 2)),
}


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.mark.parametrize("scene", sorted(_QUALITY))
def test_denoised_frame_is_closer_to_the_reference_than_the_raw_frame(built, scene):
    """N = 64 passes against the unchanged renderer at 64 * N passes (another seed), RMSE over the tone-mapped image in [0, 1] before
    quantisation, default parameters.  Measured on MI355X (960 x 540): Cornell raw 0.470, denoised / raw 0.912, denoised reference / raw
    0.119; lights and maps raw 0.031, 0.840, 0.813 (DESIGN.md "Denoising" has the sweep the default sigma_color was taken from)."""
    build, sampling = _QUALITY[scene]
    world = build()
    N = 64
    noisy, clean = _context(), _context()
    try:
        for ctx, seed in ((noisy, 20240501), (clean, 977)):
            flat, cam = flatten(world), camera_struct(world.camera)
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(sampling, Tracing(8, N), seed=seed).struct())
        noisy.render(N)
        for _ in range(64):
            clean.render(N)
        assert noisy.pass_count() == N and clean.pass_count() == 64 * N
        tm = lambda image: ref.tonemap_unquantised(image, cam.aperture, cam.exposure_time)  # noqa: E731
        reference = tm(clean.read_accum())
        noisy.denoise(), clean.denoise()
        raw = _rmse(tm(noisy.read_accum()), reference)
        denoised = _rmse(tm(noisy.read_denoised()), reference)
        blur = _rmse(tm(clean.read_denoised()), reference)
        print(f"\n{scene}: RMSE raw {N}-pass frame {raw:.5f}, denoised {denoised:.5f} (ratio {denoised / raw:.3f}), "
              f"denoised reference {blur:.5f} (ratio to raw {blur / raw:.3f})")
        assert denoised < raw, "the filter did not bring the noisy frame closer to the reference"
        assert blur <= raw, "the blur the filter adds to a clean frame exceeds the noise it removes"
    finally:
        noisy.close(), clean.close()


# =====================================================================================================================
# delivery
# =====================================================================================================================
@pytest.mark.parametrize("kind", ["single", "two-streams", "samples"])
def test_present_delivers_the_denoised_image_while_set(built, kind):
    world = _SCENES["cornell"]()
    ctx = _context(kind)
    try:
        _, cam = _setup(ctx, world)
        params = denoise_params(iterations=4)
        ctx.render(1), ctx.render(4)
        ctx.set_denoise(params)
        for _ in range(3):
            ctx.render(4)
            seq = ctx.present(100, 80)
            frame = ctx.read_frame(seq, copy=True)
            assert np.array_equal(frame["rgba8"], ctx.read_denoised_rgba8())
            assert np.array_equal(frame["depth"], ctx.read_depth()) and frame["hit"] == ctx.ray_cast(100, 80)
            ctx.tonemap()
            assert not np.array_equal(frame["rgba8"], ctx.read_rgba8())
            twin = _device_filter(ctx, ctx.read_accum(), ctx.read_guides(), params)
            assert ctx.read_denoised().tobytes() == twin.tobytes()
        ctx.set_denoise(None)
        ctx.render(4)
        frame = ctx.read_frame(ctx.present(100, 80), copy=True)
        ctx.tonemap()
        assert np.array_equal(frame["rgba8"], ctx.read_rgba8())
    finally:
        ctx.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_python_engine_delivers_denoised_frames(built, pipelined):
    params = denoise_params()
    cfg = RenderConfig(tracing=Tracing(4, 3))
    world = scenes.cornell_box(96, 64)
    engine = Engine(0, pipelined=pipelined, denoise=params)
    twin = _context()
    try:
        _setup(twin, scenes.cornell_box(96, 64), depth=4, rpp=3)
        expected = []
        for k in range(4):
            engine.renderWorld(world, cfg, sync=not pipelined)
            twin.render(3)
            twin.denoise(params)
            expected.append(twin.read_denoised_rgba8())
            want = expected[k - 1] if pipelined else expected[k]  # sync=False hands out the previous call's frame
            if pipelined and k == 0:
                continue
            assert np.array_equal(world.camera.image_buffer, want), f"call {k}"
        engine.set_denoise(None)
        engine.renderWorld(world, cfg, sync=True)
        twin.render(3), twin.tonemap()
        assert np.array_equal(world.camera.image_buffer, twin.read_rgba8())
    finally:
        twin.close()


def test_cpp_engine_delivers_denoised_frames(built, tmp_path):
    exe = str(tmp_path / "denoise_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "denoise_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DENOISE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_headless_runner_saves_the_denoised_frame_when_asked(built, tmp_path):
    world = scenes.cornell_box(128, 96)
    scene_io.save_scene_json(world, str(tmp_path / "cornell.json"))
    exe = os.path.join(CSRC, "hiprz_headless")
    frames = {}
    for name, key in (("plain", ""), ("denoised", ', "denoise": true')):
        (tmp_path / f"{name}.json").write_text('{"tasks": [{"scene path": "cornell.json", "engine": ["HIPGPU"], "rpp": 20, "timeout": 60.0, "max depth": 4' + key + "}]}")
        out_dir = tmp_path / name
        r = subprocess.run([exe, "--headless", str(tmp_path / f"{name}.json"), str(out_dir), "-r", "--quiet"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        images = [f for f in os.listdir(out_dir) if f.endswith("_HIPGPU.png")]
        assert len(images) == 1
        frames[name] = scene_io.read_image(str(out_dir / images[0]))
    # the runner's passes: one warm-up call, the 20 of the budget, the final synchronous one — on the scene file's own snapshot
    twin = _context()
    try:
        loaded = scene_io.load_scene_file(str(tmp_path / "cornell.json"))
        twin.upload_scene(loaded.flat), twin.upload_camera(loaded.camera)
        twin.set_config(RenderConfig(tracing=Tracing(4, 1)).struct())
        twin.render(22)
        twin.tonemap()
        assert np.array_equal(frames["plain"], twin.read_rgba8()), "a task file without the key no longer gives the plain frame"
        twin.denoise()
        assert np.array_equal(frames["denoised"], twin.read_denoised_rgba8())
    finally:
        twin.close()
    (tmp_path / "bad.json").write_text('{"tasks": [{"scene path": "cornell.json", "denoise": 1}]}')
    r = subprocess.run([exe, "--headless", str(tmp_path / "bad.json"), "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "denoise" in r.stdout + r.stderr


def test_pipelined_denoised_frames_of_a_two_stream_context_equal_a_synchronous_twin(built):
    """render, present, render, present ... with nothing but enqueued work between the frames: the head assembles the accumulator of frame
    N from its peer's tiles while the peer's stream already renders frame N + 1 and pushes its tiles — every frame must still be the
    frame a twin produces that waits for the device after each step."""
    world = scenes.cornell_box(1000, 600)  # large enough that the peer's next push comes before the head's filter has finished
    params = denoise_params()
    piped, twin = _context("two-streams"), _context("two-streams")
    try:
        _setup(piped, world, depth=4), _setup(twin, world, depth=4)
        piped.set_denoise(params)
        piped.render(1), twin.render(1)
        expected, seq = [], 0
        for i in range(8):
            piped.render(2)
            seq = piped.present(10, 10)
            if i:
                got = piped.read_frame(seq - 1)
                assert np.array_equal(got["rgba8"], expected[i - 1]), f"frame {i - 1} is not the synchronous twin's"
            twin.render(2)
            twin.denoise(params)
            expected.append(twin.read_denoised_rgba8())
        assert np.array_equal(piped.read_frame(seq)["rgba8"], expected[-1])
    finally:
        piped.close(), twin.close()


def test_present_on_a_shard_with_denoise_set_is_refused_before_anything_is_enqueued(built):
    ctx = _context()
    try:
        _setup(ctx, _SCENES["cornell"]())
        ctx.set_shard(0, 2)
        ctx.render(2)
        assert ctx.present(5, 5) == 1
        ctx.set_denoise(denoise_params())
        for _ in range(2):
            with pytest.raises(HiprzError) as e:
                ctx.present(5, 5)
            assert e.value.code == _abi.ERR_STATE and "shard 0 of 2" in str(e.value)
        assert ctx.read_frame()["sequence"] == 1  # nothing was presented
        ctx.set_denoise(None)
        ctx.render(2)
        ctx.tonemap()
        want = ctx.read_rgba8()
        assert ctx.present(5, 5) == 2
        assert np.array_equal(ctx.read_frame(2)["rgba8"], want)
    finally:
        ctx.close()


def test_misses_at_an_infinite_far_plane_are_filtered_without_nan(built):
    world = scenes.cornell_box(120, 72)
    ctx = _context()
    try:
        _, cam = _setup(ctx, world)
        accum, guides = _synthetic(72, 120, 23)
        miss = guides["instance"] == _abi.GUIDE_MISS
        assert miss.sum() > 200
        guides["depth"][miss] = np.inf
        got, r64, _ = _compare_with_restatement(ctx, cam, accum, guides, denoise_params(), "misses at infinity")
        assert np.isfinite(got).all() and np.isfinite(r64).all()
        assert got[miss][..., :3].std() < 0.7 * (accum[miss][..., :3] / np.maximum(accum[miss][..., 3:4], 1)).std(), "the sky was not smoothed"
    finally:
        ctx.close()
