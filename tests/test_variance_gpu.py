"""The per-pixel variance estimate (hiprz_set_variance: batch moments of the accumulator, hiprz_read_variance) and the variance-guided
a-trous filter (HIPRZ_DENOISE_VARIANCE) on the GPU: against the numpy restatement of include/hiprz.h (tests/variance_reference.py),
against the empirical variance over independent seeds, and through every way a frame leaves the project.  Every figure a bound is
compared with is printed before the assert (pytest -s shows them; DESIGN.md "Variance" quotes them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as ref
import variance_reference as vref
from rayzath_amd import _abi, _hiprt, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import (COMPAT_REPROJECTION, SHARD_SAMPLES, Context, Engine, LightSampling, RenderConfig, Tracing, denoise_params)
from rayzath_amd.scene import camera_struct, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")

pytestmark = pytest.mark.gpu

_SMALL = {
    "cornell": lambda w=80, h=48: scenes.cornell_box(w, h),
    "lights": lambda w=80, h=48: scenes.shading_inputs_scene(w, h, lights=True),
}
_CALLS = (1, 3, 8, 8, 2, 8)


def _context(kind="single", variance=True):
    ctx = Context(0) if kind == "single" else Context([0, 0])
    if kind == "samples":
        ctx.set_shard_mode(SHARD_SAMPLES)
    if variance:
        ctx.set_variance(1)
    return ctx


def _setup(ctx, world, depth=6, rpp=4, seed=20240501, sampling=None):
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(sampling, Tracing(depth, rpp), seed=seed).struct())
    return flat, cam


def _bar(got, r32, r64, what):
    """the project's bar: the device's largest deviation from the float64 restatement is at most four times the float32 restatement's"""
    dev32 = float(np.abs(r32.astype(np.float64) - r64).max())
    dev_gpu = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"\n{what}: float32 restatement deviates from float64 by {dev32:.3e}, the device by {dev_gpu:.3e} "
          f"(ratio {dev_gpu / dev32 if dev32 else float('inf'):.2f}, values up to {np.abs(r64).max():.3g})")
    assert dev_gpu <= 4 * dev32, what


def _render_with_restatement(ctx, calls):
    """render `calls`, read the accumulator after each: (last accumulator, float64 moments, float32 moments)"""
    shape = (ctx.height, ctx.width)
    m64, m32 = vref.Moments(shape, np.float64), vref.Moments(shape, np.float32)
    accum = None
    for n in calls:
        ctx.render(n)
        accum = ctx.read_accum()
        m64.close(accum), m32.close(accum)
    return accum, m64, m32


# =====================================================================================================================
# 1. moments and estimate against the restatement
# =====================================================================================================================
@pytest.mark.parametrize("scene", sorted(_SMALL))
def test_estimate_equals_the_restatement(built, scene):
    ctx = _context()
    try:
        _setup(ctx, _SMALL[scene]())
        ctx.render(_CALLS[0])
        first = ctx.read_variance()
        assert np.all(first[..., :3] == 0) and first[..., 3].max() <= 1, "one call is one batch: no estimate yet"
        ctx.reset()
        accum, m64, m32 = _render_with_restatement(ctx, _CALLS)
        got = ctx.read_variance()
        assert got.shape == accum.shape and got.dtype == np.float32
        K = m64.m1[..., 3]
        assert np.array_equal(got[..., 3], K), "K differs from the restatement's"
        late = int((K < len(_CALLS)).sum())
        print(f"\n{scene}: K from {int(K.min())} to {int(K.max())}, {late} of {K.size} pixels closed fewer batches than there were calls")
        # (a pass is one segment of every pixel's path: in the closed Cornell box no path ends in the first call's single pass)
        assert late > 0 and K.max() >= len(_CALLS) - 1, "the first calls were meant to leave pixels, not all the frame, without a finished path"
        r64 = vref.estimate(accum, m64.m0, m64.m1, np.float64)
        r32 = vref.estimate(accum, m32.m0, m32.m1, np.float32)
        assert (r64[..., :3] > 0).mean() > 0.1
        _bar(got[..., :3], r32[..., :3], r64[..., :3], f"{scene} variance estimate")
        image = np.zeros_like(got)  # the device image is the same image
        pointer = ctx.variance_device()
        ctx.sync()
        assert _hiprt.runtime().hipMemcpy(image.ctypes.data, C.c_void_p(pointer), image.nbytes, 2) == 0
        assert image.tobytes() == got.tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 2. off means off
# =====================================================================================================================
@pytest.mark.parametrize("kind", ["single", "two-streams", "samples", "split"])
def test_the_estimate_changes_nothing_else(built, kind):
    results = []
    for variance in (True, False):
        ctx = _context("single" if kind == "split" else kind, variance)
        try:
            if kind == "split":
                ctx.set_pipeline(1)
                _, cam = _setup(ctx, scenes.cornell_box(96, 64))
                calls = (4, 4, 4)
            else:
                _, cam = _setup(ctx, _SMALL["lights"]())
                calls = _CALLS
            for n in calls:
                ctx.render(n)
            if variance:
                assert ctx.read_variance()[..., 3].max() >= len(calls) - 1
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.ray_count(), ctx.pass_count(),
                            ctx.graph_captures()))
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "ray_count", "pass_count", "graph_captures"), *results):
        assert a == b, f"{kind}: {name} differs once hiprz_set_variance is on"
    if kind == "split":
        assert results[0][5] >= 1, "the split pipeline was meant to replay a captured graph"


# =====================================================================================================================
# 3. parts
# =====================================================================================================================
def test_two_streams_in_tile_mode_give_the_one_part_estimate(built):
    images = {}
    for kind in ("single", "two-streams"):
        ctx = _context(kind)
        try:
            _setup(ctx, _SMALL["cornell"](250, 150))  # frame edges inside tiles
            for n in _CALLS:
                ctx.render(n)
            images[kind] = ctx.read_variance()
        finally:
            ctx.close()
    assert images["single"][..., 3].max() >= len(_CALLS) - 1
    assert images["single"].tobytes() == images["two-streams"].tobytes()


def test_two_streams_in_sample_mode_sum_the_moments_of_their_seed_streams(built):
    seed = 4242
    runs = []
    for s in (seed, seed + 1):
        ctx = _context(variance=False)
        try:
            _setup(ctx, _SMALL["lights"](), seed=s)
            runs.append(_render_with_restatement(ctx, _CALLS))
        finally:
            ctx.close()
    ctx = _context("samples")
    try:
        _setup(ctx, _SMALL["lights"](), seed=seed)
        for n in _CALLS:
            ctx.render(n)
        got, accum = ctx.read_variance(), ctx.read_accum()
    finally:
        ctx.close()
    assert np.array_equal(accum, runs[0][0] + runs[1][0]), "the sample-mode accumulator is not the sum of the two seed streams"
    want = {}
    for T, k in ((np.float64, 1), (np.float32, 2)):
        m0 = vref.sum_parts([r[k].m0 for r in runs], T)
        m1 = vref.sum_parts([r[k].m1 for r in runs], T)
        want[T] = vref.estimate(accum, m0, m1, T)
    assert np.array_equal(got[..., 3], want[np.float64][..., 3]) and got[..., 3].max() == 2 * len(_CALLS)
    _bar(got[..., :3], want[np.float32][..., :3], want[np.float64][..., :3], "sample mode variance estimate")


def test_a_shard_of_a_frame_reads_zeros_outside_its_tiles(built):
    whole, shard = _context(), _context()
    try:
        for ctx in (whole, shard):
            _setup(ctx, _SMALL["cornell"](250, 150))
        shard.set_shard(1, 3)
        for ctx in (whole, shard):
            for n in (8, 8, 8):
                ctx.render(n)
        v, full, owned = shard.read_variance(), whole.read_variance(), shard.read_accum()[..., 3] > 0
        assert 0.2 < owned.mean() < 0.5
        assert np.all(v[~owned] == 0), "pixels of other shards hold an estimate"
        assert np.array_equal(v[owned], full[owned]) and v[owned][..., 3].max() == 3
    finally:
        whole.close(), shard.close()


# =====================================================================================================================
# 4. restarts
# =====================================================================================================================
def test_whatever_restarts_accumulation_restarts_the_estimate(built):
    ctx = _context()
    try:
        flat, cam = _setup(ctx, _SMALL["cornell"]())

        def batches():
            K = ctx.read_variance()[..., 3]
            assert (K == K.max()).mean() > 0.9
            return int(K.max())

        ctx.render(8), ctx.render(8)
        assert batches() == 2
        ctx.reset()
        ctx.render(8)
        assert batches() == 1, "hiprz_reset"
        ctx.render(8)
        cam.position[0] += 0.25
        ctx.upload_camera(cam)
        assert np.all(ctx.read_variance() == 0), "a restart is pending: there is no estimate"
        ctx.render(8)
        assert batches() == 1, "upload_camera"
        ctx.render(8)
        flat.materials["color"][2] = (10, 20, 30, 255)
        ctx.update_shading(flat)
        ctx.render(8)
        assert batches() == 1, "update_shading"
        ctx.render(8)
        ctx.set_variance(1)  # no change: nothing restarts
        assert batches() == 2 and ctx.pass_count() == 16
        ctx.set_variance(0)
        with pytest.raises(HiprzError) as e:
            ctx.read_variance()
        assert e.value.code == _abi.ERR_STATE
        ctx.render(8)
        assert ctx.pass_count() == 8, "switching the estimate off did not restart accumulation"
        ctx.set_variance(1)
        ctx.render(8)
        assert batches() == 1 and ctx.pass_count() == 8, "set_variance(0 -> 1)"
    finally:
        ctx.close()


def test_reprojected_history_is_not_a_sample(built):
    ctx = _context()
    try:
        _, cam = _setup(ctx, _SMALL["cornell"]())
        ctx.set_mode(COMPAT_REPROJECTION)
        ctx.render(8)
        assert ctx.read_variance()[..., 3].max() == 1  # the first frame has no history
        cam.position[0] += 0.05
        ctx.upload_camera(cam)
        ctx.render(8)
        assert (ctx.read_accum()[..., 3] % 1 != 0).mean() > 0.5, "the restart was meant to carry history over (its path counts come blended)"
        assert np.all(ctx.read_variance() == 0), "the call that blended history in closed a batch"
        ctx.render(8)
        v = ctx.read_variance()
        assert v[..., 3].max() == 1 and np.all(v[..., :3] == 0)
        ctx.render(8)
        assert ctx.read_variance()[..., 3].max() == 2
    finally:
        ctx.close()


def test_every_camera_keeps_moments_of_its_own_and_a_resize_drops_them(built):
    ctx = _context()
    try:
        world = _SMALL["cornell"]()
        flat, cam = flatten(world), camera_struct(world.camera)
        ctx.upload_scene(flat)
        ctx.set_config(RenderConfig(tracing=Tracing(6, 4)).struct())
        ctx.set_camera_count(2)
        other = camera_struct(_SMALL["cornell"](70, 40).camera)
        other.position[0] += 0.3
        ctx.select_camera(0), ctx.upload_camera(cam)
        ctx.select_camera(1), ctx.upload_camera(other)
        for _ in range(3):
            ctx.render(8)
        ctx.select_camera(0)
        for _ in range(2):
            ctx.render(8)
        v0 = ctx.read_variance()
        ctx.select_camera(1)
        v1 = ctx.read_variance()
        assert v0.shape == (48, 80, 4) and v1.shape == (40, 70, 4)
        assert v0[..., 3].max() == 2 and v1[..., 3].max() == 3
        # ... each the estimate of a context that renders that camera alone
        for camera, calls, want in ((cam, 2, v0), (other, 3, v1)):
            twin = _context()
            try:
                twin.upload_scene(flat), twin.upload_camera(camera)
                twin.set_config(RenderConfig(tracing=Tracing(6, 4)).struct())
                for _ in range(calls):
                    twin.render(8)
                assert twin.read_variance().tobytes() == want.tobytes()
            finally:
                twin.close()
        bigger = camera_struct(_SMALL["cornell"](90, 50).camera)
        ctx.upload_camera(bigger)
        v = ctx.read_variance()
        assert v.shape == (50, 90, 4) and np.all(v == 0), "a resized camera kept moments"
        ctx.render(8)
        assert ctx.read_variance()[..., 3].max() == 1
        ctx.select_camera(0)
        assert ctx.read_variance().tobytes() == v0.tobytes(), "the other camera's resize touched this one's moments"
    finally:
        ctx.close()


# =====================================================================================================================
# 5. calibration against the empirical variance
# =====================================================================================================================
_MEASURED_RATIO = {"cornell": 1.022, "lights": 1.438}  # MI355X, 64 x 48, 24 seeds of 8 calls of 8 passes (the docstring below)


@pytest.mark.parametrize("scene", sorted(_SMALL))
def test_estimate_is_calibrated_against_the_variance_over_seeds(built, scene):
    """sum_p mean_seeds V_g(p) / sum_p var_seeds r_g(p) over 24 independent seeds of the unchanged renderer, each 8 calls of 8 passes at
    64 x 48: 1 for an unbiased estimate; an estimate off by the batch count or by alpha would be off by 8 x or more.  Measured on MI355X:
    Cornell 1.022 (emission only: a path's radiance and its alpha land in the same batch), lights and maps 1.438 (next-event estimation
    adds light along the way: a path that straddles two calls leaves its fragment in one batch and its alpha in the next, which the
    estimate reads as extra variance); asserted with a factor 1.5 to either side (the spread of 24 seeds)."""
    seeds, calls = 24, (8,) * 8
    V, r = [], []
    ctx = _context()
    try:
        _setup(ctx, _SMALL[scene](64, 48))
        for s in range(seeds):
            ctx.set_config(RenderConfig(tracing=Tracing(6, 4), seed=1000 + 17 * s).struct())
            ctx.reset()
            for n in calls:
                ctx.render(n)
            v, a = ctx.read_variance(), ctx.read_accum().astype(np.float64)
            assert v[..., 3].max() == len(calls)
            V.append(v[..., 1].astype(np.float64))
            r.append(a[..., 1] / np.maximum(a[..., 3], 1))
    finally:
        ctx.close()
    assert np.abs(r[0] - r[1]).max() > 0, "the seeds gave the same frame"
    estimated, empirical = float(np.mean(V, axis=0).sum()), float(np.var(r, axis=0, ddof=1).sum())
    ratio = estimated / empirical
    print(f"\n{scene}: sum of the mean estimate {estimated:.6g}, sum of the variance over {seeds} seeds {empirical:.6g}, ratio {ratio:.3f}")
    measured = _MEASURED_RATIO[scene]
    assert measured / 1.5 <= ratio <= measured * 1.5


# =====================================================================================================================
# 6. the filter against the restatement
# =====================================================================================================================
_PARAM_SETS = (dict(iterations=5, sigma_color=4.0), dict(iterations=6, sigma_color=1.0, demodulate=False), dict(iterations=1, sigma_color=16.0))


def _device_filter(ctx, accum, guides, variance, params):
    """hiprz_denoise_image_variance on host arrays: (H, W, 4) float32"""
    a, g, v = _hiprt.DeviceBuffer.of(accum.astype(np.float32)), _hiprt.DeviceBuffer.of(guides), _hiprt.DeviceBuffer.of(variance.astype(np.float32))
    d = _hiprt.DeviceBuffer(accum.shape[0] * accum.shape[1] * 16)
    try:
        ctx.denoise_image_variance(a.ptr, g.ptr, v.ptr, params, d.ptr)
        ctx.sync()
        return d.download(accum.shape, np.float32)
    finally:
        a.free(), g.free(), v.free(), d.free()


def _compare_with_restatement(ctx, accum, guides, variance, params, what, pooled=None):
    """`pooled`: a list that collects (what, float32 deviation, device deviation) instead of the assertion of _bar — the caller holds the
    device to the largest float32 deviation of the whole pool (_pooled_bar)"""
    r64 = vref.atrous_variance(accum, guides, variance, params, np.float64)
    r32 = vref.atrous_variance(accum, guides, variance, params, np.float32)
    got = _device_filter(ctx, accum, guides, variance, params)
    assert np.all(got[..., 3] == 1)
    if pooled is not None:
        pooled.append((what, float(np.abs(r32[..., :3].astype(np.float64) - r64[..., :3]).max()), float(np.abs(got[..., :3].astype(np.float64) - r64[..., :3]).max())))
        print(f"\n{what}: float32 restatement deviates from float64 by {pooled[-1][1]:.3e}, the device by {pooled[-1][2]:.3e}")
    else:
        _bar(got[..., :3], r32[..., :3], r64[..., :3], what)
    return got, r64


def _pooled_bar(pooled, what):
    """the project's bar over a pool of frames: every frame's device deviation <= 4 x the largest float32 deviation of the pool, so that a
    frame on which float32 happens to be exact (one pixel, one tap) does not set a bound of zero"""
    dev32 = max(d for _, d, _ in pooled)
    worst = max(pooled, key=lambda r: r[2])
    print(f"{what}: pooled float32 deviation {dev32:.3e} over {len(pooled)} frames, largest device deviation {worst[2]:.3e} ({worst[0]})")
    assert dev32 > 0, what
    assert not [r for r in pooled if r[2] > 4 * dev32], what


def _synthetic(H, W, seed):
    """the recipe of tests/test_denoise_gpu.py's synthetic inputs, and a variance image to go with them"""
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
    variance = np.zeros((H, W, 4), np.float32)
    variance[..., :3] = rng.gamma(2.0, 0.02, (H, W, 3))
    variance[..., 3] = rng.integers(2, 10, (H, W))
    variance[rng.uniform(size=(H, W)) < 0.05, 3] = 1          # no estimate: their V is not to be read
    variance[rng.uniform(size=(H, W)) < 0.03, :3] = 0         # a converged pixel
    return accum, g, variance


def test_filter_equals_the_restatement_on_synthetic_inputs(built):
    ctx = _context(variance=False)
    try:
        _setup(ctx, scenes.cornell_box(173, 99))  # odd sizes: every step leaves partial sub-lattice tiles
        accum, guides, variance = _synthetic(99, 173, 17)
        assert 0.02 < (variance[..., 3] == 1).mean() < 0.08 and (variance[..., :3] == 0).any()
        for kw in _PARAM_SETS:
            params = denoise_params(variance=True, **kw)
            what = f"synthetic iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
            got, _ = _compare_with_restatement(ctx, accum, guides, variance, params, what)
            again = _device_filter(ctx, accum, guides, variance, params)
            assert got.tobytes() == again.tobytes(), "two calls gave different bits"
    finally:
        ctx.close()


# Frames smaller than the filter's reach (tests/test_denoise_gpu.py: SMALL_FRAMES): whole residue classes of the step hold no pixel and
# every tile is a halo.
SMALL_FRAMES = ((1, 1), (64, 3), (3, 64), (17, 41), (33, 33), (5, 3))          # width x height


@pytest.mark.parametrize("sigma_color", [0.0, None])
@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("iterations", [1, 5, 6])
def test_filter_equals_the_restatement_on_small_frames(built, iterations, demodulate, sigma_color):
    ctx = _context(variance=False)
    try:
        params = denoise_params(variance=True, iterations=iterations, demodulate=demodulate, sigma_color=sigma_color)
        pooled = []
        for k, (W, H) in enumerate(SMALL_FRAMES):
            _setup(ctx, scenes.cornell_box(W, H))
            accum, guides, variance = _synthetic(H, W, 31 + k)
            what = f"{W}x{H} iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
            got, _ = _compare_with_restatement(ctx, accum, guides, variance, params, what, pooled)
            assert got.shape == (H, W, 4) and np.isfinite(got).all(), what
            again = _device_filter(ctx, accum, guides, variance, params)
            assert got.tobytes() == again.tobytes(), f"{what}: two calls gave different bits"
        _pooled_bar(pooled, f"small frames iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["single", "two-streams", "samples"])
def test_filter_equals_the_restatement_and_hiprz_denoise_on_a_real_frame(built, kind):
    ctx = _context(kind)
    try:
        _setup(ctx, scenes.cornell_box(250, 150))
        for _ in range(8):
            ctx.render(8)
        accum, guides, variance = ctx.read_accum(), ctx.read_guides(), ctx.read_variance()
        assert variance[..., 3].max() == (16 if kind == "samples" else 8) and (variance[..., :3] > 0).mean() > 0.1
        for kw in _PARAM_SETS:
            params = denoise_params(variance=True, **kw)
            if kind == "single":
                what = f"cornell iterations {params.iterations} sigma_color {params.sigma_color:g} flags {params.flags}"
                want, _ = _compare_with_restatement(ctx, accum, guides, variance, params, what)
            else:
                want = _device_filter(ctx, accum, guides, variance, params)
            ctx.denoise(params)
            assert ctx.read_denoised().tobytes() == want.tobytes(), f"{kind}: hiprz_denoise differs from hiprz_denoise_image_variance on the read images"
            d, out8 = _hiprt.DeviceBuffer.of(want), _hiprt.DeviceBuffer(want.shape[0] * want.shape[1] * 4)
            ctx.tonemap_image(d.ptr, out8.ptr)
            ctx.sync()
            assert np.array_equal(out8.download(want.shape, np.uint8), ctx.read_denoised_rgba8())
            d.free(), out8.free()
        plain = denoise_params(**_PARAM_SETS[0])
        ctx.denoise(plain)
        assert ctx.read_denoised().tobytes() != want.tobytes()
    finally:
        ctx.close()


def test_misses_at_an_infinite_far_plane_stay_finite_under_the_flag(built):
    ctx = _context(variance=False)
    try:
        _setup(ctx, scenes.cornell_box(120, 72))
        accum, guides, variance = _synthetic(72, 120, 23)
        miss = guides["instance"] == _abi.GUIDE_MISS
        assert miss.sum() > 200
        guides["depth"][miss] = np.inf
        got, r64 = _compare_with_restatement(ctx, accum, guides, variance, denoise_params(variance=True, sigma_color=4.0), "misses at infinity")
        assert np.isfinite(got).all() and np.isfinite(r64).all()
        assert got[miss][..., :3].std() < 0.7 * (accum[miss][..., :3] / np.maximum(accum[miss][..., 3:4], 1)).std(), "the sky was not smoothed"
    finally:
        ctx.close()


# =====================================================================================================================
# 7. errors
# =====================================================================================================================
def test_argument_and_state_errors(built):
    ctx = _context(variance=False)
    try:
        flagged, plain = denoise_params(variance=True, sigma_color=4.0), denoise_params()
        for call in (ctx.read_variance, ctx.variance_device):
            with pytest.raises(HiprzError) as e:
                call()
            assert e.value.code == _abi.ERR_STATE  # off
        ctx.set_variance(1)
        for call in (ctx.read_variance, ctx.variance_device):
            with pytest.raises(HiprzError) as e:
                call()
            assert e.value.code == _abi.ERR_STATE  # before scene and camera
        ctx.set_variance(0)
        _setup(ctx, _SMALL["cornell"]())
        ctx.render(2), ctx.render(2)
        with pytest.raises(HiprzError) as e:
            ctx.denoise(flagged)
        assert e.value.code == _abi.ERR_STATE and "hiprz_set_variance" in str(e.value)
        ctx.set_denoise(flagged)  # accepted: present() then reports the same
        with pytest.raises(HiprzError) as e:
            ctx.present(0, 0)
        assert e.value.code == _abi.ERR_STATE and "hiprz_set_variance" in str(e.value)
        ctx.set_denoise(None)
        n = ctx.width * ctx.height
        a, d, v = _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer(n * 16)
        try:
            for args in ((a.ptr, None, v.ptr, plain, d.ptr),      # the flag is not set
                         (a.ptr, None, v.ptr, None, d.ptr),       # ... nor do the defaults carry it
                         (a.ptr, None, None, flagged, d.ptr),     # no variance image
                         (a.ptr, None, d.ptr, flagged, d.ptr),    # ... or one that aliases the destination
                         (a.ptr, None, v.ptr, flagged, a.ptr),    # the accumulator image aliases it
                         (None, None, v.ptr, flagged, d.ptr)):
                with pytest.raises(HiprzError) as e:
                    ctx.denoise_image_variance(*args)
                assert e.value.code == _abi.ERR_INVALID, args
            with pytest.raises(HiprzError) as e:
                ctx.denoise_image(a.ptr, None, flagged, d.ptr)
            assert e.value.code == _abi.ERR_INVALID
            for flags in (4, 4 | _abi.DENOISE_VARIANCE):
                bad = denoise_params(sigma_color=4.0)
                bad.flags = flags
                for call in (lambda: ctx.denoise(bad), lambda: ctx.set_denoise(bad), lambda: ctx.denoise_image_variance(a.ptr, None, v.ptr, bad, d.ptr)):
                    with pytest.raises(HiprzError) as e:
                        call()
                    assert e.value.code == _abi.ERR_INVALID
        finally:
            a.free(), d.free(), v.free()
        ctx.set_variance(1)
        small = np.zeros(7, np.float32)
        assert ctx.lib.hiprz_read_variance(ctx._ctx, small.ctypes.data, small.nbytes) == _abi.ERR_INVALID, "size mismatch"
    finally:
        ctx.close()


# =====================================================================================================================
# 8. quality
# =====================================================================================================================
_QUALITY = {
    "cornell": (lambda: scenes.cornell_box(960, 540), LightSampling()),
    "lights and maps": (lambda: scenes.shading_inputs_scene(960, 540, lights=True), LightSampling(2, 2)),
}


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.mark.parametrize("scene", sorted(_QUALITY))
def test_variance_guided_frame_is_closer_to_the_reference_than_the_raw_frame(built, scene):
    """The protocol of test_denoised_frame_is_closer_to_the_reference_than_the_raw_frame: N = 64 passes, rendered as 8 calls of 8, against
    the unchanged renderer at 64 * N passes (another seed, 64 calls), RMSE over the tone-mapped image before quantisation, the
    variance-guided filter at sigma_color = 4.  The ratio of the default filter on the same frame is printed beside it."""
    build, sampling = _QUALITY[scene]
    world = build()
    N = 64
    noisy, clean = _context(), _context()
    try:
        for ctx, seed in ((noisy, 20240501), (clean, 977)):
            flat, cam = flatten(world), camera_struct(world.camera)
            ctx.upload_scene(flat), ctx.upload_camera(cam)
            ctx.set_config(RenderConfig(sampling, Tracing(8, N), seed=seed).struct())
        for _ in range(8):
            noisy.render(N // 8)
        for _ in range(64):
            clean.render(N)
        assert noisy.pass_count() == N and clean.pass_count() == 64 * N
        tm = lambda image: ref.tonemap_unquantised(image, cam.aperture, cam.exposure_time)  # noqa: E731
        reference = tm(clean.read_accum())
        raw = _rmse(tm(noisy.read_accum()), reference)
        noisy.denoise()
        default = _rmse(tm(noisy.read_denoised()), reference)
        flagged = denoise_params(variance=True, sigma_color=4.0)
        noisy.denoise(flagged), clean.denoise(flagged)
        denoised = _rmse(tm(noisy.read_denoised()), reference)
        blur = _rmse(tm(clean.read_denoised()), reference)
        print(f"\n{scene}: RMSE raw {N}-pass frame {raw:.5f}, variance-guided {denoised:.5f} (ratio {denoised / raw:.3f}; the default filter on the same "
              f"frame {default / raw:.3f}), variance-guided reference {blur:.5f} (ratio to raw {blur / raw:.3f})")
        assert denoised < raw, "the filter did not bring the noisy frame closer to the reference"
        assert blur <= raw, "the blur the filter adds to a clean frame exceeds the noise it removes"
    finally:
        noisy.close(), clean.close()


# =====================================================================================================================
# 9. delivery
# =====================================================================================================================
@pytest.mark.parametrize("pipelined", [False, True])
def test_python_engine_delivers_variance_guided_frames(built, pipelined):
    params = denoise_params(variance=True, sigma_color=4.0)
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
        assert engine.context.read_variance()[..., 3].max() == 4, "the engine's calls were not one batch each"
        twin.denoise(denoise_params(sigma_color=4.0))
        assert not np.array_equal(expected[-1], twin.read_denoised_rgba8()), "the flag changed nothing"
        engine.set_denoise(None)  # the estimate goes off with the flag: accumulation restarts
        engine.renderWorld(world, cfg, sync=True)
        with pytest.raises(HiprzError):
            engine.context.read_variance()
        twin.set_variance(0)
        twin.render(3), twin.tonemap()
        assert twin.pass_count() == 3
        assert np.array_equal(world.camera.image_buffer, twin.read_rgba8())
    finally:
        twin.close()
        engine.context.close()


def test_cpp_engine_delivers_variance_guided_frames(built, tmp_path):
    exe = str(tmp_path / "variance_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "variance_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "VARIANCE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_headless_runner_takes_the_variance_key(built, tmp_path):
    """The runner sizes its calls by the clock, so the batches — and with them the filtered frame's bits — differ from run to run: what is
    checked is that the key is taken, that the frame is a filtered one, and that the passes are the plain task's."""
    world = scenes.cornell_box(128, 96)
    scene_io.save_scene_json(world, str(tmp_path / "cornell.json"))
    exe = os.path.join(CSRC, "hiprz_headless")
    frames = {}
    for name, key in (("plain", ""), ("variance", ', "denoise": "variance"')):
        (tmp_path / f"{name}.json").write_text('{"tasks": [{"scene path": "cornell.json", "engine": ["HIPGPU"], "rpp": 20, "timeout": 60.0, "max depth": 4' + key + "}]}")
        out_dir = tmp_path / name
        r = subprocess.run([exe, "--headless", str(tmp_path / f"{name}.json"), str(out_dir), "-r", "--quiet"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        images = [f for f in os.listdir(out_dir) if f.endswith("_HIPGPU.png")]
        assert len(images) == 1
        frames[name] = scene_io.read_image(str(out_dir / images[0])).astype(np.float64)
    assert frames["plain"].shape == frames["variance"].shape == (96, 128, 4)
    assert not np.array_equal(frames["plain"], frames["variance"])

    def roughness(image):  # mean absolute difference of horizontal neighbours: what a filter lowers
        return float(np.abs(np.diff(image[..., :3], axis=1)).mean())

    print(f"\nheadless: neighbour differences plain {roughness(frames['plain']):.3f}, variance-guided {roughness(frames['variance']):.3f}")
    assert roughness(frames["variance"]) < roughness(frames["plain"])
    (tmp_path / "bad.json").write_text('{"tasks": [{"scene path": "cornell.json", "denoise": "varianse"}]}')
    r = subprocess.run([exe, "--headless", str(tmp_path / "bad.json"), "--quiet"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "denoise" in r.stdout + r.stderr
