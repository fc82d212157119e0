"""The noise level of a frame (include/hiprz_noise.h: libhiprz_noise.so, hiprz_accum_device, Context.noise, Engine.render_until and the
C++ hosts) on the GPU: against the numpy restatement (tests/noise_reference.py), against the spread of the unchanged renderer over
independent seeds, and through every host.  Every figure a bound is compared with is printed before the assert (pytest -s shows them;
DESIGN.md "Noise level" quotes them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as ref
import noise_reference as nref
from rayzath_amd import _abi, _hiprt, noise, scene_io, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import SHARD_SAMPLES, Context, Engine, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")

pytestmark = pytest.mark.gpu

_SMALL = {
    "cornell": lambda w=80, h=48: scenes.cornell_box(w, h),
    "lights": lambda w=80, h=48: scenes.shading_inputs_scene(w, h, lights=True),
}
_CALLS = (1, 3, 8, 8, 2, 8) + (8,) * 4
_CAM = dict(aperture=0.02, exposure_time=1.0 / 60.0)


def _context(kind="single", variance=True):
    ctx = Context(0) if kind in ("single", "split") else Context([0, 0])
    if kind == "samples":
        ctx.set_shard_mode(SHARD_SAMPLES)
    if kind == "split":
        ctx.set_pipeline(1)
    if variance:
        ctx.set_variance(1)
    return ctx


def _setup(ctx, world, depth=6, rpp=4, seed=20240501):
    flat, cam = flatten(world), camera_struct(world.camera)
    ctx.upload_scene(flat), ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(None, Tracing(depth, rpp), seed=seed).struct())
    return flat, cam


def _bar(got, r32, r64, what):
    """the project's bar: the device's largest deviation from the float64 restatement is at most four times the float32 restatement's"""
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, r32, r64))
    dev32 = float(np.abs(r32 - r64).max())
    dev_gpu = float(np.abs(got - r64).max())
    print(f"\n{what}: float32 restatement deviates from float64 by {dev32:.3e}, the device by {dev_gpu:.3e} "
          f"(ratio {dev_gpu / dev32 if dev32 else float('inf') if dev_gpu else 0.0:.2f}, values up to {np.abs(r64).max():.3g})")
    assert dev_gpu <= 4 * dev32, what


def _against_the_restatement(summary, tiles, accum, variance, aperture, exposure_time, what, threshold=1.0 / 255.0, min_batches=8):
    """a device measurement (noise.Summary, tiles) against both restatements on the same images"""
    s32, t32 = nref.measure(accum, variance, aperture, exposure_time, threshold, min_batches, np.float32)
    s64, t64 = nref.measure(accum, variance, aperture, exposure_time, threshold, min_batches, np.float64)
    got = summary.as_dict()
    assert tiles.shape == t32.shape and tiles.dtype == np.float32
    assert np.array_equal(tiles[..., 2:], t32[..., 2:]), f"{what}: the tiles' counts differ from the restatement's"
    for name in ("estimated", "above", "pixels", "tiles_x", "tiles_y", "worst_tile"):
        assert got[name] == s32[name], (what, name, got[name], s32[name])
    print(f"\n{what}: {got['estimated']} of {got['pixels']} pixels estimated, {got['above']} above the threshold, rms {got['rms']:.6g}, tile rms max "
          f"{got['tile_rms_max']:.6g} in tile {got['worst_tile']} (the float64 restatement's worst tile: {s64['worst_tile']}), max {got['max']:.6g}; tile records "
          f"bit-equal to the float32 restatement: {tiles.tobytes() == t32.tobytes()}")
    assert np.isfinite(tiles).all()
    _bar(tiles[..., 0], t32[..., 0], t64[..., 0], f"{what}: sum of e^2 per tile")
    _bar(tiles[..., 1], t32[..., 1], t64[..., 1], f"{what}: max of e per tile")
    names = ("rms", "tile_rms_max", "max")
    _bar([got[n] for n in names], [s32[n] for n in names], [s64[n] for n in names], f"{what}: rms, tile rms max, max of the summary")
    return got


# =====================================================================================================================
# 1. synthetic images against the restatement
# =====================================================================================================================
def _synthetic(H, W, seed):
    """after the recipe of tests/test_variance_gpu.py's synthetic inputs: K from 0 to 9, pixels without a finished path, converged pixels,
    one infinite variance"""
    rng = np.random.default_rng(seed)
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., 3] = rng.integers(0, 9, (H, W))               # some pixels have no finished path: A = 0
    accum[..., :3] = rng.gamma(2.0, 0.5, (H, W, 3)) * np.maximum(accum[..., 3:4], 1)
    variance = np.zeros((H, W, 4), np.float32)
    variance[..., :3] = rng.gamma(2.0, 0.02, (H, W, 3))
    variance[..., 3] = rng.integers(0, 10, (H, W))
    variance[rng.uniform(size=(H, W)) < 0.03, :3] = 0         # a converged pixel
    if H * W > 1:
        variance[H // 2, W // 3, 1], variance[H // 2, W // 3, 3] = np.inf, 9   # e is not finite: no estimate, whatever K says
    else:
        accum[0, 0, 3], variance[0, 0, 3] = 2, 9               # the one pixel has an estimate
    return accum, variance


@pytest.mark.parametrize("size", [(173, 99), (32, 8), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_images_equal_the_restatement(built, size):
    W, H = size
    accum, variance = _synthetic(H, W, 17 + W)
    if W > 32:
        assert (accum[..., 3] == 0).any() and (variance[..., :3] == 0).all(-1).any() and np.isinf(variance).sum() == 1
        assert set(np.unique(variance[..., 3])) == set(range(10))
    meter = noise.Meter(0)
    a, v = _hiprt.DeviceBuffer.of(accum), _hiprt.DeviceBuffer.of(variance)
    tx, ty = noise.tile_grid(W, H)
    out = _hiprt.DeviceBuffer(tx * ty * 16)
    try:
        for min_batches in (4, 8):
            params = noise.Params(_CAM["aperture"], _CAM["exposure_time"], 1.0 / 255.0, min_batches)
            summary, tiles = meter.measure(a.ptr, v.ptr, W, H, params)
            got = _against_the_restatement(summary, tiles, accum, variance, **_CAM, what=f"synthetic {W}x{H} min_batches {min_batches}", min_batches=min_batches)
            assert 0 < got["estimated"] < got["pixels"] or W == 1
            again_summary, again = meter.measure(a.ptr, v.ptr, W, H, params)
            assert again.tobytes() == tiles.tobytes() and bytes(again_summary) == bytes(summary), "two calls gave different bits"
            meter.tiles(a.ptr, v.ptr, W, H, params, out.ptr)  # enqueue only, into the caller's buffer
            assert out.download(tiles.shape, np.float32).tobytes() == tiles.tobytes(), "hiprz_noise_tiles differs from hiprz_noise_measure"
            assert bytes(noise.summarise(tiles, W, H)) == bytes(summary)
    finally:
        a.free(), v.free(), out.free()
        meter.close()


# =====================================================================================================================
# 2. real frames
# =====================================================================================================================
def _device_image(ctx, pointer, shape):
    image = np.zeros(shape, np.float32)
    ctx.sync()
    assert _hiprt.runtime().hipMemcpy(image.ctypes.data, C.c_void_p(pointer), image.nbytes, 2) == 0
    return image


@pytest.mark.parametrize("scene", sorted(_SMALL))
def test_real_frames_equal_the_restatement(built, scene):
    ctx = _context()
    try:
        _, cam = _setup(ctx, _SMALL[scene]())
        for n in _CALLS:
            ctx.render(n)
        image = _device_image(ctx, ctx.accum_device(), (ctx.height, ctx.width, 4))
        accum, variance = ctx.read_accum(), ctx.read_variance()
        assert image.tobytes() == accum.tobytes(), "hiprz_accum_device is not the image hiprz_read_accum returns"
        assert variance[..., 3].max() >= len(_CALLS) - 1
        summary, tiles = ctx.noise(min_batches=6)  # (the calls of 1, 3 and 2 passes close no batch where no path finished in them)
        got = _against_the_restatement(summary, tiles, accum, variance, cam.aperture, cam.exposure_time, scene, min_batches=6)
        assert got["estimated"] > 0.5 * got["pixels"] and got["tile_rms_max"] > 0
        assert ctx.read_accum().tobytes() == accum.tobytes() and ctx.read_variance().tobytes() == variance.tobytes(), "measuring changed the images"
        strict, _ = ctx.noise(threshold=0.0, min_batches=len(_CALLS) + 1)
        assert strict.estimated == 0 and strict.rms == 0 and strict.tile_rms_max == 0
    finally:
        ctx.close()


# =====================================================================================================================
# 3. parts
# =====================================================================================================================
def test_two_streams_in_tile_mode_give_the_one_part_measurement(built):
    results = {}
    for kind in ("single", "two-streams"):
        ctx = _context(kind)
        try:
            _setup(ctx, _SMALL["cornell"](250, 150))  # frame edges inside tiles
            for n in _CALLS:
                ctx.render(n)
            summary, tiles = ctx.noise()
            results[kind] = (bytes(summary), tiles.tobytes())
            assert summary.estimated > 0 and (summary.tiles_x, summary.tiles_y) == (8, 19)
        finally:
            ctx.close()
    assert results["single"] == results["two-streams"]


def test_sample_mode_equals_the_restatement_on_its_own_reads(built):
    ctx = _context("samples")
    try:
        _, cam = _setup(ctx, _SMALL["lights"]())
        for n in _CALLS:
            ctx.render(n)
        accum, variance = ctx.read_accum(), ctx.read_variance()
        assert variance[..., 3].max() == 2 * len(_CALLS)
        assert _device_image(ctx, ctx.accum_device(), accum.shape).tobytes() == accum.tobytes(), "hiprz_accum_device is not the summed accumulator"
        summary, tiles = ctx.noise(min_batches=12)
        got = _against_the_restatement(summary, tiles, accum, variance, cam.aperture, cam.exposure_time, "sample mode", min_batches=12)
        assert got["estimated"] > 0.5 * got["pixels"]
    finally:
        ctx.close()


# =====================================================================================================================
# 4. measuring changes nothing else
# =====================================================================================================================
@pytest.mark.parametrize("kind", ["single", "two-streams", "split"])
def test_measuring_changes_nothing_else(built, kind):
    results = []
    for measure in (True, False):
        ctx = _context(kind)
        try:
            if kind == "split":
                _setup(ctx, scenes.cornell_box(96, 64))
                calls = (4, 4, 4, 4)
            else:
                _setup(ctx, _SMALL["lights"]())
                calls = _CALLS
            for k, n in enumerate(calls):
                ctx.render(n)
                if measure and k + 1 < len(calls):
                    ctx.noise(min_batches=2)
            ctx.tonemap()
            results.append((ctx.read_accum().tobytes(), ctx.read_rgba8().tobytes(), ctx.read_depth().tobytes(), ctx.read_variance().tobytes(), ctx.ray_count(),
                            ctx.pass_count(), ctx.graph_captures()))
        finally:
            ctx.close()
    for name, a, b in zip(("accum", "rgba8", "depth", "variance", "ray_count", "pass_count", "graph_captures"), *results):
        assert a == b, f"{kind}: {name} differs once the frame is measured between the render calls"
    if kind == "split":
        assert results[0][6] >= 1, "the split pipeline was meant to replay a captured graph"


# =====================================================================================================================
# 5. calibration against the spread over seeds
# =====================================================================================================================
_MEASURED_RATIO = {"cornell": 0.064, "lights": 0.994}  # MI355X, 64 x 48, 24 seeds of 8 calls of 8 passes (the docstring below)


@pytest.mark.parametrize("scene", sorted(_SMALL))
def test_predicted_error_is_calibrated_against_the_spread_over_seeds(built, scene):
    """mean over seeds of the predicted rms^2 / mean over pixels of the variance, across 24 independent seeds of the unchanged renderer, of
    the displayed luminance lum(t(r)) (tests/denoise_reference.tonemap_unquantised), each seed 8 calls of 8 passes at 64 x 48.  1 for an
    exact prediction.  Measured on MI355X: lights and maps 0.994 (next-event estimation: every path brings light, a pixel's radiance is
    near Gaussian after 64 passes and its spread is small against the knee of the tone curve); Cornell 0.064 — the prediction is 16 times
    too small in variance.  There light arrives only by paths that happen to hit the small emitter: a pixel's radiance after 64 passes is
    a handful of rare, very bright paths (k r of the order of 100, t(r) near 1) or none (r = 0, V = 0, e = 0), its displayed value jumps
    between black and white from seed to seed (variance 0.114: a standard deviation of a third of the display range), and the slope of the
    tone curve at the pixel's own mean says nothing about a spread that wide.  V itself is calibrated on that frame
    (test_estimate_is_calibrated_against_the_variance_over_seeds: 1.022): what fails is the linearisation through t, where the noise is
    wider than the curve's knee.  The figure is a lower bound on such frames and hosts must not stop on it before the passes are many
    (DESIGN.md "Noise level").  Asserted with the factor 1.5 to either side that
    test_estimate_is_calibrated_against_the_variance_over_seeds uses for the same 24-seed spread."""
    seeds, calls = 24, (8,) * 8
    predicted, shown, share = [], [], []
    ctx = _context()
    try:
        _, cam = _setup(ctx, _SMALL[scene](64, 48))
        for s in range(seeds):
            ctx.set_config(RenderConfig(tracing=Tracing(6, 4), seed=1000 + 17 * s).struct())
            ctx.reset()
            for n in calls:
                ctx.render(n)
            summary, _ = ctx.noise(min_batches=len(calls))
            predicted.append(summary.rms ** 2)
            share.append(summary.estimated / summary.pixels)
            t = ref.tonemap_unquantised(ctx.read_accum(), cam.aperture, cam.exposure_time)
            shown.append((0.2126 * t[..., 0] + 0.7152 * t[..., 1]) + 0.0722 * t[..., 2])
    finally:
        ctx.close()
    assert np.abs(shown[0] - shown[1]).max() > 0, "the seeds gave the same frame"
    empirical = float(np.var(shown, axis=0, ddof=1).mean())
    ratio = float(np.mean(predicted)) / empirical
    print(f"\n{scene}: mean predicted rms^2 {np.mean(predicted):.6g} (rms {np.sqrt(np.mean(predicted)):.5f}), mean variance over {seeds} seeds {empirical:.6g}, "
          f"ratio {ratio:.3f}; estimated share {min(share):.4f} .. {max(share):.4f}")
    measured = _MEASURED_RATIO[scene]
    assert measured / 1.5 <= ratio <= measured * 1.5


# =====================================================================================================================
# 6. more passes, less noise
# =====================================================================================================================
def test_the_noise_level_falls_with_the_passes(built):
    """On the scene with lights, whose prediction is calibrated (above).  Not on the Cornell box: there a pixel's radiance is a handful of rare,
    very bright paths into the small emitter, far past the knee of the tone curve, and the linearised figure of such a pixel is about
    N / (k h) after its first hit h in N paths — it RISES with the passes until k h / N falls to about 1.  Measured on MI355X, Cornell
    80 x 48, depth 4, calls of 4 passes: tile rms max 0.0716 after 8 calls, 0.1424 after 32, 0.1381 after 128 (rms 0.0520, 0.1227, 0.1213)."""
    ctx = _context()
    try:
        _setup(ctx, _SMALL["lights"](), depth=4)
        figures = []
        for calls in range(1, 129):
            ctx.render(4)
            if calls in (8, 32, 128):
                s, _ = ctx.noise()
                figures.append((s.tile_rms_max, s.rms, s.estimated, s.pixels))
    finally:
        ctx.close()
    for (t0, r0, _, _), (t1, r1, _, _), step in zip(figures, figures[1:], ("8 -> 32", "32 -> 128")):
        print(f"\n{step} calls of 4 passes: tile rms max {t0:.5f} -> {t1:.5f} (ratio {t1 / t0:.3f}), rms {r0:.5f} -> {r1:.5f} (ratio {r1 / r0:.3f}); theory: 0.5")
    print(f"\nestimated pixels: {[f[2] for f in figures]} of {figures[0][3]}")
    assert figures[0][0] > figures[1][0] > figures[2][0] > 0
    assert figures[0][1] > figures[1][1] > figures[2][1] > 0


# =====================================================================================================================
# 7. the Python engine renders to a target
# =====================================================================================================================
def test_engine_renders_until_the_target_is_met(built):
    rpp, first = 4, 8  # (max depth 4: every call of 4 passes finishes a path in every pixel, so every call closes a batch everywhere)
    cfg = RenderConfig(tracing=Tracing(4, rpp))
    world = _SMALL["lights"](96, 64)  # (the scene whose prediction is calibrated and falls with the passes: see the two tests above)
    engine, twin = Engine(0, streams=1), _context()
    try:
        _setup(twin, _SMALL["lights"](96, 64), depth=4, rpp=rpp)
        for _ in range(first):
            twin.render(rpp)
        n8, _ = twin.noise()
        assert n8.estimated == n8.pixels and n8.tile_rms_max > 0
        target, max_passes = n8.tile_rms_max / 2, 16 * first * rpp
        summary, passes, met = engine.render_until(world, cfg, target, max_passes)
        print(f"\nafter {first} calls of {rpp} passes: tile rms max {n8.tile_rms_max:.5f}; render_until({target:.5f}) took {passes} passes and ended at {summary.tile_rms_max:.5f}")
        assert met and first * rpp < passes < max_passes and passes % rpp == 0
        assert summary.estimated == summary.pixels and summary.tile_rms_max <= target
        assert engine.context.pass_count() == passes
        for _ in range(passes // rpp - first):
            twin.render(rpp)
        twin.tonemap()
        assert np.array_equal(world.camera.image_buffer, twin.read_rgba8()), "the measured frame is not the frame of the same calls without measurements"
        assert engine.context.read_accum().tobytes() == twin.read_accum().tobytes()
        assert bytes(twin.noise()[0]) == bytes(summary)
        # the estimate stays on, and a second call goes on from the frame it has
        assert engine.context.read_variance()[..., 3].max() == passes // rpp
        _, more, met_again = engine.render_until(world, cfg, target, rpp)
        assert met_again and more == rpp and engine.context.pass_count() == passes + rpp
    finally:
        twin.close()
        engine.context.close()
    world, engine = _SMALL["lights"](96, 64), Engine(0, streams=1)
    try:
        summary, passes, met = engine.render_until(world, cfg, 0.0, 10 * rpp)
        assert not met and passes == 10 * rpp and summary.estimated == summary.pixels and summary.tile_rms_max > 0
        engine.context.set_shard(0, 2)  # one shard of a frame: the context does not hold it
        with pytest.raises(HiprzError) as e:
            engine.render_until(world, cfg, 1.0, rpp)
        assert e.value.code == _abi.ERR_STATE and "shard" in str(e.value)
    finally:
        engine.context.close()


def test_render_until_switches_the_estimate_on_and_keeps_a_denoiser_from_switching_it_off(built):
    cfg = RenderConfig(tracing=Tracing(4, 4))
    world, engine = scenes.cornell_box(64, 48), Engine(0)
    try:
        engine.renderWorld(world, cfg), engine.renderWorld(world, cfg)
        with pytest.raises(HiprzError):
            engine.context.read_variance()
        summary, passes, met = engine.render_until(world, cfg, 1.0, 64, min_batches=2)  # (a target of the whole display range: met at the first measurement)
        assert met and passes == 8 and engine.context.pass_count() == 8, "switching the estimate on restarts accumulation"
        engine.set_denoise(None)
        engine.renderWorld(world, cfg)
        assert engine.context.pass_count() == 12 and engine.context.read_variance()[..., 3].max() == 3, "set_denoise switched the estimate off under a measuring engine"
    finally:
        engine.context.close()


# =====================================================================================================================
# 8. delivery through the C++ hosts
# =====================================================================================================================
def test_cpp_engine_renders_until_the_target_is_met(built, tmp_path):
    exe = str(tmp_path / "noise_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "noise_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "NOISE DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_headless_runner_takes_the_noise_key(built, tmp_path):
    world = scenes.cornell_box(128, 96)
    scene_io.save_scene_json(world, str(tmp_path / "cornell.json"))
    ctx = _context()
    try:
        _setup(ctx, scenes.cornell_box(128, 96), depth=4)
        for _ in range(8):
            ctx.render(8)
        n8, _ = ctx.noise()
    finally:
        ctx.close()
    assert n8.estimated == n8.pixels
    target, budget = n8.tile_rms_max / 2, 1000000
    exe = os.path.join(CSRC, "hiprz_headless")
    task = '{"tasks": [{"scene path": "cornell.json", "engine": ["HIPGPU"], "rpp": %d, "timeout": 60.0, "max depth": 4%s}]}'

    def run(name, rpp, key):
        (tmp_path / f"{name}.json").write_text(task % (rpp, key))
        r = subprocess.run([exe, "--headless", str(tmp_path / f"{name}.json"), str(tmp_path / name), "--quiet"], capture_output=True, text=True, timeout=300)
        return r, ((tmp_path / name / "report.txt").read_text() if r.returncode == 0 else "")

    r, report = run("target", budget, f', "noise": {target:.9g}')
    assert r.returncode == 0, r.stdout + r.stderr
    print("\n" + report)
    lines = report.splitlines()
    assert len(lines) == 4 and lines[3].startswith("\tnoise: tile rms max ")
    m = re.fullmatch(r"\tnoise: tile rms max ([0-9.]+) \| rms ([0-9.]+) \| estimated ([0-9.]+)% \| target ([0-9.]+) (met|not met) \| (\d+) passes", lines[3])
    assert m, lines[3]
    assert m.group(5) == "met" and float(m.group(3)) == 100.0 and float(m.group(1)) <= float(m.group(4)) + 1e-5 and float(m.group(2)) <= float(m.group(1))
    assert 8 <= int(m.group(6)) < budget, "the task was meant to stop at the target, long before its rpp"
    r, report = run("plain", 20, "")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = report.splitlines()
    assert len(lines) == 3 and "noise" not in report and lines[0] == "Scene: cornell.json" and lines[1].startswith("\tengine: HIPGPU") and lines[2].startswith("\tduration: ")
    for bad in ('"low"', "0", "-0.5", "true"):
        r, _ = run("bad", 20, f', "noise": {bad}')
        assert r.returncode != 0 and "noise" in r.stdout + r.stderr, bad


# =====================================================================================================================
# 9. errors
# =====================================================================================================================
def test_argument_and_state_errors(built):
    ctx = _context(variance=False)
    meter = noise.Meter(0)
    lib = noise.load()
    try:
        out = C.c_void_p()
        for call in (ctx.accum_device, ctx.noise):
            with pytest.raises(HiprzError) as e:
                call()
            assert e.value.code == _abi.ERR_STATE  # before scene and camera (noise: the estimate is off)
        ctx.set_variance(1)
        with pytest.raises(HiprzError) as e:
            ctx.noise()
        assert e.value.code == _abi.ERR_STATE  # the estimate is on, but there is no scene
        ctx.set_variance(0)
        _setup(ctx, _SMALL["cornell"]())
        ctx.render(2), ctx.render(2)
        assert ctx.lib.hiprz_accum_device(ctx._ctx, None) == _abi.ERR_INVALID
        assert ctx.lib.hiprz_accum_device(None, C.byref(out)) == _abi.ERR_INVALID
        assert ctx.accum_device()
        with pytest.raises(HiprzError) as e:
            ctx.noise()
        assert e.value.code == _abi.ERR_STATE and "hiprz_set_variance" in str(e.value)
        ctx.set_variance(1)
        ctx.render(2), ctx.render(2)
        for kw in (dict(min_batches=1), dict(min_batches=0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf"))):
            with pytest.raises(HiprzError) as e:
                ctx.noise(**kw)
            assert e.value.code == _abi.ERR_INVALID, kw
        assert ctx.noise(min_batches=2)[0].estimated > 0

        W, H = 45, 20
        n = W * H
        a, v, t = _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer(6 * 16)
        try:
            good = noise.Params(0.02, 1.0 / 60.0, 1.0 / 255.0, 8)
            summary = noise.Summary()

            def both(accum, variance, width, height, params, tiles_out=t.ptr):
                p = None if params is None else C.byref(params)
                return (lib.hiprz_noise_tiles(meter._meter, accum, variance, width, height, p, tiles_out, None),
                        lib.hiprz_noise_measure(meter._meter, accum, variance, width, height, p, None, C.byref(summary), None))

            assert both(a.ptr, v.ptr, W, H, good) == (_abi.OK, _abi.OK)
            for args in ((None, v.ptr, W, H, good), (a.ptr, None, W, H, good), (a.ptr, v.ptr, 0, H, good), (a.ptr, v.ptr, W, 0, good), (a.ptr, v.ptr, W, H, None)):
                assert both(*args) == (_abi.ERR_INVALID, _abi.ERR_INVALID), args
            for field, value in (("min_batches", 1), ("min_batches", 0), ("threshold", -1.0e-3), ("threshold", float("nan")), ("threshold", float("inf")),
                                 ("aperture", -0.02), ("aperture", float("nan")), ("aperture", float("inf")), ("exposure_time", -1.0),
                                 ("exposure_time", float("nan")), ("exposure_time", float("inf"))):
                bad = noise.Params(0.02, 1.0 / 60.0, 1.0 / 255.0, 8)
                setattr(bad, field, value)
                assert both(a.ptr, v.ptr, W, H, bad) == (_abi.ERR_INVALID, _abi.ERR_INVALID), (field, value)
                assert lib.hiprz_noise_last_error(meter._meter)
            # the output: null, or inside one of the images
            for tiles_out in (None, a.ptr, C.c_void_p(v.ptr.value + 16 * (n - 1))):
                assert lib.hiprz_noise_tiles(meter._meter, a.ptr, v.ptr, W, H, C.byref(good), tiles_out, None) == _abi.ERR_INVALID
            assert lib.hiprz_noise_measure(meter._meter, a.ptr, v.ptr, W, H, C.byref(good), None, None, None) == _abi.ERR_INVALID  # no summary
            ctx.sync()
        finally:
            a.free(), v.free(), t.free()
        other = C.c_void_p()
        assert lib.hiprz_noise_create(C.byref(other), 4096) == _abi.ERR_DEVICE and not other
        assert lib.hiprz_noise_create(C.byref(other), -1) == _abi.ERR_DEVICE and not other
    finally:
        meter.close()
        ctx.close()
