"""Lightmap smoothing without a GPU: the numpy restatement (tests/smooth_reference.py) of include/hiprz_smooth.h against known answers, the
no-leak property, the mutants its inputs must tell apart, and what it does to a real Monte-Carlo penumbra.  Run with -s for the figures.

MEASURED (test_it_denoises_a_penumbra: a 64 x 64 floor under a spot light of size 0.4 whose light a square occluder cuts, the light
restatement's bake at K = 4 against its bake at K = 256, smoothed at smooth.params()'s defaults): RMS error 0.0650 raw, 0.0376 smoothed,
a ratio of 0.58 (the light peaks at 1.12).  With radius = 0.5 on top of the defaults 0.0326."""
import numpy as np
import pytest

import light_reference as LR
import smooth_reference as SR
from rayzath_amd import bake, smooth
from rayzath_amd.scene import SpotLight, World, flatten

F = np.float32
# the sizes tests/test_smooth_gpu.py runs: below the reach of every step, at the block edge, and off it in both axes
SIZES = ((1, 1), (1, 7), (5, 3), (16, 16), (17, 33), (64, 64), (67, 131))


def _flat(W, H, rgb, word=5):
    """one chart on the plane y = 0 with the texel grid as positions"""
    x, z = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    points = bake.points(np.stack([x, np.zeros_like(x), z], -1).reshape(-1, 3), np.tile([0.0, 1.0, 0.0], (W * H, 1)), 1e-3, 1e3).reshape(H, W)
    records = np.zeros((H, W), SR.record_dtype)
    records["rgb"], records["word"] = rgb, word
    return points, records


def test_a_single_texel_comes_back():
    points, records = _flat(1, 1, (0.25, 3.0, 1e-3), 77)
    for kw in (dict(), SR.PARAMS, dict(iterations=8, **SR.PARAMS)):
        assert SR.smooth(points, records, **kw).tobytes() == records.tobytes(), kw
    points["normal"] = 0
    assert SR.smooth(points, records, **SR.PARAMS).tobytes() == records.tobytes()


def test_a_constant_field_stays_within_64_ulp():
    """num is at most 25 products and 24 additions of positive terms per colour, den 24 additions, then one division: each within half an
    ulp of a result that only grows, (25 + 24 + 24 + 1) / 2 = 37 ulp, rounded up to a power of two"""
    value = np.array([0.7, 1.9, 123.456], F)
    points, records = _flat(23, 19, value)
    for kw in (dict(iterations=1), dict(iterations=4), dict(iterations=5, **SR.PARAMS)):
        out = SR.smooth(points, records, **kw)["rgb"].astype(np.float64)
        assert (np.abs(out - value.astype(np.float64)) <= 64 * np.spacing(value).astype(np.float64)).all(), kw


def test_one_iteration_with_every_stop_off_is_the_b3_kernel():
    rng = np.random.default_rng(3)
    rgb = rng.uniform(0.1, 2.0, (21, 34, 3)).astype(F)
    points, records = _flat(34, 21, rgb)
    out = SR.smooth(points, records, iterations=1)["rgb"]
    want = SR.b3_blur(rgb)
    assert np.abs(out - want).max() <= 64 * 2.0 ** -24 * 2.0, "the 64 ulp of the constant field, at the largest value"
    assert np.abs(out - rgb).max() > 0.1, "and it is a blur"
    centre = np.zeros((9, 9, 3), F)
    centre[4, 4] = 256.0
    points, records = _flat(9, 9, centre)
    got = SR.smooth(points, records, iterations=1)["rgb"][2:7, 2:7, 0]
    assert got.tolist() == np.outer(SR.B3, SR.B3).tolist(), "an impulse of 256 reads the kernel itself: the weights sum to 256"


@pytest.mark.parametrize("size", SIZES)
def test_the_word_and_the_texels_that_do_not_take_part_come_back(size):
    points, records = SR.atlas(*size)
    on = SR.takes_part(points, records)
    for kw in (dict(iterations=1), dict(iterations=3, **SR.PARAMS)):
        out = SR.smooth(points, records, **kw)
        assert out["word"].tobytes() == records["word"].tobytes()
        assert out[~on].tobytes() == records[~on].tobytes()
        assert np.isfinite(out["rgb"][on]).all()


def _room():
    """a floor chart and a wall chart at right angles, four gutter texels apart, 48 x 64"""
    W, H = 48, 64
    points, records = np.zeros((H, W), bake.point_dtype), np.zeros((H, W), SR.record_dtype)
    records["word"] = SR.INVALID
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    floor, wall = x < 22, x >= 26
    points["position"][floor] = np.stack([x[floor] * 0.1, np.zeros(floor.sum()), y[floor] * 0.1], -1)
    points["normal"][floor] = (0, 1, 0)
    points["position"][wall] = np.stack([np.full(wall.sum(), 2.2), (x[wall] - 26) * 0.1, y[wall] * 0.1], -1)
    points["normal"][wall] = (-1, 0, 0)
    rng = np.random.default_rng(11)
    records["rgb"][floor | wall] = rng.uniform(0.2, 1.0, (int((floor | wall).sum()), 3))
    records["word"][floor | wall] = 9
    return points, records, floor, wall


def test_nothing_leaks_from_the_floor_into_the_wall():
    points, records, floor, wall = _room()
    lit = records.copy()
    lit["rgb"][floor] = 100.0
    for kw in (dict(iterations=5), dict(iterations=5, **SR.PARAMS), dict(iterations=3, radius=0.0, plane=0.0, sigma_colour=1e6)):
        a, b = SR.smooth(points, records, **kw), SR.smooth(points, lit, **kw)
        assert a[wall].tobytes() == b[wall].tobytes(), kw
        assert a[~floor & ~wall].tobytes() == records[~floor & ~wall].tobytes(), "the gutter keeps its bytes"
        assert a[floor].tobytes() != records[floor].tobytes()


# the sizes at which a mutant has something to change: every size from 16 x 16 on.  The three atlases below that hold a handful of texels
# 0.8 and more apart in the world — beyond `radius`, so a texel's only tap is itself and only the radius stop has a say (and at 1 x 1 nothing).
_MUTANT_SIZES = {m: SIZES[3:] for m in SR.MUTANTS}
_MUTANT_SIZES["radius"] = SIZES[1:]


@pytest.mark.parametrize("mutant", SR.MUTANTS)
def test_the_inputs_tell_every_mutant_apart(mutant):
    """at least one output byte of every mutant differs from the true restatement on the inputs the GPU test uses"""
    for size in _MUTANT_SIZES[mutant]:
        points, records = SR.atlas(*size)
        true = SR.smooth(points, records, iterations=3, **SR.PARAMS)
        assert SR.smooth(points, records, iterations=3, mutant=mutant, **SR.PARAMS).tobytes() != true.tobytes(), (mutant, size)


def test_the_parallel_charts_are_kept_apart_by_the_plane_stop_alone():
    points, records = SR.atlas(64, 64)
    assert SR.STEP < SR.PARAMS["radius"] and SR.STEP > SR.PARAMS["plane"]
    low, high = points["position"][..., 1] == 0, points["position"][..., 1] == F(SR.STEP)
    adjacent = low[:, :-1] & high[:, 1:] & (points["normal"][:, :-1] == points["normal"][:, 1:]).all(-1) & (points["normal"][:, :-1, 1] == 1)
    assert adjacent.sum() > 20, "the two charts touch along a column of the atlas, with equal normals"
    raised = records.copy()
    raised["rgb"][high] += F(0.05)          # (a change a colour stop of 0.8 lets through)
    a, b = SR.smooth(points, records, iterations=3, **SR.PARAMS), SR.smooth(points, raised, iterations=3, **SR.PARAMS)
    on_low = low & SR.takes_part(points, records) & (points["normal"][..., 1] == 1)
    assert a[on_low].tobytes() == b[on_low].tobytes(), "the floor does not see the chart a step above it"
    kw = dict(SR.PARAMS, plane=0.0)
    a, b = SR.smooth(points, records, iterations=3, **kw), SR.smooth(points, raised, iterations=3, **kw)
    assert a[on_low].tobytes() != b[on_low].tobytes(), "without the plane stop it does"


def _penumbra(N=64):
    """(points (N, N), K -> light texels (N, N)): a floor of 4 x 4 under a spot light whose disk a square at height 1.5 partly hides"""
    world = World()
    world.add(SpotLight(position=(0.3, 4.0, -0.2), direction=(0.0, -1.0, 0.0), color=(255, 240, 220, 255), size=0.4, emission=60.0, beam_angle=2.4))
    spots = flatten(world).spot_lights
    g = (np.arange(N) + 0.5) / N * 4.0 - 2.0
    x, z = np.meshgrid(g, g)
    points = bake.points(np.stack([x, np.zeros_like(x), z], -1).reshape(-1, 3), np.tile([0.0, 1.0, 0.0], (N * N, 1)), 1e-3, 1e3)

    def baked(K):
        rays, weights = LR.rays(points, spots, [], LR.disk_table(K, 4), 5)
        o, d, far = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), rays["far"].astype(np.float64)
        with np.errstate(all="ignore"):
            t = (1.5 - o[..., 1]) / d[..., 1]
            hit = o + t[..., None] * d
            occluded = (t > 1e-3) & (t < far) & (np.abs(hit[..., 0]) <= 0.7) & (np.abs(hit[..., 2]) <= 0.7)
        return LR.texels(points, weights, occluded.astype(np.uint32), LR.colour_emission(spots, [])).reshape(N, N)

    return points.reshape(N, N), baked


def test_it_denoises_a_penumbra(built):
    points, baked = _penumbra()
    truth, raw = baked(256)["light"].astype(np.float64), baked(4)
    defaults = smooth.params()
    kw = {k: defaults[k].item() for k in ("iterations", "radius", "plane", "sigma_colour")}
    smoothed = SR.smooth(points, raw, **kw)
    rms = lambda rgb: float(np.sqrt(((rgb.astype(np.float64) - truth) ** 2).mean()))
    before, after = rms(raw["light"]), rms(smoothed["rgb"])
    print(f"\nRMS error against K = 256: raw K = 4 {before:.4f}, smoothed {after:.4f}, ratio {after / before:.2f} (light up to {truth.max():.2f}); params {kw}")
    assert len(np.unique(raw["light"][..., 0])) > 16 and before > 0.01, "the scene has a penumbra and the K = 4 bake is noisy"
    assert after < before
    assert smoothed["word"].tobytes() == raw["shadowed"].tobytes()
