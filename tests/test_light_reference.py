"""Light baking without a GPU: the numpy restatement (tests/light_reference.py) of include/hiprz_light.h against known answers, the
library's host-only calls, its own float64 evaluation, closed forms, and the edge lights.  Run with -s for the measured figures.

MEASURED (this file, float32 restatement against the same rules in float64, 4 096 points x 4 lights x 64 samples of a random scene):
522 689 of 1 048 576 samples kept, none on one side only; largest component error of a kept direction 1.62e-6, largest error of a weight 3.1e-7 of the largest weight and 5.4e-3 of itself
(where the cosine is nearly 0).

CLOSED FORMS, all rays unoccluded, relative error for K = 16, 64, 256, 1024:
  direct light faced squarely, angular size 0.3:   5.4e-7 at every K.  The rule is exact in K there — cos = z is linear in r^2 and the table's
      r^2 are the midpoints (k + 0.5) / K — so nothing can fall; the error is float32 rounding and is held to 64 * 2^-24 (reasoned below).
  direct light, normal tilted by 0.5 rad:          2.2e-3, 1.4e-3, 1.8e-4, 3.0e-5: falls with K (asserted).
  spot disk on its axis at d = 2, size 0.05:       3.64e-4 at every K: the integrand depends on r^2 alone and smoothly, so K = 16 has converged;
      what is left is the closed form's own (size / d)^2 term.  It falls with the size instead: 3.5e-2, 9.0e-3, 3.6e-4, 1.5e-5 for size 0.5,
      0.25, 0.05, 0.01 (asserted), and is the same at every K to 64 * 2^-24 (asserted)."""
import numpy as np
import pytest

import light_reference as LR
from rayzath_amd import _abi, bake, light
from rayzath_amd.scene import DirectLight, SpotLight, World, flatten

F = np.float32
KS = (16, 64, 256, 1024)
# a sum of K terms of ~10 float32 operations each, added per lane and through a six-step butterfly, beside the rounding of the stored
# cosine (sin^2 = 1 - cos^2 magnifies it by 2 cos^2 / sin^2 = 21 at 0.3 rad): (10 + 16 + 6 + 11) half-ulps, rounded up to a power of two
ROUNDING = 64 * 2.0 ** -24


def _lights(spots=(), directs=()):
    """the device records of lights given as keyword dictionaries, made the way every scene's are: scene.flatten"""
    world = World()
    for kw in spots:
        world.add(SpotLight(**kw))
    for kw in directs:
        world.add(DirectLight(**kw))
    flat = flatten(world)
    return flat.spot_lights, flat.direct_lights


def _bake(points, spots, directs, table, seed=0, words=None, lights=None, mutant=None):
    """(texels, rays, weights) of the restatement with every ray unoccluded (or `words`)"""
    rays, weights = LR.rays(points, spots, directs, table, seed, lights, mutant)
    s, d = LR.select(spots, directs, lights)
    words = np.zeros(weights.shape, np.uint32) if words is None else words
    return LR.texels(points, weights, words, LR.colour_emission(s, d), mutant), rays, weights


def test_hash_and_set_known_answers(built):
    assert LR.hash32([0, 1, 2, 0xFFFFFFFF, 20261020]).tolist() == [0, 1753845952, 3507691905, 1734902346, 2312333810]
    assert LR.set_of(np.arange(8), 7, 5).tolist() == [3, 2, 1, 1, 3, 0, 2, 0]
    for seed, S in ((0, 1), (7, 5), (20261020, 64), (0xFFFFFFFF, 3)):
        assert [light.set_of(i, seed, S) for i in range(300)] == LR.set_of(np.arange(300), seed, S).tolist()
    assert light.set_of(5, 1, 0) == 0 and light.set_of(0xFFFFFFFF, 0xFFFFFFFF, 64) == 0


def test_the_c_disk_table_is_the_float64_one(built):
    for K, S in ((1, 1), (2, 5), (16, 3), (64, 4), (128, 1), (1024, 64)):
        got, want = light.disk_samples(K, S), LR.disk_table(K, S)
        assert got.shape == (S, K, 2) and got.tobytes() == want.tobytes(), (K, S)
        assert ((got[..., 0] * got[..., 0] + got[..., 1] * got[..., 1]) <= F(1.0)).all(), "a sample left the disk"
        r2 = (got.astype(np.float64) ** 2).sum(-1)
        assert np.abs(r2 - (np.arange(K) + 0.5) / K).max() < 1e-6, "r^2 of sample k is (k + 0.5) / K in every set"
    for K, S in ((0, 1), (3, 1), (2048, 1), (16, 0), (16, 65)):
        with pytest.raises(ValueError):
            light.disk_samples(K, S)


def _random_scene(rng, n):
    spots, directs = _lights(
        [dict(position=(0.5, 3.0, -0.5), direction=(-0.1, -1.0, 0.2), color=(255, 200, 90, 255), size=0.4, emission=40.0, beam_angle=0.9),
         dict(position=(-2.0, 1.0, 2.0), direction=(1.0, -0.3, -1.0), color=(30, 255, 255, 255), size=0.05, emission=9.0, beam_angle=2.5)],
        [dict(direction=(0.2, -1.0, 0.1), color=(255, 255, 255, 255), emission=3.0, angular_size=0.2),
         dict(direction=(-1.0, -0.2, 0.4), color=(90, 120, 255, 255), emission=1.5, angular_size=1.2)])
    points = bake.points(rng.uniform(-1.5, 1.5, size=(n, 3)), rng.normal(size=(n, 3)), 1e-3, 1e3)
    return points, spots, directs


def test_the_float32_restatement_against_its_float64_evaluation():
    """reported, not held to a figure chosen in advance: how far float32 arithmetic moves a direction and a weight"""
    points, spots, directs = _random_scene(np.random.default_rng(26), 4096)
    table = LR.disk_table(64, 4)
    w3, far, w, kept = LR.samples(points, spots, directs, table, 3, F)
    w3d, fard, wd, keptd = LR.samples(points, spots, directs, table, 3, np.float64)
    both = kept & keptd
    one_sided = int((kept != keptd).sum())
    direction = float(np.abs(w3[both] - w3d[both]).max())
    weight = float((np.abs(w[both] - wd[both]) / wd[both]).max())          # largest where the cosine is nearly 0: a difference of nearly equal products
    absolute = float(np.abs(w[both] - wd[both]).max() / wd[both].max())
    print(f"\n{both.sum()} of {kept.size} samples kept in both, {one_sided} on one side only; largest component error of a direction {direction:.2e}, "
          f"largest error of a weight {absolute:.2e} of the largest weight, {weight:.2e} of itself")
    assert both.sum() > kept.size // 10 and np.isfinite(direction) and np.isfinite(weight)
    assert w3.dtype == F and w.dtype == F and wd.dtype == np.float64
    # where only one side keeps a sample the other side's weight is at the rounding of a comparison: c = 0 or the beam's edge
    assert one_sided <= kept.size // 1000


def _relative(texel, want):
    return float(np.abs(texel["light"][0].astype(np.float64) - want).max() / np.abs(want).max())


def test_a_direct_light_tends_to_pi_sin_squared():
    theta, colour, emission = 0.3, (255, 128, 64, 255), 2.0
    spots, directs = _lights((), [dict(direction=(0, 0, -1), color=colour, emission=emission, angular_size=theta)])
    rgb = np.array(colour[:3]) / 255.0
    errors = {}
    for tilt in (0.0, 0.5):
        point = bake.points([[0, 0, 0]], [[np.sin(tilt), 0, np.cos(tilt)]], 1e-3, 1e3)
        want = rgb * emission * np.pi * np.sin(theta) ** 2 * np.cos(tilt)      # the cap lies above the horizon: the cosine of the tilt factors out
        errors[tilt] = [_relative(_bake(point, spots, directs, LR.disk_table(K, 1))[0], want) for K in KS]
        print(f"\ndirect light, angular size {theta}, normal tilted by {tilt}: relative error " + ", ".join(f"K {K}: {e:.2e}" for K, e in zip(KS, errors[tilt])))
    assert all(e <= ROUNDING for e in errors[0.0]), "facing the light the K-sample rule is exact: only rounding is left"
    assert all(b < a for a, b in zip(errors[0.5], errors[0.5][1:])), "the error falls with K"
    assert errors[0.5][-1] < 1e-4 < errors[0.5][0]


def test_a_small_spot_disk_tends_to_its_solid_angle():
    d, emission = 2.0, 3.0
    point = bake.points([[0, 0, 0]], [[0, 0, 1]], 1e-3, 1e3)
    by_size = []
    for size in (0.5, 0.25, 0.05, 0.01):
        spots, directs = _lights([dict(position=(0, 0, d), direction=(0, 0, -1), color=(255, 255, 255, 255), size=size, emission=emission, beam_angle=1.0)])
        want = np.full(3, emission * size * size * np.pi / (d + 1.0) ** 2)
        errors = [_relative(_bake(point, spots, directs, LR.disk_table(K, 1))[0], want) for K in KS]
        print(f"\nspot disk of size {size} at distance {d} on its axis: relative error " + ", ".join(f"K {K}: {e:.2e}" for K, e in zip(KS, errors)))
        assert max(errors) - min(errors) <= ROUNDING, "on the axis the integrand depends on r^2 alone: K = 16 has converged already"
        assert max(errors) <= (size / d) ** 2, "what is left is the closed form's own (size / d)^2 term"
        by_size.append(errors[-1])
    assert all(b < a for a, b in zip(by_size, by_size[1:])) and by_size[-1] < 1e-4, "the error falls as the disk gets small"


EDGE_SPOTS = {
    "size 0": dict(position=(0.3, 0.2, 2.0), direction=(0, 0, -1), size=0.0, emission=5.0, beam_angle=1.0),
    "beam angle 0": dict(position=(0.3, 0.2, 2.0), direction=(0, 0, -1), size=0.2, emission=5.0, beam_angle=0.0),
    "emission 0": dict(position=(0.3, 0.2, 2.0), direction=(0, 0, -1), size=0.2, emission=0.0, beam_angle=1.0),
    "at the point": dict(position=(0, 0, 0), direction=(0, 0, -1), size=0.2, emission=5.0, beam_angle=1.0),
    "behind the surface": dict(position=(0.3, 0.2, -2.0), direction=(0, 0, 1), size=0.2, emission=5.0, beam_angle=1.0),
}
EDGE_DIRECTS = {
    "angular size 0": dict(direction=(0.1, 0.2, -1), emission=5.0, angular_size=0.0),
    "emission 0": dict(direction=(0.1, 0.2, -1), emission=0.0, angular_size=0.4),
    "opposite normal": dict(direction=(0, 0, 1), emission=5.0, angular_size=0.0),
}


@pytest.mark.parametrize("K", (1, 16, 128))
def test_edge_lights_give_exactly_zero_and_walk_nothing(K):
    """The lights whose light is 0 by the rules: every weight is +0, every ray has the direction +0 the query flags invalid, and the texel
    is +0 in every bit whatever the occlusion words say.  (Off the beam's axis: ON it the rounded similarity may exceed 1 = cos 0.)"""
    point = bake.points([[0, 0, 0]], [[0, 0, 1]], 1e-3, 1e3)
    table = LR.disk_table(K, 2)
    for name, kw in EDGE_SPOTS.items():
        spots, directs = _lights([kw])
        texel, rays, weights = _bake(point, spots, directs, table, words=np.ones((1, 1, K), np.uint32))
        assert (weights.view(np.uint32) == 0).all() and (rays["direction"].view(np.uint32) == 0).all(), f"spot light, {name}"
        assert texel.tobytes() == bytes(16), f"spot light, {name}"
    for name, kw in EDGE_DIRECTS.items():
        spots, directs = _lights((), [kw])
        texel, rays, weights = _bake(point, spots, directs, table, words=np.ones((1, 1, K), np.uint32))
        assert (weights.view(np.uint32) == 0).all() and (rays["direction"].view(np.uint32) == 0).all(), f"direct light, {name}"
        assert texel.tobytes() == bytes(16), f"direct light, {name}"


def test_lights_at_their_upper_clamps_stay_finite():
    """beam angle pi lights everything in front of the disk; angular size pi is light from the whole sphere, of which the upper half
    arrives: pi * emission * (1 - 1/2 .. ) is not 0 — these are edges of the range, not lights without light"""
    point = bake.points([[0, 0, 0]], [[0, 0, 1]], 1e-3, 1e3)
    table = LR.disk_table(64, 1)
    spots, directs = _lights([dict(position=(0.3, 0.2, 2.0), direction=(0, 0, 1), size=0.2, emission=5.0, beam_angle=3.14159)])
    texel, rays, weights = _bake(point, spots, directs, table)
    assert (weights > 0).all() and np.isfinite(texel["light"]).all() and (texel["light"] > 0).all(), "a beam of angle pi reaches a point behind the light's direction"
    spots, directs = _lights((), [dict(direction=(0, 0, -1), emission=5.0, angular_size=np.pi)])
    texel, rays, weights = _bake(point, spots, directs, table)
    # uniform over the sphere: half the samples lie below the horizon, the mean of max(cos, 0) is 1/4, times 4 pi
    assert 0 < (weights > 0).sum() <= 33 and np.isfinite(texel["light"]).all()
    assert abs(float(texel["light"][0][0]) / (5.0 * np.pi) - 1.0) < 2.0 / 64, "the whole sphere: pi * emission up to one sample's share"


def test_a_normal_opposite_the_light_gives_exactly_zero():
    table = LR.disk_table(16, 1)
    spots, directs = _lights([dict(position=(0, 0, 2.0), direction=(0, 0, -1), size=0.2, emission=5.0, beam_angle=1.0)],
                             [dict(direction=(0, 0, -1), emission=5.0, angular_size=0.1)])
    point = bake.points([[0, 0, 0]], [[0, 0, -1]], 1e-3, 1e3)
    texel, rays, weights = _bake(point, spots, directs, table, words=np.ones((1, 2, 16), np.uint32))
    assert (weights.view(np.uint32) == 0).all() and (rays["direction"].view(np.uint32) == 0).all() and texel.tobytes() == bytes(16)
    facing = _bake(bake.points([[0, 0, 0]], [[0, 0, 1]], 1e-3, 1e3), spots, directs, table)
    assert (facing[2] > 0).all() and (facing[0]["light"] > 0).all(), "the same lights reach the other side"


def test_texels_follow_the_verdicts_the_lane_order_and_the_mutants():
    """shadowed counts walked rays only, an invalid point reads INVALID / +0, a range selects its lights, and each mutant changes a byte"""
    rng = np.random.default_rng(5)
    points, spots, directs = _random_scene(rng, 70)
    points["far"][3] = 0.0          # far <= near: invalid
    for K in (1, 16, 128):
        table = LR.disk_table(K, 3)
        rays, weights = LR.rays(points, spots, directs, table, 11)
        words = (rng.random(weights.shape) < 0.4).astype(np.uint32)
        ce = LR.colour_emission(spots, directs)
        texels = LR.texels(points, weights, words, ce)
        assert texels["shadowed"][3] == LR.INVALID and (texels["light"][3].view(np.uint32) == 0).all() and (weights[3] == 0).all()
        ok = np.arange(70) != 3
        assert np.array_equal(texels["shadowed"][ok], ((words != 0) & (weights > 0)).sum((1, 2))[ok])
        total = (np.where((words == 0)[..., None], ce[None, :, None, :].astype(np.float64) * weights[..., None], 0.0).sum((1, 2)) / K)[ok]
        assert np.abs(texels["light"][ok] - total).max() <= 1e-5 * np.abs(total).max(), "the fixed order sums what a plain sum sums"
        # one light alone, through a range
        alone_rays, alone_w = LR.rays(points, spots, directs, table, 11, lights=(1, 1, 0, 0))
        assert alone_rays.tobytes() == rays[:, 1:2].tobytes() and alone_w.tobytes() == weights[:, 1:2].tobytes()
        alone_rays, alone_w = LR.rays(points, spots, directs, table, 11, lights=(2, None, 1, None))
        assert alone_rays.tobytes() == rays[:, 3:4].tobytes() and alone_w.tobytes() == weights[:, 3:4].tobytes()
        caught = {}
        for mutant in LR.MUTANTS:
            m_rays, m_w = LR.rays(points, spots, directs, table, 11, mutant=mutant)
            m_texels = LR.texels(points, m_w, words, ce, mutant)
            caught[mutant] = m_rays.tobytes() != rays.tobytes() or m_w.tobytes() != weights.tobytes() or m_texels.tobytes() != texels.tobytes()
        assert all(caught.values()), (K, caught)
    with pytest.raises(ValueError):
        LR.select(spots, directs, (3, None, 0, None))
    with pytest.raises(ValueError):
        LR.select(spots, directs, (0, 3, 0, None))
    assert [len(x) for x in LR.select(spots, directs, (2, None, 2, 0))] == [0, 0]
    assert spots.dtype == _abi.spot_light_dtype and directs.dtype == _abi.direct_light_dtype
