"""What the bake pipeline's rules add up to, against the CPU oracle, without a device (tests/meaning_reference.py): the claim under "THE
MEANING" in include/hiprz_light.h and include/hiprz_gather.h — a baked view shows, at a pixel, surface colour x the light the path tracer
collects at that pixel's surface point — per group of pixels: the floor, the wall and every cube face the camera sees.

THE BAR, per group: |baked / traced - 1| <= bias + discretisation + 4 x standard error of the traced group mean.
  bias            2 x the larger solid angle of the two lights as flatten stores them (meaning_reference.bias): the tracer weights its light
                  sample with Lw = 1 / (1 + solid angle x pdf) >= 1 / (1 + solid angle) and adds a BRDF-sampled term of second order in
                  the solid angle.  2 x 1.2566e-3 = 2.513e-3 here, the direct light's (the spot's is 3.2e-4 at its nearest point).
                  The tracer's `radiance < 1e-4` cut-off (and the spot's `b < 1e-4`) drops a sample whose Le = emission x solid angle x
                  cosine is below 1e-4: with emission x solid angle = 0.25 (direct) and 0.5 .. 0.9 (spot) that is a cosine below 1e-3,
                  which carries less than 1e-3 of a full sample and no group has more than a sliver of such points.
  discretisation  |pipeline / rule - 1| of the group's mean, the CPU pipeline against direct64 / bounce64 at the pixels' own points:
                  reference against reference.  For the rules themselves it is 4 x the standard error of bounce64's own estimate.
  standard error  first_path's, over 256 seeds.

MEASURED (64 x 48 camera, 128 x 96 atlas, 256 seeds; groups floor 1 636, wall 438, cube top 287, cube front 172, cube left 95 pixels), baked /
traced per group in that order:
  rules           depth 1: 1.0001 1.0001 1.0001 1.0012 1.0006   depth 2: 1.0002 1.0010 1.0001 0.9990 1.0087
  pipeline        0 bounces nearest 0.9991 1.0012 1.0001 1.0008 1.0009, bilinear 0.9997 1.0004 1.0001 1.0009 1.0008
                  1 bounce  nearest 0.9991 1.0022 1.0001 1.0026 1.0064, bilinear 0.9996 1.0010 1.0000 1.0021 1.0046
  discretisation  0 bounces <= 1.1e-3, 1 bounce <= 4.0e-3 (cube left, bilinear; mostly bounce64's own noise)
  4 x s.e.        depth 1: 3e-4 5e-4 1e-4 1.6e-3 3.1e-3     depth 2: 7e-4 3.1e-3 2e-4 8.3e-3 1.1e-2
  teeth           overlapping charts: cube front 49.9, cube left 85.3; 1 bounce against depth 1: 1.17 (cube top) .. 17 (cube sides);
                  albedo 1: 1.275 .. 1.279 = 255 / 200; sky 0 at depth 2: floor 0.773"""
import numpy as np
import pytest

import atlas_reference as AR
import gather_world as GW
import meaning_reference as MR
from rayzath_amd import view

FILTERS = (view.NEAREST, view.BILINEAR)
SIDE_FACES = ("cube front", "cube left")


@pytest.fixture(scope="module")
def st(built):
    return MR.study()


def _check(st, baked, bounces, filter, depth, what):
    """every group within its bar; the figures printed first"""
    mean, err = st["frames"][depth]
    failed = []
    for g, m in st["groups"].items():
        ratio, _ = MR.group_ratio(baked, mean, err, m)
        limit, terms = MR.bar(st, bounces, filter, g, depth)
        print(f"{what} {g}: baked/traced {ratio:.4f}, bar {limit:.2e} = bias {terms[0]:.2e} + discretisation {terms[1]:.2e} + 4 s.e. {terms[2]:.2e}")
        if not abs(ratio - 1.0) <= limit:
            failed.append((g, ratio, limit))
    assert not failed, f"{what}: {failed}"


def _outside(st, baked, bounces, filter, depth, group, what):
    mean, err = st["frames"][depth]
    ratio, _ = MR.group_ratio(baked, mean, err, st["groups"][group])
    limit, _ = MR.bar(st, bounces, filter, group, depth)
    print(f"teeth, {what}, {group}: baked/traced {ratio:.4f}, bar {limit:.2e}")
    assert abs(ratio - 1.0) > limit, f"{what}: {group} stays within the bar ({ratio:.4f})"
    return ratio


def test_the_fixture(st):
    """no texel of a default part is claimed twice, the overlapping variant claims every cube texel six times, no edge of a cube cell lies
    near a texel boundary or a texel centre of the 64 x 48 atlas, and every group is large enough for a mean"""
    w = st["world"]
    for W, H in ((GW.W, GW.H), MR.ATLAS):
        seen = np.zeros((H, W), np.uint32)
        for instance, tris in GW.parts(w):
            claims = AR.cover(tris, W, H)[1]
            assert claims.max() == 1, f"instance {instance} claims a texel of the {W} x {H} atlas {int(claims.max())} times"
            seen += claims
        assert seen.max() == 1, "two parts claim one texel"
        cube = AR.cover(dict(GW.parts(w, overlapping=True))[GW.CUBE], W, H)[1]
        assert set(np.unique(cube).tolist()) == {0, 6}, "the overlapping cube claims every texel it covers six times"
        # the gutter: between two cells lie at least the two rings of texels the tests dilate by, at 64 x 48
        if (W, H) == (GW.W, GW.H):
            owner = AR.cover(dict(GW.parts(w))[GW.CUBE], W, H)[0] // 2
            ys, xs = np.nonzero(owner < 6)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y, x = np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)
                    assert ((owner[y, x] == owner[ys, xs]) | (owner[y, x] >= 6)).all(), "two faces lie within two texels of each other"
    cube = dict(GW.parts(w))[GW.CUBE]
    for axis, size in (("u", GW.W), ("v", GW.H)):
        at = np.concatenate([cube[f"{axis}{k}"] for k in (1, 2, 3)]).astype(np.float64) * size
        assert (np.abs(2.0 * at - np.rint(2.0 * at)) / 2.0 >= 0.05).all(), "a cell's edge lies on a texel boundary or a texel centre"
    sizes = {g: int(m.sum()) for g, m in st["groups"].items()}
    print(sizes)
    assert set(sizes) == {"floor", "wall", "cube top"} | set(SIDE_FACES) and min(sizes.values()) >= 90, sizes
    hits = st["surface"]["hits"]
    assert not (st["atlas_pixels"] & (hits["instance"] == GW.SPHERE)).any()


@pytest.mark.parametrize("depth", (1, 2))
def test_the_rules_against_the_oracle(st, depth):
    """colour x direct64 against the first paths of depth 1, colour x (direct64 + bounce64, the sky included) against those of depth 2"""
    mean, err = st["frames"][depth]
    failed = []
    for g, m in st["groups"].items():
        ratio, se = MR.group_ratio(st["rules"][depth - 1], mean, err, m)
        own = np.sqrt(((st["rule_err"][depth - 1] @ MR.LUMA)[m] ** 2).sum()) / m.sum() / MR.luminance(st["rules"][depth - 1])[m].mean()
        limit = st["bias"] + 4.0 * own + 4.0 * se
        print(f"rules, depth {depth}, {g}: rule/traced {ratio:.4f}, bar {limit:.2e} = bias {st['bias']:.2e} + 4 own s.e. {4 * own:.2e} + 4 s.e. {4 * se:.2e}")
        if not abs(ratio - 1.0) <= limit:
            failed.append((g, ratio, limit))
    assert not failed, failed


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("bounces", (0, 1))
def test_the_pipeline_against_the_oracle(st, bounces, filter):
    rgb, count = MR.pipeline(st["parts"], *MR.ATLAS, bounces, filter)
    assert rgb.tobytes() == st["baked"][bounces, filter].tobytes() and (count[st["atlas_pixels"]] > 0).all()
    _check(st, rgb, bounces, filter, bounces + 1, f"pipeline, {bounces} bounces, filter {filter}")


def test_teeth_overlapping_charts(st):
    """the cube's own UVs, six faces on the same texels: the side faces read the top face's light"""
    rgb, _ = MR.pipeline(GW.parts(st["world"], overlapping=True), *MR.ATLAS, 0, view.BILINEAR)
    for g in SIDE_FACES:
        assert _outside(st, rgb, 0, view.BILINEAR, 1, g, "overlapping charts") > 2.0
    _check(dict(st, groups={g: m for g, m in st["groups"].items() if not g.startswith("cube")}), rgb, 0, view.BILINEAR, 1, "overlapping charts")


def test_teeth_a_bounce_too_many(st):
    for g in st["groups"]:
        _outside(st, st["baked"][1, view.BILINEAR], 0, view.BILINEAR, 1, g, "1 bounce against depth 1")


def test_teeth_albedo_one(st):
    rgb, _ = MR.pipeline(st["parts"], *MR.ATLAS, 0, view.BILINEAR, albedo=(1.0, 1.0, 1.0))
    for g in st["groups"]:
        ratio = _outside(st, rgb, 0, view.BILINEAR, 1, g, "a source composed with albedo 1")
        assert abs(ratio * MR.ALBEDO[0] - 1.0) <= MR.bar(st, 0, view.BILINEAR, g, 1)[0], "albedo 1 is 255 / 200 of the light"


def test_teeth_no_sky(st):
    rgb, _ = MR.pipeline(st["parts"], *MR.ATLAS, 1, view.BILINEAR, sky=(0.0, 0.0, 0.0))
    assert _outside(st, rgb, 1, view.BILINEAR, 2, "floor", "a sky of 0 at depth 2") < 1.0
