"""What the device's bake pipeline adds up to, against the CPU oracle (tests/meaning_reference.py; the same claim, world, groups and bar as
tests/test_bake_meaning.py, which holds the numpy restatements to them without a device).  Trees 0 (reference) and 3 (device SAH), the
nearest and the bilinear filter, per group of ATLAS pixels: floor, wall and the cube faces the camera sees.

  depth 1   Context.bake_light_atlas, lit_source and view against the first paths of max_depth 1.
  depth 2   Context.bake_bounce_atlas with 1 bounce, lit_source and view against the first paths of max_depth 2.
  teeth     the same calls with one argument wrong each, every one outside the bar on the group named: the overlapping charts (the cube's
            side faces), 1 bounce against the depth-1 frames, a source composed with albedo 1, a sky of 0 at depth 2 (the floor).

THE BAR per group is tests/test_bake_meaning.py's: |baked / traced - 1| <= bias (2.51e-3) + discretisation (the CPU pipeline against the
float64 rules, <= 1.1e-3 at 0 bounces and <= 4.1e-3 at 1 bounce) + 4 x the standard error of the traced group mean (256 seeds; 2e-4 ..
3.3e-3 at depth 1, 2e-4 .. 1.1e-2 at depth 2).  The oracle's frames and the CPU side are computed once per process (MR.study()).

MEASURED ON MI355X, identical on trees 0 and 3 to the digits shown, baked / traced for floor, wall, cube top, cube front, cube left:
  depth 1   nearest  0.9992 1.0011 1.0001 1.0010 1.0013      bilinear 0.9998 1.0003 1.0000 1.0011 1.0011
  depth 2   nearest  0.9993 1.0021 1.0001 1.0021 1.0052      bilinear 0.9997 1.0008 1.0000 1.0016 1.0034
  teeth     (bilinear; nearest within 3e-3 of these) overlapping charts: cube front 49.93, cube left 85.10; 1 bounce against depth 1:
            1.316 1.783 1.172 17.06 16.88; albedo 1: 1.275 .. 1.276; sky 0 at depth 2: floor 0.774
The twelve cases take 0.3 s on the device beside the session's build fixture and the study (4 s of CPU: the float64 rules 1.5 s, the
oracle's 2 x 256 first-path frames 0.9 s, the chained restatements 1.0 s)."""
import numpy as np
import pytest

import gather_world as GW
import meaning_reference as MR
from rayzath_amd import gather, view
from rayzath_amd.engine import Context

pytestmark = pytest.mark.gpu

TREES = (0, 3)
FILTERS = (view.NEAREST, view.BILINEAR)
SIDE_FACES = ("cube front", "cube left")
BLACK = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def st(built):
    return MR.study()


@pytest.fixture(scope="module")
def frames(st):
    """what the device shows, per (tree, case, filter), computed once per tree: the cases are depth 1, depth 2 and the teeth's sources"""
    seen = {}

    def of(tree):
        if tree not in seen:
            ctx = Context(0)
            try:
                if tree:
                    ctx.set_tree(tree)
                ctx.upload_scene(st["flat"]), ctx.upload_camera(st["cam"])
                W, H = MR.ATLAS
                bake = (MR.DIRECTIONS, MR.LIGHT_SAMPLES, MR.SEED, MR.RINGS)
                out = {}

                def show(case, parts, source):
                    charts = gather.chart_tables(parts, len(st["flat"].instances))
                    for filter in FILTERS:
                        out[case, filter] = ctx.view(source, W, H, charts, None, MR.SKY, view.params(filter))

                parts = st["parts"]
                light, _, _ = ctx.bake_light_atlas(parts, W, H, MR.LIGHT_SAMPLES, MR.SEED, MR.RINGS, MR.NEAR, MR.FAR)
                show("depth 1", parts, ctx.lit_source(light, None, MR.ALBEDO, None, MR.RINGS))
                show("albedo 1", parts, ctx.lit_source(light, None, (1.0, 1.0, 1.0), None, MR.RINGS))
                direct, indirect, _ = ctx.bake_bounce_atlas(parts, W, H, MR.ALBEDO, None, 1, *bake, MR.SKY, MR.NEAR, MR.FAR)
                show("depth 2", parts, ctx.lit_source(direct, indirect, MR.ALBEDO, None, MR.RINGS))
                direct, indirect, _ = ctx.bake_bounce_atlas(parts, W, H, MR.ALBEDO, None, 1, *bake, BLACK, MR.NEAR, MR.FAR)
                show("no sky", parts, ctx.lit_source(direct, indirect, MR.ALBEDO, None, MR.RINGS))
                overlapping = GW.parts(st["world"], overlapping=True)
                light, _, _ = ctx.bake_light_atlas(overlapping, W, H, MR.LIGHT_SAMPLES, MR.SEED, MR.RINGS, MR.NEAR, MR.FAR)
                show("overlapping", overlapping, ctx.lit_source(light, None, MR.ALBEDO, None, MR.RINGS))
            finally:
                ctx.close()
            seen[tree] = out
        return seen[tree]

    return of


def _ratios(st, pixels, depth):
    """{group: baked / traced}; every pixel of a group is an ATLAS pixel of the device's frame"""
    mean, err = st["frames"][depth]
    assert pixels.shape == st["atlas_pixels"].shape
    assert np.array_equal(view.kind(pixels) == view.ATLAS, st["atlas_pixels"]), "the device's ATLAS pixels are not the oracle's front-face hits on mapped instances"
    assert (view.count(pixels)[st["atlas_pixels"]] > 0).all()
    return {g: MR.group_ratio(pixels["rgb"], mean, err, m)[0] for g, m in st["groups"].items()}


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("depth", (1, 2))
@pytest.mark.parametrize("tree", TREES)
def test_a_baked_view_shows_what_the_tracer_collects(st, frames, tree, depth, filter):
    ratios = _ratios(st, frames(tree)[f"depth {depth}", filter], depth)
    failed = []
    for g, ratio in ratios.items():
        limit, terms = MR.bar(st, depth - 1, filter, g, depth)
        print(f"tree {tree} depth {depth} filter {filter} {g}: baked/traced {ratio:.4f}, bar {limit:.2e} = bias {terms[0]:.2e} + discretisation {terms[1]:.2e} + 4 s.e. {terms[2]:.2e}")
        if not abs(ratio - 1.0) <= limit:
            failed.append((g, ratio, limit))
    assert not failed, failed


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("tree", TREES)
def test_teeth(st, frames, tree, filter):
    """each wrong argument puts the group named outside the bar that the right ones stay within"""
    got = frames(tree)
    cases = (("overlapping charts", "overlapping", 0, 1, SIDE_FACES), ("1 bounce against depth 1", "depth 2", 0, 1, tuple(st["groups"])),
             ("a source composed with albedo 1", "albedo 1", 0, 1, tuple(st["groups"])), ("a sky of 0 at depth 2", "no sky", 1, 2, ("floor",)))
    inside = []
    for what, case, bounces, depth, groups in cases:
        ratios = _ratios(st, got[case, filter], depth)
        for g in groups:
            limit, _ = MR.bar(st, bounces, filter, g, depth)
            print(f"teeth, tree {tree} filter {filter}, {what}, {g}: baked/traced {ratios[g]:.4f}, bar {limit:.2e}")
            if not abs(ratios[g] - 1.0) > limit:
                inside.append((what, g, ratios[g]))
    assert not inside, inside
