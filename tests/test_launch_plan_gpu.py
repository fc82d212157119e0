"""The launch plan on the device (rayzath_amd/csrc/hiprz_plan.cpp): a context that replays captured graphs and an eager twin go through
the same sequence of settings that change the plan — walk order, ray sort, XCD swizzle, traversal mode, LDS staging, the compat
integrator and back, light sample counts across the 30-slot limit of deferred shadow rays — two render calls after each, without a
reset in between except where the setter itself forces one.  After every call the two hold the same frame bit for bit (accumulator,
depth, ray and pass counters): the key of a captured graph is never stale.  The graph context captures exactly once per flip and not at
all on a pair of calls with nothing changed: the key is not over-eager either.  A second scene without lights runs the per-wave
resident pipeline against the split one.
"""
import numpy as np
import pytest

from rayzath_amd import scenes
from rayzath_amd.engine import Context, LightSampling, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

W, H, INSTANCES, DEPTH = 160, 96, 9, 4


def _config(spot, direct):
    return RenderConfig(light_sampling=LightSampling(spot, direct), tracing=Tracing(DEPTH, 8)).struct()


def _context(flat, cam, graph, pipeline=None):
    ctx = Context(0)
    ctx.set_lds_scene(0)
    if pipeline is not None:
        ctx.set_pipeline(pipeline)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(_config(2, 1))
    ctx.set_graph(graph)
    return ctx


def _same_frames(a, b, label):
    assert np.array_equal(a.read_accum(), b.read_accum()), f"{label}: accumulators differ"
    assert np.array_equal(a.read_depth(), b.read_depth()), f"{label}: depth differs"
    assert a.ray_count() == b.ray_count(), f"{label}: ray counts differ"
    assert a.pass_count() == b.pass_count(), f"{label}: pass counts differ"


FLIPS = [("walk order 1 -> 0", lambda c: c.set_walk_order(0)),
         ("ray sort -1 -> 0", lambda c: c.set_ray_sort(0)),
         ("ray sort 0 -> 1", lambda c: c.set_ray_sort(1)),
         ("xcd swizzle on", lambda c: c.set_xcd_swizzle(True)),
         ("traversal mode -1 -> 1", lambda c: c.set_traversal_mode(1)),
         ("lds scene 0 -> -1", lambda c: c.set_lds_scene(-1)),
         ("mode 63", lambda c: c.set_mode(63)),
         ("mode 0", lambda c: c.set_mode(0)),
         ("samples (16, 15)", lambda c: c.set_config(_config(16, 15))),
         ("samples (16, 16)", lambda c: c.set_config(_config(16, 16)))]


def test_graph_replay_follows_the_plan(built):
    world = scenes.living_room(W, H, INSTANCES)
    flat, cam = flatten(world), camera_struct(world.camera)
    graph, eager = _context(flat, cam, True), _context(flat, cam, False)
    assert graph.pipeline() == 1 and eager.pipeline() == 1    # lights, not staged: split
    captures = 0
    for k, n in enumerate((1, 4, 4)):
        graph.render(n), eager.render(n)
        _same_frames(graph, eager, f"initial call {k}")
    captures += 1
    assert graph.graph_captures() == captures, "render(4) twice with nothing changed: one capture, one replay"
    for label, flip in FLIPS:
        flip(graph), flip(eager)
        for k in range(2):
            graph.render(4), eager.render(4)
            _same_frames(graph, eager, f"{label}, call {k}")
        captures += 1
        print(f"{label}: pipeline {graph.pipeline()}, mode {graph.traversal_mode()}, captures {graph.graph_captures()}")
        assert graph.graph_captures() == captures, f"{label}: one capture for the two calls"
        assert eager.graph_captures() == 0
    for k in range(2):
        graph.render(4), eager.render(4)
        _same_frames(graph, eager, f"steady pair, call {k}")
    assert graph.graph_captures() == captures, "nothing changed: the graph is replayed"


def test_wave_resident_against_split(built):
    world = scenes.living_room(W, H, INSTANCES)
    world.spot_lights.clear(), world.direct_lights.clear()
    world.material.emission = 1.0   # the sky lights the room instead
    flat, cam = flatten(world), camera_struct(world.camera)
    resident, split = _context(flat, cam, False, pipeline=2), _context(flat, cam, False, pipeline=1)
    assert resident.pipeline() == 2 and split.pipeline() == 1
    for k, n in enumerate((1, 4, 4)):
        resident.render(n), split.render(n)
        _same_frames(resident, split, f"initial call {k}")
    for label, flip in FLIPS:
        flip(resident), flip(split)
        for k in range(2):
            resident.render(4), split.render(4)
            _same_frames(resident, split, f"{label}, call {k}")
