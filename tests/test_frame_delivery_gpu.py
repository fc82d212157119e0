"""Pipelined frame delivery on the GPU: hiprz_present assembles the frame (rgba8, depth, ray cast) on the device and a copy stream moves it
to pinned host memory; hiprz_read_frame hands it out.  Every comparison is exact: the frame equals what the synchronous reads return."""
import os
import subprocess

import numpy as np
import pytest

from rayzath_amd import _abi, scenes
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import SHARD_SAMPLES, Context, Engine, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")

pytestmark = pytest.mark.gpu


def _context(kind):
    if kind == "single":
        return Context(0)
    ctx = Context([0, 0])
    if kind == "samples":
        ctx.set_shard_mode(SHARD_SAMPLES)
    return ctx


def _setup(ctx, flat, cam, depth=8, seed=20240501):
    ctx.upload_scene(flat)
    ctx.upload_camera(cam)
    ctx.set_config(RenderConfig(tracing=Tracing(depth, 4), seed=seed).struct())


def _sync_frame(ctx, x, y):
    return dict(rgba8=ctx.read_rgba8(), depth=ctx.read_depth(), hit=ctx.ray_cast(x, y), ray_count=ctx.ray_count(), passes=ctx.pass_count())


def _assert_same(frame, want, what):
    assert np.array_equal(frame["rgba8"], want["rgba8"]), what + ": rgba8"
    assert np.array_equal(frame["depth"], want["depth"]), what + ": depth"
    assert frame["hit"] == want["hit"], what + f": ray cast {frame['hit']} != {want['hit']}"
    assert frame["ray_count"] == want["ray_count"] and frame["passes"] == want["passes"], what + ": counts"


_SCENES = {
    "B": lambda: scenes.CONFIGS["B"]["build"](),      # full size, resident pipeline (staged in LDS)
    "C-small": lambda: scenes.cornell_sphere(480, 270, 80),  # split pipeline, a frame whose edge tiles are partial
}


@pytest.mark.parametrize("kind", ["single", "two-streams", "samples"])
@pytest.mark.parametrize("scene", sorted(_SCENES))
def test_present_equals_the_synchronous_reads(built, kind, scene):
    world = _SCENES[scene]()
    flat, cam = flatten(world), camera_struct(world.camera)
    W, H = cam.width, cam.height
    ctx = _context(kind)
    try:
        _setup(ctx, flat, cam)
        ctx.render(1), ctx.render(4)
        ctx.tonemap()
        pixels = [(W // 2, H // 2), (0, 0), (W - 1, H - 1), (40, 3), (W // 3, 2 * H // 3), (W + 50, H + 7)]
        for x, y in pixels:
            want = _sync_frame(ctx, x, y)
            seq = ctx.present(x, y)
            got = ctx.read_frame()
            assert got["sequence"] == seq and (got["width"], got["height"]) == (W, H)
            _assert_same(got, want, f"{scene} {kind} pixel ({x}, {y})")
        assert any(ctx.ray_cast(x, y)[0] >= 0 for x, y in pixels), "no ray cast met anything: the comparison shows little"
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["single", "two-streams"])
def test_pipelined_loop_hands_out_the_frames_of_a_synchronous_twin(built, kind):
    world = scenes.cornell_sphere(320, 200, 40)
    flat, cam = flatten(world), camera_struct(world.camera)
    x, y = 150, 120
    piped, twin = _context(kind), _context(kind)
    try:
        _setup(piped, flat, cam), _setup(twin, flat, cam)
        expected, seq = [], 0
        for i in range(6):
            piped.render(3)
            seq = piped.present(x, y)  # no other synchronisation: frame seq - 1 travels while this one renders
            if i:
                got = piped.read_frame(seq - 1)
                assert got["sequence"] == seq - 1
                _assert_same(got, expected[i - 1], f"call {i}")
            twin.render(3)
            twin.tonemap()
            expected.append(_sync_frame(twin, x, y))
        _assert_same(piped.read_frame(seq), expected[-1], "last call")
    finally:
        piped.close(), twin.close()


def _expect_state(call):
    with pytest.raises(HiprzError) as e:
        call()
    assert e.value.code == _abi.ERR_STATE


def test_cameras_resize_and_sequences(built):
    world = scenes.cornell_box(96, 64)
    flat = flatten(world)
    cam0 = camera_struct(world.camera)
    cam1 = camera_struct(world.camera)
    cam1.width, cam1.height = 72, 40
    ctx = Context(0)
    try:
        _expect_state(lambda: ctx.present(0, 0))  # before any upload
        ctx.upload_scene(flat)
        _expect_state(lambda: ctx.present(0, 0))  # before the camera upload
        _expect_state(lambda: ctx.read_frame())
        ctx.set_camera_count(2)
        ctx.set_config(RenderConfig(tracing=Tracing(4, 4)).struct())
        ctx.select_camera(0), ctx.upload_camera(cam0)
        ctx.select_camera(1), ctx.upload_camera(cam1)
        frames = {}
        for k, cam in ((0, cam0), (1, cam1), (0, cam0), (0, cam0), (1, cam1)):
            ctx.select_camera(k)
            ctx.render(2)
            ctx.tonemap()
            want = _sync_frame(ctx, 30, 20)
            seq = ctx.present(30, 20)
            frames[(k, seq)] = want
        # camera 0 presented 1, 2, 3; camera 1 presented 1, 2: each keeps its own sequence and its newest two frames
        ctx.select_camera(0)
        for seq in (2, 3):
            got = ctx.read_frame(seq)
            assert (got["width"], got["height"], got["sequence"]) == (96, 64, seq)
            _assert_same(got, frames[(0, seq)], f"camera 0 frame {seq}")
        _expect_state(lambda: ctx.read_frame(1))  # evicted
        _expect_state(lambda: ctx.read_frame(4))  # never presented
        ctx.select_camera(1)
        for seq in (1, 2):
            got = ctx.read_frame(seq)
            assert (got["width"], got["height"], got["sequence"]) == (72, 40, seq)
            _assert_same(got, frames[(1, seq)], f"camera 1 frame {seq}")
        assert ctx.read_frame()["sequence"] == 2
        _expect_state(lambda: ctx.read_frame(3))
        # a resize frees the camera's frames and restarts its sequence
        cam1.width, cam1.height = 64, 48
        ctx.upload_camera(cam1)
        _expect_state(lambda: ctx.read_frame())
        _expect_state(lambda: ctx.read_frame(2))
        ctx.render(2)
        ctx.tonemap()
        want = _sync_frame(ctx, 5, 5)
        assert ctx.present(5, 5) == 1
        got = ctx.read_frame(1, copy=True)
        assert (got["width"], got["height"]) == (64, 48)
        _assert_same(got, want, "after the resize")
        # camera 0 was not touched by the other camera's resize
        ctx.select_camera(0)
        _assert_same(ctx.read_frame(3), frames[(0, 3)], "camera 0 after camera 1's resize")
        # destroying a context right after a present returns cleanly
        ctx.render(2)
        ctx.present(1, 1)
    finally:
        ctx.close()
    assert not ctx._ctx


def _twin_worlds():
    a, b = scenes.cornell_box(96, 64), scenes.cornell_box(96, 64)
    for w in (a, b):
        w.camera.ray_cast_pixel = (48, 40)
    return a, b


def test_python_engine_pipelined_hands_out_the_previous_frame(built):
    cfg = RenderConfig(tracing=Tracing(4, 3))
    world_p, world_d = _twin_worlds()
    piped, default = Engine(0, pipelined=True), Engine(0)
    previous = None
    for k in range(6):
        piped.renderWorld(world_p, cfg, sync=False)
        default.renderWorld(world_d, cfg, sync=False)
        cp, cd = world_p.camera, world_d.camera
        if previous is not None:
            assert np.array_equal(cp.image_buffer, previous[0]) and np.array_equal(cp.depth_buffer, previous[1]), f"call {k}"
            assert cp.ray_count == previous[2] and cp.raycasted_instance is not None
            assert world_p.instances.index(cp.raycasted_instance) == previous[3], f"call {k}"
        previous = (cd.image_buffer.copy(), cd.depth_buffer.copy(), cd.ray_count, world_d.instances.index(cd.raycasted_instance))
    # sync=True on the pipelined engine hands out the call's own frame
    piped.renderWorld(world_p, cfg, sync=True)
    default.renderWorld(world_d, cfg)
    assert np.array_equal(world_p.camera.image_buffer, world_d.camera.image_buffer)
    assert np.array_equal(world_p.camera.depth_buffer, world_d.camera.depth_buffer)


def test_cpp_engine_pipelined_frames_equal_a_synchronous_engine_one_call_behind(built, tmp_path):
    exe = str(tmp_path / "frame_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "frame_delivery_check.cpp"), "-o", exe, "-L", CSRC, "-lhiprz_host", "-lhiprz",
                    "-Wl,-rpath," + CSRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FRAME DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "compared 12 frames" in r.stdout
