"""The resident batch kernel in pass segments (rz_batch_seg_kernel, HIPRZ_BATCH_SEGMENTS): every tile's passes of a render call cut
into S self-scheduled segments, the path state handed from one segment to the next through HBM.  Per pixel the arithmetic is that of
the unsegmented kernel, so frames, path state and the counters of a counted render are equal bit for bit to S = 1 — across several
calls in a row (the per-tile epochs of consecutive launches), for pass counts that S does not divide, on a frame whose grid fits the
chip at once (where the default keeps the unsegmented kernel) and in the hosts' two-stream packaging (two contexts, one scene).
"""
import numpy as np
import pytest

from rayzath_amd import scenes
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

_SCENES = {}


def scene(name):
    if name not in _SCENES:
        preset = scenes.CONFIGS[name]
        world = preset["build"]()
        _SCENES[name] = (flatten(world), camera_struct(world.camera), preset["max_depth"])
    return _SCENES[name]


def run(monkeypatch, name, segments, calls, device=0):
    """render(n) for every n of `calls`, then one counted render of 8 passes; everything the frame holds afterwards.
    segments: HIPRZ_BATCH_SEGMENTS (read when the context is created), None = the library's choice."""
    if segments is None:
        monkeypatch.delenv("HIPRZ_BATCH_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("HIPRZ_BATCH_SEGMENTS", str(segments))
    flat, cam, depth = scene(name)
    ctx = Context(device)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(RenderConfig(tracing=Tracing(depth, 8)).struct())
    for n in calls:
        ctx.render(n)
    ctx.tonemap()
    out = dict(accum=ctx.read_accum(), rgba8=ctx.read_rgba8(), **ctx.read_state())
    out["counters"] = ctx.render_counted(8)
    ctx.tonemap()
    out["accum_after_count"], out["rgba8_after_count"] = ctx.read_accum(), ctx.read_rgba8()
    out["rays"] = ctx.ray_count()
    return out


def assert_same(got, want, label):
    for key, value in want.items():
        if isinstance(value, np.ndarray):
            assert np.array_equal(got[key], value), f"{label}: {key} differs from S = 1"
        else:
            assert got[key] == value, f"{label}: {key} {got[key]} != {value} (S = 1)"


def test_full_size_several_calls(monkeypatch):
    """B at 1920x1080, 8 passes per call, three calls + a counted one: the epochs of four launches in a row on one frame."""
    calls = (8, 8, 8)
    want = run(monkeypatch, "B", 1, calls)
    assert want["counters"]["segments"] == 8 * 1920 * 1080
    for s in (None, 2, 3, 4):
        assert_same(run(monkeypatch, "B", s, calls), want, f"B, S = {s}")


@pytest.mark.parametrize("passes", [5, 7])
def test_odd_pass_counts(monkeypatch, passes):
    """Pass counts S does not divide: segments of n // S and n // S + 1 passes."""
    calls = (1, passes, passes)
    want = run(monkeypatch, "B", 1, calls)
    for s in (2, 3, 4):
        assert_same(run(monkeypatch, "B", s, calls), want, f"B, {passes} passes, S = {s}")


def test_grid_within_the_chip(monkeypatch):
    """A (256x256: 256 tiles, one round of the chip): the default keeps the unsegmented kernel; forced segments give the same frame."""
    calls = (8, 8)
    want = run(monkeypatch, "A", 1, calls)
    for s in (None, 2, 3, 4):
        assert_same(run(monkeypatch, "A", s, calls), want, f"A, S = {s}")


def test_two_streams_one_scene(monkeypatch):
    """The hosts' packaging of B: two contexts on one GPU with one scene copy, tiles interleaved; each runs its own segmented launches."""
    calls = (8, 8)
    want = run(monkeypatch, "B", 1, calls, device=[0, 0])
    for s in (None, 2, 4):
        assert_same(run(monkeypatch, "B", s, calls, device=[0, 0]), want, f"B on two streams, S = {s}")
