"""The stagings of a multi-part head (hiprz_ctx.hpp: PartStaging) under one asynchronous chain of all their consumers.

A head context collects its peers' tile-major buffers in two staging buffers: `gather` (frame assembly for the reads and the denoiser, the
sums of sample mode, the path state, the history of a restart) and the staging of hiprz_present.  The peers push on their own streams,
which run ahead of the head's: a push may only overwrite a staging once the last kernel that reads it is done.  Here every consumer
follows the previous one with no host synchronisation in between, and every array the chain hands out has to be the one a twin context
hands out that calls sync() after each step — a push that overtook a reader shows as a difference.

Shapes where the slice arithmetic can go wrong: parts of unequal size with a clipped last tile column, parts that own nothing, and a
context that renders one shard of two and so does not hold the whole frame (pixels of the other shard stay zero).
"""
import ctypes as C

import numpy as np
import pytest

from rayzath_amd import scenes
from rayzath_amd.engine import COMPAT_REPROJECTION, SHARD_SAMPLES, SHARD_TILES, Context, RenderConfig, Tracing, denoise_params
from rayzath_amd.scene import Camera, camera_struct, flatten

pytestmark = pytest.mark.gpu


def _moved(camera):
    return Camera(position=tuple(np.asarray(camera.position) + np.array([0.25, 0.1, 0.05], dtype=np.float32)),
                  rotation=tuple(np.asarray(camera.rotation) + np.array([0.02, -0.06, 0.0], dtype=np.float32)),
                  resolution=(camera.width, camera.height), fov=camera.fov, near_far=camera.near_far,
                  focal_distance=camera.focal_distance, aperture=camera.aperture, exposure_time=camera.exposure_time)


def _hip():
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")                     # the runtime libhiprz.so itself is linked against
    hip.hipMalloc.argtypes, hip.hipMemset.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return hip


def _chain(world, parts, shard, synchronous):
    """Runs the chain on a fresh context over `parts` streams of GPU 0; returns [(what, array or tuple)] in the order it was handed out."""
    hip = _hip()
    flat, cam, cam_moved = flatten(world), camera_struct(world.camera), camera_struct(_moved(world.camera))
    ctx = Context([0] * parts)
    out = []

    def step(call, *args, **kwargs):
        result = call(*args, **kwargs)
        if synchronous:
            ctx.sync()
        return result

    def frame(seq):
        f = step(ctx.read_frame, seq, copy=True)
        out.append((f"frame {seq}", f["rgba8"])), out.append((f"frame {seq} depth", f["depth"]))
        out.append((f"frame {seq} record", (f["passes"], f["sequence"], f["ray_count"], f["hit"])))

    if shard:
        ctx.set_shard(*shard)
    ctx.set_variance(1)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(RenderConfig(tracing=Tracing(4, 4)).struct())
    capacity = ctx.local_pixel_capacity()
    tiles = C.c_void_p()
    assert hip.hipMalloc(C.byref(tiles), capacity * 16) == 0
    hip.hipMemset(tiles, 0, capacity * 16)
    hip.hipDeviceSynchronize()  # (the memset is on the null stream; the context's streams are non-blocking and do not wait for it)

    step(ctx.render, 1), step(ctx.render, 3)
    if not shard:  # (a context that does not hold the frame refuses to denoise it)
        step(ctx.set_denoise, denoise_params(variance=True))  # the present assembles accumulator and variance through `gather`
    step(ctx.present, 3, 2)
    step(ctx.set_denoise, None)
    step(ctx.render, 3)
    step(ctx.present, ctx.width - 1, ctx.height - 1)
    frame(1), frame(2)
    out.append(("variance", step(ctx.read_variance)))
    out.append(("accum", step(ctx.read_accum)))
    out.extend((f"state {k}", v) for k, v in step(ctx.read_state).items())
    step(ctx.export_accum_tiles, tiles.value, capacity * 16)
    step(ctx.set_mode, COMPAT_REPROJECTION)
    step(ctx.upload_camera, cam_moved)  # restarts the frame: the head assembles the history of the previous one from all its parts
    step(ctx.render, 1), step(ctx.render, 3)
    out.append(("accum after the restart", step(ctx.read_accum)))
    step(ctx.set_shard_mode, SHARD_SAMPLES)
    step(ctx.render, 1), step(ctx.render, 3)
    step(ctx.tonemap)
    out.append(("summed accum", step(ctx.read_accum)))
    out.append(("summed variance", step(ctx.read_variance)))
    step(ctx.present, 5, 5)
    frame(0)
    step(ctx.set_shard_mode, SHARD_TILES)
    step(ctx.render, 1), step(ctx.render, 2)
    out.append(("accum back in tile mode", step(ctx.read_accum)))

    ctx.sync()
    exported = np.zeros((capacity, 4), dtype=np.float32)
    assert hip.hipMemcpy(exported.ctypes.data, tiles, exported.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    hip.hipFree(tiles)
    out.append(("exported tiles", exported))
    ctx.close()
    return out


@pytest.mark.parametrize("scene, width, height, parts, shard", [
    ("cornell", 40, 24, 4, None),        # 6 tiles: the parts own 2, 2, 1, 1; the last tile column is clipped
    ("cornell", 32, 8, 3, None),         # 1 tile: two parts own nothing
    ("cornell", 40, 24, 2, (1, 2)),      # the context does not hold the frame: zeros elsewhere, the images are cleared first
    ("living room", 40, 24, 4, None),    # lights: deferred shadow rays, sorted ray order
])
def test_asynchronous_chain_of_every_staging_consumer_equals_a_synchronised_twin(built, scene, width, height, parts, shard):
    world = scenes.cornell_box(width, height) if scene == "cornell" else scenes.living_room(width, height, 16)
    chained, twin = _chain(world, parts, shard, False), _chain(world, parts, shard, True)
    assert [what for what, _ in chained] == [what for what, _ in twin]
    for (what, got), (_, want) in zip(chained, twin):
        if isinstance(want, tuple):
            assert got == want, what
        else:
            differing = int((got != want).sum()) if got.shape == want.shape else -1
            assert np.array_equal(got, want), f"{what}: {differing} of {want.size} values differ from the synchronised twin"
    accum = dict(chained)["accum"]
    if shard:  # half the tiles are another context's: nothing of this one's wrote them
        assert 0 < (accum[..., 3] > 0).sum() < width * height
    else:
        assert (accum[..., 3] > 0).all()
