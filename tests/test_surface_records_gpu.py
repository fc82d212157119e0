"""Surface records on the device (RZ_SURFACE_RECORDS: the kernels that stage the scene in LDS read a hit's normal, mapped normal and
material ids from per-(instance, triangle, side) records behind the hot buffer — hiprz_device.hpp: surface_from_record — instead of
deriving them in analyze_intersection).

Every world is rendered 1 + 8 passes through three launch forms — the resident pipeline, the split pipeline, and nine render(1) calls on
the default pipeline — by contexts whose launch plan stages the scene (asserted), and each form's accumulator must equal, with
np.array_equal, that of a twin under set_lds_scene(0), whose kernels read the scene from global memory and compute every normal per hit.
Then render_counted(2): all ten of the twin's counters.  Frames are 64 x 48 (12 tiles), one is 72 x 20 (partial tiles).

  cornell, behind    config B's room with the camera inside, and behind the back wall: both sides of the open wall meshes are hit
  placements         a non-uniform scale, a mirrored instance, two instances of one mesh
  smooth_1, smooth_2 spheres with vertex normals (48 triangles, inner roots) under set_traversal_mode(1) and (2): the normal comes from the
                     record, the mapped normal is interpolated per hit
  normal_mapped      a normal-mapped textured quad (those hits compute everything as before) beside a textured cube (texture coordinates per
                     hit, normals from the record)
  extremes           a zero-area triangle, scales of 3e19 and 5e-20 across a quad: flagged records, lanes that compute as before beside
                     lanes that read (tests/surface_scenes.py says why the small scale is not 1e-20)
  material_slots     slots inside, unset, beyond the instance's table and beyond 63
  spot_lit           next-event estimation: the general shading variant with inline shadow rays
  partial_72x20      config B's room on a frame of partial tiles

Further: a second upload_scene of another world into the same contexts (the section is replaced with the scene), and a context of two
streams on one GPU (one scene copy, both streams read its section).
"""
import numpy as np
import pytest

import surface_scenes
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import camera_struct, flatten

pytestmark = pytest.mark.gpu

CASES = {
    "cornell": (surface_scenes.cornell, None),
    "behind": (surface_scenes.cornell_from_behind, None),
    "placements": (surface_scenes.placements, None),
    "smooth_1": (surface_scenes.vertex_normals, 1),
    "smooth_2": (surface_scenes.vertex_normals, 2),
    "normal_mapped": (surface_scenes.normal_mapped, None),
    "extremes": (surface_scenes.extremes, None),
    "material_slots": (surface_scenes.material_slots, None),
    "spot_lit": (surface_scenes.spot_lit, None),
    "partial_72x20": (lambda: surface_scenes.cornell(72, 20), None),
}
FORMS = (("resident pipeline", 2, False), ("split pipeline", 1, False), ("one render(1) at a time", None, True))


def _config():
    return RenderConfig(tracing=Tracing(6, 8)).struct()


def _context(flat, cam, device=0, mode=None, pipeline=None, lds_scene=None):
    ctx = Context(device)
    if lds_scene is not None:
        ctx.set_lds_scene(lds_scene)
    if mode is not None:
        ctx.set_traversal_mode(mode)
    if pipeline is not None:
        ctx.set_pipeline(pipeline)
    ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(_config())
    return ctx


_twins = {}


def _twin(name):
    """(flat, cam, accumulator after 1 + 8 passes, counters of 2 more) of the case on a context that never stages the scene: computed once"""
    if name not in _twins:
        world = CASES[name][0]()
        flat, cam = flatten(world), camera_struct(world.camera)
        twin = _context(flat, cam, lds_scene=0)
        twin.render(1), twin.render(8)
        assert twin.launch_plan()[3] == 0, "the twin stages nothing"
        accum = twin.read_accum()
        counted = twin.render_counted(2)
        twin.close()
        assert np.isfinite(accum).all() and counted["hits"] > 0
        _twins[name] = (flat, cam, accum, counted)
    return _twins[name]


def _render_form(ctx, pipeline, one_at_a_time):
    if one_at_a_time:
        for _ in range(9):
            ctx.render(1)
    else:
        ctx.render(1), ctx.render(8)
        assert ctx.pipeline() == pipeline
    assert ctx.launch_plan()[3] == 1, "the scene is staged in LDS: these are the kernels that read the records"


@pytest.mark.parametrize("name", list(CASES))
def test_frames_equal_the_unstaged_twin(name):
    flat, cam, want_accum, want_counted = _twin(name)
    mode = CASES[name][1]
    for label, pipeline, one_at_a_time in FORMS:
        ctx = _context(flat, cam, mode=mode, pipeline=pipeline)
        _render_form(ctx, pipeline, one_at_a_time)
        accum = ctx.read_accum()
        differ = int((accum != want_accum).any(-1).sum())
        assert np.array_equal(accum, want_accum), f"{name}, {label}: {differ} pixels of the accumulator differ from the twin's after 1 + 8 passes"
        counted = ctx.render_counted(2)
        print(f"{name}, {label}: {counted}")
        assert counted == want_counted, f"{name}, {label}: counters {counted} != {want_counted} (twin)"
        ctx.close()


def test_a_second_upload_replaces_the_section():
    """placements, then config B's room (fewer instances, other meshes) into the SAME context: the frames are those of fresh twins"""
    first, second = _twin("placements"), _twin("cornell")
    for label, pipeline, one_at_a_time in FORMS:
        ctx = _context(first[0], first[1], pipeline=pipeline)
        _render_form(ctx, pipeline, one_at_a_time)
        assert np.array_equal(ctx.read_accum(), first[2]), label
        ctx.upload_scene(second[0]), ctx.upload_camera(second[1])
        _render_form(ctx, pipeline, one_at_a_time)
        assert np.array_equal(ctx.read_accum(), second[2]), f"{label}: after the second upload"
        ctx.close()


def test_two_streams_share_one_section():
    flat, cam, want_accum, want_counted = _twin("placements")
    ctx = _context(flat, cam, device=[0, 0])
    ctx.render(1), ctx.render(8)
    assert np.array_equal(ctx.read_accum(), want_accum)
    assert ctx.render_counted(2) == want_counted
    ctx.close()
