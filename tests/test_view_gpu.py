"""The baked view on the GPU (include/hiprz_view.h: libhiprz_view.so, Context.view / view_samples / lit_source, Engine::bakedView).  The
samples of a view are held to the query library's own closest hits on Context.pixel_rays, the texel under a hit to a float64
reconstruction of the hit, and every pixel record to the numpy float32 restatement (tests/view_reference.py) over the emitted samples, the
hits' normals and the field through tests/field_reference.py's lookup, bit for bit.  Trees 0 (reference) and 3 (device SAH).

THE WORLD is tests/gather_world.py's: floor, cube and wall are in the atlas, the sphere is not, so both branches run in one frame.  CAMERAS
(view_reference.cameras): 32 x 24, 33 x 19 (partial blocks on both axes) and 1 x 1.  SOURCES: 64 x 48 and 4 x 3 (taps beyond every atlas
edge), one texel in nine without a value.  THE FIELD: a (4, 3, 4) grid over the world with random records, one of them invalid, and the
device's own visibility records.

  1 samples        t == Context.trace(Context.pixel_rays()).t in every byte, every id and code implied by the hit's flags, instance and
                   triangle through base, bx and by give the float64 reconstruction's nearest texel on all but the capped 1 %.
  2 pixels         == the restatement over the device's own samples for nearest and bilinear, without a field, with one and with
                   visibility records; the float image == the records' RGB with alpha 1.
  3 field pixels   == Context.lookup_field on the reconstructed points times the colour, in every byte; a textured unmapped instance
                   (albedo == read_guides' bytes) and an untextured emitter (the material's bytes / 255).
  4 known answers  a source of 1.0 gives exactly 1.0 on every ATLAS pixel under bilinear; an empty world is the sky's bytes, kind SKY;
                   from inside inward_box() there is no SKY pixel; lit_source is compose and dilation, and a view of a bake shows light.
  5 mutants        every mutant of the restatement is caught on the device's data (the emission mutant in case 3's world, which has an
                   emitter).
  6 moved          a view after update_instances == the restatement of the moved world, != the view before.
  7 both builds    the RZ_VIEW_ROWS build writes the shipped build's bytes on the cases of 2.
  8 refusals       in the header's order.
  9 C++            Engine::bakedView delivers Python's bytes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gather_reference as GR
import gather_world as GW
import view_reference as VR
from rayzath_amd import _abi, _hiprt, atlas, bake, field, gather, probe, scene_io, view
from rayzath_amd._lib import HiprzError
from rayzath_amd.engine import Context, RenderConfig
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND
from rayzath_amd.scene import Instance, Material, TextureBuffer, World, camera_struct, flatten, generate_cube, generate_sphere

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayzath_amd", "csrc")
TREES = (0, 3)
F = np.float32
SKY = (0.25, 0.5, 2.0)
LO, HI, SHAPE = (-3.0, 0.1, -3.0), (3.0, 2.6, 3.0), (4, 3, 4)
FIELD_PARAMS = dict(bias=0.02, max_back=8)
FILTERS = (view.NEAREST, view.BILINEAR)


def _world(camera=0, moved=False, extras=False, geometry=True):
    w = GW.world(moved=moved, geometry=geometry)
    w.camera = VR.cameras()[camera]
    if extras:       # two more objects outside the atlas: a textured sphere and an untextured emitter
        rng = np.random.default_rng(12)
        bitmap = rng.integers(0, 256, (8, 16, 4)).astype(np.uint8)
        textured = w.add(Material((10, 20, 30, 255), roughness=1.0, texture=TextureBuffer(bitmap), name="textured"))
        glowing = w.add(Material((250, 130, 40, 255), roughness=1.0, emission=2.5, name="glowing"))
        w.add(Instance(w.add(generate_sphere(8)), [textured], position=(1.9, 0.5, -1.6), scale=(0.5, 0.5, 0.5), name="textured sphere"))
        w.add(Instance(w.add(generate_cube()), [glowing], position=(-0.4, 0.3, -2.2), rotation=(0.0, 0.4, 0.0), scale=(0.5, 0.5, 0.5), name="emitter"))
    return w


def _context(tree, world):
    ctx = Context(0)
    if tree:
        ctx.set_tree(tree)
    flat = flatten(world)
    ctx.upload_scene(flat), ctx.upload_camera(camera_struct(world.camera))
    return ctx, flat


def _field_of(ctx, with_vis=True):
    """(grid, probes, sh, vis, params record) over the world: random records, the last one invalid; the device's visibility records"""
    rng = np.random.default_rng(21)
    n = int(np.prod(SHAPE))
    probes = probe.grid(LO, HI, SHAPE, near=1e-3, far=1e3)
    sh = np.zeros(n, probe.sh_dtype)
    sh["sh"][:, 0, :3] = rng.uniform(1.0, 2.0, (n, 3))
    sh["sh"][:, 1:, :3] = rng.uniform(-0.3, 0.3, (n, 8, 3))
    sh["sh"][n - 1, 0, 3] = np.array([probe.INVALID], np.uint32).view(F)[0]
    vis = ctx.bake_visibility(probes, (64, 2), 5, 2.0) if with_vis else None
    return field.grid_of(LO, HI, SHAPE), probes, sh, vis, field.params(**FIELD_PARAMS)


def _surface(ctx, flat, guides=None):
    """(origin, direction, normal, colour, emission, hits) per pixel from the query's own rays and hits; the colour is the material's bytes /
    255, or — for a material with a texture — `guides`' albedo"""
    rays = ctx.pixel_rays()
    hits = ctx.trace(rays)
    found = (hits["flags"] & HIT_FOUND) != 0
    m = flat.materials[np.where(found & (hits["material"] >= 0), hits["material"], 0)]
    color = (m["color"][..., :3].astype(F) / F(255.0)).astype(F)
    emission = m["emission"].astype(F)
    if guides is not None:
        color = np.where((m["texture"] >= 0)[..., None], guides["albedo"], color).astype(F)
    return rays["origin"], rays["direction"], hits["normal"], color, emission, hits


@pytest.fixture(scope="module")
def seen():
    """what a (tree, camera) pair shows, computed once: context-free arrays shared by cases 1, 2 and 5"""
    return {}


def _frame(seen, tree, camera):
    key = (tree, camera)
    if key not in seen:
        world = _world(camera)
        ctx, flat = _context(tree, world)
        try:
            base, uv = gather.chart_tables(GW.parts(world), len(flat.instances))
            samples = ctx.view_samples((base, uv))
            surface = _surface(ctx, flat)
            fld = _field_of(ctx)
            got = {}
            for SW, SH in VR.SOURCES:
                source = VR.source_of(SW, SH)
                for filter in FILTERS:
                    for name, f in (("none", None), ("plain", fld[:3] + (None, fld[4])), ("vis", fld)):
                        pixels, rgba = ctx.view(source, SW, SH, None, f, SKY, view.params(filter), rgba8=True)
                        got[SW, filter, name] = pixels
                        if name == "vis":
                            got[SW, filter, "rgba8"] = rgba
            host = ctx.viewer().pixels(VR.source_of(64, 48), 64, 48, samples.shape, fld, SKY, "bilinear", image=True)
            # the device-pointer call's float image alone (no records), and what tonemap_image makes of the records' image
            n = samples.size
            bufs = [_hiprt.DeviceBuffer.of(VR.source_of(64, 48)), _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer.of(VR.image_of(got[64, view.BILINEAR, "vis"])), _hiprt.DeviceBuffer(n * 4)]
            try:
                ctx.viewer().pixels_device(bufs[0].ptr, 64, 48, None, bufs[1].ptr, None, SKY, "bilinear")
                ctx.tonemap_image(bufs[2].ptr, bufs[3].ptr)
                ctx.sync()
                got["image"], got["tonemapped"] = bufs[1].download(samples.shape + (4,), F), bufs[3].download(samples.shape + (4,), np.uint8)
            finally:
                for b in bufs:
                    b.free()
        finally:
            ctx.close()
        seen[key] = dict(world=world, flat=flat, base=base, uv=uv, samples=samples, surface=surface, field=fld, got=got, host=host)
    return seen[key]


# =====================================================================================================================
# 1. the samples are the query's
# =====================================================================================================================
@pytest.mark.parametrize("camera", range(3))
@pytest.mark.parametrize("tree", TREES)
def test_samples_match_the_query(built, seen, tree, camera):
    s = _frame(seen, tree, camera)
    samples, hits, base, uv = s["samples"], s["surface"][5], s["base"], s["uv"]
    cam = camera_struct(s["world"].camera)
    assert samples.shape == hits.shape == (cam.height, cam.width) and samples.dtype == gather.sample_dtype
    assert samples["t"].tobytes() == hits["t"].tobytes(), f"t differs on {int((samples['t'].view(np.uint32) != hits['t'].view(np.uint32)).sum())} of {samples.size} pixels"
    assert np.array_equal(samples["id"], GR.ids(hits["flags"], hits["instance"], hits["triangle"], base, len(uv)))
    found = (hits["flags"] & HIT_FOUND) != 0
    assert np.array_equal(samples["id"] == gather.BACK, found & ((hits["flags"] & HIT_EXTERNAL) == 0)) and np.array_equal(samples["id"] == gather.MISS, hits["flags"] == 0)
    assert np.array_equal(samples["id"] == gather.UNMAPPED, found & ((hits["flags"] & HIT_EXTERNAL) != 0) & (hits["instance"] == GW.SPHERE)), "the sphere alone is outside the atlas"
    assert (samples["bx"][~found].view(np.uint32) == 0).all() and (samples["by"][~found].view(np.uint32) == 0).all()
    mapped = samples["id"] < gather.MAX_CHARTS
    assert np.array_equal(samples["id"][mapped] - base[hits["instance"][mapped]], hits["triangle"][mapped])
    # the texel from bx, by against float64 barycentrics of the same pixel's ray on the device's own triangle (tests/test_gather_gpu.py's
    # way: no second walk that could disagree about a silhouette), EVERY mapped pixel but the capped 1 % on a texel boundary
    rays = s["surface"][0], s["surface"][1]
    triangles = GW.world_triangles(s["world"], s["flat"])
    inst, tri_id = hits["instance"][mapped], hits["triangle"][mapped]
    tri = np.stack([triangles[i][t] for i, t in zip(inst, tri_id)]) if mapped.any() else np.zeros((0, 3, 3))
    _, bx, by, _ = GW.barycentrics(tri, rays[0][mapped].astype(np.float64), rays[1][mapped].astype(np.float64))
    c = uv[samples["id"][mapped]]
    b1 = (1.0 - bx) - by
    u64 = c["u1"] * b1 + c["u2"] * bx + c["u3"] * by
    v64 = c["v1"] * b1 + c["v2"] * bx + c["v3"] * by
    u32, v32, _ = GR.uv(samples[mapped], uv)
    for SW, SH in VR.SOURCES:
        edge = VR.on_a_boundary(u64, v64, SW, SH)
        assert edge.sum() <= VR.CAP * int(mapped.sum()), f"{int(edge.sum())} of {int(mapped.sum())} mapped pixels lie on a texel boundary"
        x64, y64, _ = GR.texel_of(u64, v64, SW, SH)
        x32, y32, _ = GR.texel_of(u32, v32, SW, SH)
        wrong = ~edge & ((x32 != x64) | (y32 != y64))
        print(f"tree {tree} camera {cam.width} x {cam.height} source {SW} x {SH}: {int(mapped.sum())} mapped pixels, {int((~edge).sum())} held to float64, {int(edge.sum())} on a boundary, {int(wrong.sum())} wrong")
        assert not wrong.any(), f"{int(wrong.sum())} of {int((~edge).sum())} texels differ from the float64 reconstruction"
    assert mapped.any(), "every camera, the 1 x 1 one included, looks at the atlas"
    if camera < 2:
        assert mapped.mean() > 0.3 and (samples["id"] == gather.UNMAPPED).sum() >= 3 and (samples["id"] == gather.MISS).any()


# =====================================================================================================================
# 2. every pixel record is the restatement's; 5. every mutant is caught
# =====================================================================================================================
@pytest.mark.parametrize("camera", range(3))
@pytest.mark.parametrize("tree", TREES)
def test_pixels_bit_for_bit(built, seen, tree, camera):
    s = _frame(seen, tree, camera)
    samples, surface, fld, uv = s["samples"], s["surface"][:5], s["field"], s["uv"]
    caught = {m: False for m in VR.MUTANTS}
    kinds = np.zeros(5, np.int64)
    for SW, SH in VR.SOURCES:
        source = VR.source_of(SW, SH)
        for filter in FILTERS:
            for name, f in (("none", None), ("plain", fld[:3] + (None, fld[4])), ("vis", fld)):
                got = s["got"][SW, filter, name]
                want = VR.pixels(samples, uv, source, SW, SH, SKY, filter, *surface, field=f)
                what = f"tree {tree} camera {camera} source {SW} x {SH} filter {filter} field {name}"
                assert got.dtype == view.pixel_dtype and got.shape == samples.shape
                assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words of {got.size * 4} differ from the restatement"
                kinds += np.bincount(view.kind(got).reshape(-1), minlength=5)
                for m in caught:
                    caught[m] |= VR.pixels(samples, uv, source, SW, SH, SKY, filter, *surface, field=f, mutant=m).tobytes() != got.tobytes()
        assert s["got"][SW, view.BILINEAR, "plain"].tobytes() != s["got"][SW, view.BILINEAR, "vis"].tobytes() or camera == 2, "the visibility records change no pixel"
        assert s["got"][SW, view.NEAREST, "none"].tobytes() != s["got"][SW, view.BILINEAR, "none"].tobytes() or camera == 2
    # the host-pointer call gives the device-pointer call's bytes; the float image is the records' RGB with alpha 1
    pixels, image = s["host"]
    assert pixels.tobytes() == s["got"][64, view.BILINEAR, "vis"].tobytes() and image.tobytes() == VR.image_of(pixels).tobytes()
    assert s["got"]["image"].tobytes() == VR.image_of(s["got"][64, view.BILINEAR, "none"]).tobytes(), "the device-pointer call's image, asked for alone, is not the records' RGB with alpha 1"
    rgba8 = s["got"][64, view.BILINEAR, "rgba8"]
    assert rgba8.shape == samples.shape + (4,) and rgba8.dtype == np.uint8 and rgba8.any()
    assert rgba8.tobytes() == s["got"]["tonemapped"].tobytes(), "view(rgba8=True) is not tonemap_image of the records' image"
    print(f"tree {tree} camera {camera}: pixels by kind (none, atlas, field, sky, back) {kinds.tolist()}, mutants caught {caught}")
    if camera < 2:
        assert all(v for m, v in caught.items() if m != "noemission"), caught          # (this world has no emitter: case 3 catches that one)
        assert kinds[view.ATLAS] and kinds[view.FIELD] and kinds[view.SKY] and kinds[view.NONE], "a frame shows the atlas, the field, the sky and texels without a value"


# =====================================================================================================================
# 3. FIELD pixels are lookup_field's on the reconstructed points, times the colour
# =====================================================================================================================
@pytest.mark.parametrize("tree", TREES)
def test_field_pixels_are_the_lookups(built, tree):
    world = _world(0, extras=True)
    ctx, flat = _context(tree, world)
    try:
        ctx.set_config(RenderConfig().struct())
        guides = ctx.read_guides()
        charts = gather.chart_tables(GW.parts(world), len(flat.instances))
        fld = _field_of(ctx)
        origin, direction, normal, color, emission, hits = _surface(ctx, flat, guides)
        samples = ctx.view_samples(charts)
        source = VR.source_of(64, 48)
        at = samples["id"] == gather.UNMAPPED
        for name, i in (("sphere", GW.SPHERE), ("textured sphere", 4), ("emitter", 5)):
            assert (at & (hits["instance"] == i)).sum() >= 3, f"the camera does not see the {name}"
        textured = at & (hits["instance"] == 4)
        assert len(np.unique(color[textured], axis=0)) >= 3 and (flat.materials[hits["material"][textured]]["texture"] >= 0).all(), "the texture shows more than one texel"
        assert (emission[at & (hits["instance"] == 5)] == F(2.5)).all() and not emission[at & (hits["instance"] != 5)].any()
        points = bake.points(VR.hit_points(origin, direction, samples["t"])[at], normal[at])
        for f in (fld, fld[:3] + (None, fld[4])):
            got = ctx.view(source, 64, 48, None, f, SKY, "bilinear")
            looked = ctx.lookup_field(f[0], f[1], f[2], points, f[3], f[4])
            assert (looked["word"] != field.INVALID).all() and (view.kind(got)[at] == view.FIELD).all()
            want = color[at] * looked["rgb"]
            want = np.where((emission[at] > 0)[:, None], want + color[at] * emission[at][:, None], want).astype(F)
            assert got["rgb"][at].tobytes() == want.tobytes(), f"tree {tree}: {int((got['rgb'][at].view(np.uint32) != want.view(np.uint32)).sum())} words differ from lookup_field x colour"
            assert np.array_equal(view.count(got)[at], looked["word"])
            assert got.tobytes() == VR.pixels(samples, charts[1], source, 64, 48, SKY, view.BILINEAR, origin, direction, normal, color, emission, field=f).tobytes()
            for m in VR.MUTANTS:
                wrong = VR.pixels(samples, charts[1], source, 64, 48, SKY, view.BILINEAR, origin, direction, normal, color, emission, field=f, mutant=m)
                assert wrong.tobytes() != got.tobytes(), f"tree {tree}: the mutant {m} is not caught on the device's data"
    finally:
        ctx.close()


# =====================================================================================================================
# 4. known answers
# =====================================================================================================================
def test_known_answers(built):
    ones = VR.source_of(64, 48)
    ones["rgb"] = 1.0
    for tree in TREES:
        world = _world(1)
        ctx, flat = _context(tree, world)
        try:
            got = ctx.view(ones, 64, 48, gather.chart_tables(GW.parts(world), len(flat.instances)), None, SKY, "bilinear")
            lit = view.kind(got) == view.ATLAS
            assert lit.sum() > 100 and (got["rgb"][lit] == 1.0).all(), "a source of 1.0 everywhere is not exactly 1.0 under bilinear"
            # the same map set again is not placed again and changes nothing; another map is placed, and the first one after it too
            base, uv = gather.chart_tables(GW.parts(world), len(flat.instances))
            assert ctx.view(ones, 64, 48, (base.copy(), uv.copy()), None, SKY, "bilinear").tobytes() == got.tobytes()
            without_floor = base.copy()
            without_floor[GW.FLOOR] = gather.NONE
            other = ctx.view(ones, 64, 48, (without_floor, uv), None, SKY, "bilinear")
            assert (view.kind(other) == view.ATLAS).sum() < lit.sum() and ctx.view(ones, 64, 48, (base, uv), None, SKY, "bilinear").tobytes() == got.tobytes()
        finally:
            ctx.close()
    empty = _world(1, geometry=False)
    ctx, flat = _context(0, empty)
    try:
        assert not len(flat.instances)
        no_charts = (np.zeros(0, np.uint32), np.zeros(0, gather.chart_dtype))
        for filter in FILTERS:
            got = ctx.view(ones, 64, 48, no_charts, None, SKY, view.params(filter))
            assert got.shape == (19, 33) and (got["word"] == view.SKY << 28).all(), "an empty world is not all sky"
            assert got["rgb"].tobytes() == np.tile(np.asarray(SKY, F), 19 * 33).tobytes(), "an empty world is not the sky's bytes"
        assert (ctx.view_samples()["id"] == gather.MISS).all()
    finally:
        ctx.close()
    room = World()
    grey = room.add(Material((200, 200, 200, 255), roughness=1.0, name="grey"))
    room.add(Instance(room.add(GW.inward_box()), [grey], position=(0.5, 3.5, -6.0), scale=(3.0, 2.0, 2.5), rotation=(0.2, 0.4, 0.1), name="room"))
    room.camera = VR.cameras()[1]
    full = VR.source_of(64, 48, holes=False)
    full["rgb"] = 1.0
    for tree in TREES:
        ctx, flat = _context(tree, room)
        try:
            got = ctx.view(full, 64, 48, gather.chart_tables([(0, atlas.charts(room.instances[0].mesh))], 1), None, SKY, "nearest")
            assert not (view.kind(got) == view.SKY).any() and (view.kind(got) == view.ATLAS).all() and (got["rgb"] == 1.0).all(), "from inside a closed room a pixel sees the sky"
        finally:
            ctx.close()


def test_lit_source_is_compose_and_dilation(built):
    """Context.lit_source is the gather's compose and the atlas's dilation, nothing of its own; a view of it shows the bake"""
    world = _world(0)
    ctx, flat = _context(3, world)
    try:
        parts, albedo = GW.parts(world), (0.75, 0.5, 0.25)
        direct, indirect, ring = ctx.bake_bounce_atlas(parts, GW.W, GW.H, albedo, None, 1, (16, 2), (4, 2), 3, 2, SKY, 1e-3, 1e3)
        source = ctx.lit_source(direct, indirect, albedo, None, 2)
        composed = GR.compose(direct, indirect, gather.records(albedo, direct.shape), None)
        assert source.dtype == gather.record_dtype and source.shape == (GW.H, GW.W) and source.tobytes() == ctx.atlas().dilate(composed, 2)[0].tobytes()
        got = ctx.view(source, GW.W, GW.H, gather.chart_tables(parts, len(flat.instances)), None, SKY, "bilinear")
        lit = view.kind(got) == view.ATLAS
        assert lit.mean() > 0.5 and (got["rgb"][lit] >= 0).all() and got["rgb"][lit].max() > 0, "a view of a bake shows no light"
        samples = ctx.view_samples()
        assert got.tobytes() == VR.pixels(samples, gather.chart_tables(parts, len(flat.instances))[1], source, GW.W, GW.H, SKY, view.BILINEAR).tobytes()
    finally:
        ctx.close()


# =====================================================================================================================
# 6. a view sees update_instances
# =====================================================================================================================
def test_a_view_sees_update_instances(built):
    world, moved = _world(0), _world(0, moved=True)
    ctx, flat = _context(3, world)
    try:
        charts = gather.chart_tables(GW.parts(world), len(flat.instances))
        source = VR.source_of(64, 48)
        before = ctx.view(source, 64, 48, charts, None, SKY, "bilinear")
        moved_flat = flatten(moved)
        ctx.update_instances(moved_flat.instances)
        after = ctx.view(source, 64, 48, None, None, SKY, "bilinear")
        assert after.tobytes() != before.tobytes(), "the view does not see the moved cube"
        samples = ctx.view_samples()
        want = VR.pixels(samples, charts[1], source, 64, 48, SKY, view.BILINEAR)
        assert after.tobytes() == want.tobytes()
    finally:
        ctx.close()
    fresh, _ = _context(3, moved)
    try:
        assert fresh.view(source, 64, 48, charts, None, SKY, "bilinear").tobytes() == after.tobytes(), "a view after update_instances differs from a fresh context's"
        assert fresh.view_samples().tobytes() == samples.tobytes()
    finally:
        fresh.close()


# =====================================================================================================================
# 7. both builds write the same bytes
# =====================================================================================================================
_CHILD = r"""
import sys
import numpy as np
import test_view_gpu as T
from rayzath_amd import view
out = []
seen = {}
for tree in T.TREES:
    for camera in range(3):
        s = T._frame(seen, tree, camera)
        out.append(s["samples"].view(np.uint32).reshape(-1))
        for key in sorted(k for k in s["got"] if isinstance(k, tuple) and k[2] != "rgba8"):
            out.append(s["got"][key].view(np.uint32).reshape(-1))
np.save(sys.argv[1], np.concatenate(out))
print(view.layout()[7], view.LIB_PATH)
"""


def test_both_builds_of_the_kernels_write_the_same_bytes(built, tmp_path):
    """the shipped library against the RZ_VIEW_ROWS build of the same source, each in a process of its own through HIPRZ_VIEW_LIB"""
    make = open(os.path.join(CSRC, "Makefile")).read()
    cxxflags = re.search(r"^CXXFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(INC)", f"-I{os.path.join(ROOT, 'include')} -I{CSRC}")
    hipflags = re.search(r"^HIPFLAGS = (.*)$", make, flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    shipped = view.layout()[7]
    other = str(tmp_path / "libhiprz_view_other.so")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, *cxxflags.split(), *hipflags.split(), *([] if shipped else ["-DRZ_VIEW_ROWS"]), "-Wno-undefined-inline", "-I", os.path.join(CSRC, "view"),
                    "-shared", os.path.join(CSRC, "view", "hiprz_view.hip"), os.path.join(CSRC, "view", "hiprz_view_host.cpp"), "-L", CSRC, "-lhiprz", f"-Wl,-rpath,{CSRC}", "-o", other],
                   check=True, capture_output=True, timeout=600)
    results = {}
    for name, lib in (("shipped", None), ("other", other)):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
        env.pop("HIPRZ_VIEW_LIB", None)
        if lib:
            env["HIPRZ_VIEW_LIB"] = lib
        path = str(tmp_path / f"{name}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        form = r.stdout.strip().splitlines()[-1].split()
        assert form[1] == (lib or view.LIB_PATH) and int(form[0]) == (shipped if lib is None else 1 - shipped)
        results[name] = np.load(path)
    assert len(results["shipped"]) == 4 * 13 * 2 * (32 * 24 + 33 * 19 + 1)
    assert results["shipped"].tobytes() == results["other"].tobytes(), "the two forms of the kernels differ in some byte"


# =====================================================================================================================
# 8. refusals in the header's order
# =====================================================================================================================
def test_refusals_in_the_headers_order(built):
    ctx = Context(0)
    try:
        v = ctx.viewer()
        dev = 16          # a device address that is never read: every call below is refused
        grid, probes, sh, _, fp = _field_of(ctx, with_vis=False)
        bad_grid, bad_fp = grid.copy(), fp.copy()
        bad_grid["step"][1], bad_fp["bias"] = 0.0, -1.0
        bad_params = view.params().copy()
        bad_params["filter"] = 7
        n = probes.size

        def refused(code, text, call, *args, **kwargs):
            with pytest.raises(HiprzError) as e:
                call(*args, **kwargs)
            assert e.value.code == code and text in str(e.value), (code, text, str(e.value))

        wrong = (bad_grid, dev, dev, None, n, bad_fp)
        refused(_abi.ERR_INVALID, "null pointer", v.pixels_device, None, 0, 0, dev, None, wrong, SKY, bad_params)
        refused(_abi.ERR_INVALID, "null pointer", v.pixels_device, dev, 0, 0, None, None, wrong, SKY, bad_params)
        refused(_abi.ERR_INVALID, "null pointer", v.pixels_device, dev, 0, 0, dev, None, (bad_grid, None, dev, None, n, bad_fp), SKY, bad_params)
        refused(_abi.ERR_STATE, "no chart map", v.pixels_device, dev, 0, 0, dev, None, wrong, SKY, bad_params)
        refused(_abi.ERR_STATE, "no chart map", v.samples_device, dev)
        not_finite = np.zeros(1, gather.chart_dtype)
        not_finite["v3"] = np.nan
        with pytest.raises(HiprzError):
            v.set_charts(np.zeros(1, np.uint32), not_finite)
        refused(_abi.ERR_STATE, "no chart map", v.samples_device, dev)          # what was set before stays: nothing
        v.set_charts(*gather.chart_tables(GW.parts(GW.world()), 4))
        for W, H in ((0, 48), (64, 0), (16385, 48), (64, 16385)):
            refused(_abi.ERR_INVALID, "W or H", v.pixels_device, dev, W, H, dev, None, wrong, SKY, bad_params)
        refused(_abi.ERR_INVALID, "filter", v.pixels_device, dev, 64, 48, dev, None, wrong, SKY, bad_params)
        refused(_abi.ERR_INVALID, "grid step", v.pixels_device, dev, 64, 48, dev, None, wrong, SKY, "bilinear")
        refused(_abi.ERR_INVALID, "do not multiply", v.pixels_device, dev, 64, 48, dev, None, (grid, dev, dev, None, n - 1, bad_fp), SKY, "bilinear")
        refused(_abi.ERR_INVALID, "bias", v.pixels_device, dev, 64, 48, dev, None, (grid, dev, dev, None, n, bad_fp), SKY, "bilinear")
        refused(_abi.ERR_STATE, "", v.pixels_device, dev, 64, 48, dev, None, (grid, dev, dev, None, n, fp), SKY, "bilinear")          # no scene: whatever hiprz_device_view refuses
        refused(_abi.ERR_STATE, "", v.samples_device, dev)
        world = _world(2)
        flat = flatten(world)
        ctx.upload_scene(flat)
        refused(_abi.ERR_STATE, "camera", v.samples_device, dev)                # a scene without a camera
        ctx.upload_camera(camera_struct(world.camera))
        v.set_charts(np.zeros(3, np.uint32), np.zeros(0, gather.chart_dtype))
        refused(_abi.ERR_INVALID, "another number of instances", v.samples_device, dev)
        refused(_abi.ERR_INVALID, "another number of instances", v.pixels_device, dev, 64, 48, dev)
        assert ctx.view_samples(gather.chart_tables(GW.parts(world), 4)).shape == (1, 1)
    finally:
        ctx.close()


# =====================================================================================================================
# 9. the C++ Engine delivers Python's bytes
# =====================================================================================================================
def test_cpp_engine_views(built, tmp_path):
    exe = str(tmp_path / "view_delivery_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "view_delivery_check.cpp"), "-o", exe,
                    "-L", CSRC, "-lhiprz_host", "-lhiprz_view", "-lhiprz", "-Wl,-rpath," + CSRC], check=True)
    scene_path = str(tmp_path / "view.json")
    world = _world(1)
    scene_io.save_scene_json(world, scene_path)
    loaded = scene_io.load_scene_file(scene_path)
    source = VR.source_of(64, 48)
    ctx = Context(0)
    try:
        ctx.upload_scene(loaded.flat), ctx.upload_camera(loaded.camera)
        base, uv = gather.chart_tables(GW.parts(world), 4)
        grid, probes, sh, vis, fp = _field_of(ctx)
        pixels = ctx.view(source, 64, 48, (base, uv), (grid, probes, sh, vis, fp), SKY, "bilinear")
        plain = ctx.view(source, 64, 48, None, None, SKY, "bilinear")
    finally:
        ctx.close()
        loaded.close()
    assert pixels.shape == (19, 33) and pixels.tobytes() != plain.tobytes() and (view.kind(pixels) == view.FIELD).any()
    files = {name: str(tmp_path / (name + ".bin")) for name in ("source", "base", "uv", "probes", "grid", "sh", "vis", "out")}
    source.tofile(files["source"]), base.tofile(files["base"]), uv.tofile(files["uv"]), probes.tofile(files["probes"]), grid.tofile(files["grid"])
    sh.tofile(files["sh"]), vis.tofile(files["vis"])
    r = subprocess.run([exe, scene_path, files["source"], "64", "48", files["base"], files["uv"], files["probes"], files["grid"], files["sh"], files["vis"], files["out"],
                        str(view.BILINEAR), repr(FIELD_PARAMS["bias"]), str(FIELD_PARAMS["max_back"])], capture_output=True, text=True, timeout=120)
    print("\n" + r.stdout[-2000:])
    assert r.returncode == 0 and "VIEW DELIVERY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert open(files["out"], "rb").read() == pixels.tobytes(), "Engine::bakedView differs from Context.view"
    assert open(files["out"] + ".image", "rb").read() == VR.image_of(pixels).tobytes(), "Engine::bakedView's image differs from the records"
    assert open(files["out"] + ".plain", "rb").read() == plain.tobytes(), "Engine::bakedView without a field differs from Context.view"
