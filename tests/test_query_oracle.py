"""The reference of the ray queries, on the CPU oracle alone (tests/query_reference.py): that rzo_first_hit through a 1x1 camera answers
for an arbitrary ray, that the recipe's rays are worth walking, and that the comparison catches the oracle's geometry mutants.

  the proof   the 1x1-camera record of (position, pixel_d0(x, y)) equals rzo_first_hit_frame's record on EVERY pixel of the 118 scenes of
              tests/guide_scenes.py, all 64 bytes (126 885 pixels).
  the recipe  conditions, not measurements: at least 3 000 rays, at least 50 % of them hit, at least 25 % in every scene whose rays start
              on hit pixels, at least 500 hits from the inside.  Measured here: 3 264 rays from hit pixels on 102 scenes and 128 frustum
              rays on the 16 others (3 392 in all); 2 307 of them hit (68.0 %), 1 067 from the inside; the lowest scene has 50.0 % hits.
              The 16 sparse scenes are 3 empty worlds, whose rays all miss (asserted), a scene that looks away, and 12 frames of ONE pixel:
              their frustum rays cover the pixel's footprint, not its centre, and 66 of them do hit — they are held to the oracle like
              every other ray.
  power       each geometry mutant of the oracle shows in a geometric field (found, t bits, instance, scene_triangle, triangle, slot,
              material, external) of at least one ray of the pixel rays (rzo_first_hit_frame of the mutant: the same rays by the proof)
              plus the recipe's rays.  Rays that differ, pixel rays + recipe rays: mut_tie_later 873 + 26, mut_leaf_eight 33 360 + 527,
              mut_size_second 40 033 + 78, mut_slot_wrap 184 + 5, mut_slot_last 731 + 54.
              mut_abs_scale shows on NO ray in those fields: it transforms the normals of mirrored instances with the scale's magnitude and
              touches no walk, so it cannot change which triangle is met or where.  It shows in `normal` alone (11 742 pixel rays + 453
              recipe rays beyond the far rule), the field the GPU sweep holds under guide_scenes' far rule; asserted below as such.
"""
import numpy as np
import pytest

import guide_scenes as GS
import oracle
import query_reference as QR
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND

THREADS = 8
GEOMETRY_MUTANTS = ("mut_tie_later", "mut_leaf_eight", "mut_size_second", "mut_abs_scale", "mut_slot_wrap", "mut_slot_last")
NORMAL_ONLY = ("mut_abs_scale",)
CHUNK = 8
CHUNKS = [GS.SCENES[i:i + CHUNK] for i in range(0, len(GS.SCENES), CHUNK)]


def test_there_are_118_scenes():
    assert len(GS.SCENES) == 118 and len(set(GS.SCENES)) == 118


@pytest.mark.parametrize("chunk", range(len(CHUNKS)))
def test_one_pixel_camera_walks_the_pixel_ray(built, chunk):
    """the reference's own proof: all 64 bytes of rzo_first_hit under the 1x1 camera equal rzo_first_hit_frame's, on every pixel"""
    pixels = 0
    for key in CHUNKS[chunk]:
        flat, cam = GS.flat_scene(key)[:2]
        frame = GS.records(key, 0, threads=THREADS)
        d0 = QR.frame_d0(cam)
        position = np.array(cam.position[:], np.float32)
        one = type(cam).from_buffer_copy(cam)
        one.width = one.height = 1
        for y in range(cam.height):
            for x in range(cam.width):
                one.position[:] = position.tolist()
                one.z_axis[:] = d0[y, x].tolist()
                got = oracle.first_hit(flat, one, 0, 0, 0)
                assert got.tobytes() == frame[y, x].tobytes(), (key, x, y, got, frame[y, x])
        pixels += frame.size
    print(f"chunk {chunk}: {pixels} pixels, every 1x1-camera record equals the frame's")


def test_as_hits_is_the_record(built):
    """the hit_dtype view of a frame's records: found / external in flags, -1 / -1 / -1 / 0 / -1 and +0 on a miss, t = depth"""
    rec = GS.records("slots", 0, threads=THREADS)
    hits = QR.as_hits(rec)
    found = (hits["flags"] & HIT_FOUND) != 0
    assert found.any() and (~found).any()
    assert np.array_equal(found, rec["instance"] != 0xFFFFFFFF) and np.array_equal(hits["t"], rec["depth"])
    assert np.array_equal((hits["flags"] & HIT_EXTERNAL) != 0, (rec["external"] != 0) & found)
    flat, cam = GS.flat_scene("slots")[:2]
    assert QR.misses_read_as_specified(hits, QR.pixel_rays_d0(cam))
    assert np.array_equal(hits["triangle"][found], flat.tris["source_index"][hits["scene_triangle"][found]])


def test_the_recipe_is_deterministic_and_worth_walking(built):
    total = hit = internal = dense_scenes = sparse_rays = sparse_hits = blind_scenes = 0
    lowest = (1.0, None)
    for key in GS.SCENES:
        rays, dense = QR.scene_rays(key)
        ref = QR.scene_reference(key)
        found = (ref["flags"] & HIT_FOUND) != 0
        total += len(rays)
        hit += int(found.sum())
        internal += int((found & ((ref["flags"] & HIT_EXTERNAL) == 0)).sum())
        assert (rays["direction"] != 0).all() and np.isfinite(rays["direction"]).all() and np.isfinite(rays["origin"]).all()
        if dense:
            dense_scenes += 1
            assert len(rays) >= QR.RAYS_PER_SCENE - 4, (key, len(rays))
            share = found.mean()
            lowest = min(lowest, (share, key), key=lambda p: p[0])
            assert share >= 0.25, (key, share)
        else:
            sparse_rays += len(rays)
            sparse_hits += int(found.sum())
            if not len(GS.flat_scene(key)[0].instances):     # an empty world
                blind_scenes += 1
                assert not found.any(), key
            assert QR.misses_read_as_specified(ref, rays)
    print(f"recipe: {total} rays ({sparse_rays} of them frustum rays of the {len(GS.SCENES) - dense_scenes} sparse scenes), {hit} hit ({hit / total:.1%}), "
          f"{internal} from the inside; lowest scene {lowest[1]!r} at {lowest[0]:.1%}; {sparse_hits} frustum rays hit, none in the {blind_scenes} empty worlds")
    assert len(GS.SCENES) - dense_scenes == 16
    assert total >= 3000 and hit >= 0.5 * total and internal >= 500
    import zlib
    assert QR.seed_of("slots") == zlib.crc32(b"'slots'") and QR.seed_of(8) == zlib.crc32(b"8")     # no hash salt in the seed


def test_oracle_ray_is_invariant_to_the_other_axes(built):
    """any finite x_axis / y_axis: dx = dy = 0 under the 1x1 camera"""
    key = "inside_sphere"
    flat, cam = GS.flat_scene(key)[:2]
    rays = QR.scene_rays(key)[0][:8]
    other = type(cam).from_buffer_copy(cam)
    other.x_axis[:] = [3.5, -2.0, 0.25]
    other.y_axis[:] = [-7.0, 0.5, 11.0]
    assert QR.oracle_rays(flat, other, rays).tobytes() == QR.scene_reference(key)[:8].tobytes()


@pytest.mark.parametrize("mutant", GEOMETRY_MUTANTS)
def test_the_rays_catch_the_geometry_mutants(built, mutant):
    pixel = recipe = pixel_normal = recipe_normal = 0
    for key in GS.SCENES:
        plain, mutated = QR.as_hits(GS.records(key, 0, threads=THREADS)), QR.as_hits(GS.records(key, 0, mutant, threads=THREADS))
        pixel += int(QR.geometric_differs(mutated, plain).sum())
        pixel_normal += QR.compare(mutated, plain, 0)["far"]
        ref, mut = QR.scene_reference(key), QR.scene_reference(key, mutant)
        recipe += int(QR.geometric_differs(mut, ref).sum())
        recipe_normal += QR.compare(mut, ref, 0)["far"]
    print(f"{mutant}: a geometric field differs on {pixel} pixel rays + {recipe} recipe rays; normal / u / v alone beyond the far rule on {pixel_normal} + {recipe_normal}")
    if mutant in NORMAL_ONLY:      # named in the module's docstring with the reason
        assert pixel + recipe == 0 and pixel_normal > 0 and recipe_normal > 0
    else:
        assert pixel + recipe > 0
