"""The oracle for the first hit (rzo_first_hit, rzo_ray_cast of oracle/rz_oracle.c), the scenes of tests/guide_scenes.py and the rule
that tests/test_guides_oracle_gpu.py holds hiprz_read_guides and hiprz_ray_cast to, proven on the CPU: the records agree with what the
oracle already computes (rzo_pick, the first pass's depth buffer), the scenes contain every kind of first hit a guide kernel treats
differently, the libm stand-ins stay under the caps made from them, and the rule catches each guide mutant of oracle/Makefile standing in
for the device — in the modes its bug lives in, and nowhere else.  Run with -s for the tables."""
import ctypes as C

import numpy as np
import pytest

import guide_scenes as GS
import lockstep
import oracle
from guide_scenes import bad
from rayzath_amd import _abi

FILTERING_MODES = tuple(m for m in GS.MODES if m & 16)
TEXTURE_MULT_MODES = tuple(m for m in GS.MODES if m & 8)
# mutant -> the modes its bug lives in
MUTANTS = {"guide_no_flip": GS.MODES, "guide_map_scaled": GS.MODES, "guide_color_only": GS.MODES, "guide_emissive_albedo": GS.MODES,
           "guide_point_fetch": FILTERING_MODES, "guide_replace": TEXTURE_MULT_MODES}
OLDER_MUTANTS = ("slot_wrap", "slot_last", "abs_scale")


def test_new_scenes_are_small_and_the_validator_accepts_them(built):
    from rayzath_amd import _lib
    lib = _lib.load()
    assert len(GS.SCENES) == len(set(GS.SCENES)) == 60 + 48 + len(GS.NEW)
    for name in GS.NEW:
        flat, cam = GS.flat_scene(name)[:2]
        assert cam.width <= 48 and cam.height <= 32 or (cam.width, cam.height) == (33, 33), name
        msg = C.create_string_buffer(256)
        assert lib.hiprz_validate_scene(C.byref(flat.struct), msg, 256) == 0, (name, msg.value.decode())
        again = GS.world(name)[0]
        from rayzath_amd.scene import flatten
        other = flatten(again)
        assert all(getattr(flat, k).tobytes() == getattr(other, k).tobytes() for k in flat.FIELDS), name


def test_new_scenes_hold_what_they_are_named_for(built):
    """the cases NEW makes certain, read from the oracle's records"""
    def rec(name, mode=0):
        r = GS.records(name, mode)
        return r[r["instance"] != _abi.GUIDE_MISS]
    for name in ("normal_map_a", "normal_map_b", "normal_map_c"):
        flat, r = GS.flat_scene(name)[0], rec(name)
        scale = np.abs(flat.instances["scale"])
        assert (flat.instances["scale"] < 0).any(-1).all() and (scale.max(-1) > 8 * scale.min(-1)).all(), name
        assert min((r["external"] == 0).sum(), (r["external"] == 1).sum()) >= 100, name
    r = rec("inside_sphere")
    assert len(r) == 33 * 33 and (r["external"] == 0).all()
    r = rec("emission_maps")
    assert min((r["emission"] > 0).sum(), (r["emission"] == 0).sum()) >= 100
    assert (GS.records("emission_maps", 8)["emission"] != GS.records("emission_maps", 0)["emission"]).sum() >= 100     # map x emission
    r = rec("no_texcrds")
    assert len(r) >= 500 and (r["u"] == 0).all() and (r["v"] == 0).all()
    r, flat = rec("slots"), GS.flat_scene("slots")[0]
    ids = flat.tris["material_flags"][r["triangle"]] & _abi.TRI_MATERIAL_MASK
    for beyond in (70, 200):
        at = ids == beyond
        assert at.sum() >= 60 and (r["material_slot"][at] == 63).all()
        assert (r["material"][at] >= 0).sum() >= 20 and (r["material"][at] < 0).sum() >= 20      # slot 63 set on one instance only
    assert ((r["material"] < 0) & (ids < 3)).sum() >= 20                                          # an unset slot below the count


def test_oracle_against_itself_is_exact_and_the_two_entry_points_agree(built):
    for key in GS.SCENES:
        flat, cam = GS.flat_scene(key)[:2]
        for mode in GS.MODES:
            ref = GS.records(key, mode)
            again = oracle.first_hits(flat, cam, mode, threads=4)
            assert again.tobytes() == ref.tobytes(), (key, mode)
            r = GS.compare(again, ref)
            assert r["exact"] == r["pixels"] == cam.width * cam.height and bad(r) == 0, (key, mode)
            assert GS.misses_read_as_specified(oracle.guides(ref)), (key, mode)
        for y in range(0, cam.height, 7):
            for x in range(0, cam.width, 5):
                assert oracle.first_hit(flat, cam, x, y, 31).tobytes() == GS.records(key, 31)[y, x].tobytes(), (key, x, y)


def test_the_comparison_names_each_kind_of_difference(built):
    ref = oracle.guides(GS.records("address_modes_a", 16))
    hits = np.argwhere(ref["instance"] != _abi.GUIDE_MISS)
    misses = np.argwhere(ref["instance"] == _abi.GUIDE_MISS)

    def changed(field, at, value):
        got = ref.copy()
        got[field][tuple(at)] = value(got[field][tuple(at)])
        r = GS.compare(got, ref)
        return r["discrete"], r["far"], r["pixels"] - r["exact"]

    assert changed("depth", hits[0], lambda v: np.nextafter(v, np.float32(0))) == (1, 0, 1)
    assert changed("instance", hits[1], lambda v: v + 1) == (1, 0, 1)
    assert changed("instance", misses[0], lambda v: 0) == (1, 0, 1)
    assert changed("albedo", hits[2], lambda v: v + np.float32(2e-4)) == (0, 1, 1)
    assert changed("albedo", hits[2], lambda v: np.nextafter(v, np.float32(2))) == (0, 0, 1)          # close: not exact, not far
    assert changed("normal", hits[3], lambda v: -v) == (0, 1, 1)
    assert changed("normal", hits[3], lambda v: v * np.float32(np.nan)) == (0, 1, 1)
    got = ref.copy()
    got["albedo"][tuple(misses[0])] = 0.999
    assert not GS.misses_read_as_specified(got) and GS.misses_read_as_specified(ref)


@pytest.mark.parametrize("mode", GS.MODES)
def test_every_standin_stays_under_its_own_cap(built, mode):
    """the one-ulp libm stand-ins against the plain oracle: no libm call precedes a first hit's record, so every count is 0, a scene's cap 2
    and the sweep's one pixel per 100 000"""
    totals, pixels = {name: 0 for name in lockstep.STANDINS}, 0
    for key in GS.SCENES:
        counts, cap = GS.standin_counts(key, mode), GS.scene_cap(key, mode)
        pixels += counts["lo"]["pixels"]
        for name, r in counts.items():
            totals[name] += bad(r)
            assert bad(r) <= cap, (key, mode, name, r)
    cap = GS.sweep_cap(GS.SCENES, mode)
    print(f"mode {mode}: {pixels} pixels, stand-in totals {totals}, scene caps {sorted({GS.scene_cap(k, mode) for k in GS.SCENES})}, sweep cap {cap}")
    assert max(totals.values()) <= cap
    assert cap == pixels // 100000 >= 1 and all(GS.scene_cap(k, mode) == 2 for k in GS.SCENES)


def test_records_agree_with_the_pick_the_ray_cast_and_the_first_pass(built):
    """on every pixel of every scene: the record's instance and material are rzo_pick's, its slot and triangle rzo_ray_cast's, and in mode
    0 its depth is the first pass's depth buffer bit for bit.  One exception, and it is the reference's: where the first hit is a miss the
    depth is the camera's far plane, and the ray cast's shell of 0.99 .. 1.01 x that depth reaches BEYOND the far plane — on the generated
    scenes whose range clips the geometry it meets what the first pass could not see.  Such pixels are counted; they may occur only where
    the far plane is nearer than the default 1000 and must still agree between rzo_pick and rzo_ray_cast.
    A second one: a degenerate triangle (generated_scenes._irregular_mesh) passes the triangle test with an arbitrary distance, far from
    its own box; the shell's near end culls that box, and the ray cast then meets the triangle behind it (on the sweep: always of the same
    instance, sometimes with another material).  Counted as well, allowed only on scenes that hold such a mesh and on less than 1e-3 of
    the pixels."""
    beyond, behind = {}, {}
    for key in GS.SCENES:
        flat, cam, cfg = GS.flat_scene(key)[:3]
        ref = oracle.OracleRenderer(flat, cam, cfg)
        ref.render(1, threads=4)
        rec = GS.records(key, 0)
        assert np.array_equal(rec["depth"].view(np.uint32), ref.depth.view(np.uint32)), key
        degenerate = any(i.mesh.name == "irregular" for i in GS.flat_scene(key)[3].instances)
        for y in range(cam.height):
            for x in range(cam.width):
                r = rec[y, x]
                pick, cast = ref.pick(x, y), ref.ray_cast(x, y)
                assert (cast[0], cast[2]) == pick, (key, x, y)
                if r["instance"] == _abi.GUIDE_MISS:
                    assert r["depth"] == cam.near_far[1], (key, x, y)
                    if pick != (-1, -1):
                        assert cam.near_far[1] < 1e3, (key, x, y, pick)
                        beyond[key] = beyond.get(key, 0) + 1
                    else:
                        assert cast == (-1, -1, -1, 0), (key, x, y)
                    continue
                if cast != (int(r["instance"]), int(r["material_slot"]), int(r["material"]), int(r["source_index"])):
                    assert degenerate, (key, x, y, cast, r)
                    behind[key] = behind.get(key, 0) + 1
        ref.close()
        for mode in GS.MODES[1:]:     # the geometric first hit does not depend on the mode
            other = GS.records(key, mode)
            assert all(np.array_equal(other[f], rec[f]) for f in ("depth", "instance", "triangle", "material", "external")), (key, mode)
    print(f"missed pixels whose ray cast meets geometry beyond a clipping far plane: {beyond}")
    print(f"pixels whose ray cast meets another triangle than the first hit (degenerate triangles): {behind}")
    assert sum(behind.values()) <= 1e-3 * sum(GS.records(k, 0).size for k in GS.SCENES)


def test_coverage_floors(built):
    """each kind of first hit on at least 20 pixels of at least 3 scenes"""
    table = {key: GS.coverage(key) for key in GS.SCENES}
    older = [k for k in GS.SCENES if k not in GS.NEW]
    print(f"{sum(table[k]['hit'] for k in older)} hit pixels on the {len(older)} older scenes, {sum(table[k]['hit'] for k in GS.NEW)} on the {len(GS.NEW)} new ones")
    short = {}
    for kind in GS.KINDS:
        scenes = [k for k in GS.SCENES if table[k][kind] >= GS.FLOOR[0]]
        print(f"  {kind:45s} {sum(table[k][kind] for k in GS.SCENES):6d} pixels, {len(scenes):3d} scenes with >= {GS.FLOOR[0]} ({len([k for k in scenes if k in GS.NEW])} new)")
        if len(scenes) < GS.FLOOR[1]:
            short[kind] = scenes
    assert not short


def _flagged(mutant, mode):
    """(scenes on which the mutant in the device's place exceeds the scene's cap, its discrete + far total)"""
    flagged, total = [], 0
    for key in GS.SCENES:
        r = GS.compare(GS.records(key, mode, "mut_" + mutant), GS.records(key, mode), records_kept=0)
        total += bad(r)
        if bad(r) > GS.scene_cap(key, mode):
            flagged.append(key)
    return flagged, total


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_rule_flags_every_guide_mutant_where_it_lives_and_nowhere_else(built, mutant):
    for mode in GS.MODES:
        flagged, total = _flagged(mutant, mode)
        lives = mode in MUTANTS[mutant]
        print(f"mutant {mutant} mode {mode}: {'lives' if lives else 'flag off'}, flagged on {len(flagged)} scenes {flagged[:10]}, "
              f"{total} discrete + far pixels (sweep cap {GS.sweep_cap(GS.SCENES, mode)})")
        if lives:
            assert len(flagged) >= 3, (mutant, mode, flagged)
            assert total > GS.sweep_cap(GS.SCENES, mode)
        else:
            assert total == 0, (mutant, mode, total)


def test_which_older_mutants_show_through_the_guides(built):
    """reported, not required: slot_wrap, slot_last and abs_scale (oracle/Makefile) seen through the first-hit records"""
    for mutant in OLDER_MUTANTS:
        for mode in (0, 31):
            flagged, total = _flagged(mutant, mode)
            print(f"mutant {mutant} mode {mode}: flagged on {len(flagged)} scenes {flagged[:10]}, {total} discrete + far pixels")
